"""A fixed list of seeded calls, once each, at the smallest sizes on either side of the launch-routing thresholds: the check that a
host-only routing change launches the same kernels and computes the same bits.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/probe_launch_routes.py OUT.npz

Run it in a fresh process per tree (copy this file into the other tree's tools/), compare the two traces with
tools/compare_kernel_trace.py and the two OUT.npz with `--compare A.npz B.npz` (numpy.array_equal on every pair; exit 1 on a difference).
Every network call runs on variants 1, 5, 6 and 7.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(B.files)) if k not in A.files or k not in B.files or not np.array_equal(A[k], B[k], equal_nan=True)]
    print(f"{len(A.files)} arrays in {a}, {len(B.files)} in {b}: {len(bad)} differ" + (": " + ", ".join(bad[:20]) if bad else ""))
    sys.exit(1 if bad else 0)


def main(out_path):
    import contextlib
    import io

    import torch
    import weights
    from macarons_amd import _lib, ops
    from macarons_amd.networks import SconeOcc, SconeVis
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    out = {}

    def keep(name, t):
        torch.cuda.synchronize()
        out[name] = t.detach().cpu().numpy()

    def attempt(name, fn):
        """keep(name, fn()); a call the library refuses before it launches anything (an argument check, an unsupported combination) is
        recorded as such -- the other tree must refuse it too; anything else ends the probe"""
        try:
            keep(name, fn())
        except Exception as e:
            if not isinstance(e, NotImplementedError) and "(rc=1)" not in str(e):
                raise
            print(f"{name}: refused: {e}")
            out[name + ".refused"] = np.zeros(1, np.int8)

    def cube(*shape):
        return torch.from_numpy(rng.uniform(-.5, .5, shape).astype(np.float32)).to(dev)

    def normal(*shape, scale=.3):
        return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dev)

    with contextlib.redirect_stdout(io.StringIO()):
        occ, vis = SconeOcc(), SconeVis()
    sdo = weights.make_state_dict(weights.shapes_of(occ), 2)
    sdv = weights.make_state_dict(weights.shapes_of(vis), 1)
    sdo["linear3.bias"] = sdo["linear3.bias"] + np.float32(0.5)
    occ.load_state_dict({k: torch.from_numpy(v) for k, v in sdo.items()})
    vis.load_state_dict({k: torch.from_numpy(v) for k, v in sdv.items()})
    occ, vis = occ.to(dev).eval(), vis.to(dev).eval()

    # ---- building blocks (no variant argument) ----
    Xq, pcs = cube(1, 1000, 3), cube(1, 300, 3)
    for k in (1, 4, 8, 16):                                 # M = 300 is below the grid search's range: mcr_knn_points
        pts, dists, idx = ops.knn_points(Xq, pcs, k, subtract_query=True)
        keep(f"knn{k}.pts", pts); keep(f"knn{k}.dists", dists); keep(f"knn{k}.idx", idx)
    for M in (4096, 4160):                                  # either side of the 4096-row one-shot threshold of the planes GEMM
        for K in (256, 1344):
            x, w, b = normal(M, K, scale=1.), normal(512, K, scale=K ** -.5), normal(512, scale=1.)
            keep(f"linear.{M}x{K}", ops.linear(x, w, b, gelu=True))

    for v in (1, 5, 6, 7):
        with ops.variant(v), torch.no_grad():
            # ---- SconeVis / PCTransformer: 1 x 2048 and 8 x 2048 tokens (8 sequences cross the 512-block threshold of the 128-query
            # attention blocks and the 64-row-block threshold of the XCD order), per-sequence lengths, 256 tokens (below the planes route)
            for S, L in ((1, 2048), (8, 2048), (1, 256)):
                rs = np.random.default_rng(100 + S + L)
                p = torch.from_numpy(rs.uniform(0, 1, (S, L, 4)).astype(np.float32)).to(dev)
                vh = torch.from_numpy((rs.standard_normal((S, L, 64)) * .3).astype(np.float32)).to(dev)
                pc = torch.from_numpy(rs.uniform(-.5, .5, (S, L, 3)).astype(np.float32)).to(dev)
                keep(f"v{v}.vis.{S}x{L}", vis(p, view_harmonics=vh))
                keep(f"v{v}.pct.{S}x{L}", occ.global_transformer(pc))
                if S == 8:
                    lens = torch.tensor([2048, 1500, 512, 2048, 700, 2047, 16, 1024], dtype=torch.int32, device=dev)
                    keep(f"v{v}.vis.lengths", vis(p, view_harmonics=vh, lengths=lens))
            # ---- dense SconeOcc through the ABI wrapper, with scale sizes (2048, 512, 64): one scale inside the grid search's range, two
            # outside; single call and phases 1 + 2; B = 1 and the batched local path at B = 2
            for B, Q in ((1, 4096), (2, 2048)):
                rs = np.random.default_rng(200 + B)
                mk = lambda *s: torch.from_numpy(rs.uniform(-.5, .5, s).astype(np.float32)).to(dev)
                scales = [mk(B, 2048, 3), mk(B, 512, 3), mk(B, 64, 3)]
                pg, x = mk(B, 2048, 3), mk(B, Q, 3)
                vh = torch.from_numpy((rs.standard_normal((B, Q, 64)) * .3).astype(np.float32)).to(dev)
                table, blobs, head = occ._images(v)
                keep(f"v{v}.occ.{B}x{Q}.single", ops.scone_occ_forward(pg, scales, x, vh, table, blobs, head, None, phase=0))
                ops.scone_occ_forward(None, [scales[0], None, None], x, None, table, blobs, head, None, phase=1, M_scale=[2048, 512, 64], Lg=2048)
                keep(f"v{v}.occ.{B}x{Q}.phases", ops.scone_occ_forward(pg, scales, x, vh, table, blobs, head, None, phase=2))
            # ---- the layer-by-layer local path
            occ.fused_local = False
            rs = np.random.default_rng(300)
            mk = lambda *s: torch.from_numpy(rs.uniform(-.5, .5, s).astype(np.float32)).to(dev)
            scales, pg, x = [mk(1, 2048, 3), mk(1, 512, 3), mk(1, 64, 3)], mk(1, 2048, 3), mk(1, 256, 3)
            vh = torch.from_numpy((rs.standard_normal((1, 256, 64)) * .3).astype(np.float32)).to(dev)
            table, blobs, head = occ._images(v)
            attempt(f"v{v}.occ.layer_by_layer", lambda: ops.scone_occ_forward(pg, scales, x, vh, table, blobs, head, None, phase=0))
            occ.fused_local = True
            # ---- ragged SconeOcc, 5 jobs: few query blocks (the segmented search splits the candidates) and more than 1536 of them (it
            # does not); two phases (forward_ragged) and the single call on the same tables and draws
            for tag, nq in (("split", 300), ("unsplit", 39500)):
                rs = np.random.default_rng(400 + nq)
                cloud_sizes, query_sizes = [1000, 3000, 1500, 2500, 5000], [nq + 7 * j for j in range(5)]
                pc = torch.from_numpy(rs.uniform(-.5, .5, (sum(cloud_sizes), 3)).astype(np.float32)).to(dev)
                x = torch.from_numpy(rs.uniform(-.5, .5, (sum(query_sizes), 3)).astype(np.float32)).to(dev)
                vh = torch.from_numpy((rs.standard_normal((sum(query_sizes), 64)) * .3).astype(np.float32)).to(dev)
                torch.manual_seed(5)
                perms = [occ.draw_perms(m) for m in cloud_sizes]
                occ.range_guard = "off"                     # (one launch sequence per call: no re-run on variant 5)
                h = occ.forward_ragged_begin(pc, cloud_sizes, x, vh, query_sizes)
                keep(f"v{v}.ragged.{tag}.phases", occ.forward_ragged_finish(h, perms=perms))
                ia, J = occ.last_ragged_perms, len(cloud_sizes)
                pc1 = pc[ia["idx1"]]
                local_blobs, head, table = h["state"][v]
                keep(f"v{v}.ragged.{tag}.single",
                     ops.scone_occ_forward_ragged(pc[ia["g_idx"]].view(J, occ.seq_len, 3), ia["g_len"], [pc, pc1, pc1[ia["idx2"]]],
                                                  [h["d_off0"], ia["off1"], ia["off2"]], x, vh, h["d_row_job"], h["d_blocks"], table, local_blobs,
                                                  head, None, phase=0))
                occ.range_guard = "sync"
        with ops.variant(v):                                # ---- SconeVis backward at 1 x 2048
            rs = np.random.default_rng(500)
            p = torch.from_numpy(rs.uniform(0, 1, (1, 2048, 4)).astype(np.float32)).to(dev).requires_grad_(True)
            vh = torch.from_numpy((rs.standard_normal((1, 2048, 64)) * .3).astype(np.float32)).to(dev).requires_grad_(True)
            g = torch.from_numpy(rs.standard_normal((1, 2048, 64)).astype(np.float32)).to(dev)
            vis.zero_grad()

            def backward():
                vis(p, view_harmonics=vh).backward(g)
                return p.grad
            attempt(f"v{v}.vis.bwd.d_pts", backward)
            if p.grad is not None:
                keep(f"v{v}.vis.bwd.d_vh", vh.grad)
                for n, q in vis.named_parameters():
                    if q.grad is not None:
                        keep(f"v{v}.vis.bwd.{n}", q.grad)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **out)
    print(f"probe_launch_routes: {len(out)} arrays -> {out_path}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    main(sys.argv[1])
