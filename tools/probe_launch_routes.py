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

    # ---- the kernels that reduce, scan or decide through csrc/wave.h: scorer record and backward, decision glue, scene store,
    # supervision selection, the grid search's build, the plane sweep's backward -- one seeded call each at the smallest size that
    # reaches every kernel of the entry (more than one wave, a ragged tail, NaN and tied gains for the arg-max)
    rs = np.random.default_rng(600)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    for C in (65, 257):                                     # 257: the stride loop and the four-wave merge of the scorer's record
        p, h = f32(rs.uniform(-.5, .5, (3, 200, 4))), f32(rs.standard_normal((3, 200, 64)) * .5)
        h[1] = 0.                                           # every camera ties
        h[2, 5, 3] = float("nan")                           # NaN gains
        c = rs.standard_normal((3, C, 3))
        c = f32(1.5 * c / np.linalg.norm(c, axis=-1, keepdims=True))
        gains, rec = ops.sh_coverage_gain_best(p, h, c)
        keep(f"wave.scorer.{C}.gains", gains); keep(f"wave.scorer.{C}.record", rec)
        keep(f"wave.best_record.{C}", ops.best_record(gains, 3))
        for n, t in zip(("max", "idx", "record"), ops.nbv_decide(gains.clone(), torch.tensor([4, 0, 2], dtype=torch.int32, device=dev))):
            keep(f"wave.nbv_decide.{C}.{n}", t)
        for n, t in zip(("d_harm", "d_pts", "d_cams"), ops.sh_scorer_backward(p[:1], h[:1], c[:1], f32(rs.standard_normal((1, C))), False, True)):
            keep(f"wave.scorer_bwd.{C}.{n}", t)
    keep("wave.multi_gain", ops.coverage_gain_multiple(p[:1], h[:1], c[:1, :5].contiguous(), 2)[0])
    K, S = 3, 700
    vis_u, world = f32(rs.uniform(0, 1, (K, S))), f32(rs.uniform(-2, 2, (K, S, 4)))
    nu = torch.tensor([S, 0, 300], dtype=torch.int32, device=dev)
    inv = torch.from_numpy(np.stack([rs.integers(0, max(int(n), 1), S) for n in nu.tolist()])).to(dev)
    cam, vol = f32(rs.uniform(-3, 3, (K, 3))), f32(rs.uniform(.5, 2, K))
    Mv = np.tile(np.eye(4), (K, 1, 1)) + rs.standard_normal((K, 4, 4)) * .05
    for smooth in (False, True):
        keep(f"wave.macarons_gain.{smooth}", ops.macarons_gain_(vis_u.clone(), world, cam, vol, 1.5, smooth))
        keep(f"wave.macarons_gain_indexed.{smooth}", ops.macarons_gain_indexed(vis_u, world, inv, nu, cam, vol, 1.5, smooth))
        d_vis, d_vol = ops.macarons_gain_backward(f32(rs.standard_normal(K)), vis_u, world, inv, nu, cam, vol, 1.5, smooth, need_volume=True)
        keep(f"wave.macarons_gain_bwd.{smooth}.d_vis", d_vis); keep(f"wave.macarons_gain_bwd.{smooth}.d_volume", d_vol)
    for n, t in zip(("center", "cam_view"), ops.camera_boxes(world, nu, f32(Mv), cam, 0.25)):
        keep(f"wave.camera_boxes.{n}", t)
    P = 3001
    X, pr = f32(rs.uniform(-.5, .5, (P, 3))), f32(rs.uniform(0, 1, (P, 1)))
    for n, t in zip(("res", "res_h", "inverse", "uniq", "n_unique", "volume"),
                    ops.sample_proxy(X, pr, f32(rs.standard_normal((P, 64))), f32(rs.uniform(0, 1, 500)), 0.25, return_volume=True, padded=True)):
        keep(f"wave.sample_proxy.{n}", t)
    for n, t in zip(("mask", "bounds"), ops.filter_proxy_mask(X, f32(rs.uniform(-.4, .4, (777, 3))), f32(Mv[:2]), 0.05)):
        keep(f"wave.filter_proxy.{n}", t)
    nk = 71
    key = np.repeat(rs.integers(-1, nk + 2, 400), rs.integers(1, 60, 400)).astype(np.int32)      # runs, some values out of range
    key = torch.from_numpy(key).to(dev)
    for n, t in zip(("counts", "offsets"), ops.key_histogram(key, nk)):
        keep(f"wave.key_histogram.{n}", t)
    for n, t in zip(("order", "counts", "offsets"), ops.group_by_key(key, nk)):
        keep(f"wave.group_by_key.{n}", t)
    grid, lo, hi = (2, 1, 2), np.array([-4., -2., -4.]), np.array([4., 2., 4.])
    pp = rs.uniform(-1, 1, (P, 3)) * [3.9, 1.9, 3.9]
    cells = [rs.permutation(P)[:n] for n in (900, 0, 1700, 40)]          # the proxy indices stored in each cell (one cell is empty)
    fts = np.stack((np.concatenate(cells), rs.standard_normal(sum(map(len, cells)))), 1)
    off = np.concatenate(([0], np.cumsum([len(c_) for c_ in cells]))).astype(np.int64)
    sel = ops.supervision_select(torch.from_numpy(rs.random(P) < .4).to(dev), f32(pp), f32(np.concatenate((lo, hi, (hi - lo) / grid))), grid,
                                 f32(fts), int(off[-1]), torch.from_numpy(off).to(dev))
    keep("wave.supervision.counts", sel.counts); keep("wave.supervision.rows_order", sel.rows_order); keep("wave.supervision.pos", sel.pos)
    pts, dists, idx = ops.knn_points(cube(1, 1000, 3), cube(1, 2048, 3), 16, subtract_query=True)       # M = 2048: the grid search
    keep("wave.knn_grid.pts", pts); keep("wave.knn_grid.dists", dists); keep("wave.knn_grid.idx", idx)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _cost_volume_cases as cvc
    from macarons_amd.networks import ManyDepth
    cv = cvc.inputs(*cvc.SHAPES["scan"])
    cams = ManyDepth.pack_cameras(cv["R"], cv["T"], cv["R_alpha"], cv["T_alpha"]).to(dev)
    d_out = torch.randn((cv["x"].shape[0], cv["D"]) + tuple(cv["x"].shape[-2:]), generator=torch.Generator().manual_seed(601)).to(dev)
    for n, t in zip(("d_x", "d_x_alpha"), ops.cost_volume_backward(cv["x"].to(dev), cv["x_alpha"].to(dev), cams, cv["depth_bins"].to(dev), d_out,
                                                                   cv["H"], cv["W"])):
        keep(f"wave.cost_volume_bwd.{n}", t)

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
                table, local_blobs, head = h.images[v]
                keep(f"v{v}.ragged.{tag}.single",
                     ops.scone_occ_forward_ragged(pc[ia["g_idx"]].view(J, occ.seq_len, 3), ia["g_len"], [pc, pc1, pc1[ia["idx2"]]],
                                                  [h.d_off0, ia["off1"], ia["off2"]], x, vh, h.d_row_job, h.d_blocks, table, local_blobs,
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
