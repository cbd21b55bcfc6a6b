"""Does the host layer of the network modules compute, launch and synchronise what another tree's does?  The check of a refactor of
networks/ (range guard, weight tables, handles), nbv._guarded and macarons_nbv_decision that is meant to change no behaviour.

    python tools/compare_with_parent.py TAG [--root TREE] [--out DIR] [--only GROUP,GROUP]     # dump: DIR/TAG/outputs.pt, counts.json
    python tools/compare_with_parent.py DIR_A DIR_B                                            # compare two dumps, exit 1 on a difference

One fresh process per dump; --root is the tree whose package, tests/ helpers and goldens are used (default: this one), so the same
script drives a checkout of the parent commit.  Same seeds and weights in every run (tests/golden/weights.py; the overflow sets of
tests/test_range_guard_gpu.py).  Tensors are compared byte for byte (a NaN equals the same NaN), everything else with ==.
Groups: occ (SconeOcc.forward, forward_begin + forward(begun=)), ragged (forward_ragged: given draws, index_arrays re-use, native
draws, differentiable), vis (SconeVis.forward), nbv (nbv_step, nbv_step_batch), macarons (macarons_nbv_decision).  The decisions
also count, for one warm call each, the fingerprint walks (packing._param_key) and the host synchronisations
(torch.cuda.set_sync_debug_mode) -> counts.json.  For the kernel sequence run a dump of one group under
`rocprofv3 --kernel-trace --output-format csv -- python tools/compare_with_parent.py ...` in both trees and hand the two traces to
tools/compare_kernel_trace.py.

A one-off checking tool, not part of the product: it builds its scenes with helpers of the test suite (tests/conftest.py: golden;
tests/test_macarons_regime_gpu.py: _decision_scenes, _models; tests/golden/weights.py) and has to follow them if they move."""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import warnings

import numpy as np
import torch

GROUPS = ("occ", "ragged", "vis", "nbv", "macarons")
OVERFLOW = {"occ_head": (["linear1", "x_embedding.linear2"], 2.0 ** 16), "vis_encoder": (["encoders.1.ff.linear1"], 2.0 ** 17)}


def put(store, name, v):
    if torch.is_tensor(v):
        store[name] = v.detach().cpu().clone()
    elif isinstance(v, dict):
        for k in v:
            put(store, f"{name}.{k}", v[k])
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            put(store, f"{name}.{i}", x)
    else:
        store[name] = v


def same(a, b):
    if torch.is_tensor(a) != torch.is_tensor(b):
        return False
    if not torch.is_tensor(a):
        return a == b
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def compare(dir_a, dir_b):
    A, B = (torch.load(os.path.join(d, "outputs.pt"), weights_only=False) for d in (dir_a, dir_b))
    bad = sorted(set(A) ^ set(B)) + [k for k in A if k in B and not same(A[k], B[k])]
    with open(os.path.join(dir_a, "counts.json")) as fa, open(os.path.join(dir_b, "counts.json")) as fb:
        ca, cb = json.load(fa), json.load(fb)
    print(f"{len(A)} | {len(B)} entries; counts A {ca}; counts B {cb}")
    if bad or ca != cb:
        print(f"DIFFERENT: {len(bad)} entries {bad[:20]}" + ("; counts differ" if ca != cb else ""))
        sys.exit(1)
    print("same bytes in every entry, same counts")


class Counted:
    """Fingerprint walks and host synchronisations of the calls made inside `with counted(name):`."""

    def __init__(self):
        self.counts, self._walks = {}, [0]
        packing = importlib.import_module("macarons_amd.networks.packing")
        real = packing._param_key

        def walk(module, cache):
            self._walks[0] += 1
            return real(module, cache)
        for mod in ("packing", "SconeOcc", "SconeVis"):             # (wherever the name is bound)
            m = importlib.import_module("macarons_amd.networks." + mod)
            if getattr(m, "_param_key", None) is real:
                m._param_key = walk

    @contextlib.contextmanager
    def __call__(self, name):
        w0 = self._walks[0]
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode(1)
            try:
                yield
            finally:
                torch.cuda.set_sync_debug_mode(0)
        self.counts[name] = {"param_key_walks": self._walks[0] - w0, "syncs": sum("synchroniz" in str(w.message) for w in seen)}


def run(tag, root, out_dir, groups):
    sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")]
    import weights
    from conftest import golden
    from macarons_amd import networks, ops
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    store, counted = {}, Counted()

    def model(net, seed, overflow=None, bias=0.0):
        with contextlib.redirect_stdout(io.StringIO()):
            m = getattr(networks, net)()
        sd = weights.make_state_dict(weights.shapes_of(m), seed)
        if bias:
            sd["linear3.bias"] = sd["linear3.bias"] + np.float32(bias)
        if overflow:
            for layer in OVERFLOW[overflow][0]:
                for k in (layer + ".weight", layer + ".bias"):
                    sd[k] = (sd[k] * np.float32(OVERFLOW[overflow][1])).astype(np.float32)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        return m.to(dev).eval()

    def guard_state(m):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            full = m.check_range(wait=True)
        flag = m.range_flag()
        return {"flag": None if flag is None else int(flag), "full_range": bool(full), "guard": m.range_guard}

    g_occ = golden("scone_occ")

    def occ_case(tag_):
        return (T(g_occ[f"{tag_}_pc"]), T(g_occ[f"{tag_}_x"]), T(g_occ[f"{tag_}_vh"]),
                [torch.from_numpy(g_occ[f"{tag_}_perm{i}"].astype(np.int64)) for i in range(3)])

    if "occ" in groups:
        for weights_ in (None, "occ_head"):
            for v in (5, 6, 7):
                for guard in ("sync", "defer", "async", "off"):
                    if weights_ and (v != 6 or guard == "off"):
                        continue
                    for case in ("m1024_q300", "m4096_q512"):
                        pc, x, vh, perms = occ_case(case)
                        for begun in (False, True):
                            m = model("SconeOcc", 2, weights_)
                            m.range_guard = guard
                            with torch.no_grad(), ops.variant(v), warnings.catch_warnings():
                                warnings.simplefilter("ignore")
                                h = m.forward_begin(pc, x) if begun else None
                                y = [m(pc, x, vh, perms=perms, begun=h)]
                                m.check_range(wait=True)                    # ("async": the copy has landed, whatever the timing)
                                y.append(m(pc, x, vh, perms=perms))         # (under "async" after an overflow: the re-entry on variant 5)
                            put(store, f"occ.{weights_}.v{v}.{guard}.{case}.begun{int(begun)}", {"y": y, "state": guard_state(m)})

    if "ragged" in groups:
        rs = np.random.default_rng(21)
        cloud_sizes, query_sizes = [1024, 700, 3000], [300, 150, 77]
        pc = T(rs.uniform(-.5, .5, (sum(cloud_sizes), 3)).astype(np.float32))
        x = T(rs.uniform(-.5, .5, (sum(query_sizes), 3)).astype(np.float32))
        vh = T((rs.standard_normal((sum(query_sizes), 64)) * .3).astype(np.float32))
        for weights_ in (None, "occ_head"):
            for v in (5, 6, 7):
                for guard in ("sync", "defer", "async", "off"):
                    if weights_ and (v != 6 or guard == "off"):
                        continue
                    m = model("SconeOcc", 2, weights_)
                    m.range_guard = guard
                    torch.manual_seed(31)
                    perms = [m.draw_perms(n) for n in cloud_sizes]
                    res = {}
                    with torch.no_grad(), ops.variant(v):
                        res["given"] = m.forward_ragged(pc, cloud_sizes, x, vh, query_sizes, perms=perms).clone()
                        res["index_arrays"] = dict(m.last_ragged_perms)
                        res["reused"] = m.forward_ragged(pc, cloud_sizes, x, vh, query_sizes, index_arrays=m.last_ragged_perms).clone()
                        torch.manual_seed(31)
                        res["drawn"] = m.forward_ragged(pc, cloud_sizes, x, vh, query_sizes).clone()
                        res["drawn_arrays"] = dict(m.last_ragged_perms)
                        res["generator"] = torch.get_rng_state()
                        out = torch.full((sum(query_sizes), 1), -1.0, device=dev)
                        h = m.forward_ragged_begin(pc, cloud_sizes, x, vh, query_sizes)
                        res["two_halves_out"] = m.forward_ragged_finish(h, perms=perms, out=out).clone()
                    put(store, f"ragged.{weights_}.v{v}.{guard}", {"res": res, "state": guard_state(m)})
        m = model("SconeOcc", 2)
        torch.manual_seed(31)
        perms = [m.draw_perms(n) for n in cloud_sizes]
        xg, vg = x.clone().requires_grad_(True), vh.clone().requires_grad_(True)
        y = m.forward_ragged(pc, cloud_sizes, xg, vg, query_sizes, perms=perms, differentiable=True)
        y.backward(T(rs.standard_normal(tuple(y.shape)).astype(np.float32)))
        put(store, "ragged.differentiable", {"y": y, "x.grad": xg.grad, "vh.grad": vg.grad,
                                              "grads": {n: p.grad for n, p in m.named_parameters()}})

    if "vis" in groups:
        for weights_ in (None, "vis_encoder"):
            for v in (5, 6, 7):
                for guard in ("sync", "defer", "async", "off"):
                    if weights_ and (v != 6 or guard == "off"):
                        continue
                    for N in (700, 300):
                        rs = np.random.default_rng(3)
                        pts = T(np.concatenate([rs.uniform(-.5, .5, (2, N, 3)), rs.uniform(.1, 1., (2, N, 1))], -1).astype(np.float32))
                        vhs = T((rs.standard_normal((2, N, 64)) * 0.3).astype(np.float32))
                        for lengths in (None, torch.tensor([N - 37, N], dtype=torch.int32, device=dev)):
                            m = model("SconeVis", 1, weights_)
                            m.range_guard = guard
                            with torch.no_grad(), ops.variant(v), warnings.catch_warnings():
                                warnings.simplefilter("ignore")
                                y = [m(pts, view_harmonics=vhs, lengths=lengths)]
                                m.check_range(wait=True)
                                y.append(m(pts, view_harmonics=vhs, lengths=lengths))
                            put(store, f"vis.{weights_}.v{v}.{guard}.n{N}.len{int(lengths is not None)}", {"y": y, "state": guard_state(m)})

    if "nbv" in groups:
        from macarons_amd.nbv import ViewStateGrid, draw_batch, nbv_step, nbv_step_batch
        g = golden("e2e_grid_config1")
        pc, X, X_view, X_cam, grid = T(g["pc"]), T(g["X"]), T(g["X_view"]), T(g["X_cam"]), ViewStateGrid(dev)
        perms, u = [torch.from_numpy(g[f"perm{i}"].astype(np.int64)) for i in range(3)], T(g["samples"].astype(np.float32))
        for where in (None, "occ_head", "vis_encoder"):
            occ = model("SconeOcc", 2, where if where == "occ_head" else None, bias=0.5)
            vis = model("SconeVis", 1, where if where == "vis_encoder" else None)
            for rg in (True, False):
                nbv_step(occ, vis, pc, X, X_view, X_cam, grid, occ_perms=perms, samples=u, range_guard=rg)        # (warm: the images exist)
                with counted(f"nbv_step.{where}.guard{int(rg)}"):
                    r = nbv_step(occ, vis, pc, X, X_view, X_cam, grid, occ_perms=perms, samples=u, range_guard=rg)
                put(store, f"nbv_step.{where}.guard{int(rg)}", {"out": r, "occ": guard_state(occ), "vis": guard_state(vis)})
            torch.manual_seed(41)                                    # the step pins its own draws
            r = nbv_step(occ, vis, pc, X, X_view, X_cam, grid)
            put(store, f"nbv_step.{where}.drawn", {"out": r, "generator": torch.get_rng_state()})
            B = 3
            pcb, Xb = torch.cat([pc, pc * 0.9, pc.flip(1)]).contiguous(), X.expand(B, -1, -1).contiguous()
            torch.manual_seed(7)
            bp, bu = draw_batch(occ, B, pc.shape[1], 2048, dev)
            with counted(f"nbv_step_batch.{where}"):
                r = nbv_step_batch(occ, vis, pcb, Xb, X_view, X_cam, grid, occ_perms=bp, samples=bu)
            put(store, f"nbv_step_batch.{where}", {"out": r, "occ": guard_state(occ), "vis": guard_state(vis)})

    if "macarons" in groups:
        from types import SimpleNamespace as NS
        from macarons_amd.utility import macarons_utils as mu
        with contextlib.redirect_stdout(io.StringIO()):
            from test_macarons_regime_gpu import _decision_scenes, _models
        g = golden("macarons_decision")
        H, W = int(g["hw"][0]), int(g["hw"][1])
        params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=16,
                    prediction_neighborhood_size=3, n_view_state_cameras=98, sensor_range=40., min_occ_for_proxy_points=0.1, seq_len=2048,
                    distance_factor_th=17., image_height=H, image_width=W, carving_tolerance=0.05)
        dmask = np.unpackbits(g["dmask"])[:2 * H * W].reshape(2, H, W).astype(bool)
        for where in (None, "occ_head", "vis_encoder"):
            for rg in (True, False):
                with contextlib.redirect_stdout(io.StringIO()):
                    m = _models(dev)
                with torch.no_grad():
                    for layer in (OVERFLOW[where][0] if where else ()):
                        lin = (m.occupancy if where == "occ_head" else m.visibility).get_submodule(layer)
                        lin.weight.mul_(OVERFLOW[where][1]); lin.bias.mul_(OVERFLOW[where][1])
                surface, proxy = _decision_scenes(g, dev)
                for c in range(2):                                  # two consecutive decisions; the second one is counted (warm)
                    cam = mu.SceneCamera(mu.camera_record(g["Mview"][c], g["Mfull"][c], g["ndc"], g["eyes"][c], params.sensor_range).to(dev),
                                         T(g["eyes"][c:c + 1]), float(g["zfar"]))
                    nrec = torch.stack([mu.camera_record(g[f"nMview_{c}"][k], g[f"nMfull_{c}"][k], g["ndc"], g["n_eyes"][c, k],
                                                         params.sensor_range) for k in range(5)]).to(dev)
                    args = (params, m, proxy, surface, cam, T(g["depth"][c]), T(dmask[c]), nrec, T(g["n_eyes"][c]), dev)
                    torch.manual_seed(5100 + c)
                    with torch.no_grad(), (counted(f"macarons.{where}.guard{int(rg)}") if c else contextlib.nullcontext()):
                        r = mu.macarons_nbv_decision(*args, samples=T(g[f"u_{c}"]), range_guard=rg)
                    put(store, f"macarons.{where}.guard{int(rg)}.{c}", {"out": r, "proxy_proba": proxy.proxy_proba, "generator": torch.get_rng_state(),
                                                                          "occ": guard_state(m.occupancy), "vis": guard_state(m.visibility)})

    torch.cuda.synchronize()
    os.makedirs(os.path.join(out_dir, tag), exist_ok=True)
    torch.save(store, os.path.join(out_dir, tag, "outputs.pt"))
    with open(os.path.join(out_dir, tag, "counts.json"), "w") as f:
        json.dump(counted.counts, f, indent=1, sort_keys=True)
    print(f"{tag}: {len(store)} entries, counts {json.dumps(counted.counts, sort_keys=True)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", help="TAG (dump) or DIR_A DIR_B (compare)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default="parent_compare")
    ap.add_argument("--only", default=",".join(GROUPS))
    args = ap.parse_args()
    if len(args.what) == 2:
        compare(*args.what)
    else:
        run(args.what[0], os.path.abspath(args.root), args.out, args.only.split(","))


if __name__ == "__main__":
    main()
