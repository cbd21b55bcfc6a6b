#!/usr/bin/env python3
"""Golden of the occupancy supervision pass: the REFERENCE's compute_occupancy_probability_for_supervision
(macarons/utility/macarons_utils.py:1233-1392) on its own Scene / Cell objects (build container only).

    python tests/golden/make_golden_supervision.py        ->  tests/golden/occ_supervision.npz

The scene is gen_occ_field's (make_golden.py): a 2 x 1 x 2 grid, an ellipsoid shell of surface points through all four cells, 3001
proxy points (not a multiple of 32) on the 2^-6 grid.  Three cases in the one file:
  a  cap 3, four candidate cells: the walk breaks, no dummy pass;
  b  cap 6: the four cells run, two dummy passes advance the generator;
  c  an empty proxy_mask: no pass runs, the first k+1 points and zeros come back.
The proxy points are redrawn until no supervised query of cases a and b has a k / k+1 neighbour tie in any of its three clouds under
the draws the function makes (asserted to be zero): the condition under which the reference itself stays inside the 1e-4 contract.
Only data is written: inputs, the returned mask and probabilities, the size of every torch.randperm call in order, the two host draws,
the cells that ran and their query lists."""
import importlib
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _ref_macarons, _scene_cams, _StandInCameras, _grid, _boundary_ties, save, t  # noqa: E402
import torch  # noqa: E402

K = 16
N_SUP = 1200
CASES = (("a", 3, 6101, False), ("b", 6, 6102, False), ("c", 2, 6103, True))     # tag, cap, seed, empty mask


def main():
    mu = importlib.import_module("macarons.utility.macarons_utils")
    m = _ref_macarons()
    rng = np.random.default_rng(331)
    G = 64.0
    x_min, x_max = torch.tensor([-8., -4., -8.]), torch.tensor([8., 4., 8.])
    grid = (2, 1, 2)
    n_proxy = 3001
    assert n_proxy % 32

    def new_scene(capacity, resolution, feature_dim):
        return mu.Scene(x_min=x_min, x_max=x_max, grid_l=grid[0], grid_w=grid[1], grid_h=grid[2], cell_capacity=capacity,
                        cell_resolution=resolution, n_proxy_points=n_proxy, device="cpu", feature_dim=feature_dim)
    d = rng.standard_normal((2600, 3))
    surf = np.unique(_grid(d / np.linalg.norm(d, axis=1, keepdims=True) * [5.5, 2.8, 5.0] + 0.05 * rng.standard_normal((2600, 3)), G), axis=0)
    rng.shuffle(surf)
    torch.manual_seed(6000)
    surface_scene = new_scene(500, 0.2, 0)
    surface_scene.fill_cells(t(surf))
    cell_pts = {k: c.cell_pts.numpy().copy() for k, c in surface_scene.cells.items()}
    print("  surface cells:", {k: len(v) for k, v in cell_pts.items()})

    def draw_proxy(n):
        q = _grid(rng.uniform(-1, 1, (n, 3)) * [7.9, 3.9, 7.9], G)
        q[q == 0] = 1.0 / G                       # Cell.fill's box tests are strict: a point ON a cell face belongs to no cell
        return q
    proxy = draw_proxy(n_proxy)
    in_fov = rng.random(n_proxy) < 0.7            # the points registered in the proxy cells
    mask = rng.random(n_proxy) < 0.6              # proxy_mask: overlaps the stores only in part (a sampled point may be stored nowhere)
    vstates = (rng.random((n_proxy, 98)) < 0.1).astype(np.float32)
    Rp, Tp, Pp = _scene_cams(np.array([[6., 9., -14.]], np.float32))
    pred = _StandInCameras(t(Rp), t(Tp), t(Pp), squeeze=True)
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=K,
                prediction_neighborhood_size=3, n_view_state_cameras=98, n_proxy_point_for_occupancy_supervision=N_SUP)

    def build_proxy_scene():
        ps = new_scene(100000, 1e-4, 1)
        ps.initialize_proxy_points()
        ps.proxy_points = t(proxy)
        ps.view_states = t(vstates)
        idx = ps.get_proxy_indices_from_mask(torch.from_numpy(in_fov))
        torch.manual_seed(6001)
        ps.fill_cells(t(proxy)[torch.from_numpy(in_fov)], features=idx.view(-1, 1).float())
        return ps

    def ties(ps, cap, seed):
        """Replay the function's draws (no network) and list the supervised queries with a boundary tie in one of their clouds."""
        torch.manual_seed(seed)
        idx = ps.get_proxy_indices_from_mask(torch.from_numpy(mask))
        idx = idx[torch.randperm(len(idx))[:N_SUP]]
        pm = ps.get_proxy_mask_from_indices(idx)
        cells = ps.get_englobing_cells(ps.proxy_points[pm])
        bad_idx, n_pass = [], 0
        for cell in cells[torch.randperm(len(cells))]:
            if n_pass >= cap:
                break
            pcw = surface_scene.get_pt_cloud_from_cells(surface_scene.get_neighboring_cells(cell), return_features=False).numpy()
            _, ind = ps.get_pt_cloud_from_cells(cell, return_features=True)
            cmask = (ps.get_proxy_mask_from_indices(ind) * pm).numpy()
            Xw, gi = proxy[cmask], np.nonzero(cmask)[0]
            if not (pcw.shape[0] > 4 * K and len(Xw) > 0):
                continue
            M = len(pcw)
            ds = int(np.power(M / (K * 8), 1. / 2)) or 2
            torch.randperm(M)                                  # global down-sample (order of SconeOcc.forward)
            p1 = torch.randperm(M).numpy()[:M // ds]
            p2 = torch.randperm(M // ds).numpy()[:(M // ds) // ds]
            pc1 = pcw[p1]; pc2 = pc1[p2]
            bad = _boundary_ties(Xw, pcw, K, G) | _boundary_ties(Xw, pc1, K, G) | _boundary_ties(Xw, pc2, K, G)
            bad_idx += gi[bad].tolist()
            n_pass += 1
        return bad_idx

    for it in range(60):
        ps = build_proxy_scene()
        assert sum(len(c.cell_pts) for c in ps.cells.values()) == int(in_fov.sum()), "a proxy point was refused by Cell.fill"
        bad_idx = sorted(set(sum((ties(ps, cap, seed) for _, cap, seed, empty in CASES if not empty), [])))
        print(f"  occ_supervision: pass {it}: {len(bad_idx)} supervised points with boundary ties")
        if not bad_idx:
            break
        proxy[bad_idx] = draw_proxy(len(bad_idx))
    else:
        raise RuntimeError("no tie-free proxy set found")
    assert not bad_idx

    out = dict(x_min=x_min.numpy(), x_max=x_max.numpy(), grid=np.array(grid), surface=surf, n_surface_cells=np.int64(len(cell_pts)),
               proxy=proxy, in_fov=np.packbits(in_fov), proxy_mask=np.packbits(mask),
               view_states=np.packbits(vstates.astype(np.uint8), axis=-1), Mpred=pred.Mv.numpy(), k=np.int64(K), n_sup=np.int64(N_SUP),
               proxy_proba=ps.proxy_proba.numpy().copy())
    for i, (k, v) in enumerate(sorted(cell_pts.items())):
        out[f"cellkey_{i}"] = np.array(eval(k))
        out[f"cellpts_{i}"] = v
    for i, (k, c) in enumerate(sorted(ps.cells.items())):
        out[f"pcellkey_{i}"] = np.array(eval(k))
        out[f"pcellidx_{i}"] = c.cell_features.numpy()[:, 0].astype(np.int32)

    real_randperm, real_occ, real_cloud = torch.randperm, mu.compute_occupancy_probability, ps.get_pt_cloud_from_cells
    for tag, cap, seed, empty in CASES:
        perms, ran, last, n_dummy = [], [], [None], [0]

        def cap_perm(n, *a, **kw):
            p_ = real_randperm(n, *a, **kw); perms.append(p_.numpy().copy()); return p_

        def cloud(cell, return_features=True):
            res = real_cloud(cell, return_features=return_features)
            last[0] = (cell.numpy().copy(), res[1].numpy().copy())
            return res

        def occ(*a, **kw):
            if last[0] is None:
                n_dummy[0] += 1
            else:
                ran.append(last[0]); last[0] = None
            return real_occ(*a, **kw)
        pmask = torch.from_numpy(np.zeros_like(mask) if empty else mask)
        proba_before = ps.proxy_proba.clone()
        torch.randperm, mu.compute_occupancy_probability, ps.get_pt_cloud_from_cells = cap_perm, occ, cloud
        try:
            torch.manual_seed(seed)
            with torch.no_grad():
                pm, probas = mu.compute_occupancy_probability_for_supervision(params, m, None, ps, pmask, surface_scene, cap, "cpu",
                                                                               prediction_camera=pred)
        finally:
            torch.randperm, mu.compute_occupancy_probability = real_randperm, real_occ
            del ps.get_pt_cloud_from_cells
        assert torch.equal(ps.proxy_proba, proba_before)
        pm_np = pm.numpy()
        lin = [int((c[0] * grid[1] + c[1]) * grid[2] + c[2]) for c, _ in ran]
        queries = [np.nonzero(ps.get_proxy_mask_from_indices(torch.from_numpy(ind)).numpy() & pm_np)[0].astype(np.int32) for _, ind in ran]
        out.update({f"{tag}_cap": np.int64(cap), f"{tag}_seed": np.int64(seed), f"{tag}_mask_empty": np.bool_(empty),
                    f"{tag}_prediction_mask": np.packbits(pm_np), f"{tag}_probas": probas.numpy(),
                    f"{tag}_perm_sizes": np.array([len(p_) for p_ in perms], np.int64),
                    f"{tag}_sample_perm": perms[0].astype(np.int64), f"{tag}_cell_perm": perms[1].astype(np.int64),
                    f"{tag}_cells_run": np.array(lin, np.int64), f"{tag}_n_dummy": np.int64(n_dummy[0]),
                    f"{tag}_query_off": np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int64),
                    f"{tag}_queries": np.concatenate(queries + [np.zeros(0, np.int32)]).astype(np.int32)})
        print(f"  case {tag}: cap {cap}: cells run {lin}, {n_dummy[0]} dummy passes, {len(perms)} randperm draws, "
              f"{int(pm_np.sum())} points, max |p| {float(probas.abs().max()):.4f}")
    assert len(out["a_cells_run"]) == 3 and int(out["a_n_dummy"]) == 0 and len(out["a_cell_perm"]) == 4
    assert len(out["b_cells_run"]) == 4 and int(out["b_n_dummy"]) == 2
    assert len(out["c_cells_run"]) == 0 and int(out["c_n_dummy"]) == 2 and not out["c_probas"].any()
    save("occ_supervision", **out)


if __name__ == "__main__":
    main()
