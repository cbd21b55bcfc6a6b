"""Time one occupancy-supervision step of the online trainer -- compute_occupancy_probability_for_supervision, mean squared error,
backward() -- on its three routes, with HIP events after warm-up, and count the function's host synchronisations.

    python tools/time_occ_supervision.py [--iters 3] [--repeats 3] [--caps 5,10] [--routes batched,hip,pct] [--out FILE.json]

The scene: a liberty-like grid of 6 x 2 x 6 = 72 cells, 100 000 proxy points of which ~40 % are registered in the proxy cells and
form proxy_mask, a surface shell of ~60 000 points in cells of capacity 1000, n_proxy_point_for_occupancy_supervision = 6000, a cap
of 5 and of 10 cells per call (n_cell_per_occ_forward_pass), golden-seed weights; every parameter requires a gradient.
  batched  macarons_utils.compute_occupancy_probability_for_supervision: one selection, one forward_ragged(differentiable=True) over
           the cells that run, one scatter node, one mcr_scone_occ_backward_ragged
  hip      upstream's loop restated on the repo's Scene methods -- one compute_occupancy_probability call and one graph per cell --
           under MCR_SCONE_OCC_BWD=hip
  pct      the same under MCR_SCONE_OCC_BWD=pct
Every step of every route starts from the same CPU-generator seed, so all three visit the same cells with the same draws.  One
repeat times --iters whole steps of each route back to back, the routes taking turns; the JSON keeps every repeat's mean and the
median / min / max over the repeats.  Host synchronisations: torch.cuda.set_sync_debug_mode(1) around one call of the batched function
(the method of tools/find_syncs_macarons.py), with the call sites."""
import argparse
import collections
import json
import os
import sys
import traceback
import warnings
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import Macarons, SconeOcc  # noqa: E402
from macarons_amd.utility import macarons_utils as mu  # noqa: E402
from macarons_amd.utility.scene import Scene  # noqa: E402
import weights  # noqa: E402

GRID = (6, 2, 6)
N_PROXY, N_SUP, K = 100000, 6000, 16


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters            # ms per step


def build(dev):
    rng = np.random.default_rng(0)
    x_min, x_max = torch.tensor([-60., -20., -60.], device=dev), torch.tensor([60., 20., 60.], device=dev)
    surface = Scene(x_min, x_max, *GRID, cell_capacity=1000, cell_resolution=0.05, n_proxy_points=N_PROXY, device=dev)
    d = rng.standard_normal((80000, 3))
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * [52., 17., 50.] + 1.5 * rng.standard_normal((80000, 3))
    torch.manual_seed(1)
    surface.fill_cells(torch.from_numpy(shell.astype(np.float32)).to(dev))
    proxy = Scene(x_min, x_max, *GRID, cell_capacity=100000, cell_resolution=1e-4, n_proxy_points=N_PROXY, device=dev, feature_dim=1)
    torch.manual_seed(2)
    proxy.initialize_proxy_points()
    mask = torch.from_numpy(rng.random(N_PROXY) < 0.4).to(dev)
    proxy.view_states = torch.from_numpy((rng.random((N_PROXY, 98)) < 0.1).astype(np.float32)).to(dev)
    proxy.fill_cells(proxy.proxy_points[mask], features=proxy.get_proxy_indices_from_mask(mask).view(-1, 1).float())
    occ = SconeOcc()
    sd = weights.make_state_dict(weights.shapes_of(occ), 2)
    sd["linear3.bias"] = sd["linear3.bias"] + np.float32(0.5)
    occ.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    occ = occ.to(dev)
    eye = np.array([70., 40., -90.])
    z = -eye / np.linalg.norm(eye)
    xa = np.cross([0., 1., 0.], z); xa /= np.linalg.norm(xa)
    R = np.stack((xa, np.cross(z, xa), z), 1)                       # world -> view, row-vector convention
    Mv = np.eye(4, dtype=np.float32)
    Mv[:3, :3], Mv[3, :3] = R, -eye @ R
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=K, prediction_neighborhood_size=3,
                n_view_state_cameras=98, n_proxy_point_for_occupancy_supervision=N_SUP)
    return NS(surface=surface, proxy=proxy, mask=mask, occ=occ, m=Macarons(None, occ, None), Mv=torch.from_numpy(Mv), params=params, dev=dev)


def per_cell_loop(s, cap):
    """Upstream's control flow (macarons_utils.py:1233-1392), one network call per cell; the per-cell inputs come from the entries that
    make them one at a time."""
    ps, ss, dev, params = s.proxy, s.surface, s.dev, s.params
    idx = ps.get_proxy_indices_from_mask(s.mask)
    idx = idx[torch.randperm(len(idx))[:params.n_proxy_point_for_occupancy_supervision].to(dev)]
    pm = ps.get_proxy_mask_from_indices(idx)
    probas = torch.zeros_like(ps.proxy_proba)
    cells = ps.get_englobing_cells(ps.proxy_points[pm])
    prep = mu._field_prepare(params, ps, s.Mv, dev)
    perm_d, n_pass = prep["perm_t"].to(dev), 0
    for cell in cells[torch.randperm(len(cells)).to(dev)]:
        if n_pass >= cap:
            break
        pcw = ss.get_pt_cloud_from_cells(ss.get_neighboring_cells(cell), return_features=False)
        _, ind = ps.get_pt_cloud_from_cells(cell, return_features=True)
        cmask = ps.get_proxy_mask_from_indices(ind.reshape(-1).long()) & pm
        rows = torch.nonzero(cmask).reshape(-1)
        if not (pcw.shape[0] > 4 * K and rows.numel() > 0):
            continue
        c = cell.tolist()
        xf = torch.from_numpy(prep["xf_all"][(c[0] * GRID[1] + c[1]) * GRID[2] + c[2]].copy()).to(dev)
        Mv, cen, inv = xf[:16].view(4, 4).contiguous(), xf[16:19].contiguous(), float(xf[19])
        pc = ops.transform_points_(pcw.clone().contiguous(), Mv, cen, inv)
        X = ops.transform_points_(ps.proxy_points[rows].contiguous(), Mv, cen, inv)
        vh = ops.view_harmonics_rows(ps.view_states, rows.to(torch.int32), perm_d, prep["vh_mt"])
        probas[cmask] += mu.compute_occupancy_probability(s.m, pc[None], X[None], vh[None]).view(-1, 1)
        n_pass += 1
    while n_pass < cap:
        d_occ = mu.compute_occupancy_probability(s.m, ps.proxy_points[:4 * K + 1][None], ps.proxy_points[:K + 1][None],
                                                 torch.zeros(1, K + 1, 64, device=dev)).view(-1, 1) * 0.
        if n_pass == 0:
            pm = torch.zeros(N_PROXY, dtype=torch.bool, device=dev)
            pm[:K + 1] = True
            probas[pm] += 0. * d_occ
        n_pass += 1
    return pm, probas[pm]


def count_syncs(fn):
    sites = collections.Counter()

    def showwarning(message, category, filename, lineno, file=None, line=None):
        if "synchroniz" not in str(message):
            return
        st = [f for f in traceback.extract_stack() if "/macarons_amd/" in f.filename]
        if st:                                      # (torch's own notice on switching the mode on has no frame of the package)
            sites[" <- ".join(f"{os.path.basename(f.filename)}:{f.lineno}" for f in reversed(st[-3:]))] += 1
    old = warnings.showwarning
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        warnings.showwarning = showwarning
        torch.cuda.set_sync_debug_mode(1)
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
            warnings.showwarning = old
    return sites


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--caps", default="5,10")
    ap.add_argument("--routes", default="batched,hip,pct")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    routes = a.routes.split(",")
    assert set(routes) <= {"batched", "hip", "pct"}, routes
    dev = torch.device("cuda:0")
    s = build(dev)
    rows_out = []
    for cap in (int(c) for c in a.caps.split(",")):
        state = {"step": 0}

        def step(fn, env):
            def run():
                if env is None:
                    os.environ.pop("MCR_SCONE_OCC_BWD", None)
                else:
                    os.environ["MCR_SCONE_OCC_BWD"] = env
                s.occ.zero_grad(set_to_none=True)
                torch.manual_seed(1000 + state["step"] % a.iters)       # the same seeds for every route and repeat
                state["step"] += 1
                pm, pr = fn()
                ((pr - 0.25) ** 2).mean().backward()
                return pm, pr
            return run
        rec = {}
        batched = lambda: mu.compute_occupancy_probability_for_supervision(s.params, s.m, None, s.proxy, s.mask, s.surface, cap, dev,
                                                                           prediction_camera=s.Mv, record=rec)
        paths = {"batched": step(batched, None), "hip": step(lambda: per_cell_loop(s, cap), "hip"),
                 "pct": step(lambda: per_cell_loop(s, cap), "pct")}
        paths = {k: v for k, v in paths.items() if k in routes}
        runs = {k: [] for k in paths}
        for _ in range(a.repeats):
            for k, fn in paths.items():
                state["step"] = 0
                runs[k].append(timed(fn, a.iters))
        row = {"cap": cap, "grid": list(GRID), "n_proxy": N_PROXY, "n_sup": N_SUP, "iters": a.iters, "repeats": a.repeats}
        for k, v in runs.items():
            row[f"{k}_step_ms"], row[f"{k}_step_min_ms"], row[f"{k}_step_max_ms"] = float(np.median(v)), min(v), max(v)
            row[f"{k}_step_runs_ms"] = v
        if "batched" in paths:
            state["step"] = 0
            pm, pr = paths["batched"]()
            g_b = [q.grad.clone() for q in s.occ.parameters()]
            row.update(cells_run=len(rec["visited"]), jobs=len(rec["cloud_sizes"]), n_dummy=rec["n_dummy"], rows=int(rec["rows"].numel()),
                       cloud_rows=int(sum(rec["cloud_sizes"])), n_pred=int(pr.shape[0]))
            if "hip" in paths:
                state["step"] = 0
                pm_h, pr_h = paths["hip"]()
                row["values_equal_to_per_cell"] = bool(torch.equal(pm, pm_h) and torch.equal(pr.detach(), pr_h.detach()))
                scale = max(float(g.abs().max()) for g in g_b)
                row["batched_vs_hip_param_grad_diff"] = max(float((q.grad - g).abs().max()) for q, g in zip(s.occ.parameters(), g_b)) / scale
                row["batched_over_hip_median"] = row["batched_step_ms"] / row["hip_step_ms"]
            os.environ.pop("MCR_SCONE_OCC_BWD", None)
            torch.manual_seed(1000)
            sites = count_syncs(batched)
            row["host_syncs_in_function"] = int(sum(sites.values()))
            row["host_sync_sites"] = dict(sites)
        os.environ.pop("MCR_SCONE_OCC_BWD", None)
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
