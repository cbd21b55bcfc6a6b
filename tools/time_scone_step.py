"""Time the online trainer's SCONE step -- scone_supervision_step and scone_loss.backward() -- against the same step composed from
the per-frame calls that existed before it, at the trainer's size, and count the function's host synchronisations.

    python tools/time_scone_step.py [--iters 3] [--repeats 5] [--routes step,composed] [--out FILE.json]
    tools/kstats.sh scone_step -- python tools/time_scone_step.py --kernels-only 20        (the two kernels' own times)

The scene: liberty's grid of 6 x 2 x 6 = 72 cells, P = 100 000 proxy points, K = 4 depth frames of 256 x 456 pixels (analytic depth
maps of an ellipsoid seen from four poses on a ring, the sensor range past the far side), a surface store of seen points filled from an 80 000-point shell, a
proxy scene that has lived through one earlier frame, golden-seed weights; every parameter requires a gradient.  The occupancy field
handed to the step (X_world, view harmonics, occupancies: constants of the step, computed under no_grad by the trainer) is synthetic.
  step      macarons_utils.scone_supervision_step
  composed  upstream's body (train_macarons.py:375-513) written with the calls it took before: per frame a
            compute_partial_point_cloud, ops.points_in_fov, a compaction `points[mask]`, ops.signed_distance_to_depth and the
            overwrite of the close mask; the same two differentiable prediction calls; fill_cells; K camera_coverage_gain calls; a
            compacted proxy fill; per frame update_proxy_view_states and update_proxy_supervision_occ, then update_proxy_out_of_field
Every step starts from a copy of the same scenes and the same CPU-generator seed, so both routes make the same draws; the copy is not
timed.  A step is timed on the host clock between two device synchronisations (the composition's cost is largely the host waiting for
counts).  One repeat times --iters steps of each route, the routes taking turns; the JSON keeps every repeat's mean and the median /
min / max over the repeats.  Host synchronisations: torch.cuda.set_sync_debug_mode(1) around one call of the function (the method of
tools/find_syncs_macarons.py), with the call sites."""
import argparse
import copy
import json
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import Macarons, SconeOcc, SconeVis  # noqa: E402
from macarons_amd.utility import macarons_utils as mu  # noqa: E402
from macarons_amd.utility.scene import Scene  # noqa: E402
import _frames_cases as C  # noqa: E402
import weights  # noqa: E402
from time_occ_supervision import count_syncs  # noqa: E402

GRID = (6, 2, 6)
N_PROXY, N_SUP, K_NN, K = 100000, 6000, 16, 4
H, W = 256, 456
AXES = np.array([52., 17., 50.])
ZFAR, RANGE = 500., 220.
SURFACE_DISTANCE, CAP = 4.0, 5


def _camera(eye, at):
    R, T = C.look_at(eye, at)
    Mv = np.zeros((4, 4), np.float32)
    Mv[:3, :3], Mv[3, :3], Mv[3, 3] = R, T, 1.0
    P1 = C.projection(60.0, 1.0, ZFAR)
    Mf = (Mv @ P1).astype(np.float32)
    rec = mu.camera_record(Mv, Mf, C.ndc_bounds(H, W), eye, RANGE)
    cam18 = mu.depth_camera_record(Mf, float(P1[2, 2]), float(P1[3, 2]))
    depth, hit = C.ellipsoid_depth(H, W, eye, R, AXES)
    return NS(camera=mu.SceneCamera(rec, torch.from_numpy(np.asarray(eye, np.float32)), ZFAR), cam18=cam18, depth=torch.from_numpy(depth),
              mask=torch.from_numpy(hit), Mv=torch.from_numpy(Mv))


def build(dev):
    rng = np.random.default_rng(0)
    x_min, x_max = torch.tensor([-60., -20., -60.], device=dev), torch.tensor([60., 20., 60.], device=dev)
    surface = Scene(x_min, x_max, *GRID, cell_capacity=1000, cell_resolution=0.05, n_proxy_points=N_PROXY, device=dev, feature_dim=1)
    d = rng.standard_normal((80000, 3))
    shell = (d / np.linalg.norm(d, axis=1, keepdims=True) * AXES + 1.5 * rng.standard_normal((80000, 3))).astype(np.float32)
    torch.manual_seed(1)
    surface.fill_cells(torch.from_numpy(shell).to(dev), features=torch.ones(len(shell), 1, device=dev))
    proxy = Scene(x_min, x_max, *GRID, cell_capacity=100000, cell_resolution=1e-4, n_proxy_points=N_PROXY, device=dev, feature_dim=1,
                  score_threshold=0.95)
    torch.manual_seed(2)
    proxy.initialize_proxy_points()
    ring = lambda a, r=110.: np.array([r * np.cos(a), 25. * np.sin(2 * a), r * np.sin(a)], np.float32)      # noqa: E731
    cams = [_camera(ring(0.3 + 0.35 * k), np.array([4. * k, 0., -3. * k], np.float32)) for k in range(-1, K)]
    first = cams[0]                                          # the earlier frame: registers its frustum, carves, leaves non-zero counters
    rec0 = first.camera.record.to(dev)
    m0 = ops.points_in_fov(proxy.proxy_points, rec0.view(1, 40))[0]
    idx_f = torch.arange(N_PROXY, device=dev, dtype=torch.float32).view(-1, 1)
    proxy.fill_cells(proxy.proxy_points, features=idx_f, valid=m0)
    proxy.update_from_depth(m0, rec0, first.camera.X_cam.to(dev), first.depth.to(dev), first.mask.to(dev), 1.1 * ZFAR, tol=0.05)
    frames = [(c.depth.to(dev), c.mask.to(dev), torch.from_numpy(rng.random((H, W)) > 0.1).to(dev), c.camera, c.cam18) for c in cams[1:]]
    occ, vis = SconeOcc(), SconeVis()
    sdo, sdv = weights.make_state_dict(weights.shapes_of(occ), 2), weights.make_state_dict(weights.shapes_of(vis), 1)
    sdo["linear3.bias"] = sdo["linear3.bias"] + np.float32(0.5)
    occ.load_state_dict({k: torch.from_numpy(v) for k, v in sdo.items()}, strict=True)
    vis.load_state_dict({k: torch.from_numpy(v) for k, v in sdv.items()}, strict=True)
    occ, vis = occ.to(dev), vis.to(dev)
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=K_NN, prediction_neighborhood_size=3,
                n_view_state_cameras=98, n_proxy_point_for_occupancy_supervision=N_SUP, sensor_range=RANGE, min_occ_for_proxy_points=0.1,
                seq_len=2048, distance_factor_th=17., image_height=H, image_width=W, carving_tolerance=0.05, n_proxy_points=N_PROXY,
                gathering_factor=0.05, surface_epsilon_factor=2.0, occ_loss_fn="mse", cov_loss_fn="uncentered_l1")
    field = NS(X_world=proxy.proxy_points.clone(), vh=torch.from_numpy((rng.standard_normal((N_PROXY, 64)) * .3).astype(np.float32)).to(dev),
               occ=torch.from_numpy(rng.uniform(0, 1, (N_PROXY, 1)).astype(np.float32)).to(dev))
    # the scene's constants (grid tables of the field pass, box diagonal) are read back once per scene object: here, so that the copies
    # every timed step starts from carry them, for both routes
    mu._field_prepare(params, proxy, first.Mv, dev)
    proxy._mcr_box_diag = torch.linalg.norm(proxy.x_max - proxy.x_min).item()
    return NS(surface=surface, proxy=proxy, frames=frames, occ=occ, vis=vis, m=Macarons(None, occ, vis), Mpred=first.Mv, params=params,
              field=field, dev=dev, occ_fn=mu.get_occ_loss_fn(params), cov_fn=mu.get_cov_loss_fn(params))


def new_step(s, ss, ps, **kw):
    f = s.field
    return mu.scone_supervision_step(s.params, s.m, ps, ss, s.frames, f.X_world, f.vh, f.occ, SURFACE_DISTANCE, CAP, s.occ_fn, s.cov_fn, s.dev,
                                     prediction_camera=s.Mpred, **kw)["scone_loss"]


def composed_step(s, ss, ps):
    """The same step from the calls that were there before scone_supervision_step (upstream's body, statement by statement)."""
    params, dev, f = s.params, s.dev, s.field
    part_pcs, masks, sgns, recs, xcs = [], [], [], [], []
    general = torch.zeros(N_PROXY, dtype=torch.bool, device=dev)
    close = torch.zeros(N_PROXY, dtype=torch.bool, device=dev)
    for depth, mask, emask, cam, cam18 in s.frames:
        rec, xc = ops.h2d(cam.record, torch.float32, dev), ops.h2d(cam.X_cam, torch.float32, dev)
        part_pcs.append(mu.compute_partial_point_cloud(depth.view(1, H, W, 1), (mask & emask).view(1, H, W, 1), cam18, params.gathering_factor,
                                                       params.sensor_range))
        fov_mask = ops.points_in_fov(ps.proxy_points, rec.view(1, 40))[0]
        fov_pts = ps.proxy_points[fov_mask]                                    # the compaction: a count read-back
        sgn = ops.signed_distance_to_depth(fov_pts.contiguous(), rec, depth, mask, 1.1 * cam.zfar)
        general = general | fov_mask
        close[fov_mask] = sgn.abs() < SURFACE_DISTANCE
        masks.append(fov_mask); sgns.append(sgn); recs.append(rec); xcs.append(xc)
    close = close & (ps.out_of_field[..., 0] < 1.)
    prediction_mask, predicted_occs = mu.compute_occupancy_probability_for_supervision(params, s.m, None, ps, close, ss, CAP, dev,
                                                                                       prediction_camera=s.Mpred, differentiable=True)
    diag = ps._mcr_box_diag
    Mv = ops.h2d(s.Mpred.reshape(1, 4, 4), torch.float32, dev).expand(K, -1, -1)
    gains = mu.predict_coverage_gain_for_cameras(s.vis, f.X_world, f.vh, f.occ, torch.stack(recs), torch.cat(xcs).view(K, 3), Mv, diag,
                                                 seq_len=params.seq_len, min_occ=params.min_occ_for_proxy_points,
                                                 distance_th=params.distance_factor_th, differentiable=True).view(K, 1)
    complete = torch.cat(part_pcs)
    features = torch.zeros(len(complete), 1, device=dev)
    features[:len(part_pcs[0])] = 1.
    ss.fill_cells(complete, features=features)
    sup_gains = torch.zeros(K, 1, device=dev)
    for i in range(K):
        sup_gains[i, 0] = ss.camera_coverage_gain(part_pcs[i], surface_epsilon=None, surface_epsilon_factor=params.surface_epsilon_factor)
    ss.set_all_features_to_value(value=1.)
    idx = ps.get_proxy_indices_from_mask(general)
    ps.fill_cells(ps.proxy_points[general], features=idx.view(-1, 1).float())
    for i in range(K):
        ps.update_proxy_view_states(None, masks[i], signed_distances=sgns[i], distance_to_surface=None, X_cam=xcs[i])
        ps.update_proxy_supervision_occ(masks[i], sgns[i], tol=params.carving_tolerance)
    ps.update_proxy_out_of_field(general)
    occ_loss = s.occ_fn(predicted_occs, ps.proxy_supervision_occ[prediction_mask]) * predicted_occs.shape[0] / N_SUP
    return occ_loss + s.cov_fn(gains.view(1, -1, 1), sup_gains.view(1, -1, 1))


def kernels_only(s, n):
    """The two K-frame entries, and the per-frame entries they replace (ops.points_in_fov, ops.signed_distance_to_depth on ALL points,
    ops.proxy_scene_update_), n times each on the built scene: under `rocprofv3 --kernel-trace --stats` the kernels' own times."""
    dev, ps = s.dev, copy.deepcopy(s.proxy)
    recs = torch.stack([f[3].record for f in s.frames]).to(dev)
    xc = torch.stack([f[3].X_cam.reshape(3) for f in s.frames]).to(dev)
    depths, masks = torch.stack([f[0] for f in s.frames]), torch.stack([f[1] for f in s.frames])
    tables = (ps.view_states, ps.proxy_n_inside_fov, ps.proxy_n_behind_depth, ps.proxy_supervision_occ, ps.out_of_field)
    dts = 3 * ps.distance_between_proxy_points
    for _ in range(n):
        bits, sgn, _ = ops.supervision_frames(ps.proxy_points, recs, depths, masks, [1.1 * ZFAR] * K, SURFACE_DISTANCE)
        ops.proxy_scene_update_frames_(ps.proxy_points, bits, sgn, xc, dts, 0.05, ps.score_threshold, 7, 14, *tables)
        planes = ops.points_in_fov(ps.proxy_points, recs)
        for k in range(K):
            ops.signed_distance_to_depth(ps.proxy_points, recs[k], depths[k], masks[k], 1.1 * ZFAR)
            ops.proxy_scene_update_(ps.proxy_points, planes[k], recs[k], depths[k], masks[k], 1.1 * ZFAR, xc[k], dts, 0.05, ps.score_threshold,
                                    7, 14, *tables)
    torch.cuda.synchronize()
    print(json.dumps({"kernels_only": n, "P": N_PROXY, "K": K, "image": [H, W]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--routes", default="step,composed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N",
                    help="run the two K-frame entries and the per-frame entries they replace N times each and exit (for a kernel trace)")
    a = ap.parse_args()
    routes = a.routes.split(",")
    assert set(routes) <= {"step", "composed"}, routes
    dev = torch.device("cuda:0")
    s = build(dev)
    if a.kernels_only:
        return kernels_only(s, a.kernels_only)
    fns = {"step": new_step, "composed": composed_step}

    def one(route, it):
        ss, ps = copy.deepcopy(s.surface), copy.deepcopy(s.proxy)          # not timed
        s.m.zero_grad(set_to_none=True)
        torch.manual_seed(1000 + it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = fns[route](s, ss, ps)
        loss.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, loss.detach(), ps

    for r in routes:                                                        # warm-up: allocator, pinned pool, code objects
        one(r, 0)
    runs = {r: [] for r in routes}
    for _ in range(a.repeats):
        for r in routes:
            runs[r].append(float(np.mean([one(r, it)[0] for it in range(a.iters)])))
    row = {"grid": list(GRID), "n_proxy": N_PROXY, "K": K, "image": [H, W], "n_sup": N_SUP, "cap": CAP, "iters": a.iters, "repeats": a.repeats}
    for r, v in runs.items():
        row[f"{r}_ms"], row[f"{r}_min_ms"], row[f"{r}_max_ms"], row[f"{r}_runs_ms"] = float(np.median(v)), min(v), max(v), v
    if len(routes) == 2:
        (_, l_a, ps_a), (_, l_b, ps_b) = one("step", 0), one("composed", 0)
        row["loss"] = float(l_a)
        row["loss_equal"] = bool(torch.equal(l_a, l_b))
        row["state_equal"] = all(bool(torch.equal(getattr(ps_a, n), getattr(ps_b, n))) for n in
                                 ("view_states", "proxy_n_inside_fov", "proxy_n_behind_depth", "proxy_supervision_occ", "out_of_field"))
        row["step_over_composed_median"] = row["step_ms"] / row["composed_ms"]
        row["faster_by_more_than_the_composition_s_spread"] = bool(row["composed_ms"] - row["step_ms"] > row["composed_max_ms"] - row["composed_min_ms"])
    if "step" in routes:
        ss, ps = copy.deepcopy(s.surface), copy.deepcopy(s.proxy)
        torch.manual_seed(1000)
        sites = count_syncs(lambda: new_step(s, ss, ps))
        row["host_syncs_in_function"], row["host_sync_sites"] = int(sum(sites.values())), dict(sites)
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
