#!/usr/bin/env python3
"""Golden of the online trainer's SCONE step: the REFERENCE's own `memory_scene_loop` (macarons/trainers/train_macarons.py:577-780,
the same body as `loop` :375-513) called as it stands, on the reference's Scene / Cell / Camera objects (build container only).

    python tests/golden/make_golden_scone_step.py        ->  tests/golden/scone_step.npz

The trainer module imports under _ref_import's stubs, so the function itself runs; what the harness supplies is what the trainer reads
from outside: the depth files (`torch.load` of `<depths_memory_path>/<i>.pt` returns the analytic ellipsoid depth maps of
make_golden.py), the PyTorch3D cameras (`camera.get_fov_camera_from_RT` returns make_golden's stand-in cameras), the sampling uniforms
(`torch.rand` returns keyed_rng's, moved off the steps of the exact CDF as gen_trajectory does) and the occupancy field the function
computes first under no_grad (:598: computed once here with the reference function, its view harmonics rounded to the 2^-9 grid so
that they fit the file, handed to the function and stored as the step's inputs; the CPU generator is seeded AFTER it, so the recorded
draws are the step's own).
Scene: 2 x 1 x 2 grid, P = 3001 proxy points on the 2^-6 grid, an ellipsoid shell of stored surface points (all seen), a proxy scene
that has lived through one earlier frame (non-zero counters, score threshold 0.95); K = 3 frames of 24 x 40 pixels: frames 0 and 1
overlap (the overwrite rule of :661 decides the points both hold), frame 2 looks away (no pixel hit, no proxy point in its frustum).
Two cases from the same start: supervise_with_online_field True and False (only occ_loss differs).
The proxy points are redrawn until ZERO sit on a decision boundary (asserted): signed distance within 2e-3 of +-surface_distance,
distance_to_surface or -tol; frustum / range margins; view-state bin edges; kNN k / k+1 ties of the supervised queries under the
draws the function makes.  A redrawn point keeps its cell and its side of every decision, so the draw sizes do not move and the loop
converges.  Pixels whose unprojected point decides Cell.fill's admission or the coverage test within 2e-4, or sits within 2e-4 of a
cell face, are taken out through the frames' error masks (the kernels' unprojection differs from PyTorch3D's in the last bits).
Only data is written."""
import importlib
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (_ref_macarons, _ref_camera, _StandInCameras, _look_at_target, _ellipsoid_depth, _fov_projection, _grid,  # noqa: E402
                         _boundary_ties, save, t)
import keyed_rng as KR  # noqa: E402
import torch  # noqa: E402
from oracle import view_state as V  # noqa: E402

K_NN, N_SUP, CAP = 16, 50, 3
H, W = 24, 40
G = 64.0
AXES = np.array([5.5, 2.8, 5.0])
ZFAR = 500.
BASE = 7300
SEED_SETUP, SEED_FIELD, SEED_STEP = 7301, 7302, 7303
SURFACE_DISTANCE = 1.5
EYES = np.array([[5., 5., 9.], [9.5, 2., 3.], [7., -1., 8.], [9., 1., -8.]], np.float32)     # the earlier frame, then the K = 3 frames
ATS = np.array([[0., 0., 0.], [1., 0.3, 0.5], [0.5, 0., 1.], [36., 4., -32.]], np.float32)


def main():
    tm = importlib.import_module("macarons.trainers.train_macarons")
    mu = importlib.import_module("macarons.utility.macarons_utils")
    m = _ref_macarons()
    rng = np.random.default_rng(733)
    x_min, x_max = torch.tensor([-8., -4., -8.]), torch.tensor([8., 4., 8.])
    grid = (2, 1, 2)
    P = 3001
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=K_NN,
                prediction_neighborhood_size=3, n_view_state_cameras=98, sensor_range=24., min_occ_for_proxy_points=0.1, seq_len=2048,
                use_occ_to_sample_proxy_points=True, jz=False, ddp=False, distance_factor_th=17., image_height=H, image_width=W,
                carving_tolerance=0.05, n_proxy_points=P, n_poses_in_memory_scene_loops=3, random_poses_in_memory_scene_loops=False,
                gathering_factor=0.9, n_proxy_point_for_occupancy_supervision=N_SUP, surface_epsilon_factor=2.0,
                occ_loss_fn="mse", cov_loss_fn="uncentered_l1")
    cam = _ref_camera(mu, H, W)
    ndc = np.array([cam.min_ndc_x, cam.max_ndc_x, cam.min_ndc_y, cam.max_ndc_y], np.float64)
    P1 = _fov_projection(60.0, 1.0, ZFAR)
    Rc, Tc = _look_at_target(EYES, ATS)
    fcs = [_StandInCameras(t(Rc[c:c + 1]), t(Tc[c:c + 1]), t(P1[None]), squeeze=True) for c in range(4)]
    depth_np, hit_np = zip(*[_ellipsoid_depth(cam.ndc_x_tab.numpy(), cam.ndc_y_tab.numpy(), EYES[c], Rc[c], AXES) for c in range(4)])
    assert not hit_np[3].any() and min(h.sum() for h in hit_np[:3]) > 100
    err_np = [np.ones((H, W), bool) for _ in range(4)]
    for c in range(1, 4):
        err_np[c] &= rng.random((H, W)) > 0.1                     # the error mask drops a tenth of the pixels from the clouds
    Rp, Tp = _look_at_target(np.array([[6., 9., -14.]], np.float32), np.zeros((1, 3), np.float32))
    pred = _StandInCameras(t(Rp), t(Tp), t(P1[None]), squeeze=True)
    pseudo_gt = (rng.random((P, 1)) < 0.4).astype(np.float32)

    def new_scene(capacity, resolution, feature_dim, score_threshold=1.):
        return mu.Scene(x_min=x_min, x_max=x_max, grid_l=grid[0], grid_w=grid[1], grid_h=grid[2], cell_capacity=capacity,
                        cell_resolution=resolution, n_proxy_points=P, device="cpu", feature_dim=feature_dim, score_threshold=score_threshold)
    d = rng.standard_normal((1500, 3))
    surf = np.unique(_grid(d / np.linalg.norm(d, axis=1, keepdims=True) * AXES + 0.05 * rng.standard_normal((1500, 3)), G), axis=0)
    surf[surf == 0] = 1.0 / G
    rng.shuffle(surf)

    def draw_proxy(n):
        q = _grid(rng.uniform(-1, 1, (n, 3)) * [7.9, 3.9, 7.9], G)
        q[q == 0] = 1.0 / G                       # Cell.fill's box tests are strict: a point ON a cell face belongs to no cell
        return q
    proxy = draw_proxy(P)

    def dmap(c):
        return t(depth_np[c]).view(1, H, W, 1), torch.from_numpy(hit_np[c]).view(1, H, W, 1)

    def frustum_margin(pts, c):
        fc = fcs[c]
        Mv, Mf = fc.Mv[0].double().numpy(), (fc.Mv[0].double() @ fc.P[0].double()).numpy()
        p4 = np.concatenate((pts.astype(np.float64), np.ones((len(pts), 1))), 1)
        pr, vw = p4 @ Mf, p4 @ Mv
        nx, ny = pr[:, 0] / pr[:, 3], pr[:, 1] / pr[:, 3]
        mg = np.minimum.reduce([np.abs(nx - ndc[0]), np.abs(nx - ndc[1]), np.abs(ny - ndc[2]), np.abs(ny - ndc[3])])
        rg = np.abs(np.linalg.norm(pts.astype(np.float64) - EYES[c].astype(np.float64), axis=1) - params.sensor_range)
        return np.minimum(np.minimum(mg, np.abs(vw[:, 2]) * 1e-1), rg * 1e-1)

    dts_box = [None]

    def classify(pts):
        """Per point: the side of every decision it takes (an integer signature) and whether it sits on a boundary of the K frames."""
        n = len(pts)
        sig = np.zeros(n, np.int64)
        bad = np.zeros(n, bool)
        tol, dts = params.carving_tolerance, dts_box[0]
        for c in range(4):
            dm, hm = dmap(c)
            sel, mask = cam.get_points_in_fov(t(pts), return_mask=True, fov_camera=fcs[c], fov_range=params.sensor_range)
            mk = mask.numpy()
            sg = cam.get_signed_distance_to_depth_maps(pts=sel, depth_maps=dm, mask=hm, fov_camera=fcs[c]).view(-1).numpy()
            code = np.zeros(n, np.int64)
            code[mk] = 1 + (sg < dts) + 2 * (sg >= -tol) + 4 * (np.abs(sg) < SURFACE_DISTANCE)
            sig = sig * 16 + code
            if c == 0:
                continue                                  # the earlier frame only shapes the recorded start state
            bad |= frustum_margin(pts, c) < 2e-5
            near = np.zeros(n, bool)
            near[mk] = np.minimum.reduce([np.abs(sg - dts), np.abs(sg + tol), np.abs(sg - SURFACE_DISTANCE), np.abs(sg + SURFACE_DISTANCE)]) < 2e-3
            bad |= near
            upd = np.zeros(n, bool)
            upd[mk] = sg < dts
            if upd.any():
                mg = V.bin_boundary_margin(pts[upd][None], EYES[c][None], 7, 14)[0, :, 0]
                b2 = np.zeros(n, bool)
                b2[np.nonzero(upd)[0][mg < 3e-6]] = True
                bad |= b2
        cell = (pts[:, 0] > 0).astype(np.int64) * 2 + (pts[:, 2] > 0).astype(np.int64)
        return sig * 4 + cell, bad

    def build():
        """The start state: stored surface (all seen), a proxy scene after the earlier frame."""
        torch.manual_seed(SEED_SETUP)
        ss = new_scene(500, 0.2, 1)
        ss.fill_cells(t(surf), features=torch.ones(len(surf), 1))
        ps = new_scene(100000, 1e-4, 1, score_threshold=0.95)
        ps.initialize_proxy_points()
        ps.proxy_points = t(proxy)
        dts_box[0] = 3 * ps.distance_between_proxy_points
        dm, hm = dmap(0)
        cam.fov_camera, cam.X_cam, cam.fov_camera_0 = fcs[0], t(EYES[0:1]), fcs[0]
        pts0, mask0 = cam.get_points_in_fov(ps.proxy_points, return_mask=True, fov_camera=None, fov_range=params.sensor_range)
        ps.fill_cells(pts0, features=ps.get_proxy_indices_from_mask(mask0).view(-1, 1))
        sg0 = cam.get_signed_distance_to_depth_maps(pts=pts0, depth_maps=dm, mask=hm, fov_camera=None)
        ps.update_proxy_view_states(cam, mask0, signed_distances=sg0, distance_to_surface=None, X_cam=None)
        ps.update_proxy_supervision_occ(mask0, sg0, tol=params.carving_tolerance)
        ps.update_proxy_out_of_field(mask0)
        return ss, ps

    def field(ss, ps):
        torch.manual_seed(SEED_FIELD)
        with torch.no_grad():
            Xw, vh, occ = mu.compute_scene_occupancy_probability_field(params, m, None, ss, ps, "cpu", prediction_camera=pred,
                                                                       use_supervision_occ_instead_of_predicted=False)
        vh_q = torch.round(vh * 512.).clamp(-32767, 32767) / 512.
        return Xw, vh_q, occ

    def uniforms(Xw, occ, fix):
        """keyed uniforms per frame, moved to the middle of their CDF interval where they sit within 1e-6 of a step (gen_trajectory)."""
        out = []
        occ_np = occ.numpy()
        for k in range(3):
            u = KR.keyed_uniforms(BASE, 0, k)
            for j_, v_ in fix.setdefault(k, {}).items():
                u[j_, 0] = v_
            _, km = cam.get_points_in_fov(Xw, return_mask=True, fov_camera=fcs[k + 1], fov_range=params.sensor_range)
            kept = km.numpy() & (occ_np[:, 0] > params.min_occ_for_proxy_points)
            if kept.any():
                cn = np.cumsum(occ_np[kept, 0].astype(np.float64))
                cn /= cn[-1]
                u64 = u.numpy().reshape(-1).astype(np.float64)
                ii = np.minimum(np.searchsorted(cn, u64, side="left"), len(cn) - 1)
                lower, upper = np.where(ii > 0, cn[np.maximum(ii - 1, 0)], 0.0), cn[ii]
                for j_ in np.nonzero(np.minimum(upper - u64, u64 - lower) < 1e-6)[0].tolist():
                    fix[k][j_] = float(np.float32((lower[j_] + upper[j_]) / 2))
                    u[j_, 0] = fix[k][j_]
            out.append(u)
        return out

    def run(online, fld, us):
        """One call of the reference's memory_scene_loop from the start state.  -> everything observed."""
        ss, ps = build()
        Xw, vh_q, occ = fld
        before = state_of(ss, ps)
        ob = dict(perms=[], passes=[], sgn=[], masks=[], cdist=[], clouds=[], stage=["other"], cam_k=[0], last=[None, None], sup=None)
        real = dict(randperm=torch.randperm, rand=torch.rand, cdist=torch.cdist, load=tm.torch.load, field=tm.compute_scene_occupancy_probability_field,
                    occ=mu.compute_occupancy_probability, sup=tm.compute_occupancy_probability_for_supervision,
                    pred=tm.predict_coverage_gain_for_single_camera)

        def w_randperm(n, *a, **kw):
            p_ = real["randperm"](n, *a, **kw); ob["perms"].append(p_.numpy().copy()); return p_

        def w_cdist(a, b, *x, **kw):
            r_ = real["cdist"](a, b, *x, **kw)
            if ob["stage"][0] != "other" and r_.numel():
                ob["cdist"].append((ob["stage"][0], r_.min(dim=-1)[0].numpy().copy()))
            return r_

        def w_load(path, *a, **kw):
            c = int(os.path.basename(path).split(".")[0]) + 1
            dm, hm = dmap(c)
            return dict(depth=dm, mask=hm.float(), error_mask=torch.from_numpy(err_np[c]).view(1, H, W, 1).float(), R=t(Rc[c:c + 1]), T=t(Tc[c:c + 1]))

        def w_field(*a, **kw):
            torch.manual_seed(SEED_STEP)                  # the step's own draws start here
            return Xw, vh_q, occ

        def w_occ(*a, **kw):
            n0 = len(ob["perms"])
            r_ = real["occ"](*a, **kw)
            if ob["last"][0] is not None:
                ob["passes"].append((ob["last"][0], ob["last"][1], n0, len(ob["perms"])))
                ob["last"][0] = None
            return r_

        def w_sup(params_, mac, cam_, ps_, mask_, ss_, cap_, dev_, **kw):
            ob["close"] = mask_.numpy().copy()
            real_pc, real_sc = ps_.get_pt_cloud_from_cells, ss_.get_pt_cloud_from_cells

            def pc_cloud(cell, return_features=True):
                res = real_pc(cell, return_features=return_features)
                ob["last"][0] = (cell.numpy().copy(), res[1].numpy().copy())
                return res

            def sc_cloud(cells, return_features=True):
                res = real_sc(cells, return_features=return_features)
                ob["last"][1] = (res if not return_features else res[0]).numpy().copy()
                return res
            ps_.get_pt_cloud_from_cells, ss_.get_pt_cloud_from_cells = pc_cloud, sc_cloud
            ob["n_perm_sup0"] = len(ob["perms"])
            try:
                r_ = real["sup"](params_, mac, cam_, ps_, mask_, ss_, cap_, dev_, **kw)
            finally:
                del ps_.get_pt_cloud_from_cells, ss_.get_pt_cloud_from_cells
            ob["n_perm_sup1"] = len(ob["perms"])
            ob["sup"] = (r_[0].numpy().copy(), r_[1].detach().numpy().copy())
            return r_

        def w_pred(*a, **kw):
            k = ob["cam_k"][0]
            torch.rand = lambda *a_, **kw_: us[k].clone()
            try:
                r_ = real["pred"](*a, **kw)
            finally:
                torch.rand = real["rand"]
            ob["cam_k"][0] = k + 1
            ob.setdefault("pred_gains", []).append(r_[3].detach().numpy().copy())
            return r_
        n_cam = [0]

        def w_fov_cam(R_cam, T_cam):
            n_cam[0] += 1
            return fcs[n_cam[0]]
        real_sgn, real_fov, real_pp = cam.get_signed_distance_to_depth_maps, cam.get_points_in_fov, cam.compute_partial_point_cloud

        def w_sgn(*a, **kw):
            r_ = real_sgn(*a, **kw); ob["sgn"].append(r_.view(-1).numpy().copy()); return r_

        def w_fov(pts, *a, **kw):
            r_ = real_fov(pts, *a, **kw)
            if pts is ps.proxy_points:
                ob["masks"].append(r_[1].numpy().copy())
            return r_

        def w_pp(*a, **kw):
            r_ = real_pp(*a, **kw); ob["clouds"].append(r_.numpy().copy()); return r_
        real_sfill, real_gain, real_pfill = ss.fill_cells, ss.camera_coverage_gain, ps.fill_cells

        def w_sfill(*a, **kw):
            ob["stage"][0] = "fill"; ob["n_perm_sfill"] = len(ob["perms"])
            try:
                return real_sfill(*a, **kw)
            finally:
                ob["stage"][0] = "other"

        def w_gain(*a, **kw):
            ob["stage"][0] = "gain"
            try:
                r_ = real_gain(*a, **kw)
            finally:
                ob["stage"][0] = "other"
            ob.setdefault("sup_gains", []).append(float(r_))
            return r_

        def w_pfill(*a, **kw):
            ob["n_perm_pfill"] = len(ob["perms"])
            return real_pfill(*a, **kw)
        torch.randperm, torch.cdist, tm.torch.load = w_randperm, w_cdist, w_load
        tm.compute_scene_occupancy_probability_field, mu.compute_occupancy_probability = w_field, w_occ
        tm.compute_occupancy_probability_for_supervision, tm.predict_coverage_gain_for_single_camera = w_sup, w_pred
        cam.get_fov_camera_from_RT, cam.get_signed_distance_to_depth_maps, cam.get_points_in_fov = w_fov_cam, w_sgn, w_fov
        cam.compute_partial_point_cloud = w_pp
        ss.fill_cells, ss.camera_coverage_gain, ps.fill_cells = w_sfill, w_gain, w_pfill
        try:
            scone_loss, occ_loss, cov_loss, _ = tm.memory_scene_loop(
                params, 0, None, cam, "depths", ss, None, ps, t(pseudo_gt), pred, 0, SURFACE_DISTANCE, CAP, NS(scone=m),
                mu.get_occ_loss_fn(params), mu.get_cov_loss_fn(params), "cpu", False, print_result=False,
                supervise_with_online_field=online, warmup_phase=False, depth_list=[0])
        finally:
            torch.randperm, torch.cdist, tm.torch.load, torch.rand = real["randperm"], real["cdist"], real["load"], real["rand"]
            tm.compute_scene_occupancy_probability_field, mu.compute_occupancy_probability = real["field"], real["occ"]
            tm.compute_occupancy_probability_for_supervision, tm.predict_coverage_gain_for_single_camera = real["sup"], real["pred"]
            for n_ in ("get_fov_camera_from_RT", "get_signed_distance_to_depth_maps", "get_points_in_fov", "compute_partial_point_cloud"):
                delattr(cam, n_)
            del ss.fill_cells, ss.camera_coverage_gain, ps.fill_cells
        ob["rng_state"] = torch.get_rng_state().numpy().copy()
        ob["losses"] = np.array([float(scone_loss), float(occ_loss), float(cov_loss)], np.float64)
        ob["before"], ob["after"] = before, state_of(ss, ps)
        ob["ss"], ob["ps"] = ss, ps
        return ob

    def state_of(ss, ps):
        return dict(view_states=ps.view_states.numpy().copy(), n_inside=ps.proxy_n_inside_fov.numpy()[:, 0].copy(),
                    n_behind=ps.proxy_n_behind_depth.numpy()[:, 0].copy(), sup_occ=ps.proxy_supervision_occ.numpy()[:, 0].copy(),
                    oof=ps.out_of_field.numpy()[:, 0].copy(),
                    surface={k: (c.cell_pts.numpy().copy(), c.cell_features.numpy().copy()) for k, c in sorted(ss.cells.items())},
                    proxy={k: c.cell_features.numpy()[:, 0].astype(np.int32).copy() for k, c in sorted(ps.cells.items())})

    def boundaries(ob):
        """-> (proxy indices on a boundary, [(frame, pixel)] to mask out)."""
        bad = set()
        _, local = classify(proxy)
        bad |= set(np.nonzero(local)[0].tolist())
        pm = ob["sup"][0]
        for (cell, ind), pcw, n0, n1 in ob["passes"]:
            cmask = np.zeros(P, bool)
            cmask[ind[:, 0].astype(np.int64)] = True
            cmask &= pm
            Xw_, gi = proxy[cmask], np.nonzero(cmask)[0]
            M = len(pcw)
            ds = int(np.power(M / (K_NN * 8), 1. / 2)) or 2
            assert [len(p_) for p_ in ob["perms"][n0:n1]] == [M, M, M // ds], ([len(p_) for p_ in ob["perms"][n0:n1]], M, ds)
            p1 = ob["perms"][n0 + 1][:M // ds]
            p2 = ob["perms"][n0 + 2][:(M // ds) // ds]
            pc1 = pcw[p1]; pc2 = pc1[p2]
            tie = _boundary_ties(Xw_, pcw, K_NN, G) | _boundary_ties(Xw_, pc1, K_NN, G) | _boundary_ties(Xw_, pc2, K_NN, G)
            bad |= set(gi[tie].tolist())
        # the clouds: a point that decides an admission (fill: > 0.2) or a coverage test (< 0.4) within 2e-4, or next to a cell face
        n_pix = 0
        res, eps = ob["ss"].cell_resolution, ob["ss"].cell_resolution * params.surface_epsilon_factor
        n_dec = sum(int((np.abs(dmin - (res if st == "fill" else eps)) < 2e-4).sum()) for st, dmin in ob["cdist"])
        near_face = [np.nonzero((np.abs(c_[:, [0, 2]]) < 2e-4).any(1) | (np.abs(np.abs(c_) - x_max.numpy()) < 2e-4).any(1))[0] for c_ in ob["clouds"]]
        n_face = sum(len(v) for v in near_face)
        return sorted(bad), n_dec, n_face

    fix = {}
    for it in range(80):
        ss, ps = build()
        fld = field(ss, ps)
        us = uniforms(fld[0], fld[2], fix)
        ob = run(True, fld, us)
        bad, n_dec, n_face = boundaries(ob)
        print(f"  scone_step: pass {it}: {len(bad)} proxy points on a boundary, {n_dec} cloud decisions within 2e-4, {n_face} cloud points at a face; "
              f"close {int(ob['close'].sum())}, predicted {int(ob['sup'][0].sum())}, passes {len(ob['passes'])}")
        if not bad and not n_dec and not n_face:
            break
        if bad:
            sig_all, _ = classify(proxy)
            cand = draw_proxy(40000)
            sig_c, bad_c = classify(cand)
            used = np.zeros(len(cand), bool)
            for i in bad:
                ok = np.nonzero((sig_c == sig_all[i]) & ~bad_c & ~used)[0]
                assert len(ok), f"no replacement on the same side of every decision for proxy point {i}"
                proxy[i] = cand[ok[0]]
                used[ok[0]] = True
        if n_dec or n_face:                               # re-draw the error masks' dropped tenth: other pixels leave the clouds
            for c in range(1, 4):
                err_np[c] = rng.random((H, W)) > 0.1
    else:
        raise RuntimeError("no boundary-free scene found")
    assert not bad and not n_dec and not n_face
    ob2 = run(False, fld, us)
    for k_ in ("close", "rng_state"):
        assert np.array_equal(ob[k_], ob2[k_])
    assert np.array_equal(ob["sup"][1], ob2["sup"][1]) and ob["losses"][2] == ob2["losses"][2] and ob["losses"][1] != ob2["losses"][1]
    masks = np.stack(ob["masks"])
    assert masks.shape == (3, P) and not masks[2].any() and int((masks[0] & masks[1]).sum()) > 100
    decided = masks[0] & masks[1]                                     # points both frames hold
    s0, s1 = np.zeros(P, np.float32), np.zeros(P, np.float32)
    s0[masks[0]], s1[masks[1]] = ob["sgn"][0], ob["sgn"][1]
    n_overwritten = int((decided & ((np.abs(s0) < SURFACE_DISTANCE) != (np.abs(s1) < SURFACE_DISTANCE))).sum())
    assert n_overwritten > 0, "the overwrite rule decides no point"
    assert len(ob["clouds"][2]) == 0 and len(ob["passes"]) >= 1
    sgn = np.zeros((3, P), np.float32)
    for k in range(3):
        sgn[k, masks[k]] = ob["sgn"][k]
    Xw, vh_q, occ = fld
    lut = {tuple(r_): i_ for i_, r_ in enumerate(proxy.tolist())}
    x_idx = np.array([lut[tuple(r_)] for r_ in Xw.numpy().tolist()], np.int32)
    assert np.array_equal(proxy[x_idx], Xw.numpy())
    b, a = ob["before"], ob["after"]
    out = dict(x_min=x_min.numpy(), x_max=x_max.numpy(), grid=np.array(grid), hw=np.array([H, W]), G=np.float32(G), k=np.int64(K_NN),
               n_sup=np.int64(N_SUP), cap=np.int64(CAP), surface_distance=np.float32(SURFACE_DISTANCE), seed=np.int64(SEED_STEP),
               zfar=np.float32(ZFAR), sensor_range=np.float32(params.sensor_range), gathering_factor=np.float32(params.gathering_factor),
               carving_tolerance=np.float32(params.carving_tolerance), surface_epsilon_factor=np.float32(params.surface_epsilon_factor),
               min_occ=np.float32(params.min_occ_for_proxy_points), distance_factor_th=np.float32(params.distance_factor_th),
               score_threshold=np.float32(0.95), dts=np.float64(dts_box[0]), ndc=ndc.astype(np.float32), P=P1,
               proxy=np.round(proxy * G).astype(np.int16), pseudo_gt=np.packbits(pseudo_gt[:, 0].astype(np.uint8)),
               eyes=EYES[1:], Mview=np.stack([fcs[c].Mv.numpy()[0] for c in range(1, 4)]),
               Mfull=np.stack([fcs[c].get_full_projection_transform().M.numpy()[0] for c in range(1, 4)]), Mpred=pred.Mv.numpy()[0],
               depth=np.stack(depth_np[1:]), dmask=np.packbits(np.stack(hit_np[1:])), error_mask=np.packbits(np.stack(err_np[1:])),
               X_idx=x_idx, vh_q=np.round(vh_q.numpy() * 512).astype(np.int16), occ=occ.numpy()[:, 0].copy(),
               uniforms=np.stack([u.numpy()[:, 0] for u in us]),
               fov_masks=np.packbits(masks, axis=-1), sgn=sgn, close_mask=np.packbits(ob["close"]), n_overwritten=np.int64(n_overwritten),
               prediction_mask=np.packbits(ob["sup"][0]), predicted_occs=ob["sup"][1][:, 0].copy(),
               predicted_gains=np.concatenate([g_.reshape(-1) for g_ in ob["pred_gains"]]).astype(np.float32),
               supervision_gains=np.array(ob["sup_gains"], np.float32),
               perm_sizes=np.array([len(p_) for p_ in ob["perms"]], np.int64),
               perm_marks=np.array([ob["n_perm_sup0"], ob["n_perm_sup1"], ob["n_perm_sfill"], ob["n_perm_pfill"]], np.int64),
               sample_perm=ob["perms"][ob["n_perm_sup0"]].astype(np.int64), cell_perm=ob["perms"][ob["n_perm_sup0"] + 1].astype(np.int64),
               cells_run=np.array([int((c_[0] * grid[1] + c_[1]) * grid[2] + c_[2]) for (c_, _), _, _, _ in ob["passes"]], np.int64),
               rng_state=ob["rng_state"], losses_online=ob["losses"], losses_pseudo=ob2["losses"],
               cloud_sizes=np.array([len(c_) for c_ in ob["clouds"]], np.int64), clouds=np.concatenate(ob["clouds"]).astype(np.float32))
    for tag, s_ in (("before", b), ("after", a)):
        out[f"{tag}_view_states"] = np.packbits(s_["view_states"].astype(np.uint8), axis=-1)
        out[f"{tag}_n_inside"], out[f"{tag}_n_behind"] = s_["n_inside"].astype(np.uint8), s_["n_behind"].astype(np.uint8)
        out[f"{tag}_sup_occ"], out[f"{tag}_oof"] = np.packbits(s_["sup_occ"].astype(np.uint8)), np.packbits(s_["oof"].astype(np.uint8))
        for i, (k_, (pts_, fts_)) in enumerate(s_["surface"].items()):
            out[f"{tag}_skey_{i}"] = np.array(eval(k_))
            out[f"{tag}_spts_{i}"] = np.round(pts_ * G).astype(np.int16) if tag == "before" else pts_
            out[f"{tag}_sfts_{i}"] = fts_[:, 0].astype(np.uint8)
            if tag == "before":
                assert np.array_equal(out[f"{tag}_spts_{i}"].astype(np.float32) / np.float32(G), pts_)
        for i, (k_, idx_) in enumerate(s_["proxy"].items()):
            out[f"{tag}_pkey_{i}"] = np.array(eval(k_))
            out[f"{tag}_pidx_{i}"] = idx_
    assert np.array_equal(np.round(vh_q.numpy() * 512) / 512, vh_q.numpy())
    print(f"  losses online {ob['losses']}, pseudo {ob2['losses']}; predicted gains {out['predicted_gains']}, supervision gains {out['supervision_gains']}; "
          f"{len(ob['perms'])} randperm draws; overwrite rule decides {n_overwritten} points; cells run {out['cells_run'].tolist()}")
    save("scone_step", **out)
    print("  bytes:", os.path.getsize(os.path.join(HERE, "scone_step.npz")))


if __name__ == "__main__":
    main()
