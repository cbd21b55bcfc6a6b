"""The fused scene entries of csrc/scene.hip against their exact host model (tests/_scene_model.py), entry by entry and through Scene:
mcr_scene_fill_begin / _gather / _gather_perm, Scene.fill_cells (fused path and the upstream-way path for ambiguous points),
mcr_field_select / _build / _finish.  All of it is integer and byte bookkeeping plus fp32 / fp64 operations in a fixed order: every
comparison is array_equal / torch.equal.  The inputs come from tests/_scene_cases.py; tests/test_scene_model_cpu.py checks that they
keep clear of the admission threshold and contain the edges named below."""
import numpy as np
import pytest
import torch

import _scene_cases as C
import _scene_model as M

pytestmark = pytest.mark.gpu
F = np.float32


def _args(tab):
    return tab["lo"], tab["hi"], tab["x_min"], tab["x_max"], tab["step"], tab["grid"]


def _t(a, dev, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(dev)


def _gc(tab, dev):
    return _t(np.concatenate((tab["x_min"].reshape(3), tab["x_max"].reshape(3), tab["step"].reshape(3))), dev)


def _np(t):
    return t.cpu().numpy()


def _begin(ops, dev, tab, pts, valid, features, store_pts, store_off, resolution, npm):
    return ops.scene_fill_begin(_t(pts, dev), _t(valid, dev, torch.bool), _gc(tab, dev), tab["grid"], _t(tab["lo"], dev), _t(tab["hi"], dev),
                                _t(store_pts, dev) if len(store_pts) else None, _t(store_off, dev, torch.int64), resolution, npm,
                                features=_t(features, dev))


def _check_begin(h, m, tag):
    assert np.array_equal(_np(h.key), m["key"]), tag
    assert np.array_equal(_np(h.order), m["order"]), tag
    assert np.array_equal(_np(h.counts), m["counts"]), tag
    assert np.array_equal(_np(h.key2), m["key2"]), tag
    assert np.array_equal(_np(h.order2), m["order2"]), tag
    rows = m["dmin_rows"]                                 # the kernel never writes the rows of the rejected group
    assert np.array_equal(_np(h.dmin)[rows], m["dmin"][rows]), tag


# ---- the fill chain, entry by entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,grid", C.FILL_CASES)
@pytest.mark.parametrize("part_filled", [False, True])
def test_fill_chain_entry_by_entry(dev, N, grid, part_filled):
    """scene_fill_begin -> host read of counts -> scene_fill_gather_perm and scene_fill_gather, each against the model, for F in
    {0, 1, 3}, valid None / ~70 %, n_point_min 0 / 3.  The cases hold untouched cells between touched ones (shared offsets), duplicated
    candidates, candidates exactly at the resolution of a stored point, cells over capacity, odd n_pm, and (N = 1 with a store) a
    fill whose every candidate is rejected: n_new equals the old store (with n_point_min = 3 no cell is touched either)."""
    from macarons_amd import ops
    case = C.fill_case(N, grid, part_filled)
    tab, nk = case["tab"], int(np.prod(grid))
    for Fdim, frac, npm in C.FILL_VARIANTS:
        tag = (N, grid, part_filled, Fdim, frac, npm)
        valid = C.case_valid(case, frac)
        features, feats = C.case_features(case, Fdim)
        sp, so, sf = C.flat(case["store"], feats)
        n_store = int(so[-1])
        m = M.fill_begin_model(case["pts"], valid, *_args(tab), sp, so, case["resolution"], npm)
        h = _begin(ops, dev, tab, case["pts"], valid, features, sp, so, case["resolution"], npm)
        _check_begin(h, m, tag)
        counts = _np(h.counts)                                               # the host's read-back
        plan = C.gather_plan(counts, so, case["capacity"], npm, np.random.default_rng(N + npm))
        if N == 1 and part_filled:
            assert counts[2 * nk + 3:3 * nk + 3].sum() == 0 and plan["n_new"] == n_store         # every candidate rejected
        if plan["n_new"] == 0:
            continue
        pm32 = plan["pm"] if plan["n_pm"] % 2 == 0 else np.concatenate((plan["pm"], np.zeros(1, np.int32)))    # Scene's upload: padded to 8 B
        buf = _t(np.concatenate((plan["tables"], pm32.view(np.int64))), dev, torch.int64)
        sp_d, sf_d = _t(sp, dev), _t(sf, dev)
        got_p, got_f = ops.scene_fill_gather_perm(buf, plan["n_pm"], nk, plan["n_new"], h, sp_d, sf_d, n_store, Fdim)
        order, order2 = m["order"], m["order2"]
        want_p, want_f = M.gather_perm_model(plan["pm"], plan["tables"], nk, plan["n_new"], sp, sf, n_store, Fdim, case["pts"], features, order, order2)
        assert np.array_equal(_np(got_p), want_p), tag
        assert (got_f is None and want_f is None) or np.array_equal(_np(got_f), want_f), tag
        # the explicit row map: the same rows
        g = M.perm_row_map(plan["pm"], plan["tables"], nk, plan["n_new"], n_store)
        got2_p, got2_f = ops.scene_fill_gather(_t(g, dev, torch.int64), h, sp_d, sf_d, n_store, Fdim)
        assert torch.equal(got2_p, got_p) and (got_f is None or torch.equal(got2_f, got_f)), tag
        want2_p, _ = M.gather_model(g, sp, sf, n_store, Fdim, case["pts"], features, order, order2)
        assert np.array_equal(_np(got2_p), want2_p), tag


def test_fill_gather_features_default_to_zero(dev):
    """Rows whose source has no features (an old store without features, candidates offered without features) get 0."""
    from macarons_amd import ops
    case = C.fill_case(255, (3, 2, 3), True)
    tab, nk = case["tab"], 18
    features, feats = C.case_features(case, 3)
    sp, so, sf = C.flat(case["store"], feats)
    n_store = int(so[-1])
    for with_store_fts, with_features in ((False, True), (True, False)):
        fts = features if with_features else None
        h = _begin(ops, dev, tab, case["pts"], None, fts, sp, so, case["resolution"], 0)
        plan = C.gather_plan(_np(h.counts), so, case["capacity"], 0, np.random.default_rng(2))
        g = M.perm_row_map(plan["pm"], plan["tables"], nk, plan["n_new"], n_store)
        sfv = sf if with_store_fts else None
        got_p, got_f = ops.scene_fill_gather(_t(g, dev, torch.int64), h, _t(sp, dev), _t(sfv, dev), n_store, 3)
        want_p, want_f = M.gather_model(g, sp, sfv, n_store, 3, case["pts"], fts, _np(h.order), _np(h.order2))
        assert np.array_equal(_np(got_p), want_p) and np.array_equal(_np(got_f), want_f)
        assert (want_f == 0).all(1).any() and (want_f != 0).any()


# ---- Scene.fill_cells end to end ----------------------------------------------------------------------------------------------------
def _scene(dev, grid, capacity, feature_dim):
    from macarons_amd.utility.scene import Scene
    x_min, x_max = C.BOXES[tuple(grid)]
    return Scene(torch.tensor(x_min), torch.tensor(x_max), grid[0], grid[1], grid[2], capacity, C.RESOLUTION, 16, dev, feature_dim=feature_dim)


def _check_cells(sc, want, want_f, tag):
    for c, cell in enumerate(sc._cell_table()[0]):
        assert np.array_equal(_np(cell.cell_pts), want[c]), (tag, c)
        assert np.array_equal(_np(cell.cell_features), want_f[c]), (tag, c)


@pytest.mark.parametrize("grid", [(3, 2, 3), (4, 3, 5)])
def test_scene_fill_cells_three_fills(dev, grid):
    """Three successive Scene.fill_cells after torch.manual_seed == upstream's control flow with torch.randperm(n_comb)[:capacity] per
    touched cell in cell order after the same seed: every cell's points and features after each fill, and the CPU generator's state
    at the end.  Guarded inputs (fused path: the ambiguity counter is 0), then one fill of near-face points on top (upstream's way)."""
    tab = C.grid_tables(grid)
    nk = int(np.prod(grid))
    sc = _scene(dev, grid, C.E2E_CAPACITY, 2)
    _, lo, hi = sc._cell_table()
    assert np.array_equal(_np(lo), tab["lo"]) and np.array_equal(_np(hi), tab["hi"])
    fills = C.e2e_fills(tab)
    torch.manual_seed(C.E2E_SEED)
    got = []
    for k, (pts, features, valid) in enumerate(fills):
        h = sc.fill_cells_begin(_t(pts, dev), _t(features, dev), C.E2E_N_POINT_MIN, _t(valid, dev, torch.bool))
        n_amb = sc.fill_ambiguous(_np(h.counts))
        assert (n_amb == 0) == (k < 3) and n_amb == int(M.ambiguous(pts, valid, *_args(tab)).sum())
        sc.fill_cells(_t(pts, dev), _t(features, dev), C.E2E_N_POINT_MIN, None, _t(valid, dev, torch.bool))
        assert (sc._store is not None) == (k < 3)          # the fused path leaves the flat store, upstream's way the cells' own tensors
        got.append([(_np(c.cell_pts).copy(), _np(c.cell_features).copy()) for c in sc._cell_table()[0]])
    state = torch.get_rng_state()
    torch.manual_seed(C.E2E_SEED)
    stores, feats = [np.zeros((0, 3), F)] * nk, [np.zeros((0, 2), F)] * nk
    for k, (pts, features, valid) in enumerate(fills):
        stores, feats = M.fill_cells_upstream(stores, feats, pts, features, valid, *_args(tab), C.RESOLUTION, C.E2E_CAPACITY, C.E2E_N_POINT_MIN,
                                              lambda n: torch.randperm(n).numpy())
        for c in range(nk):
            assert np.array_equal(got[k][c][0], stores[c]) and np.array_equal(got[k][c][1], feats[c]), (k, c)
    assert torch.equal(state, torch.get_rng_state())


@pytest.mark.parametrize("grid", [(3, 2, 3), (4, 3, 5), (3, 3, 3)])
def test_scene_fill_cells_near_face_points(dev, grid):
    """One fill that contains near-face points equals upstream's cells (on a part-filled scene); the same call without the ambiguous
    points takes the fused path -- its counter is 0 -- and equals upstream too.  The counter is the model's count."""
    tab = C.grid_tables(grid)
    nk = int(np.prod(grid))
    first, near = C.near_face_scenario(tab)
    amb = M.ambiguous(near, None, *_args(tab))
    assert amb.sum() >= 100
    for pts, fused in ((near, False), (near[~amb], True)):
        sc = _scene(dev, grid, C.NEAR_CAPACITY, 1)
        torch.manual_seed(3)
        sc.fill_cells(_t(first, dev), _t(np.zeros((len(first), 1), F), dev))
        feat = np.arange(len(pts), dtype=F)[:, None]
        h = sc.fill_cells_begin(_t(pts, dev), _t(feat, dev))
        assert sc.fill_ambiguous(_np(h.counts)) == (0 if fused else int(amb.sum()))
        sc.fill_cells(_t(pts, dev), _t(feat, dev))
        assert (sc._store is not None) == fused
        state = torch.get_rng_state()
        torch.manual_seed(3)
        draw = lambda n: torch.randperm(n).numpy()
        stores, feats = M.fill_cells_upstream([np.zeros((0, 3), F)] * nk, [np.zeros((0, 1), F)] * nk, first, np.zeros((len(first), 1), F), None,
                                              *_args(tab), C.RESOLUTION, C.NEAR_CAPACITY, 0, draw)
        stores, feats = M.fill_cells_upstream(stores, feats, pts, feat, None, *_args(tab), C.RESOLUTION, C.NEAR_CAPACITY, 0, draw)
        assert torch.equal(state, torch.get_rng_state())
        _check_cells(sc, stores, feats, (grid, fused))


# ---- mcr_field_select ---------------------------------------------------------------------------------------------------------------
def _select_inputs(P, tab, Fdim, store_variant, rng):
    nk = int(np.prod(tab["grid"]))
    ext = (tab["x_max"] - tab["x_min"]).astype(np.float64)
    pp = (tab["x_min"] - 0.1 * ext + rng.random((P, 3)) * 1.2 * ext).astype(F)            # some proxy points outside the scene box (clamped)
    sup = rng.choice(np.array([0., 1., .5], F), P)
    oof = rng.choice(np.array([0., 1., .5], F), P)
    proba = rng.random(P).astype(F)
    if store_variant == "empty":
        return pp, sup, oof, proba, np.zeros((0, Fdim), F), np.zeros(nk + 1, np.int64)
    held = rng.permutation(P)[:max(1, (2 * P) // 3)]                                       # every index at most once
    idx = np.concatenate((held.astype(F), [-1., float(P), -1.]))                          # -1 and P: ignored
    cell = np.sort(rng.integers(0, nk, len(idx)))                                          # any cell: the store says where a point is kept
    fts = np.concatenate((idx[:, None], rng.standard_normal((len(idx), Fdim - 1)).astype(F)), 1).astype(F)
    off = np.concatenate(([0], np.cumsum(np.bincount(cell, minlength=nk)))).astype(np.int64)
    return pp, sup, oof, proba, fts, off


@pytest.mark.parametrize("P,grid", [(1, (1, 1, 1)), (7, (11, 3, 31)), (2049, (3, 2, 3)), (5000, (11, 3, 31))])
def test_field_select(dev, P, grid):
    """ops.field_select against the model: P below n_cells + 1 (7 points on 1023 cells) and across the 2048-row tile, F in {1, 3},
    use_mask 0 / 1, supervision and out-of-field values {0, 1, 0.5} (0.5 is in the field AND in the tail), an empty store, store
    features -1 and P (ignored), proxy points outside the scene box (clamped), and a pending fill: none, one with zero admissions,
    one whose admissions move stored points to other cells."""
    from macarons_amd import ops
    tab = C.grid_tables(grid)
    nk = int(np.prod(grid))
    gc = _gc(tab, dev)
    empty_off = np.zeros(nk + 1, np.int64)
    for Fdim in (1, 3):
        for store_variant in ("empty", "held"):
            rng = np.random.default_rng([P, Fdim, len(store_variant)])
            pp, sup, oof, proba, fts, off = _select_inputs(P, tab, Fdim, store_variant, rng)
            n_store = len(fts)
            feat_p = np.concatenate((np.arange(P, dtype=F)[:, None], rng.standard_normal((P, Fdim - 1)).astype(F)), 1)
            for pend in ("none", "zero", "moves"):
                pending = pend_m = None
                if pend != "none":
                    valid = np.zeros(P, bool) if pend == "zero" else rng.random(P) < 0.6
                    pending = _begin(ops, dev, tab, pp, valid, feat_p, np.zeros((0, 3), F), empty_off, C.RESOLUTION, 0)
                    bm = M.fill_begin_model(pp, valid, *_args(tab), None, empty_off, C.RESOLUTION, 0)
                    _check_begin(pending, bm, (P, grid, pend))
                    adm_off = bm["counts"][3 * nk + 4:4 * nk + 6]
                    assert (adm_off[nk] == 0) == (pend == "zero" or not M.in_box(pp, valid, tab["x_min"], tab["x_max"]).any())
                    pend_m = {"features": feat_p, "order": bm["order"], "order2": bm["order2"], "key2": bm["key2"], "adm_off": adm_off, "N": P}
                for use_mask in (0, 1):
                    tag = (P, grid, Fdim, store_variant, pend, use_mask)
                    want = M.field_select_model(pp, sup, oof, proba, fts, n_store, off, tab["x_min"], tab["step"], grid, use_mask, pend_m)
                    proba_d = _t(proba, dev)
                    s = ops.field_select(_t(pp, dev), _t(sup, dev), _t(oof, dev), proba_d, _t(fts, dev).view(n_store, Fdim), n_store,
                                         _t(off, dev, torch.int64), gc, grid, use_mask, pending)
                    assert np.array_equal(_np(s.stored_cell), want["stored_cell"]), tag
                    assert np.array_equal(_np(proba_d), want["proba"]), tag
                    assert np.array_equal(_np(s.counts), want["counts"]), tag
                    assert np.array_equal(_np(s.rows_order), want["rows_order"]), tag
                    assert np.array_equal(_np(s.oof_order), want["oof_order"]), tag
                    if pend == "moves" and store_variant == "held" and P > 100:
                        plain = M.field_select_model(pp, sup, oof, proba, fts, n_store, off, tab["x_min"], tab["step"], grid, use_mask, None)
                        moved = (plain["stored_cell"] >= 0) & (plain["stored_cell"] != want["stored_cell"])
                        assert moved.sum() > 10, tag                     # (the pending admissions did override stored cells)


# ---- mcr_field_build / mcr_field_finish ---------------------------------------------------------------------------------------------
def _neighbour_matrix(grid):
    g = np.array(grid)
    out = -np.ones((int(g.prod()), 27), np.int64)
    for c in range(int(g.prod())):
        i, j, k = c // (g[1] * g[2]), (c // g[2]) % g[1], c % g[2]
        nb = sorted({(min(max(i + a, 0), g[0] - 1) * g[1] + min(max(j + b, 0), g[1] - 1)) * g[2] + min(max(k + e, 0), g[2] - 1)
                     for a in (-1, 0, 1) for b in (-1, 0, 1) for e in (-1, 0, 1)})
        out[c, :len(nb)] = nb
    return out


def _job_tables(visit, counts, sel_off, s_off, nbm, chunk, k_for_knn):
    """The numpy branch of compute_scene_occupancy_probability_field, restated: (cell, chunk) jobs and their surface segments."""
    s_len, s_start = np.diff(s_off), s_off[:-1]
    nb_len = np.where(nbm >= 0, s_len[np.maximum(nbm, 0)], 0)
    m_cell = nb_len.sum(1)
    run = (visit != 0) & (m_cell > 2 * 2 * k_for_knn) & (counts > 0)
    cells_run = np.nonzero(run)[0]
    n_chunks = -(-counts[cells_run] // chunk)
    job_cell = np.repeat(cells_run, n_chunks)
    J = int(job_cell.size)
    lo = (np.arange(J) - np.repeat(np.cumsum(n_chunks) - n_chunks, n_chunks)) * chunk
    job_q = np.minimum(chunk, counts[job_cell] - lo).astype(np.int64)
    job_m = m_cell[job_cell].astype(np.int64)
    q_start, m_start = np.concatenate(([0], np.cumsum(job_q))), np.concatenate(([0], np.cumsum(job_m)))
    jt = np.stack((sel_off[job_cell] + lo, q_start[:-1], m_start[:-1], np.zeros(J, np.int64)), 1).astype(np.int64)
    seg_len = nb_len[job_cell]
    keep = seg_len > 0
    seg_l = seg_len[keep]
    st = np.stack((s_start[nbm[job_cell][keep]], np.cumsum(seg_l) - seg_l, np.nonzero(keep)[0], np.zeros(seg_l.size, np.int64)), 1).astype(np.int64)
    return jt, st, job_cell, int(q_start[-1]), int(m_start[-1]), n_chunks


class _Sel:
    rows_order = oof_order = None


# T -> ({cell: selected points}, chunk): one job of one row; a partly filled last block; 4097 rows -- the smallest T at which the
# 1024-block cap of the view-harmonics kernel gives a wave a second row -- with cell 0 split into three jobs by the chunk
BUILD_CASES = {1: ({4: 1}, 20000), 5: ({2: 3, 7: 2}, 20000), 4097: ({0: 1500, 5: 2000, 17: 597}, 600)}


@pytest.mark.parametrize("T", [1, 5, 4097])
def test_field_build(dev, T):
    """ops.field_build against the model: rows, row_job, X_world, X_q, pc_all and vh, for n_bins in {1, 13, 98, 128} with and without a
    bin permutation, random 0/1 view states; vh equals ops.view_harmonics_rows on the same rows.  Jobs with several surface segments;
    T = 4097 crosses the grid-stride loop of the view-harmonics kernel."""
    from macarons_amd import ops
    grid, nk = (3, 2, 3), 18
    sel_cells, chunk = BUILD_CASES[T]
    rng = np.random.default_rng(T)
    P = T + 300
    key = np.full(P, nk, np.int64)
    key[rng.permutation(P)[:T]] = np.repeat(list(sel_cells), list(sel_cells.values()))
    rows_order, counts, sel_off = M._group(key, nk)
    s_off = np.concatenate(([0], np.cumsum(rng.integers(0, 40, nk) * (rng.random(nk) < 0.7)))).astype(np.int64)
    S_all = rng.standard_normal((int(s_off[-1]), 3)).astype(F)
    pp = rng.standard_normal((P, 3)).astype(F)
    nbm = _neighbour_matrix(grid)
    jt, st, job_cell, T_, tot, n_chunks = _job_tables((counts[:nk] > 0).astype(np.int64), counts[:nk], sel_off, s_off, nbm, chunk, 1)
    J, n_seg = len(jt), len(st)
    assert T_ == T and tot > 0 and n_seg > J and (T != 4097 or (n_chunks[0] == 3 and J == 8)) and (T != 1 or J == 1)
    xf_all = rng.standard_normal((nk, 20)).astype(F)
    xf = xf_all[job_cell]
    from macarons_amd.utility import macarons_utils as mu                  # the product's planner: the same jobs, the same upload (below)
    surf = mu._SurfaceCells(None, s_off[:-1], np.diff(s_off), True, nbm)
    cells_run = np.nonzero((counts[:nk] > 0) & (surf.m_cell > 2 * 2 * 1))[0]
    sel = _Sel()
    sel.rows_order = _t(rows_order, dev, torch.int32)
    pp_d, S_d = _t(pp, dev), _t(S_all, dev)
    for n_bins in (1, 13, 98, 128):
        vs = (rng.random((P, n_bins)) < 0.3).astype(F)
        mt = rng.standard_normal((n_bins, 64)).astype(F)
        vs_d, mt_d = _t(vs, dev), _t(mt, dev)
        for perm in (None, rng.permutation(n_bins).astype(np.int32)):
            tag = (T, n_bins, perm is not None)
            raw = np.concatenate((jt.reshape(-1).view(np.uint8), st.reshape(-1).view(np.uint8), np.ascontiguousarray(xf).reshape(-1).view(np.uint8),
                                  (perm if perm is not None else np.zeros(0, np.int32)).view(np.uint8)))
            plan = mu._plan_jobs(cells_run, counts[:nk], sel_off, surf, nbm, xf_all, perm if perm is not None else np.zeros(0, np.int32), chunk)
            assert (plan.J, plan.n_seg, plan.T, plan.tot) == (J, n_seg, T, tot) and np.array_equal(plan.raw, raw), tag
            tables = _t(raw, dev, torch.uint8)
            perm_d = tables[32 * (J + n_seg) + 80 * J:].view(torch.int32) if perm is not None else None
            X_world = torch.full((T + 3, 3), -7., device=dev)
            vh = torch.full((T + 3, 64), -7., device=dev)
            rows, row_job, X_q, pc_all = ops.field_build(tables, J, n_seg, sel, pp_d, S_d, vs_d, perm_d, mt_d, T, tot, X_world, vh)
            want = M.field_build_model(jt, st, xf, rows_order, pp, S_all, vs, perm, mt, T, tot)
            for name, got in (("rows", rows), ("row_job", row_job), ("X_world", X_world[:T]), ("X_q", X_q), ("pc_all", pc_all), ("vh", vh[:T])):
                assert np.array_equal(_np(got), want[name]), (tag, name)
            assert (X_world[T:] == -7.).all() and (vh[T:] == -7.).all(), tag             # nothing past row T
            assert torch.equal(ops.view_harmonics_rows(vs_d, rows, perm_d, mt_d), vh[:T]), tag


def test_field_finish(dev):
    """ops.field_finish against the model: the scatter comes first and the tail reads the scattered probabilities (a point both
    selected and out of field carries the new value); T = 0, n_oof = 0, and both."""
    from macarons_amd import ops
    rng = np.random.default_rng(1)
    P = 3000
    pp = rng.standard_normal((P, 3)).astype(F)
    proba = rng.random(P).astype(F)
    perm = rng.permutation(P)
    rows_all, oof_all = perm[:700].astype(np.int32), np.sort(np.concatenate((perm[600:700], perm[700:1100]))).astype(np.int32)
    occ_all = (rng.random(700) + 2).astype(F)                                  # values the stored probabilities never take
    sel = _Sel()
    sel.oof_order = _t(np.concatenate((oof_all, np.setdiff1d(np.arange(P), oof_all))), dev, torch.int32)
    for T, n_oof in ((700, 500), (0, 500), (700, 0), (0, 0), (1, 1)):
        rows, occ = rows_all[:T], occ_all[:T]
        if (T, n_oof) == (1, 1):
            rows = oof_all[:1]                                                  # the one selected point is the one in the tail
        want_proba, want_X, want_occ = M.field_finish_model(rows, occ, T, proba, oof_all, n_oof, pp)
        proba_d = _t(proba, dev)
        X_tail, occ_tail = torch.full((n_oof + 2, 3), -7., device=dev), torch.full((n_oof + 2, 1), -7., device=dev)
        ops.field_finish(_t(rows, dev, torch.int32) if T else None, _t(occ, dev).view(-1, 1) if T else None, T, proba_d, sel, n_oof, _t(pp, dev),
                         X_tail, occ_tail)
        assert np.array_equal(_np(proba_d), want_proba), (T, n_oof)
        assert np.array_equal(_np(X_tail[:n_oof]), want_X) and np.array_equal(_np(occ_tail[:n_oof, 0]), want_occ), (T, n_oof)
        assert (X_tail[n_oof:] == -7.).all() and (occ_tail[n_oof:] == -7.).all()
        if T == 700 and n_oof:
            assert (want_occ >= 2).any() and (want_occ < 1).any()             # tail rows with the new value and with the stored one
        if (T, n_oof) == (1, 1):
            assert want_occ[0] == occ_all[0]                                    # selected and out of field: the tail carries the new value


# ---- the decision: a fill with ambiguous points is finished upstream's way before the selection ------------------------------------
class _PlainScene:
    """A Scene seen through the interface of a reference Scene: no fill_cells_begin, so macarons_nbv_decision takes its unfused route
    (fill_cells on the compacted frustum points, then the field pass on the final stores); the fill itself is upstream's loop."""

    def __init__(self, scene):
        object.__setattr__(self, "_scene", scene)

    def __getattr__(self, name):
        if name == "fill_cells_begin":
            raise AttributeError(name)
        return getattr(object.__getattribute__(self, "_scene"), name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_scene"), name, value)

    def fill_cells(self, pts, features=None, n_point_min=0):
        object.__getattribute__(self, "_scene").fill_cells_upstream(pts, features, n_point_min)


def test_decision_with_near_face_proxy_points_fills_upstream_way(dev, monkeypatch):
    """Decision 0 of the reference golden's scene with 300 proxy points of the frustum moved to within 2 ulp of a cell face: the fused
    decision sees a non-zero ambiguity count, finishes the fill upstream's way and selects from the final stores -- bit for bit the
    decision that fills upstream's way to begin with (cells, field, gains, choice, CPU generator)."""
    import test_macarons_regime_gpu as R
    from conftest import golden
    from types import SimpleNamespace as NS
    from macarons_amd.utility import macarons_utils as mu
    g = golden("macarons_decision")
    H, W = int(g["hw"][0]), int(g["hw"][1])
    n = len(g["proxy"])
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=16,
                prediction_neighborhood_size=3, n_view_state_cameras=98, sensor_range=40., min_occ_for_proxy_points=0.1, seq_len=2048,
                distance_factor_th=17., image_height=H, image_width=W, carving_tolerance=0.05)
    dmask = np.unpackbits(g["dmask"])[:2 * H * W].reshape(2, H, W).astype(bool)
    fov = np.nonzero(np.unpackbits(g["fov_mask_0"])[:n].astype(bool))[0]
    m = R._models(dev)

    def decide(plain):
        surface, proxy = R._decision_scenes(g, dev)
        _, lo, hi = proxy._cell_table()
        lo, hi = _np(lo), _np(hi)
        pts = g["proxy"].astype(F).copy()
        rng = np.random.default_rng(4)
        grid = [int(v) for v in g["grid"]]
        assert grid[0] > 1 or grid[2] > 1
        a = 0 if grid[0] > 1 else 2
        face = F(sorted({float(v) for v in lo[:, a]})[1])                      # the first interior face along that axis
        around = np.array([face, np.nextafter(face, F(-np.inf)), np.nextafter(face, F(np.inf)),
                           np.nextafter(np.nextafter(face, F(-np.inf)), F(-np.inf)), np.nextafter(np.nextafter(face, F(np.inf)), F(np.inf))], F)
        moved = rng.choice(fov, 300, replace=False)
        pts[moved, a] = around[rng.integers(0, 5, 300)]
        if abs(float(face)) < 1e-6:
            pts[moved[:60], a] = F(-1e-7)
        proxy.proxy_points = _t(pts, dev)
        calls = []
        inner = proxy.fill_cells_upstream
        monkeypatch.setattr(proxy, "fill_cells_upstream", lambda *a_, **k_: (calls.append(1), inner(*a_, **k_))[1])
        cam = mu.SceneCamera(mu.camera_record(g["Mview"][0], g["Mfull"][0], g["ndc"], g["eyes"][0], params.sensor_range).to(dev),
                             _t(g["eyes"][0:1], dev), float(g["zfar"]))
        nrec = torch.stack([mu.camera_record(g["nMview_0"][k], g["nMfull_0"][k], g["ndc"], g["n_eyes"][0, k], params.sensor_range)
                            for k in range(5)]).to(dev)
        torch.manual_seed(5100)
        with torch.no_grad():
            r = mu.macarons_nbv_decision(params, m, _PlainScene(proxy) if plain else proxy, surface, cam, _t(g["depth"][0], dev),
                                         _t(dmask[0], dev, torch.bool), nrec, _t(g["n_eyes"][0], dev), dev, samples=_t(g["u_0"], dev))
        assert len(calls) == 1                                                   # (fused: the ambiguity count sent the fill there)
        tab = {"lo": lo, "hi": hi, "x_min": _np(proxy.x_min).reshape(3), "x_max": _np(proxy.x_max).reshape(3),
               "step": _np(torch.stack((proxy.l, proxy.w, proxy.h))).reshape(3), "grid": tuple(grid)}
        assert M.ambiguous(pts, _np(r["fov_mask"]), *_args(tab)).sum() > 0
        cells = [(_np(c.cell_pts).copy(), _np(c.cell_features).copy()) for c in proxy._cell_table()[0]]
        return r, cells, torch.get_rng_state(), _np(proxy.proxy_proba).copy()

    (a, ca, sa, pa), (b, cb, sb, pb) = decide(False), decide(True)
    for k in ("fov_mask", "X_world", "view_harmonics", "occ_probs", "gains"):
        assert torch.equal(a[k], b[k]), k
    assert int(a["next_idx"]) == int(b["next_idx"]) and torch.equal(sa, sb) and np.array_equal(pa, pb)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(ca, cb)) and sum(len(x[0]) for x in ca) > 0
