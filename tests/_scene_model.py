"""Exact host model of the scene fill and field-pass entries of csrc/scene.hip (numpy only; TEST INFRASTRUCTURE).

Everything these entries do is integer / byte bookkeeping plus a few fp32 and fp64 operations in a fixed order, so the model is
bit-exact: tests compare with array_equal, never with a tolerance.  Two rules for Scene.fill_cells live side by side here:

  fill_cells_upstream    upstream's control flow (macarons_utils.py:2727-2737 over Cell.fill :2551-2577): every in-box point is offered
                         to EVERY englobing cell, each cell keeps the points strictly inside its box;
  fill_cells_floor_rule  what the fused path documents: a point goes to the cell the floor rule names, then passes that cell's strict
                         box test or is dropped.

They part exactly on the points `ambiguous` flags.  The grid's tables (lo, hi = Scene._cell_table(), x_min, x_max, step) are inputs.

PERTURB (a set of names, empty in every test) switches ONE documented mistake into the model: the sensitivity record of the suite --
which test notices which mistake -- is made by running the GPU tests with one name set (env SCENE_MODEL_PERTURB).  Names:
  admit_nonstrict   d >= resolution admits            first_empty_cell  first instead of last cell in the offset search
  tail_first        the tail read before the scatter  no_pending        pending admissions do not override stored_cell
  no_bin_perm       bin permutation dropped           oof_le            out_of_field <= 1 counts as in the field
"""
import os

import numpy as np

from oracle import macarons_regime as R
from oracle import scene as S

F = np.float32
PERTURB = set(os.environ.get("SCENE_MODEL_PERTURB", "").split())


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
def floor_cells(pts, x_min, step, grid):
    """Linear id of the cell upstream's floor rule names (utils.floor_divide on pts - x_min, capped at grid - 1, clamped at 0), fp32
    operation by operation like the torch expression."""
    pts, x_min, step = np.asarray(pts, F), np.asarray(x_min, F).reshape(1, 3), np.asarray(step, F).reshape(1, 3)
    d = pts - x_min
    q = (d - np.mod(d, step)) / step
    q = np.minimum(q, (np.asarray(grid) - 1).astype(F).reshape(1, 3))
    idx = np.trunc(q).astype(np.int64).clip(min=0)
    return (idx[:, 0] * grid[1] + idx[:, 1]) * grid[2] + idx[:, 2]


def in_box(pts, valid, x_min, x_max):
    """Closed scene-box mask (get_pts_in_bounding_box :2676-2691) of the offered points."""
    pts = np.asarray(pts, F)
    m = ((pts >= np.asarray(x_min, F).reshape(1, 3)) & (pts <= np.asarray(x_max, F).reshape(1, 3))).all(-1)
    return m if valid is None else m & np.asarray(valid).astype(bool)


def strictly_inside(pts, lo_c, hi_c):
    """Cell.fill's two masks (:2552, :2558) for one cell: fp32 differences against 0."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    return ((pts - np.asarray(hi_c, F).reshape(1, 3)).max(-1) < 0.) & ((pts - np.asarray(lo_c, F).reshape(1, 3)).min(-1) > 0.)


def ambiguous(pts, valid, lo, hi, x_min, x_max, step, grid):
    """bool [N]: offered in-box points that some cell OTHER than their floor cell strictly contains (every cell is tried)."""
    pts = np.asarray(pts, F)
    fc = floor_cells(pts, x_min, step, grid)
    amb = np.zeros(len(pts), bool)
    for c in range(len(lo)):
        amb |= strictly_inside(pts, lo[c], hi[c]) & (fc != c)
    return amb & in_box(pts, valid, x_min, x_max)


# ---- Scene.fill_cells, two rules ----------------------------------------------------------------------------------------------------
def _draw(perms):
    if callable(perms):
        return perms
    it = iter(perms)
    return lambda n: np.asarray(next(it))


def _cell_update(store, feat, add, addf, lo_c, hi_c, offered, resolution, capacity, n_point_min, draw):
    """One Cell.fill whose strictly-inside points are `add` (features `addf`); `offered` = what the cell was handed.  The points go
    through oracle.macarons_regime.cell_fill (pinned to the reference); the features ride the same rows."""
    if len(add) <= n_point_min:                            # (0 candidates included: Cell.fill returns before its draw)
        return store, feat
    if len(store):
        keep = S.min_dist(add, store) > resolution
        add, addf = add[keep], (addf[keep] if addf is not None else None)
    perm = np.asarray(draw(len(store) + len(add)), np.int64)
    new = R.cell_fill(store, offered, lo_c, hi_c, resolution, capacity, perm, n_point_min)
    assert np.array_equal(new, np.vstack((store, add))[perm[:capacity]])
    if feat is not None:
        feat = np.vstack((feat, addf if addf is not None else np.zeros((len(add), feat.shape[1]), F)))[perm[:capacity]]
    return new, feat


def _fill_inputs(stores, feats, pts, features, valid, x_min, x_max):
    pts = np.asarray(pts, F)
    m = in_box(pts, valid, x_min, x_max)
    stores = [np.asarray(s_, F).reshape(-1, 3) for s_ in stores]
    feats = None if feats is None else [np.asarray(f_, F) for f_ in feats]
    fin = None if (features is None or feats is None) else np.asarray(features, F).reshape(len(pts), -1)[m]
    return stores, feats, pts[m], fin


def fill_cells_upstream(stores, feats, pts, features, valid, lo, hi, x_min, x_max, step, grid, resolution, capacity, n_point_min, perms):
    """Upstream's Scene.fill_cells.  stores / feats: per cell (linear order) [n,3] / [n,F] (feats None: no features); perms: one
    permutation per touched cell in cell order, or a callable n -> permutation.  -> (stores, feats) after the fill."""
    stores, feats, inside, fin = _fill_inputs(stores, feats, pts, features, valid, x_min, x_max)
    draw = _draw(perms)
    for c in np.unique(floor_cells(inside, x_min, step, grid)).tolist():     # the englobing cells, lexicographic = linear order
        m = strictly_inside(inside, lo[c], hi[c])
        stores[c], f_ = _cell_update(stores[c], feats[c] if feats is not None else None, inside[m], fin[m] if fin is not None else None,
                                     lo[c], hi[c], inside, resolution, capacity, n_point_min, draw)
        if feats is not None:
            feats[c] = f_
    return stores, feats


def fill_cells_floor_rule(stores, feats, pts, features, valid, lo, hi, x_min, x_max, step, grid, resolution, capacity, n_point_min, perms):
    """The fused path's documented rule: the floor cell of a point, then that cell's strict box test."""
    stores, feats, inside, fin = _fill_inputs(stores, feats, pts, features, valid, x_min, x_max)
    draw = _draw(perms)
    fc = floor_cells(inside, x_min, step, grid)
    for c in np.unique(fc).tolist():
        m = (fc == c) & strictly_inside(inside, lo[c], hi[c])
        stores[c], f_ = _cell_update(stores[c], feats[c] if feats is not None else None, inside[m], fin[m] if fin is not None else None,
                                     lo[c], hi[c], inside[fc == c], resolution, capacity, n_point_min, draw)
        if feats is not None:
            feats[c] = f_
    return stores, feats


# ---- mcr_scene_fill_begin -----------------------------------------------------------------------------------------------------------
def _group(key, nk):
    """Stable grouping by key in 0 .. nk: (order, counts [nk+1], offsets [nk+2])."""
    key = np.asarray(key, np.int64)
    order = np.argsort(key, kind="stable")
    counts = np.bincount(key, minlength=nk + 1).astype(np.int64)
    return order.astype(np.int32), counts, np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def fill_begin_model(pts, valid, lo, hi, x_min, x_max, step, grid, store_pts, store_off, resolution, n_point_min):
    """What mcr_scene_fill_begin leaves behind: dict(key, order, key2 (sorted position), order2, counts = cand [nk+1] | a_off [nk+2] |
    adm [nk+1] | adm_off [nk+2] | n_ambiguous [1], dmin, dmin_rows).  The kernel never writes dmin for the rows of the rejected group
    nk: dmin_rows (bool, sorted position) marks the rows to compare."""
    pts = np.asarray(pts, F)
    nk = int(grid[0] * grid[1] * grid[2])
    fc = floor_cells(pts, x_min, step, grid)
    ok = in_box(pts, valid, x_min, x_max)
    for c in np.unique(fc[ok]).tolist():
        m = ok & (fc == c)
        ok[m] = strictly_inside(pts[m], lo[c], hi[c])
    key = np.where(ok, fc, nk).astype(np.int32)
    order, cand, a_off = _group(key, nk)
    key_s = key[order].astype(np.int64)
    dmin = np.full(len(pts), np.nan)
    store_pts = np.zeros((0, 3), F) if store_pts is None else np.asarray(store_pts, F)
    for c in range(nk):
        if cand[c]:
            rows = slice(int(a_off[c]), int(a_off[c + 1]))
            dmin[rows] = S.min_dist(pts[order[rows]], store_pts[int(store_off[c]):int(store_off[c + 1])])
    with np.errstate(invalid="ignore"):
        far = (dmin >= resolution) if "admit_nonstrict" in PERTURB else (dmin > resolution)
    key2 = np.where((key_s < nk) & (cand[np.minimum(key_s, nk)] > n_point_min) & far, key_s, nk).astype(np.int32)
    order2, adm, adm_off = _group(key2, nk)
    n_amb = int(ambiguous(pts, valid, lo, hi, x_min, x_max, step, grid).sum())
    return {"key": key, "order": order, "key2": key2, "order2": order2, "dmin": dmin, "dmin_rows": key_s < nk,
            "counts": np.concatenate((cand, a_off, adm, adm_off, [n_amb])).astype(np.int64)}


# ---- the two gathers ----------------------------------------------------------------------------------------------------------------
def _take(src_rows, store_pts, store_fts, n_store, Fdim, pts, features, order, order2):
    """Rows of the virtual table [old store | admitted candidates in cell order]; features are 0 where the source has none."""
    src_rows = np.asarray(src_rows, np.int64)
    out_p = np.empty((len(src_rows), 3), F)
    out_f = np.zeros((len(src_rows), Fdim), F) if Fdim else None
    old = src_rows < n_store
    if old.any():
        out_p[old] = np.asarray(store_pts, F)[src_rows[old]]
        if Fdim and store_fts is not None:
            out_f[old] = np.asarray(store_fts, F)[src_rows[old]]
    if (~old).any():
        src = np.asarray(order, np.int64)[np.asarray(order2, np.int64)[src_rows[~old] - n_store]]
        out_p[~old] = np.asarray(pts, F)[src]
        if Fdim and features is not None:
            out_f[~old] = np.asarray(features, F).reshape(len(pts), Fdim)[src]
    return out_p, out_f


def gather_model(g, store_pts, store_fts, n_store, Fdim, pts, features, order, order2):
    """fill_gather_kernel: new row r = row g[r] of [old store | admitted candidates in cell order]."""
    return _take(g, store_pts, store_fts, n_store, Fdim, pts, features, order, order2)


def perm_row_map(pm, tables, n_cells, n_new, n_store):
    """The row map fill_gather_pm_kernel evaluates: tables = new_off | b_off | adm_off | pm_off | touched (n_cells + 1 each); new row r
    belongs to the LAST cell with new_off[c] <= r (empty cells share an offset); its source is row pm[pm_off[c] + local] of the cell's
    [stored | admitted] rows when the cell was touched, else its local-th stored row.  -> g for gather_model."""
    n1 = n_cells + 1
    t = np.asarray(tables, np.int64)
    new_off, b_off, adm_off, pm_off, touched = (t[k * n1:(k + 1) * n1] for k in range(5))
    r = np.arange(n_new, dtype=np.int64)
    c = np.clip(np.searchsorted(new_off[:n_cells], r, side="right") - 1, 0, n_cells - 1)
    if "first_empty_cell" in PERTURB:
        c = np.searchsorted(new_off[:n_cells], new_off[c], side="left")
    local = r - new_off[c]
    pm = np.asarray(pm, np.int64)
    val = np.where(touched[c] != 0, pm[np.where(touched[c] != 0, pm_off[c] + local, 0)] if len(pm) else 0, local)
    b_len = b_off[c + 1] - b_off[c]
    return np.where(val < b_len, b_off[c] + val, n_store + adm_off[c] + (val - b_len))


def gather_perm_model(pm, tables, n_cells, n_new, store_pts, store_fts, n_store, Fdim, pts, features, order, order2):
    """fill_gather_pm_kernel: gather_model over perm_row_map."""
    return _take(perm_row_map(pm, tables, n_cells, n_new, n_store), store_pts, store_fts, n_store, Fdim, pts, features, order, order2)


# ---- mcr_field_select ---------------------------------------------------------------------------------------------------------------
def field_select_model(proxy_points, sup_occ, oof, proba, store_fts, n_store, store_off, x_min, step, grid, use_mask, pending=None):
    """What mcr_field_select leaves behind (constants: ops.FieldSelection, include/macarons_hip.h).  pending: None or dict(features,
    order, order2, key2, adm_off, N) of a fill whose gather has not run.  -> dict(stored_cell, proba, rows_order, oof_order, counts =
    visit [nk+1] | sel_counts [nk+1] | sel_off [nk+2] | oof_counts [2] | oof_off [3])."""
    pp = np.asarray(proxy_points, F)
    P, nk = len(pp), int(grid[0] * grid[1] * grid[2])
    sup_occ, oof, proba = np.asarray(sup_occ, F), np.asarray(oof, F), np.asarray(proba, F).copy()
    stored_cell = np.full(P, -1, np.int32)
    if n_store:
        p = np.trunc(np.asarray(store_fts, F).reshape(n_store, -1)[:, 0]).astype(np.int64)   # (long long) of a float: truncation
        r = np.arange(n_store)
        ok = (p >= 0) & (p < P)
        stored_cell[p[ok]] = (np.searchsorted(np.asarray(store_off, np.int64)[:nk + 1], r, side="right") - 1)[ok]
    if pending is not None and "no_pending" not in PERTURB:
        n_adm = min(int(pending["N"]), int(pending["adm_off"][nk]))
        pos = np.asarray(pending["order2"], np.int64)[:n_adm]
        feat = np.asarray(pending["features"], F).reshape(int(pending["N"]), -1)
        p = np.trunc(feat[np.asarray(pending["order"], np.int64)[pos], 0]).astype(np.int64)
        ok = (p >= 0) & (p < P)
        stored_cell[p[ok]] = np.asarray(pending["key2"])[pos][ok]
    occ = sup_occ > 0
    in_field = (oof <= 1) if "oof_le" in PERTURB else (oof < 1)
    seen = occ & in_field
    proba[seen] = 0
    visit = np.zeros(nk + 1, np.int64)
    visit[floor_cells(pp, x_min, step, grid)[seen if use_mask else in_field]] = 1
    key_sel = np.where((stored_cell >= 0) & (occ if use_mask else True), stored_cell, nk)
    key_oof = np.where(oof > 0, 0, 1)
    rows_order, sel_counts, sel_off = _group(key_sel, nk)
    oof_order, oof_counts, oof_off = _group(key_oof, 1)
    return {"stored_cell": stored_cell, "proba": proba, "rows_order": rows_order, "oof_order": oof_order,
            "counts": np.concatenate((visit, sel_counts, sel_off, oof_counts, oof_off)).astype(np.int64)}


# ---- mcr_field_build / mcr_field_finish ---------------------------------------------------------------------------------------------
def to_prediction_space(src, xf):
    """((((x m0 + y m4) + z m8) + m12) - c) inv per output column, fp32 operation by operation (the file is built without fma)."""
    src, xf = np.asarray(src, F), np.asarray(xf, F)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    return np.stack([((((x * xf[:, k] + y * xf[:, 4 + k]) + z * xf[:, 8 + k]) + xf[:, 12 + k]) - xf[:, 16 + k]) * xf[:, 19]
                     for k in range(3)], 1).astype(F)


def view_harmonics_model(view_states, rows, bin_perm, mt):
    """vh[t, k] = sum over v = 0 .. n_bins-1 of view_states[rows[t], bin_perm[v]] * mt[v, k]: one multiply, then one add, in fp32."""
    vs = np.asarray(view_states, F)[np.asarray(rows, np.int64)]
    if bin_perm is not None and "no_bin_perm" not in PERTURB:
        vs = vs[:, np.asarray(bin_perm, np.int64)]
    mt = np.asarray(mt, F)
    acc = np.zeros((len(vs), mt.shape[1]), F)
    for v in range(vs.shape[1]):
        acc = acc + vs[:, v:v + 1] * mt[v:v + 1]
    return acc


def field_build_model(jobs, segs, xf, rows_order, proxy_points, S_all, view_states, bin_perm, mt, T, tot):
    """mcr_field_build: jobs [J,4] = first position in rows_order, first query row, first cloud row, -; segs [n_seg,4] = first row in
    S_all, first cloud row, job, -; xf [J,20].  -> dict(rows, row_job, X_world, X_q, vh, pc_all)."""
    jobs, segs, xf = np.asarray(jobs, np.int64), np.asarray(segs, np.int64), np.asarray(xf, F)
    t = np.arange(T, dtype=np.int64)
    job = np.searchsorted(jobs[:, 1], t, side="right") - 1                # the last job whose first query row is <= t
    rows = np.asarray(rows_order, np.int64)[jobs[job, 0] + (t - jobs[job, 1])]
    pp = np.asarray(proxy_points, F)
    i = np.arange(tot, dtype=np.int64)
    seg = np.searchsorted(segs[:, 1], i, side="right") - 1
    src = segs[seg, 0] + (i - segs[seg, 1])
    return {"rows": rows.astype(np.int32), "row_job": job.astype(np.int32), "X_world": pp[rows], "X_q": to_prediction_space(pp[rows], xf[job]),
            "vh": view_harmonics_model(view_states, rows, bin_perm, mt), "pc_all": to_prediction_space(np.asarray(S_all, F)[src], xf[segs[seg, 2]])}


def field_finish_model(rows, occ, T, proba, oof_order, n_oof, proxy_points):
    """mcr_field_finish: the scatter proba[rows[t]] = occ[t] FIRST, then the tail reads the scattered proba.  -> (proba, X_tail, occ_tail)."""
    proba = np.asarray(proba, F).copy()
    tail = np.asarray(oof_order, np.int64)[:n_oof]
    before = proba[tail].copy()
    if T:
        proba[np.asarray(rows, np.int64)[:T]] = np.asarray(occ, F).reshape(-1)[:T]
    occ_tail = before if "tail_first" in PERTURB else proba[tail]
    return proba, np.asarray(proxy_points, F)[tail], occ_tail
