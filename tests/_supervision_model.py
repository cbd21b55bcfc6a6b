"""Exact host model of the occupancy supervision pass's selection, walk and scatter (numpy only; TEST INFRASTRUCTURE).

Restates compute_occupancy_probability_for_supervision's bookkeeping (upstream macarons_utils.py:1233-1392) -- everything except the
network -- as integer operations on plain arrays, so tests compare with array_equal:
  sample_mask   the sampled points' mask from the mask's ascending indices and the sampling permutation (:1259-1278)
  select_model  mcr_supervision_select: englobing cells by the floor rule, every cell's sampled store indices (ascending, each once),
                the counts table and pos
  walk_model    the cells that run, in visiting order, with their query lists (:1308-1373), and the number of dummy passes
  scatter_model / scatter_backward_model   mcr_supervision_scatter and its backward, fp32 additions in job order
"""
import numpy as np

from _scene_model import floor_cells

F = np.float32


def sample_mask(proxy_mask, sample_perm, n_sup):
    idx = np.nonzero(np.asarray(proxy_mask).reshape(-1))[0]
    out = np.zeros(np.asarray(proxy_mask).size, bool)
    out[idx[np.asarray(sample_perm, np.int64)[:n_sup]]] = True
    return out


def select_model(mask, proxy_points, x_min, step, grid, store_fts, store_off):
    """-> (englobing [n] uint8, per-cell index lists, counts int64 [3n+5], rows_order int32, pos int32 [P])."""
    mask = np.asarray(mask).reshape(-1).astype(bool)
    P, n = mask.size, int(grid[0] * grid[1] * grid[2])
    eng = np.zeros(n, np.int64)
    if mask.any():
        eng[floor_cells(np.asarray(proxy_points, F)[mask], x_min, step, grid)] = 1
    col0 = np.asarray(store_fts, F).reshape(len(store_fts), -1)[:, 0] if len(store_fts) else np.zeros(0, F)
    lists = []
    for c in range(n):
        p = np.trunc(col0[int(store_off[c]):int(store_off[c + 1])]).astype(np.int64)
        p = p[(p >= 0) & (p < P)]
        lists.append(np.unique(p[mask[p]]).astype(np.int32))
    cnt = np.array([len(l_) for l_ in lists] + [0], np.int64)
    off = np.concatenate(([0], np.cumsum(cnt)))
    counts = np.concatenate((eng, [0], cnt, off, [int(mask.sum())])).astype(np.int64)
    rows_order = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
    pos = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32)
    return eng.astype(np.uint8), lists, counts, rows_order, pos


def neighbourhood_sizes(surface_lens, grid):
    """Surface points in every cell's clamped, de-duplicated 27-neighbourhood (get_neighboring_cells + get_pt_cloud_from_cells)."""
    gl, gw, gh = (int(v) for v in grid)
    out = np.zeros(gl * gw * gh, np.int64)
    for c in range(gl * gw * gh):
        i, j, k = c // (gw * gh), (c // gh) % gw, c % gh
        nb = {(min(max(i + a, 0), gl - 1) * gw + min(max(j + b, 0), gw - 1)) * gh + min(max(k + d, 0), gh - 1)
              for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1)}
        out[c] = sum(int(surface_lens[v]) for v in nb)
    return out


def walk_model(englobing, lists, cell_perm, m_cell, cap, k):
    """-> (visited cells in order, their query lists, number of dummy passes): walk the permuted candidates until `cap` cells ran; a
    cell runs with more than 4k surface points around it and at least one query."""
    cand = np.nonzero(np.asarray(englobing))[0]
    visited = []
    for c in cand[np.asarray(cell_perm, np.int64)]:
        if len(visited) >= cap:
            break
        if m_cell[c] > 4 * k and len(lists[c]) > 0:
            visited.append(int(c))
    n_pass = len(visited)
    n_dummy = 0
    while n_pass < cap:
        n_dummy, n_pass = n_dummy + 1, n_pass + 1
    return visited, [lists[c] for c in visited], n_dummy


def scatter_model(rows, occ, job_offsets, J, pos, n_out):
    out = np.zeros(n_out, F)
    for j in range(J):
        for t in range(int(job_offsets[j]), int(job_offsets[j + 1])):
            i = pos[rows[t]]
            if 0 <= i < n_out:
                out[i] = F(out[i] + F(occ[t]))
    return out


def scatter_backward_model(rows, pos, d_out, T_scatter, T):
    d = np.zeros(T, F)
    for t in range(T_scatter):
        i = pos[rows[t]]
        if 0 <= i < len(d_out):
            d[t] = d_out[i]
    return d
