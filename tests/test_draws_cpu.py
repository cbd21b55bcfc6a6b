"""The batched hidden draws (csrc_torch/macarons_torch.cpp: randperm_prefixes, scone_occ_draws) make the reference's torch.randperm
calls -- same values, same generator state afterwards -- and lay the indices out as SconeOcc.forward_ragged / Scene.fill_cells need."""
import contextlib
import importlib
import io

import numpy as np
import torch


def test_randperm_prefixes_is_the_loop_of_torch_randperm():
    import macarons_amd.torch_ops  # noqa: F401
    for seed, spec in ((9, ((10, 4), (5000, 100000), (7, 7), (1, 1), (20000, 1000))), (1, ((3, 0), (2, 5)))):
        torch.manual_seed(seed)
        want = torch.cat([torch.randperm(n)[:k] for n, k in spec])
        after = torch.randperm(11)
        torch.manual_seed(seed)
        got = torch.ops.macarons.randperm_prefixes([n for n, _ in spec], [k for _, k in spec])
        assert torch.equal(got, want) and torch.equal(torch.randperm(11), after)


def _restated_index_arrays(perms, sizes, Lg):
    """The index arrays of a ragged pass from its jobs' draws, job by job: the frozen statement scone_occ_draws and the product's numpy
    builder (SconeOcc.ragged_index_arrays) are compared with.  A cloud shorter than Lg pads its global rows with its first point."""
    J = len(sizes)
    off0 = np.concatenate(([0], np.cumsum(sizes)))
    g_idx, g_len, idx1, idx2, off1, off2 = np.zeros((J, Lg), np.int64), np.zeros(J, np.int64), [], [], [0], [0]
    for j, (p0, p1, p2) in enumerate(perms):
        p0, p1, p2 = np.asarray(p0), np.asarray(p1), np.asarray(p2)
        n0 = min(len(p0), Lg)
        g_idx[j, :n0] = off0[j] + p0[:n0]; g_idx[j, n0:] = off0[j]; g_len[j] = n0
        idx1.append(off0[j] + p1); idx2.append(off1[-1] + p2)
        off1.append(off1[-1] + len(p1)); off2.append(off2[-1] + len(p2))
    return np.concatenate([g_idx.reshape(-1), np.concatenate(idx1), np.concatenate(idx2), off1, off2, g_len])


def test_scone_occ_draws_are_draw_perms_job_by_job():
    import macarons_amd.torch_ops  # noqa: F401
    M = importlib.import_module("macarons_amd.networks.SconeOcc")
    with contextlib.redirect_stdout(io.StringIO()):
        occ = M.SconeOcc()
    sizes = [700, 2300, 130, 5000, 1024, 27000, 65, 2048, 2049]
    sz = [occ.scale_sizes(m) for m in sizes]
    J, Lg = len(sizes), occ.seq_len
    torch.manual_seed(3)
    perms = [occ.draw_perms(m) for m in sizes]                     # SconeOcc.py:269, :311 -- three torch.randperm per forward
    after = torch.randperm(5)
    for j, (_, p1, p2) in enumerate(perms):
        assert len(p1) == sz[j][1] and len(p2) == sz[j][2]
    want = _restated_index_arrays(perms, sizes, Lg)
    torch.manual_seed(3)
    got = torch.ops.macarons.scone_occ_draws([s[0] for s in sz], [s[1] for s in sz], [s[2] for s in sz], Lg)
    assert np.array_equal(got.numpy(), want) and torch.equal(torch.randperm(5), after)
    # the product's numpy builder, handed the same draws, lays them out as the extension does
    built = M.ragged_index_arrays(perms, np.concatenate(([0], np.cumsum(sizes))).astype(np.int64), J, Lg)
    assert built.dtype == np.int64 and np.array_equal(built, got.numpy())


def test_ragged_index_arrays_equal_the_restatement():
    """SconeOcc.ragged_index_arrays (numpy; what forward_ragged uploads when the draws are given) == the job-by-job restatement, on
    random draws of random job lists: clouds shorter than seq_len (padding rows of the global down-sample), of exactly seq_len, and
    longer; one job and many.  No device, no extension."""
    M = importlib.import_module("macarons_amd.networks.SconeOcc")
    with contextlib.redirect_stdout(io.StringIO()):
        occ = M.SconeOcc()
    Lg = occ.seq_len
    rng = np.random.default_rng(11)
    torch.manual_seed(11)
    n_short = n_long = 0
    for trial in range(30):
        J = int(rng.integers(1, 9))
        sizes = [int(m) for m in rng.choice([65, 130, 700, 1024, Lg - 1, Lg, Lg + 1, 2300, 5000], J)]
        perms = [occ.draw_perms(m) for m in sizes]
        off0 = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        got = M.ragged_index_arrays(perms, off0, J, Lg)
        assert got.dtype == np.int64 and np.array_equal(got, _restated_index_arrays(perms, sizes, Lg)), trial
        g_len = got[-J:]
        assert g_len.tolist() == [min(m, Lg) for m in sizes]
        n_short += sum(m < Lg for m in sizes)
        n_long += sum(m > Lg for m in sizes)
    assert n_short > 20 and n_long > 20


def test_native_bin_permutation_equals_the_python_restatement():
    """torch.ops.macarons.view_space_bins (C++: the same ATen operators in the same order, one dispatcher call) returns the bins of
    scone_utils.view_space_bin_indices for random and for axis-aligned rotations (directions on bin boundaries)."""
    import torch
    from macarons_amd.utility import scone_utils as su
    if not su._native_bins():
        import pytest
        pytest.skip("C++ extension not built")
    torch.manual_seed(5)
    for n_elev, n_azim in ((7, 14), (5, 10)):
        for i in range(300):
            R = torch.linalg.qr(torch.randn(3, 3))[0].float()
            if i % 5 == 0:
                R = torch.eye(3)[torch.randperm(3)] * torch.tensor([1., -1., 1.])[torch.randperm(3)]
            a = su.view_space_bin_permutation(R, n_elev, n_azim, "cpu")
            x_ref = su._REF_DIRECTIONS[(n_elev, n_azim)]
            b = su.view_space_bin_indices((x_ref @ R.view(3, 3).T).reshape(-1, 3), n_elev, n_azim)
            assert torch.equal(a, b), (n_elev, n_azim, i)


# ---- the (cell, chunk) job tables of the occupancy passes: extension == product planner == the restatement below ------------------
def _random_job_grids():
    """The 40 random grids of the job-table tests: empty cells, cells that do not run (too few surface points, no queries, never
    visited), several chunks per cell."""
    rng = np.random.default_rng(3)
    for trial in range(40):
        n_cells = int(rng.integers(1, 80))
        chunk = int(rng.choice([7, 50, 20000]))
        k = int(rng.choice([1, 16]))
        visit = (rng.random(n_cells) < 0.7).astype(np.int64)
        counts = (rng.integers(0, 300, n_cells) * (rng.random(n_cells) < 0.8)).astype(np.int64)
        sel_off = np.concatenate(([0], np.cumsum(counts), [counts.sum()])).astype(np.int64)        # n_cells + 2 entries
        n_oof = int(rng.integers(0, 50))
        hostc = np.concatenate((visit, [0], counts, [0], sel_off, [n_oof])).astype(np.int64)
        s_len = (rng.integers(0, 400, n_cells) * (rng.random(n_cells) < 0.7)).astype(np.int64)
        s_off = np.concatenate(([0], np.cumsum(s_len))).astype(np.int64)
        nbm = np.full((n_cells, 27), -1, np.int64)
        for c in range(n_cells):
            nb = np.unique(rng.integers(0, n_cells, int(rng.integers(1, 28))))
            nbm[c, :nb.size] = nb
        xf_all = rng.standard_normal((n_cells, 20)).astype(np.float32)
        perm = rng.permutation(98).astype(np.int32)
        yield dict(trial=trial, n_cells=n_cells, chunk=chunk, k=k, visit=visit, counts=counts, sel_off=sel_off, n_oof=n_oof, hostc=hostc,
                   s_len=s_len, s_off=s_off, s_start=s_off[:-1], nbm=nbm, xf_all=xf_all, perm=perm)


def _restated_job_tables(visit, counts, sel_off, s_start, s_len, nbm, xf_all, perm, chunk, k, cells_run=None, tail=False):
    """The numpy code of the occupancy passes as it stood before macarons_utils._plan_jobs existed, restated: the frozen statement the
    product planner and the extension are compared with.  cells_run: the supervision pass's own list (visiting order, cut by its cap)
    instead of the field pass's visited cells in ascending order; tail: the supervision pass's upload (pad to 8 bytes, then q_start)."""
    nb_len = np.where(nbm >= 0, s_len[np.maximum(nbm, 0)], 0)
    m_cell = nb_len.sum(1)
    if cells_run is None:
        run = (visit != 0) & (m_cell > 2 * 2 * k) & (counts > 0)
        cells_run = np.nonzero(run)[0]
    n_chunks = -(-counts[cells_run] // chunk)
    job_cell = np.repeat(cells_run, n_chunks)
    J = int(job_cell.size)
    lo = (np.arange(J) - np.repeat(np.cumsum(n_chunks) - n_chunks, n_chunks)) * chunk
    job_q = np.minimum(chunk, counts[job_cell] - lo).astype(np.int64)
    job_m = m_cell[job_cell].astype(np.int64)
    q_start = np.concatenate(([0], np.cumsum(job_q))).astype(np.int64)
    m_start = np.concatenate(([0], np.cumsum(job_m))).astype(np.int64)
    jt = np.stack((sel_off[job_cell] + lo, q_start[:-1], m_start[:-1], np.zeros(J, np.int64)), 1).astype(np.int64) if J else np.zeros((0, 4), np.int64)
    seg_len = nb_len[job_cell]
    keep = seg_len > 0
    seg_l = seg_len[keep]
    st_ = np.stack((s_start[nbm[job_cell][keep]], np.cumsum(seg_l) - seg_l, np.nonzero(keep)[0], np.zeros(seg_l.size, np.int64)), 1).astype(np.int64)
    raw = np.concatenate((jt.reshape(-1).view(np.uint8), st_.reshape(-1).view(np.uint8),
                          np.ascontiguousarray(xf_all[job_cell]).reshape(-1).view(np.uint8), perm.view(np.uint8)))
    if tail:
        pad = (-raw.size) % 8
        raw = np.concatenate((raw, np.zeros(pad, np.uint8), q_start.astype(np.int64).view(np.uint8)))
    return dict(raw=raw, J=J, n_seg=int(st_.shape[0]), T=int(q_start[-1]), tot=int(m_start[-1]), job_cell=job_cell, job_q=job_q, job_m=job_m,
                q_start=q_start, m_start=m_start, m_cell=m_cell)


def _assert_plan_is(plan, want, tag):
    """The product's plan holds the restatement's tables, element for element; without a job there is nothing to upload."""
    assert (plan.J, plan.n_seg, plan.T, plan.tot) == (want["J"], want["n_seg"], want["T"], want["tot"]), tag
    for name in ("job_q", "job_m", "q_start", "m_start"):
        got = getattr(plan, name)
        assert got.dtype == np.int64 and np.array_equal(got, want[name]), (tag, name)
    if want["J"] == 0:
        assert plan.raw is None and (plan.T, plan.tot) == (0, 0), tag
    else:
        raw = plan.raw.numpy() if torch.is_tensor(plan.raw) else plan.raw
        assert raw.dtype == np.uint8 and np.array_equal(raw, want["raw"]), tag
        if plan.job_cell is not None:
            assert np.array_equal(plan.job_cell, want["job_cell"]), tag


def _plan_of(mu, g, cells_run, s_start=None, s_len=None, tail=False):
    surf = mu._SurfaceCells(None, g["s_start"] if s_start is None else s_start, g["s_len"] if s_len is None else s_len, True, g["nbm"])
    return mu._plan_jobs(cells_run, g["counts"], g["sel_off"], surf, g["nbm"], g["xf_all"], g["perm"], g["chunk"], tail=tail)


def test_plan_jobs_equals_the_restatement():
    """macarons_utils._plan_jobs -- the one planner of the field pass and of the supervision pass -- builds the restatement's tables
    (raw, J, n_seg, T, tot, job_q, job_m, q_start, m_start) on the 40 random grids: for the field pass's cells (visited, ascending),
    for a drawn visiting order cut by a cap as in the supervision pass, each with and without the supervision pass's tail, and for an
    empty list of cells.  No device."""
    from macarons_amd.utility import macarons_utils as mu
    n_jobs = n_empty = n_multi = 0
    for g in _random_job_grids():
        args = (g["visit"], g["counts"], g["sel_off"], g["s_start"], g["s_len"], g["nbm"], g["xf_all"], g["perm"], g["chunk"], g["k"])
        rng = np.random.default_rng(1000 + g["trial"])
        m_cell = _restated_job_tables(*args)["m_cell"]
        ascending = np.nonzero((g["visit"] != 0) & (m_cell > 2 * 2 * g["k"]) & (g["counts"] > 0))[0]
        cand = np.nonzero(g["counts"] > 0)[0]                           # the supervision pass: a drawn order, cut by the cap
        walk = cand[rng.permutation(cand.size)][:int(rng.integers(0, 6))]
        for tail in (False, True):
            want = _restated_job_tables(*args, tail=tail)
            _assert_plan_is(_plan_of(mu, g, ascending, tail=tail), want, (g["trial"], "field", tail))
            want_w = _restated_job_tables(*args, cells_run=walk, tail=tail)
            _assert_plan_is(_plan_of(mu, g, walk.tolist(), tail=tail), want_w, (g["trial"], "walk", tail))
            want_0 = _restated_job_tables(*args, cells_run=np.zeros(0, np.int64), tail=tail)
            plan_0 = _plan_of(mu, g, [], tail=tail)
            _assert_plan_is(plan_0, want_0, (g["trial"], "empty", tail))
            assert plan_0.J == 0 and plan_0.raw is None and plan_0.q_start.tolist() == [0] and plan_0.m_start.tolist() == [0]
        n_jobs += want["J"] + want_w["J"]
        n_empty += want["J"] == 0
        n_multi += int((-(-g["counts"][ascending] // g["chunk"]) > 1).sum())
    assert n_jobs > 1000 and n_multi > 100                              # the grids do hold jobs, and cells of several chunks


class _StandInCell:
    def __init__(self, ijk, n_pts, rng):
        lo = torch.tensor(ijk, dtype=torch.float32)
        self.x_min, self.x_max, self.center = lo, lo + 1.0, lo + 0.5
        self.cell_pts = torch.from_numpy(rng.random((n_pts, 3)).astype(np.float32)) + lo


class _StandInScene:
    """What the surface view reads of a reference Scene: the grid shape and a `cells` dict of per-cell tensors (no flat store)."""
    feature_dim = 0

    def __init__(self, grid, sizes, rng):
        self.grid_l, self.grid_w, self.grid_h = grid
        ijk = [(i, j, k) for i in range(grid[0]) for j in range(grid[1]) for k in range(grid[2])]
        self.cells = {str(list(c)): _StandInCell(c, int(n), rng) for c, n in zip(ijk, sizes)}


def test_surface_cells_by_key_and_its_plan():
    """macarons_utils._surface_cells on a surface scene that holds only some of the proxy grid's cells (a smaller grid: the by-key
    case) and on one with all of them (aligned): s_start / s_len per linear cell id of the proxy grid, the store's points, nb_len,
    m_cell -- and the plan over that view equals the restatement's."""
    from macarons_amd.utility import macarons_utils as mu
    rng = np.random.default_rng(7)
    pgrid = (3, 4, 3)
    nk = pgrid[0] * pgrid[1] * pgrid[2]
    proxy = _StandInScene(pgrid, np.zeros(nk, np.int64), rng)
    tab = mu._grid_tables(proxy, "cpu")
    nbm = tab["neighbour_matrix"]
    for sgrid in ((2, 3, 2), pgrid):
        sizes = (rng.integers(1, 60, sgrid[0] * sgrid[1] * sgrid[2]) * (rng.random(sgrid[0] * sgrid[1] * sgrid[2]) < 0.8)).astype(np.int64)
        surface = _StandInScene(sgrid, sizes, rng)
        surf = mu._surface_cells(surface, tab, "cpu")
        # the statement: the store holds the surface cells in lexicographic order; a proxy cell without a surface cell is empty
        s_len, s_start, at, pts = np.zeros(nk, np.int64), np.zeros(nk, np.int64), 0, []
        for (i, j, k), n in zip([(i, j, k) for i in range(sgrid[0]) for j in range(sgrid[1]) for k in range(sgrid[2])], sizes):
            lin = (i * pgrid[1] + j) * pgrid[2] + k
            s_len[lin], s_start[lin] = n, at
            at += int(n)
            pts.append(surface.cells[str([i, j, k])].cell_pts)
        assert surf.aligned == (sgrid == pgrid)
        assert np.array_equal(surf.s_len, s_len) and np.array_equal(surf.s_start, s_start)
        assert torch.equal(surf.store.pts, torch.cat(pts)) and int(surf.store.off[-1]) == at
        nb_len = np.where(nbm >= 0, s_len[np.maximum(nbm, 0)], 0)
        assert np.array_equal(surf.nb_len, nb_len) and np.array_equal(surf.m_cell, nb_len.sum(1))
        counts = (rng.integers(0, 90, nk) * (rng.random(nk) < 0.8)).astype(np.int64)
        sel_off = np.concatenate(([0], np.cumsum(counts), [counts.sum()])).astype(np.int64)
        xf_all, perm = rng.standard_normal((nk, 20)).astype(np.float32), rng.permutation(97).astype(np.int32)   # (the tail's padding: 4 bytes)
        visit = (rng.random(nk) < 0.8).astype(np.int64)
        for tail in (False, True):
            want = _restated_job_tables(visit, counts, sel_off, s_start, s_len, nbm, xf_all, perm, 40, 1, tail=tail)
            cells_run = np.nonzero((visit != 0) & (nb_len.sum(1) > 4) & (counts > 0))[0]
            plan = mu._plan_jobs(cells_run, counts, sel_off, surf, nbm, xf_all, perm, 40, tail=tail)
            _assert_plan_is(plan, want, (sgrid, tail))
            assert plan.J > len(cells_run) > 3 and plan.n_seg > plan.J
        if sgrid != pgrid:
            assert (s_len == 0).sum() >= nk - sgrid[0] * sgrid[1] * sgrid[2] and s_len.sum() > 0


def test_field_table_offsets_are_the_literal_layout():
    """ops.field_table_offsets names the byte layout of the uploaded table once: job rows of 32 B, segment rows of 32 B, 80 B of
    transform per job, then the bin permutation -- for the (J, n_seg) pairs of tests/test_scene_store_gpu.py:BUILD_CASES."""
    from macarons_amd import ops
    import _scene_model as M
    import test_scene_store_gpu as S
    assert (ops.FIELD_JOB_ROW_BYTES, ops.FIELD_SEGMENT_ROW_BYTES, ops.FIELD_TRANSFORM_ROW_BYTES) == (32, 32, 80)
    pairs = []
    for T, (sel_cells, chunk) in S.BUILD_CASES.items():                 # (the set-up of test_field_build, on the host)
        grid, nk = (3, 2, 3), 18
        rng = np.random.default_rng(T)
        P = T + 300
        key = np.full(P, nk, np.int64)
        key[rng.permutation(P)[:T]] = np.repeat(list(sel_cells), list(sel_cells.values()))
        _, counts, sel_off = M._group(key, nk)
        s_off = np.concatenate(([0], np.cumsum(rng.integers(0, 40, nk) * (rng.random(nk) < 0.7)))).astype(np.int64)
        jt, st = S._job_tables((counts[:nk] > 0).astype(np.int64), counts[:nk], sel_off, s_off, S._neighbour_matrix(grid), chunk, 1)[:2]
        pairs.append((len(jt), len(st)))
    assert [J for J, _ in pairs] == [1, 2, 8]
    for J, n_seg in pairs + [(0, 0)]:
        assert ops.field_table_offsets(J, n_seg) == (32 * J, 32 * (J + n_seg), 32 * (J + n_seg) + 80 * J)


def test_native_field_jobs_equal_the_numpy_tables():
    """torch.ops.macarons.field_jobs (C++ loop) builds the (cell, chunk) job tables of the occupancy-field pass element for element
    as the numpy restatement above does, and as the product's numpy planner (macarons_utils._plan_jobs over the visited cells) does:
    random grids, empty cells, cells that do not run (too few surface points, no queries, never visited), several chunks per cell."""
    import numpy as np
    import torch
    from macarons_amd.utility import macarons_utils as mu
    if not mu._native_field_jobs():
        import pytest
        pytest.skip("C++ extension not built")
    for g in _random_job_grids():
        trial, n_oof = g["trial"], g["n_oof"]
        raw_t, meta_t = torch.ops.macarons.field_jobs(torch.from_numpy(g["hostc"]), torch.from_numpy(g["s_off"]), torch.from_numpy(g["nbm"]),
                                                      torch.from_numpy(g["xf_all"]), torch.from_numpy(g["perm"]), g["n_cells"], g["chunk"], g["k"])
        meta = meta_t.numpy()
        w = _restated_job_tables(g["visit"], g["counts"], g["sel_off"], g["s_start"], g["s_len"], g["nbm"], g["xf_all"], g["perm"], g["chunk"], g["k"])
        J, job_q, job_m, q_start, m_start, raw = w["J"], w["job_q"], w["job_m"], w["q_start"], w["m_start"], w["raw"]
        assert int(meta[0]) == J and int(meta[1]) == w["n_seg"] and int(meta[2]) == int(q_start[-1]) and int(meta[3]) == int(m_start[-1]) and int(meta[4]) == n_oof
        assert np.array_equal(meta[5:5 + J], job_q) and np.array_equal(meta[5 + J:5 + 2 * J], job_m)
        assert np.array_equal(meta[5 + 2 * J:6 + 3 * J], q_start) and np.array_equal(meta[6 + 3 * J:7 + 4 * J], m_start)
        assert np.array_equal(raw_t.numpy(), raw), trial
        # ---- the product's numpy planner over the visited cells builds what the extension builds (and so what the restatement does)
        surf = mu._SurfaceCells(None, g["s_start"], g["s_len"], True, g["nbm"])
        ascending = np.nonzero((g["visit"] != 0) & (surf.m_cell > 2 * 2 * g["k"]) & (g["counts"] > 0))[0]
        plan = mu._plan_jobs(ascending, g["counts"], g["sel_off"], surf, g["nbm"], g["xf_all"], g["perm"], g["chunk"])
        _assert_plan_is(plan, w, trial)
        assert (plan.J, plan.n_seg, plan.T, plan.tot) == tuple(int(v) for v in meta[:4]), trial
        assert np.array_equal(plan.job_q, meta[5:5 + J]) and np.array_equal(plan.job_m, meta[5 + J:5 + 2 * J]), trial
        assert np.array_equal(plan.q_start, meta[5 + 2 * J:6 + 3 * J]) and np.array_equal(plan.m_start, meta[6 + 3 * J:7 + 4 * J]), trial
        assert (plan.raw is None and J == 0) or np.array_equal(plan.raw, raw_t.numpy()), trial


def _ragged_table_cases():
    """The 100 random job lists of the ragged-table tests (jobs without queries included), each with and without the row -> job part."""
    rng = np.random.default_rng(0)
    for _ in range(100):
        J = int(rng.integers(1, 30)); cs = rng.integers(16, 5000, J).tolist(); qs = rng.integers(0, 900, J).tolist(); rows = int(rng.choice([64, 128]))
        for wr in (True, False):
            yield cs, qs, rows, wr


def _restated_ragged_tables(cs, qs, rows, wr):
    """The numpy code of SconeOcc.forward_ragged_begin as it stood before SconeOcc.ragged_job_tables existed, restated: the frozen
    statement the product builder and the extension are compared with."""
    J = len(cs)
    off0 = np.concatenate(([0], np.cumsum(cs))).astype(np.int64); q = np.asarray(qs, np.int64); q0 = np.concatenate(([0], np.cumsum(q)))
    nb = -(-q // rows); bj = np.repeat(np.arange(J, dtype=np.int64), nb)
    b_in = np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb)
    blocks = np.stack((bj, q0[bj] + b_in * rows, np.minimum(rows, q[bj] - b_in * rows), np.zeros_like(bj)), 1)
    parts = [off0, blocks.reshape(-1)] + ([np.repeat(np.arange(J, dtype=np.int64), q)] if wr else [])
    return np.concatenate(parts)


def test_ragged_job_tables_equal_the_restatement():
    """SconeOcc.ragged_job_tables -- the product's numpy builder of the tables forward_ragged_begin uploads (cloud offsets, query blocks,
    row -> job) -- == the restatement, on the 100 random job lists.  No device, no extension."""
    so = importlib.import_module("macarons_amd.networks.SconeOcc")     # (the package re-exports the CLASS under the module's name)
    n_zero = 0
    for cs, qs, rows, wr in _ragged_table_cases():
        got = so.ragged_job_tables(cs, qs, rows, wr)
        assert got.dtype == np.int64 and np.array_equal(got, _restated_ragged_tables(cs, qs, rows, wr))
        n_zero += sum(q == 0 for q in qs)
    assert n_zero > 0                                                   # (jobs without queries: no block, no row)


def test_native_ragged_tables_equal_the_numpy_tables():
    """torch.ops.macarons.ragged_tables == the product's numpy builder (SconeOcc.ragged_job_tables) == the restatement of the tables of
    SconeOcc.forward_ragged_begin (cloud offsets, query blocks, row -> job)."""
    so = importlib.import_module("macarons_amd.networks.SconeOcc")     # (the package re-exports the CLASS under the module's name)
    if not so._native_ragged_tables():
        import pytest
        pytest.skip("C++ extension not built")
    for cs, qs, rows, wr in _ragged_table_cases():
        a = torch.ops.macarons.ragged_tables(cs, qs, rows, wr).numpy()
        assert np.array_equal(a, _restated_ragged_tables(cs, qs, rows, wr))
        assert np.array_equal(a, so.ragged_job_tables(cs, qs, rows, wr))


def test_native_field_prepare_equals_the_python_restatement():
    """torch.ops.macarons.field_prepare (the cells' prediction-box transforms + the view-space bin permutation in one C++ call over the
    same ATen operators) == macarons_utils._field_prepare's tensor code, bit for bit."""
    import torch
    from macarons_amd.utility import scone_utils as su, macarons_utils as mu
    if not (mu._native_field_jobs() and hasattr(torch.ops.macarons, "field_prepare")):
        import pytest
        pytest.skip("C++ extension not built")
    torch.manual_seed(1)
    su.view_space_bin_permutation(torch.eye(3), 7, 14, "cpu")
    x_ref = su._REF_DIRECTIONS[(7, 14)]
    for i in range(200):
        R = torch.linalg.qr(torch.randn(3, 3))[0].float()
        if i % 5 == 0:
            R = torch.eye(3)[torch.randperm(3)] * torch.tensor([1., -1., 1.])[torch.randperm(3)]
        Mv = torch.eye(4); Mv[:3, :3] = R; Mv[3, :3] = torch.randn(3) * 20
        n = int(torch.randint(1, 100, (1,)))
        cw, dg, pns = torch.randn(n, 3) * 10, torch.rand(n) * 5 + 1, 1.5
        a, b = torch.ops.macarons.field_prepare(Mv, cw, dg, x_ref, pns, 7, 14)
        cen_h = (torch.cat((cw, torch.ones(n, 1)), 1) @ Mv)[:, :3]
        inv_h = (1.0 / (pns * dg)).float()
        xf = torch.cat((Mv.reshape(1, 16).expand(n, -1), cen_h, inv_h.view(n, 1)), 1).contiguous()
        perm = su.view_space_bin_indices((x_ref @ Mv[:3, :3].contiguous().view(3, 3).T).reshape(-1, 3), 7, 14).to(torch.int32)
        assert torch.equal(a, xf) and torch.equal(b, perm), i
        if i % 10 == 0:                 # the worker-thread form: same tensors; the caller may rewrite its matrix once the ticket is out
            Mv2 = Mv.clone()
            t = torch.ops.macarons.field_prepare_async(Mv2, cw, dg, x_ref, pns, 7, 14)
            Mv2.zero_()
            a2, b2 = torch.ops.macarons.field_prepare_wait(t)
            assert torch.equal(a2, a) and torch.equal(b2, b), i
    import pytest
    tickets = [torch.ops.macarons.field_prepare_async(Mv, cw, dg, x_ref, pns, 7, 14) for _ in range(4)]     # collected out of order
    for t in reversed(tickets):
        a2, b2 = torch.ops.macarons.field_prepare_wait(t)
        assert torch.equal(a2, a) and torch.equal(b2, b)
    with pytest.raises(RuntimeError):
        torch.ops.macarons.field_prepare_wait(tickets[0])          # a ticket is good for one collection
    t = torch.ops.macarons.field_prepare_async(torch.zeros(3, 3), cw, dg, x_ref, pns, 7, 14)
    with pytest.raises(RuntimeError):                               # the job's error surfaces at the wait
        torch.ops.macarons.field_prepare_wait(t)
