"""Inputs of the scene fill / field-pass tests (numpy; TEST INFRASTRUCTURE), shared by tests/test_scene_model_cpu.py -- which checks
that they are what they claim to be: guarded against cell faces, clear of the admission threshold except for exact ties, and
covering every edge the GPU tests are about -- and tests/test_scene_store_gpu.py, which runs the kernels on them.

Guarded points keep every coordinate at least 1e-3 step away from every cell face, where upstream's rule and the fused path's
provably agree.  Exact ties with the admission threshold come from the 2^-3 lattice with resolution = 0.25: every coordinate is a
multiple of 1/8, so squares and their sums are exact in fp64 and a candidate 0.25 along one axis from a stored point is at the
resolution exactly (not admitted: the test is strict)."""
import numpy as np

F = np.float32
RESOLUTION = 0.25

BOXES = {                      # grid -> (x_min, x_max)
    (1, 1, 1): ((-1., -1., -1.), (1., 1., 1.)),
    (3, 2, 3): ((-12., -6., -12.), (12., 6., 12.)),                    # dyadic steps (8, 6, 8)
    (4, 3, 5): ((-1.3, -2., 0.5), (3.1, 2.2, 4.)),                     # steps that fp32 does not hold
    (11, 3, 31): ((-5.5, -1.5, -15.5), (5.5, 1.5, 15.5)),              # 1023 cells: the most the counting sort takes
    (3, 3, 3): ((-1., -1., -1.), (1., 1., 1.)),                        # step 2/3: the rounded boxes of neighbours overlap
}
FILL_CASES = [(1, (1, 1, 1)), (255, (3, 2, 3)), (2049, (3, 2, 3)), (5000, (4, 3, 5)), (3000, (11, 3, 31))]
FILL_VARIANTS = [(Fdim, frac, npm) for Fdim in (0, 1, 3) for frac in (None, 0.7) for npm in (0, 3)]


def grid_tables(grid, capacity=None, resolution=RESOLUTION):
    """The tables of a Scene on this grid, from the CPU tensors of Scene itself: dict(grid, x_min, x_max, step, lo, hi)."""
    import torch
    from macarons_amd.utility.scene import Scene
    x_min, x_max = BOXES[tuple(grid)]
    sc = Scene(torch.tensor(x_min), torch.tensor(x_max), grid[0], grid[1], grid[2], capacity or 8, resolution, 16, "cpu")
    _, lo, hi = sc._cell_table()
    return {"grid": tuple(grid), "x_min": sc.x_min.numpy().astype(F), "x_max": sc.x_max.numpy().astype(F),
            "step": torch.stack((sc.l, sc.w, sc.h)).numpy().astype(F), "lo": lo.numpy().astype(F), "hi": hi.numpy().astype(F)}


def face_margin(pts, tab):
    """Smallest distance (in steps) of any coordinate to any cell face of the grid, fp64."""
    x0, st = tab["x_min"].astype(np.float64), tab["step"].astype(np.float64)
    u = (np.asarray(pts, np.float64) - x0) / st
    return float(np.abs(u - np.round(u)).min()) if len(pts) else 1.0


def guarded_points(rng, n, tab, cells=None, each=False):
    """n fp32 points inside the scene box with every coordinate >= 1e-3 step (and more) away from every face; cells: linear ids to
    draw from (None = all; each=True: point i goes to cells[i])."""
    g = np.array(tab["grid"])
    lin = rng.integers(0, g.prod(), n) if cells is None else np.asarray(cells) if each else rng.choice(np.asarray(cells), n)
    idx = np.stack((lin // (g[1] * g[2]), (lin // g[2]) % g[1], lin % g[2]), 1)
    u = rng.uniform(0.01, 0.99, (n, 3))
    return (tab["x_min"].astype(np.float64) + (idx + u) * tab["step"].astype(np.float64)).astype(F)


def lattice_triples(tab, cells, n_max=6):
    """Per chosen cell a stored point s on the 2^-3 lattice near the cell's centre and three candidates: s + (1/4, 0, 0) at the
    resolution exactly (rejected), s + (1/4, 1/8, 0) beyond it (admitted), s + (1/8, 1/8, 1/8) within it (rejected).  Only cells
    where all four points keep the face guard are used.  -> (stored [k,3], stored cell ids [k], candidates [3k,3])."""
    g = np.array(tab["grid"])
    stored, ids, cands = [], [], []
    for c in cells:
        idx = np.array((c // (g[1] * g[2]), (c // g[2]) % g[1], c % g[2]))
        ctr = tab["x_min"].astype(np.float64) + (idx + 0.5) * tab["step"].astype(np.float64)
        s_ = np.round(ctr * 8) / 8
        four = np.stack((s_, s_ + (.25, 0, 0), s_ + (.25, .125, 0), s_ + (.125, .125, .125)))
        u = (four - tab["x_min"].astype(np.float64)) / tab["step"].astype(np.float64)
        if (np.floor(u) == idx).all() and np.abs(u - np.round(u)).min() > 1e-2:
            stored.append(four[0]); ids.append(c); cands.extend(four[1:])
        if len(ids) == n_max:
            break
    return np.array(stored, F).reshape(-1, 3), np.array(ids, np.int64), np.array(cands, F).reshape(-1, 3)


def fill_case(N, grid, part_filled, seed=0):
    """One fill: dict(tab, pts [N,3], store (per cell [n,3]), capacity, resolution, n_lattice).  About 60 % of the cells receive points,
    so untouched cells sit between touched ones; some candidates are duplicated; with a part-filled store some cells are driven over
    capacity, and lattice candidates sit exactly at, beyond and within the resolution of a stored lattice point.  N = 1 with a store:
    the one candidate is at the resolution exactly, i.e. every candidate is rejected."""
    tab = grid_tables(grid)
    rng = np.random.default_rng([seed, N, int(part_filled)] + list(grid))
    nk = int(np.prod(grid))
    live = np.sort(rng.choice(nk, max(1, int(round(0.6 * nk))), replace=False)) if nk > 1 else np.array([0])
    capacity = max(2, int(1.2 * N / len(live)))
    store = [np.zeros((0, 3), F) for _ in range(nk)]
    pts = guarded_points(rng, N, tab, live)
    n_lat = 0
    if part_filled:
        s_pts, s_ids, cands = lattice_triples(tab, live.tolist())
        for c in rng.choice(live, max(1, len(live) // 2), replace=False).tolist():
            store[c] = guarded_points(rng, int(rng.integers(1, capacity + 1)), tab, [c])
        for s_, c in zip(s_pts, s_ids):
            store[int(c)] = np.vstack((store[int(c)], s_[None]))[-capacity:]
        n_lat = min(len(cands), N)
        pts[:n_lat] = cands[:n_lat]
    if N >= 16:                                             # duplicated candidates inside the batch (both admitted)
        pts[N - 4:N] = pts[N - 8:N - 4]
    return {"tab": tab, "pts": pts, "store": store, "capacity": capacity, "resolution": RESOLUTION, "n_lattice": n_lat}


def case_valid(case, frac):
    """`valid` of a fill case: None, or about `frac` of the rows set (the lattice candidates stay offered)."""
    if frac is None:
        return None
    N = len(case["pts"])
    v = np.random.default_rng(N + 7).random(N) < frac
    v[:case["n_lattice"]] = True
    return v


def case_features(case, Fdim):
    N = len(case["pts"])
    if not Fdim:
        return None, None
    rng = np.random.default_rng(N + Fdim)
    feats = [rng.standard_normal((len(s_), Fdim)).astype(F) for s_ in case["store"]]
    return np.concatenate((np.arange(N, dtype=F)[:, None], rng.standard_normal((N, Fdim - 1)).astype(F)), 1), feats


def flat(store, feats=None):
    """Per-cell lists -> (store_pts [n,3], store_off [n_cells+1], store_fts [n,F] | None)."""
    off = np.concatenate(([0], np.cumsum([len(s_) for s_ in store]))).astype(np.int64)
    pts = np.concatenate(store + [np.zeros((0, 3), F)]).astype(F)
    return pts, off, (None if feats is None else np.concatenate(feats).astype(F).reshape(len(pts), feats[0].shape[1]))


def gather_plan(counts, b_off, capacity, n_point_min, rng):
    """The host part of Scene.fill_cells between the two device parts, restated: touched cells (cand > n_point_min) draw a permutation
    of their [stored | admitted] rows and keep its first `capacity` entries.  -> dict(n_new, n_pm, pm (int32), tables = new_off | b_off |
    adm_off | pm_off | touched, touched, new_off)."""
    nk = (len(counts) - 7) // 4
    cand, adm = counts[:nk], counts[2 * nk + 3:3 * nk + 3]
    b_len = np.diff(b_off)
    touched = cand > n_point_min
    n_comb = b_len + adm
    n_keep = np.where(touched, np.minimum(n_comb, capacity), b_len)
    pm = [rng.permutation(int(n_comb[c]))[:capacity] for c in np.nonzero(touched)[0]]
    pm = np.concatenate(pm + [np.zeros(0, np.int64)]).astype(np.int32)
    off = lambda a: np.concatenate(([0], np.cumsum(a))).astype(np.int64)
    new_off, pm_off = off(n_keep), off(np.where(touched, n_keep, 0))
    tables = np.concatenate([new_off, np.asarray(b_off, np.int64), off(adm), pm_off, np.concatenate((touched.astype(np.int64), [0]))])
    return {"n_new": int(new_off[-1]), "n_pm": int(pm_off[-1]), "pm": pm, "tables": tables, "touched": touched, "new_off": new_off,
            "over_capacity": bool((touched & (n_comb > capacity)).any())}


def near_face_points(tab, rng, per_cell=8):
    """The adversarial set: every coordinate 0, +-1, +-2 ulp around every interior face of the grid (the other two coordinates ordinary),
    the value -1e-7 next to a face at 0, and ordinary points in every cell so that every cell is englobing."""
    g, x0, st = np.array(tab["grid"]), tab["x_min"].astype(np.float64), tab["step"].astype(np.float64)
    out = [guarded_points(rng, per_cell * int(g.prod()), tab, np.repeat(np.arange(g.prod()), per_cell), each=True)]
    for a in range(3):
        faces = {F(tab["lo"][c][a]) for c in range(len(tab["lo"]))} | {F(tab["hi"][c][a]) for c in range(len(tab["hi"]))}
        faces |= {F(x0[a] + i * st[a]) for i in range(1, g[a])}
        faces = sorted(f_ for f_ in faces if tab["x_min"][a] < f_ < tab["x_max"][a])
        vals = []
        for f_ in faces:
            v = F(f_)
            dn1 = np.nextafter(v, F(-np.inf)); dn2 = np.nextafter(dn1, F(-np.inf))
            up1 = np.nextafter(v, F(np.inf)); up2 = np.nextafter(up1, F(np.inf))
            vals += [v, dn1, dn2, up1, up2]
            if abs(float(f_)) < 1e-6:
                vals += [F(-1e-7), F(1e-7)]
        vals = np.array(vals, F)
        n = 4000 // 3
        p = guarded_points(rng, n, tab)
        p[:, a] = vals[rng.integers(0, len(vals), n)]
        out.append(p)
    return np.concatenate(out).astype(F)


E2E_SEED, E2E_CAPACITY, E2E_N_POINT_MIN = 21, 25, 2


def e2e_fills(tab):
    """Successive fills of one scene: (pts, features [N,2], valid | None) each; three guarded clouds of different sizes, the second with
    about 80 % of its rows offered.  With E2E_CAPACITY some cells fill up and later fills are tested against their stores."""
    rng = np.random.default_rng([9] + list(tab["grid"]))
    out = []
    for k, n in enumerate((700, 901, 333)):
        pts = guarded_points(rng, n, tab)
        features = np.stack((np.arange(n, dtype=F) + 1000 * k, rng.standard_normal(n).astype(F)), 1)
        out.append((pts, features, (rng.random(n) < 0.8) if k == 1 else None))
    near = near_face_points(tab, rng)                       # a fourth fill on top: near-face points, done upstream's way
    out.append((near, np.stack((np.arange(len(near), dtype=F), np.ones(len(near), F)), 1), None))
    return out


NEAR_CAPACITY = 60


def near_face_scenario(tab):
    """(first, near): a guarded cloud that part-fills every cell (40 points per cell), then the near-face set."""
    rng = np.random.default_rng(8)
    return guarded_points(rng, 40 * int(np.prod(tab["grid"])), tab), near_face_points(tab, rng)
