"""The host model of the scene fill (tests/_scene_model.py) against itself and against the torch-CPU path of Scene: where upstream's rule
for Scene.fill_cells (every in-box point to every englobing cell) and the fused path's (floor cell, then that cell's box) agree, where
they part, and that the inputs of tests/test_scene_store_gpu.py are what they claim to be.  No GPU."""
import numpy as np
import pytest
import torch

import _scene_cases as C
import _scene_model as M

F = np.float32
NEAR_FACE_GRIDS = [(3, 2, 3), (4, 3, 5), (3, 3, 3)]


def _args(tab):
    return tab["lo"], tab["hi"], tab["x_min"], tab["x_max"], tab["step"], tab["grid"]


def _both_rules(case, features, feats, valid, npm, seed=5):
    out = []
    for rule in (M.fill_cells_upstream, M.fill_cells_floor_rule):
        rng = np.random.default_rng(seed)
        out.append(rule(case["store"], feats, case["pts"], features, valid, *_args(case["tab"]), case["resolution"], case["capacity"], npm,
                        lambda n: rng.permutation(n)))
    return out


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and \
        (a[1] is None) == (b[1] is None) and (a[1] is None or all(np.array_equal(x, y) for x, y in zip(a[1], b[1])))


@pytest.mark.parametrize("N,grid", C.FILL_CASES)
@pytest.mark.parametrize("part_filled", [False, True])
def test_rules_agree_on_guarded_clouds(N, grid, part_filled):
    """Every coordinate at least 1e-3 step from every face: no point is ambiguous and the two rules give the same cells bit for bit,
    points and features, with and without `valid`, for both n_point_min."""
    case = C.fill_case(N, grid, part_filled)
    assert C.face_margin(case["pts"], case["tab"]) >= 1e-3 and all(C.face_margin(s_, case["tab"]) >= 1e-3 for s_ in case["store"])
    assert not M.ambiguous(case["pts"], None, *_args(case["tab"])).any()
    features, feats = C.case_features(case, 3)
    for frac in (None, 0.7):
        for npm in (0, 3):
            up, fl = _both_rules(case, features, feats, C.case_valid(case, frac), npm)
            assert _same(up, fl), (frac, npm)
    assert not _same(up, (case["store"], feats)) or N == 1            # (the fill did something)


def test_rules_agree_on_face_points_of_the_dyadic_grid():
    """(3,2,3) over +-(12,6,12): steps 8, 6, 8 and every face are exact in fp32, so a point exactly on a face is strictly inside no cell
    and both rules drop it."""
    tab = C.grid_tables((3, 2, 3))
    rng = np.random.default_rng(3)
    pts = C.guarded_points(rng, 600, tab)
    faces = [np.array([-12., -4., 4., 12.]), np.array([-6., 0., 6.]), np.array([-12., -4., 4., 12.])]
    on_face = pts[:300].copy()
    for i in range(300):
        a = i % 3
        on_face[i, a] = faces[a][rng.integers(0, len(faces[a]))]
    pts = np.concatenate((on_face, pts[300:]))
    assert not M.ambiguous(pts, None, *_args(tab)).any()
    empty = [np.zeros((0, 3), F) for _ in range(18)]
    case = {"tab": tab, "pts": pts, "store": empty, "capacity": 1000, "resolution": 0.25}
    up, fl = _both_rules(case, None, None, None, 0)
    assert _same(up, fl)
    kept = np.concatenate(up[0])
    assert len(kept) == 300 and not (kept[:, None, :] == on_face[None, :, :]).all(-1).any()


@pytest.mark.parametrize("grid", NEAR_FACE_GRIDS)
def test_near_face_set_is_ambiguous_and_the_rules_part(grid):
    """Coordinates within +-2 ulp of the interior faces (and +-1e-7 next to a face at 0), every cell englobing: at least 100 points lie
    strictly inside a cell other than their floor cell, and on this set the floor rule does not give upstream's cells -- the
    divergence Scene.fill_cells closes by filling such a call upstream's way.  Without the flagged points the rules agree again."""
    tab = C.grid_tables(grid)
    pts = C.near_face_points(tab, np.random.default_rng(11))
    amb = M.ambiguous(pts, None, *_args(tab))
    print(grid, "ambiguous", int(amb.sum()), "of", len(pts))
    assert amb.sum() >= 100
    empty = [np.zeros((0, 3), F) for _ in range(int(np.prod(grid)))]
    case = {"tab": tab, "pts": pts, "store": empty, "capacity": 10 ** 6, "resolution": 0.0}
    up, fl = _both_rules(case, None, None, None, 0)
    assert not _same(up, fl)
    case["pts"] = pts[~amb]
    up, fl = _both_rules(case, None, None, None, 0)
    assert _same(up, fl)


def test_the_example_of_the_issue():
    """(1, -1e-7, 3) on (3,2,3) over +-(12,6,12): fl(-1e-7 + 6) = 6, the floor rule names cell 10 whose strict test fails; the point
    lies strictly inside cell 7."""
    tab = C.grid_tables((3, 2, 3))
    p = np.array([[1., -1e-7, 3.]], F)
    assert M.floor_cells(p, tab["x_min"], tab["step"], tab["grid"])[0] == 10
    assert M.strictly_inside(p, tab["lo"][7], tab["hi"][7])[0] and not M.strictly_inside(p, tab["lo"][10], tab["hi"][10])[0]
    assert M.ambiguous(p, None, *_args(tab))[0]


@pytest.mark.parametrize("grid", NEAR_FACE_GRIDS)
def test_scene_fallback_on_cpu_is_upstream(grid):
    """Scene.fill_cells_upstream on CPU tensors (the torch path: get_pts_in_bounding_box, the floor rule, Cell.fill) on the near-face
    set == the model of upstream's control flow, cell by cell, with the same torch.randperm draws; and Scene's tables and floor rule
    are the model's."""
    from macarons_amd.utility.scene import Scene
    tab = C.grid_tables(grid)
    pts = C.near_face_points(tab, np.random.default_rng(12))
    features = np.arange(len(pts), dtype=F)[:, None]
    x_min, x_max = C.BOXES[grid]
    sc = Scene(torch.tensor(x_min), torch.tensor(x_max), *grid, 40, 0.25, 16, "cpu", feature_dim=1)
    assert np.array_equal(sc.linear_cell_ids(torch.from_numpy(pts)).numpy(), M.floor_cells(pts, tab["x_min"], tab["step"], grid))
    valid = np.random.default_rng(1).random(len(pts)) < 0.8
    torch.manual_seed(4)
    sc.fill_cells_upstream(torch.from_numpy(pts), torch.from_numpy(features), 2, None, torch.from_numpy(valid))
    state = torch.get_rng_state()
    torch.manual_seed(4)
    nk = int(np.prod(grid))
    want, want_f = M.fill_cells_upstream([np.zeros((0, 3), F)] * nk, [np.zeros((0, 1), F)] * nk, pts, features, valid, *_args(tab), 0.25, 40, 2,
                                         lambda n: torch.randperm(n).numpy())
    assert torch.equal(state, torch.get_rng_state())
    cells = sc._cell_table()[0]
    for c in range(nk):
        assert np.array_equal(cells[c].cell_pts.numpy(), want[c]) and np.array_equal(cells[c].cell_features.numpy(), want_f[c]), c


def _begin(case, valid, npm):
    sp, so, _ = C.flat(case["store"])
    return M.fill_begin_model(case["pts"], valid, *_args(case["tab"]), sp, so, case["resolution"], npm), so


def test_gpu_inputs_keep_clear_of_the_admission_threshold_and_cover_the_edges():
    """Every fill the GPU tests run: no candidate within 1e-9 of the resolution unless it is AT the resolution (the lattice ties), so
    a kernel and the model cannot part over a last bit of the fp64 distance; and the edges the GPU tests are about do occur: untouched
    cells between touched ones (shared offsets), duplicates both admitted, exact ties rejected, a cell over capacity, odd and even
    n_pm, a fill with every candidate rejected, cells kept from drawing by n_point_min."""
    seen = set()
    for N, grid in C.FILL_CASES:
        for part_filled in (False, True):
            case = C.fill_case(N, grid, part_filled)
            for frac in (None, 0.7):
                for npm in (0, 3):
                    m, so = _begin(case, C.case_valid(case, frac), npm)
                    d = m["dmin"][m["dmin_rows"]]
                    d = d[np.isfinite(d)]
                    near = np.abs(d - case["resolution"]) < 1e-9
                    assert (d[near] == case["resolution"]).all(), (N, grid, part_filled)
                    seen.add("tie") if near.any() else None
                    nk = int(np.prod(grid))
                    cand, adm = m["counts"][:nk], m["counts"][2 * nk + 3:3 * nk + 3]
                    plan = C.gather_plan(m["counts"], so, case["capacity"], npm, np.random.default_rng(0))
                    t = np.nonzero(plan["touched"])[0]
                    if len(t) > 1 and (np.diff(plan["new_off"])[t[0]:t[-1]] == 0).any():
                        seen.add("shared_offset")
                    seen.add("over_capacity") if plan["over_capacity"] else None
                    seen.add("odd_n_pm" if plan["n_pm"] % 2 else "even_n_pm")
                    seen.add("all_rejected") if (cand.sum() > 0 and adm.sum() == 0) else None
                    seen.add("below_n_point_min") if ((cand > 0) & (cand <= npm)).any() else None
                    if N >= 16 and frac is None and npm == 0 and not part_filled:
                        k2 = np.empty(N, np.int64)
                        k2[m["order"]] = m["key2"]                     # admission per source row
                        assert (k2[N - 8:N] < nk).all()                 # the duplicated candidates: both copies admitted
                        seen.add("duplicates")
                    assert m["counts"][-1] == 0                         # guarded: nothing ambiguous
    assert seen >= {"tie", "shared_offset", "over_capacity", "odd_n_pm", "even_n_pm", "all_rejected", "below_n_point_min", "duplicates"}, seen


def _clear_of_threshold(tab, stores, pts, valid, npm):
    sp, so, _ = C.flat(stores)
    d = M.fill_begin_model(pts, valid, *_args(tab), sp, so, C.RESOLUTION, npm)
    dm = d["dmin"][d["dmin_rows"]]
    # upstream's way every englobing cell tests every point strictly inside it: the ambiguous points against every store as well
    amb = M.ambiguous(pts, valid, *_args(tab))
    extra = [M.S.min_dist(pts[amb], s_) for s_ in stores if len(s_) and amb.any()]
    dm = np.concatenate([dm] + extra)
    dm = dm[np.isfinite(dm)]
    assert not (np.abs(dm - C.RESOLUTION) < 1e-9).any()
    return int(d["counts"][-1])


def test_end_to_end_inputs_keep_clear_of_the_admission_threshold():
    """The successive fills of the end-to-end GPU tests, with the draws torch makes after the same seed: three guarded clouds (nothing
    ambiguous), then the near-face set; and the part-filled scene of the near-face test."""
    for grid in ((3, 2, 3), (4, 3, 5)):
        tab = C.grid_tables(grid)
        nk = int(np.prod(grid))
        stores, feats = [np.zeros((0, 3), F)] * nk, [np.zeros((0, 2), F)] * nk
        torch.manual_seed(C.E2E_SEED)
        for k, (pts, features, valid) in enumerate(C.e2e_fills(tab)):
            assert (_clear_of_threshold(tab, stores, pts, valid, C.E2E_N_POINT_MIN) == 0) == (k < 3)
            stores, feats = M.fill_cells_upstream(stores, feats, pts, features, valid, *_args(tab), C.RESOLUTION, C.E2E_CAPACITY,
                                                  C.E2E_N_POINT_MIN, lambda n: torch.randperm(n).numpy())
            if k == 2:
                assert max(len(s_) for s_ in stores) == C.E2E_CAPACITY       # some cell reached its capacity
    for grid in NEAR_FACE_GRIDS:
        tab = C.grid_tables(grid)
        nk = int(np.prod(grid))
        first, near = C.near_face_scenario(tab)
        torch.manual_seed(3)
        stores, _ = M.fill_cells_upstream([np.zeros((0, 3), F)] * nk, None, first, None, None, *_args(tab), C.RESOLUTION, C.NEAR_CAPACITY, 0,
                                          lambda n: torch.randperm(n).numpy())
        assert _clear_of_threshold(tab, stores, near, None, 0) >= 100


@pytest.mark.parametrize("N,grid", C.FILL_CASES)
def test_entry_models_compose_to_the_floor_rule(N, grid):
    """fill_begin_model -> the host's plan -> gather_perm_model, cut at the new offsets == fill_cells_floor_rule with the same
    permutations: the models of the three device entries are together the documented rule (and hence, on guarded inputs, upstream's)."""
    case = C.fill_case(N, grid, True)
    tab, nk = case["tab"], int(np.prod(grid))
    features, feats = C.case_features(case, 3)
    for frac in (None, 0.7):
        for npm in (0, 3):
            valid = C.case_valid(case, frac)
            sp, so, sf = C.flat(case["store"], feats)
            m = M.fill_begin_model(case["pts"], valid, *_args(tab), sp, so, case["resolution"], npm)
            plan = C.gather_plan(m["counts"], so, case["capacity"], npm, np.random.default_rng(1))
            got_p, got_f = M.gather_perm_model(plan["pm"], plan["tables"], nk, plan["n_new"], sp, sf, int(so[-1]), 3, case["pts"], features,
                                               m["order"], m["order2"])
            pm_off = plan["tables"][3 * (nk + 1):4 * (nk + 1)]
            perms = [plan["pm"][pm_off[c]:pm_off[c + 1]] for c in np.nonzero(plan["touched"])[0]]
            want, want_f = M.fill_cells_floor_rule(case["store"], feats, case["pts"], features, valid, *_args(tab), case["resolution"],
                                                   case["capacity"], npm, perms)
            for c in range(nk):
                rows = slice(int(plan["new_off"][c]), int(plan["new_off"][c + 1]))
                assert np.array_equal(got_p[rows], want[c]) and np.array_equal(got_f[rows], want_f[c]), (frac, npm, c)
