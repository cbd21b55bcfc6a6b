"""The occupancy supervision pass without a GPU: the numpy model of its selection / walk / scatter (tests/_supervision_model.py)
against the golden the REFERENCE's compute_occupancy_probability_for_supervision produced (tests/golden/make_golden_supervision.py),
and the public surface (signature, opt-in patch tier, declared C entries)."""
import inspect
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import golden

import _supervision_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "macarons")),
                                     reason="needs the MACARONS reference source tree, which is not part of this repository")


def golden_scene(g):
    """The golden's scene as plain arrays: grid constants, the proxy store (cells in linear order) and the surface cells' sizes."""
    grid = [int(v) for v in g["grid"]]
    n = grid[0] * grid[1] * grid[2]
    lin = lambda key: int((key[0] * grid[1] + key[1]) * grid[2] + key[2])
    p_idx, s_len = [None] * n, np.zeros(n, np.int64)
    for i in range(int(g["n_surface_cells"])):
        p_idx[lin(g[f"pcellkey_{i}"])] = g[f"pcellidx_{i}"].astype(np.float32)
        s_len[lin(g[f"cellkey_{i}"])] = len(g[f"cellpts_{i}"])
    off = np.concatenate(([0], np.cumsum([len(v) for v in p_idx]))).astype(np.int64)
    step = ((g["x_max"] - g["x_min"]).astype(np.float32) / np.asarray(grid, np.float32)).astype(np.float32)
    return grid, np.concatenate(p_idx)[:, None], off, s_len, step


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_model_reproduces_reference_selection(case):
    """Given the golden's inputs and its two host draws, the model names the reference's prediction_mask, the cells that ran (in
    visiting order), every cell's query list and the number of dummy passes."""
    g = golden("occ_supervision")
    P, k = len(g["proxy"]), int(g["k"])
    grid, store_fts, store_off, s_len, step = golden_scene(g)
    pmask = np.unpackbits(g["proxy_mask"])[:P].astype(bool) & (not bool(g[f"{case}_mask_empty"]))
    sampled = M.sample_mask(pmask, g[f"{case}_sample_perm"], int(g["n_sup"]))
    eng, lists, counts, rows_order, pos = M.select_model(sampled, g["proxy"], g["x_min"], step, grid, store_fts, store_off)
    assert len(g[f"{case}_cell_perm"]) == int(eng.sum())                       # the second draw's size = the candidate cells
    visited, queries, n_dummy = M.walk_model(eng, lists, g[f"{case}_cell_perm"], M.neighbourhood_sizes(s_len, grid), int(g[f"{case}_cap"]), k)
    assert np.array_equal(visited, g[f"{case}_cells_run"])
    assert n_dummy == int(g[f"{case}_n_dummy"])
    off = g[f"{case}_query_off"]
    assert len(off) == len(visited) + 1
    for j, q in enumerate(queries):
        assert np.array_equal(q, g[f"{case}_queries"][off[j]:off[j + 1]]), j
    ref_mask = np.unpackbits(g[f"{case}_prediction_mask"])[:P].astype(bool)
    if visited:
        assert np.array_equal(sampled, ref_mask)
        assert int(counts[-1]) == int(ref_mask.sum()) == len(g[f"{case}_probas"])
        # a sampled point that no run cell stores keeps upstream's 0
        stored = np.zeros(P, bool)
        stored[np.concatenate(queries)] = True
        assert not g[f"{case}_probas"][~stored[ref_mask]].any()
    else:                                                                      # no pass ran: the first k+1 points, zeros
        assert np.array_equal(np.nonzero(ref_mask)[0], np.arange(k + 1)) and not g[f"{case}_probas"].any()
    # the draw sizes the reference made: sampling, cells, three per run cell (M, M, M // ds), three per dummy pass (4k+1, 4k+1, ...)
    sizes = g[f"{case}_perm_sizes"]
    assert sizes[0] == int(pmask.sum()) and sizes[1] == int(eng.sum()) and len(sizes) == 2 + 3 * (len(visited) + n_dummy)
    assert all(int(s_) == 4 * k + 1 for s_ in sizes[2 + 3 * len(visited)::3])


def test_model_scatter_adds_in_job_order():
    """An index in two jobs is added twice, in job order; an index in no job stays 0; the backward is the gather."""
    pos = np.array([-1, 0, 1, -1, 2, 3], np.int32)
    rows = np.array([1, 4, 2, 4, 9], np.int32)[:4]
    occ = np.array([0.1, 1e8, 0.3, 1.0], np.float32)
    out = M.scatter_model(rows, occ, [0, 2, 4], 2, pos, 4)
    assert np.array_equal(out, np.array([0.1, 0.3, np.float32(1e8) + np.float32(1.0), 0.0], np.float32))
    d = M.scatter_backward_model(rows, pos, np.array([1., 2., 3., 4.], np.float32), 4, 6)
    assert np.array_equal(d, np.array([1., 3., 2., 3., 0., 0.], np.float32))


def test_signature_and_surface():
    from macarons_amd import _lib, autograd, ops, patch
    from macarons_amd.utility import macarons_utils as mu
    names = list(inspect.signature(mu.compute_occupancy_probability_for_supervision).parameters)
    assert names == ["params", "macarons", "camera", "proxy_scene", "proxy_mask", "surface_scene", "n_cell_per_occ_forward_pass", "device",
                     "prediction_camera", "default_value", "min_length", "differentiable", "record", "chunk"]
    d = {k: v.default for k, v in inspect.signature(mu.compute_occupancy_probability_for_supervision).parameters.items()}
    assert (d["prediction_camera"], d["default_value"], d["min_length"], d["differentiable"], d["record"], d["chunk"]) == \
        (None, 0., 100, True, None, 20000)
    assert "compute_occupancy_probability_for_supervision" in patch._HELPERS_ALL["utility.macarons_utils"][1]
    assert all("compute_occupancy_probability_for_supervision" not in v[1] for v in patch._HELPERS.values())     # opt-in tier only
    for n in ("mcr_supervision_select", "mcr_supervision_select_workspace_bytes", "mcr_supervision_scatter",
              "mcr_supervision_scatter_backward"):
        assert n in _lib.declared_symbols()
    assert hasattr(autograd, "SupervisionScatterFunction") and hasattr(ops, "supervision_select")


@needs_reference
def test_signature_extends_the_reference():
    """patch._signature_extends accepts the function against the reference's, and helpers="all" installs it (own interpreter: the swap
    edits sys.modules)."""
    code = f"""
    import sys, os, importlib
    sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests", "golden"))
    import _ref_import
    _ref_import.install_stubs()
    import macarons_amd
    from macarons_amd import patch
    mine = importlib.import_module("macarons_amd.utility.macarons_utils")
    ref = importlib.import_module("macarons.utility.macarons_utils")
    ref_fn = ref.compute_occupancy_probability_for_supervision
    assert ref_fn.__module__ == ref.__name__
    assert patch._signature_extends(ref_fn, mine.compute_occupancy_probability_for_supervision)
    rep = macarons_amd.patch_reference()
    assert ref.compute_occupancy_probability_for_supervision is ref_fn                       # not in the default tier
    rep = macarons_amd.patch_reference(helpers="all")
    assert ref.compute_occupancy_probability_for_supervision is mine.compute_occupancy_probability_for_supervision
    assert ("macarons.utility.macarons_utils", "compute_occupancy_probability_for_supervision") in rep["helpers"]
    macarons_amd.unpatch_reference()
    assert ref.compute_occupancy_probability_for_supervision is ref_fn
    print("__OK__")
    """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "__OK__" in r.stdout, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
