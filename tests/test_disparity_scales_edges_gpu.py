"""The disparity-scales kernels (disparity_scales.hip) on the paths that cases a-f do not reach, both ways, against the fp64 model
(tests/_disparity_model.py) on the seeded cases of tests/_depth_loss_cases.py:

  ratio 16 (DS_MAX_SHIFT = 4)      ds_backward_kernel's nb = 1, one thread sums a whole 16 x 16 tile: s8, r16row, tiles65, flat; a coarse
                                   map of one row, H_s = 1: r16row
  more than four scales            redf[wave][S + s] / part_reg[.. 2S + k], the LDS planes nrm[s DS_R] and val[s 256], thread s of
                                   ds_means, at S = 8 = DS_MAX_S: s8 (and S = 5: tiles65)
  scale 0 not the finest           the table, its threshold and the error mask come from scale 0 whatever its ratio: coarse0 (16, 1, 4)
  B > 1 with more than 64 tiles    ds_finish_kernel's (b n_tiles + t) with t += 64, ds_backward_mean_kernel for image 1: tiles65
                                   (80 x 208, 65 tiles, B = 2)
  exact degenerate inputs          a constant map (every difference exactly 0, sign(0) = 0 on both sides) and an all-zero map
                                   (den = 1e-7f): flat

Bound: the project's contract, TOL = 1e-4 of the reference's largest magnitude (tests/test_disparity_scales_gpu.py), for depth, reg,
tab, thr and every d_disp_s, the backward run three ways (both halves, d_depth only, d_reg only); the error mask must equal the model's
at every pixel that is not undecided.  tests/test_disparity_scales_cpu.py asserts the golden generator's conditions on these inputs from
the model alone.  What is exact is asserted exactly.  Every distance is printed with an ERR prefix before it is asserted; NOTES.md
("Depth module: disparity scales, regularity values and error mask", Edges) records them.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _depth_loss_cases as edge                                       # noqa: E402
import _disparity_model as model                                       # noqa: E402
from _reconstruction_model import rel                                  # noqa: E402
from test_disparity_scales_gpu import TOL, _backward3, _on, t          # noqa: E402

from macarons_amd import ops                                           # noqa: E402

pytestmark = pytest.mark.gpu

HOWS = ("both", "depth", "reg")
MODELLED = [(tag, m) for tag, m in edge.DISPARITY_VARIANTS if tag != "flat"]


@pytest.fixture(scope="module")
def cases():
    return {tag: edge.disparity_inputs(tag) for tag in edge.DISPARITY_TAGS}


@pytest.fixture(scope="module")
def weights():
    return {tag: edge.disparity_weights(tag) for tag in edge.DISPARITY_TAGS}


def _model(inp, mask, cr, g):
    m = model.forward(inp["disps"], inp["images"], mask)
    m["undecided"] = model.conditions(inp["disps"], inp["images"], mask)[3]
    m["grads"] = {"both": model.gradient(inp["disps"], inp["images"], mask, g, cr), "depth": model.gradient(inp["disps"], inp["images"], mask, g, None),
                  "reg": model.gradient(inp["disps"], inp["images"], mask, None, cr)}
    return m


@pytest.fixture(scope="module")
def modelled(cases, weights):
    """The fp64 model of every variant -- forward, undecided pixels, and the gradient three ways -- computed once and never changed."""
    return {(tag, masked): _model(cases[tag], cases[tag]["mask"] if masked else None, *weights[tag]) for tag, masked in edge.DISPARITY_VARIANTS}


def _forward(disps, images, mask):
    return ops.disparity_scales(disps, images, mask, model.ZNEAR, model.ZFAR, return_tab=True)


def _distances(what, inp, m, fwd, grads):
    """Prints and returns the distances of one forward and its three backwards to the model m, and the number of decided error-mask
    pixels that differ."""
    depth, reg, em, tab, thr = fwd
    S, (B, H, W) = len(inp["disps"]), inp["mask"].shape
    assert depth.dtype == reg.dtype == tab.dtype == thr.dtype == torch.float32 and em.dtype == torch.bool
    assert tuple(depth.shape) == (S, B, H, W) and tuple(reg.shape) == (S,) and tuple(em.shape) == tuple(tab.shape) == (B, H, W)
    assert tuple(thr.shape) == (B,)
    e = dict(depth=rel(depth, t(m["depth"])), reg=rel(reg, t(m["reg"])), tab=rel(tab, t(m["tab"])), thr=rel(thr, t(m["thr"])))
    wrong = int(((em.cpu().numpy() != m["error_mask"]) & ~m["undecided"]).sum())
    for how in HOWS:
        gs = grads[how]
        assert all(g.dtype == torch.float32 and tuple(g.shape) == d.shape and bool(torch.isfinite(g).all()) for g, d in zip(gs, inp["disps"]))
        e["d_disp " + how] = max(rel(g, t(r)) for g, r in zip(gs, m["grads"][how]))
    print(f"ERR {what}, entries vs model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
          + f"; decided error-mask pixels that differ {wrong}, undecided {int(m['undecided'].sum())}")
    return e, wrong


# ---- 1. every case and mask variant against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,masked", MODELLED)
def test_entries_match_model(dev, cases, weights, modelled, tag, masked):
    """s8: eight scales, ratio 16 twice, 2 x 3 tiles.  r16row: a coarse map of one row.  coarse0: the table and the error mask from a
    ratio-16 scale 0 (the model is fed the same order).  tiles65: 65 tiles with B = 2 in ds_finish_kernel, ds_backward_mean_kernel
    for image 1."""
    inp, m = cases[tag], modelled[tag, masked]
    disps, images, mask = _on(inp, dev, masked)
    fwd = _forward(disps, images, mask)
    grads = _backward3(disps, images, mask, *weights[tag], dev)
    e, wrong = _distances(f"case {tag} mask={masked}", inp, m, fwd, grads)
    assert max(e.values()) < TOL
    assert wrong == 0
    if masked:                                                          # a masked-out pixel of a ratio-1 scale: the image-wide term alone
        for s, r in enumerate(edge.DISPARITY[tag]["ratios"]):
            if r != 1:
                continue
            for b in range(inp["mask"].shape[0]):
                hole = ~t(inp["mask"][b])
                vals = grads["reg"][s][b].cpu()[hole]
                assert bool(hole.any()) and bool((vals == vals[0]).all()) and not bool((grads["reg"][s][b].cpu()[~hole] == vals[0]).all())


@pytest.mark.parametrize("tag,masked", edge.DISPARITY_VARIANTS)
def test_two_calls_give_the_same_bits(dev, cases, weights, tag, masked):
    disps, images, mask = _on(cases[tag], dev, masked)
    one, two = _forward(disps, images, mask), _forward(disps, images, mask)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    b1, b2 = _backward3(disps, images, mask, *weights[tag], dev), _backward3(disps, images, mask, *weights[tag], dev)
    assert all(torch.equal(a, b) for k in b1 for a, b in zip(b1[k], b2[k]))


# ---- 2. s8: each of the eight scales against a call that holds it alone ----------------------------------------------------------------------
@pytest.mark.parametrize("masked", (True, False))
def test_s8_scales_have_the_bits_of_one_scale_calls(dev, cases, weights, masked):
    """DS_MAX_S = 8 scales in one call: depth[s], reg[s] and d_disp_s (three ways) of every scale have the bits of a call with that scale
    alone -- a wrong plane, slot or stride at s = 4 .. 7 (redf[wave][S + s], part_reg[.. 2S + k], nrm[s DS_R], val[s 256], den[s]) would
    mix two scales, and the two ratio-1 and the two ratio-16 scales hold different maps.  The table belongs to scale 0: for s > 0 only
    the per-scale outputs are compared."""
    inp = cases["s8"]
    disps, images, mask = _on(inp, dev, masked)
    assert not torch.equal(disps[0], disps[1]) and not torch.equal(disps[6], disps[7])
    cr, g = weights["s8"]
    depth, reg, em, tab, thr = _forward(disps, images, mask)
    grads = _backward3(disps, images, mask, cr, g, dev)
    assert not torch.equal(depth[0], depth[1]) and not torch.equal(depth[6], depth[7]) and float(reg[0]) != float(reg[1])
    assert float(reg[6]) != float(reg[7])
    for s in range(len(disps)):
        d1, r1, em1, tab1, thr1 = _forward(disps[s:s + 1], images, mask)
        assert torch.equal(d1[0], depth[s]) and torch.equal(r1[0], reg[s]), s
        if s == 0:
            assert torch.equal(tab1, tab) and torch.equal(thr1, thr) and torch.equal(em1, em)
        g1 = _backward3(disps[s:s + 1], images, mask, cr[s:s + 1], g[s:s + 1], dev)
        for how in HOWS:
            assert torch.equal(g1[how][0], grads[how][s]), (s, how)


# ---- 3. coarse0: scale 0 is the first map, not the finest ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", (True, False))
def test_coarse0_table_is_scale_0s(dev, cases, weights, modelled, masked):
    """(16, 1, 4): tab, thr and the error mask are those of the model fed the same order (test_entries_match_model holds them within
    TOL) and NOT those of the order (1, 16, 4), neither the model's nor the entry's own: a kernel that picked scale 0 by resolution
    would fail here.  The per-scale outputs only move with their scale."""
    inp, m = cases["coarse0"], modelled["coarse0", masked]
    other = edge.reordered(inp, (1, 0, 2))
    m_other = model.forward(other["disps"], other["images"], other["mask"] if masked else None)
    disps, images, mask = _on(inp, dev, masked)
    depth, reg, em, tab, thr = _forward(disps, images, mask)
    depth2, reg2, em2, tab2, thr2 = _forward([disps[1], disps[0], disps[2]], images, mask)
    e = dict(tab=rel(tab, t(m["tab"])), thr=rel(thr, t(m["thr"])), tab_other=rel(tab, t(m_other["tab"])), thr_other=rel(thr, t(m_other["thr"])),
             tab_entry_other=rel(tab, tab2))
    decided = ~m["undecided"]
    print(f"ERR case coarse0 mask={masked}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
          + f"; error-mask pixels that differ between the two orders {int((em != em2).sum())}")
    assert e["tab"] < TOL and e["thr"] < TOL and not bool(((em.cpu().numpy() != m["error_mask"]) & decided).any())
    assert e["tab_other"] > 100 * TOL and e["thr_other"] > 100 * TOL and e["tab_entry_other"] > 100 * TOL
    assert int(((em.cpu().numpy() != m_other["error_mask"]) & decided).sum()) >= 16
    assert torch.equal(depth[[1, 0, 2]], depth2) and torch.equal(reg[[1, 0, 2]], reg2)


# ---- 4. flat: the exact zeros ----------------------------------------------------------------------------------------------------------------------
def test_flat_exact_zeros(dev, cases, weights, modelled):
    """Image 0 the constant 0.37 at ratios 1, 4 and 16: every difference is exactly 0 and sign(0) = 0 on both sides.  Image 1 all
    zeros: den = 1e-7f, n = 0 / 1e-7 = 0 and depth = 1 / b0.  So reg, tab and thr are exactly 0, no error-mask pixel is set, the
    regularity gradient is exactly 0 at every scale, and the depth half is finite and the model's."""
    inp, m = cases["flat"], modelled["flat", False]
    cr, g = weights["flat"]
    disps, images, mask = _on(inp, dev, False)
    depth, reg, em, tab, thr = _forward(disps, images, mask)
    grads = _backward3(disps, images, mask, cr, g, dev)
    assert bool((reg == 0).all()) and bool((tab == 0).all()) and bool((thr == 0).all()) and not bool(em.any())
    assert all(bool((gr == 0).all()) for gr in grads["reg"])
    b0 = np.float32(1.0) / np.float32(model.ZFAR)
    assert bool((depth[:, 1].cpu() == float(np.float32(1.0) / b0)).all())
    e = dict(depth=rel(depth, t(m["depth"])))
    for how in ("depth", "both"):
        assert all(bool(torch.isfinite(gr).all()) for gr in grads[how])
        e["d_disp " + how] = max(rel(gr, t(r)) for gr, r in zip(grads[how], m["grads"][how]))
    print("ERR case flat, entries vs model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < TOL
    assert all(torch.equal(a, b) for a, b in zip(grads["depth"], grads["both"]))      # the regularity half adds exact zeros
