"""The reconstruction loss's kernels (reconstruction_loss.hip) on the paths that the goldens' shapes and the 32 x 456 case do not reach,
both ways, against the fp64 model (tests/_reconstruction_model.py) on the seeded cases of tests/_depth_loss_cases.py:

  rl_finish_kernel, tile loop      a lane's second step, t += 64: tiles66 (32 x 528, 66 tiles); also with ssim_factor = 0
  rl_finish_kernel, pair loop      a wave's second round, i += 4, and its i * n_tiles offsets: pairs6 (S B = 6, 4 tiles an image)
  rl_mask_count_kernel             a thread's second step, i += 256, on which the backward's 1 / (cnt + 1e-7) rests: tiles66 with its
                                   mask (16 896 pixels, 264 a chunk); also with ssim_factor = 0
  a fully masked image in a batch  0 / (0 + 1e-7) forward, a norm of 1e7 times gates that are all 0 backward: pairs6_dark (image 1)
  the backward's reflections       cys with three entries, H = 3: rows3 (row 1 is pixel 1 and pixel H - 2); a tile whose single spill row
  (cys / cxs, rl_warp_region<2>)   or column is the image's last one, its reflected partner in the previous tile: spill1 (17 x 33);
                                   a two-column spill: rows3 (3 x 18)

Bound: the project's contract, TOL = 1e-4 of the reference's largest magnitude (tests/test_reconstruction_loss_gpu.py), for loss, the
per-pixel map and d_depth, d_loss non-uniform over the scales.  As there, the model's d_depth follows the kernel's index map (either
source is a valid subgradient at a near-tie) and the kernel's index must equal the model's wherever the model's margin is at least 1e-3
of the map's maximum; tiles66 compares d_depth away from kinks by test_upstream_width's rule.  tests/test_reconstruction_loss_cpu.py
asserts the caps on near-ties (5 %) and kinks (2 %) from the model alone.  Every distance is printed with an ERR prefix before it is
asserted; NOTES.md ("Depth module: the reconstruction loss", Edges) records them.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _depth_loss_cases as edge                                       # noqa: E402
import _reconstruction_model as model                                  # noqa: E402
from _reconstruction_model import rel                                  # noqa: E402
from test_reconstruction_loss_gpu import TOL, _run                     # noqa: E402

pytestmark = pytest.mark.gpu

ALL = [(t, p, m) for t in edge.RECONSTRUCTION_TAGS for p, m in edge.RECONSTRUCTION_VARIANTS[t]]


@pytest.fixture(scope="module")
def cases():
    return {t: edge.reconstruction_case(t) for t in edge.RECONSTRUCTION_TAGS}


@pytest.fixture(scope="module")
def modelled(cases):
    """The fp64 model's forward of every variant, computed once and never changed."""
    out = {}
    for t, p, m in ALL:
        c = cases[t]
        with torch.no_grad():
            out[t, p, m] = model.reconstruction(*edge.model_args(c, m), c["depth"], c["zfar"], c["ssim_factor"], p)
    return out


def _compare(what, c, m, got, d_loss, padding, masked, away_from_kinks):
    """loss, map, index and d_depth of one call against the model's forward m; returns nothing, asserts the contract."""
    loss, lmap, idx, grad = got
    S = c["depth"].shape[0]
    assert loss.dtype == lmap.dtype == grad.dtype == torch.float32 and idx.dtype == torch.uint8
    assert tuple(loss.shape) == (S,) and lmap.shape == idx.shape == grad.shape == c["depth"].shape
    ref = model.gradient(*edge.model_args(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding, d_loss=d_loss, force_index=idx)
    clear = m["margin"] >= edge.NEAR_TIE * float(m["map"].max())
    e = (grad.double() - ref).abs() / ref.abs().max()
    e_loss, e_map, e_all = rel(loss, m["loss"]), rel(lmap, m["map"]), float(e.max())
    msg = f"ERR {what} {padding} mask={masked}, entry vs model: loss {e_loss:.2e} map {e_map:.2e} d_depth {e_all:.2e}"
    e_grad = e_all
    if away_from_kinks:
        kink = edge.kinks(c, m)
        e_grad = float(e[~kink[None].expand_as(e)].max())
        msg += (f" (away from kinks {e_grad:.2e}; beyond 1e-4: {int((e > TOL).sum())}, of them at a kink {int(((e > TOL) & kink[None]).sum())}; "
                f"kink pixels {100 * float(kink.double().mean()):.2f} %)")
        assert float(kink.double().mean()) <= edge.MAX_KINKS
    print(msg + f"; index differences {int((idx.long() != m['index']).sum())} (all pixels), "
          f"{int((idx.long() != m['index'])[clear].sum())} (clear margin)")
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(lmap).all()) and bool(torch.isfinite(grad).all())
    assert e_loss < TOL and e_map < TOL and e_grad < TOL
    assert bool((idx.long() == m["index"])[clear].all())


# ---- 1. every case, both paddings, with and without its mask, against the model ---------------------------------------------------------
@pytest.mark.parametrize("tag,padding,masked", ALL)
def test_entry_matches_model(dev, cases, modelled, tag, padding, masked):
    """tiles66: the second step of rl_finish_kernel's tile loop, and with the mask of rl_mask_count_kernel's thread loop (the backward's
    norm).  pairs6: the second round of rl_finish_kernel's pair loop.  pairs6_dark: a fully masked image in a batch -- its d_depth is
    exactly 0 and the loss is the model's.  spill1: a tile row and a tile column that hold only the image's last row / column.  rows3:
    H = 3, row 1 takes both reflections; a two-column spill."""
    c, m = cases[tag], modelled[tag, padding, masked]
    d_loss = edge.D_LOSS[c["depth"].shape[0]]
    got = _run(c, dev, padding, masked, d_loss)
    _compare(f"case {tag}", c, m, got, d_loss, padding, masked, away_from_kinks=tag == "tiles66")
    if tag == "pairs6_dark":
        assert bool((got[3][:, 1] == 0).all()) and bool((got[3][:, 0] != 0).any())


# ---- 2. tiles66 where the SSIM part is skipped -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding,masked", [(p, m) for p in ("border", "zeros") for m in (True, False)])
def test_tiles66_l1_only(dev, cases, padding, masked):
    """ssim_factor = 0 at 66 tiles and 264 mask pixels a chunk: rl_finish_kernel's tile loop and rl_mask_count_kernel's thread loop on
    the path without the SSIM part.  Without the mask too: there a tile's sum that is left out is not hidden by its count that is left
    out with it."""
    c = dict(cases["tiles66"], ssim_factor=0.0)
    with torch.no_grad():
        m = model.reconstruction(*edge.model_args(c, masked), c["depth"], c["zfar"], 0.0, padding)
    assert edge.near_tie_share(m) <= edge.MAX_NEAR_TIES                 # a condition on the inputs, from the model alone
    d_loss = edge.D_LOSS[1]
    _compare("case tiles66, ssim_factor 0,", c, m, _run(c, dev, padding, masked, d_loss), d_loss, padding, masked, away_from_kinks=True)


# ---- 3. the same bits: a scale of six pairs against its own call, an image beside a dark one against its own call -------------------------
@pytest.mark.parametrize("padding,masked", (("border", True), ("zeros", False)))
def test_pairs6_scales_have_the_bits_of_one_scale_calls(dev, cases, padding, masked):
    """S B = 6: the pairs of rl_finish_kernel's second round (scale 2) give the bits of a call that holds that scale alone, as do the
    first round's; two calls give the same bits."""
    c = cases["pairs6"]
    d_loss = edge.D_LOSS[3]
    one, two = _run(c, dev, padding, masked, d_loss), _run(c, dev, padding, masked, d_loss)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    for k in range(3):
        single = _run(dict(c, depth=c["depth"][k:k + 1].contiguous()), dev, padding, masked, d_loss[k:k + 1])
        for a, b in zip(one, single):
            assert torch.equal(a[k:k + 1], b)


@pytest.mark.parametrize("padding", ("border", "zeros"))
def test_pairs6_dark_normalisation_is_each_images_own(dev, cases, padding):
    """A masked image's normalisation is its own: beside a fully masked image 1 (count 0, norm 1e7, every gate 0), image 0's map, index
    and d_depth have the bits of the B = 1 call on image 0 alone, and so has the loss (image 1 adds 0 / 1e-7 = 0)."""
    c = cases["pairs6_dark"]
    d_loss = edge.D_LOSS[3]
    loss, lmap, idx, grad = _run(c, dev, padding, True, d_loss)
    alone = dict(c, **{k: c[k][:1].contiguous() for k in ("images", "alpha_images", "mask", "R", "T", "R_alpha", "T_alpha")},
                 depth=c["depth"][:, :1].contiguous())
    loss0, lmap0, idx0, grad0 = _run(alone, dev, padding, True, d_loss)
    assert bool((grad[:, 1] == 0).all()) and bool((grad0 != 0).any())
    assert torch.equal(grad[:, :1], grad0) and torch.equal(lmap[:, :1], lmap0) and torch.equal(idx[:, :1], idx0)
    assert torch.equal(loss, loss0)
