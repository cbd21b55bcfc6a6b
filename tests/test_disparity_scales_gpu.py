"""The fused disparity-scales step on the GPU (disparity_scales.hip: mcr_disparity_scales and mcr_disparity_scales_backward behind
ops.disparity_scales, ops.disparity_scales_backward, autograd.DisparityScalesFunction and utility.macarons_utils.depth_scale_losses)
against the independent fp64 model (tests/_disparity_model.py) and the reference's own functions (tests/golden/disparity_scales.npz).

Bounds.  Against the model: the project's contract, TOL = 1e-4 of the largest magnitude (`rel` of tests/_reconstruction_model.py), for
depth, reg, tab, thr and every d_disp_s, the backward run three ways (both halves, d_depth only, d_reg only).  Against the golden: TOL plus
the golden's own distance to the model, which its generator stored.  The error mask must equal the model's at every pixel that is not
undecided (|tab - thr| < 1e-4 thr in the model).  Case f (256 x 456, upstream's size) has no golden and is held against the model alone.

Masked-out pixels and the regularity half.  The mean mu of the normalisation is taken over ALL pixels of an image, masked-out ones
included (upstream normalises before it zeroes), so every pixel of an image receives the derivative through the mean,
-sum m G D / ((mu + eps)^2 H_s W_s), and a masked-out pixel receives nothing else.  What is exact is therefore asserted exactly: at every
scale of ratio 1 all masked-out pixels of an image hold one and the same bit pattern (their own term is exactly 0), that value is the
model's, and an image that is fully masked (case e, image 1) has a regularity gradient of exactly 0.

Every distance is printed with an ERR prefix before it is asserted.  Measured on an MI355X, worst of cases a-f against the model: depth
7.5e-08, reg 6.9e-08, tab 2.8e-06 (case a without a mask, 1.6e-07 elsewhere), thr 9.1e-08, d_disp 3.1e-07 / 2.8e-07 / 3.0e-07 (both halves /
depth / reg); no decided error-mask pixel differs; depth_scale_losses against the fp64 composite chain: d_disp 5.1e-06.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _disparity_model as model                                       # noqa: E402
import _reconstruction_model as rmodel                                 # noqa: E402
from _reconstruction_model import rel                                  # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402
from macarons_amd.utility import macarons_utils as mu                  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
ALL = model.VARIANTS + [("f", True)]


def t(x):
    return torch.as_tensor(np.asarray(x))


@pytest.fixture(scope="module")
def cases():
    out = {tag: model.load_case(tag) for tag in model.GOLDEN_TAGS}
    out["f"] = model.make_inputs("f")
    return out


@pytest.fixture(scope="module")
def weights(cases):
    """The upstream gradients (c [S] for reg, g [S,B,H,W] for depth) of every variant: the golden's, and seeded ones for case f."""
    out = {}
    for tag, masked in model.VARIANTS:
        want = model.load_result(tag, masked)
        out[tag, masked] = (want["c"], want["g"])
    B, H, W = cases["f"]["mask"].shape
    out["f", True] = model.upstream_weights(np.random.default_rng(106), len(cases["f"]["disps"]), B, H, W)
    return out


@pytest.fixture(scope="module")
def modelled(cases, weights):
    """The fp64 model of every variant -- forward, undecided pixels, and the gradient three ways -- computed once and never changed."""
    out = {}
    for tag, masked in ALL:
        c = cases[tag]
        mask = c["mask"] if masked else None
        m = model.forward(c["disps"], c["images"], mask)
        m["undecided"] = model.conditions(c["disps"], c["images"], mask)[3]
        cr, g = weights[tag, masked]
        m["grads"] = {"both": model.gradient(c["disps"], c["images"], mask, g, cr), "depth": model.gradient(c["disps"], c["images"], mask, g, None),
                      "reg": model.gradient(c["disps"], c["images"], mask, None, cr)}
        out[tag, masked] = m
    return out


def _on(c, dev, masked):
    return [t(d).to(dev) for d in c["disps"]], t(c["images"]).to(dev), t(c["mask"]).to(dev) if masked else None


def _backward3(disps, images, mask, cr, g, dev):
    cr, g = t(cr).to(dev), t(g).to(dev)
    return {"both": ops.disparity_scales_backward(disps, images, mask, model.ZNEAR, model.ZFAR, g, cr),
            "depth": ops.disparity_scales_backward(disps, images, mask, model.ZNEAR, model.ZFAR, g, None),
            "reg": ops.disparity_scales_backward(disps, images, mask, model.ZNEAR, model.ZFAR, None, cr)}


# ---- 1. the entries against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,masked", ALL)
def test_entries_match_model(dev, cases, weights, modelled, tag, masked):
    c, m = cases[tag], modelled[tag, masked]
    disps, images, mask = _on(c, dev, masked)
    depth, reg, em, tab, thr = ops.disparity_scales(disps, images, mask, model.ZNEAR, model.ZFAR, return_tab=True)
    S, (B, H, W) = len(disps), c["mask"].shape
    assert depth.dtype == reg.dtype == tab.dtype == thr.dtype == torch.float32 and em.dtype == torch.bool
    assert tuple(depth.shape) == (S, B, H, W) and tuple(reg.shape) == (S,) and tuple(em.shape) == tuple(tab.shape) == (B, H, W)
    assert tuple(thr.shape) == (B,)
    e = dict(depth=rel(depth, t(m["depth"])), reg=rel(reg, t(m["reg"])), tab=rel(tab, t(m["tab"])), thr=rel(thr, t(m["thr"])))
    wrong = int(((em.cpu().numpy() != m["error_mask"]) & ~m["undecided"]).sum())
    grads = _backward3(disps, images, mask, *weights[tag, masked], dev)
    for how, gs in grads.items():
        assert all(g.dtype == torch.float32 and tuple(g.shape) == d.shape and bool(torch.isfinite(g).all()) for g, d in zip(gs, c["disps"]))
        e["d_disp " + how] = max(rel(g, t(r)) for g, r in zip(gs, m["grads"][how]))
    print(f"ERR case {tag} mask={masked}, entries vs model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
          + f"; decided error-mask pixels that differ {wrong}, undecided {int(m['undecided'].sum())}")
    assert max(e.values()) < TOL
    assert wrong == 0
    # the regularity half at masked-out pixels: nothing but the image-wide derivative through the mean (module docstring)
    if masked:
        for s, r in enumerate(model.CASES[tag]["ratios"]):
            if r != 1:
                continue
            for b in range(B):
                hole = ~t(c["mask"][b])
                vals = grads["reg"][s][b].cpu()[hole]
                if bool(hole.all()):
                    assert bool((vals == 0).all())
                elif bool(hole.any()):
                    assert bool((vals == vals[0]).all()) and not bool((grads["reg"][s][b].cpu()[~hole] == vals[0]).all())


def test_fully_masked_image(dev, cases):
    """Case e: image 1 is fully masked -- tab = 0, error_mask all false, no contribution to reg, regularity gradient exactly 0."""
    c = cases["e"]
    disps, images, mask = _on(c, dev, True)
    depth, reg, em, tab, thr = ops.disparity_scales(disps, images, mask, model.ZNEAR, model.ZFAR, return_tab=True)
    assert bool((tab[1] == 0).all()) and float(thr[1]) == 0 and not bool(em[1].any()) and bool(em[0].any()) and not bool(em[0].all())
    alone = ops.disparity_scales([disps[0][:1].contiguous()], images[:1].contiguous(), mask[:1].contiguous(), model.ZNEAR, model.ZFAR)[1]
    assert rel(2 * reg, alone) < 1e-6                                   # image 1 adds nothing to the sums, only to the count
    g = ops.disparity_scales_backward(disps, images, mask, model.ZNEAR, model.ZFAR, None, torch.ones(1, device=dev))[0]
    assert bool((g[1] == 0).all()) and bool((g[0] != 0).any())


# ---- 2. the entries against the reference's own functions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,masked", model.VARIANTS)
def test_entries_match_golden(dev, cases, modelled, tag, masked):
    c, want = cases[tag], model.load_result(tag, masked)
    disps, images, mask = _on(c, dev, masked)
    depth, reg, em, tab, thr = ops.disparity_scales(disps, images, mask, model.ZNEAR, model.ZFAR, return_tab=True)
    grads = ops.disparity_scales_backward(disps, images, mask, model.ZNEAR, model.ZFAR, t(want["g"]).to(dev), t(want["c"]).to(dev))
    e = dict(depth=rel(depth, t(want["depth"])), reg=rel(reg, t(want["reg"])), tab=rel(tab, t(want["tab"])), thr=rel(thr, t(want["thr"])),
             d_disp=max(rel(g, t(r)) for g, r in zip(grads, want["d_disp"])))
    print(f"ERR case {tag} mask={masked}, entries vs golden: " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
          + " (golden vs model: " + " ".join(f"{k} {v:.1e}" for k, v in want["distance"].items()) + ")")
    for k, v in e.items():
        assert v < TOL + want["distance"][k], k
    assert bool(((em.cpu().numpy() == want["error_mask"]) | modelled[tag, masked]["undecided"]).all())


# ---- 3. the same bits on every call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,masked", ALL)
def test_two_calls_give_the_same_bits(dev, cases, weights, tag, masked):
    disps, images, mask = _on(cases[tag], dev, masked)
    one = ops.disparity_scales(disps, images, mask, model.ZNEAR, model.ZFAR, return_tab=True)
    two = ops.disparity_scales(disps, images, mask, model.ZNEAR, model.ZFAR, return_tab=True)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    b1 = _backward3(disps, images, mask, *weights[tag, masked], dev)
    b2 = _backward3(disps, images, mask, *weights[tag, masked], dev)
    assert all(torch.equal(a, b) for k in b1 for a, b in zip(b1[k], b2[k]))


# ---- 4. the depth goes straight into the reconstruction loss ----------------------------------------------------------------------------------
def test_depth_feeds_the_reconstruction_loss_without_a_copy(dev):
    rc = rmodel.load_case("a")                                          # 20 x 28, two sources
    B, A, H, W, _ = rc["alpha_images"].shape
    rng = np.random.default_rng(31)
    disps = [t(model.smooth_disparity(rng, B, H // r, W // r)).to(dev) for r in (1, 2, 4)]
    depth = ops.disparity_scales(disps, rc["images"].to(dev), rc["mask"].to(dev), 0.5, rc["zfar"])[0]
    assert depth.is_contiguous() and tuple(depth.shape) == (3, B, H, W) and depth.dtype == torch.float32
    cams = ManyDepth.pack_cameras(rc["R"], rc["T"], rc["R_alpha"], rc["T_alpha"]).to(dev)
    args = ops._reconstruction_args(rc["images"].to(dev), rc["alpha_images"].to(dev), rc["mask"].to(dev), cams, depth, "border")
    assert args[4].data_ptr() == depth.data_ptr()                      # what the entry is handed is the tensor itself
    loss = ops.reconstruction_loss(rc["images"].to(dev), rc["alpha_images"].to(dev), rc["mask"].to(dev), cams, depth, rc["zfar"],
                                   rc["ssim_factor"], "border")
    want = ManyDepth.reconstruction_loss_composite(rc["images"], rc["alpha_images"], rc["mask"], cams.cpu(), depth.cpu(), rc["zfar"],
                                                   rc["ssim_factor"], "border")
    assert rel(loss, want) < TOL


# ---- 5. the autograd function, both routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["hip", "composite"])
@pytest.mark.parametrize("tag,masked", [("a", True), ("a", False), ("c", True)])
def test_function_on_both_routes(dev, cases, weights, modelled, monkeypatch, route, tag, masked):
    if route == "composite":
        monkeypatch.setenv("MCR_DISPARITY_SCALES_BWD", "composite")
    else:
        monkeypatch.delenv("MCR_DISPARITY_SCALES_BWD", raising=False)
    assert autograd.disparity_scales_backward_mode() == route
    c, m = cases[tag], modelled[tag, masked]
    disps, images, mask = _on(c, dev, masked)
    cr, g = (t(w).to(dev) for w in weights[tag, masked])
    leaves = [d[:, None].clone().requires_grad_(True) for d in disps]   # [B,1,H_s,W_s], as the network returns them
    depth, reg, em = autograd.DisparityScalesFunction.apply(images, mask, model.ZNEAR, model.ZFAR, *leaves)
    assert depth.requires_grad and reg.requires_grad and not em.requires_grad and em.dtype == torch.bool
    for how, loss in (("both", (reg * cr).sum() + (depth * g).sum()), ("depth", (depth * g).sum()), ("reg", (reg * cr).sum())):
        grads = torch.autograd.grad(loss, leaves, retain_graph=True)
        assert all(gr.shape == leaf.shape for gr, leaf in zip(grads, leaves))
        e = max(rel(gr[:, 0], t(r)) for gr, r in zip(grads, m["grads"][how]))
        print(f"ERR case {tag} mask={masked}, DisparityScalesFunction ({route}) {how}: d_disp {e:.2e}")
        assert e < TOL
    only_coarse = torch.autograd.grad(reg.sum(), leaves[-1], retain_graph=True)[0]     # one input of S: the others get None
    assert only_coarse.shape == leaves[-1].shape
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(reg.sum(), leaves, create_graph=True)


# ---- 6. a whole depth step: depth_scale_losses --------------------------------------------------------------------------------------------------
def test_depth_scale_losses_backward(dev, cases):
    """Case a through depth_scale_losses (one DisparityScalesFunction call, one reconstruction_losses call) against the fp64 composite
    chain, disparity_scales_composite followed by reconstruction_loss_composite.  One source per image: the minimum over several sources
    is selected differently by two evaluations at a near-tie, which is the reconstruction loss's tests' subject, not this one's."""
    c = cases["a"]
    rc = rmodel.load_case("a")                                          # its target and first-source poses
    B, H, W = c["mask"].shape
    alpha = t(model.smooth_images(np.random.default_rng(41), B, H, W))[:, None]
    params = SimpleNamespace(znear=model.ZNEAR, zfar=model.ZFAR, ssim_factor=0.85, use_depth_mask=True, regularity_loss=True, regularity_factor=1.0)
    R, T, Ra, Ta = rc["R"], rc["T"], rc["R_alpha"][:, :1], rc["T_alpha"][:, :1] * 0.2
    cameras = SimpleNamespace(R=R.to(dev), T=T.to(dev))
    alpha_cameras = SimpleNamespace(R=Ra.reshape(-1, 3, 3).to(dev), T=Ta.reshape(-1, 3).to(dev))
    leaves = [t(d)[:, None].to(dev).requires_grad_(True) for d in c["disps"]]
    dl, rl, depth, mask, em = mu.depth_scale_losses(params, leaves, t(c["images"]).to(dev), alpha.to(dev), t(c["mask"]).to(dev)[..., None],
                                                    cameras, alpha_cameras, "border")
    (dl + rl).backward()
    assert tuple(depth.shape) == tuple(mask.shape) == tuple(em.shape) == (B, H, W, 1) and not depth.requires_grad
    ref = [t(d).double().requires_grad_(True) for d in c["disps"]]
    d6, r6, e6 = ManyDepth.disparity_scales_composite(ref, t(c["images"]), t(c["mask"]), model.ZNEAR, model.ZFAR)
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta).double()
    l6 = ManyDepth.reconstruction_loss_composite(t(c["images"]), alpha, t(c["mask"]), cams, d6, model.ZFAR, 0.85, "border")
    want_reg = sum(r6[s] * 0.5 ** s for s in range(len(ref)))
    (l6.sum() + want_reg).backward()
    e = dict(depth_loss=rel(dl, l6.sum()), regularity_loss=rel(rl, want_reg), depth=rel(depth[..., 0], d6[0]),
             d_disp=max(rel(a.grad[:, 0], b.grad) for a, b in zip(leaves, ref)))
    print("ERR case a, depth_scale_losses vs the fp64 composite chain: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < TOL
    undecided = model.conditions(c["disps"], c["images"], c["mask"])[3]
    assert bool(((em[..., 0].cpu() == e6) | t(undecided)).all())
    # the forward alone
    out = mu.depth_scale_losses(params, [leaf.detach() for leaf in leaves], t(c["images"]).to(dev), alpha.to(dev), t(c["mask"]).to(dev)[..., None],
                                cameras, alpha_cameras, "border", compute_loss=False)
    assert out[0] == 0. and out[1] == 0. and torch.equal(out[2], depth) and torch.equal(out[4], em)
    # without the regularity loss that half is 0. and its backward is skipped: the gradient is the depth loss's alone
    params.regularity_loss = False
    again = [leaf.detach().clone().requires_grad_(True) for leaf in leaves]
    dl2, rl2, *_ = mu.depth_scale_losses(params, again, t(c["images"]).to(dev), alpha.to(dev), t(c["mask"]).to(dev)[..., None], cameras,
                                         alpha_cameras, "border")
    assert rl2 == 0. and isinstance(rl2, float)
    dl2.backward()
    for b in ref:
        b.grad = None
    d6, _, _ = ManyDepth.disparity_scales_composite(ref, t(c["images"]), t(c["mask"]), model.ZNEAR, model.ZFAR)
    ManyDepth.reconstruction_loss_composite(t(c["images"]), alpha, t(c["mask"]), cams, d6, model.ZFAR, 0.85, "border").sum().backward()
    assert max(rel(a.grad[:, 0], b.grad) for a, b in zip(again, ref)) < TOL


# ---- 7. the C entries refuse before they launch ------------------------------------------------------------------------------------------------
def test_c_entries_refuse_without_launching(dev):
    L = _lib.lib()
    B, H, W = 1, 8, 16
    full, half = torch.full((B, H, W), 0.5, device=dev), torch.full((B, 4, 8), 0.5, device=dev)
    images = torch.full((B, H, W, 3), 0.5, device=dev)
    outs = dict(depth=torch.full((2, B, H, W), -7.0, device=dev), reg=torch.full((2,), -7.0, device=dev),
                em=torch.full((B, H, W), 7, dtype=torch.uint8, device=dev), g0=torch.full((B, H, W), -7.0, device=dev),
                g1=torch.full((B, 4, 8), -7.0, device=dev))
    d_reg = torch.ones(2, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    i64, ci, cf, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p

    def call(S=2, hs=(8, 4), wss=(16, 8), H_=H, W_=W, znear=0.5, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), back=False, d_reg_ptr=d_reg.data_ptr()):
        n = max(len(hs), 1)
        ptrs = (vp * n)(*([full.data_ptr(), half.data_ptr()] * 5)[:n])
        gptrs = (vp * n)(*([outs["g0"].data_ptr(), outs["g1"].data_ptr()] * 5)[:n])
        a_hs, a_ws = (ci * n)(*hs), (ci * n)(*wss)
        if back:
            return L.mcr_disparity_scales_backward(ptrs, a_hs, a_ws, vp(images.data_ptr()), None, None, vp(d_reg_ptr) if d_reg_ptr else None,
                                                   gptrs, ci(S), i64(B), ci(H_), ci(W_), cf(znear), cf(750.0), vp(ws_ptr), ctypes.c_size_t(ws_bytes),
                                                   None)
        return L.mcr_disparity_scales(ptrs, a_hs, a_ws, vp(images.data_ptr()), None, vp(outs["depth"].data_ptr()), vp(outs["reg"].data_ptr()),
                                      vp(outs["em"].data_ptr()), None, None, ci(S), i64(B), ci(H_), ci(W_), cf(znear), cf(750.0), vp(ws_ptr),
                                      ctypes.c_size_t(ws_bytes), None)

    refused = [dict(S=0), dict(S=9, hs=(8,) * 9, wss=(16,) * 9), dict(H_=1, hs=(1, 1), wss=(16, 8)), dict(W_=1, hs=(8, 4), wss=(1, 1)),
               dict(hs=(8, 3), wss=(16, 6)),                            # 8 rows is no multiple of 3
               dict(H_=12, hs=(12, 4), wss=(16, 8)),                    # ratio 3 down, 2 across
               dict(H_=96, W_=192, hs=(96, 3), wss=(192, 6)),           # ratio 32
               dict(hs=(8, 4), wss=(16, 7)),                            # a mismatched width
               dict(znear=0.0), dict(ws_bytes=64), dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=ws.numel() - 4)]
    for back in (False, True):
        for kw in refused:
            assert call(back=back, **kw) == 1, (back, kw)
            assert L.mcr_last_error().decode().startswith("mcr_disparity_scales"), kw
    assert call(back=True, d_reg_ptr=None) == 1 and "both NULL" in L.mcr_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((v == (7 if v.dtype == torch.uint8 else -7.0)).all()) for v in outs.values())       # nothing was launched
    assert call() == 0 and call(back=True) == 0                         # and the same calls, well-formed, run
    torch.cuda.synchronize()
    assert bool((outs["depth"] > 0).all()) and bool((outs["em"] <= 1).all()) and bool((outs["g0"] != -7.0).all())
