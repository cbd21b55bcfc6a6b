"""The fused photometric reconstruction loss on the GPU (reconstruction_loss.hip: mcr_reconstruction_loss and
mcr_reconstruction_loss_backward behind ops.reconstruction_loss, ops.reconstruction_loss_backward, autograd.ReconstructionLossFunction
and utility.macarons_utils.get_reconstruction_loss_fn) against the independent fp64 model (tests/_reconstruction_model.py) and the
reference's own function (tests/golden/reconstruction_loss.npz).

Bounds.  Against the model: the project's contract, TOL = 1e-4 of the largest magnitude, for loss, the per-pixel map and d_depth; for
d_depth the model is forced to the kernel's index map (either source is a valid subgradient at a near-tie), and the kernel's index must
equal the model's wherever the model's margin is at least 1e-3 of the map's maximum.  Against the golden: TOL plus the golden's own
distance to the model, which its generator stored (the golden carries upstream's fp32 cancellation in E[y^2] - mu^2, the kernel's window
moments are centred); for d_depth the 3x3 neighbourhoods of pixels whose index differs from the golden's are left out, each such pixel
must have a margin below 1e-3 of the map's maximum and together they may cover at most 5 % of the image.  Every distance is printed with
an ERR prefix before it is asserted; NOTES.md ("Depth module: the reconstruction loss") records them.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _reconstruction_model as model                                  # noqa: E402
from _reconstruction_model import VARIANTS, load_case, load_result, rel  # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402
from macarons_amd.utility import macarons_utils as mu                  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
ALL = [(t, p, m) for t in "abcd" for p, m in VARIANTS[t]]


@pytest.fixture(scope="module")
def cases():
    return {t: load_case(t) for t in "abcd"}


@pytest.fixture(scope="module")
def modelled(cases):
    """The fp64 model's forward of every variant, computed once and never changed."""
    out = {}
    for t, p, m in ALL:
        c = cases[t]
        with torch.no_grad():
            out[t, p, m] = model.reconstruction(*_margs(c, m), c["depth"], c["zfar"], c["ssim_factor"], p)
    return out


def _margs(c, masked):
    return (c["images"], c["alpha_images"], c["mask"] if masked else None, c["R"], c["T"], c["R_alpha"], c["T_alpha"])


def _on(c, dev, masked):
    cams = ManyDepth.pack_cameras(c["R"], c["T"], c["R_alpha"], c["T_alpha"])
    return (c["images"].to(dev), c["alpha_images"].to(dev), c["mask"].to(dev) if masked else None, cams.to(dev), c["depth"].to(dev))


def _run(c, dev, padding, masked, d_loss=None):
    im, al, mk, cams, depth = _on(c, dev, masked)
    loss, lmap, idx = ops.reconstruction_loss(im, al, mk, cams, depth, c["zfar"], c["ssim_factor"], padding, return_map=True)
    g = torch.ones_like(loss) if d_loss is None else d_loss.to(dev)
    grad = ops.reconstruction_loss_backward(im, al, mk, cams, depth, g, c["zfar"], c["ssim_factor"], padding)
    return loss.cpu(), lmap.cpu(), idx.cpu(), grad.cpu()


# ---- 1. the entry against the model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,padding,masked", ALL)
def test_entry_matches_model(dev, cases, modelled, tag, padding, masked):
    c, m = cases[tag], modelled[tag, padding, masked]
    S = c["depth"].shape[0]
    d_loss = torch.linspace(0.5, 1.5, S) if S > 1 else torch.tensor([0.75])
    loss, lmap, idx, grad = _run(c, dev, padding, masked, d_loss)
    assert loss.dtype == lmap.dtype == grad.dtype == torch.float32 and idx.dtype == torch.uint8
    assert tuple(loss.shape) == (S,) and lmap.shape == idx.shape == grad.shape == c["depth"].shape
    ref = model.gradient(*_margs(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding, d_loss=d_loss, force_index=idx)
    clear = m["margin"] >= 1e-3 * float(m["map"].max())
    n_diff = int((idx.long() != m["index"]).sum())
    e_loss, e_map, e_grad = rel(loss, m["loss"]), rel(lmap, m["map"]), rel(grad, ref)
    print(f"ERR case {tag} {padding} mask={masked}, entry vs model: loss {e_loss:.2e} map {e_map:.2e} d_depth {e_grad:.2e}; "
          f"index differences {n_diff} (all pixels), {int((idx.long() != m['index'])[clear].sum())} (clear margin)")
    assert bool(torch.isfinite(grad).all())
    assert e_loss < TOL and e_map < TOL and e_grad < TOL
    assert bool((idx.long() == m["index"])[clear].all())


# ---- 2. the entry against the reference's own function ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,padding,masked", ALL)
def test_entry_matches_golden(dev, cases, modelled, tag, padding, masked):
    c, m, want = cases[tag], modelled[tag, padding, masked], load_result(tag, padding, masked)
    loss, lmap, idx, grad = _run(c, dev, padding, masked)
    g_loss, g_map, g_grad = (float(v) for v in want["distance"])
    differ = idx != want["index"]
    e_loss, e_map = rel(loss, want["loss"]), rel(lmap, want["map"])
    keep = 1.0 - F.max_pool2d(differ.float(), 3, 1, 1) if differ.shape[-2] >= 2 else 1.0 - differ.float()
    e_grad = float(((grad - want["d_depth"]).abs() * keep).max() / want["d_depth"].abs().max())
    print(f"ERR case {tag} {padding} mask={masked}, entry vs golden: loss {e_loss:.2e} map {e_map:.2e} d_depth {e_grad:.2e}; "
          f"index differences {int(differ.sum())} (golden vs model: {g_loss:.1e} {g_map:.1e} {g_grad:.1e})")
    assert e_loss < TOL + g_loss and e_map < TOL + g_map and e_grad < TOL + g_grad
    if bool(differ.any()):
        assert float(m["margin"][differ].max()) < 1e-3 * float(m["map"].max())
        assert float(differ.float().mean()) <= 0.05


# ---- 2b. the other paths of the kernels: no SSIM part, and the largest number of sources ----------------------------------------------------
def _check_against_model(what, c, dev, padding, masked):
    with torch.no_grad():
        m = model.reconstruction(*_margs(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding)
    loss, lmap, idx, grad = _run(c, dev, padding, masked)
    ref = model.gradient(*_margs(c, masked), c["depth"], c["zfar"], c["ssim_factor"], padding, force_index=idx)
    clear = m["margin"] >= 1e-3 * float(m["map"].max())
    e_loss, e_map, e_grad = rel(loss, m["loss"]), rel(lmap, m["map"]), rel(grad, ref)
    print(f"ERR {what}, entry vs model: loss {e_loss:.2e} map {e_map:.2e} d_depth {e_grad:.2e}; "
          f"index differences {int((idx.long() != m['index']).sum())}, sources selected {sorted(set(idx.flatten().tolist()))}")
    assert e_loss < TOL and e_map < TOL and e_grad < TOL and bool((idx.long() == m["index"])[clear].all())
    return idx


def test_l1_only(dev, cases):
    """ssim_factor = 0: the SSIM part is skipped, the loss is the L1 term alone."""
    c = dict(cases["b"], ssim_factor=0.0)
    for padding in ("border", "zeros"):
        _check_against_model(f"case b {padding}, ssim_factor 0", c, dev, padding, True)


def test_eight_sources(dev, cases):
    """A = 8, the entry's limit and the largest LDS footprint: case c's three sources, then five more made from them by shifting the image
    and moving the camera."""
    c = cases["c"]
    al, Ra, Ta = [c["alpha_images"]], [c["R_alpha"]], [c["T_alpha"]]
    for k in range(5):
        a = k % 3
        al.append(torch.roll(c["alpha_images"][:, a:a + 1], shifts=(k + 1, 2 * k + 3), dims=(2, 3)))
        Ra.append(c["R_alpha"][:, a:a + 1])
        Ta.append(c["T_alpha"][:, a:a + 1] + torch.tensor([0.05 * (k + 1), -0.04 * (k + 1), 0.03 * k]))
    c8 = dict(c, alpha_images=torch.cat(al, 1).contiguous(), R_alpha=torch.cat(Ra, 1).contiguous(), T_alpha=torch.cat(Ta, 1).contiguous())
    idx = _check_against_model("case c with 8 sources, border", c8, dev, "border", True)
    assert int(idx.max()) >= 3                                          # a source past the first three is selected somewhere


# ---- 2c. upstream's width ------------------------------------------------------------------------------------------------------------------
from _depth_loss_cases import wide_case as _wide_case                  # noqa: E402  (32 x 456 here; the edge tests use it at 32 x 528)


@pytest.mark.parametrize("padding", ("border", "zeros"))
def test_upstream_width(dev, padding):
    """32 x 456: the contract at upstream's width, where an fp32 pixel coordinate is spaced 3e-5 apart.  d_depth is compared away from
    kinks, by rule: an fp32 coordinate of magnitude up to max(H, W) that went through eight roundings is within delta = 8 x 2^-24 x
    max(H, W) = 2.2e-4 of the model's, so a pixel with a source sample within delta of a source pixel boundary may take the bilinear slope
    of either cell, and one with |I - Iw| below delta x (the steepest slope of the source images) + 4 x 2^-24 in a channel may take
    either sign of the L1 term; either is a valid fp32 value.  Such pixels may be 2 % of the image at the most."""
    c = _wide_case()
    H, W = c["depth"].shape[-2:]
    with torch.no_grad():
        m = model.reconstruction(*_margs(c, True), c["depth"], c["zfar"], c["ssim_factor"], padding)
    loss, lmap, idx, grad = _run(c, dev, padding, True)
    ref = model.gradient(*_margs(c, True), c["depth"], c["zfar"], c["ssim_factor"], padding, force_index=idx)
    delta = 8 * 2.0 ** -24 * max(H, W)
    al = c["alpha_images"].double()
    slope = max(float((al[:, :, 1:] - al[:, :, :-1]).abs().max()), float((al[:, :, :, 1:] - al[:, :, :, :-1]).abs().max()))
    xy, warped = m["parts"][0]["xy"], m["parts"][0]["warped"]
    kink = ((xy - xy.round()).abs() < delta).any(-1).any(1)
    kink |= ((c["images"].double()[:, None] - warped).abs() < delta * slope + 4 * 2.0 ** -24).any(-1).any(1)
    e = (grad.double() - ref).abs() / ref.abs().max()
    clear = m["margin"] >= 1e-3 * float(m["map"].max())
    e_loss, e_map, e_grad = rel(loss, m["loss"]), rel(lmap, m["map"]), float(e[~kink[None]].max())
    print(f"ERR 32x456 {padding}, entry vs model: loss {e_loss:.2e} map {e_map:.2e} d_depth away from kinks {e_grad:.2e} (all pixels "
          f"{float(e.max()):.2e}, beyond 1e-4: {int((e > TOL).sum())}, of them at a kink {int(((e > TOL) & kink[None]).sum())}); kink pixels "
          f"{100 * float(kink.double().mean()):.2f} %; index differences {int((idx.long() != m['index']).sum())}")
    assert float(kink.double().mean()) <= 0.02
    assert e_loss < TOL and e_map < TOL and e_grad < TOL and bool((idx.long() == m["index"])[clear].all())


# ---- 3. the same bits: two runs, S scales in one call against S calls ---------------------------------------------------------------------
def test_reproducible_and_scales_are_independent(dev, cases):
    c = cases["a"]
    d_loss = torch.tensor([0.5, 1.5])
    one, two = _run(c, dev, "border", True, d_loss), _run(c, dev, "border", True, d_loss)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    for k in range(2):
        single = _run(dict(c, depth=c["depth"][k:k + 1]), dev, "border", True, d_loss[k:k + 1])
        for a, b in zip(one, single):
            assert torch.equal(a[k:k + 1], b)


# ---- 4. the mask ------------------------------------------------------------------------------------------------------------------------
def test_masked_pixels_have_exactly_zero_gradient(dev, cases):
    c = cases["a"]
    masked, plain = _run(c, dev, "zeros", True), _run(c, dev, "zeros", False)
    hole = ~c["mask"][None].expand_as(masked[3])
    assert bool(hole.any()) and bool((masked[3][hole] == 0).all()) and bool((masked[3][~hole] != 0).any())
    assert not torch.equal(masked[0], plain[0]) and not torch.equal(masked[1], plain[1]) and bool((plain[3][hole] != 0).any())


# ---- 5. upstream's interface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", (True, False))
def test_returned_function_gives_the_entry_bits(dev, cases, masked):
    c = cases["b"]
    B, A, H, W, _ = c["alpha_images"].shape
    im, al, mk, cams, depth = _on(c, dev, True)
    params = SimpleNamespace(use_depth_mask=masked, zfar=c["zfar"], ssim_factor=c["ssim_factor"])
    cameras = SimpleNamespace(R=c["R"].to(dev), T=c["T"].to(dev))
    alpha_cameras = SimpleNamespace(R=c["R_alpha"].reshape(-1, 3, 3).to(dev), T=c["T_alpha"].reshape(-1, 3).to(dev))
    fn = mu.get_reconstruction_loss_fn(params)
    want = ops.reconstruction_loss(im, al, mk if masked else None, cams, depth, c["zfar"], c["ssim_factor"], "zeros")
    want_grad = ops.reconstruction_loss_backward(im, al, mk if masked else None, cams, depth, torch.ones(1, device=dev), c["zfar"],
                                                 c["ssim_factor"], "zeros")
    ssim = type("SSIM", (torch.nn.Module,), {})()                      # upstream's layer, as far as the function looks at it
    ssim.C1, ssim.C2, ssim.mu_x_pool = 0.01 ** 2, 0.03 ** 2, torch.nn.AvgPool2d(3, 1)
    for last in (True, False):
        leaf = depth[0].reshape(B, H, W, 1).clone().requires_grad_(True)
        a, b = (im, al) if last else (im.permute(0, 3, 1, 2), al.permute(0, 1, 4, 2, 3))
        got = fn(params, a, b, mk[..., None], cameras, alpha_cameras, leaf, None, ssim, channel_is_at_the_end=last, padding_mode="zeros")
        assert got.dim() == 0 and torch.equal(got, want[0])
        got.backward()
        assert torch.equal(leaf.grad.reshape(1, B, H, W), want_grad)
    with torch.no_grad():                                               # all scales in one call
        many = mu.reconstruction_losses(params, im, al, mk, cameras, alpha_cameras, depth.expand(3, -1, -1, -1), padding_mode="zeros")
    assert tuple(many.shape) == (3,) and bool((many == want[0]).all())


def test_routes(dev, cases, modelled, monkeypatch):
    c, m = cases["a"], modelled["a", "border", True]
    im, al, mk, cams, depth = _on(c, dev, True)
    d_loss = torch.tensor([0.5, 1.5])
    calls = []
    real = ops.reconstruction_loss_backward
    monkeypatch.setattr(ops, "reconstruction_loss_backward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run():
        d = depth.clone().requires_grad_(True)
        loss = autograd.ReconstructionLossFunction.apply(d, im, al, mk, cams, c["zfar"], c["ssim_factor"], "border", ops.COST_VOLUME_FOV_SCALE)
        (loss * d_loss.to(dev)).sum().backward()
        return d.grad.cpu()

    monkeypatch.delenv("MCR_RECONSTRUCTION_LOSS_BWD", raising=False)
    hip = run()
    assert autograd.reconstruction_loss_backward_mode() == "hip" and len(calls) == 1
    monkeypatch.setenv("MCR_RECONSTRUCTION_LOSS_BWD", "composite")
    comp = run()
    assert autograd.reconstruction_loss_backward_mode() == "composite" and len(calls) == 1     # the entry was not called
    ref = model.gradient(*_margs(c, True), c["depth"], c["zfar"], c["ssim_factor"], "border", d_loss=d_loss)
    tie = F.max_pool2d((m["margin"] < 1e-3 * float(m["map"].max())).float(), 3, 1, 1) > 0
    e = float(((hip - comp).abs() * ~tie).max() / ref.abs().max())
    print(f"ERR routes: d_depth, HIP vs composite away from near-ties: {e:.2e}")
    assert e < 2 * TOL


def test_reflection_takes_the_composite(dev, cases, monkeypatch):
    c = cases["c"]
    B, A, H, W, _ = c["alpha_images"].shape
    im, al, mk, cams, depth = _on(c, dev, True)
    monkeypatch.setattr(ops, "reconstruction_loss", lambda *a, **k: pytest.fail("the entry does not take reflection padding"))
    params = SimpleNamespace(use_depth_mask=True, zfar=c["zfar"], ssim_factor=c["ssim_factor"])
    cameras = SimpleNamespace(R=c["R"].to(dev), T=c["T"].to(dev))
    alpha_cameras = SimpleNamespace(R=c["R_alpha"].reshape(-1, 3, 3).to(dev), T=c["T_alpha"].reshape(-1, 3).to(dev))
    leaf = depth[0].reshape(B, H, W, 1).clone().requires_grad_(True)
    got = mu.get_reconstruction_loss_fn(params)(params, im, al, mk[..., None], cameras, alpha_cameras, leaf, None, None,
                                                padding_mode="reflection")
    got.backward()
    with torch.no_grad():
        m = model.reconstruction(*_margs(c, True), c["depth"], c["zfar"], c["ssim_factor"], "reflection")
    ref = model.gradient(*_margs(c, True), c["depth"], c["zfar"], c["ssim_factor"], "reflection")
    tie = F.max_pool2d((m["margin"] < 1e-3 * float(m["map"].max())).float(), 3, 1, 1) > 0
    e_loss = rel(got, m["loss"][0])
    e_grad = float(((leaf.grad.cpu().reshape(1, B, H, W) - ref).abs() * ~tie).max() / ref.abs().max())
    print(f"ERR reflection padding (composite on the GPU) vs model: loss {e_loss:.2e} d_depth away from near-ties {e_grad:.2e}")
    assert e_loss < TOL and e_grad < TOL


# ---- 6. degenerate geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", ("zeros", "border"))
def test_zero_w_and_a_source_at_3e30_stay_finite(dev, cases, padding):
    """Target at the origin, source 0 two units ahead along the view axis with the depth exactly 2 on a block of pixels (v_z = 0 there,
    exactly: M = I), source 1 at T = 3e30."""
    c = cases["b"]
    B, A, H, W, _ = c["alpha_images"].shape
    eye = torch.eye(3)
    R, T = eye.expand(B, 3, 3).contiguous(), torch.zeros(B, 3)
    Ra, Ta = eye.expand(B, A, 3, 3).contiguous(), torch.tensor([[0.1, 0.0, -2.0], [3e30, 0.0, 0.0]]).expand(B, A, 3).contiguous()
    depth = c["depth"].clone()
    depth[:, :, 4:9, 5:17] = 2.0
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta).to(dev)
    im, al, mk = c["images"].to(dev), c["alpha_images"].to(dev), c["mask"].to(dev)
    loss, lmap, idx = ops.reconstruction_loss(im, al, mk, cams, depth.to(dev), c["zfar"], c["ssim_factor"], padding, return_map=True)
    grad = ops.reconstruction_loss_backward(im, al, mk, cams, depth.to(dev), torch.ones(1, device=dev), c["zfar"], c["ssim_factor"], padding)
    for t in (loss, lmap, grad):
        assert bool(torch.isfinite(t).all())
    assert float(loss) > 0 and int(idx.max()) <= 1


@pytest.mark.parametrize("padding", ("zeros", "border"))
def test_pixel_coordinate_that_overflows_samples_nothing(dev, cases, padding):
    """Case c's first source alone, 3e38 units off: the grid coordinate is finite (3e37 or more), 20 times it is not.  The entry and the
    composite both sample nothing: with no SSIM part and no mask the loss is the mean of |I|."""
    c = cases["c"]
    cams = ManyDepth.pack_cameras(c["R"], c["T"], c["R_alpha"][:, :1], torch.tensor([[[3e38, 0.0, 0.0]]])).to(dev)
    im, al, depth = c["images"].to(dev), c["alpha_images"][:, :1].contiguous().to(dev), c["depth"].to(dev)
    got = ops.reconstruction_loss(im, al, None, cams, depth, c["zfar"], 0.0, padding)
    comp = ManyDepth.reconstruction_loss_composite(im, al, None, cams, depth, c["zfar"], 0.0, padding)
    want = c["images"].abs().mean()
    assert torch.allclose(got.cpu()[0], want, rtol=1e-6, atol=0) and torch.allclose(comp.cpu()[0], want, rtol=1e-6, atol=0)
    grad = ops.reconstruction_loss_backward(im, al, None, cams, depth, torch.ones(1, device=dev), c["zfar"], 0.0, padding)
    assert bool((grad == 0).all())


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, cases):
    c = cases["c"]
    im, al, mk, cams, depth = _on(c, dev, True)
    S, B, H, W = depth.shape
    A = al.shape[1]
    args = (c["zfar"], c["ssim_factor"], "border")
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):      # a CPU tensor
        ops.reconstruction_loss(im, c["alpha_images"], mk, cams, depth, *args)
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):
        ops.reconstruction_loss_backward(im, al, mk, cams, c["depth"], torch.ones(1, device=dev), *args)
    al9, cams9 = al[:, :1].expand(B, 9, H, W, 3).contiguous(), cams[:, [0] + [1] * 9].contiguous()
    with pytest.raises(_lib.MacaronsHipError, match="sources"):         # A = 9
        ops.reconstruction_loss(im, al9, mk, cams9, depth, *args)
    with pytest.raises(_lib.MacaronsHipError, match="sources"):
        ops.reconstruction_loss_backward(im, al9, mk, cams9, depth, torch.ones(1, device=dev), *args)
    with pytest.raises(_lib.MacaronsHipError, match="at least 2"):      # H = 1
        ops.reconstruction_loss(im[:, :1].contiguous(), al[:, :, :1].contiguous(), mk[:, :1].contiguous(), cams, depth[:, :, :1].contiguous(), *args)
    with pytest.raises(ValueError, match="padding_mode"):
        ops.reconstruction_loss(im, al, mk, cams, depth, c["zfar"], c["ssim_factor"], "reflection")
    # at the C ABI: the outputs hold a fill value and keep it
    L = _lib.lib()
    i64, ci, cf = ctypes.c_int64, ctypes.c_int, ctypes.c_float
    need = int(L.mcr_reconstruction_loss_workspace_bytes(i64(S), i64(B), i64(A), i64(H), i64(W)))
    need_b = int(L.mcr_reconstruction_loss_backward_workspace_bytes(i64(S), i64(B), i64(A), i64(H), i64(W)))
    assert need > 0 and need_b > 0
    ws = torch.empty(max(need, need_b), dtype=torch.uint8, device=dev)
    loss, lmap = torch.full((S,), -7.25, device=dev), torch.full((S, B, H, W), -7.25, device=dev)
    amin, grad = torch.full((S, B, H, W), 77, dtype=torch.uint8, device=dev), torch.full((S, B, H, W), -7.25, device=dev)
    d_loss = torch.ones(S, device=dev)

    def fwd(mode, ws_bytes):
        return L.mcr_reconstruction_loss(ops._p(im), ops._p(al), ops._p(mk), ops._p(cams), ops._p(depth), ops._p(loss), ops._p(lmap),
                                         ops._p(amin), i64(S), i64(B), ci(A), ci(H), ci(W), cf(ops.COST_VOLUME_FOV_SCALE), cf(c["zfar"]),
                                         cf(c["ssim_factor"]), ci(mode), ops._p(ws), ctypes.c_size_t(ws_bytes), ops._stream())

    def bwd(mode, ws_bytes):
        return L.mcr_reconstruction_loss_backward(ops._p(im), ops._p(al), ops._p(mk), ops._p(cams), ops._p(depth), ops._p(d_loss),
                                                  ops._p(grad), i64(S), i64(B), ci(A), ci(H), ci(W), cf(ops.COST_VOLUME_FOV_SCALE),
                                                  cf(c["zfar"]), cf(c["ssim_factor"]), ci(mode), ops._p(ws), ctypes.c_size_t(ws_bytes),
                                                  ops._stream())

    assert fwd(2, need) != 0 and b"padding mode" in L.mcr_last_error()
    assert bwd(2, need_b) != 0 and b"padding mode" in L.mcr_last_error()
    assert fwd(1, need - 1) != 0 and b"workspace" in L.mcr_last_error()
    assert bwd(1, need_b - 1) != 0 and b"workspace" in L.mcr_last_error()
    torch.cuda.synchronize()
    assert bool((loss == -7.25).all()) and bool((lmap == -7.25).all()) and bool((amin == 77).all()) and bool((grad == -7.25).all())
    assert fwd(1, need) == 0 and bwd(1, need_b) == 0                    # and the same calls with their workspaces run
    torch.cuda.synchronize()
    want = _run(c, dev, "border", True)
    assert torch.equal(loss.cpu(), want[0]) and torch.equal(lmap.cpu(), want[1]) and torch.equal(amin.cpu(), want[2])
    assert torch.equal(grad.cpu(), want[3])
