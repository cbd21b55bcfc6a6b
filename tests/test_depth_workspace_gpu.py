"""The workspaces of the six depth-module entries (cost volume, reconstruction loss, disparity scales; forward and backward), at the C ABI:
each entry gets EXACTLY the bytes its *_workspace_bytes states, carved 256-byte aligned out of the NaN-filled, guard-banded arena of
tests/_strided.py.  It must leave the guard intact, give the bits of the same call through ops.* (whose cached workspace is roomy and
holds whatever the last call left: the entries are documented to give the same bits on every run, so an entry that read scratch it
never wrote, or wrote past its size, shows here), and refuse a workspace one byte short with "workspace" in the message.

Shapes: the smallest that still take every path.  Cost volume: P = 15 positions is under one 16-position workgroup and D = 5 is no
multiple of the 4 planes of a workgroup; the backward runs with both gradients and with d_x alone (no sample list).  Reconstruction loss:
17 x 18 pixels are 2 x 2 partial 16 x 16 tiles.  Disparity scales: ratios 1 and 2 on 18 x 20 pixels, again 2 x 2 partial tiles.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _strided import Workspace                                         # noqa: E402

from macarons_amd import _lib, ops                                     # noqa: E402

pytestmark = pytest.mark.gpu

i64, ci, cf = ctypes.c_int64, ctypes.c_int, ctypes.c_float
_p = ops._p


def _opt(t):
    return _p(t) if t is not None else None


def _cams(B, A, gen):
    """[B,1+A,12]: rotations a few degrees from the identity (the matrix exponential of a small skew matrix), small translations."""
    w = 0.05 * torch.randn((B, 1 + A, 3), generator=gen, dtype=torch.float64)
    K = torch.zeros((B, 1 + A, 3, 3), dtype=torch.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    R = torch.matrix_exp(K - K.transpose(-1, -2))
    T = 0.05 * torch.randn((B, 1 + A, 3), generator=gen, dtype=torch.float64)
    return torch.cat((R.reshape(B, 1 + A, 9), T), -1).float().contiguous()


def _guarded(dev, size_fn, sizes, entry):
    """entry(workspace pointer, bytes) -> rc on exactly the stated bytes inside a guarded arena; then one byte short."""
    L = _lib.lib()
    need = int(size_fn(*sizes))
    assert need > 0 and need % 256 == 0
    ws = Workspace(need, device=dev)
    assert ws.ptr % 256 == 0
    assert entry(ctypes.c_void_p(ws.ptr), need) == 0, L.mcr_last_error()
    torch.cuda.synchronize()
    ws.check_guard("workspace")
    return need


def _refused_one_short(dev, need, entry, outputs):
    """The same call with need - 1 bytes: refused before any launch, the outputs keep their bits."""
    L = _lib.lib()
    ws = Workspace(need, device=dev)
    before = [o.clone() for o in outputs]
    assert entry(ctypes.c_void_p(ws.ptr), need - 1) != 0 and b"workspace" in L.mcr_last_error()
    torch.cuda.synchronize()
    ws.check_unchanged("refused workspace")
    assert all(torch.equal(o.view(torch.uint8), b.view(torch.uint8)) for o, b in zip(outputs, before))


# ---- the plane sweep -----------------------------------------------------------------------------------------------------------------
CV = dict(B=2, A=2, C=64, H=12, W=12, Hf=3, Wf=5, D=5)


@pytest.fixture(scope="module")
def cv(dev):
    g = torch.Generator().manual_seed(71)
    s = CV
    x = torch.randn((s["B"], s["C"], s["Hf"], s["Wf"]), generator=g)
    xa = torch.randn((s["B"], s["A"], s["C"], s["Hf"], s["Wf"]), generator=g)
    bins = torch.linspace(0.8, 3.0, s["D"])
    d_out = torch.randn((s["B"], s["D"], s["Hf"], s["Wf"]), generator=g)
    return tuple(t.to(dev) for t in (x, xa, _cams(s["B"], s["A"], g), bins, d_out))


def test_cost_volume(dev, cv):
    x, xa, cams, bins, _ = cv
    s, L = CV, _lib.lib()
    out = torch.full((s["B"], s["D"], s["Hf"], s["Wf"]), -7.25, device=dev)

    def entry(ws, n):
        return L.mcr_cost_volume(_p(x), _p(xa), _p(cams), _p(bins), _p(out), i64(s["D"] * s["Hf"] * s["Wf"]), i64(s["B"]), ci(s["A"]), ci(s["C"]),
                                 ci(s["H"]), ci(s["W"]), ci(s["Hf"]), ci(s["Wf"]), ci(s["D"]), cf(ops.COST_VOLUME_FOV_SCALE), ws,
                                 ctypes.c_size_t(n), ops._stream())

    sizes = (i64(s["B"]), i64(s["A"]), i64(s["C"]), i64(s["Hf"]), i64(s["Wf"]))
    _refused_one_short(dev, int(L.mcr_cost_volume_workspace_bytes(*sizes)), entry, [out])
    _guarded(dev, L.mcr_cost_volume_workspace_bytes, sizes, entry)
    want = ops.cost_volume(x, xa, cams, bins, s["H"], s["W"])
    assert bool(torch.isfinite(want).all()) and bool((want > 0).any())
    assert torch.equal(out, want)


@pytest.mark.parametrize("both", [True, False], ids=["both", "d_x_only"])
def test_cost_volume_backward(dev, cv, both):
    x, xa, cams, bins, d_out = cv
    s, L = CV, _lib.lib()
    d_x, d_xa = torch.full_like(x, -7.25), torch.full_like(xa, -7.25)

    def entry(ws, n):
        return L.mcr_cost_volume_backward(_p(x), _p(xa), _p(cams), _p(bins), _p(d_out), i64(s["D"] * s["Hf"] * s["Wf"]), _p(d_x),
                                          _p(d_xa) if both else None, i64(s["B"]), ci(s["A"]), ci(s["C"]), ci(s["H"]), ci(s["W"]), ci(s["Hf"]),
                                          ci(s["Wf"]), ci(s["D"]), cf(ops.COST_VOLUME_FOV_SCALE), ws, ctypes.c_size_t(n), ops._stream())

    sizes = (i64(s["B"]), i64(s["A"]), i64(s["C"]), i64(s["Hf"]), i64(s["Wf"]), i64(s["D"]))
    _refused_one_short(dev, int(L.mcr_cost_volume_backward_workspace_bytes(*sizes)), entry, [d_x, d_xa])
    _guarded(dev, L.mcr_cost_volume_backward_workspace_bytes, sizes, entry)
    want_x, want_xa = ops.cost_volume_backward(x, xa, cams, bins, d_out, s["H"], s["W"], need_x_alpha=both)
    assert bool(torch.isfinite(want_x).all()) and bool((want_x != 0).any())
    assert torch.equal(d_x, want_x)
    if both:
        assert bool((want_xa != 0).any()) and torch.equal(d_xa, want_xa)
    else:
        assert bool((d_xa == -7.25).all())                               # not asked for: not touched


# ---- the reconstruction loss ---------------------------------------------------------------------------------------------------------
RL = dict(S=2, B=2, A=2, H=17, W=18, zfar=10.0, f=0.85, mode="border")


@pytest.fixture(scope="module")
def rl(dev):
    g = torch.Generator().manual_seed(72)
    s = RL
    images = torch.rand((s["B"], s["H"], s["W"], 3), generator=g)
    alpha = torch.rand((s["B"], s["A"], s["H"], s["W"], 3), generator=g)
    depth = 1.0 + 2.0 * torch.rand((s["S"], s["B"], s["H"], s["W"]), generator=g)
    mask = torch.rand((s["B"], s["H"], s["W"]), generator=g) < 0.7
    d_loss = torch.randn((s["S"],), generator=g)
    return tuple(t.to(dev) for t in (images, alpha, _cams(s["B"], s["A"], g), depth, mask, d_loss))


def _rl_common(s):
    return (i64(s["S"]), i64(s["B"]), ci(s["A"]), ci(s["H"]), ci(s["W"]), cf(ops.COST_VOLUME_FOV_SCALE), cf(s["zfar"]), cf(s["f"]),
            ci(ops.RECONSTRUCTION_PADDING_MODES[s["mode"]]))


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no_mask"])
def test_reconstruction_loss(dev, rl, masked):
    images, alpha, cams, depth, mask, _ = rl
    mask = mask if masked else None
    s, L = RL, _lib.lib()
    loss = torch.full((s["S"],), -7.25, device=dev)
    lmap = torch.full((s["S"], s["B"], s["H"], s["W"]), -7.25, device=dev)
    amin = torch.full((s["S"], s["B"], s["H"], s["W"]), 77, dtype=torch.uint8, device=dev)

    def entry(ws, n):
        return L.mcr_reconstruction_loss(_p(images), _p(alpha), _opt(mask), _p(cams), _p(depth), _p(loss), _p(lmap), _p(amin), *_rl_common(s), ws,
                                         ctypes.c_size_t(n), ops._stream())

    sizes = tuple(i64(s[k]) for k in ("S", "B", "A", "H", "W"))
    _refused_one_short(dev, int(L.mcr_reconstruction_loss_workspace_bytes(*sizes)), entry, [loss, lmap, amin])
    _guarded(dev, L.mcr_reconstruction_loss_workspace_bytes, sizes, entry)
    want = ops.reconstruction_loss(images, alpha, mask, cams, depth, s["zfar"], s["f"], s["mode"], return_map=True)
    assert bool(torch.isfinite(want[0]).all()) and bool((want[0] > 0).all())
    for got, w in zip((loss, lmap, amin), want):
        assert torch.equal(got, w)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no_mask"])
def test_reconstruction_loss_backward(dev, rl, masked):
    images, alpha, cams, depth, mask, d_loss = rl
    mask = mask if masked else None
    s, L = RL, _lib.lib()
    d_depth = torch.full_like(depth, -7.25)

    def entry(ws, n):
        return L.mcr_reconstruction_loss_backward(_p(images), _p(alpha), _opt(mask), _p(cams), _p(depth), _p(d_loss), _p(d_depth), *_rl_common(s), ws,
                                                  ctypes.c_size_t(n), ops._stream())

    sizes = tuple(i64(s[k]) for k in ("S", "B", "A", "H", "W"))
    _refused_one_short(dev, int(L.mcr_reconstruction_loss_backward_workspace_bytes(*sizes)), entry, [d_depth])
    _guarded(dev, L.mcr_reconstruction_loss_backward_workspace_bytes, sizes, entry)
    want = ops.reconstruction_loss_backward(images, alpha, mask, cams, depth, d_loss, s["zfar"], s["f"], s["mode"])
    assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
    assert torch.equal(d_depth, want)


# ---- the disparity scales ------------------------------------------------------------------------------------------------------------
DS = dict(B=2, H=18, W=20, ratios=(1, 2), znear=0.5, zfar=10.0)


@pytest.fixture(scope="module")
def ds(dev):
    g = torch.Generator().manual_seed(73)
    s = DS
    disps = [0.05 + torch.rand((s["B"], s["H"] // r, s["W"] // r), generator=g) for r in s["ratios"]]
    images = torch.rand((s["B"], s["H"], s["W"], 3), generator=g)
    mask = torch.rand((s["B"], s["H"], s["W"]), generator=g) < 0.7
    d_depth = torch.randn((len(disps), s["B"], s["H"], s["W"]), generator=g)
    d_reg = torch.randn((len(disps),), generator=g)
    return [d.to(dev) for d in disps], images.to(dev), mask.to(dev), d_depth.to(dev), d_reg.to(dev)


def _ds_common(disps, s):
    S = len(disps)
    ptrs = (ctypes.c_void_p * S)(*[d.data_ptr() for d in disps])
    hs, wss = (ctypes.c_int * S)(*[d.shape[1] for d in disps]), (ctypes.c_int * S)(*[d.shape[2] for d in disps])
    return (ptrs, hs, wss), (ci(S), i64(s["B"]), ci(s["H"]), ci(s["W"]), cf(s["znear"]), cf(s["zfar"])), (i64(S), i64(s["B"]), i64(s["H"]), i64(s["W"]))


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no_mask"])
def test_disparity_scales(dev, ds, masked):
    disps, images, mask, _, _ = ds
    mask = mask if masked else None
    s, L = DS, _lib.lib()
    S = len(disps)
    maps, tail, sizes = _ds_common(disps, s)
    depth = torch.full((S, s["B"], s["H"], s["W"]), -7.25, device=dev)
    reg, thr = torch.full((S,), -7.25, device=dev), torch.full((s["B"],), -7.25, device=dev)
    em = torch.full((s["B"], s["H"], s["W"]), 77, dtype=torch.uint8, device=dev)
    tab = torch.full((s["B"], s["H"], s["W"]), -7.25, device=dev)

    def entry(tab_, thr_):
        return lambda ws, n: L.mcr_disparity_scales(*maps, _p(images), _opt(mask), _p(depth), _p(reg), _p(em), _opt(tab_), _opt(thr_), *tail, ws,
                                                    ctypes.c_size_t(n), ops._stream())

    _refused_one_short(dev, int(L.mcr_disparity_scales_workspace_bytes(*sizes)), entry(tab, thr), [depth, reg, em, tab, thr])
    _guarded(dev, L.mcr_disparity_scales_workspace_bytes, sizes, entry(tab, thr))
    want = ops.disparity_scales(disps, images, mask, s["znear"], s["zfar"], return_tab=True)
    assert bool(torch.isfinite(want[1]).all()) and bool((want[1] > 0).all()) and 0 < int(want[2].sum()) < want[2].numel()
    for got, w in zip((depth, reg, em.bool(), tab, thr), want):
        assert torch.equal(got, w)
    # without the caller's tab and thr the entry keeps them in its workspace: the same outputs, the guard still intact
    depth.fill_(-7.25), reg.fill_(-7.25), em.fill_(77)
    _guarded(dev, L.mcr_disparity_scales_workspace_bytes, sizes, entry(None, None))
    for got, w in zip((depth, reg, em.bool()), want):
        assert torch.equal(got, w)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "no_mask"])
@pytest.mark.parametrize("with_reg", [True, False], ids=["both", "d_depth_only"])
def test_disparity_scales_backward(dev, ds, masked, with_reg):
    disps, images, mask, d_depth, d_reg = ds
    mask, d_reg = (mask if masked else None), (d_reg if with_reg else None)
    s, L = DS, _lib.lib()
    maps, tail, sizes = _ds_common(disps, s)
    grads = [torch.full_like(d, -7.25) for d in disps]
    gptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])

    def entry(ws, n):
        return L.mcr_disparity_scales_backward(*maps, _p(images), _opt(mask), _p(d_depth), _opt(d_reg), gptrs, *tail, ws, ctypes.c_size_t(n),
                                               ops._stream())

    _refused_one_short(dev, int(L.mcr_disparity_scales_backward_workspace_bytes(*sizes)), entry, grads)
    _guarded(dev, L.mcr_disparity_scales_backward_workspace_bytes, sizes, entry)
    want = ops.disparity_scales_backward(disps, images, mask, s["znear"], s["zfar"], d_depth, d_reg)
    for got, w in zip(grads, want):
        assert bool(torch.isfinite(w).all()) and bool((w != 0).any())
        assert torch.equal(got, w)
