"""The fused plane sweep on the GPU (cost_volume.hip: mcr_cost_volume behind ops.cost_volume, autograd.CostVolumeFunction and
networks.ManyDepth.CostVolumeBuilder / adopt_cost_volume_builder) against the reference's own forward (tests/golden/cost_volume.npz) and
the fp64 model (tests/_cost_volume_model.py).

Bound: the project's contract, 1e-4 of the largest magnitude of the output (or gradient), everywhere.  Every measured distance is printed
with an ERR prefix before it is asserted; NOTES.md ("Depth module: the plane sweep") records them.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cost_volume_model as model                                     # noqa: E402
from _cost_volume_model import load_case, rel                          # noqa: E402
from test_cost_volume_cpu import _StandIn                              # noqa: E402

from macarons_amd import _lib, ops                                     # noqa: E402
from macarons_amd.autograd import CostVolumeFunction                   # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = ("a", "b", "c")


@pytest.fixture(scope="module")
def cases():
    return {t: load_case(t) for t in CASES}


@pytest.fixture(scope="module")
def modelled(cases):
    out = {}
    for t, c in cases.items():
        with torch.no_grad():
            out[t] = model.forward(c["x"], c["R"], c["T"], c["x_alpha"], c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"],
                                   c["conv_reduce_weight"], c["conv_reduce_bias"])
    return out


def _on(c, dev):
    """(x, x_alpha, cams, bins) of a case on the device."""
    cams = ManyDepth.pack_cameras(c["R"], c["T"], c["R_alpha"], c["T_alpha"])
    return c["x"].to(dev), c["x_alpha"].to(dev), cams.to(dev), c["depth_bins"].to(dev)


def _mirror(c, dev):
    Hf, Wf = c["x"].shape[-2:]
    m = ManyDepth.CostVolumeBuilder(c["H"], c["W"], Hf, Wf, 64, c["x_alpha"].shape[1], float(c["d_range"][0]), float(c["d_range"][1]),
                                    c["D"], c["out_ch"])
    m.load_state_dict({"conv_reduce.weight": c["conv_reduce_weight"], "conv_reduce.bias": c["conv_reduce_bias"]})
    return m.to(dev)


def _call(m, c, dev, x=None, xa=None, **kw):
    B, A = c["x_alpha"].shape[:2]
    return m(c["x"].to(dev) if x is None else x, c["R"].to(dev), c["T"].to(dev), torch.full((B,), 750.0, device=dev),
             c["x_alpha"].to(dev) if xa is None else xa, c["R_alpha"].to(dev), c["T_alpha"].to(dev), torch.full((B, A), 750.0, device=dev),
             dev, **kw)


@pytest.mark.parametrize("tag", CASES)
def test_entry_against_golden_and_model(dev, cases, modelled, tag):
    c = cases[tag]
    x, xa, cams, bins = _on(c, dev)
    cv = ops.cost_volume(x, xa, cams, bins, c["H"], c["W"])
    assert cv.dtype == torch.float32 and tuple(cv.shape) == tuple(c["cost_volume"].shape)
    e_g, e_m, e_r = rel(cv, c["cost_volume"]), rel(cv, modelled[tag][1]), rel(c["cost_volume"], modelled[tag][1])
    print(f"ERR case {tag}: HIP vs golden {e_g:.2e}, HIP vs model {e_m:.2e} (reference vs model {e_r:.2e})")
    assert e_g < TOL and e_m < TOL


def test_two_runs_give_the_same_bits(dev, cases):
    x, xa, cams, bins = _on(cases["a"], dev)
    one = ops.cost_volume(x, xa, cams, bins, cases["a"]["H"], cases["a"]["W"]).clone()
    two = ops.cost_volume(x, xa, cams, bins, cases["a"]["H"], cases["a"]["W"])
    assert torch.equal(one, two)


@pytest.mark.parametrize("tag", ("a", "b"))
def test_out_as_channel_offset_view(dev, cases, tag):
    """out = channels C.. of a [B,C+D,Hf,Wf] buffer: the same bits as the plain call, channels 0..C-1 untouched."""
    c = cases[tag]
    x, xa, cams, bins = _on(c, dev)
    B, C, Hf, Wf = x.shape
    plain = ops.cost_volume(x, xa, cams, bins, c["H"], c["W"])
    buf = torch.full((B, C + c["D"], Hf, Wf), -7.25, device=dev)
    ret = ops.cost_volume(x, xa, cams, bins, c["H"], c["W"], out=buf[:, C:])
    assert ret.data_ptr() == buf[:, C:].data_ptr()
    assert torch.equal(buf[:, C:], plain)
    assert bool((buf[:, :C] == -7.25).all())


@pytest.mark.parametrize("tag", CASES)
def test_mirror_class_forward(dev, cases, modelled, tag):
    c = cases[tag]
    m = _mirror(c, dev)
    with torch.no_grad():
        res = _call(m, c, dev)
        both = _call(m, c, dev, return_cost_volume=True)
    assert torch.is_tensor(res) and isinstance(both, tuple) and len(both) == 2
    assert torch.equal(both[0], res) and tuple(both[1].shape) == tuple(c["cost_volume"].shape)
    e_g, e_m = rel(res, c["res"]), rel(res, modelled[tag][0])
    print(f"ERR case {tag}: mirror-class res vs golden {e_g:.2e}, vs model {e_m:.2e}; cost volume vs golden {rel(both[1], c['cost_volume']):.2e}")
    assert e_g < TOL and e_m < TOL and rel(both[1], c["cost_volume"]) < TOL


def test_adopted_instance_matches_mirror_class(dev, cases):
    c = cases["a"]
    s = _StandIn()
    s.conv_reduce.load_state_dict({"weight": c["conv_reduce_weight"], "bias": c["conv_reduce_bias"]})
    s.conv_reduce.to(dev)
    ManyDepth.adopt_cost_volume_builder(s)
    with torch.no_grad():
        res_s, cv_s = _call(s.forward, c, dev, return_cost_volume=True)
        res_m, cv_m = _call(_mirror(c, dev), c, dev, return_cost_volume=True)
    assert torch.equal(res_s, res_m) and torch.equal(cv_s, cv_m)
    assert s.warp() == "upstream warp"


def test_adopted_forward_moves_the_pixel_tables(dev, cases):
    """Upstream's forward is where x_tab / y_tab / depth_bins reach the device (they are no buffers); upstream's reconstruction loss
    then calls reproject_depth_map with a device depth.  Adopted right after construction, the HIP forward has to do the same."""
    c = cases["a"]
    s = _StandIn()
    s.conv_reduce.to(dev)
    ManyDepth.adopt_cost_volume_builder(s)
    assert s.x_tab.device.type == "cpu" and s.y_tab.device.type == "cpu" and s.depth_bins.device.type == "cpu"
    with torch.no_grad():
        _call(s.forward, c, dev)
    assert s.x_tab.device == dev and s.y_tab.device == dev and s.depth_bins.device == dev
    pts = s.reproject_depth_map(torch.full((2, 26, 42, 1), 3.0, device=dev))                 # reads self.x_tab / self.y_tab
    assert pts.device == dev and tuple(pts.shape) == (2, 26 * 42, 3)
    assert torch.equal(pts[0, :, 0].cpu(), _StandIn().x_tab.reshape(-1)) and torch.equal(pts[1, :, 1].cpu(), _StandIn().y_tab.reshape(-1))


@pytest.mark.parametrize("tag", ("a", "c"))
def test_gradients_through_the_function(dev, cases, tag):
    """loss = a fixed random weighting of res; gradients of x, x_alpha, conv_reduce.weight and conv_reduce.bias against fp64 autograd
    through the model."""
    c = cases[tag]
    m = _mirror(c, dev)
    x, xa = c["x"].to(dev).requires_grad_(True), c["x_alpha"].to(dev).requires_grad_(True)
    lw = torch.randn(c["res"].shape, generator=torch.Generator().manual_seed(5))
    res = _call(m, c, dev, x=x, xa=xa)
    got = torch.autograd.grad((res * lw.to(dev)).sum(), (x, xa, m.conv_reduce.weight, m.conv_reduce.bias))
    x6, xa6, w6, b6 = (t.detach().double().requires_grad_(True) for t in (c["x"], c["x_alpha"], c["conv_reduce_weight"], c["conv_reduce_bias"]))
    res6, _ = model.forward(x6, c["R"], c["T"], xa6, c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"], w6, b6)
    want = torch.autograd.grad((res6 * lw.double()).sum(), (x6, xa6, w6, b6))
    assert rel(res, res6) < TOL
    for name, g, r in zip(("x", "x_alpha", "conv_reduce.weight", "conv_reduce.bias"), got, want):
        e = rel(g, r)
        print(f"ERR case {tag}: gradient of {name}: {e:.2e}")
        assert e < TOL, name


def test_function_without_concat_and_once_only(dev, cases):
    c = cases["c"]
    x, xa, cams, bins = _on(c, dev)
    x.requires_grad_(True)
    cv = CostVolumeFunction.apply(x, xa, cams, bins, c["H"], c["W"], ops.COST_VOLUME_FOV_SCALE, False)
    assert torch.equal(cv.detach(), ops.cost_volume(x.detach(), xa, cams, bins, c["H"], c["W"]))
    (g,) = torch.autograd.grad(cv.sum(), x, retain_graph=True)
    assert g.shape == x.shape and bool(torch.isfinite(g).all()) and xa.grad is None
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(cv.sum(), x, create_graph=True)


def test_refusals(dev, cases):
    c = cases["c"]
    x, xa, cams, bins = _on(c, dev)
    with pytest.raises(_lib.MacaronsHipError, match="64"):                      # C != 64
        ops.cost_volume(x[:, :32].contiguous(), xa[:, :, :32].contiguous(), cams, bins, c["H"], c["W"])
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):              # a CPU tensor
        ops.cost_volume(x, c["x_alpha"], cams, bins, c["H"], c["W"])
    # a short workspace, at the C ABI
    L = _lib.lib()
    B, C, Hf, Wf = x.shape
    A = xa.shape[1]
    need = int(L.mcr_cost_volume_workspace_bytes(ctypes.c_int64(B), ctypes.c_int64(A), ctypes.c_int64(C), ctypes.c_int64(Hf), ctypes.c_int64(Wf)))
    assert need >= B * A * C * Hf * Wf * 4
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.zeros((B, c["D"], Hf, Wf), device=dev)
    rc = L.mcr_cost_volume(ops._p(x), ops._p(xa), ops._p(cams), ops._p(bins), ops._p(out), ctypes.c_int64(c["D"] * Hf * Wf), ctypes.c_int64(B),
                           ctypes.c_int(A), ctypes.c_int(C), ctypes.c_int(c["H"]), ctypes.c_int(c["W"]), ctypes.c_int(Hf), ctypes.c_int(Wf),
                           ctypes.c_int(c["D"]), ctypes.c_float(ops.COST_VOLUME_FOV_SCALE), ops._p(ws), ctypes.c_size_t(need - 1), ops._stream())
    assert rc != 0 and b"workspace" in L.mcr_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                               # refused before any launch


def near_zero_w_case():
    """One target at the origin, three sources over 18x30 -> 5x7, 5 planes (0.5, 2.33, 4.17, 6 and 2e-5).  Sources 0 and 2 are yawed by
    0.3 and placed so that their view depth w = d u_z + t_z changes sign at image column 12, a bicubic tap, on plane 1 (source 0) and
    on the plane at 2e-5 (source 2): what is left at that column is the rounding of t_z to fp32 -- about 1e-7 for source 0 (above the
    1e-8 clamp: coordinates of 1e6 and more next to ordinary taps) and about 1e-12 for source 2 (below the clamp, sign kept).  Source 1
    sits exactly on plane 2 (w = 0 at every pixel, clamped to +1e-8) and 3e30 to the side: its coordinates are +-infinity on that plane
    (the cubic sum turns them into NaN) and ~1e30 on the others -- far outside what an int holds."""
    H, W, Hf, Wf = 18, 30, 5, 7
    g = torch.Generator().manual_seed(11)
    x, xa = torch.randn(1, 64, Hf, Wf, generator=g), torch.randn(1, 3, 64, Hf, Wf, generator=g)
    bins = torch.cat((torch.linspace(0.5, 6.0, 4), torch.tensor([2e-5])))
    th = 0.3
    yaw = torch.tensor([[np.cos(th), 0.0, np.sin(th)], [0.0, 1.0, 0.0], [-np.sin(th), 0.0, np.cos(th)]], dtype=torch.float32)
    # u_z = n_x sin(th) + cos(th) at image column 12
    n_x = (W / min(H, W) - 2.0 * 12 / (min(H, W) - 1)) / model.FOV_SCALE
    u_z = n_x * np.sin(th) + np.cos(th)
    Ra = torch.stack((yaw, torch.eye(3), yaw))[None]
    Ta = torch.tensor([[[0.3, 0.0, -float(bins[1]) * u_z], [3e30, 0.0, -float(bins[2])], [0.3, 0.0, -float(bins[4]) * u_z]]], dtype=torch.float32)
    return dict(x=x, x_alpha=xa, R=torch.eye(3)[None], T=torch.zeros(1, 3), R_alpha=Ra, T_alpha=Ta, depth_bins=bins, H=H, W=W, D=5)


def test_near_zero_w_is_finite_and_indexes_nothing(dev):
    c = near_zero_w_case()
    Hf, Wf = c["x"].shape[-2:]
    with torch.no_grad():
        ref = model.cost_volume(c["x"], c["R"], c["T"], c["x_alpha"], c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"])
        taps = model.tap_abs_w(c["R"], c["T"], c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"], Hf, Wf)
    wmin = taps.amin(dim=(4, 6)).amin(1)
    good = wmin > 1e-3
    # the case reaches the clamp from both sides: taps at exactly 0, taps that are non-zero and below 1e-8, taps just above it
    below = taps[(taps > 0) & (taps < 1e-8)]
    print(f"near-zero w: {int((taps == 0).sum())} taps at w = 0, {below.numel()} non-zero below the 1e-8 clamp (smallest {float(below.min()):.1e}), "
          f"{int(((taps >= 1e-8) & (taps < 1e-6)).sum())} in [1e-8, 1e-6)")
    assert bool((taps == 0).any()) and below.numel() > 0 and float(below.min()) < 1e-11 and bool(((taps >= 1e-8) & (taps < 1e-6)).any())
    assert 0.3 < float(good.float().mean()) < 0.95                                   # and both kinds of position
    x, xa, cams, bins = _on(c, dev)
    cv = ops.cost_volume(x, xa, cams, bins, c["H"], c["W"]).cpu()
    assert bool(torch.isfinite(cv).all())
    upper = (c["x"].abs().sum(1) + c["x_alpha"].abs().amax(dim=(3, 4)).mean(1).sum(1)[:, None, None]) / 64   # |mean - x| <= |x| + max |x_alpha|
    assert bool((cv >= 0).all()) and bool((cv <= upper[:, None] * (1 + 1e-5)).all())
    e = float((cv.double() - ref)[good].abs().max() / ref.abs().max())
    print(f"ERR near-zero w: HIP vs model at the {int(good.sum())} of {good.numel()} positions whose taps all have |w| > 1e-3: {e:.2e}")
    assert e < TOL
