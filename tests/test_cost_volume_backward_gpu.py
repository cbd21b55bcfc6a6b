"""The HIP backward of the plane sweep (cost_volume_bwd.hip: mcr_cost_volume_backward behind ops.cost_volume_backward and
autograd.CostVolumeFunction) against fp64 autograd through the model (tests/_cost_volume_model.py).

Bound: the project's contract, TOL = 1e-4 of the largest magnitude of the reference gradient (tests/test_cost_volume_gpu.py).  The loss
is a fixed seeded random weighting of the output.  Every measured distance is printed with an ERR prefix before it is asserted; NOTES.md
("Depth module: the plane sweep", Backward) records them.

The sign margin.  A gradient is a sum of +-g over the channels' signs of m_c - x_c, so an fp32 and an fp64 evaluation agree only where
they agree on every sign.  The cases whose numbers this file chooses (the pile-up's poses, the near-zero-w inputs under their mask) assert
that the model's smallest non-zero |m_c - x_c| exceeds 1e-5.  The goldens a, b and c are fixed data and the ReLU case is case a's own
features under a ReLU: their margins are 5.4e-06, 5.9e-06, 4.2e-06 and 5.0e-07, below 1e-5, and there is no seed to change (400 seeds of
ReLU'd normal features on case a's geometry gave no margin above 1e-5 either: a zero target channel next to a source sample of small
bilinear weight is what such features are made of).  Their margins are printed, not asserted; their gradients carry the same TOL.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cost_volume_model as model                                     # noqa: E402
from _cost_volume_model import load_case, rel                          # noqa: E402
from test_cost_volume_gpu import TOL, near_zero_w_case                 # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.autograd import CostVolumeFunction                   # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1e-5


def _diff(c):
    """m_c - x_c of the model, [B,C,D,Hf,Wf] float64."""
    Hf, Wf = c["x"].shape[-2:]
    with torch.no_grad():
        g, _ = model.grid_coordinates(c["R"], c["T"], c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"], Hf, Wf)
        return model.sample(c["x_alpha"], g).mean(1) - c["x"].double()[:, :, None]


def _reference(c, lw):
    """fp64 autograd through the model: the gradients of sum(cost volume * lw) for x and x_alpha."""
    x6, xa6 = c["x"].double().requires_grad_(True), c["x_alpha"].double().requires_grad_(True)
    cv = model.cost_volume(x6, c["R"], c["T"], xa6, c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"])
    return torch.autograd.grad((cv * lw.double()).sum(), (x6, xa6))


@pytest.fixture(scope="module")
def world():
    """Per case: the inputs, a seeded weighting lw of a [B,C+D,Hf,Wf] buffer (channels C.. weight the cost volume), the reference
    gradients under lw[:, C:], the sign margin and the share of exact zeros among m_c - x_c.  Computed once, never changed."""
    cs = {t: load_case(t) for t in "abc"}
    cs["relu"] = dict(cs["a"], x=cs["a"]["x"].relu(), x_alpha=cs["a"]["x_alpha"].relu())
    b = cs["b"]
    cs["pile"] = dict(b, R_alpha=b["R"][:, None].expand_as(b["R_alpha"]).clone(), T_alpha=b["T"][:, None].expand_as(b["T_alpha"]).clone())
    out = {}
    for seed, (t, c) in enumerate(cs.items()):
        B, C, Hf, Wf = c["x"].shape
        lw = torch.randn((B, C + c["D"], Hf, Wf), generator=torch.Generator().manual_seed(40 + seed))
        d = _diff(c).abs()
        out[t] = dict(c=c, lw=lw, ref=_reference(c, lw[:, C:]), margin=float(d[d > 0].min()), zeros=float((d == 0).double().mean()))
        print(f"case {t}: sign margin {out[t]['margin']:.2e}, exact zeros {out[t]['zeros']:.4f}")
    return out


def _on(c, dev):
    cams = ManyDepth.pack_cameras(c["R"], c["T"], c["R_alpha"], c["T_alpha"])
    return c["x"].to(dev), c["x_alpha"].to(dev), cams.to(dev), c["depth_bins"].to(dev)


def _check(what, got, want):
    for name, g, r in zip(("x", "x_alpha"), got, want):
        e = rel(g, r)
        print(f"ERR {what}: gradient of {name}: {e:.2e}")
        assert bool(torch.isfinite(g).all()) and e < TOL, (what, name, e)


def _direct(w, dev, **kw):
    c = w["c"]
    x, xa, cams, bins = _on(c, dev)
    C = x.shape[1]
    return ops.cost_volume_backward(x, xa, cams, bins, w["lw"][:, C:].contiguous().to(dev), c["H"], c["W"], **kw)


# ---- 1. the goldens ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("a", "b", "c"))
def test_goldens_through_the_entry(dev, world, tag):
    w = world[tag]
    d_x, d_xa = _direct(w, dev)
    assert d_x.shape == w["c"]["x"].shape and d_xa.shape == w["c"]["x_alpha"].shape and d_x.dtype == d_xa.dtype == torch.float32
    _check(f"case {tag}, entry", (d_x, d_xa), w["ref"])
    if "away" in w["c"]:                                                 # a source that looks away receives nothing, exactly
        b, a = w["c"]["away"]
        assert bool((d_xa[b, a] == 0).all()) and bool((w["ref"][1][b, a] == 0).all())


@pytest.mark.parametrize("concat", (False, True))
@pytest.mark.parametrize("tag", ("a", "b", "c"))
def test_goldens_through_the_function(dev, world, tag, concat):
    w = world[tag]
    c = w["c"]
    x, xa, cams, bins = _on(c, dev)
    C = x.shape[1]
    x.requires_grad_(True), xa.requires_grad_(True)
    out = CostVolumeFunction.apply(x, xa, cams, bins, c["H"], c["W"], ops.COST_VOLUME_FOV_SCALE, concat)
    lw = w["lw"] if concat else w["lw"][:, C:]
    assert out.shape == lw.shape
    got = torch.autograd.grad((out * lw.to(dev)).sum(), (x, xa))
    want = w["ref"]
    if concat:                                                           # the buffer's first C channels are x itself
        assert float(lw[:, :C].abs().min()) > 0
        want = (want[0] + lw[:, :C].double(), want[1])
    _check(f"case {tag}, function, concat={concat}", got, want)


# ---- 2. ReLU'd features: differences that are exactly zero -------------------------------------------------------------------------------
def test_relu_features_have_three_sign_states(dev, world):
    w = world["relu"]
    assert w["zeros"] >= 0.01, w["zeros"]                                # a condition on the inputs
    got = _direct(w, dev)
    _check("ReLU'd case a", got, w["ref"])
    # what a two-state sign would give is out of bound: the test would not notice it otherwise
    d = _diff(w["c"])
    C, lw = d.shape[1], w["lw"]
    two = -(lw[:, C:].double()[:, None] * torch.where(d < 0, -1.0, 1.0)).sum(2) / C
    assert rel(two, w["ref"][0]) > 10 * TOL


# ---- 3. pile-up: every plane of a position lands on the same source pixels ----------------------------------------------------------------
def test_pile_up_lists_and_bit_reproducibility(dev, world):
    w = world["pile"]
    assert w["margin"] > MARGIN and w["c"]["D"] == 96
    one = _direct(w, dev)
    _check("pile-up", one, w["ref"])
    two = _direct(w, dev)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


# ---- 4. near-zero w -------------------------------------------------------------------------------------------------------------------------
def test_near_zero_w(dev):
    c = near_zero_w_case()
    B, C, Hf, Wf = c["x"].shape
    with torch.no_grad():
        good = model.tap_min_abs_w(c["R"], c["T"], c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"], Hf, Wf) > 1e-3
    d = _diff(c).abs()
    d = d[good[:, None].expand_as(d)]
    assert float(d[d > 0].min()) > MARGIN
    lw = torch.randn((B, c["D"], Hf, Wf), generator=torch.Generator().manual_seed(46))
    x, xa, cams, bins = _on(c, dev)
    masked = lw * good
    got = ops.cost_volume_backward(x, xa, cams, bins, masked.to(dev), c["H"], c["W"])
    _check("near-zero w, masked", got, _reference(c, masked))
    for g in ops.cost_volume_backward(x, xa, cams, bins, lw.to(dev), c["H"], c["W"]):
        assert bool(torch.isfinite(g).all())


# ---- 5. halves ------------------------------------------------------------------------------------------------------------------------------
def test_halves(dev, world):
    w = world["a"]
    c = w["c"]
    d_x, d_xa = _direct(w, dev)
    only_x = _direct(w, dev, need_x_alpha=False)
    only_xa = _direct(w, dev, need_x=False)
    assert only_x[1] is None and torch.equal(only_x[0], d_x)
    assert only_xa[0] is None and torch.equal(only_xa[1], d_xa)
    C = c["x"].shape[1]
    for i in (0, 1):
        x, xa, cams, bins = _on(c, dev)
        (x, xa)[i].requires_grad_(True)
        cv = CostVolumeFunction.apply(x, xa, cams, bins, c["H"], c["W"], ops.COST_VOLUME_FOV_SCALE, False)
        (cv * w["lw"][:, C:].to(dev)).sum().backward()
        assert (x, xa)[1 - i].grad is None and torch.equal((x, xa)[i].grad, (d_x, d_xa)[i])


# ---- 6. strided d_out -----------------------------------------------------------------------------------------------------------------------
def test_strided_d_out(dev, world):
    w = world["a"]
    c = w["c"]
    x, xa, cams, bins = _on(c, dev)
    C = x.shape[1]
    buf_grad = w["lw"].to(dev)
    view = buf_grad[:, C:]
    assert not view.is_contiguous()
    got = ops.cost_volume_backward(x, xa, cams, bins, view, c["H"], c["W"])
    want = ops.cost_volume_backward(x, xa, cams, bins, view.contiguous(), c["H"], c["W"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 7. routes ------------------------------------------------------------------------------------------------------------------------------
def test_routes(dev, world, monkeypatch):
    w = world["c"]
    c = w["c"]
    C = c["x"].shape[1]
    calls = []
    real = ops.cost_volume_backward
    monkeypatch.setattr(ops, "cost_volume_backward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run():
        x, xa, cams, bins = _on(c, dev)
        x.requires_grad_(True), xa.requires_grad_(True)
        out = CostVolumeFunction.apply(x, xa, cams, bins, c["H"], c["W"], ops.COST_VOLUME_FOV_SCALE, True)
        return torch.autograd.grad((out * w["lw"].to(dev)).sum(), (x, xa))

    monkeypatch.delenv("MCR_COST_VOLUME_BWD", raising=False)
    hip = run()
    assert autograd.cost_volume_backward_mode() == "hip" and len(calls) == 1
    monkeypatch.setenv("MCR_COST_VOLUME_BWD", "composite")
    comp = run()
    assert autograd.cost_volume_backward_mode() == "composite" and len(calls) == 1          # the old route: the entry was not called
    for name, h, k, r in zip(("x", "x_alpha"), hip, comp, (w["ref"][0] + w["lw"][:, :C].double(), w["ref"][1])):
        e = float((h - k).abs().max() / r.abs().max())
        print(f"ERR routes: gradient of {name}, HIP vs composite: {e:.2e} (composite vs model {rel(k, r):.2e})")
        assert e < 2 * TOL


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, world):
    w = world["c"]
    c = w["c"]
    x, xa, cams, bins = _on(c, dev)
    B, C, Hf, Wf = x.shape
    A, D = xa.shape[1], c["D"]
    d_out = w["lw"][:, C:].contiguous().to(dev)
    with pytest.raises(_lib.MacaronsHipError, match="64"):                      # C != 64
        ops.cost_volume_backward(x[:, :32].contiguous(), xa[:, :, :32].contiguous(), cams, bins, d_out, c["H"], c["W"])
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):              # a CPU tensor
        ops.cost_volume_backward(x, c["x_alpha"], cams, bins, d_out, c["H"], c["W"])
    with pytest.raises(ValueError, match="d_out"):                              # a d_out of the wrong shape
        ops.cost_volume_backward(x, xa, cams, bins, d_out[:, 1:], c["H"], c["W"])
    # at the C ABI: the outputs hold a sentinel and keep it
    L = _lib.lib()
    i64, ci = ctypes.c_int64, ctypes.c_int
    need = int(L.mcr_cost_volume_backward_workspace_bytes(i64(B), i64(A), i64(C), i64(Hf), i64(Wf), i64(D)))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d_x, d_xa = torch.full_like(x, -7.25), torch.full_like(xa, -7.25)

    def entry(p_dx, p_dxa, ws_bytes):
        return L.mcr_cost_volume_backward(ops._p(x), ops._p(xa), ops._p(cams), ops._p(bins), ops._p(d_out), i64(D * Hf * Wf), p_dx, p_dxa, i64(B),
                                          ci(A), ci(C), ci(c["H"]), ci(c["W"]), ci(Hf), ci(Wf), ci(D), ctypes.c_float(ops.COST_VOLUME_FOV_SCALE),
                                          ops._p(ws), ctypes.c_size_t(ws_bytes), ops._stream())

    assert entry(ops._p(d_x), ops._p(d_xa), need - 1) != 0 and b"workspace" in L.mcr_last_error()
    assert entry(None, None, need) != 0 and b"nothing to do" in L.mcr_last_error()
    torch.cuda.synchronize()
    assert bool((d_x == -7.25).all()) and bool((d_xa == -7.25).all())          # refused before any launch
    assert entry(ops._p(d_x), ops._p(d_xa), need) == 0                          # and the same call with its workspace runs
    torch.cuda.synchronize()
    _check("case c, C ABI", (d_x, d_xa), w["ref"])
