"""The expansion layer's backward without a GPU: the fp64 model of the six gradients (tests/_expansion_layer_backward_model.py) against
torch's autograd through the composite in float64 and against the reference's own layer under autograd
(tests/golden/expansion_layer_backward.npz); the exact operands' headroom; that the real-valued cases exercise both branches of both ELU
derivatives; the C ABI's size function and refusals; the argument checks of ops.expansion_layer_backward; the 'function' route of
networks.ManyDepth for every reason that keeps a forward off it; and ExpansionLayerFunction's composite backward on the CPU.

Bounds.  Model against float64 autograd: 1e-10 of the largest magnitude.  Model against golden: the golden's stored distance (the
reference's fp32 against this model, measured by the generator, at most 8.7e-7, asserted below 1e-5) plus 1e-5.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expansion_layer_backward_model as bmodel                      # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

KEYS = ("x", "x_add", "up_weight", "up_bias", "i_weight", "i_bias")
NAMES = bmodel.NAMES


def t(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(dtype)


def autograd_of(c, d_y, dtype):
    """name -> the gradient of sum(d_y * composite) by torch's autograd, in `dtype` on the CPU."""
    leaves = [None if c[k] is None else t(c[k], dtype).requires_grad_(True) for k in KEYS]
    y = ManyDepth.expansion_layer_composite(*leaves, c["output_size"])
    grads = iter(torch.autograd.grad(y, [v for v in leaves if v is not None], t(d_y, dtype)))
    return {k: None if v is None else next(grads) for k, v in zip(NAMES, leaves)}


@pytest.fixture(scope="module")
def modelled():
    cache = {}

    def get(tag):
        if tag not in cache:
            c, d_y = bmodel.make_inputs(tag), bmodel.make_d_y(tag)
            cache[tag] = (c, d_y, bmodel.backward(*bmodel.args_of(c), d_y))
        return cache[tag]

    return get


# ---- 1, 2. the model against autograd and against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", bmodel.ALL_TAGS)
def test_model_matches_autograd_in_float64(modelled, tag):
    c, d_y, got = modelled(tag)
    want = autograd_of(c, d_y, torch.float64)
    e = {k: bmodel.rel(got[k], v.numpy()) for k, v in want.items() if v is not None}
    print(f"ERR case {tag}, model vs autograd through the composite (float64): " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert (got["d_x_add"] is None) == (c["x_add"] is None) and len(e) == (5 if c["x_add"] is None else 6)
    assert all(got[k].shape == tuple(want[k].shape) for k in e) and max(e.values()) < 1e-10


@pytest.mark.parametrize("tag", bmodel.GOLDEN_TAGS)
def test_model_matches_golden(modelled, tag):
    c, d_y, got = modelled(tag)
    g = bmodel.load_golden_backward(tag)
    assert np.array_equal(g["d_y"], d_y) and (g["d_x_add"] is None) == (c["x_add"] is None)
    e = {k: bmodel.rel(got[k], g[k]) for k in g["distance"]}
    print(f"ERR case {tag}, model vs golden: " + " ".join(f"{k} {v:.2e} (stored {g['distance'][k]:.2e})" for k, v in e.items()))
    for k, v in e.items():
        assert g[k].dtype == np.float32 and g["distance"][k] < 1e-5 and v <= g["distance"][k] + 1e-5, k


def test_golden_holds_data_only():
    z = np.load(bmodel.GOLDEN)
    assert os.path.getsize(bmodel.GOLDEN) < 2 ** 20 and all(z[k].dtype in (np.float32, np.float64) for k in z.files)
    assert not any(k.endswith(("_x", "_x_add", "_up_weight", "_i_weight")) and not k.split("_", 1)[1].startswith("d_") for k in z.files)


# ---- 3, 4. the operands of the GPU tests --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", bmodel.ALL_TAGS)
def test_exact_operands_have_headroom(tag):
    e, d_y = bmodel.make_exact_backward(tag)
    room = bmodel.exact_headroom_backward(e, d_y)
    got = bmodel.backward(*bmodel.args_of(e), d_y)
    print(f"ERR case {tag}, exact operands: headroom " + " ".join(f"{k} 2^{np.log2(max(v, 1.0)):.1f}" for k, v in room.items())
          + f", {int((d_y != 0).sum())} non-zeros in d_y")
    assert max(room.values()) < 2 ** 24, room
    assert got["z1"].min() > 0 and got["z2"].min() > 0 and (d_y != 0).any() and d_y.min() >= 0 and d_y.max() <= 3
    for k in NAMES:
        if got[k] is None:
            continue
        q = got[k] / bmodel.EXACT_UNITS[k]
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= room[k], k       # integer multiples of the unit, within the bound
        assert np.array_equal(got[k].astype(np.float32).astype(np.float64), got[k]), k
    assert np.abs(got["d_x"]).max() > 0 and np.abs(got["d_up_weight"]).max() > 0 and np.abs(got["d_i_weight"]).max() > 0


@pytest.mark.parametrize("tag", bmodel.ALL_TAGS)
def test_real_cases_take_both_branches_of_both_elus(modelled, tag):
    _, _, got = modelled(tag)
    for name in ("z1", "z2"):
        z = got[name]
        if z.size <= 64:
            continue
        pos = float((z > 0).mean())
        assert 0.1 <= pos <= 0.9, (tag, name, pos)


# ---- 5. symbols and ABI without a device ------------------------------------------------------------------------------------------------------------
def test_symbols_and_workspace_arithmetic():
    names, L = _lib.declared_symbols(), _lib.lib()
    for n in ("mcr_expansion_layer_backward", "mcr_expansion_layer_backward_workspace_bytes"):
        assert n in names and hasattr(L, n), n
    size, i64 = L.mcr_expansion_layer_backward_workspace_bytes, ctypes.c_int64
    assert size.restype is ctypes.c_size_t

    def r(n_floats):
        return (4 * n_floats + 255) // 256 * 256

    # case b (2,3,2,3,5, 3x5 -> 7x9): g2 [2,5,7,9], G [2,5,9,11], g1 [2,2,3,5]; the partials: the convolution's pass has 2 x 2 pixel tiles
    # of 4 x 32, one part each, 5 * 5 * 9 + 5 outputs; the transposed convolution's 2 parts of 3 * 2 * 9 + 2: the larger of the two
    assert size(*(i64(v) for v in (2, 3, 2, 3, 5, 3, 5, 7, 9))) == r(630) + r(990) + r(60) + r(max(4 * 230, 2 * 56)) == 10752
    # upstream's expansion5 at B 1: 128 blocks of 32 x 32 channel pairs in either pass; 4 pixel tiles and parts over 16 x 29, 2 over 8 x 15
    n_out = 256 * 512 * 9 + 256
    assert size(*(i64(v) for v in (1, 512, 256, 256, 256, 8, 15, 16, 29))) == r(256 * 464) + r(512 * 18 * 31) + r(256 * 120) + r(4 * n_out) \
        == 20619264
    for bad in ((0, 1, 1, 0, 1, 1, 1, 2, 2), (1, 0, 1, 0, 1, 1, 1, 2, 2), (1, 513, 1, 0, 1, 1, 1, 2, 2), (1, 1, 513, 0, 1, 1, 1, 2, 2),
                (1, 1, 257, 256, 1, 1, 1, 2, 2), (1, 1, 1, -1, 1, 1, 1, 2, 2), (1, 1, 1, 0, 0, 1, 1, 2, 2), (1, 1, 1, 0, 513, 1, 1, 2, 2),
                (1, 1, 1, 0, 1, 0, 1, 2, 2), (1, 1, 1, 0, 1, 1, 0, 2, 2), (1, 1, 1, 0, 1, 1, 1, 1, 2), (1, 1, 1, 0, 1, 1, 1, 2, 1),
                (2 ** 22, 512, 1, 0, 1, 1, 1, 2, 2), (2 ** 18, 1, 256, 256, 1, 1, 1, 2, 2)):
        assert size(*(i64(v) for v in bad)) == 0, bad
    assert size(*(i64(v) for v in (1, 1, 1, 0, 1, 1, 1, 2, 2))) > 0


def test_entry_refuses_without_a_device():
    """Every refusal precedes the first launch, so it can be asked for where there is no GPU; the pointers are never followed."""
    L, i64, ci, vp, sz = _lib.lib(), ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    p = vp(4096)

    def call(B=1, Cin=3, Cmid=2, Cadd=3, Cout=5, h=3, w=5, H=7, W=9, x=p, x_add=p, u=p, d_y=p, outs=(p,) * 6, ws=p, ws_bytes=1 << 40):
        return L.mcr_expansion_layer_backward(x, x_add, p, p, u, p, d_y, *outs, i64(B), ci(Cin), ci(Cmid), ci(Cadd), ci(Cout), ci(h), ci(w),
                                              ci(H), ci(W), ws, sz(ws_bytes), None)

    for bad in (dict(H=1), dict(W=1), dict(h=0), dict(w=0), dict(Cin=0), dict(Cin=513), dict(Cmid=0), dict(Cmid=513, Cadd=0), dict(Cout=0),
                dict(Cout=513), dict(Cadd=-1), dict(Cmid=257, Cadd=256), dict(B=0), dict(B=-1), dict(B=2 ** 22, Cin=512, h=1, w=1),
                dict(B=2 ** 20, Cout=512, H=2, W=2), dict(B=2 ** 20, Cadd=400, H=2, W=3), dict(B=2 ** 20, Cmid=512, Cadd=0, h=2, w=2),
                dict(B=2 ** 18, Cmid=256, Cadd=256, Cout=1, H=2, W=2),                      # only the padded correlation is too large
                dict(x=None), dict(x_add=None), dict(u=None), dict(d_y=None), dict(outs=(None,) * 6),
                dict(Cadd=0, x_add=None),                                                   # d_x_add with Cadd = 0
                dict(ws=None), dict(ws_bytes=16), dict(ws=vp(4100))):
        assert call(**bad) == 1, bad
        msg = L.mcr_last_error().decode()
        assert msg.startswith("mcr_expansion_layer_backward") and "kernel" not in msg, (bad, msg)
    assert call(outs=(None,) * 6) == 1 and "all six" in L.mcr_last_error().decode()
    assert call(Cadd=0, x_add=None) == 1 and "d_x_add" in L.mcr_last_error().decode()
    assert call(ws_bytes=16) == 1 and "workspace" in L.mcr_last_error().decode()


# ---- 6. ops.expansion_layer_backward: the argument checks ---------------------------------------------------------------------------------------------
def test_ops_argument_checks(monkeypatch):
    def no_library():
        raise AssertionError("an argument check let a call through to the library")

    z = torch.zeros
    good = dict(x=z(2, 3, 3, 5), x_add=z(2, 3, 7, 9), wu=z(3, 2, 3, 3), wi=z(5, 5, 3, 3), u=z(2, 2, 3, 5), y=z(2, 5, 7, 9), d_y=z(2, 5, 7, 9),
                size=(7, 9), need=(True,) * 6)
    call = lambda a: ops.expansion_layer_backward(a["x"], a["x_add"], a["wu"], a["wi"], a["u"], a["y"], a["d_y"], a["size"], need=a["need"])  # noqa: E731
    monkeypatch.setattr(ops, "lib", no_library)
    for bad in (dict(x=z(3, 3, 5)), dict(x=z(0, 3, 3, 5)), dict(x=z(2, 4, 3, 5)), dict(x=None), dict(size=(1, 9)), dict(size=7),
                dict(x_add=z(2, 3, 7, 8)), dict(x_add=z(2, 4, 7, 9)), dict(x_add=None), dict(wu=z(3, 2, 3)), dict(wu=z(3, 4, 3, 3)),
                dict(wi=z(5, 5, 1, 1)), dict(wi=z(513, 5, 3, 3)), dict(u=z(2, 2, 3, 4)), dict(u=z(2, 3, 3, 5)), dict(u=None),
                dict(y=z(2, 5, 7, 8)), dict(y=z(2, 4, 7, 9)), dict(d_y=z(2, 5, 9, 7)), dict(d_y=z(5, 7, 9)), dict(d_y=None),
                dict(need=(False,) * 6), dict(need=(True,) * 5), dict(need=(True,) * 7)):
        args = dict(good)
        args.update(bad)
        with pytest.raises(ValueError):
            call(args)
    with pytest.raises(ValueError, match="at least one"):               # d_x_add alone, and no x_add to take it
        ops.expansion_layer_backward(good["x"], None, good["wu"], z(5, 2, 3, 3), good["u"], good["y"], good["d_y"], (7, 9),
                                     need=(False, True, False, False, False, False))
    big = z(1).expand(2 ** 20, 512, 2, 2)                                # 2^31 elements, no memory behind them
    with pytest.raises(ValueError, match="2\\^31"):
        ops.expansion_layer_backward(big, None, z(512, 1, 3, 3), z(1, 1, 3, 3), z(1), z(1), z(1), (2, 2))
    ring = z(1).expand(2 ** 18, 1, 1, 1)                                 # only G [B,512,4,4] has 2^31 elements
    with pytest.raises(ValueError, match="2\\^31"):
        ops.expansion_layer_backward(ring, z(1).expand(2 ** 18, 256, 2, 2), z(1, 256, 3, 3), z(1, 512, 3, 3), z(1).expand(2 ** 18, 256, 1, 1),
                                     z(1).expand(2 ** 18, 1, 2, 2), z(1).expand(2 ** 18, 1, 2, 2), (2, 2))
    monkeypatch.undo()
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):      # well-formed CPU tensors: no fall-back to torch
        call(good)


# ---- 7. the route ---------------------------------------------------------------------------------------------------------------------------------
def stand_in():
    """A plain nn.Module with upstream's attributes (ManyDepth.py:308-344), case b's sizes."""
    m = nn.Module()
    m.upconv, m.upelu = nn.ConvTranspose2d(3, 2, kernel_size=3, stride=1, padding=1), nn.ELU()
    m.iconv, m.ielu = nn.Conv2d(5, 5, kernel_size=3, stride=1, padding=1, padding_mode="reflect"), nn.ELU()
    m.input_channels, m.output_channels, m.output_size, m.inner_channels, m.additional_channels = 3, 5, (7, 9), 2, 3
    m.kernel_size, m.stride, m.padding = 3, 1, 1
    return m


def test_backward_mode_switch(monkeypatch):
    monkeypatch.delenv("MCR_EXPANSION_LAYER_BWD", raising=False)
    assert autograd.expansion_layer_backward_mode() == "composite"
    for value, want in (("hip", "hip"), ("HIP", "hip"), ("composite", "composite"), ("", "composite"), ("other", "composite"), ("1", "composite")):
        monkeypatch.setenv("MCR_EXPANSION_LAYER_BWD", value)
        assert autograd.expansion_layer_backward_mode() == want, value


def test_function_route_for_every_fallback_reason(monkeypatch):
    """CPU tensors stand for HIP tensors (the device predicate is replaced), ops.expansion_layer and ExpansionLayerFunction.apply are
    recorders: 'function' exactly when a gradient is recorded, the mode is hip and the forward's conditions hold."""
    entry_calls, fn_calls = [], []
    monkeypatch.setattr(ops, "expansion_layer", lambda *a, **k: entry_calls.append(a) or "fused")
    monkeypatch.setattr(autograd.ExpansionLayerFunction, "apply", staticmethod(lambda *a: fn_calls.append(a) or "function"))
    layer = ManyDepth.ExpansionLayer(3, 2, 5, (7, 9), additional_channels=3)
    adopted = ManyDepth.adopt_expansion_layer(stand_in())
    x, x_add = torch.randn(2, 3, 3, 5), torch.randn(2, 3, 7, 9)
    xg = x.clone().requires_grad_(True)

    def via_function(m, *a, **k):
        n, e = len(fn_calls), len(entry_calls)
        out = m(*a, **k)
        return len(fn_calls) == n + 1 and len(entry_calls) == e and isinstance(out, str) and out == "function"

    monkeypatch.setenv("MCR_EXPANSION_LAYER_BWD", "hip")
    monkeypatch.delenv("MCR_EXPANSION_LAYER", raising=False)
    assert not via_function(layer, x, x_add)                            # CPU tensors
    monkeypatch.setattr(ManyDepth, "_is_hip_tensor", lambda v: True)
    for m in (layer, adopted):
        m.requires_grad_(True)
        for forward_knob in (None, "hip", "composite"):                 # the forward's knob has no say under a gradient
            if forward_knob is None:
                monkeypatch.delenv("MCR_EXPANSION_LAYER", raising=False)
            else:
                monkeypatch.setenv("MCR_EXPANSION_LAYER", forward_knob)
            assert via_function(m, x, x_add) and via_function(m, x=x, x_add=x_add)
            got = fn_calls[-1]
            assert got[0] is x and got[1] is x_add and got[2] is m.upconv.weight and got[3] is m.upconv.bias and got[4] is m.iconv.weight \
                and got[5] is m.iconv.bias and tuple(got[6]) == (7, 9)
        monkeypatch.delenv("MCR_EXPANSION_LAYER", raising=False)
        m.requires_grad_(False)
        assert not via_function(m, x, x_add)                            # nothing requires a gradient
        assert via_function(m, xg, x_add) and via_function(m, x, x_add.clone().requires_grad_(True))   # an input does
        for prm in (m.upconv.weight, m.upconv.bias, m.iconv.weight, m.iconv.bias):
            prm.requires_grad_(True)
            assert via_function(m, x, x_add)                            # one parameter does
            prm.requires_grad_(False)
        with torch.no_grad():
            assert not via_function(m, xg, x_add)                       # grad mode off: nothing is recorded
        # every single reason for falling back, one at a time, around a call that goes to the Function
        assert via_function(m, xg, x_add)
        assert not via_function(m, xg.transpose(2, 3).contiguous().transpose(2, 3), x_add)              # a strided x
        assert not via_function(m, xg, x_add.transpose(2, 3).contiguous().transpose(2, 3))              # a strided x_add
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not via_function(m, xg, x_add)                       # autocast
        monkeypatch.setattr(ManyDepth, "_is_hip_tensor", lambda v: v is not x_add)
        assert not via_function(m, xg, x_add)                           # an operand elsewhere
        monkeypatch.setattr(ManyDepth, "_is_hip_tensor", lambda v: True)
        n = len(fn_calls)
        with pytest.raises(RuntimeError):
            m(xg, None)                                                 # additional_channels without x_add: the composite, failing as upstream does
        assert len(fn_calls) == n
        # the variable unset (or anything but hip): the composite under a gradient whatever MCR_EXPANSION_LAYER says
        for bwd in (None, "composite", "1"):
            if bwd is None:
                monkeypatch.delenv("MCR_EXPANSION_LAYER_BWD")
            else:
                monkeypatch.setenv("MCR_EXPANSION_LAYER_BWD", bwd)
            for forward_knob in ("hip", "composite"):
                monkeypatch.setenv("MCR_EXPANSION_LAYER", forward_knob)
                n, e = len(fn_calls), len(entry_calls)
                y = m(xg, x_add)
                assert isinstance(y, torch.Tensor) and y.grad_fn is not None and len(fn_calls) == n and len(entry_calls) == e
            monkeypatch.delenv("MCR_EXPANSION_LAYER")
        monkeypatch.setenv("MCR_EXPANSION_LAYER_BWD", "hip")
    layer64 = ManyDepth.ExpansionLayer(3, 2, 5, (7, 9), additional_channels=3).double()
    assert not via_function(layer64, xg.double(), x_add.double())       # another dtype
    params = (layer.upconv.weight, layer.upconv.bias, layer.iconv.weight, layer.iconv.bias)
    assert ManyDepth.expansion_layer_route(xg, x_add, params, (7, 9), 3) == "function"
    assert ManyDepth.expansion_layer_route(x, x_add, params, (7, 9), 3) == "composite"                # no gradient, the forward's knob unset
    monkeypatch.setenv("MCR_EXPANSION_LAYER", "hip")
    assert ManyDepth.expansion_layer_route(x, x_add, params, (7, 9), 3) == "hip"                      # ... and set: the forward's own route
    assert ManyDepth.expansion_layer_route(xg, None, params, (7, 9), 3) == "composite"
    assert ManyDepth.expansion_layer_route(xg, x_add, params, (1, 9), 3) == "composite"               # outside the entry's limits: H = 1
    wide = (torch.zeros(3, 513, 3, 3), torch.zeros(513), torch.zeros(5, 513, 3, 3), torch.zeros(5))
    assert ManyDepth.expansion_layer_route(xg, None, wide, (7, 9), None) == "composite"               # 513 channels
    ring = torch.zeros(1).expand(2 ** 18, 1, 1, 1).requires_grad_(True)                                 # only the backward's G is too large
    many = (torch.zeros(1, 256, 3, 3), torch.zeros(256), torch.zeros(1, 512, 3, 3), torch.zeros(1))
    assert ManyDepth.expansion_layer_route(ring, torch.zeros(1).expand(2 ** 18, 256, 2, 2), many, (2, 2), 256) == "composite"


# ---- 8. the Function's composite backward on the CPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "g"])
def test_function_composite_backward_is_the_composites_autograd(monkeypatch, tag):
    """The forward entry is replaced by the float32 composite (u is never read on this route); the Function's backward in the mode
    'composite' must give torch's own gradients of the composite bit for bit, and None where no gradient is needed."""
    monkeypatch.delenv("MCR_EXPANSION_LAYER_BWD", raising=False)
    c, d_y = bmodel.make_inputs(tag), bmodel.make_d_y(tag)

    def entry(x, x_add, wu, bu, wi, bi, size, return_u=False):
        assert return_u
        return ManyDepth.expansion_layer_composite(x, x_add, wu, bu, wi, bi, size), torch.zeros(x.shape[0], wu.shape[1], *x.shape[2:])

    monkeypatch.setattr(ops, "expansion_layer", entry)
    want = autograd_of(c, d_y, torch.float32)
    leaves = [None if c[k] is None else t(c[k]).requires_grad_(True) for k in KEYS]
    y = autograd.ExpansionLayerFunction.apply(*leaves, c["output_size"])
    y.backward(t(d_y))
    for k, v in zip(NAMES, leaves):
        assert (v is None and want[k] is None) or torch.equal(v.grad, want[k]), k
    only_x = [None if c[k] is None else t(c[k]).requires_grad_(k == "x") for k in KEYS]
    autograd.ExpansionLayerFunction.apply(*only_x, c["output_size"]).backward(t(d_y))
    assert torch.equal(only_x[0].grad, want["d_x"]) and all(v is None or v.grad is None for v in only_x[1:])
    with pytest.raises(RuntimeError, match="once"):                      # differentiable once
        x = t(c["x"]).requires_grad_(True)
        y = autograd.ExpansionLayerFunction.apply(x, *[None if c[k] is None else t(c[k]) for k in KEYS[1:]], c["output_size"])
        torch.autograd.grad(y, x, t(d_y), create_graph=True)
