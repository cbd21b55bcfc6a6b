"""The disparity head without a GPU: the fp64 model (tests/_disparity_head_model.py) and the torch composite against the reference's own
DisparityLayer (tests/golden/disparity_head.npz), the mirror class and the adoption seam of networks.ManyDepth, the argument checks of
ops.disparity_head / disparity_head_backward, the C ABI's size function and refusals, the backward-mode switch.

Bounds.  Model against golden: the golden's stored distance (the reference's fp32 against this model, measured by the generator, at most
6e-7) plus the contract TOL = 1e-4 of the largest magnitude.  Composite (fp32, CPU) against golden: TOL -- both are torch's fp32
convolution; the composite in fp64 against the model: 1e-12.
"""
import copy
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _disparity_head_model as model                                  # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

TOL = 1e-4


def t(x):
    return torch.as_tensor(np.asarray(x))


def stand_in(input_channels, **conv):
    """A plain nn.Module with upstream's attributes (ManyDepth.py:366-384: channels, conv, sigmoid) -- an instance of a class this test
    module does not define, so that it pickles wherever the tests are imported from."""
    m = nn.Module()
    args = dict(in_channels=input_channels, out_channels=1, kernel_size=3, stride=1, padding=1, padding_mode="reflect")
    args.update(conv)
    m.channels, m.conv, m.sigmoid = input_channels, nn.Conv2d(**args), nn.Sigmoid()
    return m


def upstream_forward(m, x):
    return m.sigmoid(m.conv(x))


# ---- the model and the composite against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", model.GOLDEN_TAGS)
def test_model_matches_golden(tag):
    g = model.load_golden(tag)
    assert tuple(g["x"].shape) == model.CASES[tag]["shape"]
    inp = model.make_inputs(tag)
    assert all(np.array_equal(inp[k].reshape(-1), g[k].reshape(-1)) for k in ("x", "weight", "bias", "g_out"))     # the stored inputs are the seeded ones
    _, y = model.forward(g["x"], g["weight"], g["bias"])
    grads = dict(zip(("d_x", "d_weight", "d_bias"), model.backward(g["x"], g["weight"], y, g["g_out"])))
    e = dict(y=model.rel(g["y"], y), **{k: model.rel(g[k], v) for k, v in grads.items()})
    print(f"ERR case {tag}, model vs golden: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= g["distance"][k] + TOL and g["distance"][k] < 1e-5, k


@pytest.mark.parametrize("tag", model.GOLDEN_TAGS)
def test_composite_matches_golden_and_model(tag):
    g = model.load_golden(tag)
    for dtype, tol in ((torch.float32, TOL), (torch.float64, 1e-12)):
        x, w, b = (t(g[k]).to(dtype).requires_grad_(True) for k in ("x", "weight", "bias"))
        y = ManyDepth.disparity_head_composite(x, w, b)
        assert tuple(y.shape) == tuple(g["y"].shape) and y.dtype == dtype
        (y[:, 0] * t(g["g_out"]).to(dtype)).sum().backward()
        got = dict(y=y.detach(), d_x=x.grad, d_weight=w.grad, d_bias=b.grad)
        if dtype == torch.float32:
            want = g
        else:
            _, ym = model.forward(g["x"], g["weight"], g["bias"])
            want = dict(zip(("d_x", "d_weight", "d_bias"), model.backward(g["x"], g["weight"], ym, g["g_out"])), y=ym)
        e = {k: model.rel(v.numpy(), want[k]) for k, v in got.items()}
        print(f"ERR case {tag}, composite ({dtype}) vs {'golden' if dtype == torch.float32 else 'model'}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) < tol


def test_model_fold_on_a_two_pixel_axis():
    """Hs = Ws = 2 by hand: pixel (0,0) is read by every output pixel; the taps that reach it are counted from the padded array."""
    x = np.zeros((1, 1, 2, 2))
    w = np.arange(1.0, 10.0).reshape(1, 3, 3)
    g = np.array([[[1.0, 10.0], [100.0, 1000.0]]])
    d_x = model.backward_from_g(x, w, g)[0]
    # padded 4 x 4 of [[a,b],[c,d]] is [[d,c,d,c],[b,a,b,a],[d,c,d,c],[b,a,b,a]]: a sits at padded (1,1), (1,3), (3,1), (3,3)
    want_a = sum(w[0, pi - i, pj - j] * g[0, i, j] for pi in (1, 3) for pj in (1, 3) for i in (0, 1) for j in (0, 1)
                 if 0 <= pi - i <= 2 and 0 <= pj - j <= 2)
    assert d_x[0, 0, 0, 0] == want_a


# ---- the mirror class ------------------------------------------------------------------------------------------------------------------------
def test_mirror_loads_the_reference_state_dict():
    z = np.load(model.GOLDEN)
    names, shapes = [str(n) for n in z["state_dict_names"]], [tuple(int(v) for v in str(s).split(",")) for s in z["state_dict_shapes"]]
    assert names == ["conv.bias", "conv.weight"] and shapes == [(1,), (1, 1, 3, 3)]
    for tag in model.GOLDEN_TAGS:
        g = model.load_golden(tag)
        C = model.CASES[tag]["shape"][1]
        layer = ManyDepth.DisparityLayer(C)
        assert layer.channels == C and sorted(layer.state_dict()) == names
        layer.load_state_dict({"conv.weight": t(g["weight"]), "conv.bias": t(g["bias"])}, strict=True)
        with torch.no_grad():
            y = layer(t(g["x"]))                                        # on the CPU: the composite
        assert tuple(y.shape) == tuple(g["y"].shape) and model.rel(y.numpy(), g["y"]) < TOL


def test_mirror_on_the_cpu_is_the_composite():
    g = model.load_golden("b")
    layer = ManyDepth.DisparityLayer(3)
    layer.load_state_dict({"conv.weight": t(g["weight"]), "conv.bias": t(g["bias"])})
    x = t(g["x"]).requires_grad_(True)
    y = layer(x)
    assert torch.equal(y, ManyDepth.disparity_head_composite(x, layer.conv.weight, layer.conv.bias)) and y.requires_grad
    assert layer.double()(t(g["x"]).double()).dtype == torch.float64   # another dtype: the composite as well


# ---- adoption --------------------------------------------------------------------------------------------------------------------------------
def test_adopt_disparity_layer():
    torch.manual_seed(5)
    layer = stand_in(3)
    x = torch.randn(2, 3, 3, 5)
    want = upstream_forward(layer, x)
    assert ManyDepth.adopt_disparity_layer(layer) is layer
    fwd = vars(layer)["forward"]
    assert ManyDepth.adopt_disparity_layer(layer) is layer and vars(layer)["forward"] is fwd          # idempotent
    got = layer(x)
    assert torch.equal(got, ManyDepth.disparity_head_composite(x, layer.conv.weight, layer.conv.bias))  # the CPU fallback, bit for bit
    assert torch.equal(got, want)                                       # which is upstream's op sequence
    for clone in (pickle.loads(pickle.dumps(layer)), copy.deepcopy(layer)):
        assert isinstance(vars(clone)["forward"], type(fwd)) and vars(clone)["forward"].layer is clone
        assert torch.equal(clone(x), want)
        with torch.no_grad():
            clone.conv.bias += 1.0                                      # the clone's forward reads the clone's parameters
        assert not torch.equal(clone(x), want) and torch.equal(layer(x), want)
    got.sum().backward()
    assert layer.conv.weight.grad is not None


@pytest.mark.parametrize("conv", [dict(padding_mode="zeros"), dict(out_channels=2), dict(kernel_size=5, padding=2), dict(stride=2),
                                  dict(padding=2), dict(bias=False)])
def test_adopt_refuses_another_convolution(conv):
    with pytest.raises(TypeError, match="adopt_disparity_layer"):
        ManyDepth.adopt_disparity_layer(stand_in(4, **conv))
    with pytest.raises(TypeError, match="adopt_disparity_layer"):
        ManyDepth.adopt_disparity_layer(nn.Linear(2, 2))


def test_adopt_depth_decoder():
    builder = nn.Module()
    builder.height, builder.width, builder.feature_height, builder.feature_width, builder.feature_channels = 8, 12, 4, 6, 2
    builder.n_alpha, builder.d_min, builder.d_max, builder.n_depth = 1, 0.5, 2.0, 3
    builder.depth_bins = torch.linspace(0.5, 2.0, 3)
    builder.conv_reduce = nn.Conv2d(5, 2, 3, padding=1)
    dec = nn.Module()
    dec.cost_volume_builder = builder
    dec.disp1, dec.disp2, dec.disp3, dec.disp4 = (stand_in(c) for c in (16, 32, 64, 128))
    assert ManyDepth.adopt_depth_decoder(dec) is dec
    assert isinstance(vars(dec.cost_volume_builder)["forward"], ManyDepth._AdoptedForward)
    assert all(isinstance(vars(getattr(dec, f"disp{k}"))["forward"], ManyDepth._AdoptedHeadForward) for k in (1, 2, 3, 4))
    copy.deepcopy(dec), pickle.loads(pickle.dumps(dec))
    with pytest.raises(TypeError, match="adopt_depth_decoder"):
        ManyDepth.adopt_depth_decoder(stand_in(3))


# ---- ops: the argument checks ------------------------------------------------------------------------------------------------------------------
def test_ops_argument_checks():
    x, w, b = torch.zeros(2, 3, 4, 5), torch.zeros(1, 3, 3, 3), torch.zeros(1)
    y = torch.zeros(2, 1, 4, 5)
    for bad in (dict(x=torch.zeros(3, 4, 5)), dict(x=torch.zeros(2, 3, 1, 5)), dict(x=torch.zeros(2, 3, 4, 1)), dict(x=torch.zeros(0, 3, 4, 5)),
                dict(x=torch.zeros(1, 513, 2, 2), w=torch.zeros(1, 513, 3, 3)), dict(w=torch.zeros(1, 4, 3, 3)), dict(w=torch.zeros(3, 9)),
                dict(b=torch.zeros(2))):
        args = dict(x=x, w=w, b=b)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.disparity_head(args["x"], args["w"], args["b"])
        if "b" not in bad:
            with pytest.raises(ValueError):
                ops.disparity_head_backward(args["x"], args["w"], y, y)
    with pytest.raises(ValueError):
        ops.disparity_head_backward(x, w, y, torch.zeros(2, 1, 4, 6))
    with pytest.raises(ValueError, match="at least one"):
        ops.disparity_head_backward(x, w, y, y, need=(False, False, False))
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):      # well-formed CPU tensors: no fall-back to torch
        ops.disparity_head(x, w, b)
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):
        ops.disparity_head_backward(x, w, y, y)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("mcr_disparity_head", "mcr_disparity_head_backward_workspace_bytes", "mcr_disparity_head_backward")


def test_symbols_declared_and_exported():
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in SYMBOLS:
        assert n in names and hasattr(L, n), n


def test_workspace_arithmetic():
    size = _lib.lib().mcr_disparity_head_backward_workspace_bytes
    assert size.restype is ctypes.c_size_t
    i64 = ctypes.c_int64

    def up(v):
        return (v + 255) // 256 * 256

    for B, C, Hs, Ws in ((1, 1, 2, 2), (2, 3, 3, 5), (1, 16, 17, 33), (2, 128, 32, 57), (4, 16, 256, 456), (1, 512, 2, 3), (1, 9, 129, 513)):
        tiles = ((Hs + 15) // 16) * ((Ws + 63) // 64)                   # one float per output and 64 x 16 tile of every image
        assert size(i64(B), i64(C), i64(Hs), i64(Ws)) == up(4 * (9 * C + 1) * B * tiles), (B, C, Hs, Ws)
    for B, C, Hs, Ws in ((0, 1, 4, 4), (-1, 1, 4, 4), (1, 0, 4, 4), (1, 513, 4, 4), (1, 1, 1, 4), (1, 1, 4, 1), (1, 1, -4, 4),
                         (2 ** 29, 1, 2, 2), (1, 512, 2 ** 11, 2 ** 11), (1, 1, 2 ** 16, 2 ** 16), (2 ** 40, 2, 2 ** 31, 2 ** 31)):
        assert size(i64(B), i64(C), i64(Hs), i64(Ws)) == 0, (B, C, Hs, Ws)
    assert size(i64(2 ** 29 - 1), i64(1), i64(2), i64(2)) > 0          # the largest operand just fits


def test_c_entries_refuse_on_the_host():
    """The refusals come before anything touches a device: they can be asked for without one (the pointers are never read)."""
    L = _lib.lib()
    i64, ci, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    p = vp(4096)
    for B, C, Hs, Ws in ((1, 1, 1, 4), (1, 1, 4, 1), (1, 0, 4, 4), (1, 513, 4, 4), (0, 1, 4, 4), (2 ** 29, 1, 2, 2), (1, 512, 2 ** 11, 2 ** 11)):
        assert L.mcr_disparity_head(p, p, p, p, None, i64(B), ci(C), ci(Hs), ci(Ws), None) == 1
        assert L.mcr_last_error().decode().startswith("mcr_disparity_head:"), (B, C, Hs, Ws)
        assert L.mcr_disparity_head_backward(p, p, p, p, p, p, p, i64(B), ci(C), ci(Hs), ci(Ws), p, sz(1 << 30), None) == 1
        assert L.mcr_last_error().decode().startswith("mcr_disparity_head_backward:"), (B, C, Hs, Ws)
    assert L.mcr_disparity_head_backward(p, p, p, p, None, None, None, i64(1), ci(1), ci(4), ci(4), p, sz(1 << 20), None) == 1
    assert "all NULL" in L.mcr_last_error().decode()
    assert L.mcr_disparity_head_backward(p, p, p, p, p, p, p, i64(1), ci(1), ci(4), ci(4), p, sz(16), None) == 1        # short
    assert "workspace" in L.mcr_last_error().decode()
    assert L.mcr_disparity_head_backward(p, p, p, p, p, p, p, i64(1), ci(1), ci(4), ci(4), vp(4100), sz(1 << 20), None) == 1   # misaligned
    assert "aligned" in L.mcr_last_error().decode()


# ---- the switch --------------------------------------------------------------------------------------------------------------------------------
def test_backward_mode(monkeypatch):
    """The default is the composite: profiles/disparity_head_times.json does not show the HIP step faster with the intervals apart."""
    monkeypatch.delenv("MCR_DISPARITY_HEAD_BWD", raising=False)
    assert autograd.disparity_head_backward_mode() == "composite"
    monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", "HIP")
    assert autograd.disparity_head_backward_mode() == "hip"
    monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", "something")
    assert autograd.disparity_head_backward_mode() == "composite"


def test_exact_operands_have_headroom():
    """What the GPU's bit-equality tests rest on, checked where no GPU is needed: every sum of magnitudes stays below 2^24 units."""
    for tag in model.ALL_TAGS:
        room = model.exact_headroom(model.make_exact(tag))
        assert max(room) < 2 ** 24, (tag, room)
