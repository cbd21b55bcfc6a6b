"""The expansion layer without a GPU: the fp64 model (tests/_expansion_layer_model.py) and the torch composite against each other and
against the reference's own ExpansionLayer (tests/golden/expansion_layer.npz), the model's nearest rule against F.interpolate, the mirror
class and the adoption seam of networks.ManyDepth, the argument checks of ops.expansion_layer, the C ABI's size function and refusals,
and the route of a forward for every reason that sends it to the composite.

Bounds.  Model against golden: the golden's stored distance (the reference's fp32 against this model, measured by the generator, at most
3.6e-7, asserted below 1e-5) plus the contract TOL = 1e-4 of the largest magnitude.  Composite (fp32, CPU) against golden: TOL -- both
are torch's fp32 convolutions; the composite in fp64 against the model: 1e-12.
"""
import copy
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expansion_layer_model as model                                 # noqa: E402

from macarons_amd import _lib, ops                                     # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

TOL = 1e-4
PARAMS = ("up_weight", "up_bias", "i_weight", "i_bias")


def t(x, dtype=None):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(dtype or torch.float32)


def targs(c, dtype=None):
    return [t(c[k], dtype) for k in ("x", "x_add") + PARAMS] + [c["output_size"]]


def stand_in(input_channels=3, inner_channels=2, output_channels=5, output_size=(7, 9), additional_channels=3, upconv=None, iconv=None,
             upelu=None, ielu=None):
    """A plain nn.Module with upstream's attributes (ManyDepth.py:308-344) -- an instance of a class this test module does not define,
    so that it pickles wherever the tests are imported from."""
    m = nn.Module()
    up = dict(in_channels=input_channels, out_channels=inner_channels, kernel_size=3, stride=1, padding=1)
    up.update(upconv or {})
    ic = dict(in_channels=inner_channels + (additional_channels or 0), out_channels=output_channels, kernel_size=3, stride=1, padding=1,
              padding_mode="reflect")
    ic.update(iconv or {})
    m.upconv, m.upelu, m.iconv, m.ielu = nn.ConvTranspose2d(**up), upelu or nn.ELU(), nn.Conv2d(**ic), ielu or nn.ELU()
    m.input_channels, m.output_channels, m.output_size = input_channels, output_channels, output_size
    m.inner_channels, m.additional_channels = inner_channels, additional_channels
    m.kernel_size, m.stride, m.padding = 3, 1, 1
    return m


def upstream_forward(m, x, x_add=None):
    res = F.interpolate(m.upelu(m.upconv(x)), size=m.output_size, mode="nearest")
    if x_add is not None and m.additional_channels is not None:
        res = torch.cat((res, x_add), dim=-3)
    return m.ielu(m.iconv(res))


def load_into(layer, g):
    layer.load_state_dict({"upconv.weight": t(g["up_weight"]), "upconv.bias": t(g["up_bias"]), "iconv.weight": t(g["i_weight"]),
                           "iconv.bias": t(g["i_bias"])}, strict=True)
    return layer


def mirror_of(tag):
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes(tag)
    return ManyDepth.ExpansionLayer(Cin, Cmid, Cout, (H, W), additional_channels=Cadd)


# ---- the model, the composite and the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", model.NEAREST_PAIRS)
def test_model_nearest_rule_is_torchs(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1).expand(1, 1, n_in, 2).contiguous()
    rows = F.interpolate(src, size=(n_out, 2), mode="nearest")[0, 0, :, 0].long().numpy()
    cols = F.interpolate(src.transpose(2, 3).contiguous(), size=(2, n_out), mode="nearest")[0, 0, 0].long().numpy()
    want = model.nearest_index(n_in, n_out)
    assert np.array_equal(rows, want) and np.array_equal(cols, want)


@pytest.mark.parametrize("tag", [k for k in model.ALL_TAGS if k not in "fj"])
def test_model_matches_composite_in_float64(tag):
    c = model.make_inputs(tag)
    y = ManyDepth.expansion_layer_composite(*targs(c, torch.float64))
    want = model.forward(*model.args_of(c))["y"]
    e = model.rel(y.numpy(), want)
    print(f"ERR case {tag}, composite (float64) vs model: y {e:.2e}")
    assert tuple(y.shape) == want.shape and y.dtype == torch.float64 and e < 1e-12


@pytest.mark.parametrize("tag", model.GOLDEN_TAGS)
def test_model_and_composite_match_golden(tag):
    g = model.load_golden(tag)
    inp = model.make_inputs(tag)
    assert all(np.array_equal(inp[k], g[k]) for k in ("x",) + PARAMS) and inp["output_size"] == g["output_size"]      # the stored inputs are the seeded ones
    assert (inp["x_add"] is None) == (g["x_add"] is None) and (g["x_add"] is None or np.array_equal(inp["x_add"], g["x_add"]))
    e_model = model.rel(model.forward(*model.args_of(g))["y"], g["y"])
    with torch.no_grad():
        e_comp = model.rel(ManyDepth.expansion_layer_composite(*targs(g)).numpy(), g["y"])
    print(f"ERR case {tag}, vs golden: model {e_model:.2e} composite (float32) {e_comp:.2e}, golden's own distance {g['distance']:.2e}")
    assert g["distance"] < 1e-5 and e_model <= g["distance"] + TOL and e_comp < TOL


def test_exact_operands_have_headroom_and_both_signs():
    for tag in "abdgi":
        e = model.make_exact(tag)
        r = model.forward(*model.args_of(e))
        assert max(model.exact_headroom(e)) < 2 ** 24 and r["z1"].min() > 0 and (r["z2"] > 0).any() and (r["z2"] < 0).any()
        assert np.array_equal(r["z2"].astype(np.float32).astype(np.float64), r["z2"])


# ---- the mirror class ------------------------------------------------------------------------------------------------------------------------
def test_mirror_loads_the_reference_state_dict():
    z = np.load(model.GOLDEN)
    names, shapes = [str(n) for n in z["state_dict_names"]], [tuple(int(v) for v in str(s).split(",")) for s in z["state_dict_shapes"]]
    assert names == ["iconv.bias", "iconv.weight", "upconv.bias", "upconv.weight"]
    assert shapes == [(5,), (5, 5, 3, 3), (2,), (3, 2, 3, 3)]                      # case b's layer
    sd = mirror_of("b").state_dict()
    assert sorted(sd) == names and [tuple(sd[k].shape) for k in names] == shapes
    for tag in model.GOLDEN_TAGS:
        g = model.load_golden(tag)
        B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes(tag)
        layer = load_into(mirror_of(tag), g)
        assert (layer.input_channels, layer.inner_channels, layer.output_channels, layer.output_size, layer.additional_channels) == \
            (Cin, Cmid, Cout, (H, W), Cadd) and (layer.kernel_size, layer.stride, layer.padding) == (3, 1, 1)
        assert isinstance(layer.upelu, nn.ELU) and isinstance(layer.ielu, nn.ELU)
        with torch.no_grad():
            y = layer(t(g["x"]), t(g["x_add"]))                             # on the CPU: the composite
        assert tuple(y.shape) == tuple(g["y"].shape) and model.rel(y.numpy(), g["y"]) < TOL


def test_mirror_on_the_cpu_is_the_composite():
    g = model.load_golden("b")
    layer = load_into(mirror_of("b"), g)
    x, x_add = t(g["x"]).requires_grad_(True), t(g["x_add"])
    y = layer(x, x_add)
    params = (layer.upconv.weight, layer.upconv.bias, layer.iconv.weight, layer.iconv.bias)
    assert torch.equal(y, ManyDepth.expansion_layer_composite(x, x_add, *params, (7, 9))) and y.requires_grad
    assert torch.equal(layer.upsample(x), F.interpolate(x, size=(7, 9), mode="nearest"))
    assert layer.double()(x.detach().double(), x_add.double()).dtype == torch.float64          # another dtype: the composite as well
    # like upstream, x_add counts only with additional_channels set
    plain = ManyDepth.ExpansionLayer(3, 2, 5, (7, 9))
    assert plain.iconv.in_channels == 2 and torch.equal(plain(x.detach(), x_add), plain(x.detach()))


# ---- adoption --------------------------------------------------------------------------------------------------------------------------------
def test_adopt_expansion_layer():
    torch.manual_seed(5)
    layer = stand_in()
    x, x_add = torch.randn(2, 3, 3, 5), torch.randn(2, 3, 7, 9)
    want = upstream_forward(layer, x, x_add)
    assert ManyDepth.adopt_expansion_layer(layer) is layer
    fwd = vars(layer)["forward"]
    assert ManyDepth.adopt_expansion_layer(layer) is layer and vars(layer)["forward"] is fwd          # idempotent
    got = layer(x, x_add=x_add)                                         # upstream's decoder passes both by keyword
    assert torch.equal(got, layer(x=x, x_add=x_add))
    assert torch.allclose(got, want, rtol=0, atol=1e-6)                 # upstream's op sequence (its convolution pads by itself)
    params = (layer.upconv.weight, layer.upconv.bias, layer.iconv.weight, layer.iconv.bias)
    assert torch.equal(got, ManyDepth.expansion_layer_composite(x, x_add, *params, (7, 9)))          # the CPU fallback, bit for bit
    for clone in (pickle.loads(pickle.dumps(layer)), copy.deepcopy(layer)):
        assert isinstance(vars(clone)["forward"], type(fwd)) and vars(clone)["forward"].layer is clone
        assert torch.equal(clone(x, x_add), got)
        with torch.no_grad():
            clone.iconv.bias += 1.0                                     # the clone's forward reads the clone's parameters
        assert not torch.equal(clone(x, x_add), got) and torch.equal(layer(x, x_add), got)
    got.sum().backward()
    assert layer.upconv.weight.grad is not None and layer.iconv.weight.grad is not None
    bare = ManyDepth.adopt_expansion_layer(stand_in(additional_channels=None))
    assert torch.equal(bare(x, x_add), bare(x)) and tuple(bare(x).shape) == (2, 5, 7, 9)


@pytest.mark.parametrize("wrong", [
    dict(upconv=dict(kernel_size=5, padding=2)), dict(upconv=dict(stride=2)), dict(upconv=dict(padding=0)), dict(upconv=dict(stride=2, output_padding=1)),
    dict(upconv=dict(dilation=2)), dict(upconv=dict(groups=2), input_channels=4), dict(upconv=dict(bias=False)),
    dict(iconv=dict(kernel_size=5, padding=2)), dict(iconv=dict(stride=2)), dict(iconv=dict(padding=2)), dict(iconv=dict(padding_mode="zeros")),
    dict(iconv=dict(dilation=2)), dict(iconv=dict(groups=5)), dict(iconv=dict(bias=False)),
    dict(upelu=nn.ELU(alpha=0.5)), dict(ielu=nn.ELU(alpha=2.0)), dict(output_size=7), dict(output_size=(7.0, 9.0)), dict(output_size=(7, 9, 1))])
def test_adopt_refuses_another_layer(wrong):
    with pytest.raises(TypeError, match="adopt_expansion_layer"):
        ManyDepth.adopt_expansion_layer(stand_in(**wrong))


def test_adopt_refuses_a_non_layer():
    for other in (nn.Linear(2, 2), nn.Conv2d(2, 2, 3), object()):
        with pytest.raises(TypeError, match="adopt_expansion_layer"):
            ManyDepth.adopt_expansion_layer(other)
    partial = stand_in()
    del partial.ielu
    with pytest.raises(TypeError, match="adopt_expansion_layer"):
        ManyDepth.adopt_expansion_layer(partial)


def head_stand_in(C):
    m = nn.Module()
    m.channels, m.conv, m.sigmoid = C, nn.Conv2d(C, 1, 3, padding=1, padding_mode="reflect"), nn.Sigmoid()
    return m


def decoder_stand_in(expansions):
    builder = nn.Module()
    builder.height, builder.width, builder.feature_height, builder.feature_width, builder.feature_channels = 8, 12, 4, 6, 2
    builder.n_alpha, builder.d_min, builder.d_max, builder.n_depth = 1, 0.5, 2.0, 3
    builder.depth_bins = torch.linspace(0.5, 2.0, 3)
    builder.conv_reduce = nn.Conv2d(5, 2, 3, padding=1)
    dec = nn.Module()
    dec.cost_volume_builder = builder
    dec.disp1, dec.disp2, dec.disp3, dec.disp4 = (head_stand_in(c) for c in (4, 4, 4, 4))
    for k in expansions:
        setattr(dec, f"expansion{k}", stand_in())
    return dec


def test_adopt_depth_decoder_with_expansion_layers():
    dec = decoder_stand_in((1, 2, 3, 4, 5))
    assert ManyDepth.adopt_depth_decoder(dec) is dec
    assert all(isinstance(vars(getattr(dec, f"expansion{k}"))["forward"], ManyDepth._AdoptedExpansionForward) for k in (1, 2, 3, 4, 5))
    assert all(isinstance(vars(getattr(dec, f"disp{k}"))["forward"], ManyDepth._AdoptedHeadForward) for k in (1, 2, 3, 4))
    copy.deepcopy(dec), pickle.loads(pickle.dumps(dec))
    none = decoder_stand_in(())
    assert ManyDepth.adopt_depth_decoder(none) is none and isinstance(vars(none.disp1)["forward"], ManyDepth._AdoptedHeadForward)
    for some in ((5,), (1, 2, 3, 4), (2, 4)):
        dec = decoder_stand_in(some)
        with pytest.raises(TypeError, match="adopt_depth_decoder"):
            ManyDepth.adopt_depth_decoder(dec)
        assert "forward" not in vars(dec.disp1) and "forward" not in vars(dec.cost_volume_builder)     # refused before anything is rebound
    bad = decoder_stand_in((1, 2, 3, 4))
    bad.expansion5 = stand_in(iconv=dict(padding_mode="zeros"))
    with pytest.raises(TypeError, match="adopt_expansion_layer"):
        ManyDepth.adopt_depth_decoder(bad)


# ---- ops: the argument checks ------------------------------------------------------------------------------------------------------------------
def test_ops_argument_checks(monkeypatch):
    def no_library():
        raise AssertionError("an argument check let a call through to the library")

    good = dict(x=torch.zeros(2, 3, 3, 5), x_add=torch.zeros(2, 3, 7, 9), wu=torch.zeros(3, 2, 3, 3), bu=torch.zeros(2),
                wi=torch.zeros(5, 5, 3, 3), bi=torch.zeros(5), size=(7, 9))
    call = lambda a: ops.expansion_layer(a["x"], a["x_add"], a["wu"], a["bu"], a["wi"], a["bi"], a["size"])     # noqa: E731
    monkeypatch.setattr(ops, "lib", no_library)
    for bad in (dict(x=torch.zeros(3, 3, 5)), dict(x=torch.zeros(0, 3, 3, 5)), dict(x=torch.zeros(2, 3, 0, 5)), dict(x=torch.zeros(2, 4, 3, 5)),
                dict(size=(1, 9)), dict(size=(7, 1)), dict(size=7), dict(size=(7, 9, 2)),
                dict(x_add=torch.zeros(2, 3, 7, 8)), dict(x_add=torch.zeros(1, 3, 7, 9)), dict(x_add=torch.zeros(2, 0, 7, 9)), dict(x_add=None),
                dict(x_add=torch.zeros(2, 4, 7, 9)), dict(wu=torch.zeros(3, 2, 3)), dict(wu=torch.zeros(3, 2, 5, 5)), dict(wu=torch.zeros(3, 4, 3, 3)),
                dict(bu=torch.zeros(3)), dict(bi=torch.zeros(5, 1)), dict(wi=torch.zeros(5, 5, 1, 1)),
                dict(x=torch.zeros(1, 513, 1, 1), wu=torch.zeros(513, 2, 3, 3), x_add=torch.zeros(1, 3, 7, 9)),
                dict(wu=torch.zeros(3, 513, 3, 3), bu=torch.zeros(513), wi=torch.zeros(5, 513, 3, 3), x_add=None),
                dict(wu=torch.zeros(3, 510, 3, 3), bu=torch.zeros(510), wi=torch.zeros(5, 513, 3, 3)),
                dict(wi=torch.zeros(513, 5, 3, 3), bi=torch.zeros(513))):
        args = dict(good)
        args.update(bad)
        with pytest.raises(ValueError):
            call(args)
    big = torch.zeros(1).expand(2 ** 20, 512, 2, 2)                      # 2^31 elements, no memory behind them
    with pytest.raises(ValueError, match="2\\^31"):
        ops.expansion_layer(big, None, good["wu"].new_zeros(512, 1, 3, 3), torch.zeros(1), torch.zeros(1, 1, 3, 3), torch.zeros(1), (2, 2))
    monkeypatch.undo()
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):      # well-formed CPU tensors: no fall-back to torch
        call(good)


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------------------------
def test_symbols_and_workspace_arithmetic():
    names, L = _lib.declared_symbols(), _lib.lib()
    for n in ("mcr_expansion_layer", "mcr_expansion_layer_workspace_bytes"):
        assert n in names and hasattr(L, n), n
    size, i64 = L.mcr_expansion_layer_workspace_bytes, ctypes.c_int64
    assert size.restype is ctypes.c_size_t
    assert size(i64(1), i64(256), i64(8), i64(15)) == 256 * 120 * 4                   # u [B,Cmid,h,w], already a multiple of 256 bytes
    assert size(i64(2), i64(3), i64(3), i64(5)) == 512                                # 360 bytes, rounded to the arena's 256
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 513, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (2 ** 22, 512, 1, 1)):
        assert size(*(i64(v) for v in bad)) == 0, bad


def test_entry_refuses_without_a_device():
    """Every refusal precedes the first launch, so it can be asked for where there is no GPU; the pointers are never followed."""
    L, i64, ci, vp, sz = _lib.lib(), ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    p = vp(4096)

    def call(B=1, Cin=3, Cmid=2, Cadd=3, Cout=5, h=3, w=5, H=7, W=9, x=p, x_add=p, ws=p, ws_bytes=1 << 40):
        return L.mcr_expansion_layer(x, x_add, p, p, p, p, p, i64(B), ci(Cin), ci(Cmid), ci(Cadd), ci(Cout), ci(h), ci(w), ci(H), ci(W), ws,
                                     sz(ws_bytes), None)

    for bad in (dict(H=1), dict(W=1), dict(h=0), dict(w=0), dict(Cin=0), dict(Cin=513), dict(Cmid=0), dict(Cmid=513, Cadd=0), dict(Cout=0),
                dict(Cout=513), dict(Cadd=-1), dict(Cmid=257, Cadd=256), dict(B=0), dict(B=-1), dict(B=2 ** 22, Cin=512, h=1, w=1),
                dict(B=2 ** 20, Cout=512, H=2, W=2), dict(B=2 ** 20, Cadd=400, H=2, W=3), dict(B=2 ** 20, Cmid=512, Cadd=0, h=2, w=2),
                dict(x=None), dict(x_add=None), dict(ws=None), dict(ws_bytes=16), dict(ws=vp(4100))):
        assert call(**bad) == 1, bad
        msg = L.mcr_last_error().decode()
        assert msg.startswith("mcr_expansion_layer") and "kernel" not in msg, (bad, msg)


# ---- the route ---------------------------------------------------------------------------------------------------------------------------------
def test_mode_switch(monkeypatch):
    monkeypatch.delenv("MCR_EXPANSION_LAYER", raising=False)
    assert ManyDepth.expansion_layer_mode() == ManyDepth.EXPANSION_LAYER_DEFAULT and ManyDepth.EXPANSION_LAYER_DEFAULT in ("hip", "composite")
    for value, want in (("hip", "hip"), ("composite", "composite"), (" HIP ", "hip"), ("other", ManyDepth.EXPANSION_LAYER_DEFAULT)):
        monkeypatch.setenv("MCR_EXPANSION_LAYER", value)
        assert ManyDepth.expansion_layer_mode() == want


def test_route_for_every_fallback_reason(monkeypatch):
    """CPU tensors stand for HIP tensors (the device predicate is replaced) and ops.expansion_layer for the entry (a recorder), so the
    decision itself is what is tested: every reason of the route for the composite, one at a time, around a call that goes to HIP."""
    calls = []

    def entry(*args):
        calls.append(args)
        return "fused"

    monkeypatch.setattr(ops, "expansion_layer", entry)
    monkeypatch.setenv("MCR_EXPANSION_LAYER", "hip")
    layer = load_into(mirror_of("b"), model.load_golden("b")).requires_grad_(False)
    adopted = ManyDepth.adopt_expansion_layer(stand_in().requires_grad_(False))
    x, x_add = torch.randn(2, 3, 3, 5), torch.randn(2, 3, 7, 9)

    def fused(m, *a, **k):
        n = len(calls)
        out = m(*a, **k)
        return len(calls) == n + 1 and out == "fused"

    assert not fused(layer, x, x_add)                                   # CPU tensors
    monkeypatch.setattr(ManyDepth, "_is_hip_tensor", lambda v: True)
    for m in (layer, adopted):
        assert fused(m, x, x_add) and fused(m, x=x, x_add=x_add)
        got = calls[-1]
        assert got[0] is x and got[1] is x_add and got[2] is m.upconv.weight and got[3] is m.upconv.bias and got[4] is m.iconv.weight \
            and got[5] is m.iconv.bias and tuple(got[6]) == (7, 9)
        with torch.no_grad():
            assert fused(m, x.clone().requires_grad_(True), x_add)      # grad mode off: nothing is recorded
        assert not fused(m, x.clone().requires_grad_(True), x_add)      # an input requires grad
        assert not fused(m, x, x_add.clone().requires_grad_(True))
        for prm in (m.upconv.weight, m.upconv.bias, m.iconv.weight, m.iconv.bias):
            prm.requires_grad_(True)
            assert not fused(m, x, x_add) and m(x, x_add).grad_fn is not None      # a parameter requires grad: autograd through the composite
            prm.requires_grad_(False)
    layer64 = copy.deepcopy(layer).double()
    assert not fused(layer64, x.double(), x_add.double()) and layer64(x.double(), x_add.double()).dtype == torch.float64
    assert not fused(layer, x.transpose(2, 3).contiguous().transpose(2, 3), x_add)                   # a strided x
    assert not fused(layer, x, x_add.transpose(2, 3).contiguous().transpose(2, 3))                   # a strided x_add
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not fused(layer, x, x_add)                               # autocast
    n = len(calls)
    with pytest.raises(RuntimeError):
        layer(x, None)                                                  # additional_channels without x_add: the composite, which fails as upstream does
    assert len(calls) == n
    params = (layer.upconv.weight, layer.upconv.bias, layer.iconv.weight, layer.iconv.bias)
    assert ManyDepth.expansion_layer_route(x, x_add, params, (7, 9), 3) == "hip"
    assert ManyDepth.expansion_layer_route(x, None, params, (7, 9), 3) == "composite"
    assert ManyDepth.expansion_layer_route(x, x_add, params, (1, 9), 3) == "composite"                # outside the entry's limits: H = 1
    wide = (torch.zeros(3, 513, 3, 3), torch.zeros(513), torch.zeros(5, 513, 3, 3), torch.zeros(5))
    assert ManyDepth.expansion_layer_route(x, None, wide, (7, 9), None) == "composite"               # 513 channels
    monkeypatch.setenv("MCR_EXPANSION_LAYER", "composite")
    assert not fused(layer, x, x_add)                                   # forced
    monkeypatch.delenv("MCR_EXPANSION_LAYER")
    assert fused(layer, x, x_add) == (ManyDepth.EXPANSION_LAYER_DEFAULT == "hip")
    plain = ManyDepth.ExpansionLayer(3, 2, 5, (7, 9)).requires_grad_(False)
    monkeypatch.setenv("MCR_EXPANSION_LAYER", "hip")
    assert fused(plain, x, x_add) and calls[-1][1] is None              # an x_add the layer ignores is not handed on
