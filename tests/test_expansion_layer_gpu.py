"""The fused expansion layer on the GPU (expansion_layer.hip: mcr_expansion_layer behind ops.expansion_layer and
networks.ManyDepth.ExpansionLayer / adopt_expansion_layer) against the independent fp64 model (tests/_expansion_layer_model.py) and the
reference's own layer (tests/golden/expansion_layer.npz).

Cases (B, Cin, Cmid, Cadd, Cout, h x w -> H x W), CASES of the model file: a (1,1,1,none,1, 2x2 -> 2x2) both mirrors inside a two-pixel
axis, no x_add, identity resize; b (2,3,2,3,5, 3x5 -> 7x9) batch stride, odd sizes, non-integer ratios; c (1,8,4,4,16, 8x15 -> 16x29)
upstream's expansion5 geometry; d (1,20,17,3,17, 9x17 -> 17x33); e (2,32,16,3,16, 16x29 -> 32x57) expansion1's channels; f
(1,512,256,256,256, 8x15 -> 16x29) expansion5 itself; g (1,6,4,2,4, 7x5 -> 3x4) an output smaller than the input; and, added to the
issue's seven, one case per tile of the kernel that is one more than the tile in every tiled dimension, in both launches:
  ROWS16 (4 x 32 pixels x 16 output channels, chunks of 16 input channels; every launch with at most 16 output channels: a, b, c's second,
    e, g):  h (1,17,16,1,16, 5x33 -> 9x65): 4+1 rows, 32+1 columns, then 2*4+1 and 2*32+1, 16+1 input channels in both launches;
  SPLIT (2 x 16 pixels x 16 output channels, chunks of 32 input channels divided among the four waves; more than 16 output channels on
    fewer than 256 workgroups of ROWS32: d, f):  i (1,33,17,16,17, 3x17 -> 5x33): 2+1 rows, 16+1 columns, 16+1 output channels, 32+1
    input channels in both launches (d: 4*2+1 rows, 16+1 columns and output channels);
  ROWS32 (4 x 32 pixels x 32 output channels, chunks of 16; from 256 workgroups on):  j (2,17,33,2,33, 33x225 -> 37x231): 288 and 320
    workgroups, 8*4+1 rows, 7*32+1 columns, 32+1 output channels, 16+1 and 2*16+3 input channels.

1. Exact operands, bit equality, no tolerance (make_exact of the model file: x and x_add small non-negative integers, both weights
+-m 2^-3, up_bias such that every z1 > 0 -- ELU is the identity and u exact --, i_bias such that z2 takes both signs).  The headroom (the
largest sum of magnitudes in units of the smallest term, below 2^24) and z1 > 0 are asserted in the model before the GPU is asked.  Where
the model's z2 > 0, y must equal it bit for bit; where z2 <= 0, y must equal expm1(z2) to 1e-6 relative.
2. Real-valued cases.  Against the model: the project's contract, rel < TOL = 1e-4 of the largest magnitude; against the golden (cases
a, b, c, d, e, g): TOL plus the golden's own stored distance.  Every distance is printed with an ERR prefix before it is asserted.
3. Poisoning: y filled with -7 and the arena with NaN bytes beforehand; y must come back finite without a -7.
4. Two calls give the same bits.  5. The C entry refuses bad sizes and workspaces without launching.  6. The module's routes.
7. The decoder's tail, five layers and four heads on HIP against the float64 composites.

Measured on an MI355X, worst of the cases: exact operands, 0 positive outputs differ, the negative branch 6.0e-08 from expm1; against the
model y 1.2e-06 (case f, K = 4608; elsewhere at most 5.7e-07); against the golden 6.3e-07 (case e; the golden itself is 3.6e-07 from the
model); the composite in fp32 on the device against the entry (case d) 3.2e-07; the decoder's tail against the fp64 composite chain
disp4 1.4e-07, disp3 1.2e-07, disp2 1.5e-07, disp1 1.4e-07.
"""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expansion_layer_model as model                                 # noqa: E402
from _reconstruction_model import rel                                 # noqa: E402

from macarons_amd import _lib, ops                                     # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
TAGS = list(model.ALL_TAGS)
KEYS = ("x", "x_add", "up_weight", "up_bias", "i_weight", "i_bias")


def t(x):
    return torch.as_tensor(np.asarray(x))


def on(c, dev):
    """The entry's arguments of a case, on the device."""
    return [None if c[k] is None else t(c[k]).to(dev) for k in KEYS] + [c["output_size"]]


@pytest.fixture(scope="module")
def inputs():
    return {tag: model.make_inputs(tag) for tag in TAGS}


@pytest.fixture(scope="module")
def modelled(inputs):
    """The fp64 model's y of every case, computed once and never changed."""
    return {tag: model.forward(*model.args_of(c))["y"] for tag, c in inputs.items()}


def poison_arena(dev, tag):
    """NaN bytes over the arena that ops.expansion_layer will hand to the entry for this case (the same cached tensor)."""
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes(tag)
    i64 = ctypes.c_int64
    ws = ops._entry_workspace(torch.device(dev), _lib.lib().mcr_expansion_layer_workspace_bytes, i64(B), i64(Cmid), i64(h), i64(w))
    ws.fill_(0xFF)
    return ws


# ---- 1. exact operands: bit equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_exact_operands(dev, tag):
    e = model.make_exact(tag)
    room = model.exact_headroom(e)
    want = model.forward(*model.args_of(e))
    assert max(room) < 2 ** 24, room
    assert want["z1"].min() > 0 and (want["z2"] > 0).any() and (want["z2"] < 0).any()
    z2 = want["z2"]
    assert np.array_equal(z2.astype(np.float32).astype(np.float64), z2)              # the model's z2 is an fp32 value
    poison_arena(dev, tag)
    y = ops.expansion_layer(*on(e, dev))
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes(tag)
    assert tuple(y.shape) == (B, Cout, H, W) and y.dtype == torch.float32 and y.is_contiguous()
    got = y.cpu().numpy()
    pos = z2 > 0
    wrong = int((got[pos] != z2[pos].astype(np.float32)).sum())
    print(f"ERR case {tag}, exact operands: headroom 2^{np.log2(room[0]):.1f} 2^{np.log2(room[1]):.1f}, {int(pos.sum())} positive outputs, {wrong} differ")
    assert wrong == 0
    neg = np.expm1(z2[~pos])
    err = float(np.max(np.abs(got[~pos].astype(np.float64) - neg) / np.maximum(np.abs(neg), 1e-300))) if neg.size else 0.0
    print(f"ERR case {tag}, exact operands: negative branch vs expm1, relative {err:.2e}")
    assert err < 1e-6 and np.array_equal(got[~pos][neg == 0.0], neg[neg == 0.0])


# ---- 2. real values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_real_values_match_the_model(dev, inputs, modelled, tag):
    y = ops.expansion_layer(*on(inputs[tag], dev))
    e = rel(y, t(modelled[tag]))
    print(f"ERR case {tag}, entry vs model: y {e:.2e}")
    assert e < TOL


@pytest.mark.parametrize("tag", model.GOLDEN_TAGS)
def test_real_values_match_the_golden(dev, tag):
    g = model.load_golden(tag)
    y = ops.expansion_layer(*on(g, dev))
    e = rel(y, t(g["y"]))
    print(f"ERR case {tag}, entry vs golden: y {e:.2e} (the golden's distance to the model {g['distance']:.2e})")
    assert g["distance"] < 1e-5 and e < TOL + g["distance"]


# ---- 3. poisoning --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_every_output_is_written_and_no_unwritten_u_is_read(dev, inputs, monkeypatch, tag):
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes(tag)
    ws = poison_arena(dev, tag)
    assert bool(torch.isnan(ws[:B * Cmid * h * w * 4].view(torch.float32)).all())
    poisoned, real_empty = [], torch.empty

    def empty(*size, **kw):                                             # the y that the entry is handed holds -7
        if kw.get("dtype") is not torch.float32:
            return real_empty(*size, **kw)
        out = torch.full(*size, -7.0, **kw)
        poisoned.append(out)
        return out

    monkeypatch.setattr(ops.torch, "empty", empty)
    y = ops.expansion_layer(*on(inputs[tag], dev))
    monkeypatch.undo()
    assert any(p is y for p in poisoned)
    assert bool(torch.isfinite(y).all()) and not bool((y == -7.0).any())


# ---- 4. the same bits on every call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_two_calls_give_the_same_bits(dev, inputs, tag):
    args = on(inputs[tag], dev)
    assert torch.equal(ops.expansion_layer(*args), ops.expansion_layer(*args))


# ---- 5. the C entry refuses before it launches -----------------------------------------------------------------------------------------------
def test_c_entry_refuses_without_launching(dev):
    L = _lib.lib()
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = 1, 3, 2, 3, 5, 3, 5, 7, 9
    x, x_add = torch.ones(B, Cin, h, w, device=dev), torch.ones(B, Cadd, H, W, device=dev)
    wu, bu = torch.ones(Cin, Cmid, 3, 3, device=dev), torch.zeros(Cmid, device=dev)
    wi, bi = torch.ones(Cout, Cmid + Cadd, 3, 3, device=dev), torch.zeros(Cout, device=dev)
    y = torch.full((B, Cout, H, W), -7.0, device=dev)
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    i64, ci, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

    def call(B=B, Cin=Cin, Cmid=Cmid, Cadd=Cadd, Cout=Cout, h=h, w=w, H=H, W=W, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), x_ptr=x.data_ptr(),
             add_ptr=x_add.data_ptr()):
        return L.mcr_expansion_layer(vp(x_ptr), vp(add_ptr), vp(wu.data_ptr()), vp(bu.data_ptr()), vp(wi.data_ptr()), vp(bi.data_ptr()),
                                     vp(y.data_ptr()), i64(B), ci(Cin), ci(Cmid), ci(Cadd), ci(Cout), ci(h), ci(w), ci(H), ci(W), vp(ws_ptr),
                                     sz(ws_bytes), None)

    sizes = [dict(H=1), dict(W=1), dict(h=0), dict(w=0), dict(Cin=0), dict(Cin=513), dict(Cmid=0), dict(Cmid=513, Cadd=0), dict(Cout=0),
             dict(Cout=513), dict(Cadd=-1), dict(Cmid=510, Cadd=3), dict(B=0), dict(B=-1), dict(B=2 ** 31), dict(B=2 ** 22, Cin=512, h=1, w=1),
             dict(B=2 ** 20, Cmid=512, Cadd=0, h=2, w=2), dict(B=2 ** 20, Cadd=400, H=2, W=3), dict(B=2 ** 20, Cout=512, H=2, W=2),
             dict(Cout=512, H=2 ** 11, W=2 ** 11)]
    for kw in sizes:
        assert call(**kw) == 1, kw
        assert L.mcr_last_error().decode().startswith("mcr_expansion_layer"), kw
    for kw in (dict(ws_bytes=64), dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=ws.numel() - 4), dict(ws_ptr=None)):
        assert call(**kw) == 1 and "workspace" in L.mcr_last_error().decode(), kw
    for kw in (dict(x_ptr=None), dict(add_ptr=None)):
        assert call(**kw) == 1 and "NULL" in L.mcr_last_error().decode(), kw
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((ws == 0xFF).all())       # nothing was launched
    assert call() == 0                                                  # and the same call, well-formed, runs
    torch.cuda.synchronize()
    ones = [np.ones(v.shape) for v in (x, x_add, wu)] + [np.zeros(Cmid), np.ones(wi.shape), np.zeros(Cout)]
    assert np.array_equal(y.cpu().numpy(), model.forward(*ones, (H, W))["y"])                     # small integers: exact
    y.fill_(-7.0)
    assert call(Cadd=0, add_ptr=None) == 0                              # no x_add: a NULL pointer with Cadd = 0 (i_weight is then read as [Cout,Cmid,3,3])
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), model.forward(ones[0], None, ones[2], ones[3], np.ones((Cout, Cmid, 3, 3)), ones[5], (H, W))["y"])


# ---- 6. the module: mirror and adopted upstream-like instance -----------------------------------------------------------------------------------
def _upstream_like(Cin, Cmid, Cout, size, Cadd):
    m = torch.nn.Module()
    m.upconv, m.upelu = torch.nn.ConvTranspose2d(Cin, Cmid, 3, stride=1, padding=1), torch.nn.ELU()
    m.iconv, m.ielu = torch.nn.Conv2d(Cmid + (Cadd or 0), Cout, 3, stride=1, padding=1, padding_mode="reflect"), torch.nn.ELU()
    m.input_channels, m.inner_channels, m.output_channels, m.output_size, m.additional_channels = Cin, Cmid, Cout, size, Cadd
    return m


def test_layer_routes(dev, inputs, monkeypatch):
    monkeypatch.setenv("MCR_EXPANSION_LAYER", "hip")
    c = inputs["d"]
    x, x_add, wu, bu, wi, bi, size = on(c, dev)
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes("d")
    state = {"upconv.weight": wu, "upconv.bias": bu, "iconv.weight": wi, "iconv.bias": bi}
    layer = ManyDepth.ExpansionLayer(Cin, Cmid, Cout, (H, W), additional_channels=Cadd).to(dev)
    adopted = ManyDepth.adopt_expansion_layer(_upstream_like(Cin, Cmid, Cout, (H, W), Cadd).to(dev))
    want = ops.expansion_layer(x, x_add, wu, bu, wi, bi, size)
    for m in (layer, adopted):
        m.load_state_dict(state)
        with torch.no_grad():
            assert torch.equal(m(x, x_add), want) and torch.equal(m(x=x, x_add=x_add), want)      # no gradient: the entry itself
        y = m(x, x_add)                                                 # parameters require grad: the composite under autograd
        assert y.grad_fn is not None and rel(y, want) < TOL
        y.sum().backward()
        assert m.upconv.weight.grad is not None and m.iconv.bias.grad is not None
        m.requires_grad_(False)
        assert torch.equal(m(x, x_add), want)                           # nothing requires grad: the entry, grad mode on or off
        xg = x.clone().requires_grad_(True)
        assert m(xg, x_add).grad_fn is not None
        with torch.no_grad():
            comp = ManyDepth.expansion_layer_composite(x, x_add, wu, bu, wi, bi, size)
            strided = x.transpose(2, 3).contiguous().transpose(2, 3)
            assert not strided.is_contiguous() and torch.equal(m(strided, x_add), comp)           # a strided x: the composite
            with torch.autocast("cuda", dtype=torch.float16):
                assert m(x, x_add).dtype == torch.float16              # autocast: the composite
            with pytest.raises(RuntimeError):
                m(x)                                                    # additional_channels without x_add: the composite, failing as upstream does
        monkeypatch.setenv("MCR_EXPANSION_LAYER", "composite")
        with torch.no_grad():
            assert torch.equal(m(x, x_add), comp)                       # forced
        monkeypatch.setenv("MCR_EXPANSION_LAYER", "hip")
    with torch.no_grad():
        assert layer.double()(x.double(), x_add.double()).dtype == torch.float64                   # another dtype: the composite
    print(f"ERR case d, composite (float32, device) vs entry: y {rel(comp, want):.2e}")
    assert rel(comp, want) < TOL


# ---- 7. the decoder's tail: five expansion layers, four heads between them --------------------------------------------------------------------
def _smooth_features(rng, C, Hs, Ws):
    v, u = np.meshgrid((np.arange(Hs) + 0.5) / Hs, (np.arange(Ws) + 0.5) / Ws, indexing="ij")
    out = np.empty((1, C, Hs, Ws), np.float32)
    for c in range(C):
        k, th, ph = rng.uniform(2.0, 6.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        out[0, c] = np.sin(k * (np.cos(th) * u + np.sin(th) * v) + ph) + 0.3 * (u - 0.5) * rng.choice([-1.0, 1.0])
    return out


def test_decoder_tail(dev, monkeypatch):
    """expansion5 .. expansion1 with disp4 .. disp1 between them at the sizes upstream's decoder derives from an H 32, W 57 input (the
    shapes of test_four_heads_feed_the_depth_losses), every layer and head routed to HIP, against the same chain in float64 on the
    composites."""
    monkeypatch.setenv("MCR_EXPANSION_LAYER", "hip")
    H, W = 32, 57
    rng = np.random.default_rng(91)
    torch.manual_seed(91)
    # (Cin, Cmid, Cadd, Cout, output size) of expansion5 .. 1, ManyDepth.py:428-471
    spec = [(512, 256, 256, 256, (H // 16, W // 16 + (W % 16 > 0))), (256, 128, 128, 128, (H // 8, W // 8 + (W % 8 > 0))),
            (128, 64, 64, 64, (H // 4, W // 4 + (W % 4 > 0))), (64, 32, 64, 32, (H // 2, W // 2 + (W % 2 > 0))), (32, 16, 3, 16, (H, W))]
    layers = [ManyDepth.ExpansionLayer(ci_, cm, co, size, additional_channels=ca) for ci_, cm, ca, co, size in spec]
    heads = [ManyDepth.DisparityLayer(co) for _, _, _, co, _ in spec[1:]]
    layer4 = t(_smooth_features(rng, 512, 1, 2))
    skips = [t(_smooth_features(rng, ca, *size)) for _, _, ca, _, size in spec]

    def chain(layers, heads, x, skips):
        disps = []
        for k, (layer, skip) in enumerate(zip(layers, skips)):
            x = layer(x, skip)
            if k:
                disps.append(heads[k - 1](x))
        return disps

    fused = []
    real = ops.expansion_layer
    monkeypatch.setattr(ops, "expansion_layer", lambda *a: fused.append(1) or real(*a))
    with torch.no_grad():
        got = chain([copy_to(m, dev) for m in layers], [copy_to(m, dev) for m in heads], layer4.to(dev), [s.to(dev) for s in skips])
        want = chain([m.double() for m in layers], [m.double() for m in heads], layer4.double(), [s.double() for s in skips])
    assert len(fused) == 5
    e = {f"disp{4 - k}": rel(g, w_) for k, (g, w_) in enumerate(zip(got, want))}
    print("ERR decoder tail on HIP vs the fp64 composite chain: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert [tuple(g.shape) for g in got] == [(1, 1, 4, 8), (1, 1, 8, 15), (1, 1, 16, 29), (1, 1, 32, 57)] and max(e.values()) < TOL


def copy_to(module, dev):
    return copy.deepcopy(module).to(dev)
