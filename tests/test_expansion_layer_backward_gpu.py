"""The backward of the fused expansion layer on the GPU (expansion_layer_bwd.hip: mcr_expansion_layer_backward behind
ops.expansion_layer_backward, autograd.ExpansionLayerFunction and the module's 'function' route) against the independent fp64 model
(tests/_expansion_layer_backward_model.py, whose docstring lists the cases and which tile of which kernel each one serves) and the
reference's own layer under autograd (tests/golden/expansion_layer_backward.npz).  Every case goes through
ops.expansion_layer(..., return_u=True) and then ops.expansion_layer_backward.

1. Exact operands (make_exact_backward: small integers, weights +-m 2^-3, both biases lifting the pre-activations above zero, d_y small
thinned integers): all six gradients bit-equal to the model, np.array_equal on float32; the headroom (below 2^24) is asserted first.
2. Real values: each gradient within the project's contract, rel < 1e-4 of its largest magnitude, of the model; against the golden 1e-4 plus
the golden's stored distance; the fp32 composite's autograd on the device against the model is printed for comparison.
3. u of the forward against the model's (bit-equal in the exact cases); y with return_u bit-equal to y without.
4. Poisoning: outputs filled with -7, the arena with NaN bytes.  5. need: every single output, the data pair, each weight pair.
6. Two calls give the same bits.  7. The C entry refuses without launching.  8. The module under MCR_EXPANSION_LAYER_BWD.
9. The decoder's tail, five layers and four heads, forward and backward.
Every distance is printed with an ERR prefix before it is asserted.

Measured on an MI355X, worst of the thirteen cases.  Exact operands: 0 elements of any gradient differ (headroom at most 2^20.5).  Against
the model: d_x 1.2e-06 (n), d_x_add 1.8e-06 (n), d_up_weight 6.8e-07 (m), d_up_bias 1.7e-06 (n), d_i_weight 7.0e-07 (m), d_i_bias 3.5e-07 (m);
the fp32 composite's autograd on the device against the model: d_x 6.0e-07, d_x_add 5.2e-07, d_up_weight 5.4e-07, d_up_bias 6.9e-07,
d_i_weight 8.6e-07 (f), d_i_bias 2.6e-07.  Against the golden: at most 9.4e-07 (d_up_bias, case e; the golden itself is 8.7e-07 from the
model there).  u of the forward against the model: at most 1.0e-06 (f).  The module, case d, against the float64 composite: at most 2.9e-07
(d_i_weight).  The decoder's tail against the fp64 composite chain: parameters (worst of 28) 1.1e-06, layer4 features 6.5e-07, skips 5.8e-07,
4.5e-07, 2.7e-07, 2.7e-07, 1.6e-07.
"""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expansion_layer_backward_model as bmodel                      # noqa: E402
from _reconstruction_model import rel                                 # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
TAGS = list(bmodel.ALL_TAGS)
NAMES = bmodel.NAMES
KEYS = ("x", "x_add", "up_weight", "up_bias", "i_weight", "i_bias")


def t(x):
    return torch.as_tensor(np.asarray(x))


def on(c, dev):
    """The forward entry's arguments of a case, on the device."""
    return [None if c[k] is None else t(c[k]).to(dev) for k in KEYS] + [c["output_size"]]


def run(c, d_y, dev, need=(True,) * 6):
    """-> (the six gradients, u, y) of a case on the device."""
    a = on(c, dev)
    y, u = ops.expansion_layer(*a, return_u=True)
    x, x_add, wu, _, wi, _, size = a
    return ops.expansion_layer_backward(x, x_add, wu, wi, u, y, t(d_y).to(dev), size, need=need), u, y


@pytest.fixture(scope="module")
def inputs():
    return {tag: (bmodel.make_inputs(tag), bmodel.make_d_y(tag)) for tag in TAGS}


@pytest.fixture(scope="module")
def modelled(inputs):
    """The fp64 model's gradients of every case, computed once and never changed."""
    return {tag: bmodel.backward(*bmodel.args_of(c), d_y) for tag, (c, d_y) in inputs.items()}


@pytest.fixture(scope="module")
def exact():
    """tag -> (operands, d_y, the model's result, the headroom), each computed once."""
    cache = {}

    def get(tag):
        if tag not in cache:
            e, d_y = bmodel.make_exact_backward(tag)
            cache[tag] = (e, d_y, bmodel.backward(*bmodel.args_of(e), d_y), bmodel.exact_headroom_backward(e, d_y))
        return cache[tag]

    return get


def poison_arena(dev, tag):
    """NaN bytes over the arena that ops.expansion_layer_backward will hand to the entry for this case (the same cached tensor)."""
    i64 = ctypes.c_int64
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = bmodel.sizes(tag)
    ws = ops._entry_workspace(torch.device(dev), _lib.lib().mcr_expansion_layer_backward_workspace_bytes,
                              *(i64(v) for v in (B, Cin, Cmid, Cadd or 0, Cout, h, w, H, W)))
    ws.fill_(0xFF)
    return ws


def distances(got, want):
    return {k: rel(g, t(want[k])) for k, g in zip(NAMES, got) if g is not None}


def show(d):
    return " ".join(f"{k} {v:.2e}" for k, v in d.items())


# ---- 1. exact operands: bit equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_exact_operands(dev, exact, tag):
    e, d_y, want, room = exact(tag)
    assert max(room.values()) < 2 ** 24, room
    assert want["z1"].min() > 0 and want["z2"].min() > 0 and (d_y != 0).any()
    poison_arena(dev, tag)
    got, u, y = run(e, d_y, dev)
    assert np.array_equal(u.cpu().numpy(), want["u"].astype(np.float32)) and np.array_equal(y.cpu().numpy(), want["y"].astype(np.float32))
    wrong = {}
    for k, g in zip(NAMES, got):
        if want[k] is None:
            assert g is None
            continue
        assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == want[k].shape, k
        assert np.array_equal(want[k].astype(np.float32).astype(np.float64), want[k]), k           # the model's value is an fp32 value
        wrong[k] = int((g.cpu().numpy() != want[k].astype(np.float32)).sum())
    print(f"ERR case {tag}, exact operands: headroom 2^{np.log2(max(room.values())):.1f}, elements that differ: "
          + " ".join(f"{k} {v}" for k, v in wrong.items()))
    assert not any(wrong.values())


# ---- 2. real values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_real_values_match_the_model(dev, inputs, modelled, tag):
    c, d_y = inputs[tag]
    got, _, _ = run(c, d_y, dev)
    e = distances(got, modelled[tag])
    print(f"ERR case {tag}, entry vs model: {show(e)}")
    leaves = [None if v is None else v.requires_grad_(True) for v in on(c, dev)[:6]]
    comp = ManyDepth.expansion_layer_composite(*leaves, c["output_size"])
    grads = iter(torch.autograd.grad(comp, [v for v in leaves if v is not None], t(d_y).to(dev)))
    ce = distances([None if v is None else next(grads) for v in leaves], modelled[tag])
    print(f"ERR case {tag}, composite (float32, device, autograd) vs model: {show(ce)}")
    assert len(e) == (6 if c["x_add"] is not None else 5) and max(e.values()) < TOL


@pytest.mark.parametrize("tag", bmodel.GOLDEN_TAGS)
def test_real_values_match_the_golden(dev, inputs, tag):
    c, d_y = inputs[tag]
    g = bmodel.load_golden_backward(tag)
    assert np.array_equal(g["d_y"], d_y)
    got, _, _ = run(c, d_y, dev)
    e = distances(got, g)
    print(f"ERR case {tag}, entry vs golden: {show(e)} (the golden's distances to the model: {show(g['distance'])})")
    for k, v in e.items():
        assert g["distance"][k] < 1e-5 and v < TOL + g["distance"][k], k


# ---- 3. u and y of the forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_u_returned_by_the_forward(dev, inputs, modelled, tag):
    c, _ = inputs[tag]
    a = on(c, dev)
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = bmodel.sizes(tag)
    y, u = ops.expansion_layer(*a, return_u=True)
    assert tuple(u.shape) == (B, Cmid, h, w) and u.dtype == torch.float32 and u.is_contiguous()
    e = rel(u, t(modelled[tag]["u"]))
    print(f"ERR case {tag}, u of the forward vs model: {e:.2e}")
    assert e < TOL
    other = ops.expansion_layer(*on(bmodel.make_inputs("b"), dev))     # another call on the shared arena does not touch the returned u
    assert other is not None and rel(u, t(modelled[tag]["u"])) == e
    assert torch.equal(y, ops.expansion_layer(*a))


# ---- 4. poisoning --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_every_output_is_written(dev, inputs, modelled, monkeypatch, tag):
    c, d_y = inputs[tag]
    ws = poison_arena(dev, tag)
    assert bool(torch.isnan(ws[:1024].view(torch.float32)).all())
    poisoned, real_empty = [], torch.empty

    def empty(*size, **kw):                                             # every gradient that the entry is handed holds -7
        if kw.get("dtype") is not torch.float32:
            return real_empty(*size, **kw)
        out = torch.full(*size, -7.0, **kw)
        poisoned.append(out)
        return out

    monkeypatch.setattr(ops.torch, "empty", empty)
    got, _, _ = run(c, d_y, dev)
    monkeypatch.undo()
    for k, g in zip(NAMES, got):
        if g is None:
            assert k == "d_x_add" and c["x_add"] is None
            continue
        assert any(p is g for p in poisoned), k
        assert bool(torch.isfinite(g).all()) and not bool((g == -7.0).any()), k
    # what no pixel reads of u (case g: most of it) reaches d_x as zeros of d_u, not as what the arena held
    assert max(distances(got, modelled[tag]).values()) < TOL


# ---- 5. need ---------------------------------------------------------------------------------------------------------------------------------
SUBSETS = [tuple(i == k for i in range(6)) for k in range(6)] + [(True, True, False, False, False, False),
                                                                 (False, False, True, True, False, False), (False, False, False, False, True, True)]


@pytest.mark.parametrize("tag", ["a", "b", "i"])
def test_need_computes_what_is_asked_and_nothing_else(dev, inputs, tag):
    c, d_y = inputs[tag]
    full, _, _ = run(c, d_y, dev)
    for need in SUBSETS:
        if c["x_add"] is None and not any(n for k, n in enumerate(need) if k != 1):
            with pytest.raises(ValueError):
                run(c, d_y, dev, need=need)                             # d_x_add alone without an x_add: nothing to compute
            continue
        poison_arena(dev, tag)
        got, _, _ = run(c, d_y, dev, need=need)
        for k, n, g, f in zip(NAMES, need, got, full):
            if n and f is not None:
                assert torch.equal(g, f), (need, k)
            else:
                assert g is None, (need, k)


def test_null_outputs_are_untouched_through_the_c_entry(dev, inputs):
    c, d_y = inputs["b"]
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = bmodel.sizes("b")
    a = on(c, dev)
    y, u = ops.expansion_layer(*a, return_u=True)
    x, x_add, wu, _, wi, _, _ = a
    g = t(d_y).to(dev)
    full = ops.expansion_layer_backward(x, x_add, wu, wi, u, y, g, (H, W))
    L, i64, ci, vp, sz = _lib.lib(), ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    ws = poison_arena(dev, "b")
    for need in SUBSETS:
        outs = [torch.full_like(f, -7.0) for f in full]
        rc = L.mcr_expansion_layer_backward(*(vp(v.data_ptr()) for v in (x, x_add, wu, wi, u, y, g)),
                                            *(vp(o.data_ptr()) if n else None for o, n in zip(outs, need)), i64(B), ci(Cin), ci(Cmid),
                                            ci(Cadd), ci(Cout), ci(h), ci(w), ci(H), ci(W), vp(ws.data_ptr()), sz(ws.numel()), None)
        assert rc == 0, L.mcr_last_error().decode()
        torch.cuda.synchronize()
        for k, n, o, f in zip(NAMES, need, outs, full):
            assert torch.equal(o, f) if n else bool((o == -7.0).all()), (need, k)


# ---- 6. the same bits on every call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_two_calls_give_the_same_bits(dev, inputs, tag):
    c, d_y = inputs[tag]
    first, _, _ = run(c, d_y, dev)
    poison_arena(dev, tag)
    second, _, _ = run(c, d_y, dev)
    for k, p, q in zip(NAMES, first, second):
        assert (p is None and q is None) or torch.equal(p, q), k


# ---- 7. the C entry refuses before it launches -----------------------------------------------------------------------------------------------
def test_c_entry_refuses_without_launching(dev):
    L = _lib.lib()
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = 1, 3, 2, 3, 5, 3, 5, 7, 9
    ones = lambda *s: torch.ones(*s, device=dev)                       # noqa: E731
    x, x_add, wu, wi, u, y, d_y = ones(B, Cin, h, w), ones(B, Cadd, H, W), ones(Cin, Cmid, 3, 3), ones(Cout, Cmid + Cadd, 3, 3), \
        ones(B, Cmid, h, w), ones(B, Cout, H, W), ones(B, Cout, H, W)
    outs = [torch.full(s, -7.0, device=dev) for s in ((B, Cin, h, w), (B, Cadd, H, W), (Cin, Cmid, 3, 3), (Cmid,), (Cout, Cmid + Cadd, 3, 3), (Cout,))]
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    i64, ci, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

    def call(B=B, Cin=Cin, Cmid=Cmid, Cadd=Cadd, Cout=Cout, h=h, w=w, H=H, W=W, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), x_ptr=x.data_ptr(),
             add_ptr=x_add.data_ptr(), u_ptr=u.data_ptr(), need=(True,) * 6):
        return L.mcr_expansion_layer_backward(vp(x_ptr), vp(add_ptr), vp(wu.data_ptr()), vp(wi.data_ptr()), vp(u_ptr), vp(y.data_ptr()),
                                              vp(d_y.data_ptr()), *(vp(o.data_ptr()) if n else None for o, n in zip(outs, need)), i64(B),
                                              ci(Cin), ci(Cmid), ci(Cadd), ci(Cout), ci(h), ci(w), ci(H), ci(W), vp(ws_ptr), sz(ws_bytes), None)

    sizes = [dict(H=1), dict(W=1), dict(h=0), dict(w=0), dict(Cin=0), dict(Cin=513), dict(Cmid=0), dict(Cmid=513, Cadd=0), dict(Cout=0),
             dict(Cout=513), dict(Cadd=-1), dict(Cmid=510, Cadd=3), dict(B=0), dict(B=-1), dict(B=2 ** 31), dict(B=2 ** 22, Cin=512, h=1, w=1),
             dict(B=2 ** 20, Cmid=512, Cadd=0, h=2, w=2), dict(B=2 ** 20, Cadd=400, H=2, W=3), dict(B=2 ** 20, Cout=512, H=2, W=2),
             dict(Cout=512, H=2 ** 11, W=2 ** 11), dict(B=2 ** 18, Cmid=256, Cadd=256, Cout=1, H=2, W=2)]       # the last: only G, with its ring, is too large
    for kw in sizes:
        assert call(**kw) == 1, kw
        assert L.mcr_last_error().decode().startswith("mcr_expansion_layer_backward"), kw
    for kw in (dict(ws_bytes=64), dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=ws.numel() - 4), dict(ws_ptr=None)):
        assert call(**kw) == 1 and "workspace" in L.mcr_last_error().decode(), kw
    for kw in (dict(x_ptr=None), dict(add_ptr=None), dict(u_ptr=None)):
        assert call(**kw) == 1 and "NULL" in L.mcr_last_error().decode(), kw
    assert call(need=(False,) * 6) == 1 and "all six" in L.mcr_last_error().decode()
    assert call(Cadd=0, add_ptr=None) == 1 and "d_x_add" in L.mcr_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((ws == 0xFF).all())       # nothing was launched
    assert call() == 0                                                  # and the same call, well-formed, runs
    torch.cuda.synchronize()
    # u, y and d_y are ones, so both derivatives are 1 and every tap reads a one at every pixel
    assert np.array_equal(outs[5].cpu().numpy(), np.full(Cout, float(B * H * W)))
    assert np.array_equal(outs[4].cpu().numpy(), np.full(wi.shape, float(B * H * W)))
    assert all(bool(torch.isfinite(o).all()) and not bool((o == -7.0).any()) for o in outs)


# ---- 8. the module: mirror and adopted upstream-like instance -----------------------------------------------------------------------------------
def _upstream_like(Cin, Cmid, Cout, size, Cadd):
    m = torch.nn.Module()
    m.upconv, m.upelu = torch.nn.ConvTranspose2d(Cin, Cmid, 3, stride=1, padding=1), torch.nn.ELU()
    m.iconv, m.ielu = torch.nn.Conv2d(Cmid + (Cadd or 0), Cout, 3, stride=1, padding=1, padding_mode="reflect"), torch.nn.ELU()
    m.input_channels, m.inner_channels, m.output_channels, m.output_size, m.additional_channels = Cin, Cmid, Cout, size, Cadd
    return m


def test_layer_under_the_backward_knob(dev, inputs, monkeypatch):
    c, d_y = inputs["d"]
    x, x_add, wu, bu, wi, bi, size = on(c, dev)
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = bmodel.sizes("d")
    state = {"upconv.weight": wu, "upconv.bias": bu, "iconv.weight": wi, "iconv.bias": bi}
    g = t(d_y).to(dev)
    # the float64 composite's gradients, on the CPU
    leaves = [t(c[k]).double().requires_grad_(True) for k in KEYS]
    want = torch.autograd.grad(ManyDepth.expansion_layer_composite(*leaves, size), leaves, t(d_y).double())
    y_entry = ops.expansion_layer(x, x_add, wu, bu, wi, bi, size)
    layer = ManyDepth.ExpansionLayer(Cin, Cmid, Cout, (H, W), additional_channels=Cadd).to(dev)
    adopted = ManyDepth.adopt_expansion_layer(_upstream_like(Cin, Cmid, Cout, (H, W), Cadd).to(dev))
    calls = []
    real = ops.expansion_layer_backward
    monkeypatch.setattr(ops, "expansion_layer_backward", lambda *a, **k: calls.append(k.get("need")) or real(*a, **k))
    for name, m in (("mirror", layer), ("adopted", adopted)):
        m.load_state_dict(state)
        monkeypatch.setenv("MCR_EXPANSION_LAYER_BWD", "hip")
        assert autograd.expansion_layer_backward_mode() == "hip"
        xg, ag = x.clone().requires_grad_(True), x_add.clone().requires_grad_(True)
        y = m(xg, ag)
        assert type(y.grad_fn).__name__.startswith("ExpansionLayerFunction") and torch.equal(y, y_entry)
        n = len(calls)
        y.backward(g)
        assert len(calls) == n + 1 and calls[-1] == (True,) * 6
        got = (xg.grad, ag.grad, m.upconv.weight.grad, m.upconv.bias.grad, m.iconv.weight.grad, m.iconv.bias.grad)
        e = {k: rel(a, b) for k, a, b in zip(NAMES, got, want)}
        print(f"ERR case d, {name} layer under MCR_EXPANSION_LAYER_BWD=hip vs the float64 composite: {show(e)}")
        assert max(e.values()) < TOL
        # only x requires a gradient: the parameter gradients stay None; a strided d_y is served
        m.zero_grad(set_to_none=True)
        m.requires_grad_(False)
        xg = x.clone().requires_grad_(True)
        y = m(xg, x_add)
        assert type(y.grad_fn).__name__.startswith("ExpansionLayerFunction")
        strided = g.transpose(2, 3).contiguous().transpose(2, 3)
        assert not strided.is_contiguous()
        y.backward(strided)
        assert calls[-1] == (True, False, False, False, False, False)
        assert all(p.grad is None for p in m.parameters()) and rel(xg.grad, want[0]) < TOL
        m.requires_grad_(True)
        # the variable unset: the same calls run the composite under autograd
        monkeypatch.delenv("MCR_EXPANSION_LAYER_BWD")
        n = len(calls)
        xg = x.clone().requires_grad_(True)
        y = m(xg, x_add)
        assert y.grad_fn is not None and not type(y.grad_fn).__name__.startswith("ExpansionLayerFunction")
        y.backward(g)
        assert len(calls) == n and rel(xg.grad, want[0]) < TOL and rel(m.iconv.weight.grad, want[4]) < TOL
        m.zero_grad(set_to_none=True)


# ---- 9. the decoder's tail: five expansion layers, four heads, forward and backward ------------------------------------------------------------
def _smooth_features(rng, C, Hs, Ws):
    v, u = np.meshgrid((np.arange(Hs) + 0.5) / Hs, (np.arange(Ws) + 0.5) / Ws, indexing="ij")
    out = np.empty((1, C, Hs, Ws), np.float32)
    for c in range(C):
        k, th, ph = rng.uniform(2.0, 6.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        out[0, c] = np.sin(k * (np.cos(th) * u + np.sin(th) * v) + ph) + 0.3 * (u - 0.5) * rng.choice([-1.0, 1.0])
    return out


def test_decoder_tail_backward(dev, monkeypatch):
    """expansion5 .. expansion1 with disp4 .. disp1 between them at the sizes upstream's decoder derives from an H 32, W 57 input
    (test_decoder_tail's geometry of the forward's file), all three HIP knobs on, a seeded weighted sum of the four disparity maps as the
    loss: the gradients of all 28 parameter tensors, of the layer4 features and of the five skip tensors against the same chain in float64
    on the composites."""
    for knob in ("MCR_EXPANSION_LAYER", "MCR_EXPANSION_LAYER_BWD", "MCR_DISPARITY_HEAD_BWD"):
        monkeypatch.setenv(knob, "hip")
    H, W = 32, 57
    rng = np.random.default_rng(92)
    torch.manual_seed(92)
    spec = [(512, 256, 256, 256, (H // 16, W // 16 + (W % 16 > 0))), (256, 128, 128, 128, (H // 8, W // 8 + (W % 8 > 0))),
            (128, 64, 64, 64, (H // 4, W // 4 + (W % 4 > 0))), (64, 32, 64, 32, (H // 2, W // 2 + (W % 2 > 0))), (32, 16, 3, 16, (H, W))]
    layers = [ManyDepth.ExpansionLayer(ci_, cm, co, size, additional_channels=ca) for ci_, cm, ca, co, size in spec]
    heads = [ManyDepth.DisparityLayer(co) for _, _, _, co, _ in spec[1:]]
    layer4 = t(_smooth_features(rng, 512, 1, 2))
    skips = [t(_smooth_features(rng, ca, *size)) for _, _, ca, _, size in spec]
    weights = [t(rng.standard_normal((1, 1) + size).astype(np.float32)) for _, _, _, _, size in spec[1:]]

    def step(layers, heads, x, skips, weights):
        x, skips = x.requires_grad_(True), [s.requires_grad_(True) for s in skips]
        feats, loss = x, 0.0
        for k, (layer, skip) in enumerate(zip(layers, skips)):
            feats = layer(feats, skip)
            if k:
                loss = loss + (heads[k - 1](feats) * weights[k - 1]).sum()
        loss.backward()
        params = [p.grad for m in list(layers) + list(heads) for p in m.parameters()]
        return params, x.grad, [s.grad for s in skips]

    calls = []
    real = ops.expansion_layer_backward
    monkeypatch.setattr(ops, "expansion_layer_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    got = step([copy.deepcopy(m).to(dev) for m in layers], [copy.deepcopy(m).to(dev) for m in heads], layer4.to(dev),
               [s.to(dev) for s in skips], [w_.to(dev) for w_ in weights])
    assert len(calls) == 5
    want = step([copy.deepcopy(m).double() for m in layers], [copy.deepcopy(m).double() for m in heads], layer4.double(),
                [s.double() for s in skips], [w_.double() for w_ in weights])
    assert len(calls) == 5 and len(got[0]) == 28 and all(g is not None for g in got[0])
    e_params = [rel(g, w_) for g, w_ in zip(got[0], want[0])]
    e_x, e_skips = rel(got[1], want[1]), [rel(g, w_) for g, w_ in zip(got[2], want[2])]
    print(f"ERR decoder tail, forward and backward on HIP vs the fp64 composite chain: parameters (worst of 28) {max(e_params):.2e}, "
          f"layer4 features {e_x:.2e}, skips " + " ".join(f"{v:.2e}" for v in e_skips))
    assert max(e_params) < TOL and e_x < TOL and max(e_skips) < TOL
