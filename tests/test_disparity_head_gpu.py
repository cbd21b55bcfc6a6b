"""The fused disparity head on the GPU (disparity_head.hip: mcr_disparity_head and mcr_disparity_head_backward behind ops.disparity_head,
ops.disparity_head_backward, autograd.DisparityHeadFunction and networks.ManyDepth.DisparityLayer / adopt_disparity_layer) against the
independent fp64 model (tests/_disparity_head_model.py) and the reference's own layer (tests/golden/disparity_head.npz).

Cases (B,C,Hs,Ws), CASES of the model file: a (1,1,2,2) both mirrors of both axes inside a two-pixel axis; b (2,3,3,5) small and odd, row 1
is also row Hs-2; c (1,16,17,33) whole tiles plus one row and one column -- the kernels' tiles are 16 x 4 pixels (forward and d_x; 17 = 4 * 4
+ 1, 33 = 2 * 16 + 1) and 64 x 16 (d_weight; 17 = 16 + 1) --; d (2,128,32,57) upstream's scale 4; e (1,16,35,50); f (1,512,2,3) the channel
cap; g (1,9,129,513), added to the issue's six: from 256 tiles of 32 x 8 on the forward and d_x switch to that tile, which no smaller map
reaches (17 x 17 = 289 tiles, 129 = 16 * 8 + 1, 513 = 16 * 32 + 1 = 8 * 64 + 1; 9 channels: two passes of that tile's 8, so its prefetch runs).

Exact operands, bit equality, no tolerance.  x small integers, weight[c,t] = +-(9c + t + 1) 2^-13 (distinct per tap and channel), bias 0.5:
every partial sum of z in every order is a multiple of 2^-13 below 2^24 of them, so z must equal the model's bit for bit at every pixel
(the reflection indexing, the tile borders, the channel loop).  Backward: y = 0.5 everywhere (y (1 - y) = 0.25) and d_y = k 2^-4: d_x,
d_weight and d_bias must equal the model's bit for bit.  The headroom (the largest sum of magnitudes, in units of the smallest term) is
computed in the model and asserted below 2^24 before the GPU is asked.

Real-valued cases.  Against the model: the project's contract, rel <= TOL = 1e-4 of the largest magnitude (`rel` of
tests/_reconstruction_model.py), for y, d_x, d_weight, d_bias.  Against the golden (cases a, b, c, f): TOL plus the golden's own stored
distance to the model.  Every distance is printed with an ERR prefix before it is asserted.  Measured on an MI355X, worst of the cases:
entries against the model y 1.7e-06, d_x 2.3e-06, d_weight 1.6e-06, d_bias 2.7e-05 (all four in case f, 512 channels on six pixels: d_bias is a
sum of six terms of both signs; elsewhere y <= 9.7e-07, d_x <= 7.0e-07, d_weight <= 4.6e-07, d_bias <= 7.9e-07), the same figures whichever
halves are asked for; against the golden y 2.0e-06, d_x 2.7e-06, d_weight 2.0e-06, d_bias 2.9e-05 (case f; the golden itself is 2.8e-06 from
the model there); DisparityHeadFunction's composite route against its HIP route 8.8e-07, against the model 4.4e-07; four heads through
depth_scale_losses against the fp64 composite chain: losses 1.4e-07, feature gradients 2.7e-06, weight gradients 2.2e-06, bias gradients
1.4e-06.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _disparity_head_model as model                                  # noqa: E402
import _reconstruction_model as rmodel                                 # noqa: E402
from _reconstruction_model import rel                                  # noqa: E402

from macarons_amd import _lib, autograd, ops                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402
from macarons_amd.utility import macarons_utils as mu                  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
TAGS = list(model.ALL_TAGS)
NAMES = ("d_x", "d_weight", "d_bias")
WAYS = {"all": (True, True, True), "x": (True, False, False), "wb": (False, True, True)}


def t(x):
    return torch.as_tensor(np.asarray(x))


@pytest.fixture(scope="module")
def inputs():
    return {tag: model.make_inputs(tag) for tag in TAGS}


@pytest.fixture(scope="module")
def modelled(inputs):
    """The fp64 model of every case -- y and the three gradients of sum(y * g_out) -- computed once and never changed."""
    out = {}
    for tag, c in inputs.items():
        _, y = model.forward(c["x"], c["weight"], c["bias"])
        out[tag] = dict(zip(NAMES, model.backward(c["x"], c["weight"], y, c["g_out"])), y=y)
    return out


def _on(c, dev, keys):
    return [t(c[k]).to(dev) for k in keys]


# ---- 1. exact operands: bit equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_forward_exact_operands(dev, tag):
    e = model.make_exact(tag)
    room = model.exact_headroom(e)
    assert room[0] < 2 ** 24, room
    want, _ = model.forward(e["x"], e["weight"], e["bias"])
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # the model's z is an fp32 value
    x, w, b = _on(e, dev, ("x", "weight", "bias"))
    y, z = ops.disparity_head(x, w, b, return_z=True)
    B, C, Hs, Ws = model.CASES[tag]["shape"]
    assert tuple(y.shape) == tuple(z.shape) == (B, 1, Hs, Ws) and y.dtype == z.dtype == torch.float32
    assert np.array_equal(z[:, 0].cpu().numpy(), want.astype(np.float32)), int((z[:, 0].cpu().numpy() != want.astype(np.float32)).sum())
    assert torch.equal(ops.disparity_head(x, w[None], b), y)                          # upstream's [1,C,3,3], without z: the same y
    assert rel(y[:, 0], t(1.0 / (1.0 + np.exp(-want)))) < 1e-6


@pytest.mark.parametrize("tag", TAGS)
def test_backward_exact_operands(dev, tag):
    e = model.make_exact(tag)
    room = model.exact_headroom(e)
    assert max(room[1:]) < 2 ** 24, room
    want = model.backward(e["x"], e["weight"], e["y"], e["d_y"])
    assert all(np.array_equal(v.astype(np.float32).astype(np.float64), v) for v in want)
    x, w, y, d_y = _on(e, dev, ("x", "weight", "y", "d_y"))
    for how, need in WAYS.items():
        got = ops.disparity_head_backward(x, w, y, d_y, need=need)
        for name, g, v, n in zip(NAMES, got, want, need):
            assert (g is not None) == n, (how, name)
            if n:
                assert g.dtype == torch.float32 and np.array_equal(g.cpu().numpy().reshape(v.shape), v.astype(np.float32)), (how, name)


# ---- 2. real values against the model and the golden ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_entries_match_model(dev, inputs, modelled, tag):
    c, m = inputs[tag], modelled[tag]
    x, w, b, g_out = _on(c, dev, ("x", "weight", "bias", "g_out"))
    y = ops.disparity_head(x, w, b)
    e = dict(y=rel(y[:, 0], t(m["y"])))
    for how, need in WAYS.items():
        got = ops.disparity_head_backward(x, w, y, g_out, need=need)
        for name, g, n in zip(NAMES, got, need):
            if n:
                assert tuple(g.shape) == tuple(c[name[2:]].shape if name != "d_bias" else (1,)) and bool(torch.isfinite(g).all())
                e[f"{name} ({how})"] = rel(g.reshape(m[name].shape), t(m[name]))
    print(f"ERR case {tag}, entries vs model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < TOL


@pytest.mark.parametrize("tag", model.GOLDEN_TAGS)
def test_entries_match_golden(dev, tag):
    g = model.load_golden(tag)
    x, w, b, g_out = _on(g, dev, ("x", "weight", "bias", "g_out"))
    y = ops.disparity_head(x, w, b)
    got = dict(zip(NAMES, ops.disparity_head_backward(x, w, y, g_out)), y=y)
    e = {k: rel(v, t(g[k])) for k, v in got.items()}
    print(f"ERR case {tag}, entries vs golden: " + " ".join(f"{k} {v:.2e}" for k, v in e.items())
          + " (golden vs model: " + " ".join(f"{k} {v:.1e}" for k, v in g["distance"].items()) + ")")
    for k, v in e.items():
        assert v < TOL + g["distance"][k], k


# ---- 3. the backward three ways through the C ABI: a half that is not asked for is not written --------------------------------------------
def _c_backward(L, x, w, y, d_y, outs, need, ws):
    B, C, Hs, Ws = x.shape
    vp = ctypes.c_void_p
    ptr = [vp(o.data_ptr()) if n else None for o, n in zip(outs, need)]
    return L.mcr_disparity_head_backward(vp(x.data_ptr()) if need[1] else None, vp(w.data_ptr()) if need[0] else None, vp(y.data_ptr()),
                                         vp(d_y.data_ptr()), *ptr, ctypes.c_int64(B), ctypes.c_int(C), ctypes.c_int(Hs), ctypes.c_int(Ws),
                                         vp(ws.data_ptr()), ctypes.c_size_t(ws.numel()), None)


@pytest.mark.parametrize("tag", ["b", "c", "f"])
def test_backward_three_ways_leaves_the_rest_untouched(dev, inputs, tag):
    L = _lib.lib()
    c = inputs[tag]
    x, w, b, g_out = _on(c, dev, ("x", "weight", "bias", "g_out"))
    y = ops.disparity_head(x, w, b)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    full = ops.disparity_head_backward(x, w, y, g_out)
    ways = dict(WAYS, w=(False, True, False), b=(False, False, True))    # the ABI also takes d_weight and d_bias apart
    for how, need in ways.items():
        outs = [torch.full_like(x, -7.0), torch.full_like(w, -7.0), torch.full((1,), -7.0, device=dev)]
        assert _c_backward(L, x, w, y, g_out, outs, need, ws) == 0, L.mcr_last_error().decode()
        torch.cuda.synchronize()
        for name, o, f, n in zip(NAMES, outs, full, need):
            assert torch.equal(o, f) if n else bool((o == -7.0).all()), (how, name)       # the operands it does not need were NULL as well


# ---- 4. the same bits on every call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_two_calls_give_the_same_bits(dev, inputs, tag):
    x, w, b, g_out = _on(inputs[tag], dev, ("x", "weight", "bias", "g_out"))
    one, two = ops.disparity_head(x, w, b, return_z=True), ops.disparity_head(x, w, b, return_z=True)
    assert all(torch.equal(p, q) for p, q in zip(one, two))
    b1, b2 = ops.disparity_head_backward(x, w, one[0], g_out), ops.disparity_head_backward(x, w, one[0], g_out)
    assert all(torch.equal(p, q) for p, q in zip(b1, b2))


# ---- 5. the autograd function ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["b", "c", "d"])
def test_function_is_the_backward_entry(dev, inputs, monkeypatch, tag):
    monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", "hip")
    assert autograd.disparity_head_backward_mode() == "hip"
    x, w, b, g_out = _on(inputs[tag], dev, ("x", "weight", "bias", "g_out"))
    leaves = [x.clone().requires_grad_(True), w[None].clone().requires_grad_(True), b.clone().requires_grad_(True)]
    y = autograd.DisparityHeadFunction.apply(*leaves)
    assert y.requires_grad and torch.equal(y, ops.disparity_head(x, w, b))
    grads = torch.autograd.grad((y[:, 0] * g_out).sum(), leaves, retain_graph=True)
    want = ops.disparity_head_backward(x, w, y.detach(), g_out)
    assert all(g.shape == leaf.shape and torch.equal(g.reshape(v.shape), v) for g, leaf, v in zip(grads, leaves, want))
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(y.sum(), leaves, create_graph=True)


@pytest.mark.parametrize("tag", ["b", "c", "d"])
def test_function_composite_route(dev, inputs, modelled, monkeypatch, tag):
    x, w, b, g_out = _on(inputs[tag], dev, ("x", "weight", "bias", "g_out"))
    grads = {}
    for route in ("hip", "composite"):
        monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", route)
        assert autograd.disparity_head_backward_mode() == route
        leaves = [x.clone().requires_grad_(True), w[None].clone().requires_grad_(True), b.clone().requires_grad_(True)]
        y = autograd.DisparityHeadFunction.apply(*leaves)
        grads[route] = torch.autograd.grad((y[:, 0] * g_out).sum(), leaves)
    e = {n: rel(c_, h) for n, h, c_ in zip(NAMES, grads["hip"], grads["composite"])}
    e.update({n + " vs model": rel(c_.reshape(modelled[tag][n].shape), t(modelled[tag][n])) for n, c_ in zip(NAMES, grads["composite"])})
    print(f"ERR case {tag}, DisparityHeadFunction composite route vs hip route: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < TOL


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, False, True), (True, True, False)])
def test_function_honours_needs_input_grad(dev, inputs, monkeypatch, needs):
    monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", "hip")
    x, w, b, g_out = _on(inputs["b"], dev, ("x", "weight", "bias", "g_out"))
    asked = []
    real = ops.disparity_head_backward
    monkeypatch.setattr(ops, "disparity_head_backward", lambda *a, **k: asked.append(k["need"]) or real(*a, **k))
    leaves = [v.clone().requires_grad_(n) for v, n in zip((x, w[None], b), needs)]
    y = autograd.DisparityHeadFunction.apply(*leaves)
    (y[:, 0] * g_out).sum().backward()
    assert asked == [needs]                                             # one call, only the halves that an input needs
    full = real(x, w, y.detach(), g_out)
    for leaf, n, f in zip(leaves, needs, full):
        assert (leaf.grad is None) if not n else torch.equal(leaf.grad.reshape(f.shape), f)


# ---- 6. the module: mirror and adopted upstream-like instance -----------------------------------------------------------------------------------
def test_layer_routes(dev, inputs, monkeypatch):
    c = inputs["c"]
    x, w, b = _on(c, dev, ("x", "weight", "bias"))
    layer = ManyDepth.DisparityLayer(16).to(dev)
    layer.load_state_dict({"conv.weight": w[None], "conv.bias": b})
    with torch.no_grad():
        assert torch.equal(layer(x), ops.disparity_head(x, w, b))      # no gradient: the entry itself
    # with a gradient required the route is the backward mode's: the composite under autograd by default, the Function with =hip
    monkeypatch.delenv("MCR_DISPARITY_HEAD_BWD", raising=False)
    y = layer(x)
    assert y.grad_fn is not None and "DisparityHeadFunction" not in type(y.grad_fn).__name__
    assert rel(y, ops.disparity_head(x, w, b)) < TOL
    monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", "hip")
    y = layer(x)
    assert y.grad_fn is not None and "DisparityHeadFunction" in type(y.grad_fn).__name__ and torch.equal(y, ops.disparity_head(x, w, b))
    # what the entry does not take goes to the composite: another dtype, autocast, a strided input
    assert layer.double()(x.double()).dtype == torch.float64
    layer.float()
    with torch.no_grad():
        strided = layer(x.transpose(2, 3))
        assert rel(strided, ManyDepth.disparity_head_composite(x.transpose(2, 3), layer.conv.weight, layer.conv.bias)) < 1e-6
        with torch.autocast("cuda", dtype=torch.float16):
            assert layer(x).dtype == torch.float16
    # an adopted upstream-like instance takes the same route
    up = torch.nn.Module()
    up.channels, up.conv, up.sigmoid = 16, torch.nn.Conv2d(16, 1, 3, padding=1, padding_mode="reflect"), torch.nn.Sigmoid()
    up = ManyDepth.adopt_disparity_layer(up.to(dev))
    up.load_state_dict(layer.state_dict())
    assert torch.equal(up(x), y)


# ---- 7. the C entries refuse before they launch ---------------------------------------------------------------------------------------------------
def test_c_entries_refuse_without_launching(dev):
    L = _lib.lib()
    B, C, Hs, Ws = 1, 3, 4, 6
    x, w, b = torch.ones(B, C, Hs, Ws, device=dev), torch.ones(C, 3, 3, device=dev), torch.zeros(1, device=dev)
    y_in, d_y = torch.full((B, Hs, Ws), 0.5, device=dev), torch.ones(B, Hs, Ws, device=dev)
    outs = dict(y=torch.full((B, Hs, Ws), -7.0, device=dev), z=torch.full((B, Hs, Ws), -7.0, device=dev), d_x=torch.full_like(x, -7.0),
                d_w=torch.full_like(w, -7.0), d_b=torch.full((1,), -7.0, device=dev))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    i64, ci, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

    def call(back, B_=B, C_=C, Hs_=Hs, Ws_=Ws, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), none=False):
        if back:
            o = [None] * 3 if none else [vp(outs[k].data_ptr()) for k in ("d_x", "d_w", "d_b")]
            return L.mcr_disparity_head_backward(vp(x.data_ptr()), vp(w.data_ptr()), vp(y_in.data_ptr()), vp(d_y.data_ptr()), *o, i64(B_), ci(C_),
                                                 ci(Hs_), ci(Ws_), vp(ws_ptr), sz(ws_bytes), None)
        return L.mcr_disparity_head(vp(x.data_ptr()), vp(w.data_ptr()), vp(b.data_ptr()), vp(outs["y"].data_ptr()), vp(outs["z"].data_ptr()),
                                    i64(B_), ci(C_), ci(Hs_), ci(Ws_), None)

    sizes = [dict(Hs_=1), dict(Ws_=1), dict(C_=0), dict(C_=513), dict(B_=0), dict(B_=-1), dict(B_=2 ** 31, C_=1, Hs_=2, Ws_=2),
             dict(C_=512, Hs_=2 ** 11, Ws_=2 ** 11)]
    for back in (False, True):
        for kw in sizes:
            assert call(back, **kw) == 1, (back, kw)
            assert L.mcr_last_error().decode().startswith("mcr_disparity_head"), kw
    for kw in (dict(ws_bytes=64), dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=ws.numel() - 4), dict(ws_ptr=None)):
        assert call(True, **kw) == 1 and "workspace" in L.mcr_last_error().decode(), kw
    assert call(True, none=True) == 1 and "all NULL" in L.mcr_last_error().decode()
    for bad in (dict(x=torch.ones(B, C, 1, Ws, device=dev)), dict(x=torch.ones(B, 513, 2, 2, device=dev), weight=torch.ones(513, 3, 3, device=dev))):
        with pytest.raises(ValueError):
            ops.disparity_head(bad["x"], bad.get("weight", w), b)
    with pytest.raises(ValueError):
        ops.disparity_head_backward(x, w, y_in, d_y, need=(False, False, False))
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in outs.values())         # nothing was launched
    assert call(False) == 0 and call(True) == 0                         # and the same calls, well-formed, run
    torch.cuda.synchronize()
    assert all(bool((v != -7.0).all()) for v in outs.values())
    assert bool((outs["z"] == 27.0).all()) and bool((outs["d_b"] == 0.25 * B * Hs * Ws).all())      # 27 ones; sum of 1 * 0.25


# ---- 8. end to end: from the decoder's features to the loss and back ----------------------------------------------------------------------------
def _smooth_features(rng, C, Hs, Ws):
    v, u = np.meshgrid((np.arange(Hs) + 0.5) / Hs, (np.arange(Ws) + 0.5) / Ws, indexing="ij")
    out = np.empty((1, C, Hs, Ws), np.float32)
    for c in range(C):
        k, th, ph = rng.uniform(2.0, 6.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        out[0, c] = np.sin(k * (np.cos(th) * u + np.sin(th) * v) + ph) + 0.3 * (u - 0.5) * rng.choice([-1.0, 1.0])
    return out


def test_four_heads_feed_the_depth_losses(dev, monkeypatch):
    """Four heads at the (H 32, W 57)-derived shapes of upstream's decoder feed depth_scale_losses; the gradients into the four feature
    maps and the eight parameters against the same chain in float64 on the composites (disparity_head_composite,
    disparity_scales_composite, reconstruction_loss_composite).  Smooth features, so that the disparities are smooth and no sign or
    selection sits at a tie; one source per image, as in test_disparity_scales_gpu.py.  MCR_DISPARITY_HEAD_BWD=hip: the heads' HIP backward is the subject."""
    monkeypatch.setenv("MCR_DISPARITY_HEAD_BWD", "hip")
    H, W = 32, 57
    shapes = [(16, 32, 57), (32, 16, 29), (64, 8, 15), (128, 4, 8)]
    rng = np.random.default_rng(77)
    torch.manual_seed(77)
    feats = [t(_smooth_features(rng, *s)) for s in shapes]
    heads = [ManyDepth.DisparityLayer(s[0]) for s in shapes]
    smooth = np.random.default_rng(78)
    import _disparity_model as dmodel
    images, alpha = t(dmodel.smooth_images(smooth, 1, H, W)), t(dmodel.smooth_images(smooth, 1, H, W))[:, None]
    mask = torch.ones(1, H, W, dtype=torch.bool)
    mask[:, 5:11, 20:33] = False
    rc = rmodel.load_case("a")                                          # its target and first-source poses
    R, T, Ra, Ta = rc["R"][:1], rc["T"][:1], rc["R_alpha"][:1, :1], rc["T_alpha"][:1, :1] * 0.2
    params = SimpleNamespace(znear=0.5, zfar=750.0, ssim_factor=0.85, use_depth_mask=True, regularity_loss=True, regularity_factor=1.0)
    # the HIP chain
    dev_heads = [ManyDepth.DisparityLayer(h.channels).to(dev) for h in heads]
    for d, h in zip(dev_heads, heads):
        d.load_state_dict(h.state_dict())
    leaves = [f.to(dev).requires_grad_(True) for f in feats]
    disps = [h(f) for h, f in zip(dev_heads, leaves)]
    assert all("DisparityHeadFunction" in type(d.grad_fn).__name__ for d in disps)
    dl, rl, *_ = mu.depth_scale_losses(params, disps, images.to(dev), alpha.to(dev), mask.to(dev)[..., None], SimpleNamespace(R=R.to(dev), T=T.to(dev)),
                                       SimpleNamespace(R=Ra.reshape(-1, 3, 3).to(dev), T=Ta.reshape(-1, 3).to(dev)), "border")
    (dl + rl).backward()
    # the same chain in float64 on the composites
    ref_heads = [h.double() for h in heads]
    ref = [f.double().requires_grad_(True) for f in feats]
    d6 = [ManyDepth.disparity_head_composite(f, h.conv.weight, h.conv.bias) for h, f in zip(ref_heads, ref)]
    depth6, reg6, _ = ManyDepth.disparity_scales_composite(d6, images, mask, 0.5, 750.0)
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta).double()
    l6 = ManyDepth.reconstruction_loss_composite(images, alpha, mask, cams, depth6, 750.0, 0.85, "border")
    want_reg = sum(reg6[s] * 0.5 ** s for s in range(4))
    (l6.sum() + want_reg).backward()
    e = dict(depth_loss=rel(dl, l6.sum()), regularity_loss=rel(rl, want_reg))
    for k, (a, b_, hd, hr) in enumerate(zip(leaves, ref, dev_heads, ref_heads)):
        e[f"d_feat{k + 1}"] = rel(a.grad, b_.grad)
        e[f"d_weight{k + 1}"] = rel(hd.conv.weight.grad, hr.conv.weight.grad)
        e[f"d_bias{k + 1}"] = rel(hd.conv.bias.grad, hr.conv.bias.grad)
    print("ERR four heads -> depth_scale_losses vs the fp64 composite chain: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) < TOL
