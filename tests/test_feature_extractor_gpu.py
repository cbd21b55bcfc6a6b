"""The fused front of the depth encoder on the GPU (resnet_stem.hip, basic_block.hip: mcr_resnet_stem, mcr_basic_block and
mcr_feature_extractor behind ops.resnet_stem, ops.basic_block and ops.feature_extractor; networks.ManyDepth.FeatureExtractor,
adopt_feature_extractor, adopt_depth_front) against the independent fp64 model (tests/_feature_extractor_model.py) and upstream's own
extractor (tests/golden/feature_extractor.npz).

Stem cases (N0, N1, Cin, Cout, H x W), STEM_CASES of the model file: a (1,0,1,1, 1x1); b (2,1,3,5, 7x9); c (1,2,3,64, 16x30); d (1,1,6,17,
9x20) with a convolution bias; e (0,2,8,64, 5x4); f (1,1,3,17, 10x62), one more than the kernel's tile -- 2 x 15 pooled pixels, 16 output
channels a wave -- in every tiled dimension.  Block cases (B, C, H x W): a (1,1, 1x1); b (2,3, 5x7); c (1,64, 16x29); d (1,17, 9x17); e
(2,33, 33x225), 288 workgroups of the 32-channel tile; f (1,512, 8x15).  The extractor: (1,2, 3 -> 64, 32x57) with two blocks, without
blocks, and without conv1.

1. Exact operands, bit equality, no tolerance (make_*_exact of the model file); the headroom is asserted in the model before the GPU is
asked.  2. Real values against the model (rel < 1e-4 of the largest magnitude), the golden (that plus its stored distance) and the fp32
composite on the device.  3. Poisoning.  4. Two calls give the same bits.  5. The C entries refuse without launching.  6. The routes.

Measured on an MI355X, worst of the cases: exact operands, 0 values differ in every case (stem pooled and conv1, block t and y, the
extractor with 2 and with 0 blocks); against the model the stem 4.3e-07 pooled (case b) and 5.3e-07 conv1 (case d), the block t 1.2e-06 and
y 5.7e-07 (case f, K = 4608; elsewhere at most 5.8e-07), the extractor features 3.5e-07, conv1 3.7e-07; against the golden 5.9e-07 (case
d; the golden itself is at most 5.8e-07 from the model); the composite in fp32 on the device against the entry 6.5e-07 (stem b), 5.3e-07
(block f), 4.8e-07 (extractor); the adopted extractor against its own modules in torch (the blocks included: a mirror BasicBlock is
never routed) 4.2e-07; the adopted decoder against the unadopted one, which is torch throughout, disp1 1.1e-07, disp2 1.1e-07, disp3
1.2e-07, disp4 1.2e-07.
"""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _feature_extractor_model as model                               # noqa: E402
from _depth_front_stand_in import StandInDecoder, decoder_inputs, randomize_batch_norms, resnet_front    # noqa: E402

from macarons_amd import _lib, ops                                     # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4


def on(v, dev):
    """A case's operand on the device: arrays become tensors, tuples and lists keep their structure, floats and None pass."""
    if isinstance(v, (tuple, list)):
        return type(v)(on(u, dev) for u in v)
    return v if v is None or isinstance(v, float) else torch.as_tensor(np.asarray(v)).to(dev)


def stem_args(c, dev):
    return [on(c[k], dev) for k in ("x", "x_more", "weight", "bias", "bn")] + [c["eps"]]


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy(), np.asarray(want, np.float64).astype(np.float32))


@pytest.fixture(scope="module")
def stem_inputs():
    return {tag: model.make_stem_inputs(tag) for tag in model.STEM_TAGS}


@pytest.fixture(scope="module")
def stem_modelled(stem_inputs):
    """The fp64 model of every real-valued stem case, computed once and never changed."""
    return {tag: model.stem(model.images_of(c), c["weight"], c["bias"], c["bn"], c["eps"]) for tag, c in stem_inputs.items()}


@pytest.fixture(scope="module")
def block_inputs():
    return {tag: model.make_block_inputs(tag) for tag in model.BLOCK_TAGS}


@pytest.fixture(scope="module")
def block_modelled(block_inputs):
    return {tag: model.block(c["x"], *c["block"]) for tag, c in block_inputs.items()}


@pytest.fixture(scope="module")
def extractor_inputs():
    return model.make_extractor_inputs()


@pytest.fixture(scope="module")
def extractor_modelled(extractor_inputs):
    c = extractor_inputs
    return model.extractor(model.images_of(c), c["weight"], c["bias"], c["bn"], c["eps"], c["blocks"])


def poison(monkeypatch):
    """Every float32 tensor ops allocates with torch.empty holds -7 (the outputs), every arena NaN bytes; -> the poisoned outputs."""
    poisoned, real_empty = [], torch.empty

    def empty(*size, **kw):
        out = real_empty(*size, **kw)
        if kw.get("dtype") is torch.float32:
            out.fill_(-7.0)
            poisoned.append(out)
        elif kw.get("dtype") is torch.uint8:
            out.fill_(0xFF)
        return out

    monkeypatch.setattr(ops.torch, "empty", empty)
    for buf in ops._ws_cache.values():
        buf.fill_(0xFF)
    return poisoned


def clean(t):
    return bool(torch.isfinite(t).all()) and not bool((t == -7.0).any())


# ---- 1. exact operands: bit equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", model.STEM_TAGS)
def test_stem_exact_operands(dev, tag):
    e = model.make_stem_exact(tag)
    room = model.stem_headroom(e)
    want = model.stem(model.images_of(e), e["weight"], e["bias"], e["bn"], 0.0)
    assert room < 2 ** 24 and model.is_fp32(want["conv1"]) and model.is_fp32(want["pooled"])
    N0 = model.STEM_CASES[tag]["shape"][0]
    pooled, conv1 = ops.resnet_stem(*stem_args(e, dev))
    wrong = int((pooled.cpu().numpy() != want["pooled"].astype(np.float32)).sum())
    wrong1 = 0 if N0 == 0 else int((conv1.cpu().numpy() != want["conv1"][:N0].astype(np.float32)).sum())
    print(f"ERR stem case {tag}, exact operands: headroom 2^{np.log2(room):.1f}, pooled {wrong} of {pooled.numel()} differ, conv1 {wrong1} differ, "
          f"{int((want['pre'] > 0).sum())} positive and {int((want['pre'] < 0).sum())} negative before ReLU, "
          f"{int((model.max_pool(want['pre']) < 0).sum())} windows all negative")
    assert (conv1 is None) == (N0 == 0) and pooled.dtype == torch.float32 and pooled.is_contiguous()
    assert tuple(pooled.shape) == want["pooled"].shape and wrong == 0 and wrong1 == 0


@pytest.mark.parametrize("tag", model.BLOCK_TAGS)
def test_block_exact_operands(dev, tag):
    e = model.make_block_exact(tag)
    room = model.block_headroom(e)
    want = model.block(e["x"], *e["block"])
    assert max(room) < 2 ** 24 and model.is_fp32(want["t"]) and model.is_fp32(want["y"])
    flips = int(((want["pre"] < 0) & (want["pre"] + e["x"] > 0)).sum())
    y, t = ops.basic_block(on(e["x"], dev), *on(e["block"], dev), return_t=True)
    wrong_t, wrong_y = int((t.cpu().numpy() != want["t"].astype(np.float32)).sum()), int((y.cpu().numpy() != want["y"].astype(np.float32)).sum())
    print(f"ERR block case {tag}, exact operands: headroom 2^{np.log2(max(room[0], 1)):.1f} 2^{np.log2(room[1]):.1f}, t {wrong_t} and y {wrong_y} of "
          f"{y.numel()} differ; {int((want['y'] > 0).sum())} positive outputs, the residual changes the sign of {flips}")
    assert wrong_t == 0 and wrong_y == 0 and (tag == "a" or (flips > 0 and (want["y"] == 0).any() and (want["t"] > 0).any()))


@pytest.mark.parametrize("n_blocks", [2, 0])
def test_extractor_exact_operands(dev, n_blocks):
    e = model.make_extractor_exact(n_blocks)
    rooms = model.extractor_headroom(e)
    want = model.extractor(model.images_of(e), e["weight"], None, e["bn"], 0.0, e["blocks"])
    assert max(rooms) < 2 ** 24 and all(model.is_fp32(want[k]) for k in want)
    feats, conv1 = ops.feature_extractor(*stem_args(e, dev), on(e["blocks"], dev))
    print(f"ERR extractor with {n_blocks} blocks, exact operands: headroom 2^{np.log2(max(rooms)):.1f}, "
          f"{int((want['features'] > 0).sum())} of {want['features'].size} features positive")
    assert same_bits(feats, want["features"]) and same_bits(conv1, want["conv1"][:1])
    assert (want["features"] > 0).any() and (want["features"] == 0).any()


# ---- 2. real values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", model.STEM_TAGS)
def test_stem_real_values(dev, stem_inputs, stem_modelled, tag):
    c, want = stem_inputs[tag], stem_modelled[tag]
    N0 = model.STEM_CASES[tag]["shape"][0]
    pooled, conv1 = ops.resnet_stem(*stem_args(c, dev))
    images = torch.cat([v for v in stem_args(c, dev)[:2] if v is not None])
    comp_pooled, comp_conv1 = ManyDepth.resnet_stem_composite(images, *stem_args(c, dev)[2:])
    e = [model.rel(pooled.cpu().numpy(), want["pooled"]), 0.0 if N0 == 0 else model.rel(conv1.cpu().numpy(), want["conv1"][:N0]),
         model.rel(comp_pooled.cpu().numpy(), pooled.cpu().numpy())]
    print(f"ERR stem case {tag}, entry vs model: pooled {e[0]:.2e} conv1 {e[1]:.2e}; composite (float32, device) vs entry: pooled {e[2]:.2e}")
    assert max(e) < TOL


@pytest.mark.parametrize("tag", model.BLOCK_TAGS)
def test_block_real_values(dev, block_inputs, block_modelled, tag):
    c, want = block_inputs[tag], block_modelled[tag]
    y, t = ops.basic_block(on(c["x"], dev), *on(c["block"], dev), return_t=True)
    comp = ManyDepth.basic_block_composite(on(c["x"], dev), *on(c["block"], dev))
    e = [model.rel(t.cpu().numpy(), want["t"]), model.rel(y.cpu().numpy(), want["y"]), model.rel(comp.cpu().numpy(), y.cpu().numpy())]
    print(f"ERR block case {tag}, entry vs model: t {e[0]:.2e} y {e[1]:.2e}; composite (float32, device) vs entry: y {e[2]:.2e}")
    assert max(e) < TOL


def test_extractor_real_values(dev, extractor_inputs, extractor_modelled):
    c, want = extractor_inputs, extractor_modelled
    feats, conv1 = ops.feature_extractor(*stem_args(c, dev), on(c["blocks"], dev))
    none, no_conv1 = ops.feature_extractor(*stem_args(c, dev), [], want_conv1=True)[0], ops.feature_extractor(*stem_args(c, dev), on(c["blocks"], dev), want_conv1=False)
    images = torch.cat(stem_args(c, dev)[:2])
    comp, comp_conv1 = ManyDepth.feature_extractor_composite(images, *stem_args(c, dev)[2:], on(c["blocks"], dev))
    e = [model.rel(feats.cpu().numpy(), want["features"]), model.rel(conv1.cpu().numpy(), want["conv1"][:1]),
         model.rel(none.cpu().numpy(), want["pooled"]), model.rel(comp.cpu().numpy(), feats.cpu().numpy())]
    print(f"ERR extractor, entry vs model: features {e[0]:.2e} conv1 {e[1]:.2e}, without blocks {e[2]:.2e}; composite (float32, device) vs entry: "
          f"features {e[3]:.2e}")
    assert tuple(feats.shape) == (3, 64, 8, 15) and tuple(conv1.shape) == (1, 64, 16, 29) and max(e) < TOL
    assert no_conv1[1] is None and torch.equal(no_conv1[0], feats)
    # the pieces give the whole: the stem and two block entries
    y = ops.resnet_stem(*stem_args(c, dev))[0]
    for blk in on(c["blocks"], dev):
        y = ops.basic_block(y, *blk)
    assert torch.equal(y, feats)


@pytest.mark.parametrize("tag", model.GOLDEN_TAGS)
def test_real_values_match_the_golden(dev, tag):
    g = model.load_golden(tag)
    feats, _ = ops.feature_extractor(*stem_args(g, dev), on(g["blocks"], dev), want_conv1=False)
    e = model.rel(feats.cpu().numpy(), g["features"])
    print(f"ERR golden case {tag}, entry vs golden: features {e:.2e} (the golden's distance to the model {g['distance']:.2e})")
    assert g["distance"] < 1e-5 and e < TOL + g["distance"]


def test_an_infinite_pixel_stays_within_the_windows_that_cover_it(dev, stem_inputs):
    """Case f (K = 147, one padded k; four tiles): an Inf at pixel (1,1) of the second image -- a cell the padded k would read if it
    multiplied staged pixels instead of zeros -- gives the infinities of the model, in the windows that cover the pixel, and no NaN."""
    c = dict(stem_inputs["f"])
    c["x_more"] = c["x_more"].copy()
    c["x_more"][0, 0, 1, 1] = np.inf
    with np.errstate(invalid="ignore"):
        want = model.stem(model.images_of(c), c["weight"], c["bias"], c["bn"], c["eps"])
    pooled, conv1 = ops.resnet_stem(*stem_args(c, dev))
    got, inf = pooled.cpu().numpy(), np.isinf(want["pooled"])
    assert not np.isnan(want["pooled"]).any() and inf[1].any() and not inf[0].any() and not inf[1, :, 2:].any() and not inf[1, :, :, 2:].any()
    assert not np.isnan(got).any() and np.array_equal(np.isinf(got), inf)
    assert model.rel(np.where(inf, 0.0, got), np.where(inf, 0.0, want["pooled"])) < TOL and model.rel(conv1.cpu().numpy(), want["conv1"][:1]) < TOL


# ---- 3. poisoning, 4. the same bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", model.STEM_TAGS)
def test_stem_writes_every_output_and_gives_the_same_bits(dev, stem_inputs, monkeypatch, tag):
    args = stem_args(stem_inputs[tag], dev)
    poisoned = poison(monkeypatch)
    pooled, conv1 = ops.resnet_stem(*args)
    monkeypatch.undo()
    assert any(p is pooled for p in poisoned) and clean(pooled) and (conv1 is None or (any(p is conv1 for p in poisoned) and clean(conv1)))
    again = ops.resnet_stem(*args)
    assert torch.equal(again[0], pooled) and (conv1 is None or torch.equal(again[1], conv1))
    assert torch.equal(ops.resnet_stem(*args, want_conv1=False)[0], pooled)


def test_stem_without_conv1_leaves_its_neighbour_alone(dev, stem_inputs):
    """The C entry with conv1 NULL: a sentinel buffer right behind `pooled` in one allocation is untouched."""
    c = stem_inputs["c"]
    N0, N1, Cin, Cout, (H, W) = model.STEM_CASES["c"]["shape"]
    Hc, Wc, Hp, Wp = ops.resnet_stem_sizes(H, W)
    n = (N0 + N1) * Cout * Hp * Wp
    both = torch.full((n + N0 * Cout * Hc * Wc,), -7.0, device=dev)
    x, x_more, w, _, bn, eps = stem_args(c, dev)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    rc = _lib.lib().mcr_resnet_stem(vp(x.data_ptr()), vp(x_more.data_ptr()), vp(w.data_ptr()), None, *[vp(t.data_ptr()) for t in bn],
                                    ctypes.c_float(eps), vp(both.data_ptr()), None, i64(N0), i64(N1), ci(Cin), ci(Cout), ci(H), ci(W), None)
    torch.cuda.synchronize()
    assert rc == 0 and clean(both[:n]) and bool((both[n:] == -7.0).all())
    assert torch.equal(both[:n].view(N0 + N1, Cout, Hp, Wp), ops.resnet_stem(x, x_more, w, None, bn, eps)[0])


@pytest.mark.parametrize("tag", model.BLOCK_TAGS)
def test_block_writes_every_output_and_gives_the_same_bits(dev, block_inputs, monkeypatch, tag):
    x, blk = on(block_inputs[tag]["x"], dev), on(block_inputs[tag]["block"], dev)
    poisoned = poison(monkeypatch)
    y = ops.basic_block(x, *blk)
    monkeypatch.undo()
    assert any(p is y for p in poisoned) and clean(y)
    assert torch.equal(ops.basic_block(x, *blk), y)


def test_extractor_writes_every_output_and_gives_the_same_bits(dev, extractor_inputs, monkeypatch):
    c = extractor_inputs
    args = stem_args(c, dev) + [on(c["blocks"], dev)]
    poisoned = poison(monkeypatch)
    feats, conv1 = ops.feature_extractor(*args)
    one = ops.feature_extractor(*args[:-1], args[-1][:1], want_conv1=False)[0]
    monkeypatch.undo()
    assert len(poisoned) == 3 and clean(feats) and clean(conv1) and clean(one)
    again = ops.feature_extractor(*args)
    assert torch.equal(again[0], feats) and torch.equal(again[1], conv1)


# ---- 5. the C entries refuse before they launch ------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_without_launching(dev):
    L = _lib.lib()
    vp, i64, ci, cf, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    N0, N1, Cin, Cout, H, W = 2, 1, 3, 5, 7, 9
    Hc, Wc, Hp, Wp = ops.resnet_stem_sizes(H, W)
    x, xm, w = torch.ones(N0, Cin, H, W, device=dev), torch.ones(N1, Cin, H, W, device=dev), torch.ones(Cout, Cin, 7, 7, device=dev)
    bn = [torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev), torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)]
    blk = [torch.ones(Cout, Cout, 3, 3, device=dev)] + bn + [torch.ones(Cout, Cout, 3, 3, device=dev)] + bn
    pooled, conv1 = torch.full((N0 + N1, Cout, Hp, Wp), -7.0, device=dev), torch.full((N0, Cout, Hc, Wc), -7.0, device=dev)
    bx, by = torch.ones(N0, Cout, Hp, Wp, device=dev), torch.full((N0, Cout, Hp, Wp), -7.0, device=dev)
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    pointers = (ctypes.c_void_p * 10)(*[t.data_ptr() for t in blk])
    eps2 = (ctypes.c_float * 2)(0.0, 0.0)
    ptr = lambda t: None if t is None else vp(t.data_ptr())                                               # noqa: E731

    def stem(N0=N0, N1=N1, Cin=Cin, Cout=Cout, H=H, W=W, x=x, xm=xm, w=w, bn0=bn[0], var=bn[3], pooled=pooled):
        return L.mcr_resnet_stem(ptr(x), ptr(xm), ptr(w), None, ptr(bn0), ptr(bn[1]), ptr(bn[2]), ptr(var), cf(0.0), ptr(pooled), ptr(conv1),
                                 i64(N0), i64(N1), ci(Cin), ci(Cout), ci(H), ci(W), None)

    def extractor(N0=N0, N1=N1, Cin=Cin, Cout=Cout, H=H, W=W, x=x, xm=xm, n_blocks=1, pointers=pointers, eps=eps2, ws_ptr=ws.data_ptr(),
                  ws_bytes=ws.numel(), feats=pooled):
        return L.mcr_feature_extractor(ptr(x), ptr(xm), ptr(w), None, *[ptr(t) for t in bn], cf(0.0), pointers, eps, ci(n_blocks), ptr(feats),
                                       ptr(conv1), i64(N0), i64(N1), ci(Cin), ci(Cout), ci(H), ci(W), vp(ws_ptr), sz(ws_bytes), None)

    def block(B=N0, C=Cout, H=Hp, W=Wp, x=bx, y=by, w2=blk[5], mean=bn[2], ws_ptr=ws.data_ptr(), ws_bytes=ws.numel()):
        return L.mcr_basic_block(ptr(x), ptr(blk[0]), ptr(bn[0]), ptr(bn[1]), ptr(mean), ptr(bn[3]), cf(0.0), ptr(w2), *[ptr(t) for t in bn],
                                 cf(0.0), ptr(y), i64(B), ci(C), ci(H), ci(W), vp(ws_ptr), sz(ws_bytes), None)

    big = 2 ** 31
    stem_sizes = [dict(H=0), dict(W=0), dict(Cin=0), dict(Cin=9), dict(Cout=0), dict(Cout=65), dict(N0=-1), dict(N1=-1), dict(N0=0, N1=0),
                  dict(N0=big), dict(N0=2 ** 20, Cin=8, H=16, W=16), dict(N1=2 ** 21, Cout=64, H=8, W=8), dict(Cout=64, H=2 ** 13, W=2 ** 13)]
    for entry, name in ((stem, "mcr_resnet_stem"), (extractor, "mcr_feature_extractor")):
        for kw in stem_sizes:
            assert entry(**kw) == 1 and L.mcr_last_error().decode().startswith(name), (name, kw)
            if entry is extractor:
                sizes = dict(N0=N0, N1=N1, Cin=Cin, Cout=Cout, H=H, W=W)
                sizes.update(kw)
                assert L.mcr_feature_extractor_workspace_bytes(*[i64(sizes[k]) for k in ("N0", "N1", "Cin", "Cout", "H", "W")], i64(1)) == 0, kw
        for kw in (dict(x=None), dict(xm=None)):
            assert entry(**kw) == 1 and "NULL" in L.mcr_last_error().decode(), (name, kw)
    for kw in (dict(w=None), dict(bn0=None), dict(var=None), dict(pooled=None)):
        assert stem(**kw) == 1 and "NULL" in L.mcr_last_error().decode(), kw
    null_block = (ctypes.c_void_p * 10)(*[t.data_ptr() for t in blk[:7]], None, *[t.data_ptr() for t in blk[8:]])
    for kw in (dict(feats=None), dict(pointers=None), dict(eps=None), dict(pointers=null_block)):
        assert extractor(**kw) == 1 and "NULL" in L.mcr_last_error().decode(), kw
    for kw in (dict(n_blocks=-1), dict(n_blocks=5)):
        assert extractor(**kw) == 1 and "n_blocks" in L.mcr_last_error().decode(), kw
        assert L.mcr_feature_extractor_workspace_bytes(i64(N0), i64(N1), i64(Cin), i64(Cout), i64(H), i64(W), i64(kw["n_blocks"])) == 0
    for entry in (extractor, block):
        for kw in (dict(ws_bytes=64), dict(ws_ptr=ws.data_ptr() + 4, ws_bytes=ws.numel() - 4), dict(ws_ptr=None)):
            assert entry(**kw) == 1 and "workspace" in L.mcr_last_error().decode(), kw
    block_sizes = [dict(H=0), dict(W=0), dict(C=0), dict(C=513), dict(B=0), dict(B=-1), dict(B=big), dict(B=2 ** 20, C=512, H=2, W=2),
                   dict(C=512, H=2 ** 11, W=2 ** 11)]
    for kw in block_sizes:
        assert block(**kw) == 1 and L.mcr_last_error().decode().startswith("mcr_basic_block"), kw
        sizes = dict(B=N0, C=Cout, H=Hp, W=Wp)
        sizes.update(kw)
        assert L.mcr_basic_block_workspace_bytes(*[i64(sizes[k]) for k in ("B", "C", "H", "W")]) == 0, kw
    for kw in (dict(x=None), dict(y=None), dict(w2=None), dict(mean=None)):
        assert block(**kw) == 1 and "NULL" in L.mcr_last_error().decode(), kw
    assert block(y=bx) == 1                                             # in place
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (pooled, conv1, by)) and bool((ws == 0xFF).all())        # nothing was launched
    # and the same calls, well-formed, run: all-ones operands, an identity BatchNorm -- small integers, exact
    ones = model.extractor(np.ones((N0 + N1, Cin, H, W)), np.ones((Cout, Cin, 7, 7)), None, [t.cpu().numpy() for t in bn], 0.0,
                           [(np.ones((Cout, Cout, 3, 3)), [t.cpu().numpy() for t in bn], 0.0) * 2])
    assert stem() == 0
    torch.cuda.synchronize()
    assert same_bits(pooled, ones["pooled"]) and same_bits(conv1, ones["conv1"][:N0])
    assert extractor() == 0
    torch.cuda.synchronize()
    assert same_bits(pooled, ones["features"])
    pooled.fill_(-7.0)
    assert extractor(n_blocks=0, ws_ptr=None, ws_bytes=0) == 0        # no blocks: 0 bytes are needed and a NULL workspace is taken
    torch.cuda.synchronize()
    assert same_bits(pooled, ones["pooled"])
    assert L.mcr_feature_extractor_workspace_bytes(i64(N0), i64(N1), i64(Cin), i64(Cout), i64(H), i64(W), i64(0)) == 0
    assert block() == 0
    torch.cuda.synchronize()
    assert same_bits(by, model.block(np.ones((N0, Cout, Hp, Wp)), np.ones((Cout, Cout, 3, 3)), [t.cpu().numpy() for t in bn], 0.0,
                                     np.ones((Cout, Cout, 3, 3)), [t.cpu().numpy() for t in bn], 0.0)["y"])
    assert L.mcr_basic_block_workspace_bytes(i64(N0), i64(Cout), i64(Hp), i64(Wp)) >= 4 * N0 * Cout * Hp * Wp
    assert L.mcr_feature_extractor_workspace_bytes(i64(N0), i64(N1), i64(Cin), i64(Cout), i64(H), i64(W), i64(1)) >= 8 * (N0 + N1) * Cout * Hp * Wp


# ---- 6. the routes ----------------------------------------------------------------------------------------------------------------------------------
def count_calls(monkeypatch, name):
    calls, real = [], getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: calls.append((a, k)) or real(*a, **k))
    return calls


def test_adopted_extractor_routes(dev, monkeypatch):
    monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "hip")
    net = randomize_batch_norms(resnet_front(3, 64, 2), 7)
    upstream = torch.nn.Module()
    upstream.conv1, upstream.bn1, upstream.relu, upstream.maxpool, upstream.layer = net.conv1, net.bn1, net.relu, net.maxpool, net.layer1
    mirror = ManyDepth.FeatureExtractor(copy.deepcopy(net))
    x = torch.rand(2, 3, 32, 57, generator=torch.Generator().manual_seed(1)).to(dev)
    calls = count_calls(monkeypatch, "feature_extractor")
    for m in (ManyDepth.adopt_feature_extractor(upstream.to(dev).eval()), mirror.to(dev).eval()):
        assert ManyDepth.adopt_feature_extractor(m) is m                # twice: nothing changes
        del calls[:]
        with torch.no_grad():
            got = m(x)
            comp = m.layer(m.maxpool(m.relu(m.bn1(m.conv1(x)))))
            assert len(calls) == 1 and calls[0][1] == dict(want_conv1=False)
            e = model.rel(got.cpu().numpy(), comp.cpu().numpy())
            print(f"ERR adopted extractor on HIP vs its own modules (float32, device): {e:.2e}")
            assert tuple(got.shape) == (2, 64, 8, 15) and e < TOL
            assert torch.equal(copy.deepcopy(m)(x), got) and len(calls) == 2                              # survives a deep copy, still on HIP
            with torch.autocast("cuda", dtype=torch.float16):
                assert m(x).dtype == torch.float16 and len(calls) == 2                                    # autocast: the modules
            assert torch.equal(m(x.transpose(2, 3).contiguous().transpose(2, 3)), comp) and len(calls) == 2   # a strided x
        assert m(x).grad_fn is not None and len(calls) == 2             # the parameters require a gradient: the modules under autograd
        m.requires_grad_(False)
        assert torch.equal(m(x), got) and len(calls) == 3               # nothing to record: the entry, grad mode on
        assert m(x.clone().requires_grad_(True)).grad_fn is not None and len(calls) == 3
        m.train()
        with torch.no_grad():
            m(x)
        assert len(calls) == 3                                          # training mode: batch statistics, the modules
        m.eval()
        monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "composite")
        with torch.no_grad():
            m(x)
        assert len(calls) == 3
        monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "hip")

def test_adopted_depth_front(dev, monkeypatch):
    """A stand-in decoder at 32 x 64, B 2, n_alpha 2: after adopt_depth_front, in eval mode without a gradient, target and sources make
    exactly ONE extractor call; disp1..4 are within 1e-4 of the unadopted decoder's; training mode, a gradient and autocast each send
    the same call to the modules."""
    monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "hip")
    H, W, B, A = 32, 64, 2, 2
    plain = StandInDecoder(H, W, A).to(dev).eval()
    adopted = ManyDepth.adopt_depth_front(ManyDepth.adopt_depth_decoder(copy.deepcopy(plain)))
    assert ManyDepth.adopt_depth_front(adopted) is adopted
    args = [v.to(dev) if torch.is_tensor(v) else v for v in decoder_inputs(B, A, H, W)]
    calls = count_calls(monkeypatch, "feature_extractor")
    with torch.no_grad():
        want, got = plain(*args, dev), adopted(*args, device=dev)
    assert len(calls) == 1
    (x, x_more), kw = calls[0][0][:2], calls[0][1]
    assert tuple(x.shape) == (B, 3, H, W) and tuple(x_more.shape) == (B * A, 3, H, W) and kw.get("want_conv1", True)
    assert x_more.data_ptr() == args[4].data_ptr()                       # the sources as they lie in x_alpha: no concatenated copy
    e = {f"disp{k + 1}": model.rel(g.cpu().numpy(), w.cpu().numpy()) for k, (g, w) in enumerate(zip(got, want))}
    print("ERR adopted decoder (HIP front) vs the unadopted one: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert [tuple(g.shape) for g in got] == [(B, 1, H, W), (B, 1, H // 2, W // 2), (B, 1, H // 4, W // 4), (B, 1, H // 8, W // 8)]
    assert max(e.values()) < TOL
    with torch.no_grad():
        again = copy.deepcopy(adopted)(*args, device=dev)
        # (not bit for bit: the vendor library's convolutions behind the front may choose another algorithm on a later call)
        assert len(calls) == 2 and all(model.rel(a.cpu().numpy(), g.cpu().numpy()) < TOL for a, g in zip(again, got))
        with torch.autocast("cuda", dtype=torch.float16):                 # (the sweep behind the front takes float32 only: the route itself)
            assert ManyDepth.feature_extractor_route(adopted.feature_extractor, args[0], args[4].reshape(-1, 3, H, W)) == "composite"
        assert ManyDepth.feature_extractor_route(adopted.feature_extractor, args[0], args[4].reshape(-1, 3, H, W)) == "hip"
    out = adopted(*args, device=dev)                                     # the parameters require a gradient
    assert len(calls) == 2 and out[0].grad_fn is not None
    adopted.requires_grad_(False)
    adopted.feature_extractor.train()
    with torch.no_grad():
        adopted(*args, device=dev)
    assert len(calls) == 2
    adopted.eval()
    with torch.no_grad():
        adopted(*args, device=dev)
    assert len(calls) == 3
