"""The feature extractor without a GPU: the independent fp64 model (tests/_feature_extractor_model.py) against torch's own convolution,
BatchNorm and pooling and against the composites of networks.ManyDepth, in float64 on the CPU to 1e-12; the mirrors' state-dict names;
every refusal of adopt_feature_extractor and adopt_depth_front; the route for everything the entry does not take; a stand-in decoder
after adopt_depth_front against the unadopted one, bit for bit; the committed golden's own bound; the argument checks of the ops.
"""
import copy
import os
import pickle
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _feature_extractor_model as model                               # noqa: E402
from _depth_front_stand_in import MeanBuilder, StandInDecoder, decoder_inputs, randomize_batch_norms, resnet_front   # noqa: E402

from macarons_amd import ops                                           # noqa: E402
from macarons_amd.networks import ManyDepth                            # noqa: E402

TIGHT = 1e-12


def t64(v):
    if isinstance(v, tuple):
        return tuple(t64(u) for u in v)
    return None if v is None else torch.as_tensor(np.asarray(v, np.float64))


def torch_stem(images, weight, bias, bn, eps):
    w, b, m, v = bn
    conv1 = F.relu(F.batch_norm(F.conv2d(images, weight, bias, stride=2, padding=3), m, v, w, b, False, 0.0, eps))
    return F.max_pool2d(conv1, 3, 2, 1), conv1


# ---- the model against torch and the composites -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", model.STEM_TAGS)
def test_stem_model_matches_torch_and_the_composite(tag):
    c = model.make_stem_inputs(tag)
    images = model.images_of(c)
    want = model.stem(images, c["weight"], c["bias"], c["bn"], c["eps"])
    N0, N1, Cin, Cout, (H, W) = model.STEM_CASES[tag]["shape"]
    Hc, Wc, Hp, Wp = ops.resnet_stem_sizes(H, W)
    assert want["conv1"].shape == (N0 + N1, Cout, Hc, Wc) and want["pooled"].shape == (N0 + N1, Cout, Hp, Wp)
    args = (t64(images), t64(c["weight"]), t64(c["bias"]), t64(c["bn"]), c["eps"])
    for name, (pooled, conv1) in (("torch", torch_stem(*args)), ("composite", ManyDepth.resnet_stem_composite(*args))):
        e = (model.rel(conv1.numpy(), want["conv1"]), model.rel(pooled.numpy(), want["pooled"]))
        print(f"ERR stem case {tag}, model vs {name} (fp64): conv1 {e[0]:.1e} pooled {e[1]:.1e}")
        assert max(e) < TIGHT


@pytest.mark.parametrize("tag", model.BLOCK_TAGS)
def test_block_model_matches_torch_and_the_composite(tag):
    c = model.make_block_inputs(tag)
    want = model.block(c["x"], *c["block"])
    x, (w1, bn1, eps1, w2, bn2, eps2) = t64(c["x"]), (t64(v) if not isinstance(v, float) else v for v in c["block"])
    t = F.relu(F.batch_norm(F.conv2d(x, w1, None, 1, 1), bn1[2], bn1[3], bn1[0], bn1[1], False, 0.0, eps1))
    y = F.relu(F.batch_norm(F.conv2d(t, w2, None, 1, 1), bn2[2], bn2[3], bn2[0], bn2[1], False, 0.0, eps2) + x)
    comp = ManyDepth.basic_block_composite(x, w1, bn1, eps1, w2, bn2, eps2)
    e = (model.rel(t.numpy(), want["t"]), model.rel(y.numpy(), want["y"]), model.rel(comp.numpy(), want["y"]))
    print(f"ERR block case {tag}, model vs torch (fp64): t {e[0]:.1e} y {e[1]:.1e}; vs the composite: y {e[2]:.1e}")
    assert max(e) < TIGHT


def test_extractor_model_matches_the_composite():
    c = model.make_extractor_inputs()
    images = model.images_of(c)
    want = model.extractor(images, c["weight"], c["bias"], c["bn"], c["eps"], c["blocks"])
    blocks = [tuple(v if isinstance(v, float) else t64(v) for v in blk) for blk in c["blocks"]]
    feats, conv1 = ManyDepth.feature_extractor_composite(t64(images), t64(c["weight"]), None, t64(c["bn"]), c["eps"], blocks)
    e = (model.rel(feats.numpy(), want["features"]), model.rel(conv1.numpy(), want["conv1"]))
    print(f"ERR extractor, model vs the composite (fp64): features {e[0]:.1e} conv1 {e[1]:.1e}")
    assert feats.shape == (3, 64, 8, 15) and conv1.shape == (3, 64, 16, 29) and max(e) < TIGHT


def test_exact_operands_have_headroom_and_both_branches():
    """What the GPU test relies on, checked where no GPU is needed: the bounds, and the signs the cases were drawn for."""
    all_negative = 0
    for tag in model.STEM_TAGS:
        e = model.make_stem_exact(tag)
        s = model.stem(model.images_of(e), e["weight"], e["bias"], e["bn"], 0.0)
        assert model.stem_headroom(e) < 2 ** 24 and model.is_fp32(s["conv1"]) and model.is_fp32(s["pooled"])
        if tag != "a":
            assert (s["pre"] > 0).any() and (s["pre"] < 0).any()
        all_negative += int((model.max_pool(s["pre"]) < 0).sum())
    assert all_negative > 0
    for tag in "abcd":                                                  # (e and f: in the GPU test, which computes them anyway)
        e = model.make_block_exact(tag)
        r = model.block(e["x"], *e["block"])
        assert max(model.block_headroom(e)) < 2 ** 24 and model.is_fp32(r["t"]) and model.is_fp32(r["y"])
        if tag != "a":
            assert (r["t"] > 0).any() and (r["y"] > 0).any() and (r["y"] == 0).any()
            assert ((r["pre"] < 0) & (r["pre"] + e["x"] > 0)).any()     # the residual changes the sign of some outputs
    e = model.make_extractor_exact()
    assert max(model.extractor_headroom(e)) < 2 ** 24


def test_golden_is_close_to_the_model():
    for tag in model.GOLDEN_TAGS:
        g = model.load_golden(tag)
        want = model.extractor(model.images_of(g), g["weight"], g["bias"], g["bn"], g["eps"], g["blocks"])["features"]
        d = model.rel(g["features"], want)
        print(f"ERR golden case {tag} vs model: features {d:.1e} (stored {g['distance']:.1e})")
        assert g["distance"] < 1e-5 and abs(d - g["distance"]) < 1e-9
        seeded = model.make_golden_inputs(tag)
        assert np.array_equal(seeded["weight"], g["weight"]) and len(seeded["blocks"]) == len(g["blocks"])


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------------
def test_mirror_state_dict_names():
    block = ManyDepth.BasicBlock(4, 4)
    bn = ["bias", "num_batches_tracked", "running_mean", "running_var", "weight"]
    assert sorted(block.state_dict()) == sorted(["conv1.weight", "conv2.weight"] + [f"bn{i}.{k}" for i in (1, 2) for k in bn])
    down = ManyDepth.BasicBlock(4, 8, stride=2, downsample=nn.Sequential(nn.Conv2d(4, 8, 1, 2, bias=False), nn.BatchNorm2d(8)))
    assert {"downsample.0.weight", "downsample.1.running_mean"} <= set(down.state_dict()) and down.stride == 2
    assert [n for n, _ in block.named_children()] == ["conv1", "bn1", "relu", "conv2", "bn2"]
    fe = ManyDepth.FeatureExtractor(resnet_front(3, 16, 2))
    assert [n for n, _ in fe.named_children()] == ["conv1", "bn1", "relu", "maxpool", "layer"]
    z = np.load(model.GOLDEN)
    assert sorted(fe.state_dict()) == list(z["state_dict_names"])       # upstream's own FeatureExtractor over the same stand-in
    assert [",".join(str(n) for n in fe.state_dict()[k].shape) for k in sorted(fe.state_dict())] == list(z["state_dict_shapes"])
    with torch.no_grad():                                               # stride and downsample: the module sequence
        assert down.eval()(torch.rand(1, 4, 6, 6)).shape == (1, 8, 3, 3)


# ---- adopt: refusals --------------------------------------------------------------------------------------------------------------------------
def upstream_like(**changes):
    """An extractor as upstream's class leaves it (a plain module with the five attributes), one fact changed."""
    net = resnet_front(3, 8, 2)
    for k, v in changes.items():
        target, name = net, k
        if "." in k:
            head, name = k.rsplit(".", 1)
            for part in head.split("."):
                target = target[int(part)] if part.isdigit() else getattr(target, part)
        setattr(target, name, v)
    fe = nn.Module()
    fe.conv1, fe.bn1, fe.relu, fe.maxpool, fe.layer = net.conv1, net.bn1, net.relu, net.maxpool, net.layer1
    return fe


WRONG = [
    ("conv1.kernel_size", {"conv1": nn.Conv2d(3, 8, 5, 2, 3, bias=False)}),
    ("conv1.stride", {"conv1": nn.Conv2d(3, 8, 7, 1, 3, bias=False)}),
    ("conv1.padding", {"conv1": nn.Conv2d(3, 8, 7, 2, 2, bias=False)}),
    ("conv1.padding_mode", {"conv1": nn.Conv2d(3, 8, 7, 2, 3, bias=False, padding_mode="reflect")}),
    ("conv1.dilation", {"conv1": nn.Conv2d(3, 8, 7, 2, 3, dilation=2, bias=False)}),
    ("conv1.groups", {"conv1": nn.Conv2d(4, 8, 7, 2, 3, groups=2, bias=False)}),
    ("bn1.weight", {"bn1": nn.BatchNorm2d(8, affine=False)}),
    ("bn1.running_mean", {"bn1": nn.BatchNorm2d(8, track_running_stats=False)}),
    ("relu", {"relu": nn.ELU()}),
    ("maxpool.kernel_size", {"maxpool": nn.MaxPool2d(2, 2, 1)}),
    ("maxpool.stride", {"maxpool": nn.MaxPool2d(3, 1, 1)}),
    ("maxpool.padding", {"maxpool": nn.MaxPool2d(3, 2, 0)}),
    ("maxpool.ceil_mode", {"maxpool": nn.MaxPool2d(3, 2, 1, ceil_mode=True)}),
    (r"layer\[1\].conv1.stride", {"layer1.1.conv1": nn.Conv2d(8, 8, 3, 2, 1, bias=False)}),
    (r"layer\[0\].conv2.bias", {"layer1.0.conv2": nn.Conv2d(8, 8, 3, 1, 1, bias=True)}),
    (r"layer\[0\].conv1.kernel_size", {"layer1.0.conv1": nn.Conv2d(8, 8, 1, 1, 1, bias=False)}),
    (r"layer\[1\].downsample", {"layer1.1.downsample": nn.Sequential(nn.Conv2d(8, 8, 1))}),
    (r"layer\[0\].stride", {"layer1.0.stride": 2}),
    (r"layer\[1\].bn2.running_var", {"layer1.1.bn2": nn.BatchNorm2d(8, track_running_stats=False)}),
    ("layer is not a sequence", {"layer1": nn.Sequential(*[ManyDepth.BasicBlock(8, 8) for _ in range(5)])}),
    (r"layer\[0\] lacks", {"layer1": nn.Sequential(nn.Conv2d(8, 8, 3, 1, 1))}),
]


@pytest.mark.parametrize("named,change", WRONG, ids=[w[0] for w in WRONG])
def test_adopt_feature_extractor_names_the_wrong_fact(named, change):
    fe = upstream_like(**change)
    with pytest.raises(TypeError, match="adopt_feature_extractor.*" + named):
        ManyDepth.adopt_feature_extractor(fe)
    assert "forward" not in vars(fe)


def test_adopt_feature_extractor_names_every_wrong_fact_and_refuses_non_extractors():
    fe = upstream_like(conv1=nn.Conv2d(3, 8, 5, 1, 3, bias=False), maxpool=nn.MaxPool2d(3, 2, 1, ceil_mode=True))
    with pytest.raises(TypeError) as err:
        ManyDepth.adopt_feature_extractor(fe)
    assert all(s in str(err.value) for s in ("conv1.kernel_size", "conv1.stride", "maxpool.ceil_mode"))
    for other in (nn.Linear(2, 2), nn.Conv2d(2, 2, 3), object()):
        with pytest.raises(TypeError, match="adopt_feature_extractor: not a FeatureExtractor"):
            ManyDepth.adopt_feature_extractor(other)


def test_adopt_feature_extractor_and_depth_front():
    fe = upstream_like().eval()
    assert ManyDepth.adopt_feature_extractor(fe) is fe and ManyDepth.adopt_feature_extractor(fe) is fe
    assert isinstance(vars(fe)["forward"], ManyDepth._AdoptedExtractorForward)
    assert ManyDepth.adopt_feature_extractor(upstream_like(conv1=nn.Conv2d(6, 8, 7, 2, 3, bias=True))) is not None     # the pose decoder's stem
    x = torch.rand(2, 3, 9, 11)
    with torch.no_grad():
        want = fe.layer(fe.maxpool(fe.relu(fe.bn1(fe.conv1(x)))))
        for m in (fe, copy.deepcopy(fe), pickle.loads(pickle.dumps(fe))):
            assert torch.equal(m(x), want)
    dec = StandInDecoder(builder=MeanBuilder(64))
    for name in ManyDepth._DEPTH_FRONT_ATTRIBUTES:
        partial = copy.copy(dec)
        partial._modules, partial.__dict__ = dict(dec._modules), dict(dec.__dict__)
        partial._modules.pop(name, None), partial.__dict__.pop(name, None)
        with pytest.raises(TypeError, match="adopt_depth_front.*" + name):
            ManyDepth.adopt_depth_front(partial)
    bad = StandInDecoder(builder=MeanBuilder(64))
    bad.feature_extractor.maxpool = nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    with pytest.raises(TypeError, match="adopt_feature_extractor.*maxpool.ceil_mode"):
        ManyDepth.adopt_depth_front(bad)
    assert "forward" not in vars(bad)
    with pytest.raises(TypeError, match="adopt_depth_front"):
        ManyDepth.adopt_depth_front(nn.Linear(2, 2))


# ---- the route --------------------------------------------------------------------------------------------------------------------------------
def test_route_is_the_composite_for_everything_the_entry_does_not_take(monkeypatch):
    fe = randomize_batch_norms(ManyDepth.FeatureExtractor(resnet_front(3, 8, 2)), 1).eval().requires_grad_(False)
    x = torch.rand(1, 3, 9, 11)
    assert ManyDepth.FEATURE_EXTRACTOR_DEFAULT in ("hip", "composite")
    monkeypatch.delenv("MCR_FEATURE_EXTRACTOR", raising=False)
    assert ManyDepth.feature_extractor_mode() == ManyDepth.FEATURE_EXTRACTOR_DEFAULT
    monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "composite")
    assert ManyDepth.feature_extractor_mode() == "composite" and ManyDepth.feature_extractor_route(fe, x) == "composite"
    monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "hip")
    assert ManyDepth.feature_extractor_mode() == "hip"
    monkeypatch.setattr(ops, "feature_extractor", lambda *a, **k: pytest.fail("the entry was called"))
    monkeypatch.setattr(ops, "basic_block", lambda *a, **k: pytest.fail("the entry was called"))
    assert ManyDepth.feature_extractor_route(fe, x) == "composite"       # CPU tensors
    assert ManyDepth.feature_extractor_route(fe, x, x) == "composite"
    with torch.no_grad():
        want = fe.layer(fe.maxpool(fe.relu(fe.bn1(fe.conv1(x)))))
        assert torch.equal(fe(x), want)
    # the other reasons, each on tensors that claim to be on a HIP device (the device check is the only one a CPU machine cannot pass)
    monkeypatch.setattr(ManyDepth, "_is_hip_tensor", lambda t: True)
    assert ManyDepth.feature_extractor_route(fe, x) == "hip" and ManyDepth.feature_extractor_route(fe, x, torch.rand(2, 3, 9, 11)) == "hip"
    fe.train()
    assert ManyDepth.feature_extractor_route(fe, x) == "composite"
    fe.eval()
    fe.layer[1].bn2.train()
    assert ManyDepth.feature_extractor_route(fe, x) == "composite"       # one BatchNorm of a block in training mode
    fe.eval()
    assert ManyDepth.feature_extractor_route(fe, x.clone().requires_grad_(True)) == "composite"
    fe.layer[0].conv2.weight.requires_grad_(True)
    assert ManyDepth.feature_extractor_route(fe, x) == "composite"
    with torch.no_grad():
        assert ManyDepth.feature_extractor_route(fe, x) == "hip"         # nothing is recorded
    fe.requires_grad_(False)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert ManyDepth.feature_extractor_route(fe, x) == "composite"
    assert ManyDepth.feature_extractor_route(fe, x.double()) == "composite"
    assert ManyDepth.feature_extractor_route(fe, x.transpose(2, 3).contiguous().transpose(2, 3)) == "composite"
    assert ManyDepth.feature_extractor_route(fe, x, torch.rand(2, 3, 9, 12)) == "composite"               # another image size
    assert ManyDepth.feature_extractor_route(fe, torch.rand(1, 4, 9, 11)) == "composite"
    wide = ManyDepth.FeatureExtractor(resnet_front(3, 65, 0)).eval().requires_grad_(False)
    assert ManyDepth.feature_extractor_route(wide, x) == "composite"     # beyond the entry's 64 output channels
    strided = ManyDepth.FeatureExtractor(resnet_front(3, 8, 1)).eval().requires_grad_(False)
    strided.layer[0].stride = 2
    assert ManyDepth.feature_extractor_route(strided, x) == "composite"
    assert ManyDepth.feature_extractor_route(fe, x) == "hip"


def test_adopted_decoder_equals_the_unadopted_one_on_the_cpu(monkeypatch):
    monkeypatch.setenv("MCR_FEATURE_EXTRACTOR", "hip")                    # even so: CPU tensors take upstream's sequence
    H, W, B, A = 32, 64, 1, 2
    plain = StandInDecoder(H, W, A, builder=MeanBuilder(64))
    adopted = ManyDepth.adopt_depth_front(copy.deepcopy(plain))
    assert ManyDepth.adopt_depth_front(adopted) is adopted and isinstance(vars(adopted)["forward"], ManyDepth._AdoptedDepthForward)
    assert isinstance(vars(adopted.feature_extractor)["forward"], ManyDepth._AdoptedExtractorForward)
    args = decoder_inputs(B, A, H, W)
    for mode in ("eval", "train"):
        getattr(plain, mode)(), getattr(adopted, mode)()
        with torch.no_grad():
            want, got = plain(*args, "cpu"), adopted(*args, device="cpu")
        assert [tuple(d.shape) for d in got] == [(B, 1, H, W), (B, 1, H // 2, W // 2), (B, 1, H // 4, W // 4), (B, 1, H // 8, W // 8)]
        assert all(torch.equal(g, w) for g, w in zip(got, want)), mode
    # training mode updated the running statistics of both in the same way: x first, then the sources
    assert torch.equal(plain.feature_extractor.bn1.running_mean, adopted.feature_extractor.bn1.running_mean)
    got = copy.deepcopy(adopted).eval()
    with torch.no_grad():
        assert all(torch.equal(g, w) for g, w in zip(got(*args, "cpu"), adopted.eval()(*args, "cpu")))
    assert got.feature_extractor.forward.extractor is got.feature_extractor and got.forward.decoder is got


# ---- ops: the argument checks -------------------------------------------------------------------------------------------------------------------
def test_ops_argument_checks(monkeypatch):
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("an argument check let a call through to the library"))
    c = model.make_stem_inputs("b")
    x, x_more, w = (torch.as_tensor(c[k]) for k in ("x", "x_more", "weight"))
    bn = tuple(torch.as_tensor(v) for v in c["bn"])
    bad = [dict(x=None, x_more=None), dict(x=x[0]), dict(x_more=x_more[:, :2]), dict(weight=w[:, :, :5]), dict(weight=w[:, :2]),
           dict(bias=torch.zeros(4)), dict(bn=bn[:3]), dict(bn=(bn[0][:3],) + bn[1:]), dict(x=torch.zeros(1, 9, 7, 9), x_more=None, weight=torch.zeros(5, 9, 7, 7)),
           dict(weight=torch.zeros(65, 3, 7, 7))]
    for kw in bad:
        args = dict(x=x, x_more=x_more, weight=w, bias=None, bn=bn)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.resnet_stem(args["x"], args["x_more"], args["weight"], args["bias"], args["bn"], 1e-5)
        with pytest.raises(ValueError):
            ops.feature_extractor(args["x"], args["x_more"], args["weight"], args["bias"], args["bn"], 1e-5, [])
    b = model.make_block_inputs("b")
    bx = torch.as_tensor(b["x"])
    w1, bn1, e1, w2, bn2, e2 = (v if isinstance(v, float) else tuple(torch.as_tensor(u) for u in v) if isinstance(v, tuple) else torch.as_tensor(v)
                                for v in b["block"])
    for args in ((bx[0], w1, bn1, e1, w2, bn2, e2), (bx, w1[:2], bn1, e1, w2, bn2, e2), (bx, w1, bn1, e1, w2[:, :, :2], bn2, e2),
                 (bx, w1, bn1[:2], e1, w2, bn2, e2), (bx, w1, bn1, e1, w2, (bn2[0][:1],) + bn2[1:], e2), (torch.zeros(1, 513, 2, 2), w1, bn1, e1, w2, bn2, e2)):
        with pytest.raises(ValueError):
            ops.basic_block(*args)
    with pytest.raises(ValueError, match="at most 4"):
        ops.feature_extractor(x, x_more, w, None, bn, 1e-5, [None] * 5)
    with pytest.raises(ValueError, match=r"blocks\[0\]"):
        ops.feature_extractor(x, x_more, w, None, bn, 1e-5, [(w1, bn1, e1, w2, bn2, e2)])        # 3 channels after a 5-channel stem
    assert ops.resnet_stem_sizes(256, 456) == (128, 228, 64, 114) and ops.resnet_stem_sizes(1, 1) == (1, 1, 1, 1)
