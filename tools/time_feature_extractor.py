"""Time the front of the depth encoder -- the 7x7 / 2 convolution, eval-mode BatchNorm, ReLU, the 3x3 / 2 max-pool and the two basic blocks of
layer1 -- at upstream's size (256 x 456 images, n_alpha 2, B 1 and 4), the fused HIP entries against upstream's op sequence in torch on the
same GPU in the same run:

    python tools/time_feature_extractor.py [--window 0.5] [--repeats 7] [--out profiles/feature_extractor_times.json]

  stem             ops.resnet_stem on the B target and 2 B source images (one launch) against resnet_stem_composite on each operand
  block            ops.basic_block at [3 B, 64, 64, 114] (two launches) against basic_block_composite
  whole_extractor  an upstream-like extractor through the adopted decoder's front (ManyDepth.extractor_front, the route included) under
                   MCR_FEATURE_EXTRACTOR=hip -- one ops.feature_extractor call for target and sources, conv1 kept for the target (five
                   launches) -- against upstream's piecewise sequence of modules, two calls (target, then sources), under no_grad

The extractor is made of torch's own modules and of a basic block written out here from them, so that no part of the baseline can take
another route than torch's.  Neither route of a row runs anything the other does not: the HIP stem returns one pooled map for target and
sources, the torch stem two, and they are cut to the same form only when they are compared, outside the timed windows.

The method is that of tools/time_expansion_layer.py: host clock between two device synchronisations over a window of calls, the same inputs
every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about --window seconds; one repeat
times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the repeats, the distance
between the two routes' results, and `hip_faster_than_composite_intervals_apart`: the HIP route's whole interval lies below the composite's
whole interval.  `hip_is_default_by_the_rule` is true only if that holds in the whole_extractor row of both batch sizes.
Reads nothing outside the repository."""
import argparse
import json
import math
import os
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402

H, W, N_ALPHA, C = 256, 456, 2, 64


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


class TorchBlock(nn.Module):
    """torchvision's BasicBlock without stride or downsample, from torch's modules alone."""

    def __init__(self, planes):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.downsample, self.stride = None, 1

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        return self.relu(self.bn2(self.conv2(out)) + x)


def extractor(dev, gen):
    """An extractor as upstream's class leaves it: torch's modules with torch's initial weights, BatchNorms away from the identity, eval."""
    net = nn.Module()
    net.conv1 = nn.Conv2d(3, C, kernel_size=7, stride=2, padding=3, bias=False)
    net.bn1, net.relu, net.maxpool = nn.BatchNorm2d(C), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    net.layer = nn.Sequential(TorchBlock(C), TorchBlock(C))
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(C, generator=gen) * 0.2), m.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
                m.weight.copy_(torch.rand(C, generator=gen) + 0.5), m.bias.copy_(torch.randn(C, generator=gen) * 0.2)
    return net.to(dev).eval().requires_grad_(False)


def rows_of(B, dev, gen):
    fe = extractor(dev, gen)
    x = torch.rand(B, 3, H, W, generator=gen).to(dev)
    x_alpha = torch.rand(B, N_ALPHA, 3, H, W, generator=gen).to(dev)
    sources = x_alpha.reshape(-1, 3, H, W)
    weight, bias, bn, eps, blocks = ManyDepth._extractor_operands(fe)
    y = torch.rand(B * (1 + N_ALPHA), C, H // 4, W // 4, generator=gen).to(dev)

    def stem_hip():
        return ops.resnet_stem(x, sources, weight, bias, bn, eps)

    def stem_composite():
        with torch.no_grad():
            pooled, conv1 = ManyDepth.resnet_stem_composite(x, weight, bias, bn, eps)
            return pooled, ManyDepth.resnet_stem_composite(sources, weight, bias, bn, eps)[0], conv1

    def stem_form(out):                                  # (pooled of both, conv1) -> the composite's three
        return out[0][:B], out[0][B:], out[1]

    def block_hip():
        return (ops.basic_block(y, *blocks[0]),)

    def block_composite():
        with torch.no_grad():
            return (ManyDepth.basic_block_composite(y, *blocks[0]),)

    assert ManyDepth.feature_extractor_route(fe, x, sources) == "hip"

    def whole_hip():
        return ManyDepth.extractor_front(fe, x, sources)

    def whole_composite():
        with torch.no_grad():
            layer1, conv1 = ManyDepth._extractor_pieces(fe, x)
            return layer1, ManyDepth._extractor_pieces(fe, sources)[0], conv1

    same = lambda out: out                               # noqa: E731
    return {"stem": (stem_hip, stem_composite, stem_form), "block": (block_hip, block_composite, same),
            "whole_extractor": (whole_hip, whole_composite, same)}


def far(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def measure(hip, composite, form, window, repeats):
    routes = {"forward_hip": hip, "forward_composite": composite}
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(window / (timed(fn, 5) * 1e-3))))
    dist = max(far(a, b) for a, b in zip(form(hip()), composite()))
    runs = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            runs[k].append(timed(fn, iters[k]))
    res = {"iters": iters, "hip_vs_composite_rel": dist}
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["hip_faster_than_composite_intervals_apart"] = res["forward_hip_ms"]["max"] < res["forward_composite_ms"]["min"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_extractor_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_feature_extractor: no HIP device; a time is taken on the GPU or not at all")
    os.environ["MCR_FEATURE_EXTRACTOR"] = "hip"
    dev = torch.device("cuda:0")
    res = {"images": [3, H, W], "n_alpha": N_ALPHA, "channels": C, "blocks": 2, "device": torch.cuda.get_device_name(0), "window_s": a.window,
           "repeats": a.repeats, "clock": "host, between device synchronisations"}
    apart = []
    for B in (1, 4):
        rows = {k: measure(*fns, a.window, a.repeats) for k, fns in rows_of(B, dev, torch.Generator().manual_seed(17)).items()}
        apart.append(rows["whole_extractor"]["hip_faster_than_composite_intervals_apart"])
        res[f"B{B}"] = rows
        for k, r in rows.items():
            print(f"B{B} {k}: " + "  ".join(f"{n} {r[n + '_ms']['median']:.4f} [{r[n + '_ms']['min']:.4f}, {r[n + '_ms']['max']:.4f}]"
                                            for n in ("forward_hip", "forward_composite"))
                  + f"  rel {r['hip_vs_composite_rel']:.1e}  apart {r['hip_faster_than_composite_intervals_apart']}", flush=True)
    res["hip_is_default_by_the_rule"] = all(apart)
    print(f"hip_is_default_by_the_rule {res['hip_is_default_by_the_rule']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
