"""Time the disparity heads of the depth decoder at upstream's four shapes ([B,16,256,456], [B,32,128,228], [B,64,64,114], [B,128,32,57];
B 1 and 4) and the four heads together, the fused HIP entries against upstream's op sequence (reflection-padded copy, library convolution,
sigmoid: networks.ManyDepth.disparity_head_composite) in torch on the same GPU in the same run:

    python tools/time_disparity_head.py [--window 0.5] [--repeats 7] [--out profiles/disparity_head_times.json]

  forward_hip        ops.disparity_head (mcr_disparity_head), without a graph
  forward_composite  disparity_head_composite under no_grad
  step_hip           DisparityHeadFunction forward, then the backward of sum(g * y) into x, weight and bias (mcr_disparity_head_backward);
                     the tool sets MCR_DISPARITY_HEAD_BWD=hip for itself -- the package's default backward is the composite -- checks that
                     the mode took, and records it in the JSON
  step_composite     the composite under autograd, forward and backward

The method is that of tools/time_disparity_scales.py: host clock between two device synchronisations over a window of calls, the same
inputs every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about --window seconds; one
repeat times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the repeats, the
distance between the two routes' results, and `hip_faster_than_composite_intervals_apart`: the HIP route's whole interval lies below the
composite's whole interval.  Reads nothing outside the repository."""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["MCR_DISPARITY_HEAD_BWD"] = "hip"            # what step_hip times is the HIP backward, whatever the caller's environment holds

from macarons_amd import ops  # noqa: E402
from macarons_amd.autograd import DisparityHeadFunction, disparity_head_backward_mode  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402

SHAPES = {"scale1": (16, 256, 456), "scale2": (32, 128, 228), "scale3": (64, 64, 114), "scale4": (128, 32, 57)}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def head(B, C, Hs, Ws, dev, gen):
    """Features of unit size, weights of upstream's initialisation range, a gradient of the size a mean over the map hands back."""
    x = torch.randn(B, C, Hs, Ws, generator=gen).to(dev)
    bound = 1.0 / math.sqrt(9 * C)
    w = ((torch.rand(1, C, 3, 3, generator=gen) * 2 - 1) * bound).to(dev)
    b = ((torch.rand(1, generator=gen) * 2 - 1) * bound).to(dev)
    g = (torch.randn(B, 1, Hs, Ws, generator=gen) / (Hs * Ws)).to(dev)
    return x, w, b, g


def routes_of(heads):
    def leaves():
        return [[v.detach().requires_grad_(True) for v in (x, w, b)] for x, w, b, _ in heads]

    def forward_hip():
        return [ops.disparity_head(x, w, b) for x, w, b, _ in heads]

    def forward_composite():
        with torch.no_grad():
            return [ManyDepth.disparity_head_composite(x, w, b) for x, w, b, _ in heads]

    def step(fn):
        ls = leaves()
        loss = sum((fn(*l) * h[3]).sum() for l, h in zip(ls, heads))
        return torch.autograd.grad(loss, [v for l in ls for v in l])

    return {"forward_hip": forward_hip, "forward_composite": forward_composite,
            "step_hip": lambda: step(DisparityHeadFunction.apply), "step_composite": lambda: step(ManyDepth.disparity_head_composite)}


def far(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def measure(heads, window, repeats):
    routes = routes_of(heads)
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(window / (timed(fn, 5) * 1e-3))))
    dist = {"y": max(far(a, b) for a, b in zip(routes["forward_hip"](), routes["forward_composite"]())),
            "step_grads": max(far(a, b) for a, b in zip(routes["step_hip"](), routes["step_composite"]()))}
    runs = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            runs[k].append(timed(fn, iters[k]))
    res = {"iters": iters, "hip_vs_composite_rel": dist}
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["hip_faster_than_composite_intervals_apart"] = {k: res[k + "_hip_ms"]["max"] < res[k + "_composite_ms"]["min"] for k in ("forward", "step")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disparity_head_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_disparity_head: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    if disparity_head_backward_mode() != "hip":
        raise SystemExit("time_disparity_head: the backward mode is not 'hip'; step_hip would time another route")
    res = {"backward_mode_of_step_hip": disparity_head_backward_mode(), "shapes": {k: list(v) for k, v in SHAPES.items()}, "device": torch.cuda.get_device_name(0), "window_s": a.window,
           "repeats": a.repeats, "clock": "host, between device synchronisations"}
    for B in (1, 4):
        gen = torch.Generator().manual_seed(13)
        heads = {k: head(B, *s, dev, gen) for k, s in SHAPES.items()}
        rows = {k: measure([h], a.window, a.repeats) for k, h in heads.items()}
        rows["four_heads"] = measure(list(heads.values()), a.window, a.repeats)
        res[f"B{B}"] = rows
        for k, r in rows.items():
            print(f"B{B} {k}: " + "  ".join(f"{n} {r[n + '_ms']['median']:.4f}" for n in ("forward_hip", "forward_composite", "step_hip", "step_composite"))
                  + f"  apart {r['hip_faster_than_composite_intervals_apart']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
