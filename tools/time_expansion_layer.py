"""Time the expansion layers of the depth decoder at upstream's five shapes (B 1 and 4) and the decoder's tail -- the five layers chained,
the four disparity heads between them --, the fused HIP entry against upstream's op sequence (transposed convolution, ELU, nearest
resize, concatenation, reflection-padded copy, convolution, ELU: networks.ManyDepth.expansion_layer_composite) in torch on the same GPU
in the same run:

    python tools/time_expansion_layer.py [--window 0.5] [--repeats 7] [--out profiles/expansion_layer_times.json]

  forward_hip        ops.expansion_layer (mcr_expansion_layer), without a graph
  forward_composite  expansion_layer_composite under no_grad

  (Cin, Cmid, Cadd, Cout, h x w -> H x W):   expansion5 (512, 256, 256, 256, 8x15 -> 16x29)    expansion4 (256, 128, 128, 128, 16x29 -> 32x57)
  expansion3 (128, 64, 64, 64, 32x57 -> 64x114)   expansion2 (64, 32, 64, 32, 64x114 -> 128x228)   expansion1 (32, 16, 3, 16, 128x228 -> 256x456)

The decoder row runs expansion5 .. 1 on each other's results with the skip features as x_add, and disp4 .. disp1 on the results of
expansion4 .. 1; the heads are the fused ops.disparity_head in the HIP route and disparity_head_composite in the other.

The method is that of tools/time_disparity_head.py: host clock between two device synchronisations over a window of calls, the same
inputs every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about --window seconds; one
repeat times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the repeats, the
distance between the two routes' results, and `hip_faster_than_composite_intervals_apart`: the HIP route's whole interval lies below the
composite's whole interval.  `hip_is_default_by_the_rule` is true only if that holds in every single-layer row of both batch sizes.
Reads nothing outside the repository."""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402

# name -> (Cin, Cmid, Cadd, Cout, (h, w), (H, W)), in the order the decoder runs them
SHAPES = {"expansion5": (512, 256, 256, 256, (8, 15), (16, 29)), "expansion4": (256, 128, 128, 128, (16, 29), (32, 57)),
          "expansion3": (128, 64, 64, 64, (32, 57), (64, 114)), "expansion2": (64, 32, 64, 32, (64, 114), (128, 228)),
          "expansion1": (32, 16, 3, 16, (128, 228), (256, 456))}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def uniform(gen, bound, *shape):
    return (torch.rand(*shape, generator=gen) * 2 - 1) * bound


def layer(B, Cin, Cmid, Cadd, Cout, hw, HW, dev, gen):
    """Features of unit size, parameters of upstream's initialisation ranges (torch's defaults for the two convolutions), a head."""
    bu, bi, bh = 1.0 / math.sqrt(9 * Cmid), 1.0 / math.sqrt(9 * (Cmid + Cadd)), 1.0 / math.sqrt(9 * Cout)
    v = dict(x=torch.randn(B, Cin, *hw, generator=gen), x_add=torch.randn(B, Cadd, *HW, generator=gen),
             up_weight=uniform(gen, bu, Cin, Cmid, 3, 3), up_bias=uniform(gen, bu, Cmid), i_weight=uniform(gen, bi, Cout, Cmid + Cadd, 3, 3),
             i_bias=uniform(gen, bi, Cout), head_weight=uniform(gen, bh, 1, Cout, 3, 3), head_bias=uniform(gen, bh, 1))
    v = {k: t.to(dev) for k, t in v.items()}
    v["output_size"] = HW
    return v


def args_of(v, x=None):
    return (v["x"] if x is None else x, v["x_add"], v["up_weight"], v["up_bias"], v["i_weight"], v["i_bias"], v["output_size"])


def routes_of(layers, chained):
    """layers: one, or the five in the decoder's order with `chained`: each runs on the one before and a head follows all but the first."""
    def run(expansion, head):
        outs, x = [], None
        for k, v in enumerate(layers):
            x = expansion(*args_of(v, x if chained else None))
            outs.append(head(x, v["head_weight"], v["head_bias"]) if chained and k else x)
        return outs

    def forward_hip():
        return run(ops.expansion_layer, ops.disparity_head)

    def forward_composite():
        with torch.no_grad():
            return run(ManyDepth.expansion_layer_composite, ManyDepth.disparity_head_composite)

    return {"forward_hip": forward_hip, "forward_composite": forward_composite}


def far(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def measure(layers, window, repeats, chained=False):
    routes = routes_of(layers, chained)
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(window / (timed(fn, 5) * 1e-3))))
    dist = max(far(a, b) for a, b in zip(routes["forward_hip"](), routes["forward_composite"]()))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expansion_layer_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_expansion_layer: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    res = {"shapes": {k: [*v[:4], list(v[4]), list(v[5])] for k, v in SHAPES.items()}, "shape_columns": "Cin, Cmid, Cadd, Cout, [h, w], [H, W]",
           "device": torch.cuda.get_device_name(0), "window_s": a.window, "repeats": a.repeats, "clock": "host, between device synchronisations"}
    apart = []
    for B in (1, 4):
        gen = torch.Generator().manual_seed(17)
        layers = {k: layer(B, *s, dev, gen) for k, s in SHAPES.items()}
        rows = {k: measure([v], a.window, a.repeats) for k, v in layers.items()}
        apart += [r["hip_faster_than_composite_intervals_apart"] for r in rows.values()]
        rows["decoder_tail_five_layers_four_heads"] = measure(list(layers.values()), a.window, a.repeats, chained=True)
        res[f"B{B}"] = rows
        for k, r in rows.items():
            print(f"B{B} {k}: " + "  ".join(f"{n} {r[n + '_ms']['median']:.4f}" for n in ("forward_hip", "forward_composite"))
                  + f"  rel {r['hip_vs_composite_rel']:.1e}  apart {r['hip_faster_than_composite_intervals_apart']}", flush=True)
    res["hip_is_default_by_the_rule"] = all(apart)
    print(f"hip_is_default_by_the_rule {res['hip_is_default_by_the_rule']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
