"""Time the backward of the decoder's expansion layers at upstream's five shapes (B 1 and 4) and a training step's pass through the
decoder's tail -- the five layers chained, the four disparity heads between them, forward and backward --, the HIP entries against
upstream's op sequence under autograd (networks.ManyDepth.expansion_layer_composite) in torch on the same GPU in the same run:

    python tools/time_expansion_layer_backward.py [--window 0.5] [--repeats 7] [--out profiles/expansion_layer_backward_times.json]

  backward_hip        ops.expansion_layer_backward (mcr_expansion_layer_backward) alone, all six outputs, on a kept u and y
  backward_composite  torch.autograd.grad of all six through expansion_layer_composite, on a recorded graph that is kept
  step_hip            autograd.ExpansionLayerFunction: the fused forward and the HIP backward, all six gradients
  step_composite      expansion_layer_composite under autograd, forward and backward, all six gradients

  (Cin, Cmid, Cadd, Cout, h x w -> H x W):   expansion5 (512, 256, 256, 256, 8x15 -> 16x29)    expansion4 (256, 128, 128, 128, 16x29 -> 32x57)
  expansion3 (128, 64, 64, 64, 32x57 -> 64x114)   expansion2 (64, 32, 64, 32, 64x114 -> 128x228)   expansion1 (32, 16, 3, 16, 128x228 -> 256x456)

The decoder row runs the modules (ManyDepth.ExpansionLayer, DisparityLayer) as a trainer does: expansion5 .. 1 on each other's results
with the skip features as x_add, disp4 .. disp1 on the results of expansion4 .. 1, a weighted sum of the four maps as the loss, backward
into all 28 parameter tensors, the layer4 features and the skips; `step_hip` with MCR_EXPANSION_LAYER, MCR_EXPANSION_LAYER_BWD and
MCR_DISPARITY_HEAD_BWD set to hip, `step_composite` with all three unset (every module on its composite).

The method is that of tools/time_expansion_layer.py: host clock between two device synchronisations over a window of calls, the same
inputs every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about --window seconds; one
repeat times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the repeats, the
distance between the two routes' gradients (the largest over the gradients, each relative to its largest magnitude), and per pair
`hip_faster_than_composite_intervals_apart`: the HIP route's whole interval lies below the composite's whole interval.
`hip_would_be_default_by_the_rule` is true only if that holds for the `step` pair in all ten single-layer rows; the default route under
a gradient does not follow it (MCR_EXPANSION_LAYER_BWD stays opt-in).  Reads nothing outside the repository."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_expansion_layer import SHAPES, far, layer, timed  # noqa: E402

from macarons_amd import autograd, ops  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402

KNOBS = ("MCR_EXPANSION_LAYER", "MCR_EXPANSION_LAYER_BWD", "MCR_DISPARITY_HEAD_BWD")
KEYS = ("x", "x_add", "up_weight", "up_bias", "i_weight", "i_bias")
PAIRS = (("backward_hip", "backward_composite"), ("step_hip", "step_composite"))


def knobs(value):
    for k in KNOBS:
        if value is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = value


def single_layer_routes(v, gen):
    leaves = [v[k].clone().requires_grad_(True) for k in KEYS]
    size = v["output_size"]
    with torch.no_grad():
        y, u = ops.expansion_layer(*leaves, size, return_u=True)
    d_y = torch.randn(y.shape, generator=gen).to(y.device)
    recorded = ManyDepth.expansion_layer_composite(*leaves, size)
    x, x_add, wu, _, wi, _ = [t.detach() for t in leaves]

    def backward_hip():
        return ops.expansion_layer_backward(x, x_add, wu, wi, u, y, d_y, size)

    def backward_composite():
        return torch.autograd.grad(recorded, leaves, d_y, retain_graph=True)

    def step_hip():
        return torch.autograd.grad(autograd.ExpansionLayerFunction.apply(*leaves, size), leaves, d_y)

    def step_composite():
        return torch.autograd.grad(ManyDepth.expansion_layer_composite(*leaves, size), leaves, d_y)

    return {"backward_hip": backward_hip, "backward_composite": backward_composite, "step_hip": step_hip, "step_composite": step_composite}


def tail_routes(layers, gen):
    dev = layers[0]["x"].device
    mods, heads = [], []
    for k, v in enumerate(layers):
        Cin, Cmid = v["up_weight"].shape[:2]
        Cout, Cadd = v["i_weight"].shape[0], v["x_add"].shape[1]
        m = ManyDepth.ExpansionLayer(Cin, Cmid, Cout, tuple(v["output_size"]), additional_channels=Cadd).to(dev)
        m.load_state_dict({"upconv.weight": v["up_weight"], "upconv.bias": v["up_bias"], "iconv.weight": v["i_weight"], "iconv.bias": v["i_bias"]})
        mods.append(m)
        if k:
            hd = ManyDepth.DisparityLayer(Cout).to(dev)
            hd.load_state_dict({"conv.weight": v["head_weight"], "conv.bias": v["head_bias"]})
            heads.append(hd)
    x0 = layers[0]["x"].clone().requires_grad_(True)
    skips = [v["x_add"].clone().requires_grad_(True) for v in layers]
    weights = [torch.randn(v["x"].shape[0], 1, *v["output_size"], generator=gen).to(dev) for v in layers[1:]]
    wrt = [x0] + skips + [p for m in mods + heads for p in m.parameters()]

    def step():
        x, loss = x0, 0.0
        for k, (m, s) in enumerate(zip(mods, skips)):
            x = m(x, s)
            if k:
                loss = loss + (heads[k - 1](x) * weights[k - 1]).sum()
        return torch.autograd.grad(loss, wrt)

    def step_hip():
        knobs("hip")
        return step()

    def step_composite():
        knobs(None)
        return step()

    return {"step_hip": step_hip, "step_composite": step_composite}


def measure(routes, pairs, window, repeats):
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(window / (timed(fn, 5) * 1e-3))))
    res = {"iters": iters}
    for hip, comp in pairs:
        res[f"{hip}_vs_{comp}_rel"] = max(far(a, b) for a, b in zip(routes[hip](), routes[comp]()))
    runs = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            runs[k].append(timed(fn, iters[k]))
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["hip_faster_than_composite_intervals_apart"] = {hip.split("_")[0]: res[hip + "_ms"]["max"] < res[comp + "_ms"]["min"] for hip, comp in pairs}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expansion_layer_backward_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_expansion_layer_backward: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    res = {"shapes": {k: [*v[:4], list(v[4]), list(v[5])] for k, v in SHAPES.items()}, "shape_columns": "Cin, Cmid, Cadd, Cout, [h, w], [H, W]",
           "device": torch.cuda.get_device_name(0), "window_s": a.window, "repeats": a.repeats, "clock": "host, between device synchronisations"}
    apart = []
    for B in (1, 4):
        gen = torch.Generator().manual_seed(23)
        layers = {k: layer(B, *s, dev, gen) for k, s in SHAPES.items()}
        rows = {}
        knobs(None)
        os.environ["MCR_EXPANSION_LAYER_BWD"] = "hip"        # the Function's backward is the HIP entry in the single-layer rows
        for k, v in layers.items():
            rows[k] = measure(single_layer_routes(v, gen), PAIRS, a.window, a.repeats)
            apart.append(rows[k]["hip_faster_than_composite_intervals_apart"]["step"])
        rows["decoder_tail_five_layers_four_heads"] = measure(tail_routes(list(layers.values()), gen), PAIRS[1:], a.window, a.repeats)
        knobs(None)
        res[f"B{B}"] = rows
        for k, r in rows.items():
            print(f"B{B} {k}: " + "  ".join(f"{n} {r[n + '_ms']['median']:.4f} [{r[n + '_ms']['min']:.4f}, {r[n + '_ms']['max']:.4f}]"
                                          for n in ("backward_hip", "backward_composite", "step_hip", "step_composite") if n + "_ms" in r)
                  + f"  rel {r['step_hip_vs_step_composite_rel']:.1e}  apart {r['hip_faster_than_composite_intervals_apart']}", flush=True)
    res["hip_would_be_default_by_the_rule"] = all(apart)
    print(f"hip_would_be_default_by_the_rule {res['hip_would_be_default_by_the_rule']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
