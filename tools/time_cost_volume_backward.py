"""Time the backward of the depth module's plane sweep at upstream's size (the inputs of tools/time_cost_volume.py's build(): B 1, 2
sources, 96 planes, 256 x 456 images, 64 x 114 x 64 features), the HIP route against the composite route in the same run:

    python tools/time_cost_volume_backward.py [--window 0.5] [--repeats 7] [--out profiles/cost_volume_backward_times.json]
    tools/kstats.sh cost_volume_backward 14 -- python tools/time_cost_volume_backward.py --kernels-only 50   (the kernels' own times)

  backward_hip           ops.cost_volume_backward (mcr_cost_volume_backward), both gradients
  backward_hip_x_only    the same entry, need_x_alpha=False
  backward_hip_function  CostVolumeFunction.backward on the HIP route, called through torch.autograd.grad on a retained graph: the HIP
                         entry with the same autograd overhead as backward_composite carries
  backward_composite     CostVolumeFunction.backward under MCR_COST_VOLUME_BWD=composite (the recomputation in torch, 8 planes at a
                         time), called the same way
  step_hip, step_composite   the mirror class: forward, then the backward of res.sum() for x, x_alpha and conv_reduce's parameters

The method is that of tools/time_cost_volume.py: host clock between two device synchronisations over a window of calls, the same inputs
and workspace every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about --window
seconds; one repeat times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the
repeats ("the interval").  It also keeps the peak of torch.cuda.max_memory_allocated over one step of either route above what the
inputs hold (the workspace arena is dropped first, so the HIP step's figure includes it), the workspace bytes of the entry, the distance
between the two routes' gradients (max |difference| / max |composite|; both routes are fp32, and where they round some m_c - x_c to
different sides of zero -- a few of 45 million at this size -- a gradient element moves by 2 g / C: those elements are counted and the
distance over all the others is given beside the maximum), and `hip_faster_than_composite_intervals_apart`: the HIP route's whole
interval lies below the composite's whole interval, for the backward (through the function, and the entry alone) and for the step.
Reads nothing outside the repository."""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_cost_volume import A, B, C, D, H, HF, OUT_CH, W, WF, build, timed  # noqa: E402

from macarons_amd import _lib, ops  # noqa: E402
from macarons_amd.autograd import CostVolumeFunction  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_volume_backward_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cost_volume_backward: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    m, t = build(dev)
    x, R, T, zf, xa, Ra, Ta, zfa = t
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta)
    bins = m.depth_bins.to(dev)
    d_out = torch.randn((B, D, HF, WF), generator=torch.Generator().manual_seed(2)).to(dev)

    if a.kernels_only:
        for _ in range(a.kernels_only):
            ops.cost_volume_backward(x, xa, cams, bins, d_out, H, W)
        torch.cuda.synchronize()
        return

    xg, xag = x.clone().requires_grad_(True), xa.clone().requires_grad_(True)
    cv = CostVolumeFunction.apply(xg, xag, cams, bins, H, W, ops.COST_VOLUME_FOV_SCALE, False)
    params = tuple(m.conv_reduce.parameters())

    def under(mode, fn):
        def run():
            os.environ["MCR_COST_VOLUME_BWD"] = mode
            try:
                return fn()
            finally:
                del os.environ["MCR_COST_VOLUME_BWD"]
        return run

    def function_backward():
        return torch.autograd.grad(cv, (xg, xag), d_out, retain_graph=True)

    def step():
        res = m(xg, R, T, zf, xag, Ra, Ta, zfa, dev)
        return torch.autograd.grad(res.sum(), (xg, xag) + params)

    routes = {
        "backward_hip": lambda: ops.cost_volume_backward(x, xa, cams, bins, d_out, H, W),
        "backward_hip_x_only": lambda: ops.cost_volume_backward(x, xa, cams, bins, d_out, H, W, need_x_alpha=False),
        "backward_hip_function": under("hip", function_backward),
        "backward_composite": under("composite", function_backward),
        "step_hip": under("hip", step),
        "step_composite": under("composite", step),
    }
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(a.window / (timed(fn, 5) * 1e-3))))
    g_hip, g_comp = routes["backward_hip_function"](), routes["backward_composite"]()
    dist = {}
    for n, h, c in zip(("x", "x_alpha"), g_hip, g_comp):
        e = (h - c).abs() / c.abs().max()
        far = e > 1e-4                                   # elements where the two fp32 routes took a different sign of some m_c - x_c
        dist[n] = {"max": float(e.max()), "elements_beyond_1e-4": int(far.sum()), "elements": e.numel(),
                   "max_over_the_others": float(e[~far].max())}
    del g_hip, g_comp
    runs = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():
            runs[k].append(timed(fn, iters[k]))

    def peak(fn):
        ops._ws_cache.clear()                            # the arena is allocated again inside: it counts
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    mem = {k: peak(routes[k]) for k in ("step_hip", "step_composite")}
    i64 = ctypes.c_int64
    res = {"size": dict(B=B, A=A, C=C, D=D, H=H, W=W, Hf=HF, Wf=WF, out_channels=OUT_CH), "device": torch.cuda.get_device_name(0),
           "window_s": a.window, "iters": iters, "repeats": a.repeats, "clock": "host, between device synchronisations",
           "hip_vs_composite_gradient_rel": dist}
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["peak_memory_above_inputs_MiB"] = mem
    res["workspace_bytes"] = int(_lib.lib().mcr_cost_volume_backward_workspace_bytes(i64(B), i64(A), i64(C), i64(HF), i64(WF), i64(D)))
    res["hip_faster_than_composite_intervals_apart"] = {
        "backward": res["backward_hip_function_ms"]["max"] < res["backward_composite_ms"]["min"],
        "backward_entry_alone": res["backward_hip_ms"]["max"] < res["backward_composite_ms"]["min"],
        "step": res["step_hip_ms"]["max"] < res["step_composite_ms"]["min"]}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
