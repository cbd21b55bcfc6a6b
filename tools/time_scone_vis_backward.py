"""Time SconeVis's HIP backward (mcr_scone_vis_backward) against the composite backward it replaces, with HIP events after warm-up.

    python tools/time_scone_vis_backward.py [--iters 50] [--repeats 5] [--batches 1,4,8] [--hip-only] [--out FILE.json]

Per batch B x 2048: the forward (SconeVis.forward without a graph), the HIP backward call (ops.scone_vis_backward: recompute
included, every gradient) and the composite backward (autograd.scone_vis recomputed in fp32 and differentiated, as
autograd._HipForwardTorchBackward does).  One repeat times --iters whole calls of each path back to back, the paths taking turns
(forward, HIP, composite, forward, HIP, ...); the JSON keeps every repeat's mean and the median / min / max over the repeats.  Peak
memory: what one backward call adds to the allocated memory, each measured from an empty workspace arena (the HIP figure includes
growing the arena to the backward's size; the composite allocates everything itself).  --hip-only: the forward and the HIP backward
alone (profiler runs).  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from macarons_amd import autograd as A  # noqa: E402
from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import SconeVis  # noqa: E402
import weights  # noqa: E402

FLOP_PER_CLOUD = 44e9


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters            # ms per call


def peak_rise(fn, dev):
    ops._ws_cache.clear()                       # an empty workspace arena: the HIP backward's figure includes growing it
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = SconeVis()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(weights.shapes_of(m), 1).items()}, strict=True)
    m = m.to(dev)
    rng = np.random.default_rng(0)
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        N = 2048
        pts = torch.from_numpy(np.concatenate([rng.uniform(-.5, .5, (B, N, 3)), rng.uniform(.1, 1, (B, N, 1))], -1).astype(np.float32)).to(dev)
        vh = torch.from_numpy((rng.standard_normal((B, N, 64)) * 0.3).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((B, N, 64)).astype(np.float32)).to(dev)
        tab = m._table_cache.get(m, m.weight_table_with_planes)

        def fwd():
            with torch.no_grad():
                m(pts, view_harmonics=vh)

        def hip():
            ops.scone_vis_backward(pts, vh, g, tab)

        params = list(m.parameters())

        def comp():
            p, v = pts.detach().requires_grad_(True), vh.detach().requires_grad_(True)
            with torch.enable_grad():
                y = A.scone_vis(m, p, v)
                torch.autograd.grad(y, [p, v] + params, g)

        paths = {"forward_ms": fwd, "hip_backward_ms": hip}
        if not a.hip_only:
            paths["composite_backward_ms"] = comp
        runs = {k: [] for k in paths}
        for _ in range(a.repeats):
            for k, fn in paths.items():
                runs[k].append(timed(fn, a.iters))
        row = {"B": B, "N": N, "iters": a.iters, "repeats": a.repeats}
        for k, v in runs.items():
            row[k] = float(np.median(v))
            row[k.replace("_ms", "_min_ms")], row[k.replace("_ms", "_max_ms")] = min(v), max(v)
            row[k.replace("_ms", "_runs_ms")] = v
        row["hip_peak_rise_MB"] = peak_rise(hip, dev)
        if not a.hip_only:
            row["composite_peak_rise_MB"] = peak_rise(comp, dev)
            row["speedup_median"] = row["composite_backward_ms"] / row["hip_backward_ms"]
            row["speedup_worst"] = row["composite_backward_min_ms"] / row["hip_backward_max_ms"]
        row["hip_TFLOPs"] = FLOP_PER_CLOUD * B / (row["hip_backward_ms"] * 1e-3) / 1e12
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
