"""Time SconeOcc.forward + backward on its three backward routes (env MCR_SCONE_OCC_BWD: composite, pct, hip), with HIP events after warm-up.

    python tools/time_scone_occ_backward.py [--iters 5] [--repeats 3] [--shapes 3x6000x16384x2048,1x6000x16384x2048]
                                            [--routes composite,pct,hip] [--out FILE.json]

Per shape B x Q x M x Lg (clouds, queries per cloud, surface points per cloud, tokens of the global sequence -- the pre-training shape
is 3 x 6000 x 16384 x 2048, configs/scone/occupancy): one training step's autograd work, `occ(pc, x, vh, perms=...).sum().backward()`
with every parameter, x and the harmonics requiring a gradient (pc does not: no trainer asks for it), the hidden draws pinned.  One
repeat times --iters whole steps of each route back to back, the routes taking turns (composite, pct, hip, composite, ...); the JSON keeps
every repeat's mean and the median / min / max over the repeats, and the no-grad forward's time for scale.  Peak memory: what one
step adds to the allocated memory (torch.cuda.max_memory_allocated), each measured from an empty workspace arena and empty gradients
(the HIP figures include growing the arena; torch allocates its graph itself).  Kernel times come from a separate
rocprofv3 --kernel-trace --stats run of this tool (--routes hip).
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
from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import SconeOcc  # noqa: E402
import weights  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters            # ms per step


def peak_rise(fn, dev):
    ops._ws_cache.clear()                       # an empty workspace arena: the HIP figures include growing it
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return (torch.cuda.max_memory_allocated(dev) - base) / 2**20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="3x6000x16384x2048,1x6000x16384x2048")
    ap.add_argument("--routes", default="composite,pct,hip")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    routes = a.routes.split(",")
    assert set(routes) <= {"composite", "pct", "hip"}, routes
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rows = []
    for B, Q, M, Lg in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        occ = SconeOcc(seq_len=Lg)
        occ.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(weights.shapes_of(occ), 2).items()}, strict=True)
        occ = occ.to(dev)
        torch.manual_seed(4)
        perms = occ.draw_perms(M)
        pc = torch.from_numpy(rng.uniform(-.5, .5, (B, M, 3)).astype(np.float32)).to(dev)
        x = torch.from_numpy(rng.uniform(-.5, .5, (B, Q, 3)).astype(np.float32)).to(dev).requires_grad_(True)
        vh = torch.from_numpy((rng.standard_normal((B, Q, 64)) * 0.3).astype(np.float32)).to(dev).requires_grad_(True)

        def drop_grads():
            occ.zero_grad(set_to_none=True)
            x.grad = vh.grad = None

        def fwd():
            with torch.no_grad():
                occ(pc, x, vh, perms=perms)

        def step(route):
            def fn():
                os.environ["MCR_SCONE_OCC_BWD"] = route
                drop_grads()
                occ(pc, x, vh, perms=perms).sum().backward()
            return fn

        paths = {"forward_ms": fwd}
        paths.update({f"{r}_step_ms": step(r) for r in routes})
        runs = {k: [] for k in paths}
        for _ in range(a.repeats):
            for k, fn in paths.items():
                runs[k].append(timed(fn, a.iters))
        row = {"B": B, "Q": Q, "M": M, "Lg": Lg, "iters": a.iters, "repeats": a.repeats, "q_chunk": ops.scone_occ_backward_chunk(Q)}
        for k, v in runs.items():
            row[k] = float(np.median(v))
            row[k.replace("_ms", "_min_ms")], row[k.replace("_ms", "_max_ms")] = min(v), max(v)
            row[k.replace("_ms", "_runs_ms")] = v
        drop_grads()
        row["forward_peak_rise_MB"] = peak_rise(fwd, dev)
        for r in routes:
            drop_grads()
            row[f"{r}_step_peak_rise_MB"] = peak_rise(step(r), dev)
        if "pct" in routes and "hip" in routes:
            row["hip_over_pct_median"] = row["hip_step_ms"] / row["pct_step_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del occ, pc, x, vh
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
