"""Time one training step of the occupancy supervision pass -- forward, mean squared error, backward() -- on its three routes, with HIP
events after warm-up.

    python tools/time_scone_occ_ragged_backward.py [--iters 3] [--repeats 3] [--routes ragged,hip,pct] [--out FILE.json]

The supervision shape (macarons_utils.py:1233-1392 of the reference: ~6000 proxy points spread over the grid cells that hold them):
J = 8 jobs, T = 6000 query rows split unevenly over them (one job of 9 rows), surface clouds of 3000 to 27 000 points, Lg = 2048,
golden-seed weights, the hidden draws pinned; every parameter, x and the harmonics require a gradient.
  ragged   ONE SconeOcc.forward_ragged(..., differentiable=True) call, one graph, one mcr_scone_occ_backward_ragged
  hip      J forward() calls under MCR_SCONE_OCC_BWD=hip, J graphs, J mcr_scone_occ_backward calls, gradients accumulated by torch
  pct      the same under MCR_SCONE_OCC_BWD=pct (torch composite around the HIP PCTransformer backward)
The per-job routes are what the code ran before the ragged backward existed.  One repeat times --iters whole steps of each route back
to back, the routes taking turns; the JSON keeps every repeat's mean and the median / min / max over the repeats.  Peak memory: what one
step adds to the allocated memory (torch.cuda.max_memory_allocated), measured from an empty workspace arena and empty gradients.
Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool (--routes ragged).
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

CLOUDS = (27000, 3000, 12000, 5000, 20000, 8000, 16384, 4000)
ROWS = (1800, 9, 1200, 300, 1500, 400, 700, 91)


def timed(fn, iters, warmup=1):
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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--routes", default="ragged,hip,pct")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    routes = a.routes.split(",")
    assert set(routes) <= {"ragged", "hip", "pct"}, routes
    assert sum(ROWS) == 6000 and len(ROWS) == len(CLOUDS) and min(ROWS) < 16
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    J, n = len(ROWS), sum(ROWS)
    occ = SconeOcc()
    occ.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(weights.shapes_of(occ), 2).items()}, strict=True)
    occ = occ.to(dev)
    torch.manual_seed(4)
    perms = [occ.draw_perms(M) for M in CLOUDS]
    pc = torch.from_numpy(rng.uniform(-.5, .5, (sum(CLOUDS), 3)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.uniform(-.5, .5, (n, 3)).astype(np.float32)).to(dev).requires_grad_(True)
    vh = torch.from_numpy((rng.standard_normal((n, 64)) * 0.3).astype(np.float32)).to(dev).requires_grad_(True)
    target = torch.from_numpy(rng.uniform(0, 1, (n, 1)).astype(np.float32)).to(dev)
    o0, r0 = np.concatenate(([0], np.cumsum(CLOUDS))), np.concatenate(([0], np.cumsum(ROWS)))

    # the per-job routes' operands: tensors of their own (mcr_scone_occ_backward wants 16-byte aligned operands, which a row slice is not)
    jobs = [(pc[o0[j]:o0[j + 1]][None].clone(), x.detach()[r0[j]:r0[j + 1]][None].clone().requires_grad_(True),
             vh.detach()[r0[j]:r0[j + 1]][None].clone().requires_grad_(True), target[r0[j]:r0[j + 1]].clone()) for j in range(J)]

    def drop_grads():
        occ.zero_grad(set_to_none=True)
        x.grad = vh.grad = None
        for _, xj, vj, _ in jobs:
            xj.grad = vj.grad = None

    def ragged():
        os.environ.pop("MCR_SCONE_OCC_BWD", None)
        drop_grads()
        y = occ.forward_ragged(pc, list(CLOUDS), x, vh, list(ROWS), perms=perms, differentiable=True)
        ((y - target) ** 2).mean().backward()

    def per_job(route):
        def fn():
            os.environ["MCR_SCONE_OCC_BWD"] = route
            drop_grads()
            for (pcj, xj, vj, tj), pj in zip(jobs, perms):        # the mean over all T rows, job by job: J graphs, gradients accumulate
                (((occ(pcj, xj, vj, perms=pj)[0] - tj) ** 2).sum() / n).backward()
        return fn

    paths = {f"{r}_step_ms": (ragged if r == "ragged" else per_job(r)) for r in routes}
    runs = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, fn in paths.items():
            runs[k].append(timed(fn, a.iters))
    row = {"J": J, "T": n, "rows": list(ROWS), "clouds": list(CLOUDS), "Lg": occ.seq_len, "iters": a.iters, "repeats": a.repeats,
           "q_chunk": ops.scone_occ_backward_chunk(n)}
    for k, v in runs.items():
        row[k] = float(np.median(v))
        row[k.replace("_ms", "_min_ms")], row[k.replace("_ms", "_max_ms")] = min(v), max(v)
        row[k.replace("_ms", "_runs_ms")] = v
    for r in routes:
        drop_grads()
        row[f"{r}_step_peak_rise_MB"] = peak_rise(paths[f"{r}_step_ms"], dev)
    if "ragged" in routes and "hip" in routes:
        row["ragged_over_hip_median"] = row["ragged_step_ms"] / row["hip_step_ms"]
    # the three routes compute the same gradients: the largest difference of a parameter gradient, over the largest gradient
    if "ragged" in routes and "hip" in routes:
        ragged()
        g_r = [q.grad.clone() for q in occ.parameters()]
        per_job("hip")()
        scale = max(float(g.abs().max()) for g in g_r)
        row["ragged_vs_hip_param_grad_diff"] = max(float((q.grad - g).abs().max()) for q, g in zip(occ.parameters(), g_r)) / scale
    os.environ.pop("MCR_SCONE_OCC_BWD", None)
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump([row], f, indent=1)


if __name__ == "__main__":
    main()
