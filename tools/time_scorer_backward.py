"""Time the scorer's HIP backward (mcr_sh_scorer_backward) with HIP events, after warm-up.

    python tools/time_scorer_backward.py [--iters 50] [--out FILE.json]

Per shape (B, N, C): the forward scorer (ops.sh_coverage_gain), the backward for gains with d_harm alone (what the trainers ask for)
and with all three gradients, and -- at the pretraining shapes -- the composite backward it replaces (recompute autograd.coverage_gain
in fp32 and differentiate it, as autograd._HipForwardTorchBackward did).  Each figure is the mean of --iters calls (whole calls: the
Python wrapper, allocations and every launch).  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from macarons_amd import autograd as A  # noqa: E402
from macarons_amd import ops  # noqa: E402

SHAPES = [(1, 2048, 52), (3, 2048, 52), (1, 20_000, 200), (1, 100_000, 200)]
PRETRAIN = SHAPES[:2]


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters            # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rows = []
    for B, N, C in SHAPES:
        pts = torch.from_numpy(np.concatenate([rng.uniform(-.5, .5, (B, N, 3)), rng.uniform(.1, 1, (B, N, 1))], -1).astype(np.float32)).to(dev)
        harm = torch.from_numpy((rng.standard_normal((B, N, 64)) * 0.5).astype(np.float32)).to(dev)
        cams = rng.standard_normal((B, C, 3))
        cams = torch.from_numpy((1.5 * cams / np.linalg.norm(cams, axis=-1, keepdims=True)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).to(dev)
        r = dict(B=B, N=N, C=C, pairs=B * N * C)
        r["forward_us"] = timed(lambda: ops.sh_coverage_gain(pts, harm, cams), a.iters)
        r["bwd_harm_only_us"] = timed(lambda: ops.sh_scorer_backward(pts, harm, cams, g, False, True, need=(True, False, False)), a.iters)
        r["bwd_all_us"] = timed(lambda: ops.sh_scorer_backward(pts, harm, cams, g, False, True), a.iters)
        if (B, N, C) in PRETRAIN:
            def composite():
                h = harm.detach().requires_grad_(True)
                with torch.enable_grad():
                    out = A.coverage_gain(pts, h, cams, True)
                    return torch.autograd.grad(out, [h], g)
            r["composite_harm_only_us"] = timed(composite, max(5, a.iters // 5))
            r["speedup_harm_only"] = r["composite_harm_only_us"] / r["bwd_harm_only_us"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
