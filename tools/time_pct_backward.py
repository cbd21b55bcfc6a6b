"""Time the PCTransformer's HIP backward (mcr_pc_transformer_backward) against the composite backward, with HIP events after warm-up.

    python tools/time_pct_backward.py [--iters 50] [--repeats 5] [--shapes 6000x16,18000x16,1x2048,8x2048] [--hip-only] [--out FILE.json]

Per shape S x L (feature_dim 256 for 16-token sequences, 512 otherwise): the forward (PCTransformer.forward without a graph), the
HIP backward call (ops.pc_transformer_backward: recompute included, every gradient) and the composite backward
(autograd.pc_transformer recomputed in fp32 and differentiated).  One repeat times --iters whole calls of each path back to back,
the paths taking turns (forward, HIP, composite, forward, HIP, ...); the JSON keeps every repeat's mean and the median / min / max
over the repeats.  Peak memory: what one call adds to the allocated memory (torch.cuda.max_memory_allocated), each measured from an
empty workspace arena (the HIP figures include growing the arena; the composite allocates everything itself).  --hip-only: the
forward and the HIP backward alone (profiler runs).  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool.
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
from macarons_amd.networks.SconeOcc import PCTransformer  # noqa: E402
import weights  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="6000x16,18000x16,1x2048,8x2048")
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rows = []
    for S, L in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]:
        fd = 256 if L == 16 else 512
        m = PCTransformer(seq_len=L, pts_embedding_dim=128, feature_dim=fd)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(weights.shapes_of(m), 12).items()}, strict=True)
        m = m.to(dev)
        pc = torch.from_numpy(rng.uniform(-.05 if L == 16 else -.5, .05 if L == 16 else .5, (S, L, 3)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((S, fd)).astype(np.float32)).to(dev)
        tab = m.weight_table()
        params = list(m.parameters())

        def fwd():
            with torch.no_grad():
                m(pc)

        def hip():
            ops.pc_transformer_backward(pc, g, tab, fd)

        def comp():
            p = pc.detach().requires_grad_(True)
            with torch.enable_grad():
                torch.autograd.grad(A.pc_transformer(m, p), [p] + params, g)

        paths = {"forward_ms": fwd, "hip_backward_ms": hip}
        if not a.hip_only:
            paths["composite_backward_ms"] = comp
        runs = {k: [] for k in paths}
        for _ in range(a.repeats):
            for k, fn in paths.items():
                runs[k].append(timed(fn, a.iters))
        row = {"S": S, "L": L, "feature_dim": fd, "iters": a.iters, "repeats": a.repeats,
               "chunk": ops.pc_transformer_backward_chunk(S, L)}
        for k, v in runs.items():
            row[k] = float(np.median(v))
            row[k.replace("_ms", "_min_ms")], row[k.replace("_ms", "_max_ms")] = min(v), max(v)
            row[k.replace("_ms", "_runs_ms")] = v
        row["forward_peak_rise_MB"] = peak_rise(fwd, dev)
        row["hip_peak_rise_MB"] = peak_rise(hip, dev)
        if not a.hip_only:
            row["composite_peak_rise_MB"] = peak_rise(comp, dev)
            row["speedup_median"] = row["composite_backward_ms"] / row["hip_backward_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
