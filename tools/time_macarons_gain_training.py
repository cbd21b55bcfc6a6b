"""Time the MACARONS-regime training step predict_coverage_gain_for_cameras(...) -> loss -> backward() two ways, with HIP events after warm-up.

    python tools/time_macarons_gain_training.py [--cameras 5,30] [--points 100000] [--seq-len 2048] [--iters 3] [--repeats 5] [--out FILE.json]

  batched     one call of K cameras: one padded SconeVis forward / backward, one weight-gradient pass, one scorer and one gain backward;
  per_camera  K calls of one camera each, their gains concatenated into the same loss -- the shape of upstream's loop
              (train_macarons.py:438-444 over predict_coverage_gain_for_single_camera): K SconeVis backwards, K weight-gradient passes.

Scene: P proxy points uniform in the single_camera golden's box with uniform occupancy probabilities and that test's view harmonics; the
K cameras are the golden's three non-empty cameras taken in turn (camera k = golden camera k mod 3); weights from the golden seed, as
tests/test_macarons_regime_gpu.py::_models builds them; the same uniforms for both routes.  One repeat times --iters whole steps of each
route back to back, the routes taking turns; the JSON keeps every repeat's mean and the median / min / max over the repeats.  The share of
the new kernel: mcr_macarons_gain_backward alone on the batched step's own operands (HIP events around 200 launches) over the batched
step's median.  Kernel times by name come from a separate rocprofv3 --kernel-trace --stats run of this tool."""
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
from macarons_amd.networks import SconeVis  # noqa: E402
from macarons_amd.utility import macarons_utils as mu  # noqa: E402
import weights  # noqa: E402


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
    return e0.elapsed_time(e1) / iters            # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", default="5,30")
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--seq-len", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "single_camera.npz"))
    rng = np.random.default_rng(0)
    P, S = a.points, a.seq_len
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    X_world = T(rng.uniform(-40, 40, (P, 3)).astype(np.float32))
    occ = T(rng.uniform(0, 1, (P, 1)).astype(np.float32))
    vh = T((rng.standard_normal(P)[:, None] * g["vh_v"][None, :] + g["vh_w"][np.arange(P) % 16]).astype(np.float32))
    vis = SconeVis()
    vis.load_state_dict({k: torch.from_numpy(v) for k, v in weights.make_state_dict(weights.shapes_of(vis), 1).items()}, strict=True)
    vis = vis.to(dev).eval()
    rows = []
    for K in [int(v) for v in a.cameras.split(",")]:
        sel = [k % 3 for k in range(K)]
        recs = torch.stack([mu.camera_record(g["Mview"][c], g["Mfull"][c], g["ndc"], g["center"][c], float(g["sensor_range"])) for c in sel]).to(dev)
        eyes = T(g["eyes"][sel])
        Mpred = T(np.repeat(g["Mpred"], K, 0))
        u = T(rng.uniform(0, 1, (K, S)).astype(np.float32))
        target = T(rng.uniform(0, 50, K).astype(np.float32))
        box_diag = float(g["box_diag"])

        def gains_of(lo, hi):
            return mu.predict_coverage_gain_for_cameras(vis, X_world, vh, occ, recs[lo:hi], eyes[lo:hi], Mpred[lo:hi], box_diag, seq_len=S,
                                                        samples=u[lo:hi], differentiable=True)

        def batched():
            vis.zero_grad(set_to_none=True)
            ((gains_of(0, K) - target) ** 2).mean().backward()

        def per_camera():
            vis.zero_grad(set_to_none=True)
            ((torch.cat([gains_of(k, k + 1) for k in range(K)]) - target) ** 2).mean().backward()

        # the two routes compute the same step: compare once
        batched()
        ref = {n: p.grad.clone() for n, p in vis.named_parameters()}
        per_camera()
        scale = max(float(t.abs().max()) for t in ref.values())
        agree = max(float((p.grad - ref[n]).abs().max()) for n, p in vis.named_parameters()) / scale
        # the gain backward's own operands, as the batched step hands them over
        seen = []
        inner = ops.macarons_gain_backward
        ops.macarons_gain_backward = lambda *args, **kw: (seen.append((args, kw)), inner(*args, **kw))[1]
        try:
            batched()
        finally:
            ops.macarons_gain_backward = inner
        (args, kw), = seen
        kernel_ms = timed(lambda: inner(*args, **kw), 200, warmup=5)

        paths = {"batched_step_ms": batched, "per_camera_step_ms": per_camera}
        runs = {k: [] for k in paths}
        for _ in range(a.repeats):
            for k, fn in paths.items():
                runs[k].append(timed(fn, a.iters))
        row = {"K": K, "P": P, "S": S, "iters": a.iters, "repeats": a.repeats, "n_unique": [int(v) for v in args[4].tolist()],
               "routes_max_grad_difference_over_largest": agree, "gain_backward_kernel_ms": kernel_ms}
        for k, v in runs.items():
            row[k] = float(np.median(v))
            row[k.replace("_ms", "_min_ms")], row[k.replace("_ms", "_max_ms")] = min(v), max(v)
            row[k.replace("_ms", "_runs_ms")] = v
        row["per_camera_over_batched_median"] = row["per_camera_step_ms"] / row["batched_step_ms"]
        row["gain_backward_share_of_batched_step"] = kernel_ms / row["batched_step_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
