"""Time the depth module's plane sweep at upstream's size (B 1, n_alpha 2, C 64, 96 planes 0.5 .. 750, 256 x 456 images, 64 x 114
features; random features, poses of the kind of the golden's case a):

    python tools/time_cost_volume.py [--iters 5000] [--base-iters 64] [--repeats 7] [--out profiles/cost_volume_times.json]
    tools/kstats.sh cost_volume 10 -- python tools/time_cost_volume.py --kernels-only 50          (the two kernels' own times)

  entry     ops.cost_volume alone (mcr_cost_volume: the layout kernel and the sweep kernel)
  forward   networks.ManyDepth.CostVolumeBuilder.forward: camera packing, the entry writing into the concatenated buffer, conv_reduce, ReLU
  baseline  upstream's op sequence (ManyDepth.py:207-305) as upstream materialises it, restated here in unchunked torch ops on the same
            device, the expands made contiguous where upstream makes them: B*D and B*D*A cameras as 4x4 matrices, the unprojection of
            B*D depth maps through the inverted full projection, the A-fold copy of the world points, the projection with the eps rule,
            the channel transposes, F.interpolate(bicubic), the D-fold copy of the source maps, F.grid_sample, mean, L1 norm;
            `baseline_forward` adds the cat, conv_reduce and ReLU

A call is timed on the host clock between two device synchronisations over --iters (--base-iters) calls after a warm-up -- windows of
about half a second; the same inputs and workspace every call, so every route runs with its operands hot in the caches; one repeat times
every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the repeats ("the interval"), the
peak of torch.cuda.max_memory_allocated over one call of `forward` and of `baseline_forward` above what the inputs hold, the distance between
the entry's and the baseline's cost volume, and the bytes the sweep reads through its bilinear corners (positions x planes x sources x 4
x 256 B) over the entry's time.  Reads nothing outside the repository."""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from macarons_amd import ops  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402

B, A, C, D, H, W, HF, WF, OUT_CH = 1, 2, 64, 96, 256, 456, 64, 114, 64
D_MIN, D_MAX, ZNEAR, ZFAR, FOV = 0.5, 750.0, 1.0, 750.0, 60.0


def rot(axis, angle):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return (torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K).float()


def build(dev):
    g = torch.Generator().manual_seed(0)
    x, xa = torch.randn(B, C, HF, WF, generator=g), torch.randn(B, A, C, HF, WF, generator=g)
    R, T = rot([0, 1, 0], 0.1)[None], torch.tensor([[0.1, 0.2, 0.3]])
    Ra = torch.stack([rot([0, 1, 0], 0.12), rot([0.2, 1, 0], -0.07)])[None]
    Ta = torch.tensor([[[0.5, 0.0, -2.0], [-0.3, 0.1, 0.2]]])
    m = ManyDepth.CostVolumeBuilder(H, W, HF, WF, C, A, D_MIN, D_MAX, D, OUT_CH)
    torch.manual_seed(1)
    m.conv_reduce.reset_parameters()
    t = [v.to(dev) for v in (x, R, T, torch.full((B,), ZFAR), xa, Ra, Ta, torch.full((B, A), ZFAR))]
    return m.to(dev), t


def _projection(n, dev):
    """FoVPerspectiveCameras' default projection, row-vector form, n copies."""
    s = 1.0 / math.tan(math.radians(FOV) / 2)
    P = torch.tensor([[s, 0, 0, 0], [0, s, 0, 0], [0, 0, ZFAR / (ZFAR - ZNEAR), 1], [0, 0, -ZFAR * ZNEAR / (ZFAR - ZNEAR), 0]], device=dev)
    return P[None].expand(n, -1, -1).contiguous()


def _world_to_view(R, T):
    n = R.shape[0]
    M = torch.zeros(n, 4, 4, device=R.device)
    M[:, :3, :3], M[:, 3, :3], M[:, 3, 3] = R, T, 1.0
    return M


def baseline(x, R, T, zfar, xa, Ra, Ta, zfar_a, bins, conv=None):
    dev = x.device
    # B*D target cameras, B*D*A source cameras
    Rd, Td = R[:, None].expand(B, D, 3, 3).reshape(B * D, 3, 3), T[:, None].expand(B, D, 3).reshape(B * D, 3)
    Rad, Tad = Ra[:, None].expand(B, D, A, 3, 3).reshape(B * D * A, 3, 3), Ta[:, None].expand(B, D, A, 3).reshape(B * D * A, 3)
    P = _projection(B * D, dev)
    full = torch.bmm(_world_to_view(Rd, Td), P)
    full_a = torch.bmm(_world_to_view(Rad, Tad), _projection(B * D * A, dev))
    # unprojection of D constant depth maps per batch element
    depth = bins[None, :, None].expand(B, D, H * W).reshape(B * D, H * W, 1)          # materialised, as upstream's depth maps are
    m = min(H, W)
    ndc_x = (W / m - 2 * torch.arange(W, device=dev, dtype=torch.float32) / (m - 1))[None, :].expand(H, W).reshape(1, -1, 1)
    ndc_y = (H / m - 2 * torch.arange(H, device=dev, dtype=torch.float32) / (m - 1))[:, None].expand(H, W).reshape(1, -1, 1)
    ndc = torch.cat((ndc_x.expand(B * D, -1, -1), ndc_y.expand(B * D, -1, -1), depth), -1)
    sdepth = (P[:, 2, 2].view(-1, 1, 1) * ndc[..., 2:3] + P[:, 3, 2].view(-1, 1, 1)) / ndc[..., 2:3]
    p4 = torch.cat((ndc[..., :2], sdepth, torch.ones_like(sdepth)), -1)
    p4 = torch.bmm(p4, torch.linalg.inv(full))
    world = p4[..., :3] / p4[..., 3:4]
    # the A-fold copy of the world points, then their projection into the sources with the eps rule
    pts = world.view(B, D, 1, H * W, 3).expand(B, D, A, H * W, 3).reshape(B * D * A, H * W, 3)
    q4 = torch.baddbmm(full_a[:, 3:4, :], pts, full_a[:, :3, :])                     # [x y z 1] M
    w = q4[..., 3]
    w = torch.where(w < 0, -torch.ones_like(w), torch.ones_like(w)) * w.abs().clamp(min=1e-8)
    to_grid = torch.tensor([-min(WF, HF) / WF, -min(WF, HF) / HF], device=dev)
    grid = (q4[..., :2] / w[..., None]) * to_grid                                    # a new tensor, as upstream's slice-and-assign ends in one
    # channels first for the resize (a copy, as upstream's transposes are), bicubic to the feature size, channels last again (a copy)
    grid = grid.view(B * D * A, H, W, 2).permute(0, 3, 1, 2).contiguous()
    grid = F.interpolate(grid, size=(HF, WF), mode="bicubic", align_corners=False)
    grid = grid.permute(0, 2, 3, 1).contiguous()
    # the D-fold copy of the source maps, the sampling, the mean over the sources, the L1 distance over the channels
    src = xa.view(B, 1, A, C, HF, WF).expand(B, D, A, C, HF, WF).reshape(B * D * A, C, HF, WF)
    warped = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False).view(B, D, A, C, HF, WF)
    cv = (warped.mean(2) - x[:, None]).abs().sum(2) / C
    if conv is None:
        return cv
    return F.relu(conv(torch.cat((x, cv), 1)))


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--base-iters", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_volume_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cost_volume: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    m, t = build(dev)
    x, R, T, zf, xa, Ra, Ta, zfa = t
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta)
    bins = m.depth_bins.to(dev)
    with torch.no_grad():
        routes = {
            "entry": (lambda: ops.cost_volume(x, xa, cams, bins, H, W), a.iters),
            "forward": (lambda: m(x, R, T, zf, xa, Ra, Ta, zfa, dev), a.iters),
            "baseline": (lambda: baseline(x, R, T, zf, xa, Ra, Ta, zfa, bins), a.base_iters),
            "baseline_forward": (lambda: baseline(x, R, T, zf, xa, Ra, Ta, zfa, bins, m.conv_reduce), a.base_iters),
        }
        if a.kernels_only:
            for _ in range(a.kernels_only):
                routes["entry"][0]()
            torch.cuda.synchronize()
            return
        for fn, _ in routes.values():                    # warm-up: code objects, the convolution's algorithm choice, the allocator
            for _ in range(3):
                fn()
        cv_hip, cv_base = routes["entry"][0](), routes["baseline"][0]()
        dist = float((cv_hip - cv_base).abs().max() / cv_base.abs().max())
        res_dist = float((routes["forward"][0]() - routes["baseline_forward"][0]()).abs().max())
        del cv_hip, cv_base
        runs = {k: [] for k in routes}
        for _ in range(a.repeats):
            for k, (fn, iters) in routes.items():
                runs[k].append(timed(fn, iters))
        mem = {k: peak(routes[k][0]) for k in ("forward", "baseline_forward")}
    res = {"size": dict(B=B, A=A, C=C, D=D, H=H, W=W, Hf=HF, Wf=WF, out_channels=OUT_CH), "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "base_iters": a.base_iters, "repeats": a.repeats, "clock": "host, between device synchronisations",
           "entry_vs_baseline_cost_volume_rel": dist, "forward_vs_baseline_forward_max_abs": res_dist}
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["peak_memory_above_inputs_MiB"] = mem
    corner_bytes = HF * WF * D * A * B * 4 * C * 4
    res["sweep_corner_read_GB"] = corner_bytes / 1e9
    res["sweep_corner_read_TB_per_s_over_entry_median"] = corner_bytes / (res["entry_ms"]["median"] * 1e-3) / 1e12
    res["entry_faster_than_baseline_intervals_apart"] = res["entry_ms"]["max"] < res["baseline_ms"]["min"]
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
