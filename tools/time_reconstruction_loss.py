"""Time the depth module's photometric reconstruction loss at upstream's size (S 4 scales, 256 x 456 images, 2 sources, a mask with a
hole, border padding, ssim_factor 0.85; B 1 and 4), the fused HIP entries against the torch composite on the same GPU in the same run:

    python tools/time_reconstruction_loss.py [--window 0.5] [--repeats 7] [--out profiles/reconstruction_loss_times.json]
    tools/kstats.sh reconstruction_loss 8 -- python tools/time_reconstruction_loss.py --kernels-only 50 [--batch 1]   (the kernels' own times)

  forward_hip             ops.reconstruction_loss (mcr_reconstruction_loss), all S scales in one call
  forward_composite       networks.ManyDepth.reconstruction_loss_composite without a graph
  step_hip                ReconstructionLossFunction forward, then the backward of loss.sum() into the depth (HIP both ways)
  step_composite          the composite under autograd, forward and backward
  backward_hip            ops.reconstruction_loss_backward alone

The method is that of tools/time_cost_volume_backward.py: host clock between two device synchronisations over a window of calls, the
same inputs and workspace every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about
--window seconds; one repeat times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max
over the repeats.  It also keeps the distance between the two routes' losses and gradients (max |difference| / max |composite|; both are
fp32; a pixel near a tie of its two best sources may take either, so the gradient's distance is also given over the pixels whose 3x3
neighbourhood holds no pixel on which the two routes chose differently; among those, a pixel whose sample lies within rounding of a
source pixel boundary takes the slope of either bilinear cell -- such pixels are counted, beyond 1e-4, and the distance over all the
others is given beside the maximum), and `hip_faster_than_composite_intervals_apart`: the HIP
route's whole interval lies below the composite's whole interval.  Reads nothing outside the repository."""
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
from macarons_amd.autograd import ReconstructionLossFunction  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402

S, H, W, A = 4, 256, 456, 2
ZFAR, SSIM_FACTOR, PADDING = 50.0, 0.85, "border"


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def rot_y(angle):
    c, s = math.cos(angle), math.sin(angle)
    return torch.tensor([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def inputs(B, dev):
    """Smooth images (sums of sinusoids), a wavy depth per scale, sources turned 0.15 rad either way and a few tenths of a unit off."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gen = torch.Generator().manual_seed(7)

    def image(n):
        k, th, ph = torch.rand(n, 3, 4, generator=gen) * 0.5 + 0.1, torch.rand(n, 3, 4, generator=gen) * 6.2832, torch.rand(n, 3, 4, generator=gen) * 6.2832
        arg = k[..., None, None] * (th.cos()[..., None, None] * xx + th.sin()[..., None, None] * yy) + ph[..., None, None]
        return (0.5 + 0.12 * arg.sin().sum(2)).clamp(0, 1).permute(0, 2, 3, 1).contiguous()

    images, alpha = image(B), image(B * A).reshape(B, A, H, W, 3)
    depth = torch.stack([3.0 + 1.5 * torch.sin(0.03 * xx + 0.02 * yy + 0.4 * s) + 0.2 * b for s in range(S) for b in range(B)]).reshape(S, B, H, W)
    mask = torch.ones(B, H, W, dtype=torch.bool)
    mask[:, 60:120, 100:220] = False
    R, T = torch.eye(3).expand(B, 3, 3), torch.zeros(B, 3)
    Ra = torch.stack([rot_y(0.15), rot_y(-0.15)]).expand(B, A, 3, 3)
    Ta = torch.tensor([[0.3, 0.0, 0.1], [-0.3, 0.1, 0.0]]).expand(B, A, 3)
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta)
    return tuple(t.to(dev).contiguous() for t in (images, alpha, mask, cams, depth))


def measure(B, dev, window, repeats):
    images, alpha, mask, cams, depth = inputs(B, dev)
    ones = torch.ones(S, device=dev)

    def step_hip():
        d = depth.detach().requires_grad_(True)
        loss = ReconstructionLossFunction.apply(d, images, alpha, mask, cams, ZFAR, SSIM_FACTOR, PADDING, ops.COST_VOLUME_FOV_SCALE)
        return loss, torch.autograd.grad(loss.sum(), d)[0]

    def step_composite():
        d = depth.detach().requires_grad_(True)
        loss = ManyDepth.reconstruction_loss_composite(images, alpha, mask, cams, d, ZFAR, SSIM_FACTOR, PADDING)
        return loss, torch.autograd.grad(loss.sum(), d)[0]

    def forward_composite():
        with torch.no_grad():
            return ManyDepth.reconstruction_loss_composite(images, alpha, mask, cams, depth, ZFAR, SSIM_FACTOR, PADDING)

    routes = {
        "forward_hip": lambda: ops.reconstruction_loss(images, alpha, mask, cams, depth, ZFAR, SSIM_FACTOR, PADDING),
        "forward_composite": forward_composite,
        "backward_hip": lambda: ops.reconstruction_loss_backward(images, alpha, mask, cams, depth, ones, ZFAR, SSIM_FACTOR, PADDING),
        "step_hip": step_hip,
        "step_composite": step_composite,
    }
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(window / (timed(fn, 5) * 1e-3))))
    (l_hip, g_hip), (l_comp, g_comp) = step_hip(), step_composite()
    with torch.no_grad():
        i_hip = ops.reconstruction_loss(images, alpha, mask, cams, depth, ZFAR, SSIM_FACTOR, PADDING, return_map=True)[2]
        i_comp = ManyDepth.reconstruction_loss_composite(images, alpha, mask, cams, depth, ZFAR, SSIM_FACTOR, PADDING, return_map=True)[2]
    differ = i_hip.long() != i_comp
    away = F.max_pool2d(differ.float(), 3, 1, 1) == 0
    e = (g_hip - g_comp).abs() / g_comp.abs().max()
    far = (e > 1e-4) & away                              # where the two fp32 routes sample either side of a pixel boundary (a bilinear kink)
    dist = {"loss": float(((l_hip - l_comp).abs() / l_comp.abs().max()).max()), "d_depth_max": float(e.max()),
            "pixels_selected_differently": int(differ.sum()), "pixels": differ.numel(), "d_depth_max_away_from_them": float(e[away].max()),
            "pixels_beyond_1e-4_away_from_them": int(far.sum()), "d_depth_max_over_the_others": float(e[away & ~far].max())}
    runs = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            runs[k].append(timed(fn, iters[k]))
    res = {"iters": iters, "hip_vs_composite_rel": dist}
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["hip_faster_than_composite_intervals_apart"] = {"forward": res["forward_hip_ms"]["max"] < res["forward_composite_ms"]["min"],
                                                        "step": res["step_hip_ms"]["max"] < res["step_composite_ms"]["min"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruction_loss_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reconstruction_loss: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    if a.kernels_only:
        images, alpha, mask, cams, depth = inputs(a.batch, dev)
        ones = torch.ones(S, device=dev)
        for _ in range(a.kernels_only):
            ops.reconstruction_loss(images, alpha, mask, cams, depth, ZFAR, SSIM_FACTOR, PADDING)
            ops.reconstruction_loss_backward(images, alpha, mask, cams, depth, ones, ZFAR, SSIM_FACTOR, PADDING)
        torch.cuda.synchronize()
        return
    res = {"size": dict(S=S, A=A, H=H, W=W, padding_mode=PADDING, ssim_factor=SSIM_FACTOR, masked=True), "device": torch.cuda.get_device_name(0),
           "window_s": a.window, "repeats": a.repeats, "clock": "host, between device synchronisations"}
    for B in (1, 4):
        res[f"B{B}"] = measure(B, dev, a.window, a.repeats)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
