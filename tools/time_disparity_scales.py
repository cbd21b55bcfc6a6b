"""Time the disparity-scales step of the depth module at upstream's size (S 4 scales of ratios 1, 2, 4, 8, 256 x 456 images, a mask with a
hole, znear 0.5, zfar 750; B 1 and 4), the fused HIP entries against the same mathematics in torch ops on the same GPU in the same run:

    python tools/time_disparity_scales.py [--window 0.5] [--repeats 7] [--out profiles/disparity_scales_times.json]
    tools/kstats.sh disparity_scales 8 -- python $PWD/tools/time_disparity_scales.py --kernels-only 50 [--batch 1]   (the kernels' own times)

  forward_hip             ops.disparity_scales (mcr_disparity_scales): depths, regularity values and error mask of all scales in one call
  forward_composite       networks.ManyDepth.disparity_scales_composite without a graph
  step_hip                DisparityScalesFunction forward, then the backward of sum(g * depth) + sum(c * reg) into the S disparity maps
  step_composite          the composite under autograd, forward and backward
  losses_hip              utility.macarons_utils.depth_scale_losses (the two fused entries) and the backward of depth_loss + regularity_loss
  losses_composite        disparity_scales_composite followed by reconstruction_loss_composite under autograd, the same two losses

The method is that of tools/time_reconstruction_loss.py: host clock between two device synchronisations over a window of calls, the same
inputs and workspace every call; the number of calls of a route is set once, from a first estimate, so that a window lasts about --window
seconds; one repeat times every route, the routes taking turns; the JSON keeps each repeat's mean and the median / min / max over the
repeats.  It also keeps the distance between the two routes' results (max |difference| / max |composite|; both are fp32; `step_d_disp` is
this entry's gradient alone, `losses_d_disp` goes through the reconstruction loss as well, where the two fp32 routes select or sample a
few pixels differently -- profiles/reconstruction_loss_times.json counts those -- and such a pixel's gradient differs by its whole size) and
`hip_faster_than_composite_intervals_apart`: the HIP route's whole interval lies below the composite's whole interval.  Reads nothing
outside the repository."""
import argparse
import json
import math
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from macarons_amd import ops  # noqa: E402
from macarons_amd.autograd import DisparityScalesFunction  # noqa: E402
from macarons_amd.networks import ManyDepth  # noqa: E402
from macarons_amd.utility import macarons_utils as mu  # noqa: E402

H, W, A, RATIOS = 256, 456, 2, (1, 2, 4, 8)
S = len(RATIOS)
ZNEAR, ZFAR, SSIM_FACTOR, PADDING, REGULARITY_FACTOR = 0.5, 750.0, 0.85, "border", 1e-3


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
    """Smooth images (sums of sinusoids), disparities of a ramp plus sinusoids drawn at each scale's own resolution (0.1 .. 0.9), sources
    turned 0.15 rad either way and a few hundredths of a unit off (the depths are about 1)."""
    gen = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")

    def image(n):
        k, th, ph = torch.rand(n, 3, 4, generator=gen) * 0.5 + 0.1, torch.rand(n, 3, 4, generator=gen) * 6.2832, torch.rand(n, 3, 4, generator=gen) * 6.2832
        arg = k[..., None, None] * (th.cos()[..., None, None] * xx + th.sin()[..., None, None] * yy) + ph[..., None, None]
        return (0.5 + 0.12 * arg.sin().sum(2)).clamp(0, 1).permute(0, 2, 3, 1).contiguous()

    def disparity(r):
        v, u = torch.meshgrid((torch.arange(H // r) + 0.5) / (H // r), (torch.arange(W // r) + 0.5) / (W // r), indexing="ij")
        out = []
        for b in range(B):
            ph = torch.rand(3, generator=gen) * 6.2832
            d = 0.5 + 0.3 * (u - 0.5) - 0.28 * (v - 0.5) + 0.012 * (torch.sin(4 * u + ph[0]) + torch.sin(5 * v + ph[1]) + torch.sin(3 * (u + v) + ph[2]))
            out.append(d + 0.01 * b)
        return torch.stack(out)[:, None].contiguous()

    images, alpha = image(B), image(B * A).reshape(B, A, H, W, 3)
    disps = [disparity(r) for r in RATIOS]
    mask = torch.ones(B, H, W, dtype=torch.bool)
    mask[:, 60:120, 100:220] = False
    R, T = torch.eye(3).expand(B, 3, 3), torch.zeros(B, 3)
    Ra = torch.stack([rot_y(0.15), rot_y(-0.15)]).expand(B, A, 3, 3)
    Ta = torch.tensor([[0.06, 0.0, 0.02], [-0.06, 0.02, 0.0]]).expand(B, A, 3)
    g = (2e-3 * torch.sin(0.37 * xx + 0.23 * yy)).expand(S, B, H, W).contiguous()
    c = torch.tensor([0.5 ** s for s in range(S)])
    to = lambda v: v.to(dev).contiguous()
    return [to(d) for d in disps], to(images), to(alpha), to(mask), (to(R), to(T), to(Ra), to(Ta)), to(g), to(c)


def measure(B, dev, window, repeats):
    disps, images, alpha, mask, (R, T, Ra, Ta), g, c = inputs(B, dev)
    params = SimpleNamespace(znear=ZNEAR, zfar=ZFAR, ssim_factor=SSIM_FACTOR, use_depth_mask=True, regularity_loss=True,
                             regularity_factor=REGULARITY_FACTOR)
    cameras, alpha_cameras = SimpleNamespace(R=R, T=T), SimpleNamespace(R=Ra.reshape(-1, 3, 3), T=Ta.reshape(-1, 3))
    cams = ManyDepth.pack_cameras(R, T, Ra, Ta)
    weights = torch.tensor([REGULARITY_FACTOR * 0.5 ** s for s in range(S)], device=dev)

    def leaves():
        return [d.detach().requires_grad_(True) for d in disps]

    def forward_composite():
        with torch.no_grad():
            return ManyDepth.disparity_scales_composite(disps, images, mask, ZNEAR, ZFAR)

    def step_hip():
        ls = leaves()
        depth, reg, _ = DisparityScalesFunction.apply(images, mask, ZNEAR, ZFAR, *ls)
        return torch.autograd.grad((depth * g).sum() + (reg * c).sum(), ls)

    def step_composite():
        ls = leaves()
        depth, reg, _ = ManyDepth.disparity_scales_composite(ls, images, mask, ZNEAR, ZFAR)
        return torch.autograd.grad((depth * g).sum() + (reg * c).sum(), ls)

    def losses_hip():
        ls = leaves()
        dl, rl, *_ = mu.depth_scale_losses(params, ls, images, alpha, mask, cameras, alpha_cameras, PADDING)
        return torch.autograd.grad(dl + rl, ls)

    def losses_composite():
        ls = leaves()
        depth, reg, _ = ManyDepth.disparity_scales_composite(ls, images, mask, ZNEAR, ZFAR)
        dl = ManyDepth.reconstruction_loss_composite(images, alpha, mask, cams, depth, ZFAR, SSIM_FACTOR, PADDING).sum()
        return torch.autograd.grad(dl + (reg * weights).sum(), ls)

    routes = {
        "forward_hip": lambda: ops.disparity_scales(disps, images, mask, ZNEAR, ZFAR),
        "forward_composite": forward_composite,
        "step_hip": step_hip,
        "step_composite": step_composite,
        "losses_hip": losses_hip,
        "losses_composite": losses_composite,
    }
    iters = {}
    for k, fn in routes.items():                         # warm-up, then the number of calls that fills a window
        for _ in range(3):
            fn()
        iters[k] = max(3, int(math.ceil(window / (timed(fn, 5) * 1e-3))))

    def far(a, b):
        return float((a.float() - b.float()).abs().max() / b.float().abs().max())

    f_hip, f_comp = routes["forward_hip"](), forward_composite()
    dist = {"depth": far(f_hip[0], f_comp[0]), "reg": far(f_hip[1], f_comp[1]),
            "error_mask_pixels_that_differ": int((f_hip[2] != f_comp[2]).sum()), "pixels": f_hip[2].numel(),
            "step_d_disp": max(far(a, b) for a, b in zip(step_hip(), step_composite())),
            "losses_d_disp": max(far(a, b) for a, b in zip(losses_hip(), losses_composite()))}
    runs = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            runs[k].append(timed(fn, iters[k]))
    res = {"iters": iters, "hip_vs_composite_rel": dist}
    for k, v in runs.items():
        s = sorted(v)
        res[k + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "runs": v}
    res["hip_faster_than_composite_intervals_apart"] = {k: res[k + "_hip_ms"]["max"] < res[k + "_composite_ms"]["min"]
                                                        for k in ("forward", "step", "losses")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disparity_scales_times.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_disparity_scales: no HIP device; a time is taken on the GPU or not at all")
    dev = torch.device("cuda:0")
    if a.kernels_only:
        disps, images, _, mask, _, g, c = inputs(a.batch, dev)
        for _ in range(a.kernels_only):
            ops.disparity_scales(disps, images, mask, ZNEAR, ZFAR)
            ops.disparity_scales_backward(disps, images, mask, ZNEAR, ZFAR, g, c)
        torch.cuda.synchronize()
        return
    res = {"size": dict(S=S, ratios=list(RATIOS), A=A, H=H, W=W, znear=ZNEAR, zfar=ZFAR, masked=True, padding_mode=PADDING,
                        ssim_factor=SSIM_FACTOR, regularity_factor=REGULARITY_FACTOR),
           "device": torch.cuda.get_device_name(0), "window_s": a.window, "repeats": a.repeats,
           "clock": "host, between device synchronisations"}
    for B in (1, 4):
        res[f"B{B}"] = measure(B, dev, a.window, a.repeats)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
