"""Closed-form fp64 statement of the depth module's plane sweep (CostVolumeBuilder.forward, macarons/networks/ManyDepth.py:207-297), in
torch on the CPU: the five steps spelled out with explicit index arithmetic and gathers -- no F.interpolate, no F.grid_sample, no shared
code with the product's composite (macarons_amd/networks/ManyDepth.py).  Differentiable in x and x_alpha.

  1. ray of image pixel (p, q) at depth d, target view -> world   (unproject_points, scaled_depth_input=False)
  2. world -> source view, w clamped by sign(w) max(|w|, 1e-8), grid coordinate g
  3. bicubic resize of the g image to Hf x Wf (align_corners=False, A = -0.75, clamped tap indices)
  4. bilinear sample of the source features at g (zeros padding, align_corners=False)
  5. mean over the sources, sum_c |mean - x| / C
"""
import math

import torch

FOV_SCALE = 1.0 / math.tan(math.radians(60.0) / 2)
DT = torch.float64


def _cubic_taps(n_in, n_out):
    """(indices [n_out,4] clamped, weights [n_out,4]) of a 1-D bicubic resize."""
    src = (torch.arange(n_out, dtype=DT) + 0.5) * (n_in / n_out) - 0.5
    fl = torch.floor(src)
    t = src - fl
    A = -0.75

    def near(z):                                         # |z| <= 1
        return ((A + 2) * z - (A + 3)) * z * z + 1

    def far(z):                                          # 1 < |z| < 2
        return ((A * z - 5 * A) * z + 8 * A) * z - 4 * A

    w = torch.stack((far(t + 1), near(t), near(1 - t), far(2 - t)), -1)
    idx = (fl.long()[:, None] + torch.arange(-1, 3)[None, :]).clamp(0, n_in - 1)
    return idx, w


def grid_coordinates(R, T, R_alpha, T_alpha, bins, H, W, Hf, Wf, fov_scale=FOV_SCALE):
    """Steps 1-3: (g [B,A,D,Hf,Wf,2] resized grid coordinates, w [B,A,D,H,W] the unclamped source-view depths of all pixels)."""
    R, T, Ra, Ta, d = R.to(DT), T.to(DT), R_alpha.to(DT), T_alpha.to(DT), bins.to(DT)
    B, A, D, s = Ra.shape[0], Ra.shape[1], d.numel(), fov_scale
    m, mf = min(H, W), min(Hf, Wf)
    ndc_x = (W / m - 2 * torch.arange(W, dtype=DT) / (m - 1))[None, :].expand(H, W)
    ndc_y = (H / m - 2 * torch.arange(H, dtype=DT) / (m - 1))[:, None].expand(H, W)
    dd = d.view(D, 1, 1)
    view = torch.stack((ndc_x * dd / s, ndc_y * dd / s, dd.expand(D, H, W)), -1)                       # [D,H,W,3]
    world = torch.einsum("bdhwj,bij->bdhwi", view[None] - T.view(B, 1, 1, 1, 3), R)                    # (view - T) R^T
    v = torch.einsum("bdhwi,baij->badhwj", world, Ra) + Ta.view(B, A, 1, 1, 1, 3)                      # world R_a + T_a
    w_raw = v[..., 2]
    w = (torch.sign(w_raw) + (w_raw == 0).to(DT)) * w_raw.abs().clamp(min=1e-8)
    g = torch.stack((-(mf / Wf) * s * v[..., 0] / w, -(mf / Hf) * s * v[..., 1] / w), -1)              # [B,A,D,H,W,2]
    iy, wy = _cubic_taps(H, Hf)
    ix, wx = _cubic_taps(W, Wf)
    g = (g[:, :, :, iy] * wy.view(Hf, 4, 1, 1)).sum(4)                                                  # rows:    [B,A,D,Hf,W,2]
    g = (g[:, :, :, :, ix] * wx.view(Wf, 4, 1)).sum(5)                                                  # columns: [B,A,D,Hf,Wf,2]
    return g, w_raw


def sample(x_alpha, g):
    """Step 4: x_alpha [B,A,C,Hf,Wf], g [B,A,D,Hf,Wf,2] -> [B,A,C,D,Hf,Wf]; a coordinate that is not finite samples nothing."""
    B, A, C, Hf, Wf = x_alpha.shape
    D = g.shape[2]
    px, py = ((g[..., 0] + 1) * Wf - 1) / 2, ((g[..., 1] + 1) * Hf - 1) / 2
    ok = torch.isfinite(px) & torch.isfinite(py) & (px > -1) & (px < Wf) & (py > -1) & (py < Hf)
    px, py = torch.where(ok, px, torch.zeros_like(px)), torch.where(ok, py, torch.zeros_like(py))
    x0, y0 = torch.floor(px), torch.floor(py)
    flat = x_alpha.to(DT).reshape(B, A, C, Hf * Wf)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xc, yc = x0 + dx, y0 + dy
            wgt = (1 - (px - xc).abs()) * (1 - (py - yc).abs())
            inside = ok & (xc >= 0) & (xc < Wf) & (yc >= 0) & (yc < Hf)
            idx = (yc.clamp(0, Hf - 1) * Wf + xc.clamp(0, Wf - 1)).long().reshape(B, A, 1, -1).expand(-1, -1, C, -1)
            val = torch.gather(flat, 3, idx).reshape(B, A, C, D, Hf, Wf)
            out = out + val * (wgt * inside.to(DT))[:, :, None]
    return out


def cost_volume(x, R, T, x_alpha, R_alpha, T_alpha, bins, H, W, fov_scale=FOV_SCALE):
    """-> [B,D,Hf,Wf] float64."""
    Hf, Wf = x.shape[-2:]
    g, _ = grid_coordinates(R, T, R_alpha, T_alpha, bins, H, W, Hf, Wf, fov_scale)
    smp = sample(x_alpha, g).mean(1)                                                                     # [B,C,D,Hf,Wf]
    return (smp - x.to(DT)[:, :, None]).abs().sum(1) / x.shape[1]


def forward(x, R, T, x_alpha, R_alpha, T_alpha, bins, H, W, weight, bias):
    """(res, cost volume): relu(conv2d(cat(x, cost volume), weight, bias, padding=1)) in fp64."""
    cv = cost_volume(x, R, T, x_alpha, R_alpha, T_alpha, bins, H, W)
    res = torch.relu(torch.nn.functional.conv2d(torch.cat((x.to(DT), cv), 1), weight.to(DT), bias.to(DT), padding=1))
    return res, cv


def tap_abs_w(R, T, R_alpha, T_alpha, bins, H, W, Hf, Wf):
    """[B,A,D,Hf,4,Wf,4]: |w| (unclamped) of the 16 bicubic taps of every output position, plane and source."""
    _, w = grid_coordinates(R, T, R_alpha, T_alpha, bins, H, W, Hf, Wf)
    iy, _ = _cubic_taps(H, Hf)
    ix, _ = _cubic_taps(W, Wf)
    return w.abs()[:, :, :, iy][:, :, :, :, :, ix]


def tap_min_abs_w(R, T, R_alpha, T_alpha, bins, H, W, Hf, Wf):
    """[B,D,Hf,Wf]: the smallest |w| among the 16 bicubic taps of every output position, over the sources."""
    return tap_abs_w(R, T, R_alpha, T_alpha, bins, H, W, Hf, Wf).amin(dim=(4, 6)).amin(1)


# ---- the committed golden (tests/golden/cost_volume.npz, written by tests/golden/make_golden_cost_volume.py) ----------------------
def load_case(tag):
    """One case of the golden as a dict of CPU tensors (+ H, W, D, out_ch ints and the state-dict names / shapes)."""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cost_volume.npz"))
    c = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + "_")}
    out = {k: torch.from_numpy(v) for k, v in c.items() if v.dtype.kind == "f"}
    out["H"], out["W"], out["D"], out["out_ch"] = (int(v) for v in c["dims"])
    out["state_keys"] = [str(k) for k in c["state_keys"]]
    out["state_shapes"] = [tuple(int(n) for n in row if n) for row in c["state_shapes"]]
    if "away" in c:
        out["away"] = tuple(int(v) for v in c["away"])
    return out


def rel(a, b):
    """max |a - b| over max |b|."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())
