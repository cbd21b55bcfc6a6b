"""Closed-form fp64 statement of the depth module's photometric reconstruction loss (upstream's reconstruction_loss_fn,
macarons/utility/macarons_utils.py:1120-1185, with reproject_depth_map / warp of ManyDepth.py:111-205 and SSIM of :809-842), in torch on
the CPU with explicit index arithmetic and gathers: no F.grid_sample, no pooling, no padding op, and no code shared with the product's
composite (macarons_amd/networks/ManyDepth.py).  Differentiable in depth.

  1. d = mask ? depth : zfar; pixel (p, q) at depth d, target view -> world -> source view (unproject_points, then view = world R + T)
  2. w clamped by sign(w) max(|w|, 1e-8), grid coordinate g, pixel coordinate (align_corners = False)
  3. bilinear sample, zeros, border or reflection padding; a coordinate that is not finite samples nothing
  4. l1 = mean_c |I - Iw|; ssim over the 3x3 windows of the reflection-padded images, moments centred on the window means
  5. f ssim + (1 - f) l1, min over the sources (lowest index on a tie) or a FORCED index map, masked sum of per-image means / plain mean

`force_index`: either source is a valid subgradient at a near-tie, so the model can follow a given selection instead of its own.
"""
import math
import os

import numpy as np
import torch

FOV_SCALE = 1.0 / math.tan(math.radians(60.0) / 2)
DT = torch.float64
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _reflect(n):
    """Indices of the reflection-padded axis (pad 1): positions -1 .. n -> 1, 0 .. n-1, n-2."""
    return torch.tensor([1] + list(range(n)) + [n - 2])


def _windows(img):
    """img [..., H, W] -> [..., H, W, 9]: the 3x3 window of every pixel of the reflection-padded image."""
    H, W = img.shape[-2:]
    pad = img.index_select(-2, _reflect(H)).index_select(-1, _reflect(W))
    return torch.stack([pad[..., i:i + H, j:j + W] for i in range(3) for j in range(3)], -1)


def ssim(x, y):
    """x, y [..., H, W] -> clamp((1 - n/d)/2, 0, 1) and the unclamped value."""
    wx, wy = _windows(x), _windows(y)
    mx, my = wx.mean(-1), wy.mean(-1)
    dx, dy = wx - mx[..., None], wy - my[..., None]
    sx, sy, sxy = (dx * dx).mean(-1), (dy * dy).mean(-1), (dx * dy).mean(-1)
    n = (2 * mx * my + C1) * (2 * sxy + C2)
    d = (mx ** 2 + my ** 2 + C1) * (sx + sy + C2)
    raw = (1 - n / d) / 2
    return raw.clamp(0, 1), raw


def warp(alpha_images, R, T, Ra, Ta, d, padding, fov_scale=FOV_SCALE):
    """alpha_images [B,A,H,W,3], d [B,H,W] -> (warped [B,A,H,W,3], unclamped w [B,A,H,W], inside [B,A,H,W]: some corner inside,
    pixel coordinates [B,A,H,W,2] before the padding rule)."""
    B, A, H, W, _ = alpha_images.shape
    R, T, Ra, Ta, s = R.to(DT), T.to(DT), Ra.to(DT), Ta.to(DT), fov_scale
    m = min(H, W)
    ndc_x = (W / m - 2 * torch.arange(W, dtype=DT) / (m - 1))[None, :].expand(H, W)
    ndc_y = (H / m - 2 * torch.arange(H, dtype=DT) / (m - 1))[:, None].expand(H, W)
    view = torch.stack((ndc_x * d / s, ndc_y * d / s, d), -1)                                            # [B,H,W,3]
    world = torch.einsum("bhwj,bij->bhwi", view - T.view(B, 1, 1, 3), R)                                 # (view - T) R^T
    v = torch.einsum("bhwi,baij->bahwj", world, Ra) + Ta.view(B, A, 1, 1, 3)
    w_raw = v[..., 2]
    w = (torch.sign(w_raw) + (w_raw == 0).to(DT)) * w_raw.abs().clamp(min=1e-8)
    gx, gy = -(m / W) * s * v[..., 0] / w, -(m / H) * s * v[..., 1] / w
    px, py = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    some = (px > -1) & (px < W) & (py > -1) & (py < H)
    raw_xy = torch.stack((px, py), -1).detach()                                                          # before any padding rule
    if padding == "zeros":
        ok = torch.isfinite(px) & torch.isfinite(py) & some
    elif padding == "border":
        ok = torch.isfinite(px) & torch.isfinite(py)
        zero, hx, hy = torch.zeros_like(px), torch.full_like(px, W - 1.0), torch.full_like(px, H - 1.0)
        px = torch.where(px <= 0, zero, torch.where(px >= W - 1, hx, px))                                # a held coordinate: gradient 0
        py = torch.where(py <= 0, zero, torch.where(py >= H - 1, hy, py))
    elif padding == "reflection":                                                                        # about -0.5 and size - 0.5
        ok = torch.isfinite(px) & torch.isfinite(py)

        def fold(p, n):
            a = (torch.where(ok, p, torch.zeros_like(p)) + 0.5).abs()
            flips = torch.floor(a.detach() / n)
            extra = a - flips * n
            r = torch.where(flips % 2 == 0, extra - 0.5, n - extra - 0.5)
            return torch.where(r <= 0, torch.zeros_like(r), torch.where(r >= n - 1, torch.full_like(r, n - 1.0), r))

        px, py = fold(px, W), fold(py, H)
    else:
        raise ValueError(padding)
    px, py = torch.where(ok, px, torch.zeros_like(px)), torch.where(ok, py, torch.zeros_like(py))
    x0, y0 = torch.floor(px.detach()), torch.floor(py.detach())
    flat = alpha_images.to(DT).reshape(B, A, H * W, 3)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xc, yc = x0 + dx, y0 + dy
            wgt = (1 - (px - xc).abs()) * (1 - (py - yc).abs())
            inside = ok & (xc >= 0) & (xc < W) & (yc >= 0) & (yc < H)
            idx = (yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)).long().reshape(B, A, H * W, 1).expand(-1, -1, -1, 3)
            val = torch.gather(flat, 2, idx).reshape(B, A, H, W, 3)
            out = out + val * (wgt * inside.to(DT))[..., None]
    return out, w_raw, some, raw_xy


def per_source(images, alpha_images, mask, R, T, Ra, Ta, depth, zfar, f, padding, fov_scale=FOV_SCALE):
    """One scale: depth [B,H,W] -> dict(loss_a [B,A,H,W], ssim_raw [B,A,H,W,3] or None, w [B,A,H,W], inside [B,A,H,W],
    xy [B,A,H,W,2], warped [B,A,H,W,3])."""
    depth = depth.to(DT)
    d = depth if mask is None else torch.where(mask, depth, torch.full_like(depth, float(zfar)))
    y, w_raw, inside, xy = warp(alpha_images, R, T, Ra, Ta, d, padding, fov_scale)
    x = images.to(DT)[:, None].expand_as(y)
    loss = (x - y).abs().mean(-1)
    raw = None
    if f > 0:
        s, raw = ssim(x.permute(0, 1, 4, 2, 3), y.permute(0, 1, 4, 2, 3))                                # [B,A,3,H,W]
        loss = f * s.mean(2) + (1 - f) * loss
        raw = raw.permute(0, 1, 3, 4, 2)
    return dict(loss_a=loss, ssim_raw=raw, w=w_raw, inside=inside, xy=xy, warped=y.detach())


def select(loss_a, force_index=None):
    """loss_a [B,A,H,W] -> (selected [B,H,W], index [B,H,W] long, margin [B,H,W]: second best minus best, inf for one source)."""
    A = loss_a.shape[1]
    best, idx = loss_a[:, 0], torch.zeros(loss_a[:, 0].shape, dtype=torch.long)
    for a in range(1, A):
        better = loss_a[:, a] < best
        best, idx = torch.where(better, loss_a[:, a], best), torch.where(better, torch.full_like(idx, a), idx)
    if A > 1:
        srt = loss_a.detach().sort(1).values
        margin = srt[:, 1] - srt[:, 0]
    else:
        margin = torch.full_like(best.detach(), float("inf"))
    if force_index is not None:
        idx = force_index.long()
        best = loss_a.gather(1, idx[:, None])[:, 0]
    return best, idx, margin


def reduce(sel, mask):
    if mask is None:
        return sel.mean()
    mk = mask.to(DT)
    return (sel * mk / (mk.sum((1, 2), keepdim=True) + 1e-7)).sum()


def reconstruction(images, alpha_images, mask, R, T, Ra, Ta, depth, zfar, f, padding, force_index=None, fov_scale=FOV_SCALE):
    """depth [S,B,H,W] -> dict(loss [S], map [S,B,H,W], index [S,B,H,W], margin [S,B,H,W], parts: the per_source dict of every scale).
    force_index [S,B,H,W] or None."""
    out = dict(loss=[], map=[], index=[], margin=[], parts=[])
    for k in range(depth.shape[0]):
        ps = per_source(images, alpha_images, mask, R, T, Ra, Ta, depth[k], zfar, f, padding, fov_scale)
        sel, idx, margin = select(ps["loss_a"], None if force_index is None else force_index[k])
        out["loss"].append(reduce(sel, mask)), out["map"].append(sel), out["index"].append(idx), out["margin"].append(margin)
        out["parts"].append(ps)
    for k in ("loss", "map", "index", "margin"):
        out[k] = torch.stack(out[k])
    return out


def gradient(images, alpha_images, mask, R, T, Ra, Ta, depth, zfar, f, padding, d_loss=None, force_index=None, fov_scale=FOV_SCALE):
    """d (sum_s d_loss[s] loss[s]) / d depth [S,B,H,W] in fp64 (d_loss None: ones)."""
    d6 = depth.detach().to(DT).requires_grad_(True)
    loss = reconstruction(images, alpha_images, mask, R, T, Ra, Ta, d6, zfar, f, padding, force_index, fov_scale)["loss"]
    wgt = torch.ones_like(loss) if d_loss is None else d_loss.to(DT)
    return torch.autograd.grad((loss * wgt).sum(), d6)[0]


# ---- the committed golden (tests/golden/reconstruction_loss.npz, written by tests/golden/make_golden_reconstruction_loss.py) ------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reconstruction_loss.npz")
VARIANTS = {"a": [(p, m) for p in ("border", "zeros") for m in (True, False)], "b": [("border", True), ("zeros", True)],
            "c": [("border", True)], "d": [("border", True), ("zeros", False)]}


def load_case(tag):
    """The inputs of a case as CPU tensors: images, alpha_images, mask, R, T, R_alpha, T_alpha, depth, zfar, ssim_factor."""
    z = np.load(GOLDEN)
    c = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + "_") and not k.startswith(tag + "_out_")}
    out = {k: torch.from_numpy(v) for k, v in c.items() if v.dtype.kind in "fb" and v.ndim}
    out["zfar"], out["ssim_factor"] = float(c["zfar"]), float(c["ssim_factor"])
    return out


def load_result(tag, padding, masked):
    """The reference's results of a variant: loss [S], d_depth [S,B,H,W], map [S,B,H,W], index [S,B,H,W]."""
    z = np.load(GOLDEN)
    pre = f"{tag}_out_{padding}_{'mask' if masked else 'nomask'}_"
    return {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}


def parameter_names():
    return [str(n) for n in np.load(GOLDEN)["parameter_names"]]


def rel(a, b):
    """max |a - b| over max |b|."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())
