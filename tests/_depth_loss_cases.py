"""Seeded cases of the depth module's two loss stages (reconstruction_loss.hip, disparity_scales.hip) at the sizes where their kernels
take a path that the goldens' shapes do not reach, built on the CPU in the shape of the dicts that _reconstruction_model.load_case and
_disparity_model.make_inputs return, with the conditions on the inputs that make the fp64 models a fair reference for fp32 kernels.  The
conditions are properties of the inputs, read from the models alone, not measurements of a kernel: tests/test_reconstruction_loss_cpu.py
and tests/test_disparity_scales_cpu.py assert them for every case below, tests/test_reconstruction_loss_edges_gpu.py and
tests/test_disparity_scales_edges_gpu.py rely on them.  If a seed misses a condition, the seed changes, never the condition.

Reconstruction loss (two sources everywhere; smooth images, a wavy depth, a mask with a hole):
  tiles66      S 1, B 1, 32 x 528   66 tiles and 16 896 pixels = 264 a mask chunk: the second step of rl_finish_kernel's tile loop (t += 64)
                                    and of rl_mask_count_kernel's thread loop (i += 256)
  pairs6       S 3, B 2, 20 x 28    golden case a and a third depth: S B = 6, the second round of rl_finish_kernel's pair loop (i += 4) and
                                    its i * n_tiles offsets
  pairs6_dark  pairs6, mask[1] off  a fully masked image in a batch: 0 / (0 + 1e-7) forward, a norm of 1e7 times gates of 0 backward
  spill1       S 1, B 2, 17 x 33    H = W = 16 k + 1: a tile row and a tile column that hold only the image's last row / column, whose
                                    reflected partner (pixel size - 2) lies in the previous tile
  rows3        S 1, B 1, 3 x 18     H = 3: row 1 is both "pixel 1" and "pixel H - 2" and takes three padded rows (cys); a two-column spill

Disparity scales (B, H x W, ratios in the order given, the mask's hole):
  s8           2, 32 x 48, (1, 1, 2, 2, 4, 8, 16, 16)   DS_MAX_S = 8 scales (redf[wave][S + s], part_reg[.. 2S + k], nrm[s DS_R], val[s 256],
                                                         thread s of ds_means), ratio 16 twice (nb = 1: one thread sums 256 values), 2 x 3 tiles
  r16row       1, 16 x 32, (1, 16)                      a coarse map of ONE row (1 x 2)
  coarse0      2, 32 x 48, (16, 1, 4)                   scale 0 is not the full-resolution one: the table and the error mask are its
  tiles65      2, 80 x 208, (1, 2, 4, 8, 16)            65 tiles with B = 2: (b n_tiles + t) with t += 64 in ds_finish_kernel, and
                                                         ds_backward_mean_kernel for image 1
  flat         2, 16 x 32, (1, 4, 16), no mask          image 0 the constant 0.37 at every scale (every difference exactly 0, sign(0) = 0),
                                                         image 1 all zeros (den = 1e-7)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _disparity_model as dmodel                                      # noqa: E402
import _reconstruction_model as rmodel                                 # noqa: E402

# ---- what the cases are for, in the kernels' own numbers (asserted by the CPU tests: a later change of a tile edge or a chunk count
# cannot silently empty a case) -------------------------------------------------------------------------------------------------------
TILE = 16                        # RL_T and DS_T
FINISH_LANES = 64                # rl_finish_kernel and ds_finish_kernel: a lane adds tiles t, t + 64, ...
FINISH_WAVES = 4                 # rl_finish_kernel: a wave takes the (scale, image) pairs i, i + 4, ...
COUNT_CHUNKS, COUNT_THREADS = 64, 256                                  # rl_mask_count_kernel: RL_CNT_CHUNKS chunks an image, i += 256


def cdiv(a, b):
    return -(-a // b)


def n_tiles(H, W):
    return cdiv(H, TILE) * cdiv(W, TILE)


# ---- the reconstruction loss ------------------------------------------------------------------------------------------------------------
NEAR_TIE = 1e-3                  # a margin below this share of the map's maximum is a near-tie: either source is a valid selection
MAX_NEAR_TIES = 0.05             # the share of near-ties the golden comparison allows
MAX_KINKS = 0.02                 # test_upstream_width's cap on kink pixels
RECONSTRUCTION_TAGS = ("tiles66", "pairs6", "pairs6_dark", "spill1", "rows3")
# (padding, masked) of every case; pairs6_dark without its mask is pairs6 without its mask
RECONSTRUCTION_VARIANTS = {t: [(p, m) for p in ("border", "zeros") for m in ((True,) if t == "pairs6_dark" else (True, False))]
                           for t in RECONSTRUCTION_TAGS}
D_LOSS = {1: torch.tensor([0.75]), 3: torch.tensor([0.5, 1.0, 1.5])}


def wide_case(H=32, W=456):
    """One image of upstream's width, two sources turned 0.15 rad either way and a few tenths of a unit off; smooth images as the golden's
    (0.5 + four sinusoids of amplitude 0.12, 0.1 .. 0.6 rad/pixel), a wavy depth, a mask with a hole."""
    rng = np.random.default_rng(17)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def image(n):
        out = np.full((n, 3, H, W), 0.5)
        for i in range(n):
            for ch in range(3):
                for _ in range(4):
                    k, th, ph = rng.uniform(0.1, 0.6), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
                    out[i, ch] += 0.12 * np.sin(k * (np.cos(th) * xx + np.sin(th) * yy) + ph)
        return torch.from_numpy(np.clip(out, 0, 1).transpose(0, 2, 3, 1).astype(np.float32)).contiguous()

    def rot_y(t):
        return torch.tensor([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]], dtype=torch.float32)

    mask = torch.ones(1, H, W, dtype=torch.bool)
    mask[:, 8:20, 100:220] = False
    depth = torch.from_numpy((3.0 + 1.5 * np.sin(0.03 * xx + 0.2 * yy)).astype(np.float32))[None, None]
    return dict(images=image(1), alpha_images=image(2)[None], mask=mask, R=torch.eye(3)[None], T=torch.zeros(1, 3),
                R_alpha=torch.stack([rot_y(0.15), rot_y(-0.15)])[None], T_alpha=torch.tensor([[[0.3, 0.0, 0.1], [-0.3, 0.1, 0.0]]]),
                depth=depth, zfar=50.0, ssim_factor=0.85)


def _small_case(seed, B, H, W, hole):
    """S = 1, two sources: the poses of golden case a (its first B images), images as _disparity_model.smooth_images draws them, the
    golden generator's depth 3 + 1.5 sin(0.3 x + 0.2 y), + 0.7 on the second image, and a rectangular hole in the mask."""
    a = rmodel.load_case("a")
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.stack([3.0 + 1.5 * np.sin(0.3 * xx + 0.2 * yy) + 0.7 * (b == 1) for b in range(B)])[None]
    mask = torch.ones(B, H, W, dtype=torch.bool)
    y0, y1, x0, x1 = hole
    mask[:, y0:y1, x0:x1] = False
    images = torch.from_numpy(dmodel.smooth_images(rng, B, H, W))
    alpha = torch.from_numpy(dmodel.smooth_images(rng, 2 * B, H, W)).reshape(B, 2, H, W, 3)
    return dict(images=images, alpha_images=alpha, mask=mask, R=a["R"][:B].clone(), T=a["T"][:B].clone(), R_alpha=a["R_alpha"][:B].clone(),
                T_alpha=a["T_alpha"][:B].clone(), depth=torch.from_numpy(depth.astype(np.float32)), zfar=a["zfar"], ssim_factor=a["ssim_factor"])


def reconstruction_case(tag):
    """The inputs of a case as CPU tensors, in load_case's shape: images, alpha_images, mask, R, T, R_alpha, T_alpha, depth, zfar,
    ssim_factor."""
    if tag == "tiles66":
        return wide_case(32, 528)
    if tag in ("pairs6", "pairs6_dark"):
        c = rmodel.load_case("a")
        c["depth"] = torch.cat([c["depth"], c["depth"][:1] * 1.05 + 0.1]).contiguous()
        if tag == "pairs6_dark":
            c["mask"] = c["mask"].clone()
            c["mask"][1] = False
        return c
    if tag == "spill1":
        return _small_case(21, 2, 17, 33, (4, 9, 12, 25))
    if tag == "rows3":
        return _small_case(22, 1, 3, 18, (1, 2, 6, 10))
    raise KeyError(tag)


def model_args(c, masked):
    return (c["images"], c["alpha_images"], c["mask"] if masked else None, c["R"], c["T"], c["R_alpha"], c["T_alpha"])


def near_tie_share(m):
    """The share of pixels whose two best sources lie within NEAR_TIE of the map's maximum, from the model's forward."""
    return float((m["margin"] < NEAR_TIE * float(m["map"].max())).double().mean())


def kinks(c, m):
    """test_upstream_width's rule, from the model's forward m of an S = 1 case: the pixels [B,H,W] where an fp32 evaluation may take
    another bilinear cell or another sign of the L1 term than the model.  An fp32 coordinate of magnitude up to max(H, W) that went
    through eight roundings is within delta = 8 x 2^-24 x max(H, W) of the model's; a pixel with a source sample within delta of a
    source pixel boundary, or with |I - Iw| below delta x (the steepest slope of the source images) + 4 x 2^-24 in a channel, is a kink."""
    H, W = c["depth"].shape[-2:]
    delta = 8 * 2.0 ** -24 * max(H, W)
    al = c["alpha_images"].double()
    slope = max(float((al[:, :, 1:] - al[:, :, :-1]).abs().max()), float((al[:, :, :, 1:] - al[:, :, :, :-1]).abs().max()))
    xy, warped = m["parts"][0]["xy"], m["parts"][0]["warped"]
    kink = ((xy - xy.round()).abs() < delta).any(-1).any(1)
    kink |= ((c["images"].double()[:, None] - warped).abs() < delta * slope + 4 * 2.0 ** -24).any(-1).any(1)
    return kink


# ---- disparity scales ---------------------------------------------------------------------------------------------------------------------
MIN_GAP = 1e-4                   # tests/golden/make_golden_disparity_scales.py's own rule
MAX_UNDECIDED = 0.01
DISPARITY = {
    "s8":      dict(B=2, H=32, W=48, ratios=(1, 1, 2, 2, 4, 8, 16, 16), hole=(5, 20, 9, 30), variants=(True, False), seed=7),
    "r16row":  dict(B=1, H=16, W=32, ratios=(1, 16), hole=(3, 9, 7, 15), variants=(True, False), seed=8),
    "coarse0": dict(B=2, H=32, W=48, ratios=(16, 1, 4), hole=(5, 20, 9, 30), variants=(True, False), seed=9),
    "tiles65": dict(B=2, H=80, W=208, ratios=(1, 2, 4, 8, 16), hole=(20, 50, 60, 150), variants=(True, False), seed=10),
    "flat":    dict(B=2, H=16, W=32, ratios=(1, 4, 16), hole=None, variants=(False,), seed=11),
}
DISPARITY_TAGS = tuple(DISPARITY)
DISPARITY_VARIANTS = [(t, m) for t in DISPARITY_TAGS for m in DISPARITY[t]["variants"]]
FLAT_VALUE = 0.37


def disparity_inputs(tag):
    """The seeded inputs of a case in make_inputs's shape and drawing order: dict(disps [list of [B,H_s,W_s]], images [B,H,W,3],
    mask [B,H,W] bool), numpy.  flat: image 0 holds FLAT_VALUE at every scale, image 1 zeros."""
    c = DISPARITY[tag]
    rng = np.random.default_rng(c["seed"])
    B, H, W = c["B"], c["H"], c["W"]
    images = dmodel.smooth_images(rng, B, H, W)
    if tag == "flat":
        disps = [np.ascontiguousarray(np.stack([np.full((H // r, W // r), FLAT_VALUE), np.zeros((H // r, W // r))]).astype(np.float32))
                 for r in c["ratios"]]
    else:
        disps = [dmodel.smooth_disparity(rng, B, H // r, W // r) for r in c["ratios"]]
    mask = np.ones((B, H, W), bool)
    if c["hole"] is not None:
        y0, y1, x0, x1 = c["hole"]
        mask[:, y0:y1, x0:x1] = False
    return dict(disps=disps, images=images, mask=mask)


def disparity_weights(tag):
    """The upstream gradients of a case (c [S] for reg, g [S,B,H,W] for depth), seeded as the golden generator seeds them."""
    c = DISPARITY[tag]
    return dmodel.upstream_weights(np.random.default_rng(100 + c["seed"]), len(c["ratios"]), c["B"], c["H"], c["W"])


def reordered(inp, order):
    """The same maps in another order of the scales."""
    return dict(inp, disps=[inp["disps"][i] for i in order])
