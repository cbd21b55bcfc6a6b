"""An independent fp64 model of the disparity-scales step (numpy, no code shared with macarons_amd): the S depths at full resolution, the S
edge-aware regularity values, the error-mask table of scale 0 with its threshold, and the analytic gradient for the disparities.  Also the
cases of the tests, their seeded inputs and the loaders of tests/golden/disparity_scales.npz.

With a = 1/znear - 1/zfar, b = 1/zfar, per scale s of ratio r (np.repeat is the nearest upsampling for these ratios):
  D = repeat(disp_s, r), depth = 1 / (a D + b), mu = mean of D per image, n = D / (mu + 1e-7), n = 0 outside the mask
  reg[s] = sum |n[y,x] - n[y,x+1]| e_x / (B H (W-1)) + sum |n[y,x] - n[y+1,x]| e_y / (B (H-1) W),  e = exp(-mean_c |I - I'|)
  tab[i,j] from P(i,j) = n_0[rho(i), rho(j)], rho(i) = reflect(i - 1), gathered with explicit index arrays; thr = mean + std (N - 1)
  d_disp_s[j] = sum over block j of (-a depth^2 d_depth + m G / (mu + eps)) - sum over the image of m G D / ((mu + eps)^2 H_s W_s)
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disparity_scales.npz")
ZNEAR, ZFAR = 0.5, 750.0                                  # upstream's configuration

# tag -> B, H, W, ratios, the mask hole (y0, y1, x0, x1) or None, the variants (masked?), the seed
CASES = {
    "a": dict(B=2, H=16, W=24, ratios=(1, 2, 4, 8), hole=(3, 9, 7, 15), variants=(True, False), seed=1),
    "b": dict(B=2, H=19, W=37, ratios=(1, 1), hole=(4, 11, 18, 30), variants=(True,), seed=2),
    "c": dict(B=1, H=40, W=72, ratios=(1, 2, 4, 8), hole=(10, 22, 30, 50), variants=(True,), seed=3),
    "d": dict(B=1, H=2, W=3, ratios=(1,), hole=None, variants=(False,), seed=4),
    "e": dict(B=2, H=16, W=24, ratios=(1,), hole=(5, 9, 4, 12), variants=(True,), seed=5, fully_masked=1),
    "f": dict(B=1, H=256, W=456, ratios=(1, 2, 4, 8), hole=(60, 120, 100, 220), variants=(True,), seed=6),      # GPU only, no golden
}
GOLDEN_TAGS = "abcde"
VARIANTS = [(t, m) for t in GOLDEN_TAGS for m in CASES[t]["variants"]]


def smooth_images(rng, B, H, W):
    """[B,H,W,3] float32: 0.5 + four sinusoids of amplitude 0.12 per image and channel, 0.1 .. 0.6 rad/pixel, clamped to [0, 1]."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.full((B, 3, H, W), 0.5)
    for i in range(B):
        for c in range(3):
            for _ in range(4):
                k, th, ph = rng.uniform(0.1, 0.6), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
                out[i, c] += 0.12 * np.sin(k * (np.cos(th) * xx + np.sin(th) * yy) + ph)
    return np.ascontiguousarray(np.clip(np.moveaxis(out, 1, -1), 0.0, 1.0).astype(np.float32))


def smooth_disparity(rng, B, Hs, Ws):
    """[B,Hs,Ws] float32 in (0.1, 0.9), drawn at this resolution: 0.5 + a ramp of 0.25 .. 0.35 per image side along each axis (either
    sign) + three sinusoids whose slopes together stay below the ramp's, so neighbours never tie."""
    v, u = np.meshgrid((np.arange(Hs) + 0.5) / Hs, (np.arange(Ws) + 0.5) / Ws, indexing="ij")
    out = np.empty((B, Hs, Ws))
    for i in range(B):
        gu, gv = rng.choice([-1.0, 1.0]) * rng.uniform(0.25, 0.35), rng.choice([-1.0, 1.0]) * rng.uniform(0.25, 0.35)
        d = 0.5 + gu * (u - 0.5) + gv * (v - 0.5)
        for _ in range(3):
            k, th, ph = rng.uniform(2.0, 6.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
            d += 0.012 * np.sin(k * (np.cos(th) * u + np.sin(th) * v) + ph)
        out[i] = d
    return np.ascontiguousarray(out.astype(np.float32))


def make_inputs(tag, seed=None):
    """The seeded inputs of a case: dict(disps [list of [B,H_s,W_s]], images [B,H,W,3], mask [B,H,W] bool), numpy."""
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    B, H, W = c["B"], c["H"], c["W"]
    images = smooth_images(rng, B, H, W)
    disps = [smooth_disparity(rng, B, H // r, W // r) for r in c["ratios"]]
    mask = np.ones((B, H, W), bool)
    if c["hole"] is not None:
        y0, y1, x0, x1 = c["hole"]
        mask[:, y0:y1, x0:x1] = False
    if "fully_masked" in c:
        mask[c["fully_masked"]] = False
    return dict(disps=disps, images=images, mask=mask)


def upstream_weights(rng, S, B, H, W):
    """The fixed upstream gradients of the golden: c [S] for reg and a smooth g [S,B,H,W] for depth, sized so that the two halves of the
    disparity gradient have comparable magnitudes."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    g = np.stack([[2e-3 * np.sin(0.37 * xx + 0.23 * yy + rng.uniform(0, 2 * np.pi)) for _ in range(B)] for _ in range(S)])
    return (0.5 ** np.arange(S)).astype(np.float32), g.astype(np.float32)


def _ab(znear, zfar):
    return 1.0 / znear - 1.0 / zfar, 1.0 / zfar


def _pair_weights(images):
    img = np.asarray(images, np.float64)
    ex = np.exp(-np.abs(img[:, :, :-1] - img[:, :, 1:]).sum(-1) / 3.0)       # [B,H,W-1]
    ey = np.exp(-np.abs(img[:, :-1] - img[:, 1:]).sum(-1) / 3.0)             # [B,H-1,W]
    return ex, ey


def _scale(disp, H, W, mask):
    d = np.asarray(disp, np.float64)
    r = H // d.shape[1]
    assert d.shape[1] * r == H and d.shape[2] * r == W
    D = np.repeat(np.repeat(d, r, axis=1), r, axis=2)
    den = D.reshape(D.shape[0], -1).sum(1) / (H * W) + 1e-7
    n = D / den[:, None, None]
    if mask is not None:
        n = np.where(mask, n, 0.0)
    return r, D, den, n


def forward(disps, images, mask, znear=ZNEAR, zfar=ZFAR):
    """dict(depth [S,B,H,W], reg [S], tab [B,H,W], thr [B], error_mask [B,H,W], n [S,B,H,W], ratios), fp64."""
    B, H, W, _ = images.shape
    a, b = _ab(znear, zfar)
    ex, ey = _pair_weights(images)
    depth, reg, ns, ratios = [], [], [], []
    for disp in disps:
        r, D, den, n = _scale(disp, H, W, mask)
        depth.append(1.0 / (a * D + b))
        reg.append((np.abs(n[:, :, :-1] - n[:, :, 1:]) * ex).sum() / (B * H * (W - 1)) + (np.abs(n[:, :-1] - n[:, 1:]) * ey).sum() / (B * (H - 1) * W))
        ns.append(n), ratios.append(r)
    # the table: P(i,j) = n_0[rho(i), rho(j)], rho(i) = reflect(i - 1); rows / columns 0 .. size of the padded copy are what it reads
    rho_y, rho_x = np.abs(np.arange(H + 1) - 1), np.abs(np.arange(W + 1) - 1)
    img = np.asarray(images, np.float64)

    def at(t, iy, ix):
        return t[:, iy][:, :, ix]

    r0, r1, c0, c1 = rho_y[:H], rho_y[1:], rho_x[:W], rho_x[1:]
    n0 = ns[0]
    wx = np.exp(-np.abs(at(img, r0, c0) - at(img, r0, c1)).sum(-1) / 3.0)
    wy = np.exp(-np.abs(at(img, r0, c0) - at(img, r1, c0)).sum(-1) / 3.0)
    tab = np.abs(at(n0, r0, c0) - at(n0, r0, c1)) * wx + np.abs(at(n0, r0, c0) - at(n0, r1, c0)) * wy
    flat = tab.reshape(B, -1)
    mean = flat.sum(1) / (H * W)
    thr = mean + np.sqrt(((flat - mean[:, None]) ** 2).sum(1) / (H * W - 1))
    return dict(depth=np.stack(depth), reg=np.array(reg), tab=tab, thr=thr, error_mask=tab < thr[:, None, None], n=np.stack(ns), ratios=ratios)


def gradient(disps, images, mask, d_depth, d_reg, znear=ZNEAR, zfar=ZFAR):
    """The S gradients [B,H_s,W_s] of sum(d_depth * depth) + sum(d_reg * reg), analytically; a half that is None is left out."""
    B, H, W, _ = images.shape
    a, b = _ab(znear, zfar)
    ex, ey = _pair_weights(images)
    out = []
    for s, disp in enumerate(disps):
        r, D, den, n = _scale(disp, H, W, mask)
        dD = np.zeros_like(D)
        if d_depth is not None:
            dD += -a * (1.0 / (a * D + b)) ** 2 * np.asarray(d_depth[s], np.float64)
        if d_reg is not None:
            G = np.zeros_like(D)
            sx = np.sign(n[:, :, :-1] - n[:, :, 1:]) * ex / (B * H * (W - 1))
            sy = np.sign(n[:, :-1] - n[:, 1:]) * ey / (B * (H - 1) * W)
            G[:, :, :-1] += sx
            G[:, :, 1:] -= sx
            G[:, :-1] += sy
            G[:, 1:] -= sy
            G *= float(d_reg[s])
            if mask is not None:
                G = np.where(mask, G, 0.0)
            dD += G / den[:, None, None] - ((G * D).reshape(B, -1).sum(1) / (den ** 2 * H * W))[:, None, None]
        out.append(dD.reshape(B, H // r, r, W // r, r).sum((2, 4)))
    return out


def conditions(disps, images, mask, znear=ZNEAR, zfar=ZFAR):
    """(the least |n[p] - n[p']| over every block border and mask-free neighbour pair of every scale, the largest share of undecided
    pixels of an image, whether the error mask of every not fully masked image holds both values, the undecided pixels [B,H,W])."""
    m = forward(disps, images, mask, znear, zfar)
    B, H, W = m["tab"].shape
    free = np.ones((B, H, W), bool) if mask is None else mask
    gap = np.inf
    for n, r in zip(m["n"], m["ratios"]):
        bx = (np.arange(1, W) % r == 0)[None, None, :] & free[:, :, :-1] & free[:, :, 1:]
        by = (np.arange(1, H) % r == 0)[None, :, None] & free[:, :-1] & free[:, 1:]
        for d, sel in ((np.abs(n[:, :, :-1] - n[:, :, 1:]), bx), (np.abs(n[:, :-1] - n[:, 1:]), by)):
            if sel.any():
                gap = min(gap, float(d[sel].min()))
    undecided = np.abs(m["tab"] - m["thr"][:, None, None]) < 1e-4 * m["thr"][:, None, None]
    both = all(bool(m["error_mask"][i].any()) and not bool(m["error_mask"][i].all()) for i in range(B) if free[i].any())
    return gap, float(undecided.reshape(B, -1).mean(1).max()), both, undecided


def rel(a, b):
    """max |a - b| over max |b| (0 when both are all zero)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    top = np.abs(b).max()
    err = np.abs(a - b).max()
    return float(err / top) if top > 0 else float(err)


def load_case(tag):
    """The stored inputs of a golden case: dict(disps, images, mask), numpy."""
    z = np.load(GOLDEN)
    S = len(CASES[tag]["ratios"])
    return dict(disps=[z[f"{tag}_disp{s}"] for s in range(S)], images=z[f"{tag}_images"], mask=z[f"{tag}_mask"])


def load_result(tag, masked):
    """The reference's results of a variant: depth, reg, tab, thr, error_mask, d_disp (list), c [S], g [S,B,H,W], distance (dict)."""
    z = np.load(GOLDEN)
    pre = f"{tag}_out_{'mask' if masked else 'nomask'}_"
    S = len(CASES[tag]["ratios"])
    out = {k: z[pre + k] for k in ("depth", "reg", "tab", "thr", "error_mask", "c", "g")}
    out["d_disp"] = [z[pre + f"d_disp{s}"] for s in range(S)]
    out["distance"] = dict(zip(("depth", "reg", "tab", "thr", "d_disp"), (float(v) for v in z[pre + "distance"])))
    return out
