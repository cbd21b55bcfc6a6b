"""An independent fp64 model of the disparity head (numpy, no code shared with macarons_amd): a reflection pad, a 3 x 3 convolution to one
output channel, a sigmoid -- forward and backward -- and the cases of the tests, their seeded inputs and the loader of
tests/golden/disparity_head.npz.

Forward: the padded array is built explicitly, xp = np.pad(x, 1, mode="reflect") on the two map axes, and
  z[b,i,j] = bias + sum_c sum_{di,dj in 0..2} weight[c,di,dj] xp[b,c,i+di,j+dj],   y = 1 / (1 + exp(-z)).
Backward, with g = d_y y (1 - y): d_bias = sum g; d_weight[c,di,dj] = sum g xp[b,c,i+di,j+dj]; the gradient of the PADDED array is
scattered, d_xp[b,c,i+di,j+dj] += weight[c,di,dj] g[b,i,j], and then folded back the way the pad unfolded: padded row 0 (row -1) onto row
1, padded row Hs+1 (row Hs) onto row Hs-2, then the columns likewise.  A scatter and a fold, where the kernel gathers.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disparity_head.npz")

# tag -> (B, C, Hs, Ws), seed.  The kernels' tiles: forward and d_x 16 x 4 pixels (32 x 8 from 256 such tiles on), d_weight 64 x 16.
CASES = {
    "a": dict(shape=(1, 1, 2, 2), seed=1),          # both mirrors of both axes land inside a two-pixel axis
    "b": dict(shape=(2, 3, 3, 5), seed=2),          # small and odd: row 1 is row Hs-2, it receives both mirrors
    "c": dict(shape=(1, 16, 17, 33), seed=3),       # whole tiles plus one row and one column: 4 * 4 + 1 rows (16 + 1 of the d_weight tile), 2 * 16 + 1 columns
    "d": dict(shape=(2, 128, 32, 57), seed=4),      # upstream's scale 4: the odd width, the largest C
    "e": dict(shape=(1, 16, 35, 50), seed=5),
    "f": dict(shape=(1, 512, 2, 3), seed=6),        # the channel cap
    "g": dict(shape=(1, 9, 129, 513), seed=7),      # the 32 x 8 tile (17 x 17 = 289 of them): 16 * 8 + 1 rows, 16 * 32 + 1 = 8 * 64 + 1 columns; two passes of its 8 channels
}
ALL_TAGS = "abcdefg"
GOLDEN_TAGS = "abcf"                                  # the cases small enough to commit


def pad(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")


def forward(x, weight, bias):
    """x [B,C,Hs,Ws], weight [C,3,3], bias [1] -> (z, y) [B,Hs,Ws], float64."""
    x, w = np.asarray(x, np.float64), np.asarray(weight, np.float64).reshape(-1, 3, 3)
    B, C, Hs, Ws = x.shape
    xp = pad(x)
    z = np.full((B, Hs, Ws), float(np.asarray(bias, np.float64).reshape(-1)[0]))
    for di in range(3):
        for dj in range(3):
            z += np.einsum("c,bcij->bij", w[:, di, dj], xp[:, :, di:di + Hs, dj:dj + Ws])
    return z, 1.0 / (1.0 + np.exp(-z))


def backward_from_g(x, weight, g):
    """(d_x [B,C,Hs,Ws], d_weight [C,3,3], d_bias [1]) of sum(g * z), float64."""
    x, w, g = np.asarray(x, np.float64), np.asarray(weight, np.float64).reshape(-1, 3, 3), np.asarray(g, np.float64)
    B, C, Hs, Ws = x.shape
    g = g.reshape(B, Hs, Ws)
    xp = pad(x)
    d_w = np.empty((C, 3, 3))
    d_xp = np.zeros_like(xp)
    for di in range(3):
        for dj in range(3):
            d_w[:, di, dj] = np.einsum("bij,bcij->c", g, xp[:, :, di:di + Hs, dj:dj + Ws])
            d_xp[:, :, di:di + Hs, dj:dj + Ws] += w[None, :, di, dj, None, None] * g[:, None]
    # fold the rows (padded index 0 is row -1, the image of row 1 = padded 2; padded Hs+1 is row Hs, the image of row Hs-2 = padded Hs-1) ...
    d_xp[:, :, 2] += d_xp[:, :, 0]
    d_xp[:, :, Hs - 1] += d_xp[:, :, Hs + 1]
    rows = d_xp[:, :, 1:Hs + 1]
    # ... then the columns of what is left
    rows[:, :, :, 2] += rows[:, :, :, 0]
    rows[:, :, :, Ws - 1] += rows[:, :, :, Ws + 1]
    return np.ascontiguousarray(rows[:, :, :, 1:Ws + 1]), d_w, np.array([g.sum()])


def backward(x, weight, y, d_y):
    y, d_y = np.asarray(y, np.float64), np.asarray(d_y, np.float64)
    return backward_from_g(x, weight, (d_y * y * (1.0 - y)).reshape(y.shape[0], y.shape[-2], y.shape[-1]))


def rel(a, b):
    """max |a - b| over max |b| (0 when both are all zero)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    top = np.abs(b).max()
    err = np.abs(a.reshape(b.shape) - b).max()
    return float(err / top) if top > 0 else float(err)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------------
def make_inputs(tag):
    """Real-valued: x ~ N(0,1), weight ~ N(0,1) 2 / sqrt(9 C) (z of unit order), bias, and the gradient g_out of y.  float32."""
    B, C, Hs, Ws = CASES[tag]["shape"]
    rng = np.random.default_rng(700 + CASES[tag]["seed"])
    f = np.float32
    return dict(x=rng.standard_normal((B, C, Hs, Ws)).astype(f), weight=(rng.standard_normal((C, 3, 3)) * 2.0 / np.sqrt(9.0 * C)).astype(f),
                bias=np.array([rng.uniform(-0.5, 0.5)], f), g_out=rng.standard_normal((B, Hs, Ws)).astype(f))


WEIGHT_UNIT = 2.0 ** -13                              # 9 * 512 = 4608 distinct multiples of it fit below 1
G_UNIT = 2.0 ** -6


def make_exact(tag):
    """Operands whose every partial sum is exact in fp32, in any order: x small integers (|x| <= 3, |x| <= 1 beyond 128 channels),
    weight[c,t] = +-(9 c + t + 1) 2^-13 -- distinct per tap and channel, the sign alternating --, bias 0.5; for the backward y = 0.5
    (y (1 - y) = 0.25 exactly) and d_y = k 2^-4, |k| <= 4, so g = k 2^-6."""
    B, C, Hs, Ws = CASES[tag]["shape"]
    rng = np.random.default_rng(900 + CASES[tag]["seed"])
    amp = 3 if C <= 128 else 1
    f = np.float32
    m = np.arange(1, 9 * C + 1, dtype=np.float64)
    weight = (m * np.where(np.arange(9 * C) % 2 == 0, 1.0, -1.0) * WEIGHT_UNIT).reshape(C, 3, 3)
    return dict(x=rng.integers(-amp, amp + 1, (B, C, Hs, Ws)).astype(f), weight=weight.astype(f), bias=np.array([0.5], f),
                y=np.full((B, Hs, Ws), 0.5, f), d_y=(rng.integers(-4, 5, (B, Hs, Ws)) * 2.0 ** -4).astype(f))


def exact_headroom(e):
    """The largest sum of magnitudes behind any output of the exact operands, in units of that output's smallest term: (z, d_x, d_weight,
    d_bias).  Below 2^24 every partial sum of every order is an integer multiple of the unit that fp32 holds exactly."""
    x, w, g = np.abs(e["x"].astype(np.float64)), np.abs(e["weight"].astype(np.float64)), np.abs(e["d_y"].astype(np.float64)) * 0.25
    bias = np.array([abs(float(e["bias"][0]))])
    z = forward(x, w, bias)[0].max() / WEIGHT_UNIT
    d_x, d_w, d_b = backward_from_g(x, w, g)
    return z, d_x.max() / (WEIGHT_UNIT * G_UNIT), d_w.max() / G_UNIT, d_b.max() / G_UNIT


# ---- the golden ---------------------------------------------------------------------------------------------------------------------------------
def load_golden(tag):
    """dict(x, weight, bias, g_out, y, d_x, d_weight, d_bias, distance = dict(y, d_x, d_weight, d_bias)) of a committed case: the reference
    layer's own results on the CPU in fp32 and their distance to this model."""
    z = np.load(GOLDEN)
    out = {k: z[f"{tag}_{k}"] for k in ("x", "weight", "bias", "g_out", "y", "d_x", "d_weight", "d_bias")}
    out["distance"] = dict(zip(("y", "d_x", "d_weight", "d_bias"), z[f"{tag}_distance"].tolist()))
    return out
