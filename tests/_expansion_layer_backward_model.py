"""An independent fp64 model of the six gradients of the decoder's expansion layer (numpy; no torch autograd, no code of macarons_amd), the
cases of the backward's tests, their seeded d_y, the exact operands and the loader of tests/golden/expansion_layer_backward.npz.

The gradients are written as SCATTERS, the transposes of what tests/_expansion_layer_model.py's forward reads: every output pixel adds,
per tap, into the padded cell it read (a shifted slice of a padded array); every padded cell adds into the pixel that
model.reflect_index names; every resized pixel adds into the source that model.nearest_index names (a source that no pixel reads keeps
its zero); the transposed convolution, which the forward scatters, is gathered back from the padded map.  No ranges of destinations per
source are formed anywhere: that is what the kernel does, and what this model checks.  The two ELU derivatives come from the
pre-activations (exp(z) below zero), not from the outputs as in the kernel.

Cases (B, Cin, Cmid, Cadd, Cout, h x w -> H x W): a .. j are the forward's (CASES of the forward's model file); what they are to the
backward: a (2 x 2 -> 2 x 2) the two mirrors of an axis land on different pixels, no x_add; g (7 x 5 -> 3 x 4) H = 3, so row 1 takes both
mirrors, and the map shrinks, so most of u has no destination and d_u is zero there; b (3 x 5 -> 7 x 9, B 2) sources with two and three
destinations, the batch in the weight sums; f the channel caps; j 17 094 pixels in the weight sums; h / i / j one past each tile of the
two correlations.  The weight-gradient kernel has two tiles over (a channels) x (summed channels) x (4 rows x 32 columns of pixels) and
divides the B x tiles pixel tiles among `parts` workgroups, min(B tiles, ceil(1024 / channel blocks)) of them; its two passes are
(Cout, Cmid + Cadd) over H x W and (Cin, Cmid) over h x w:
  PIX, 16 x 16 channels (a side with at most 16 channels): h, 16 x 16+1 over 2*4+1 rows and 2*32+1 columns (9 parts) and 16+1 x 16 over
    4+1 rows and 32+1 columns (4 parts); one part: a, g (both passes).
  CHAN, 32 x 32 channels: k (1,33,33,1,33, 5x33 -> 5x33), added here: 32+1 x 32+2 and 32+1 x 32+1 channels over 4+1 rows and 32+1
    columns, four parts each; one part: i's second pass (33 x 17 channels over 3 x 17 pixels); j: 160 and 144 parts.
  more pixel tiles than parts, so that a workgroup walks several tiles and the last one fewer, added here:
    m (1,512,256,256,512, 17x5 -> 17x5), CHAN: 512 x 512 channels are 256 blocks, 3 parts for 5 tiles (2, 2, 1);
    n (1,4,8,8,512, 5x2 -> 130x3), PIX: 512 x 16 channels are 32 blocks, 17 parts for 33 tiles (2, 2, .. 1), the last tile two
    rows of four; W = 3, so column 1 takes both mirrors.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expansion_layer_model as model                                 # noqa: E402
from _expansion_layer_model import CASES, GOLDEN_TAGS, WEIGHT_UNIT, args_of, make_exact, make_inputs, rel, sizes   # noqa: E402,F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expansion_layer_backward.npz")

# make_inputs, make_exact and sizes look a tag up in the forward's table, so the backward's own cases are entered there (the forward's tests
# name their tags one by one and do not see them)
CASES.update({
    "k": dict(shape=(1, 33, 33, 1, 33, (5, 33), (5, 33)), seed=11),
    "m": dict(shape=(1, 512, 256, 256, 512, (17, 5), (17, 5)), seed=12),
    "n": dict(shape=(1, 4, 8, 8, 512, (5, 2), (130, 3)), seed=13),
})
ALL_TAGS = "abcdefghijkmn"
NAMES = ("d_x", "d_x_add", "d_up_weight", "d_up_bias", "d_i_weight", "d_i_bias")


def make_d_y(tag):
    """The seeded upstream gradient of a real-valued case: N(0,1), float32 [B,Cout,H,W]."""
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = sizes(tag)
    return np.random.default_rng(1500 + CASES[tag]["seed"]).standard_normal((B, Cout, H, W)).astype(np.float32)


def _scatter_axis(a, index, n, axis):
    """out[.., index[p], ..] += a[.., p, ..] along `axis`: a one-hot matrix per index list, contracted over the forward's own axis."""
    onehot = np.zeros((len(index), n))
    onehot[np.arange(len(index)), index] = 1.0
    return np.moveaxis(np.tensordot(a, onehot, axes=([axis], [0])), -1, axis)


def backward(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size, d_y):
    """-> dict of NAMES, float64 (d_x_add None without an x_add), and u, y of the forward."""
    f = model.forward(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size)
    x, wu, wi = np.asarray(x, np.float64), np.asarray(up_weight, np.float64), np.asarray(i_weight, np.float64)
    B, Cin, h, w = x.shape
    H, W = output_size
    Cmid = wu.shape[1]
    near_h, near_w, refl_h, refl_w = model.nearest_index(h, H), model.nearest_index(w, W), model.reflect_index(H), model.reflect_index(W)
    g2 = np.asarray(d_y, np.float64) * np.where(f["z2"] > 0, 1.0, np.exp(np.minimum(f["z2"], 0.0)))
    c = f["u"][:, :, near_h][:, :, :, near_w]
    if x_add is not None:
        c = np.concatenate((c, np.asarray(x_add, np.float64)), 1)
    cp = c[:, :, refl_h][:, :, :, refl_w]                              # what the convolution read
    d_wi, d_cp = np.zeros_like(wi), np.zeros_like(cp)
    for di in range(3):
        for dj in range(3):
            d_wi[:, :, di, dj] = np.einsum("boij,bkij->ok", g2, cp[:, :, di:di + H, dj:dj + W])
            d_cp[:, :, di:di + H, dj:dj + W] += np.einsum("boij,ok->bkij", g2, wi[:, :, di, dj])      # every pixel adds into the cell it read
    d_c = _scatter_axis(_scatter_axis(d_cp, refl_h, H, 2), refl_w, W, 3)                             # every cell into the pixel it mirrors
    d_u = _scatter_axis(_scatter_axis(d_c[:, :Cmid], near_h, h, 2), near_w, w, 3)                    # every pixel into its nearest source
    g1 = d_u * np.where(f["z1"] > 0, 1.0, np.exp(np.minimum(f["z1"], 0.0)))
    d_full = np.zeros((B, Cmid, h + 2, w + 2))                         # the (h+2) x (w+2) map the transposed convolution scatters into
    d_full[:, :, 1:h + 1, 1:w + 1] = g1
    d_wu, d_x = np.zeros_like(wu), np.zeros_like(x)
    for ki in range(3):
        for kj in range(3):
            d_wu[:, :, ki, kj] = np.einsum("bcij,bdij->cd", x, d_full[:, :, ki:ki + h, kj:kj + w])
            d_x += np.einsum("bdij,cd->bcij", d_full[:, :, ki:ki + h, kj:kj + w], wu[:, :, ki, kj])
    return dict(d_x=d_x, d_x_add=None if x_add is None else d_c[:, Cmid:], d_up_weight=d_wu, d_up_bias=g1.sum(axis=(0, 2, 3)),
                d_i_weight=d_wi, d_i_bias=g2.sum(axis=(0, 2, 3)), u=f["u"], y=f["y"], z1=f["z1"], z2=f["z2"])


# ---- exact operands -------------------------------------------------------------------------------------------------------------------------------
def make_exact_backward(tag):
    """(operands, d_y) whose every gradient is an integer multiple of a power of two that fp32 holds, in any order of summation: x, x_add
    and both weights as in make_exact (small integers; +-m 2^-3), up_bias as there (every z1 > 0, u = z1 a multiple of 2^-3), i_bias
    lifting every z2 above zero as well (the smallest z2 of a channel becomes 2^-6), so that both ELU derivatives are exactly 1; d_y small
    integers 0 .. 3, thinned where the sums are long: about 64 non-zeros per output channel over the pixels (the weight sums) and about 16
    among the 9 Cout terms behind an element of the data gradients, whichever is fewer, and never fewer than four in all."""
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = sizes(tag)
    e = dict(make_exact(tag))
    zero = np.zeros(Cout)
    z2 = model.forward(e["x"], e["x_add"], e["up_weight"], e["up_bias"], e["i_weight"], zero, (H, W))["z2"]
    e["i_bias"] = (WEIGHT_UNIT ** 2 - z2.min(axis=(0, 2, 3))).astype(np.float32)
    rng = np.random.default_rng(1700 + CASES[tag]["seed"])
    keep = min(1.0, 64.0 / (B * H * W), 16.0 / (9.0 * Cout))
    d_y = rng.integers(1, 4, (B, Cout, H, W)) * (rng.random((B, Cout, H, W)) < max(keep, 4.0 / (B * Cout * H * W)))
    if not d_y.any():
        d_y.reshape(-1)[::max(1, d_y.size // 4)] = 1
    return e, d_y.astype(np.float32)


# the smallest term of every gradient of the exact operands: d_y is an integer, u a multiple of 2^-3, a weight one of 2^-3
EXACT_UNITS = dict(d_x=WEIGHT_UNIT ** 2, d_x_add=WEIGHT_UNIT, d_up_weight=WEIGHT_UNIT, d_up_bias=WEIGHT_UNIT, d_i_weight=WEIGHT_UNIT, d_i_bias=1.0)


def exact_headroom_backward(e, d_y):
    """name -> the largest sum of magnitudes behind any element of that gradient of the exact operands, the pixel sums of the weight
    gradients included, in units of its smallest term (EXACT_UNITS): the model on the magnitudes (both derivatives are 1, so every
    gradient of the magnitudes is the sum of the magnitudes of its terms; it also bounds every intermediate that feeds it, g1, d_c and
    the padded correlation, because every weight is at least one unit).  Below 2^24 every partial sum of every order is exact in fp32."""
    mag = backward(np.abs(e["x"]), None if e["x_add"] is None else np.abs(e["x_add"]), np.abs(e["up_weight"]), np.abs(e["up_bias"]),
                   np.abs(e["i_weight"]), np.abs(e["i_bias"]), e["output_size"], np.abs(d_y))
    return {k: float(np.max(mag[k]) / EXACT_UNITS[k]) for k in NAMES if mag[k] is not None}


# ---- the golden -----------------------------------------------------------------------------------------------------------------------------------
def load_golden_backward(tag):
    """dict(d_y, the six gradients (d_x_add None where absent), distance: name -> float) of a committed case: the reference layer's own
    autograd on the CPU in fp32 and its distances to this model.  The inputs are make_inputs(tag)."""
    z = np.load(GOLDEN)
    out = {k: (z[f"{tag}_{k}"] if f"{tag}_{k}" in z.files else None) for k in ("d_y",) + NAMES}
    out["distance"] = {k: float(z[f"{tag}_{k}_distance"]) for k in NAMES if out[k] is not None}
    return out
