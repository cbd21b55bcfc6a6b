"""An independent fp64 model of the decoder's expansion layer (numpy, no code shared with macarons_amd, no convolution of torch's): a
transposed 3 x 3 convolution, ELU, a nearest resize, a channel concatenation, a reflection-padded 3 x 3 convolution, ELU -- and the cases of
the tests, their seeded inputs, the exact operands and the loader of tests/golden/expansion_layer.npz.

The transposed convolution is modelled as what its definition says, a SCATTER: input pixel (i,j) of channel ci adds x W[ci,co,ki,kj] to
pixel (i + ki, j + kj) of an (h+2) x (w+2) map, of which padding 1 keeps the middle h x w (the kernel gathers with a flipped kernel
instead).  The nearest rule is indexed here, source = min(floor(dst * scale), in - 1) with scale = in / out and the product in float32
(torch's mode='nearest'; tests/test_expansion_layer_cpu.py pins it against F.interpolate).  The reflection is an index list, [1, 0 .. n-1,
n-2]; the convolution is nine shifted channel contractions of the gathered array.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expansion_layer.npz")

# tag -> (B, Cin, Cmid, Cadd (None: no x_add), Cout, (h, w), (H, W)), seed.  The kernel's tiles, which the host chooses per launch from the
# launch's output (its channels Co = Cmid for the transposed convolution, Cout for the convolution): ROWS16, 4 x 32 pixels x 16 channels in
# chunks of 16 input channels, whenever Co <= 16; otherwise ROWS32, 4 x 32 pixels x 32 channels in chunks of 16, from 256 workgroups on,
# and SPLIT, 2 x 16 pixels x 16 channels in chunks of 32 divided among the waves, below.
CASES = {
    "a": dict(shape=(1, 1, 1, None, 1, (2, 2), (2, 2)), seed=1),          # both mirrors inside a two-pixel axis, no x_add, identity resize
    "b": dict(shape=(2, 3, 2, 3, 5, (3, 5), (7, 9)), seed=2),             # batch stride, odd sizes, non-integer ratios, no channel count a multiple of 4
    "c": dict(shape=(1, 8, 4, 4, 16, (8, 15), (16, 29)), seed=3),         # upstream's expansion5 geometry on few channels
    "d": dict(shape=(1, 20, 17, 3, 17, (9, 17), (17, 33)), seed=4),       # one past a 16-tile in pixels and in output channels (SPLIT: 4 * 2 + 1 rows), 20 concatenated channels
    "e": dict(shape=(2, 32, 16, 3, 16, (16, 29), (32, 57)), seed=5),      # expansion1's channel pattern, the 19-channel tail (ROWS16, two chunks)
    "f": dict(shape=(1, 512, 256, 256, 256, (8, 15), (16, 29)), seed=6),  # upstream's expansion5 itself: the channel caps, K 4608 (SPLIT, 16 chunks)
    "g": dict(shape=(1, 6, 4, 2, 4, (7, 5), (3, 4)), seed=7),             # an output smaller than the input
    # added to the issue's seven: one more than the tile in every tiled dimension, per tile
    "h": dict(shape=(1, 17, 16, 1, 16, (5, 33), (9, 65)), seed=8),        # ROWS16, both launches: 4 + 1 rows, 32 + 1 columns (then 2 * 4 + 1, 2 * 32 + 1), 16 + 1 input channels
    "i": dict(shape=(1, 33, 17, 16, 17, (3, 17), (5, 33)), seed=9),       # SPLIT, both launches: 2 + 1 rows, 16 + 1 columns, 16 + 1 output channels, 32 + 1 input channels
    "j": dict(shape=(2, 17, 33, 2, 33, (33, 225), (37, 231)), seed=10),   # ROWS32, both launches (288 and 320 workgroups): 8 * 4 + 1 rows, 7 * 32 + 1 columns, 32 + 1 output channels, 16 + 1 and 2 * 16 + 3 input channels
}
ALL_TAGS = "abcdefghij"
GOLDEN_TAGS = "abcdeg"
NEAREST_PAIRS = [(8, 16), (15, 29), (16, 32), (29, 57), (32, 64), (57, 114), (64, 128), (114, 228), (128, 256), (228, 456),
                 (1, 2), (2, 2), (3, 7), (5, 9), (7, 3), (15, 29)]


def nearest_index(n_in, n_out):
    """The source index of every destination index of an axis resized n_in -> n_out by torch's mode='nearest'."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1)


def reflect_index(n):
    """Indices of the reflection-padded axis (pad 1): positions -1 .. n -> 1, 0 .. n-1, n-2."""
    return np.array([1] + list(range(n)) + [n - 2])


def elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def forward(x, x_add, up_weight, up_bias, i_weight, i_bias, output_size):
    """-> dict(z1, u [B,Cmid,h,w], z2, y [B,Cout,H,W]), float64.  x_add None: no concatenation."""
    x, wu, bu = np.asarray(x, np.float64), np.asarray(up_weight, np.float64), np.asarray(up_bias, np.float64)
    wi, bi = np.asarray(i_weight, np.float64), np.asarray(i_bias, np.float64)
    B, Cin, h, w = x.shape
    H, W = output_size
    full = np.zeros((B, wu.shape[1], h + 2, w + 2))
    for ki in range(3):
        for kj in range(3):
            full[:, :, ki:ki + h, kj:kj + w] += np.einsum("bcij,cd->bdij", x, wu[:, :, ki, kj])
    z1 = full[:, :, 1:h + 1, 1:w + 1] + bu[None, :, None, None]
    u = elu(z1)
    c = u[:, :, nearest_index(h, H)][:, :, :, nearest_index(w, W)]
    if x_add is not None:
        c = np.concatenate((c, np.asarray(x_add, np.float64)), 1)
    cp = c[:, :, reflect_index(H)][:, :, :, reflect_index(W)]
    z2 = np.zeros((B, wi.shape[0], H, W)) + bi[None, :, None, None]
    for di in range(3):
        for dj in range(3):
            z2 += np.einsum("oc,bcij->boij", wi[:, :, di, dj], cp[:, :, di:di + H, dj:dj + W])
    return dict(z1=z1, u=u, z2=z2, y=elu(z2))


def rel(a, b):
    """max |a - b| over max |b|: `rel` of tests/_reconstruction_model.py, on arrays."""
    import torch
    from _reconstruction_model import rel as rel_
    b = np.asarray(b, np.float64)
    return rel_(torch.as_tensor(np.asarray(a, np.float64).reshape(b.shape)), torch.as_tensor(b))


def sizes(tag):
    B, Cin, Cmid, Cadd, Cout, (h, w), (H, W) = CASES[tag]["shape"]
    return B, Cin, Cmid, Cadd, Cout, h, w, H, W


def args_of(c):
    """The model's (and the entries') argument order."""
    return c["x"], c["x_add"], c["up_weight"], c["up_bias"], c["i_weight"], c["i_bias"], c["output_size"]


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------------
def make_inputs(tag):
    """Real-valued: features ~ N(0,1), weights ~ N(0,1) / sqrt(9 channels summed) (both pre-activations of unit order, so ELU's two
    branches both occur), biases uniform in (-0.5, 0.5).  float32; x_add None where the case has none."""
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = sizes(tag)
    rng = np.random.default_rng(1100 + CASES[tag]["seed"])
    f = np.float32
    Ctot = Cmid + (Cadd or 0)
    return dict(x=rng.standard_normal((B, Cin, h, w)).astype(f),
                x_add=None if Cadd is None else rng.standard_normal((B, Cadd, H, W)).astype(f),
                up_weight=(rng.standard_normal((Cin, Cmid, 3, 3)) / np.sqrt(9.0 * Cin)).astype(f), up_bias=rng.uniform(-0.5, 0.5, Cmid).astype(f),
                i_weight=(rng.standard_normal((Cout, Ctot, 3, 3)) / np.sqrt(9.0 * Ctot)).astype(f), i_bias=rng.uniform(-0.5, 0.5, Cout).astype(f),
                output_size=(H, W))


WEIGHT_UNIT = 2.0 ** -3


def make_exact(tag):
    """Operands whose every partial sum, in any order, is exact in fp32.  x: integers 0 .. 3, sparse where the sum is long (about 16
    non-zeros among the 9 Cin terms of an output); both weights +-m 2^-3 with m a seeded draw from 1 .. 7 (1 .. 3 from 1024 terms on):
    a sum of K <= 4608 products feeding a second such sum cannot hold K distinct integers below 2^24, so they are drawn, not
    enumerated -- a misplaced tap, channel or pixel still changes almost every output; up_bias lifts every z1 above zero (ELU is the
    identity there and u = z1 is exact, a multiple of 2^-3); x_add: integers 0 .. 3; i_bias is minus the median of the biasless z2 of
    its channel, rounded to 2^-6, so z2 takes both signs."""
    B, Cin, Cmid, Cadd, Cout, h, w, H, W = sizes(tag)
    rng = np.random.default_rng(1300 + CASES[tag]["seed"])
    f = np.float32
    Ctot = Cmid + (Cadd or 0)

    def weights(shape, terms):
        top = 7 if terms < 1024 else 3
        return rng.integers(1, top + 1, shape) * rng.choice((-1.0, 1.0), shape) * WEIGHT_UNIT

    x = rng.integers(0, 4, (B, Cin, h, w)) * (rng.random((B, Cin, h, w)) < min(1.0, 16.0 / (9.0 * Cin)))
    x_add = None if Cadd is None else rng.integers(0, 4, (B, Cadd, H, W)).astype(f)
    wu, wi = weights((Cin, Cmid, 3, 3), 9 * Cin), weights((Cout, Ctot, 3, 3), 9 * Ctot)
    zero_u, zero_i = np.zeros(Cmid), np.zeros(Cout)
    z1 = forward(x, x_add, wu, zero_u, wi, zero_i, (H, W))["z1"]
    bu = WEIGHT_UNIT - z1.min(axis=(0, 2, 3))                                   # the smallest z1 of every channel becomes 2^-3
    z2 = forward(x, x_add, wu, bu, wi, zero_i, (H, W))["z2"]
    bi = -np.round(np.median(z2, axis=(0, 2, 3)) / WEIGHT_UNIT ** 2) * WEIGHT_UNIT ** 2
    return dict(x=x.astype(f), x_add=x_add, up_weight=wu.astype(f), up_bias=bu.astype(f), i_weight=wi.astype(f), i_bias=bi.astype(f),
                output_size=(H, W))


def exact_headroom(e):
    """(z1, z2): the largest sum of magnitudes behind any pre-activation of the exact operands, the bias included, in units of its
    smallest term (2^-3 for z1, 2^-6 for z2: a weight times a u).  Below 2^24 every partial sum of every order is an integer multiple of
    the unit that fp32 holds exactly."""
    mag = forward(np.abs(e["x"]), None if e["x_add"] is None else np.abs(e["x_add"]), np.abs(e["up_weight"]), np.abs(e["up_bias"]),
                  np.abs(e["i_weight"]), np.abs(e["i_bias"]), e["output_size"])
    # u of the magnitudes bounds |u| of the operands (z1 > 0 there, so u = z1 <= the sum of its terms' magnitudes)
    return float(mag["z1"].max() / WEIGHT_UNIT), float(mag["z2"].max() / WEIGHT_UNIT ** 2)


# ---- the golden ---------------------------------------------------------------------------------------------------------------------------------
def load_golden(tag):
    """dict(x, x_add (None where absent), up_weight, up_bias, i_weight, i_bias, output_size, y, distance) of a committed case: the reference
    layer's own result on the CPU in fp32 and its distance to this model."""
    z = np.load(GOLDEN)
    out = {k: z[f"{tag}_{k}"] for k in ("x", "up_weight", "up_bias", "i_weight", "i_bias", "y")}
    out["x_add"] = z[f"{tag}_x_add"] if f"{tag}_x_add" in z.files else None
    out["output_size"] = tuple(int(v) for v in z[f"{tag}_output_size"])
    out["distance"] = float(z[f"{tag}_distance"])
    return out
