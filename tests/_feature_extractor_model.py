"""An independent fp64 model of the front of the depth module's ResNet encoder (numpy, no code shared with macarons_amd, no convolution or
pooling of torch's): the 7 x 7 / 2 convolution, eval-mode BatchNorm, ReLU, the 3 x 3 / 2 max-pool, and the basic blocks of `layer1` --
and the cases of the tests, their seeded inputs, the exact operands and the loader of tests/golden/feature_extractor.npz.

The convolution is what its definition says: one shifted, strided slice of the zero-padded array per tap, contracted over the input
channels.  The pooling is an explicit maximum over the cells of every window that lie inside the map (no padding value takes part).
BatchNorm is (z - mean) / sqrt(var + eps) * weight + bias.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_extractor.npz")

# The stem kernel's tile: a workgroup owns 2 x 15 pooled pixels of one image and every output channel, a wave 16 output channels.
# tag -> (N0, N1, Cin, Cout, (H, W)), bias, seed.
STEM_CASES = {
    "a": dict(shape=(1, 0, 1, 1, (1, 1)), bias=False, seed=1),      # every tap but the centre is padding, one pooled pixel
    "b": dict(shape=(2, 1, 3, 5, (7, 9)), bias=False, seed=2),      # odd sizes, batch strides of both operands, channels no multiple of 4 or 16
    "c": dict(shape=(1, 2, 3, 64, (16, 30)), bias=False, seed=3),   # upstream's channels; Wc = 15 is odd: the last pooling window hangs over the edge
    "d": dict(shape=(1, 1, 6, 17, (9, 20)), bias=True, seed=4),     # a convolution bias; 16 + 1 output channels, K = 294 with a zero-padded tail
    "e": dict(shape=(0, 2, 8, 64, (5, 4)), bias=False, seed=5),     # no x, the channel caps
    # one more than the tile in every tiled dimension: 2 + 1 pooled rows, 15 + 1 pooled columns, 16 + 1 output channels
    "f": dict(shape=(1, 1, 3, 17, (10, 62)), bias=False, seed=6),
}
STEM_TAGS = "abcdef"

# tag -> (B, C, (H, W)), seed.  The tiles are the expansion layers' (tests/_expansion_layer_model.py): ROWS16 up to 16 channels, SPLIT
# below 256 workgroups of ROWS32, ROWS32 from there on.
BLOCK_CASES = {
    "a": dict(shape=(1, 1, (1, 1)), seed=11),
    "b": dict(shape=(2, 3, (5, 7)), seed=12),
    "c": dict(shape=(1, 64, (16, 29)), seed=13),
    "d": dict(shape=(1, 17, (9, 17)), seed=14),
    "e": dict(shape=(2, 33, (33, 225)), seed=15),                   # reaches the 32-channel tile: 288 workgroups
    "f": dict(shape=(1, 512, (8, 15)), seed=16),                    # the cap
}
BLOCK_TAGS = "abcdef"

# the whole extractor: (N0, N1, Cin, Cout, (H, W)) with two blocks: 32 x 57 -> 16 x 29 -> 8 x 15
EXTRACTOR_CASE = dict(shape=(1, 2, 3, 64, (32, 57)), n_blocks=2, seed=21)

# The golden: upstream's FeatureExtractor.forward, which takes one image operand (cat(x, x_more)), on the stem cases below without blocks
# and, tag 'x', on the extractor case with 16 channels instead of 64 and its two blocks (64 would be 600 KB of block weights).
GOLDEN_STEM_TAGS = "abcd"
GOLDEN_EXTRACTOR = dict(shape=(1, 2, 3, 16, (32, 57)), n_blocks=2, seed=31)
GOLDEN_TAGS = GOLDEN_STEM_TAGS + "x"


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def conv2d(x, weight, bias, stride, pad):
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    N, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((N, C, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    z = np.zeros((N, O, Ho, Wo))
    for di in range(kh):
        for dj in range(kw):
            tap = xp[:, :, di:di + stride * (Ho - 1) + 1:stride, dj:dj + stride * (Wo - 1) + 1:stride]
            z += np.matmul(weight[None, :, :, di, dj], tap.reshape(N, C, Ho * Wo)).reshape(N, O, Ho, Wo)   # the contraction over c
    if bias is not None:
        z += np.asarray(bias, np.float64)[None, :, None, None]
    return z


def batch_norm(z, bn, eps):
    weight, bias, mean, var = (np.asarray(v, np.float64)[None, :, None, None] for v in bn)
    return (z - mean) / np.sqrt(var + eps) * weight + bias


def max_pool(v):
    """3 x 3, stride 2, padding 1; only the cells inside the map take part."""
    N, C, H, W = v.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = np.full((N, C, Hp, Wp), -np.inf)
    for py in range(Hp):
        for px in range(Wp):
            ys = [y for y in (2 * py - 1, 2 * py, 2 * py + 1) if 0 <= y < H]
            xs = [x for x in (2 * px - 1, 2 * px, 2 * px + 1) if 0 <= x < W]
            out[:, :, py, px] = v[:, :, ys][:, :, :, xs].max(axis=(2, 3))
    return out


def stem(images, weight, bias, bn, eps):
    """images [N,Cin,H,W] -> dict(z (the convolution with its bias), pre (after BatchNorm), conv1 (after ReLU), pooled), float64."""
    z = conv2d(images, weight, bias, 2, 3)
    pre = batch_norm(z, bn, eps)
    conv1 = np.maximum(pre, 0.0)
    return dict(z=z, pre=pre, conv1=conv1, pooled=max_pool(conv1))


def block(x, w1, bn1, eps1, w2, bn2, eps2):
    """-> dict(z1, t, z2, pre (BN2 of z2, before the residual), y), float64."""
    x = np.asarray(x, np.float64)
    z1 = conv2d(x, w1, None, 1, 1)
    t = np.maximum(batch_norm(z1, bn1, eps1), 0.0)
    z2 = conv2d(t, w2, None, 1, 1)
    pre = batch_norm(z2, bn2, eps2)
    return dict(z1=z1, t=t, z2=z2, pre=pre, y=np.maximum(pre + x, 0.0))


def extractor(images, weight, bias, bn, eps, blocks):
    """-> dict(conv1, pooled, features)."""
    s = stem(images, weight, bias, bn, eps)
    y = s["pooled"]
    for blk in blocks:
        y = block(y, *blk)["y"]
    return dict(conv1=s["conv1"], pooled=s["pooled"], features=y)


def rel(a, b):
    """max |a - b| over max |b| (1 where b is all zero)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0


def images_of(c):
    """x and x_more of a case as the one batch the model (and upstream) takes."""
    return np.concatenate([v for v in (c["x"], c["x_more"]) if v is not None], 0)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------------
def _real_bn(rng, C):
    f = np.float32
    return (rng.uniform(0.5, 1.5, C).astype(f), rng.normal(0, 0.3, C).astype(f), rng.normal(0, 0.3, C).astype(f), rng.uniform(0.5, 1.5, C).astype(f))


def _real_block(rng, C):
    f = np.float32
    return ((rng.standard_normal((C, C, 3, 3)) / np.sqrt(9.0 * C)).astype(f), _real_bn(rng, C), 1e-5,
            (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9.0 * C)).astype(f), _real_bn(rng, C), 1e-5)


def _real_stem(rng, shape, bias):
    N0, N1, Cin, Cout, (H, W) = shape
    f = np.float32
    return dict(x=rng.uniform(0, 1, (N0, Cin, H, W)).astype(f) if N0 else None, x_more=rng.uniform(0, 1, (N1, Cin, H, W)).astype(f) if N1 else None,
                weight=(rng.standard_normal((Cout, Cin, 7, 7)) / np.sqrt(49.0 * Cin) * 4).astype(f),
                bias=rng.uniform(-0.5, 0.5, Cout).astype(f) if bias else None, bn=_real_bn(rng, Cout), eps=1e-5)


def make_stem_inputs(tag):
    """Real-valued: images uniform in (0,1), weights of unit-order pre-activations, BatchNorm vectors around the identity, eps 1e-5."""
    c = STEM_CASES[tag]
    return _real_stem(np.random.default_rng(2100 + c["seed"]), c["shape"], c["bias"])


def make_block_inputs(tag):
    """-> dict(x, block=(w1, bn1, eps1, w2, bn2, eps2)); x >= 0 as after a ReLU."""
    c = BLOCK_CASES[tag]
    B, C, (H, W) = c["shape"]
    rng = np.random.default_rng(2200 + c["seed"])
    return dict(x=np.abs(rng.standard_normal((B, C, H, W))).astype(np.float32), block=_real_block(rng, C))


def make_extractor_inputs(n_blocks=None):
    c = EXTRACTOR_CASE
    rng = np.random.default_rng(2300 + c["seed"])
    out = _real_stem(rng, c["shape"], False)
    blocks = [_real_block(rng, c["shape"][3]) for _ in range(c["n_blocks"])]
    out["blocks"] = blocks if n_blocks is None else blocks[:n_blocks]
    return out


def make_golden_inputs(tag):
    """The seeded inputs of a golden case, with `blocks`."""
    if tag != "x":
        return dict(make_stem_inputs(tag), blocks=[])
    c = GOLDEN_EXTRACTOR
    rng = np.random.default_rng(2700 + c["seed"])
    out = _real_stem(rng, c["shape"], False)
    out["blocks"] = [_real_block(rng, c["shape"][3]) for _ in range(c["n_blocks"])]
    return out


# ---- exact operands ------------------------------------------------------------------------------------------------------------------------------
WEIGHT_UNIT = 2.0 ** -3


def _exact_weights(rng, shape, terms):
    top = 7 if terms < 1024 else 3
    return rng.integers(1, top + 1, shape) * rng.choice((-1.0, 1.0), shape) * WEIGHT_UNIT


def _exact_bn(rng, z, quantiles, ks, variances, biases):
    """A BatchNorm with eps 0 whose scale is a power of two: weight +-2^k, var from `variances` (1 / sqrt(var) is 2, 1, 1/2 or 1/4), the mean
    the integer next to the quantile of z that leaves, after the sign of the scale, the share 1 - q of the channel positive, bias an integer.
    ks None: weight = +-sqrt(var), a scale of +-1 (a chain of layers then loses three bits a convolution, not seven)."""
    C = z.shape[1]
    var = rng.choice(variances, C)
    weight = rng.choice((-1.0, 1.0), C) * (np.sqrt(var) if ks is None else 2.0 ** rng.choice(ks, C))
    q = np.array([quantiles[c % len(quantiles)] for c in range(C)])
    q = np.where(weight > 0, q, 1 - q)
    mean = np.array([np.round(np.quantile(z[:, c], q[c])) for c in range(C)])
    return (weight, rng.choice(biases, C).astype(np.float64), mean, var)


def _as32(v):
    if isinstance(v, tuple):
        return tuple(_as32(u) for u in v)
    return None if v is None else np.asarray(v, np.float32)


def make_stem_exact(tag):
    """Operands whose every partial sum, in any order, is exact in fp32: images integers 0 .. 3, weights +-m 2^-3 with m from 1 .. 7, a
    convolution bias (case d) m 2^-3, BatchNorm as _exact_bn with eps 0 -- of every three channels one keeps half of its map positive, one a
    twentieth (whole pooling windows are negative before ReLU) and one most of it."""
    c = STEM_CASES[tag]
    N0, N1, Cin, Cout, (H, W) = c["shape"]
    rng = np.random.default_rng(2400 + c["seed"])
    x = rng.integers(0, 4, (N0, Cin, H, W)).astype(np.float64) if N0 else None
    x_more = rng.integers(0, 4, (N1, Cin, H, W)).astype(np.float64) if N1 else None
    weight = _exact_weights(rng, (Cout, Cin, 7, 7), 49 * Cin)
    bias = rng.integers(-8, 9, Cout) * WEIGHT_UNIT if c["bias"] else None
    z = conv2d(images_of(dict(x=x, x_more=x_more)), weight, bias, 2, 3)
    bn = _exact_bn(rng, z, (0.5, 0.95, 0.3), (-1, 0, 1), (0.25, 1.0, 4.0, 16.0), (-1, 0, 1))
    return dict(x=_as32(x), x_more=_as32(x_more), weight=_as32(weight), bias=_as32(bias), bn=_as32(bn), eps=0.0)


def _bound(inp, w, cbias, bn, stride, pad):
    """The largest sum of magnitudes behind any output of a convolution and its BatchNorm over the ACTUAL input: the products, the
    convolution's bias, the mean, times the scale, plus the BatchNorm's bias."""
    mag = conv2d(np.abs(inp), np.abs(np.asarray(w, np.float64)), None if cbias is None else np.abs(cbias), stride, pad)
    g, b, m, v = (np.abs(np.asarray(t, np.float64))[None, :, None, None] for t in bn)
    return (mag + m) * g / np.sqrt(v) + b


def stem_headroom(e):
    """_bound of the exact stem in units of its smallest term (2^-3 of a weight times 2^-3, the smallest scale).  Below 2^24 every partial
    sum of every order is a multiple of the unit that fp32 holds exactly."""
    return float(_bound(images_of(e), e["weight"], e["bias"], e["bn"], 2, 3).max() / (WEIGHT_UNIT * 2.0 ** -3))


def make_block_exact(tag):
    """x integers 0 .. 3, sparse where the sum is long (about 16 non-zeros among the 9 C terms of an output); both weights +-m 2^-3 (m from
    1 .. 7, 1 .. 3 from 1024 terms on); BN1 with scales 2^-3 .. 1 that leaves a fifth of t positive (t is a sparse multiple of 2^-6), BN2
    with its mean at the median of z2 and a bias of -2 .. 0, so that the residual x changes the sign of some outputs; eps 0."""
    c = BLOCK_CASES[tag]
    B, C, (H, W) = c["shape"]
    rng = np.random.default_rng(2500 + c["seed"])
    x = rng.integers(0, 4, (B, C, H, W)) * (rng.random((B, C, H, W)) < min(1.0, 16.0 / (9.0 * C)))
    w1, w2 = _exact_weights(rng, (C, C, 3, 3), 9 * C), _exact_weights(rng, (C, C, 3, 3), 9 * C)
    bn1 = _exact_bn(rng, conv2d(x, w1, None, 1, 1), (0.8,), (-1, 0), (1.0, 4.0, 16.0), (-1, 0))
    t = block(x, w1, bn1, 0.0, w2, bn1, 0.0)["t"]
    bn2 = _exact_bn(rng, conv2d(t, w2, None, 1, 1), (0.5,), (-1, 0, 1), (0.25, 1.0, 4.0, 16.0), (-2, -1, 0))
    return dict(x=_as32(x), block=(_as32(w1), _as32(bn1), 0.0, _as32(w2), _as32(bn2), 0.0))


def block_headroom(e):
    """(first, second): as stem_headroom for the two convolutions of an exact block, each over its ACTUAL input (x; then t, which is
    exact once the first bound holds), in units of 2^-6 (a weight times the smallest scale of BN1) and 2^-12 (t's unit times a weight times
    the smallest scale of BN2); the second includes the residual."""
    x = np.asarray(e["x"], np.float64)
    w1, bn1, _, w2, bn2, _ = e["block"]
    t = block(x, *e["block"])["t"]
    return float(_bound(x, w1, None, bn1, 1, 1).max() / 2.0 ** -6), float((_bound(t, w2, None, bn2, 1, 1) + x).max() / 2.0 ** -12)


def make_extractor_exact(n_blocks=None):
    """The exact stem of EXTRACTOR_CASE followed by exact blocks, each drawn for the map before it.  Every BatchNorm has a scale of +-1
    (weight = +-sqrt(var)), so the unit of the map shrinks by the 2^-3 of a weight per convolution only: 2^-3 after the stem, 2^-15 after
    the second block; and seven of eight of the blocks' weights are zero (m = 0), because five dense convolutions in a row gain five bits
    each -- the dense weights are the block cases' business.  Every block's BN1 keeps a twentieth of t positive, which keeps the sums short."""
    c = EXTRACTOR_CASE
    rng = np.random.default_rng(2600 + c["seed"])
    N0, N1, Cin, Cout, (H, W) = c["shape"]
    variances = (0.25, 1.0, 4.0, 16.0)
    x, x_more = rng.integers(0, 4, (N0, Cin, H, W)).astype(np.float64), rng.integers(0, 4, (N1, Cin, H, W)).astype(np.float64)
    images = np.concatenate((x, x_more), 0)
    weight = _exact_weights(rng, (Cout, Cin, 7, 7), 49 * Cin)
    bn = _exact_bn(rng, conv2d(images, weight, None, 2, 3), (0.97, 0.98, 0.95), None, variances, (-1, 0))
    out = dict(x=_as32(x), x_more=_as32(x_more), weight=_as32(weight), bias=None, bn=_as32(bn), eps=0.0, blocks=[])
    y = stem(images, weight, None, bn, 0.0)["pooled"]
    for _ in range(c["n_blocks"] if n_blocks is None else n_blocks):
        w1, w2 = (_exact_weights(rng, (Cout, Cout, 3, 3), 1024) * (rng.random((Cout, Cout, 3, 3)) < 0.125) for _ in range(2))
        bn1 = _exact_bn(rng, conv2d(y, w1, None, 1, 1), (0.95,), None, variances, (-1, 0))
        t = block(y, w1, bn1, 0.0, w2, bn1, 0.0)["t"]
        bn2 = _exact_bn(rng, conv2d(t, w2, None, 1, 1), (0.9,), None, variances, (-1, 0))
        blk = (_as32(w1), _as32(bn1), 0.0, _as32(w2), _as32(bn2), 0.0)
        y = block(y, *blk)["y"]
        out["blocks"].append(blk)
    return out


def extractor_headroom(e):
    """_bound of every convolution of the exact extractor over its actual input (the residual included), in units of 2^-3 per
    convolution so far: one figure for the stem and two per block."""
    images = images_of(e)
    rooms = [float(_bound(images, e["weight"], None, e["bn"], 2, 3).max() / WEIGHT_UNIT)]
    y = stem(images, e["weight"], None, e["bn"], 0.0)["pooled"]
    for i, blk in enumerate(e["blocks"]):
        r = block(y, *blk)
        rooms.append(float(_bound(y, blk[0], None, blk[1], 1, 1).max() / WEIGHT_UNIT ** (2 * i + 2)))
        rooms.append(float((_bound(r["t"], blk[3], None, blk[4], 1, 1) + y).max() / WEIGHT_UNIT ** (2 * i + 3)))
        y = r["y"]
    return rooms


def is_fp32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


# ---- the golden ---------------------------------------------------------------------------------------------------------------------------------
def load_golden(tag):
    """A committed case of upstream's own FeatureExtractor.forward on the CPU in fp32: dict(x, x_more, weight, bias, bn, eps, blocks,
    features, distance); tag: one of GOLDEN_TAGS."""
    z = np.load(GOLDEN)
    has = lambda k: f"{tag}_{k}" in z.files                       # noqa: E731
    get = lambda k: z[f"{tag}_{k}"]                                # noqa: E731
    bn_of = lambda p: tuple(get(f"{p}_{k}") for k in ("weight", "bias", "mean", "var"))   # noqa: E731
    blocks = [(get(f"b{i}_w1"), bn_of(f"b{i}_bn1"), float(get(f"b{i}_eps1")), get(f"b{i}_w2"), bn_of(f"b{i}_bn2"), float(get(f"b{i}_eps2")))
              for i in range(int(get("n_blocks")))]
    return dict(x=get("x") if has("x") else None, x_more=get("x_more") if has("x_more") else None, weight=get("weight"),
                bias=get("bias") if has("bias") else None, bn=bn_of("bn"), eps=float(get("eps")), blocks=blocks, features=get("features"),
                distance=float(get("distance")))
