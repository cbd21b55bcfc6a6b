"""Operands, expected values and bounds of the fp32 linear layers' exact tests (test_linear_cases_cpu.py checks this file on the CPU,
test_linear_exact_gpu.py runs the kernels on it).  numpy only.  TEST INFRASTRUCTURE ONLY.

split3 is the bit-level model of split8 (lp_split.h): hi = x with its low 16 bits cleared, r = x - hi, mid = r with its low 16 bits
cleared, lo = r - mid.  Truncation, not rounding: the three pieces carry x's sign, hi + mid + lo == x, lo has at most 8 significant bits.

linear3_kernel keeps six of the nine plane products (KEPT, in the kernel's order) and drops three (DROPPED).  With truncation
|mid| < 2^-7 2^e and |lo| < 2^-15 2^e for |x| in [2^e, 2^(e+1)), so per product |mid lo'| + |lo mid'| + |lo lo'| < (2^-22 + 2^-22 + 2^-30)
2^e 2^e' <= DROPPED_BOUND |x| |w| with DROPPED_BOUND = 2^-21; x = w = 1 + 2^-7 - 2^-23 comes within 3 % of it.

Exact operands.  fp32 routes and the backward: small integers, every sum of magnitudes far below 2^24, so every partial sum in any
order is an integer fp32 holds and the result is the fp64 product's bit for bit.  Split route: three operand classes on the quantum
Q = 2^-16 --

    x3_wint   X = +-(a + b 2^-8 + c 2^-16), W integers      needs lo.hi, mid.hi, hi.hi
    xint_w3   X integers, W = +-(a + b 2^-8 + c 2^-16)      needs hi.lo, hi.mid, hi.hi
    x2_w2     X, W = +-(a + b 2^-8)                         needs mid.mid, mid.hi, hi.mid, hi.hi
    dense     X, W integers, every element non-zero         hi.hi alone: every K chunk of every tile carries weight

(a in {1, 2}; b, c in {0..3}; integers in -2..2): every plane product is a multiple of Q, the three dropped products are exactly
zero, and the sum of the magnitudes of all terms, bias and residual included, stays below 2^24 Q, so the six-term sum is the full
product, an fp32 value, in any summation order.  The operands are thinned (SPLIT_TERMS non-zero products per output on average) so
that the headroom holds at every K; headroom() measures it and both tests assert it before they compare anything.
"""
import numpy as np

Q = 2.0 ** -16                   # quantum of the split-route operands' products
U24 = 2.0 ** -24                 # unit roundoff of fp32
LIMIT = 2.0 ** 24                # sums of magnitudes (in quanta) below which every partial sum is exact in fp32
DROPPED_BOUND = 2.0 ** -21       # |mid.lo + lo.mid + lo.lo| < DROPPED_BOUND * sum |x| |w|  (derived in the header)
PLANES = ("hi", "mid", "lo")
KEPT = (("lo", "hi"), ("hi", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi"))     # (plane of X, plane of W), the kernel's order
DROPPED = (("mid", "lo"), ("lo", "mid"), ("lo", "lo"))
SPLIT_CLASSES = {"x3_wint": (("lo", "hi"), ("mid", "hi"), ("hi", "hi")), "xint_w3": (("hi", "lo"), ("hi", "mid"), ("hi", "hi")),
                 "x2_w2": (("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi")), "dense": (("hi", "hi"),)}
SPLIT_TERMS = 24                 # mean number of non-zero products per output of the thinned split-route operands


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _top16(x):
    return (bits(x) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x):
    """(hi, mid, lo) of float32 x, as split8 computes them."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = _top16(x)
    r = x - hi
    mid = _top16(r)
    return hi, mid, r - mid


def planes64(x):
    return dict(zip(PLANES, (p.astype(np.float64) for p in split3(x))))


def plane_products(x, w, pairs):
    """{(plane of x, plane of w): plane(x) plane(w)^T in fp64} for the given pairs."""
    px, pw = planes64(x), planes64(w)
    return {p: px[p[0]] @ pw[p[1]].T for p in pairs}


def six_term(x, w, without=None):
    """The product linear3_kernel forms, in fp64: the six kept plane products (all but `without`)."""
    return sum(v for p, v in plane_products(x, w, KEPT).items() if p != without)


def dropped_terms(x, w):
    return sum(plane_products(x, w, DROPPED).values())


def magnitudes(x, w, b=None, r=None):
    """B[m, n] = sum_k |x_mk| |w_nk| + |b_n| + |r_mn| in fp64."""
    B = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    if b is not None:
        B = B + np.abs(b.astype(np.float64))
    if r is not None:
        B = B + np.abs(r.astype(np.float64))
    return B


def headroom(x, w, b=None, r=None, quantum=1.0):
    """The largest sum of magnitudes of one output, in quanta; exact cases need it below LIMIT."""
    return float(magnitudes(x, w, b, r).max() / quantum)


def exact_ref(x, w, b=None, r=None):
    """fp64 product (exact: every sum of magnitudes is far below 2^53), + bias, + residual, as float32."""
    y = x.astype(np.float64) @ w.astype(np.float64).T
    if b is not None:
        y = y + b.astype(np.float64)
    if r is not None:
        y = y + r.astype(np.float64)
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y), "the expected value is not an fp32 number"
    return y32


# ---- integer operands: the fp32 routes and the backward --------------------------------------------------------------------------------
INT_MAX = 15                     # |x|, |w| <= 15: K = 256 terms sum to at most 2^15.9


def _ints(rng, shape, hi):
    return rng.integers(-hi, hi + 1, size=shape).astype(np.float32)


def int_case(M, N, K, seed=0):
    """(x [M, K], w [N, K], b [N], r [M, N]) of integers; b and r use more of the mantissa than the product does."""
    rng = np.random.default_rng([M, N, K, seed])
    return _ints(rng, (M, K), INT_MAX), _ints(rng, (N, K), INT_MAX), _ints(rng, N, 1000), _ints(rng, (M, N), 1000)


BWD_MAX = 7                      # |x|, |w|, |dY| <= 7: 2^15 rows sum to at most 2^20.6


def int_backward_case(M, N, K, seed=0):
    """(x [M, K], w [N, K], dY [M, N], base [M, K]) of integers."""
    rng = np.random.default_rng([M, N, K, seed, 1])
    return _ints(rng, (M, K), BWD_MAX), _ints(rng, (N, K), BWD_MAX), _ints(rng, (M, N), BWD_MAX), _ints(rng, (M, K), 1000)


def backward_ref(x, w, g, base=None):
    """(dX, dW, db) of sum((x w^T + b) * g), exact, as float32; dX on top of `base` when given."""
    x64, w64, g64 = (t.astype(np.float64) for t in (x, w, g))
    dx = g64 @ w64 + (0 if base is None else base.astype(np.float64))
    outs = dx, g64.T @ x64, g64.sum(0)
    for o in outs:
        assert np.array_equal(o.astype(np.float32).astype(np.float64), o)
    return tuple(o.astype(np.float32) for o in outs)


def backward_headroom(x, w, g, base=None):
    ax, aw, ag = (np.abs(t.astype(np.float64)) for t in (x, w, g))
    dx = ag @ aw + (0 if base is None else np.abs(base.astype(np.float64)))
    return float(max(dx.max(), (ag.T @ ax).max(), ag.sum(0).max()))


# ---- split-route operands --------------------------------------------------------------------------------------------------------------
def _three(rng, shape, with_c):
    a, b = rng.integers(1, 3, size=shape), rng.integers(0, 4, size=shape)
    c = rng.integers(0, 4, size=shape) if with_c else 0
    s = rng.integers(0, 2, size=shape) * 2 - 1
    v = s * (a + b * 2.0 ** -8 + c * 2.0 ** -16)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


def _thin(rng, a, keep):
    return a if keep >= 1.0 else np.where(rng.random(a.shape) < keep, a, np.float32(0)).astype(np.float32)


def split_case(cls, M, N, K, seed=0):
    """(x, w, b, r) of class `cls` (a key of SPLIT_CLASSES); b and r are integers, multiples of Q."""
    rng = np.random.default_rng([M, N, K, seed, sorted(SPLIT_CLASSES).index(cls)])
    if cls == "dense":
        x, w = (np.where(rng.random(s) < 0.5, np.float32(1), np.float32(-1)) * rng.integers(1, 3, size=s).astype(np.float32)
                for s in ((M, K), (N, K)))                  # +-1, +-2: the quantum is 1 here (split_quantum)
    else:
        gen = {"x3_wint": (lambda s: _three(rng, s, True), lambda s: _ints(rng, s, 2)),
               "xint_w3": (lambda s: _ints(rng, s, 2), lambda s: _three(rng, s, True)),
               "x2_w2": (lambda s: _three(rng, s, False), lambda s: _three(rng, s, False))}[cls]
        keep = min(1.0, np.sqrt(SPLIT_TERMS / K))
        x, w = _thin(rng, gen[0]((M, K)), keep), _thin(rng, gen[1]((N, K)), keep)
    return x, w, _ints(rng, N, 3), _ints(rng, (M, N), 3)


def split_quantum(cls):
    return 1.0 if cls == "dense" else Q


# ---- the routing predicates, recomputed from the constants quoted in launch_linear / linear3_applicable / launch_linear3 ---------------
def cdiv(a, b):
    return -(-a // b)


def split_route(M, N, K):
    """None when the packed, aligned call does not take linear3_kernel; else (column tiles per wave, XCD-aware order, row blocks).
    linear3_shape_ok: K % 8 == 0, K >= 64, N >= 128 (ld % 4 == 0 and 16-byte alignment are the caller's); linear3_applicable:
    cdiv(M, 128) * cdiv(N, 128) >= 256; launch_linear3: nt = 2 if K <= 512 else 4, halved while cdiv(M, 128) * cdiv(N, 32 nt) < 512;
    XCD order from 64 row blocks."""
    mb = cdiv(M, 128)
    if not (K % 8 == 0 and K >= 64 and N >= 128 and mb * cdiv(N, 128) >= 256):
        return None
    nt = 2 if K <= 512 else 4
    while nt > 1 and mb * cdiv(N, nt * 32) < 512:
        nt >>= 1
    return nt, mb >= 64, mb


# (M, N, K, column tiles per wave, XCD-aware order): the shapes of the split-route tests and the route each is there for
SPLIT_SHAPES = [
    (8192, 512, 72, 2, True),        # 64 row blocks: XCD order
    (8193, 512, 72, 2, True),        # 65 row blocks padded to 72: the `m0 >= M` exit
    (8100, 1024, 520, 4, True),      # K % 32 != 0: the last chunk is half empty
    (8065, 448, 1344, 1, True),      # the head's K
    (1000, 4096, 72, 2, False),      # row-block-fastest order, 8 row blocks
    (1000, 4032, 520, 1, False),
    (897, 4000, 64, 1, False),       # smallest K, N no multiple of 128
]


def fp32_route(M, N, K, ldy_mult4=True, aligned=True):
    """("smallk" | "deep" | "generic", column tiles) of a call that does not take the split route (launch_linear, route_rows = 0)."""
    if K <= 4 and N % 4 == 0 and ldy_mult4 and M * (N // 4) >= 65536:
        return "smallk", 0
    mb = cdiv(M, 128)
    deep = K >= 128 and K % 4 == 0 and mb * cdiv(N, 64) <= 512
    nt = 2 if deep else 8
    while nt > 1 and (nt // 2) * 32 >= N:
        nt >>= 1
    while nt > 1 and mb * cdiv(N, nt * 32) < 512:
        nt >>= 1
    return ("deep" if deep else "generic"), nt


# ---- real-valued operands and power-of-two scales ----------------------------------------------------------------------------------------
def normal_case(M, N, K, seed=0):
    rng = np.random.default_rng([M, N, K, seed, 2])
    return (rng.standard_normal((M, K)).astype(np.float32), (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32),
            rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32))


POW2_X_FLOOR, POW2_W_FLOOR, POW2_MAX = 2.0 ** -10, 2.0 ** -16, 20


def pow2_case(M, N, K, seed=0):
    """(x, w, a [M], b [N]): a normal_case whose smallest magnitudes are raised to POW2_X_FLOOR / POW2_W_FLOOR, and exponents in
    -POW2_MAX..POW2_MAX for the rows of x and of w.  The lowest bit of any kept plane product of the scaled operands is then at least
    2^-30 2^-36 2^-30 = 2^-96 (operand floors times 2^-20; 23 + 7 bits below the leading ones) and no sum exceeds
    2^26 2^26 K: everything stays a normal fp32 number, where scaling by a power of two is exact."""
    x, w, _, _ = normal_case(M, N, K, seed)
    floor = lambda t, lo: np.where(np.abs(t) < lo, np.copysign(np.float32(lo), t), t).astype(np.float32)
    rng = np.random.default_rng([M, N, seed, 3])
    return (floor(x, POW2_X_FLOOR), floor(w, POW2_W_FLOOR), rng.integers(-POW2_MAX, POW2_MAX + 1, size=M),
            rng.integers(-POW2_MAX, POW2_MAX + 1, size=N))


def adversarial_mantissas():
    """fp32 values whose mid and lo pieces are as large as truncation allows (all bits below hi's and below mid's set), with
    neighbours, over a few exponents and both signs."""
    base = np.array([0x3F80FFFF, 0x3F80FFFE, 0x3F81FFFF, 0x3FFFFFFF, 0x3F80FF7F, 0x3F807FFF, 0x3F8000FF, 0x3F800001], np.uint32).view(np.float32)
    assert base[0] == np.float32(1 + 2.0 ** -7 - 2.0 ** -23)
    return np.concatenate([s * base * np.float32(2.0 ** e) for e in (-20, -1, 0, 1, 20) for s in (np.float32(1), np.float32(-1))])
