"""The operands, expected values and bounds of the fp32 linear layers' exact tests (tests/_linear_cases.py), checked on the CPU: the
split model is an exact three-way truncation; every exact case has its headroom; on the split-route classes the six kept plane
products sum to the exact product, the three dropped ones are zero and every kept product of the class is needed by at least a
quarter of the outputs (a GPU result that lost one cannot pass); the dropped products obey the derived 2^-21 bound on random and
on adversarial mantissas, which nearly attain it.  Prints (with -s) the headrooms, the shares of outputs each term decides and
the worst dropped-term ratio."""
import numpy as np
import pytest

import _linear_cases as lc


def _random_fp32(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 2.0 ** rng.integers(-60, 61, size=n)).astype(np.float32)
    return np.concatenate([x, rng.integers(0x3F800000, 0x40000000, size=n, dtype=np.uint32).view(np.float32)])


def test_split3_is_an_exact_truncating_split():
    x = np.concatenate([_random_fp32(200000, 0), lc.adversarial_mantissas(), np.float32([0.0, 1.0, -1.0, 3.0, 1 + 2.0 ** -8, 1 + 2.0 ** -16])])
    hi, mid, lo = lc.split3(x)
    x64, h64, m64, l64 = (t.astype(np.float64) for t in (x, hi, mid, lo))
    assert np.array_equal(h64 + m64 + l64, x64)
    for p in (hi, mid, lo):                                   # each piece is a bf16 number: 8 significant bits
        assert not (lc.bits(p) & np.uint32(0xFFFF)).any()
    assert np.array_equal(lc.bits(hi), lc.bits(x) & np.uint32(0xFFFF0000))
    # truncation: the pieces carry x's sign and shrink by 2^-8 each: |x - hi| < 2^-7 2^e, |x - hi - mid| < 2^-15 2^e
    assert np.all(h64 * x64 >= 0) and np.all(m64 * x64 >= 0) and np.all(l64 * x64 >= 0)
    e = 2.0 ** np.floor(np.log2(np.abs(x64[x64 != 0])))
    assert np.all(np.abs(m64 + l64)[x64 != 0] < 2.0 ** -7 * e) and np.all(np.abs(l64)[x64 != 0] < 2.0 ** -15 * e)
    # rounding hi to nearest instead would overshoot |x| on these
    assert np.all(np.abs(h64) <= np.abs(x64))


def test_dropped_terms_obey_the_derived_bound():
    """|mid lo' + lo mid' + lo lo'| < 2^-21 |x| |w| per product (the header of _linear_cases.py derives it), nearly attained."""
    worst = {}
    adv = lc.adversarial_mantissas()
    rnd = _random_fp32(300000, 1)
    for name, x, w in (("random", rnd, rnd[::-1].copy()), ("adversarial", np.repeat(adv, adv.size), np.tile(adv, adv.size))):
        (_, xm, xl), (_, wm, wl) = (tuple(p.astype(np.float64) for p in lc.split3(t)) for t in (x, w))
        d = np.abs(xm * wl + xl * wm + xl * wl)
        ratio = d / (np.abs(x.astype(np.float64)) * np.abs(w.astype(np.float64)))
        worst[name] = float(ratio.max() / lc.DROPPED_BOUND)
        assert np.all(ratio < lc.DROPPED_BOUND), name
    x1 = np.float32(1 + 2.0 ** -7 - 2.0 ** -23)
    hi, mid, lo = (float(p[0]) for p in lc.split3(np.float32([x1])))
    assert (hi, mid, lo) == (1.0, 2.0 ** -7 - 2.0 ** -15, 2.0 ** -15 - 2.0 ** -23)
    print(f"ERR dropped split terms / (2^-21 |x| |w|): random {worst['random']:.3f}, adversarial {worst['adversarial']:.3f}")
    assert worst["adversarial"] > 0.95 and worst["random"] > 0.125         # random data alone exceeds 2^-24 = 0.125 of the bound
    # and as a matrix product: the bound times the sum of magnitudes
    x, w, _, _ = lc.normal_case(64, 48, 136)
    assert np.all(np.abs(lc.dropped_terms(x, w)) < lc.DROPPED_BOUND * lc.magnitudes(x, w))
    full = x.astype(np.float64) @ w.astype(np.float64).T
    assert np.abs(lc.six_term(x, w) + lc.dropped_terms(x, w) - full).max() < 1e-13


@pytest.mark.parametrize("M,N,K", [(129, 33, 33), (1, 1, 1), (257, 125, 125), (130, 126, 4), (65531, 200, 20), (257, 512, 256), (16377, 256, 132),
                                   (2048, 128, 3), (16384, 4, 1), (65536, 4, 1)])
def test_integer_cases_have_headroom(M, N, K):
    x, w, b, r = lc.int_case(M, N, K)
    for t in (x, w, b, r):
        assert t.dtype == np.float32 and np.array_equal(t, np.round(t))
    h = lc.headroom(x, w, b, r)
    print(f"ERR headroom int M={M} N={N} K={K}: 2^{np.log2(h):.1f}")
    assert h < lc.LIMIT
    assert np.abs(x).max() == lc.INT_MAX or M * K < 100
    y = lc.exact_ref(x, w, b, r)
    assert np.array_equal(y, np.round(y)) and y.dtype == np.float32


@pytest.mark.parametrize("M,N,K", [(257, 65, 64), (4097, 63, 62), (16390, 5, 6), (16377, 256, 130)])
def test_integer_backward_cases_have_headroom(M, N, K):
    x, w, g, base = lc.int_backward_case(M, N, K)
    h = lc.backward_headroom(x, w, g, base)
    print(f"ERR headroom backward M={M} N={N} K={K}: 2^{np.log2(h):.1f}")
    assert h < lc.LIMIT
    dx, dw, db = lc.backward_ref(x, w, g, base)
    assert dx.shape == (M, K) and dw.shape == (N, K) and db.shape == (N,)
    # against the definition, on a few elements
    assert dw[N - 1, K - 1] == sum(float(g[m, N - 1]) * float(x[m, K - 1]) for m in range(M))
    assert db[0] == float(g[:, 0].astype(np.float64).sum()) and dx[M - 1, 0] == float(g[M - 1].astype(np.float64) @ w[:, 0]) + base[M - 1, 0]


@pytest.mark.parametrize("cls", sorted(lc.SPLIT_CLASSES))
@pytest.mark.parametrize("M,N,K,nt,xcd", lc.SPLIT_SHAPES)
def test_split_cases(cls, M, N, K, nt, xcd):
    assert lc.split_route(M, N, K) == (nt, xcd, lc.cdiv(M, 128))
    x, w, b, r = lc.split_case(cls, M, N, K)
    q = lc.split_quantum(cls)
    h = lc.headroom(x, w, b, r, q)
    assert h < lc.LIMIT, f"headroom 2^{np.log2(h):.2f}"
    # the plane products on a band of rows at either end (the operands are identically distributed; the headroom above is over all)
    rows = np.r_[0:min(M, 160), M - 96:M]
    xs, rs = x[rows], r[rows]
    full = xs.astype(np.float64) @ w.astype(np.float64).T
    kept = lc.plane_products(xs, w, lc.KEPT)
    assert np.array_equal(sum(kept.values()), full), "the six kept products do not sum to the exact product"
    assert np.array_equal(np.round(full / q) * q, full), "the product is no multiple of the quantum"
    px, pw = lc.planes64(xs), lc.planes64(w)
    for a, c in lc.DROPPED:                                   # zero term by term, not by cancellation
        assert not (np.abs(px[a]) @ np.abs(pw[c]).T).any(), f"dropped product {a}.{c} is not zero"
    y = lc.exact_ref(xs, w, b, rs)                            # asserts that the expected value is an fp32 number
    shares = {}
    for p in lc.KEPT:
        share = float((kept[p] != 0).mean())                  # outputs that come out wrong without this product
        if p in lc.SPLIT_CLASSES[cls]:
            shares[".".join(p)] = share
            assert share >= 0.25, f"product {p} decides only {share:.2f} of the outputs"
            assert np.array_equal(lc.six_term(xs, w, without=p), full - kept[p])
        else:
            assert share == 0.0, f"product {p} should be empty in class {cls}"
    print(f"ERR split case {cls} M={M} N={N} K={K}: headroom 2^{np.log2(h):.2f}, outputs decided by "
          + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()) + f", |y| max {np.abs(y).max():.4f}")


def test_routes_of_the_fp32_shapes():
    """The shapes of the GPU test reach the kernels they are there for (launch_linear's predicates, recomputed)."""
    want = {(129, 33, 33): ("generic", 1), (1, 1, 1): ("generic", 1), (257, 125, 125): ("generic", 1), (130, 126, 4): ("generic", 1),
            (16381, 200, 20): ("generic", 2), (32765, 200, 20): ("generic", 4), (65531, 200, 20): ("generic", 8),
            (257, 512, 256): ("deep", 1), (300, 1, 256): ("deep", 1), (129, 65, 132): ("deep", 1), (16377, 256, 132): ("deep", 2),
            (129, 64, 130): ("generic", 1), (2048, 128, 3): ("smallk", 0), (2048, 128, 4): ("smallk", 0), (16384, 4, 1): ("generic", 1), (65536, 4, 1): ("smallk", 0),
            (2047, 128, 3): ("generic", 1), (1000, 200, 20): ("generic", 1)}
    for (M, N, K), route in want.items():
        assert lc.split_route(M, N, K) is None
        assert lc.fp32_route(M, N, K) == route, (M, N, K, lc.fp32_route(M, N, K))
    assert lc.fp32_route(2048, 128, 3, ldy_mult4=False) == ("generic", 1)


def test_pow2_scales_stay_in_range():
    x, w, a, b = lc.pow2_case(8193, 512, 72)
    assert a.min() == -lc.POW2_MAX and a.max() == lc.POW2_MAX and b.min() == -lc.POW2_MAX and b.max() == lc.POW2_MAX
    assert np.abs(x).min() == lc.POW2_X_FLOOR and np.abs(w).min() >= lc.POW2_W_FLOOR and np.abs(x).max() < 8 and np.abs(w).max() < 8
    assert (np.abs(x) == lc.POW2_X_FLOOR).mean() < 1e-3                  # the floor touches a handful of elements
    xs, ws = np.ldexp(x, a[:, None]), np.ldexp(w, b[:, None])
    assert xs.dtype == np.float32 and np.abs(xs).min() >= 2.0 ** -30 and np.abs(ws).min() >= 2.0 ** -36
    assert -30 - 36 - 30 > -126 and 2 * (3 + 20) + 11 < 127               # lowest product bit, largest sum of K <= 2048 terms
