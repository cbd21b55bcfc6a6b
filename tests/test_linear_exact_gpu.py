"""mcr_linear and mcr_linear_backward bit for bit: every route behind the two entries, every product of the split route.

The other tests of these entries use standard-normal operands and a bar relative to the LARGEST output (2e-5): a split product that
lost one of its 2^-16-class terms, a wrong row at a tile edge that happens to be small, a K group dropped from a half-empty chunk of
sparse data all pass it.  Here (operands and expected values from tests/_linear_cases.py, checked on the CPU by
test_linear_cases_cpu.py; calls through ctypes on the guarded arenas of tests/_strided.py):

  exact operands      the result must equal the fp64 product's bits: integers on the fp32 routes (linear_kernel<1|2|4|8, 32>,
                      linear_kernel<1|2, 128>, linear_smallk_kernel) and on the backward (vb_gemm / vb_reduce / vb_transpose and the
                      deep kernels under dX); three operand classes on the split route (linear3_kernel<1|2|4>, both block orders),
                      each of which needs a different subset of the six plane products and zeroes the three dropped ones
  invariances         real-valued data, bit for bit: rows of X and W times powers of two; the small-K kernel against the matrix path;
                      the split and the generic kernel across tile widths, block orders and M
  componentwise bound real-valued data, |y - ref| <= (K + 3) 2^-24 (sum_k |x||w| + |b| + |r|) element by element, against the fp64
                      product on the fp32 routes and against the six-term model on the split route (+ 2^-21 of the same sum
                      against the full product), also with rows scaled by 2^-10 and 2^10

Every output starts as the arena's fill; guards and inputs are checked after every call.  Shares of the bounds are printed with the
ERR prefix.  Measured on an MI355X: zero differing bits in every exact and invariance case (GELU after the small-K kernel included);
the shares of the componentwise bounds are in the docstrings of the two bound tests, 0.45 at the worst (K = 3), 0.07 on the split route.
"""
import ctypes

import numpy as np
import pytest
import torch

import _linear_cases as lc
from _strided import Arena, Workspace

pytestmark = pytest.mark.gpu

I64, CI, VP, SZ = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
# (ldx - K, ldy - N, ldr - N, offset X, offset Y, offset residual): "packed" and "all" of test_abi_strided_gpu.py's LIN_LAYOUTS; "pad"
# moves and pads Y and the residual only, which no routing predicate reads past ldy % 4 (the split route needs X aligned, ldx % 4 == 0)
LAYOUTS = {"packed": (0, 0, 0, 0, 0, 0), "all": (1, 3, 4, 1, 1, 1), "pad": (4, 3, 4, 0, 1, 2)}
# (ldx - K, ldz - N, ldy - N, ld_dx - K, offsets X, Z, dY, dX): "packed" and "all" of LB_LAYOUTS
B_LAYOUTS = {"packed": (0, 0, 0, 0, 0, 0, 0, 0), "all": (1, 4, 1, 4, 1, 0, 1, 1)}


def L_():
    from macarons_amd import _lib
    return _lib.lib()


def stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def P(a):
    return VP(a.ptr) if a is not None else VP(None)


def sync_ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {L_().mcr_last_error().decode()}"


def same_bits(got, want, what):
    g, w = lc.bits(got), lc.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} element(s) differ, first (row, column, got, want): "
                           f"{[(int(i), int(j), float(got[i, j]), float(want[i, j])) for i, j in bad[:6]]}")


def run_linear(dev, x, w, b, r, layout, tag, gelu=False, alias=False):
    """One call of mcr_linear; alias: the residual IS the output (R == Y, ldr == ldy), as gemm_dx accumulates."""
    (M, K), N = x.shape, w.shape[0]
    dx, dy, dr, ox, oy, orr = LAYOUTS[layout]
    X, W = Arena(M, K, K + dx, ox, x, dev), Arena(N, K, data=w, device=dev)
    B = Arena(1, N, data=b[None], device=dev) if b is not None else None
    if alias:
        Y = Arena(M, N, N + dy, oy, r, dev)
        R = Y
    else:
        Y = Arena(M, N, N + dy, oy, device=dev)
        R = Arena(M, N, N + dr, orr, r, dev) if r is not None else None
    rc = L_().mcr_linear(P(X), I64(X.ld), P(W), P(B), P(R), I64(R.ld if R else 0), P(Y), I64(Y.ld), I64(M), CI(N), CI(K), CI(int(gelu)), stream())
    sync_ok(rc, tag)
    Y.check_guard(tag + " Y")
    for a in (X, W, B, None if alias else R):
        if a is not None:
            a.check_unchanged(tag + " input")
    return Y.packed()


# =====================================================================================================================================
# 2. exact operands
# =====================================================================================================================================
# The routes of launch_linear (nn_kernels.hip; lc.fp32_route recomputes its predicates):
#   small-K kernel: K <= 4, N % 4 == 0, ldy % 4 == 0, Y aligned, M * N / 4 >= 65536
#   deep K (128-wide chunks): K >= 128, K % 4 == 0, cdiv(M, 128) * cdiv(N, 64) <= 512; column tiles 2, halved like the generic kernel's
#   generic kernel: column tiles 8, halved while (nt / 2) * 32 >= N, then while cdiv(M, 128) * cdiv(N, 32 nt) < 512
#   16-byte loads of X / W only when K % 4 == 0, ld % 4 == 0 and the operand is aligned; scalar loads otherwise
FP32_SHAPES = [
    ("nt1", 129, 33, 33, "generic", 1), ("one", 1, 1, 1, "generic", 1), ("nt1_scalar", 257, 125, 125, "generic", 1),
    ("nt1_k4", 130, 126, 4, "generic", 1), ("nt2", 16381, 200, 20, "generic", 2), ("nt4", 32765, 200, 20, "generic", 4),
    ("nt8", 65531, 200, 20, "generic", 8),
    ("deep", 257, 512, 256, "deep", 1), ("deep_n1", 300, 1, 256, "deep", 1), ("deep_ragged_chunk", 129, 65, 132, "deep", 1),
    ("deep_nt2", 16377, 256, 132, "deep", 2), ("not_deep_k130", 129, 64, 130, "generic", 1),
    ("smallk_k3", 2048, 128, 3, "smallk", 0), ("smallk_k4", 2048, 128, 4, "smallk", 0),
    ("k1_n4_below", 16384, 4, 1, "generic", 1),          # M * N / 4 = 16384 < 65536: the matrix path (one 4-column tile)
    ("smallk_k1_n4", 65536, 4, 1, "smallk", 0),          # ... and the first M at which N = 4 takes the small-K kernel
]


@pytest.mark.parametrize("name,M,N,K,route,nt", FP32_SHAPES, ids=[s[0] for s in FP32_SHAPES])
def test_forward_fp32_routes_exact(dev, name, M, N, K, route, nt):
    assert lc.split_route(M, N, K) is None and lc.fp32_route(M, N, K) == (route, nt)
    x, w, b, r = lc.int_case(M, N, K)
    assert lc.headroom(x, w, b, r) < lc.LIMIT
    for bias in (True, False):
        for res in (True, False):
            want = lc.exact_ref(x, w, b if bias else None, r if res else None)
            for lay in ("packed", "all"):
                tag = f"{name} M={M} N={N} K={K} bias={bias} res={res} {lay}"
                same_bits(run_linear(dev, x, w, b if bias else None, r if res else None, lay, tag), want, tag)
    for lay in ("packed", "all"):
        tag = f"{name} M={M} N={N} K={K} residual == Y {lay}"
        same_bits(run_linear(dev, x, w, b, r, lay, tag, alias=True), lc.exact_ref(x, w, b, r), tag)


# The split route (linear3.hip; lc.split_route recomputes linear3_applicable and launch_linear3 from the constants quoted there).
# (bias, residual, layout) per class: every class once with both, the layouts alternate
SPLIT_FLAGS = {"x3_wint": (True, True, "packed"), "xint_w3": (True, True, "pad"), "x2_w2": (True, True, "packed"), "dense": (False, False, "pad")}


@pytest.mark.parametrize("cls", sorted(lc.SPLIT_CLASSES))
@pytest.mark.parametrize("M,N,K,nt,xcd", lc.SPLIT_SHAPES)
def test_forward_split_route_exact(dev, cls, M, N, K, nt, xcd):
    mb = lc.cdiv(M, 128)
    assert K % 8 == 0 and K >= 64 and N >= 128 and mb * lc.cdiv(N, 128) >= 256            # linear3_applicable
    assert lc.split_route(M, N, K) == (nt, xcd, mb) and xcd == (mb >= 64)
    x, w, b, r = lc.split_case(cls, M, N, K)
    bias, res, lay = SPLIT_FLAGS[cls]
    b, r = b if bias else None, r if res else None
    h = lc.headroom(x, w, b, r, lc.split_quantum(cls))
    assert h < lc.LIMIT, f"headroom 2^{np.log2(h):.2f}"
    tag = f"split {cls} M={M} N={N} K={K} nt={nt} xcd={xcd} {lay}"
    same_bits(run_linear(dev, x, w, b, r, lay, tag), lc.exact_ref(x, w, b, r), tag)


# mcr_linear_backward: [dW | db] = dY^T [X | 1] on 64 x 64 tiles over (N, K + 1) and slabs of rows (vb_gemm_kernel, vb_reduce_kernel;
# 256-row slabs up to 16384 rows, longer ones beyond); dX = dY W through vb_transpose_kernel and launch_linear routed on ONE row:
# the deep kernels whenever the inner dimension N >= 128 and N % 4 == 0.
BWD_SHAPES = ([(257, N, K) for N in (63, 64, 65) for K in (62, 63, 64)]                  # the ones column inside / last in / alone in a tile
              + [(M, 5, 6) for M in (255, 256, 257, 511, 513, 4097, 16390)]                    # slab edges; N K = 30: one ragged transpose block
              + [(M, 65, 63) for M in (256, 513)]
              + [(M, N, K) for (M, K) in ((300, 70), (16377, 130)) for N in (128, 132, 256)])   # dX on the deep kernels


@pytest.mark.parametrize("M,N,K", BWD_SHAPES)
def test_backward_exact(dev, M, N, K):
    x, w, g, base = lc.int_backward_case(M, N, K)
    assert lc.backward_headroom(x, w, g, base) < lc.LIMIT
    if N >= 128:
        assert lc.fp32_route(1, K, N)[0] == "deep" and N % 4 == 0      # (routing rows = 1; output width K, inner dimension N)
    for acc in (False, True):
        rdx, rdw, rdb = lc.backward_ref(x, w, g, base if acc else None)
        for lay, (px, pz, py, pd, ox, oz, oy, od) in B_LAYOUTS.items():
            tag = f"backward M={M} N={N} K={K} acc={acc} {lay}"
            X, W = Arena(M, K, K + px, ox, x, dev), Arena(N, K, data=w, device=dev)
            G = Arena(M, N, N + py, oy, g, dev)
            DX = Arena(M, K, K + pd, od, base if acc else None, dev)
            DW, DB = Arena(N, K, device=dev), Arena(1, N, device=dev)
            ws = Workspace(int(L_().mcr_linear_backward_workspace_bytes(I64(M), CI(N), CI(K))), dev)
            rc = L_().mcr_linear_backward(P(X), I64(X.ld), P(W), VP(None), I64(0), P(G), I64(G.ld), I64(M), CI(N), CI(K), CI(0), P(DX), I64(DX.ld),
                                          CI(int(acc)), P(DW), P(DB), P(ws), SZ(ws.n_bytes), stream())
            sync_ok(rc, tag)
            for a in (X, W, G):
                a.check_unchanged(tag + " input")
            ws.check_guard(tag + " workspace")
            for name, arena, want in (("dX", DX, rdx), ("dW", DW, rdw), ("db", DB, rdb[None])):
                arena.check_guard(f"{tag} {name}")
                same_bits(arena.packed(), want, f"{tag} {name}")


# =====================================================================================================================================
# 3. invariances, bit for bit on real-valued data
# =====================================================================================================================================
POW2_SHAPES = [("generic_scalar", 257, 125, 125), ("generic_nt8", 65531, 200, 20), ("deep_ragged_chunk", 129, 65, 132), ("deep_nt2", 16377, 256, 132),
               ("smallk_k3", 2048, 128, 3), ("split_nt2_xcd_exit", 8193, 512, 72), ("split_nt4_half_chunk", 8100, 1024, 520),
               ("split_nt1_rows_fastest", 897, 4000, 64)]


@pytest.mark.parametrize("name,M,N,K", POW2_SHAPES, ids=[s[0] for s in POW2_SHAPES])
def test_power_of_two_scales_commute(dev, name, M, N, K):
    """Row m of X times 2^a_m and row n of W times 2^b_n: Y'[m, n] == 2^(a_m + b_n) Y[m, n] bit for bit.  The truncating split, every
    product and every fp32 sum commute with powers of two as long as nothing leaves the normal range, so a kernel that mixes rows or
    columns at an edge, or loses what a small row contributes, cannot pass -- the max-norm bar never looked at those rows."""
    x, w, a, b = lc.pow2_case(M, N, K)
    xs, ws = np.ldexp(x, a[:, None]).astype(np.float32), np.ldexp(w, b[:, None]).astype(np.float32)
    assert np.abs(xs).min() >= 2.0 ** -30 and np.abs(ws).min() >= 2.0 ** -36 and max(np.abs(xs).max(), np.abs(ws).max()) < 2.0 ** 23
    y = run_linear(dev, x, w, None, None, "packed", f"{name} unscaled")
    ys = run_linear(dev, xs, ws, None, None, "packed", f"{name} scaled")
    assert np.isfinite(y).all()
    same_bits(ys, np.ldexp(y, a[:, None] + b[None, :]).astype(np.float32), f"{name} M={M} N={N} K={K} scaled by powers of two")


def _ulps(a, b):
    o = lambda t: np.where(t.view(np.int32) >= 0, t.view(np.int32).astype(np.int64), -(t.view(np.int32).astype(np.int64) & 0x7FFFFFFF))
    return np.abs(o(a) - o(b))


def test_small_k_kernel_equals_the_matrix_path(dev):
    """The claim above linear_smallk_kernel: its fmaf chain in ascending k, then + bias, is bit for bit what the zero-padded fp32 MFMA
    path returns.  The first 2047 rows of (2048, 128, 3) inside the full call (small-K kernel) and alone (M = 2047 is below the
    kernel's threshold: linear_kernel<1, 32>), same bias and residual.  With the GELU both kernels call the same gelu_erf on the same
    pre-activation; what differs is printed (a finding, not an assertion: the comment claims the chain and the bias only).
    Measured on an MI355X: GELU, 0 of 262016 elements differ."""
    M, N, K = 2048, 128, 3
    assert lc.fp32_route(M, N, K) == ("smallk", 0) and lc.fp32_route(M - 1, N, K) == ("generic", 1)
    x, w, b, r = lc.normal_case(M, N, K)
    for bias, res in ((True, True), (False, False), (True, False)):
        bb, rr = b if bias else None, r if res else None
        tag = f"small K vs matrix path bias={bias} res={res}"
        ya = run_linear(dev, x, w, bb, rr, "packed", tag + " M=2048")[:M - 1]
        yb = run_linear(dev, x[:M - 1], w, bb, None if rr is None else rr[:M - 1], "packed", tag + " M=2047")
        same_bits(ya, yb, tag)
    ya = run_linear(dev, x, w, b, r, "packed", "small K gelu M=2048", gelu=True)[:M - 1]
    yb = run_linear(dev, x[:M - 1], w, b, r[:M - 1], "packed", "small K gelu M=2047", gelu=True)
    d = _ulps(ya, yb)
    print(f"ERR small K vs matrix path with GELU: {int((d != 0).sum())} of {d.size} elements differ, largest difference {int(d.max())} ulp")
    assert np.isfinite(ya).all() and np.isfinite(yb).all()


def test_split_result_does_not_depend_on_tile_width_block_order_or_m(dev):
    """The note on L3G_NT in linear3.hip: one X [8192, 520], one W [4032, 520]; A = all rows against W[:512] (64-column blocks, XCD
    order), C = all rows against W[:1024] (128-column blocks), B = X[:1000] against all of W (32-column blocks, row block fastest)."""
    assert lc.split_route(8192, 512, 520) == (2, True, 64) and lc.split_route(8192, 1024, 520) == (4, True, 64)
    assert lc.split_route(1000, 4032, 520) == (1, False, 8)
    x, w, b, _ = lc.normal_case(8192, 4032, 520)
    ya = run_linear(dev, x, w[:512], b[:512], None, "packed", "split A")
    yc = run_linear(dev, x, w[:1024], b[:1024], None, "packed", "split C")
    yb = run_linear(dev, x[:1000], w, b, None, "packed", "split B")
    same_bits(yc[:, :512], ya, "split route, 128-column blocks against 64-column blocks")
    same_bits(yb[:, :512], ya[:1000], "split route, 32-column blocks in row-block-fastest order against 64-column blocks in XCD order")


def test_generic_result_does_not_depend_on_tile_width_or_m(dev):
    """Rows 0..999 alone (linear_kernel<1, 32>) and inside M = 65531 (linear_kernel<8, 32>), N = 200, K = 20."""
    assert lc.fp32_route(1000, 200, 20) == ("generic", 1) and lc.fp32_route(65531, 200, 20) == ("generic", 8)
    x, w, b, r = lc.normal_case(65531, 200, 20)
    y8 = run_linear(dev, x, w, b, r, "packed", "generic M=65531")
    y1 = run_linear(dev, x[:1000], w, b, r[:1000], "packed", "generic M=1000")
    same_bits(y8[:1000], y1, "generic kernel, 8 column tiles against 1")


# =====================================================================================================================================
# 4. componentwise bound on real-valued data
# =====================================================================================================================================
def _row_scales(M):
    """2^-10, 1, 2^10 in blocks of 37 rows (no multiple of a wave's 32 or a block's 128 rows)."""
    return np.array([-10, 0, 10])[(np.arange(M) // 37) % 3]


def _bound_case(M, N, K, scaled):
    x, w, b, r = lc.normal_case(M, N, K, seed=4)
    if scaled:                                            # every row a scaled copy: no bias, the residual scaled with its row
        e = _row_scales(M)[:, None]
        return np.ldexp(x, e).astype(np.float32), w, None, np.ldexp(r, e).astype(np.float32)
    return x, w, b, r


def _share(y, ref64, bound, what):
    assert np.isfinite(y).all(), what
    s = np.abs(y.astype(np.float64) - ref64) / bound
    i = np.unravel_index(np.argmax(s), s.shape)
    print(f"ERR {what}: worst share of the bound {s[i]:.4f} at {tuple(int(v) for v in i)}")
    return float(s[i]), f"{what}: |y - ref| = {s[i]:.3f} of the bound at {i}: got {y[i]!r}, reference {ref64[i]!r}"


BOUND_FP32 = [("generic_scalar", 257, 125, 125), ("generic_nt2", 16381, 200, 20), ("deep_ragged_chunk", 129, 65, 132), ("deep", 257, 512, 256),
              ("smallk_k3", 2048, 128, 3)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled_rows"])
@pytest.mark.parametrize("name,M,N,K", BOUND_FP32, ids=[s[0] for s in BOUND_FP32])
def test_componentwise_bound_fp32_routes(dev, name, M, N, K, scaled):
    """|y - ref64| <= (K + 3) u B, B = sum_k |x||w| + |b| + |r|, u = 2^-24: the bound of a K-term fma chain in any order plus the bias
    and residual additions.  Measured on an MI355X (worst share of the bound, plain / scaled rows): generic K = 125 0.029 / 0.028,
    generic K = 20 0.18 / 0.20, deep K = 132 0.019 / 0.021, deep K = 256 0.016 / 0.017, small K = 3 0.45 / 0.40 (six roundings
    allowed, three or four made)."""
    x, w, b, r = _bound_case(M, N, K, scaled)
    y = run_linear(dev, x, w, b, r, "packed", f"bound {name}")
    ref = x.astype(np.float64) @ w.astype(np.float64).T + (0 if b is None else b.astype(np.float64)) + r.astype(np.float64)
    s, msg = _share(y, ref, (K + 3) * lc.U24 * lc.magnitudes(x, w, b, r), f"fp32 route {name} M={M} N={N} K={K} scaled={scaled}")
    assert s <= 1.0, msg


BOUND_SPLIT = [("nt2_xcd", 8192, 512, 72), ("nt1_rows_fastest", 1000, 4032, 520), ("nt1_k64", 897, 4000, 64)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled_rows"])
@pytest.mark.parametrize("name,M,N,K", BOUND_SPLIT, ids=[s[0] for s in BOUND_SPLIT])
def test_componentwise_bound_split_route(dev, name, M, N, K, scaled):
    """The header's "fp32-class" claim: |y - (T + b + r)| <= (K + 3) u B against the six-term model T (lc.six_term), and against the full
    product with the derived 2^-21 B of the dropped terms on top.  Measured on an MI355X (worst share, plain / scaled rows), against
    the six terms: K = 72 0.056 / 0.058, K = 520 0.0081 / 0.0088, K = 64 0.056 / 0.070; against the full product: 0.048 / 0.049,
    0.0078 / 0.0085, 0.056 / 0.066."""
    assert lc.split_route(M, N, K) is not None
    x, w, b, r = _bound_case(M, N, K, scaled)
    y = run_linear(dev, x, w, b, r, "packed", f"bound split {name}")
    tail = (0 if b is None else b.astype(np.float64)) + r.astype(np.float64)
    B = lc.magnitudes(x, w, b, r)
    s6, msg6 = _share(y, lc.six_term(x, w) + tail, (K + 3) * lc.U24 * B, f"split route {name} M={M} N={N} K={K} scaled={scaled} vs six terms")
    full = x.astype(np.float64) @ w.astype(np.float64).T + tail
    sf, msgf = _share(y, full, ((K + 3) * lc.U24 + lc.DROPPED_BOUND) * B, f"split route {name} M={M} N={N} K={K} scaled={scaled} vs full product")
    assert s6 <= 1.0, msg6
    assert sf <= 1.0, msgf
