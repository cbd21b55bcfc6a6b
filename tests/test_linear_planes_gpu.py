"""The planes GEMMs (macarons_amd/csrc/linear3p.hip) through their own entry points: mcr_split_to_planes, mcr_linear_planes,
mcr_linear_planes_dot (include/macarons_hip.h), called through ctypes on guarded arenas (tests/_strided.py).

(a) EXACT parity.  The kernels take the hi and lo planes as independent operands, so the planes are filled with small integers: every
    product and every partial sum is an integer below 2^24, exactly representable in fp32, and the result does not depend on the
    summation order.  The kernel must equal the integer reference (Wl Xh + Wh Xl + Wh Xh) wscale_inv + bias (+ row bias) (+ R) BIT FOR
    BIT; a dropped, doubled or mis-swizzled chunk, a wrong plane pairing, an lo x lo term, a stale stage or a wrong row / column at a
    tile edge changes bits.  Every case asserts that its own inputs stay below 2^24.
(b) The three tile forms, and the dot form against its two-launch equivalent, agree bit for bit on real-valued data.
(c) Split + GEMM against fp64 on the original fp32 values: the project's bar for split-precision linears, 2e-5 max(1, max|ref|)
    (test_linear_vs_numpy); one plane: against fp64 on the operands rounded to fp16 (the same bar: accumulation and GELU error only).
(d) mcr_split_to_planes bit for bit against numpy: hi = float16(x), lo = float16(x - float32(hi)).
(e) Every precondition of the entries violated once: return code 1, a message naming the entry, nothing written.

Which kernel a case launches (launch_linear3p's rule: one-shot if M <= 4096, no row bias and K = 128 or K % 256 == 0; else the
two-stage SMALL tile if K <= 512; else the three-stage large tile), every case with n_planes 1 and 2 and with fp32 and planes output:
    test_exact_once[*]      linear3p_once_kernel<F32 | PLANES, 1 | 2>                    (direct epilogue, its only one)
    test_exact_small[*]     linear3p_kernel<F32 | PLANES, SMALL, 1 | 2>   fp32: transposed fp32 epilogue; planes: transposed planes
    test_exact_large[*]     linear3p_kernel<F32 | PLANES, large, 1 | 2>   epilogue where N % 8 == 0, the direct form elsewhere
    test_exact_dot[*]       linear3p_kernel<DOT, large, 1 | 2>
    test_exact_residual / test_exact_row_bias / test_epilogue_selectors / test_exact_chip_filling: the same instantiations with a
    residual (separate and aliasing Y), a row bias (planes: transposed planes epilogue; fp32: direct), and each selector of the
    direct form (N % 8, ldy % 8, an output off the 16-byte grid, ldr % 4, a row bias on fp32 rows) against the transposed result.
"""
import ctypes

import numpy as np
import pytest
import torch

import _strided as st
from _strided import Arena, HalfArena

pytestmark = pytest.mark.gpu

I64, CI, VP, CF = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
TOL = 2e-5                       # the project's bar for split-precision linears (test_linear_vs_numpy)
F16, F32, F64 = np.float16, np.float32, np.float64
LIMIT = float(2 ** 24)


def L_():
    from macarons_amd import _lib
    return _lib.lib()


def stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def last_error():
    return L_().mcr_last_error().decode()


def ptr(a):
    if a is None:
        return VP(None)
    return VP(a) if isinstance(a, int) else VP(a.ptr)


def c_linear_planes(Xh, Xl, ldx, Wh, Wl, ldw, bias, Y, Yh, Yl, ldy, M, N, K, gelu, inv, rb, rpg, rg, R, ldr, npl):
    return L_().mcr_linear_planes(ptr(Xh), ptr(Xl), I64(ldx), ptr(Wh), ptr(Wl), I64(ldw), ptr(bias), ptr(Y), ptr(Yh), ptr(Yl), I64(ldy),
                                  I64(M), CI(N), CI(K), CI(int(gelu)), CF(inv), ptr(rb), I64(rpg), ptr(rg), ptr(R), I64(ldr), CI(npl), stream())


def c_dot(Xh, Xl, ldx, Wh, Wl, ldw, bias, M, K, gelu, inv, v, c, gelu2, out, npl):
    return L_().mcr_linear_planes_dot(ptr(Xh), ptr(Xl), I64(ldx), ptr(Wh), ptr(Wl), I64(ldw), ptr(bias), I64(M), CI(K), CI(int(gelu)), CF(inv),
                                      ptr(v), ptr(c), CI(int(gelu2)), ptr(out), CI(npl), stream())


def c_split(X, ldx, Ph, Pl, ldp, M, E):
    return L_().mcr_split_to_planes(ptr(X), I64(ldx), ptr(Ph), ptr(Pl), I64(ldp), I64(M), CI(E), stream())


def sync_ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {last_error()}"


def split_np(x):
    """The two-term fp16 split of the project: hi = fp16(x) (round to nearest even), lo = fp16(x - hi)."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(F16)
        lo = (x - hi.astype(F32)).astype(F16)
    return hi, lo


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (f"{what}: {len(bad)} of {g.size} element(s) differ, first at {bad[:6].tolist()}: got "
                           f"{[np.asarray(got)[tuple(i)] for i in bad[:6]]} want {[np.asarray(want)[tuple(i)] for i in bad[:6]]}")


# =====================================================================================================================================
# one call of mcr_linear_planes on arenas
# =====================================================================================================================================
class Lay:
    """Padding (elements) and offsets (elements) of the operands of one call; the defaults keep every fast path's conditions."""

    def __init__(self, dx=8, ox=8, dw=16, ow=0, dy=8, oy=8, dr=4, orr=4):
        self.dx, self.ox, self.dw, self.ow, self.dy, self.oy, self.dr, self.orr = dx, ox, dw, ow, dy, oy, dr, orr


class Operands:
    """The device arenas of one problem's inputs (built once, shared by the calls on it)."""

    def __init__(self, dev, xh, xl, wh, wl, bias=None, lay=None):
        lay = lay or Lay()
        (M, K), N = xh.shape, wh.shape[0]
        self.M, self.N, self.K, self.lay = M, N, K, lay
        self.Xh = HalfArena(M, K, K + lay.dx, lay.ox, xh, dev)
        self.Xl = HalfArena(M, K, K + lay.dx, lay.ox, xl, dev)
        self.Wh = HalfArena(N, K, K + lay.dw, lay.ow, wh, dev)
        self.Wl = HalfArena(N, K, K + lay.dw, lay.ow, wl, dev)
        self.B = Arena(1, N, data=np.asarray(bias, F32)[None], device=dev) if bias is not None else None

    def inputs(self):
        return [a for a in (self.Xh, self.Xl, self.Wh, self.Wl, self.B) if a is not None]


def run_linear(dev, ops, out, npl, inv, gelu=False, rb=None, rpg=0, rgroup=None, r=None, alias=False, lay=None, tag=""):
    """out 'f32' -> fp32 [M, N]; 'planes' -> (hi, lo) float16 [M, N] (lo None when npl == 1: the Yl arena must then be untouched)."""
    lay = lay or ops.lay
    M, N, K = ops.M, ops.N, ops.K
    RB = Arena(rb.shape[0], N, data=rb, device=dev) if rb is not None else None
    RG = torch.from_numpy(np.asarray(rgroup, np.int32)).to(dev) if rgroup is not None else None
    Y = Yh = Yl = R = None
    if out == "f32":
        Y = Arena(M, N, N + lay.dy, lay.oy, r if alias else None, dev)
        if r is not None and not alias:
            R = Arena(M, N, N + lay.dr, lay.orr, r, dev)
        ldy = Y.ld
    else:
        assert r is None
        Yh = HalfArena(M, N, N + lay.dy, lay.oy, device=dev)
        Yl = HalfArena(M, N, N + lay.dy, lay.oy, device=dev)
        ldy = Yh.ld
    rc = c_linear_planes(ops.Xh, ops.Xl if npl == 2 else None, ops.Xh.ld, ops.Wh, ops.Wl if npl == 2 else None, ops.Wh.ld, ops.B, Y, Yh,
                         Yl, ldy, M, N, K, gelu, inv, RB, rpg, RG.data_ptr() if RG is not None else None, Y if alias else R,
                         Y.ld if alias else (R.ld if R else 0), npl)
    sync_ok(rc, tag)
    for a in ops.inputs() + [a for a in (RB, R) if a is not None]:
        a.check_unchanged(tag + " input")
    if out == "f32":
        Y.check_guard(tag + " Y")
        return Y.packed()
    Yh.check_guard(tag + " Yh")
    if npl == 1:
        Yl.check_unchanged(tag + " Yl of a one-plane call")
        return Yh.packed(), None
    Yl.check_guard(tag + " Yl")
    return Yh.packed(), Yl.packed()


# =====================================================================================================================================
# (a) exact-integer parity
# =====================================================================================================================================
def int_planes(rng, shape, amax):
    return rng.integers(-amax, amax + 1, shape).astype(F16)


class IntProblem:
    def __init__(self, M, N, K, seed, amax=7, bias_max=2000):
        rng = np.random.default_rng(seed)
        self.M, self.N, self.K, self.amax = M, N, K, amax
        self.xh, self.xl = int_planes(rng, (M, K), amax), int_planes(rng, (M, K), amax)
        self.wh, self.wl = int_planes(rng, (N, K), amax), int_planes(rng, (N, K), amax)
        assert np.abs(self.xl).max() > 0 and np.abs(self.wl).max() > 0          # the low planes can change the answer
        self.bias = rng.integers(-bias_max, bias_max + 1, N).astype(F32)
        self.rng = rng
        self._acc = {}

    def acc(self, npl):
        """X W^T of the planes in fp64 BLAS: exact, every sum is an integer far below 2^53."""
        if npl not in self._acc:
            xh, wh = self.xh.astype(F64), self.wh.astype(F64)
            self._acc[npl] = xh @ wh.T if npl == 1 else (xh + self.xl.astype(F64)) @ wh.T + xh @ self.wl.astype(F64).T
        return self._acc[npl]

    def sum_abs_bound(self, npl):
        """An upper bound of the sum of |terms| of one output element, from the planes' own maxima."""
        a = lambda t: float(np.abs(t.astype(F32)).max())
        per_k = a(self.wh) * a(self.xh) + (a(self.wl) * a(self.xh) + a(self.wh) * a(self.xl) if npl == 2 else 0.0)
        return self.K * per_k

    def ref(self, npl, inv, rb_rows=None, r=None):
        extra = sum(float(np.abs(t).max()) for t in (self.bias, rb_rows, r) if t is not None)
        # everything is a multiple of wscale_inv: in those units the sums must stay below 2^24 to be exact in fp32
        assert self.sum_abs_bound(npl) + extra / inv < LIMIT, (self.sum_abs_bound(npl), extra, inv)
        y = self.acc(npl) * inv
        for t in (self.bias, rb_rows, r):
            if t is not None:
                y = y + t.astype(F64)
        y32 = y.astype(F32)
        assert np.array_equal(y32.astype(F64), y)                              # the reference itself is exact in fp32
        return y32

    def planes_inv(self, npl, extra=0.0):
        """2^-5 for planes output: with five fractional bits next to an integer bias of up to 11 bits most outputs need more than the
        11 bits of one fp16 (the low plane is exercised at every K), and |y| stays far inside the fp16 range."""
        inv = 2.0 ** -5
        assert self.sum_abs_bound(npl) * inv + float(np.abs(self.bias).max()) + extra < 60000.0
        return inv


def check_exact(dev, p, ops, npl, out, tag, **kw):
    rb, rpg, rgroup, r = kw.get("rb"), kw.get("rpg", 0), kw.get("rgroup"), kw.get("r")
    rb_rows = None
    if rb is not None:
        rb_rows = rb[np.asarray(rgroup)] if rgroup is not None else rb[np.arange(p.M) // rpg]
    extra = float(np.abs(rb).max()) if rb is not None else 0.0
    inv = p.planes_inv(npl, extra) if out == "planes" else 0.5
    want = p.ref(npl, inv, rb_rows, r)
    got = run_linear(dev, ops, out, npl, inv, tag=tag, **kw)
    if out == "f32":
        same_bits(got, want, tag)
        return got
    assert np.abs(want).max() < 65504.0
    hi, lo = split_np(want)
    same_bits(got[0], hi, tag + " hi")
    if npl == 2:
        same_bits(got[1], lo, tag + " lo")
        assert want.size < 256 or np.count_nonzero(lo) > want.size // 8, "the low output plane is (nearly) all zero: the case does not test it"
    return got


def exact_cell(dev, M, N, K):
    p = IntProblem(M, N, K, seed=M * 7919 + N * 31 + K)
    ops = Operands(dev, p.xh, p.xl, p.wh, p.wl, p.bias)
    for npl in (1, 2):
        for out in ("f32", "planes"):
            check_exact(dev, p, ops, npl, out, f"exact M={M} N={N} K={K} planes={npl} out={out}")


ONCE = [(1, 4, 128), (63, 60, 256), (64, 64, 512), (65, 68, 128), (200, 192, 256)]
SMALL = [(1, 4, 32), (127, 12, 64), (128, 124, 96), (129, 128, 384), (1153, 132, 32), (4097, 260, 512), (1153, 260, 96)]
LARGE = [(1, 4, 544), (255, 124, 1344), (256, 128, 544), (257, 132, 1344), (2305, 512, 544)]
DOT = [(1, 32), (127, 64), (128, 512), (129, 32), (1153, 64), (1153, 512)]


def form_of(M, K, row_bias=False):
    if M <= 4096 and not row_bias and (K == 128 or K % 256 == 0):
        return "once"
    return "small" if K <= 512 else "large"


@pytest.mark.parametrize("M,N,K", ONCE, ids=lambda v: str(v))
def test_exact_once(dev, M, N, K):
    assert form_of(M, K) == "once"
    exact_cell(dev, M, N, K)


@pytest.mark.parametrize("M,N,K", SMALL, ids=lambda v: str(v))
def test_exact_small(dev, M, N, K):
    assert form_of(M, K) == "small"
    exact_cell(dev, M, N, K)


@pytest.mark.parametrize("M,N,K", LARGE, ids=lambda v: str(v))
def test_exact_large(dev, M, N, K):
    assert form_of(M, K) == "large"
    exact_cell(dev, M, N, K)


def run_dot(dev, xh, xl, wh, wl, bias, v, c, npl, inv, gelu=False, gelu2=False, tag=""):
    (M, K) = xh.shape
    ops = Operands(dev, xh, xl, wh, wl, bias)
    V = Arena(1, 256, data=np.asarray(v, F32)[None], device=dev)
    C = Arena(1, 1, data=np.asarray([[c]], F32), device=dev) if c is not None else None
    O = Arena(M, 1, 1, 1, device=dev)                                          # (4-byte aligned, off the 16-byte grid)
    rc = c_dot(ops.Xh, ops.Xl if npl == 2 else None, ops.Xh.ld, ops.Wh, ops.Wl if npl == 2 else None, ops.Wh.ld, ops.B, M, K, gelu, inv, V, C,
               gelu2, O, npl)
    sync_ok(rc, tag)
    O.check_guard(tag + " out")
    for a in ops.inputs() + [V] + ([C] if C else []):
        a.check_unchanged(tag + " input")
    return O.packed()[:, 0]


@pytest.mark.parametrize("M,K", DOT, ids=lambda v: str(v))
def test_exact_dot(dev, M, K):
    p = IntProblem(M, 256, K, seed=M * 13 + K, amax=3, bias_max=50)
    v = p.rng.integers(-3, 4, 256).astype(F32)
    c = 11.0
    for npl in (1, 2):
        for bias, cc in ((p.bias, c), (None, None)):
            inv = 0.5
            ymax = p.sum_abs_bound(npl) + (50.0 / inv if bias is not None else 0.0)           # |y| in units of inv
            assert 256 * 3.0 * ymax + abs(c) / inv < LIMIT                                    # the 256-term reduction stays exact too
            y = p.acc(npl) * inv + (bias.astype(F64) if bias is not None else 0.0)
            want = (y @ v.astype(F64) + (cc or 0.0)).astype(F32)
            got = run_dot(dev, p.xh, p.xl, p.wh, p.wl, bias, v, cc, npl, inv, tag=f"dot M={M} K={K} planes={npl} bias={bias is not None}")
            same_bits(got, want, f"dot M={M} K={K} planes={npl} bias={bias is not None}")


@pytest.mark.parametrize("M,N,K", [(65, 68, 256), (129, 132, 96), (257, 132, 544)], ids=lambda v: str(v))
def test_exact_residual(dev, M, N, K):
    """fp32 output with a residual on a buffer of its own, and aliasing Y (the encoders' in-place x += ...), in every form."""
    p = IntProblem(M, N, K, seed=M + N + K)
    ops = Operands(dev, p.xh, p.xl, p.wh, p.wl, p.bias)
    r = p.rng.integers(-1000, 1001, (M, N)).astype(F32)
    for npl in (1, 2):
        for alias in (False, True):
            check_exact(dev, p, ops, npl, "f32", f"residual {form_of(M, K)} M={M} N={N} K={K} planes={npl} alias={alias}", r=r, alias=alias)


@pytest.mark.parametrize("M,N,K", [(330, 136, 512), (330, 132, 96), (330, 136, 1344)], ids=lambda v: str(v))
def test_exact_row_bias(dev, M, N, K):
    """A row bias by rows_per_group (boundaries at 50, 100 ... fall inside 32-row tiles; the last group has 30 rows) and by
    row_group[m]; a row bias keeps K = 512 off the one-shot form."""
    assert form_of(M, K, True) in ("small", "large")
    p = IntProblem(M, N, K, seed=M + N + K + 1)
    ops = Operands(dev, p.xh, p.xl, p.wh, p.wl, p.bias)
    rb = p.rng.integers(-200, 201, (7, N)).astype(F32)
    rgroup = p.rng.integers(0, 7, M).astype(np.int32)
    for npl in (1, 2):
        for out in ("f32", "planes"):
            check_exact(dev, p, ops, npl, out, f"row bias rpg M={M} N={N} K={K} planes={npl} out={out}", rb=rb, rpg=50)
            check_exact(dev, p, ops, npl, out, f"row bias idx M={M} N={N} K={K} planes={npl} out={out}", rb=rb, rgroup=rgroup)


@pytest.mark.parametrize("K", [96, 544], ids=["small", "large"])
@pytest.mark.parametrize("kind", ["int", "real_gelu"])
def test_epilogue_selectors(dev, K, kind):
    """Every condition that sends a pipelined call through the direct epilogue, against the transposed-epilogue result of the same
    problem, bit for bit (integers: both also equal the reference; real values with GELU: the GELU and the split of both forms)."""
    M, N = 300, 136
    p = IntProblem(M, N, K, seed=K + 5)
    gelu = kind == "real_gelu"
    if gelu:
        rng = np.random.default_rng(K)
        p.xh, p.xl = split_np(rng.standard_normal((M, K)) * 2.5)
        p.wh, p.wl = split_np(rng.standard_normal((N, K)) / np.sqrt(K) * 256.0)
        p.bias = rng.standard_normal(N).astype(F32)
    ops = Operands(dev, p.xh, p.xl, p.wh, p.wl, p.bias)
    r = p.rng.integers(-1000, 1001, (M, N)).astype(F32)
    rb = np.zeros((3, N), F32) if gelu else p.rng.integers(-200, 201, (3, N)).astype(F32)
    for npl in (1, 2):
        inv_p, inv_f = (1.0 / 256.0, 1.0 / 256.0) if gelu else (p.planes_inv(npl), 0.5)
        run = lambda out, inv, lay=None, **kw: run_linear(dev, ops, out, npl, inv, gelu=gelu, lay=lay, tag=f"selectors K={K} {kind} planes={npl}", **kw)
        # planes output: ldy % 8, an offset of 8 bytes, N % 8 (the first 132 features of the same problem)
        base = run("planes", inv_p)
        for name, lay in (("ldy % 8 != 0", Lay(dy=4)), ("Yh off the 16-byte grid", Lay(oy=4))):
            got = run("planes", inv_p, lay)
            same_bits(got[0], base[0], f"{name} hi")
            if npl == 2:
                same_bits(got[1], base[1], f"{name} lo")
        ops132 = Operands(dev, p.xh, p.xl, p.wh[:132], p.wl[:132], p.bias[:132])
        got = run_linear(dev, ops132, "planes", npl, inv_p, gelu=gelu, tag=f"selectors N=132 K={K} {kind} planes={npl}")
        same_bits(got[0], base[0][:, :132], "N % 8 != 0 hi")
        if npl == 2:
            same_bits(got[1], base[1][:, :132], "N % 8 != 0 lo")
        # fp32 output: Y off the grid, a residual with ldr % 4 != 0 or off the grid, a row bias
        base = run("f32", inv_f)
        same_bits(run("f32", inv_f, Lay(oy=1)), base, "Y off the 16-byte grid")
        base_r = run("f32", inv_f, r=r)
        same_bits(base_r, base + r, "residual (transposed epilogue)")
        same_bits(run("f32", inv_f, Lay(dr=1), r=r), base_r, "ldr % 4 != 0")
        same_bits(run("f32", inv_f, Lay(orr=1), r=r), base_r, "R off the 16-byte grid")
        if gelu:
            same_bits(run("f32", inv_f, rb=rb, rpg=128), base, "a zero row bias on fp32 rows")
        else:
            rows = rb[np.arange(M) // 128]
            same_bits(run("f32", inv_f, rb=rb, rpg=128), p.ref(npl, inv_f, rows), "a row bias on fp32 rows")
            same_bits(base, p.ref(npl, inv_f), "transposed fp32 epilogue")


@pytest.mark.parametrize("K,out", [(512, "planes"), (1344, "f32")], ids=["small", "large"])
def test_exact_chip_filling(dev, K, out):
    """One launch per pipelined form that fills the chip: 258 (129) row blocks x 4 column blocks, co-resident and more than one
    round; every row against the exact fp64 BLAS reference."""
    M, N = 33001, 512
    assert form_of(M, K) == ("small" if K == 512 else "large")
    p = IntProblem(M, N, K, seed=K)
    ops = Operands(dev, p.xh, p.xl, p.wh, p.wl, p.bias)
    check_exact(dev, p, ops, 2, out, f"chip filling K={K} out={out}")


# =====================================================================================================================================
# (b) the forms agree bit for bit on real-valued data
# =====================================================================================================================================
def device_split(dev, x, low=True):
    """Planes of x by mcr_split_to_planes."""
    M, E = x.shape
    X = Arena(M, E, data=x, device=dev)
    Ph, Pl = HalfArena(M, E, device=dev), HalfArena(M, E, device=dev)
    sync_ok(c_split(X, X.ld, Ph, Pl if low else None, E, M, E), "split")
    return Ph.packed(), Pl.packed() if low else None


def real_problem(dev, M, N, K, seed, scale=1.0):
    from macarons_amd.networks import packing
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, K)) * scale).astype(F32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32)
    b = rng.standard_normal(N).astype(F32)
    xh, xl = device_split(dev, x)
    wp = packing.weight_planes(torch.from_numpy(w)).numpy()
    return x, w, b, xh, xl, wp[0], wp[1]


def all_outputs(dev, xh, xl, wh, wl, b, gelu):
    ops = Operands(dev, xh, xl, wh, wl, b)
    res = {}
    for npl in (1, 2):
        res[npl, "f32"] = run_linear(dev, ops, "f32", npl, 1.0 / 256.0, gelu=gelu)
        res[npl, "hi"], res[npl, "lo"] = run_linear(dev, ops, "planes", npl, 1.0 / 256.0, gelu=gelu)
    return res


def assert_same_outputs(a, b, rows, what):
    for k in a:
        if a[k] is not None:
            same_bits(a[k][:rows], b[k][:rows], f"{what} {k}")


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
@pytest.mark.parametrize("K", [128, 512])
def test_forms_agree(dev, K, gelu):
    """One-shot (M = 4096) == SMALL (the same rows inside M = 4097) == large (K = 512 zero-padded to 544: the added chunk
    contributes exact zeros)."""
    M, N = 4097, 192
    _, _, b, xh, xl, wh, wl = real_problem(dev, M, N, K, seed=K, scale=2.5)
    assert form_of(M - 1, K) == "once" and form_of(M, K) == "small"
    once = all_outputs(dev, xh[:M - 1], xl[:M - 1], wh, wl, b, gelu)
    small = all_outputs(dev, xh, xl, wh, wl, b, gelu)
    assert_same_outputs(once, small, M - 1, f"one-shot vs SMALL K={K}")
    if K == 512:
        pad = lambda t: np.concatenate([t, np.zeros((t.shape[0], 32), F16)], 1)
        assert form_of(M, K + 32) == "large"
        large = all_outputs(dev, pad(xh), pad(xl), pad(wh), pad(wl), b, gelu)
        assert_same_outputs(small, large, M, "SMALL vs large")


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, on numpy arrays: the product is exact in fp64; the fp64 sum is turned into its
    round-to-odd value (truncate, then set the last bit if inexact), which rounds to fp32 as the exact sum would."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                             # two-sum: p + c == s + e exactly
    away = (e != 0) & ((e > 0) != (s > 0))                                     # |exact| < |s|: step one ulp towards zero
    t = np.where(away, np.nextafter(s, 0.0), s)
    ti = t.view(np.int64) | (e != 0).astype(np.int64)
    return ti.view(F64).astype(F32)


def dot_in_kernel_order(y, v, c):
    """The dot epilogue's documented order: per wave (32 features) and lane half the 16 terms by fma in register order, the two halves
    added, then the eight waves in wave order, then c."""
    M = y.shape[0]
    parts = []
    for w in range(8):
        halves = []
        for h in range(2):
            s = np.zeros(M, F32)
            for g in range(4):
                for e in range(4):
                    n = 32 * w + 8 * g + 4 * h + e
                    s = fma32(y[:, n], np.full(M, v[n], F32), s)
            halves.append(s)
        parts.append(halves[0] + halves[1])
    out = parts[0]
    for w in range(1, 8):
        out = out + parts[w]
    return out + F32(c)


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
def test_dot_form_equals_two_launches(dev, gelu):
    """The fused 512 -> 256 -> 1 tail == the 256-wide layer through mcr_linear_planes, then the 256-term dot on the host in the
    kernel's order; and a row's result does not depend on M (rows of M = 129 inside M = 1153)."""
    M, K = 1153, 512
    rng = np.random.default_rng(9)
    _, _, b, xh, xl, wh, wl = real_problem(dev, M, 256, K, seed=K + 1, scale=2.5)
    v = rng.standard_normal(256).astype(F32)
    for npl in (1, 2):
        y = run_linear(dev, Operands(dev, xh, xl, wh, wl, b), "f32", npl, 1.0 / 256.0, gelu=gelu)
        big = run_dot(dev, xh, xl, wh, wl, b, v, 0.25, npl, 1.0 / 256.0, gelu=gelu, tag="dot 1153")
        same_bits(big, dot_in_kernel_order(y, v, 0.25), f"dot form vs two launches planes={npl}")
        few = run_dot(dev, xh[:129], xl[:129], wh, wl, b, v, 0.25, npl, 1.0 / 256.0, gelu=gelu, tag="dot 129")
        same_bits(few, big[:129], f"dot form M = 129 inside M = 1153 planes={npl}")


# =====================================================================================================================================
# (c) split + GEMM against fp64 on the original fp32 values
# =====================================================================================================================================
def err_vs(got, ref, what):
    e = float(np.abs(got.astype(F64) - ref).max() / max(1.0, np.abs(ref).max()))
    print(f"ERR planes {what}: {e:.2e} (max|ref| {np.abs(ref).max():.2f})")
    assert np.isfinite(got).all(), what
    assert e < TOL, f"{what}: {e:.3e}"


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
@pytest.mark.parametrize("M,N,K", [(200, 192, 256), (129, 128, 384), (257, 132, 1344)], ids=["once", "small", "large"])
def test_against_fp64(dev, M, N, K, gelu):
    x, w, b, xh, xl, wh, wl = real_problem(dev, M, N, K, seed=M + K, scale=2.5 if gelu else 1.0)
    ops = Operands(dev, xh, xl, wh, wl, b)
    ref2 = st.linear_ref(x, w, b, gelu)
    # one plane: fp64 on the ROUNDED operands (what is left is accumulation and GELU error)
    ref1 = st.linear_ref(xh.astype(F32), wh.astype(F32) / 256.0, b, gelu)
    tag = f"{form_of(M, K)} M={M} N={N} K={K} gelu={gelu}"
    err_vs(run_linear(dev, ops, "f32", 2, 1.0 / 256.0, gelu=gelu), ref2, tag + " planes=2 fp32")
    hi, lo = run_linear(dev, ops, "planes", 2, 1.0 / 256.0, gelu=gelu)
    err_vs(hi.astype(F32) + lo.astype(F32), ref2, tag + " planes=2 hi+lo")
    err_vs(run_linear(dev, ops, "f32", 1, 1.0 / 256.0, gelu=gelu), ref1, tag + " planes=1 fp32")


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
def test_dot_against_fp64(dev, gelu):
    M, K = 129, 512
    x, w, b, xh, xl, wh, wl = real_problem(dev, M, 256, K, seed=77, scale=2.5 if gelu else 1.0)
    v = (np.random.default_rng(5).standard_normal(256) / 16.0).astype(F32)
    for npl, xr, wr in ((2, x, w), (1, xh.astype(F32), wh.astype(F32) / 256.0)):
        z = st.linear_ref(xr, wr, b, gelu) @ v.astype(F64) + 0.25
        ref = st.gelu64(z) if gelu else z
        got = run_dot(dev, xh, xl, wh, wl, b, v, 0.25, npl, 1.0 / 256.0, gelu=gelu, gelu2=gelu, tag="dot fp64")
        err_vs(got, ref, f"dot M={M} K={K} gelu={gelu} planes={npl}")


# =====================================================================================================================================
# (d) mcr_split_to_planes bit for bit against numpy
# =====================================================================================================================================
def split_inputs():
    """name -> fp32 values of one class where a split can go wrong (all finite, |x| < 65520: fp16(x) is finite)."""
    rng = np.random.default_rng(3)
    f = lambda b: np.asarray(b, np.uint32).view(F32)
    pm = lambda a: np.concatenate([a, -a]).astype(F32)
    ulp16 = lambda e: 2.0 ** (e - 10)
    cls = {}
    cls["zeros"] = np.array([0.0, -0.0], F32)
    # hi an fp16 subnormal (|x| < 2^-14): multiples of 2^-24 exactly, in between, and below the smallest subnormal
    cls["subnormal hi"] = pm(np.array([2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 1023 * 2.0 ** -24, 2.0 ** -24 * 1.25, 2.0 ** -24 * 1.5,
                                       2.0 ** -24 * 2.5, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -26, 2.0 ** -30, 1e-20, 1e-38, 1e-42]))
    # hi normal, lo an fp16 subnormal or zero: x = hi (1 + small)
    his = np.array([1.0, 1.5, 2.0 ** -10, 0.001, 3.14159, 2.0 ** -14], F64)
    cls["subnormal lo"] = pm(np.concatenate([his + k * 2.0 ** -24 for k in (0, 1, 3, 0.5, 1.5, 2.5, 100.25)]))
    # exact halfway cases of the rounding to fp16, even and odd neighbours below, at several exponents
    halves = []
    for e in (-14, -3, 0, 7, 15):
        for m in (0, 1, 2, 511, 1022):
            halves.append((1.0 + m * 2.0 ** -10) * 2.0 ** e + 0.5 * ulp16(e))
    cls["halfway hi"] = pm(np.array([h for h in halves if h < 65520.0]))
    # lo itself halfway between two fp16 values: x = 1 + (m + 0.5) 2^-21 (lo near 2^-11: ulp 2^-21 ... )
    cls["halfway lo"] = pm(np.array([1.0 + 2.0 ** -11 * (1.0 + (m + 0.5) * 2.0 ** -10) * 0.5 for m in (0, 1, 2, 3, 510, 511)]))
    cls["below 65504"] = pm(np.array([65503.996, 65504.0, 65500.0, 65488.0, 65519.996, 65519.0, 65472.0 + 16.0]))
    cls["2^14 and up"] = pm(np.array([16384.0, 16384.002, 20000.123, 32768.0, 32767.998, 40000.5, 49151.99, 65000.01]))
    e = rng.integers(113, 143, 4096).astype(np.uint32)                         # fp16 normal range: 2^-14 .. 2^16
    x = f((rng.integers(0, 2, 4096).astype(np.uint32) << 31) | (e << 23) | rng.integers(0, 1 << 23, 4096).astype(np.uint32))
    cls["random bits"] = x[np.abs(x) < 65504.0]
    for k, a in cls.items():
        assert np.isfinite(a).all() and np.abs(a).max() < 65520.0, k
    return cls


def test_split_classes(dev):
    cls = split_inputs()
    x = np.concatenate(list(cls.values()))
    names = np.concatenate([[k] * len(a) for k, a in cls.items()])
    E = 64
    n = -(-x.size // E) * E
    xp = np.concatenate([x, np.ones(n - x.size, F32)]).reshape(-1, E)
    hi, lo = device_split(dev, xp)
    whi, wlo = split_np(xp)
    for got, want, pl in ((hi, whi, "hi"), (lo, wlo, "lo")):
        bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
        assert bad.size == 0, (f"{pl}: {bad.size} differ: " +
                               "; ".join(f"{names[i] if i < x.size else 'pad'} x={xp.ravel()[i]!r} ({bits(xp).ravel()[i]:#010x}) got "
                                         f"{bits(got).ravel()[i]:#06x} want {bits(want).ravel()[i]:#06x}" for i in bad[:12]))
    assert (bits(wlo).ravel()[:x.size] & 0x7C00 == 0).sum() > 40              # the reference really holds subnormal / zero low halves
    assert ((bits(whi).ravel()[:x.size] & 0x7C00 == 0) & (bits(whi).ravel()[:x.size] & 0x3FF != 0)).sum() > 10


@pytest.mark.parametrize("E,dx,dp,low", [(4, 4, 4, True), (64, 0, 8, True), (64, 8, 0, False), (1344, 4, 12, True), (1344, 0, 0, False)])
def test_split_layouts(dev, E, dx, dp, low):
    M = 37
    x = (np.random.default_rng(E + dx).standard_normal((M, E)) * 300.0).astype(F32)
    X = Arena(M, E, E + dx, 4, x, dev)
    Ph, Pl = HalfArena(M, E, E + dp, 4, device=dev), HalfArena(M, E, E + dp, 4, device=dev)
    sync_ok(c_split(X, X.ld, Ph, Pl if low else None, Ph.ld, M, E), "split")
    X.check_unchanged("split X")
    Ph.check_guard("split Ph")
    hi, lo = split_np(x)
    same_bits(Ph.packed(), hi, "hi")
    if low:
        Pl.check_guard("split Pl")
        same_bits(Pl.packed(), lo, "lo")
    else:
        Pl.check_unchanged("split Pl of a one-plane call")


def test_split_out_of_range_is_nonfinite(dev):
    """What the range guard relies on: beyond the fp16 range (and for inf / NaN) hi is non-finite, and a GEMM over such a plane gives a
    non-finite output in every row that held one, finite rows elsewhere."""
    M, K, N = 16, 64, 8
    x = np.ones((M, K), F32)
    vals = [np.inf, -np.inf, np.nan, 65520.0, -65520.0, 1e5, -3e38, 65536.0]
    for m, val in enumerate(vals):
        x[m, 5 * m + 1] = val
    hi, lo = device_split(dev, x)
    assert not np.isfinite(hi[np.arange(len(vals)), 5 * np.arange(len(vals)) + 1].astype(F32)).any()
    assert np.isfinite(hi[len(vals):].astype(F32)).all() and np.isfinite(lo[len(vals):].astype(F32)).all()
    w = np.ones((N, K), F16)
    for npl in (1, 2):
        y = run_linear(dev, Operands(dev, hi, lo, w, np.zeros_like(w)), "f32", npl, 1.0)
        assert not np.isfinite(y[:len(vals)]).any() and np.isfinite(y[len(vals):]).all()


# =====================================================================================================================================
# (e) refusals
# =====================================================================================================================================
def _refusal_base(dev, M=40, N=16, K=64):
    p = IntProblem(M, N, K, seed=1)
    ops = Operands(dev, p.xh, p.xl, p.wh, p.wl, p.bias, Lay(dx=8, ox=0, dw=8, ow=0))
    return p, ops


def assert_refused(rc, entry, outs):
    torch.cuda.synchronize()
    for o in outs:
        o.check_unchanged(f"{entry}: output of a refused call")
    assert rc == 1, f"{entry}: rc {rc} ({last_error()!r})"
    assert entry + ":" in last_error(), last_error()


LINEAR_VIOLATIONS = ["K % 32", "K < 32", "N % 4", "ldx % 8", "ldw % 8", "ldy % 4", "Xh unaligned", "Xl unaligned", "Wh unaligned", "Wl unaligned",
                     "n_planes 0", "n_planes 3", "Xl null", "Wl null", "Yl null", "ldx < K", "ldw < K", "ldy < N", "ldr < N", "both outputs",
                     "no output", "R with planes", "row_bias without groups", "bias unaligned", "row_bias unaligned", "Yh unaligned", "M 0"]


@pytest.mark.parametrize("what", LINEAR_VIOLATIONS)
def test_linear_planes_refuses(dev, what):
    p, ops = _refusal_base(dev)
    M, N, K = p.M, p.N, p.K
    Y, R = Arena(M, N, N + 4, device=dev), Arena(M, N, N + 4, data=np.zeros((M, N), F32), device=dev)
    Yh, Yl = HalfArena(M, N, N + 8, device=dev), HalfArena(M, N, N + 8, device=dev)
    RB = Arena(2, N, data=np.zeros((2, N), F32), device=dev)
    a = dict(Xh=ops.Xh.ptr, Xl=ops.Xl.ptr, ldx=ops.Xh.ld, Wh=ops.Wh.ptr, Wl=ops.Wl.ptr, ldw=ops.Wh.ld, bias=ops.B.ptr, Y=Y.ptr, Yh=None, Yl=None,
             ldy=Y.ld, M=M, N=N, K=K, gelu=0, inv=1.0, rb=None, rpg=0, rg=None, R=None, ldr=0, npl=2)
    planes_out = dict(Y=None, Yh=Yh.ptr, Yl=Yl.ptr, ldy=Yh.ld)
    change = {
        "K % 32": dict(K=48), "K < 32": dict(K=0), "N % 4": dict(N=14), "ldx % 8": dict(ldx=K + 4), "ldw % 8": dict(ldw=K + 4),
        "ldy % 4": dict(ldy=N + 2), "Xh unaligned": dict(Xh=a["Xh"] + 8), "Xl unaligned": dict(Xl=a["Xl"] + 8), "Wh unaligned": dict(Wh=a["Wh"] + 8),
        "Wl unaligned": dict(Wl=a["Wl"] + 8), "n_planes 0": dict(npl=0), "n_planes 3": dict(npl=3), "Xl null": dict(Xl=None), "Wl null": dict(Wl=None),
        "Yl null": dict(planes_out, Yl=None), "ldx < K": dict(ldx=K - 8), "ldw < K": dict(ldw=K - 8), "ldy < N": dict(ldy=N - 4),
        "ldr < N": dict(R=R.ptr, ldr=N - 4), "both outputs": dict(Yh=Yh.ptr, Yl=Yl.ptr), "no output": dict(Y=None),
        "R with planes": dict(planes_out, R=R.ptr, ldr=R.ld), "row_bias without groups": dict(rb=RB.ptr), "bias unaligned": dict(bias=a["bias"] + 4),
        "row_bias unaligned": dict(rb=RB.ptr + 4, rpg=20), "Yh unaligned": dict(planes_out, Yh=Yh.ptr + 4), "M 0": dict(M=0),
    }[what]
    a.update(change)
    rc = c_linear_planes(a["Xh"], a["Xl"], a["ldx"], a["Wh"], a["Wl"], a["ldw"], a["bias"], a["Y"], a["Yh"], a["Yl"], a["ldy"], a["M"], a["N"],
                         a["K"], a["gelu"], a["inv"], a["rb"], a["rpg"], a["rg"], a["R"], a["ldr"], a["npl"])
    assert_refused(rc, "mcr_linear_planes", [Y, Yh, Yl])


DOT_VIOLATIONS = ["K % 32", "ldx % 8", "ldw % 8", "Xh unaligned", "Wl unaligned", "n_planes 3", "Xl null", "ldx < K", "ldw < K", "v null",
                  "v unaligned", "bias unaligned", "out null", "M 0"]


@pytest.mark.parametrize("what", DOT_VIOLATIONS)
def test_linear_planes_dot_refuses(dev, what):
    p, ops = _refusal_base(dev, N=256)
    M, K = p.M, p.K
    V = Arena(1, 260, data=np.zeros((1, 260), F32), device=dev)
    O = Arena(M, 1, device=dev)
    a = dict(Xh=ops.Xh.ptr, Xl=ops.Xl.ptr, ldx=ops.Xh.ld, Wh=ops.Wh.ptr, Wl=ops.Wl.ptr, ldw=ops.Wh.ld, bias=ops.B.ptr, M=M, K=K, v=V.ptr, out=O.ptr,
             npl=2)
    a.update({
        "K % 32": dict(K=48), "ldx % 8": dict(ldx=K + 4), "ldw % 8": dict(ldw=K + 4), "Xh unaligned": dict(Xh=a["Xh"] + 8),
        "Wl unaligned": dict(Wl=a["Wl"] + 8), "n_planes 3": dict(npl=3), "Xl null": dict(Xl=None), "ldx < K": dict(ldx=K - 8),
        "ldw < K": dict(ldw=K - 8), "v null": dict(v=None), "v unaligned": dict(v=V.ptr + 4), "bias unaligned": dict(bias=a["bias"] + 4),
        "out null": dict(out=None), "M 0": dict(M=0),
    }[what])
    rc = c_dot(a["Xh"], a["Xl"], a["ldx"], a["Wh"], a["Wl"], a["ldw"], a["bias"], a["M"], a["K"], 0, 1.0, a["v"], None, 0, a["out"], a["npl"])
    assert_refused(rc, "mcr_linear_planes_dot", [O])


SPLIT_VIOLATIONS = ["E % 4", "ldx % 4", "ldp % 4", "X unaligned", "Ph unaligned", "Pl unaligned", "ldx < E", "ldp < E", "Ph null", "M 0"]


@pytest.mark.parametrize("what", SPLIT_VIOLATIONS)
def test_split_to_planes_refuses(dev, what):
    M, E = 9, 16
    X = Arena(M, E, E + 4, data=np.ones((M, E), F32), device=dev)
    Ph, Pl = HalfArena(M, E, E + 4, device=dev), HalfArena(M, E, E + 4, device=dev)
    a = dict(X=X.ptr, ldx=X.ld, Ph=Ph.ptr, Pl=Pl.ptr, ldp=Ph.ld, M=M, E=E)
    a.update({
        "E % 4": dict(E=14), "ldx % 4": dict(ldx=E + 2), "ldp % 4": dict(ldp=E + 2), "X unaligned": dict(X=X.ptr + 4), "Ph unaligned": dict(Ph=Ph.ptr + 4),
        "Pl unaligned": dict(Pl=Pl.ptr + 2), "ldx < E": dict(ldx=E - 4), "ldp < E": dict(ldp=E - 4), "Ph null": dict(Ph=None), "M 0": dict(M=0),
    }[what])
    rc = c_split(a["X"], a["ldx"], a["Ph"], a["Pl"], a["ldp"], a["M"], a["E"])
    assert_refused(rc, "mcr_split_to_planes", [Ph, Pl])
