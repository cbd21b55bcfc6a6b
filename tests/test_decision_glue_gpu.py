"""The decision-glue kernels (csrc/glue.hip) entry by entry, at their edges, against exact host models: the proxy sampler, the frustum
mask, the signed distance to a depth map, the single-frame scene update, view-state binning, the point transform, depth unprojection,
n-camera gains, the distance-weighted MACARONS gain and the arg-max records.  Host models: oracle/view_state.py,
oracle/macarons_regime.py, oracle/scene.py, tests/_frames_model.py and, for what those do not cover, tests/_glue_model.py.

The exactness device: fp32 inputs are small dyadic numbers (integers times 2^-k, matrices over {0, +-1, +-0.5, ...}), so every product
and sum is exact in fp32 whether or not the compiler contracts it into an fma, and the comparison is array_equal; every such case
asserts on the host that its intermediates are exact (fp32 evaluation == fp64 evaluation).  Where a shape makes a quotient inexact
(-min(H, W) / W for W = 3 or 5, j / (m - 1) for m = 24) the equality rests on glue.hip's own `-ffp-contract=off`, and the case says so.

Case -> branch of glue.hip it reaches (conditions read from the code):
  test_sampler_sizes[65537-*]                    smp_block_sums: second 256-wide round of the block-sum scan with a non-zero carry (257 sums)
  test_sampler_sizes[*-3 / 1023 / 1025 / 4095]   smp_unique: padding keys (n_sample not a power of two)
  test_sampler_sizes[*] (n >= 14)                twelve uniforms EXACTLY on a CDF step (the kept total is a power of two): `>=` picks i, not i + 1
  test_sampler_patterns[nothing_kept*]           smp_unique: the invalid key -> inverse 0, n_unique 0, zero-filled gather; volume 0
  test_sampler_patterns[equal_min_occ]           `p > min_occ` is strict in smp_block_sums, smp_search and the backward walk
  test_sampler_patterns[one_kept_*]              one kept point at 0 / 255 / 256 / P - 1: every sample ends on it
  test_sampler_patterns[empty_chunk_between]     a block whose sum is 0 between two kept blocks (equal exclusive offsets)
  test_sampler_patterns[first_chunk_only]        2049 points kept only in block 0, u = 0.99999994 and u = 1 (the last step): with exact
                                                 sums the offsets of the empty blocks EQUAL the total, the binary search stays in block 0
                                                 and neither walk runs -- the walks need rounding, see the next two
  test_sampler_walks[forward]                    smp_search forward walk: u = 1, the in-block running sum ends one ulp under the total,
                                                 the loop moves to the (empty) later blocks and falls back on the last kept point
  test_sampler_walks[backward]                   smp_search backward walk (`for blk = lo - 1 ...`): u = 1, the exclusive offset of an EMPTY
                                                 trailing block is one ulp under the total, the search starts there and keeps nothing
                                                 (both from occupancies spread over 2^36, min_occ 0; the model's fp64 additions are in the
                                                 kernels' order and its trace says which walk ran)
  test_sampler_patterns[all_same / all_distinct] n_unique = 1 / n_unique = n_sample = 4096
  test_sampler_patterns[u0_first_not_kept]       u = 0 with point 0 not kept: the first KEPT point
  test_fov_mask[*]                               inclusive ndc bounds, z_view == 0, pw == 0 and < 0, distance == range, range <= 0, max < min
  test_signed_distance_dyadic[*]                 ix1 == W and iy1 == H skips, the clamp on either side, H > W, a mask under each tap
  test_signed_distance_border_column             the east tap at ix1 == W must not be READ (its weight is 0; the pixel there is inf)
  test_view_state_poles_and_axes                 yr = +-1 (cos(elev) ~ 0), q = +-1, x < 0 meeting azim = pi; +-Y on the 4 x 6 lattice sits
                                                 EXACTLY on the elevation rounding threshold (fmod(pi/2, pi/5) == pi/10 in fp32)
  test_view_state_lattice_centres[*]             one ray per bin, a quarter step off the lattice angles (the bin centres themselves are
                                                 discontinuities of upstream's fp32 formula: _glue_model.decision_margin)
  test_view_state_zero_length_ray                NaN direction: the final `%` and its fix-up keep the index inside the row
"""
import ctypes

import numpy as np
import pytest
import torch

import _frames_model as FM
import _glue_model as G
from _strided import Arena, Workspace, FILL_BITS
from oracle import view_state as V
from test_abi_strided_gpu import refused, last_error

pytestmark = pytest.mark.gpu

F = np.float32
I64, CI, VP, SZ, CF = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float


def L_():
    from macarons_amd import _lib
    return _lib.lib()


def stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {last_error()}"


class Guarded:
    """A device tensor of any dtype inside one allocation with PAD sentinel elements on either side (compared as bits)."""
    PAD = 64

    def __init__(self, shape, dtype, dev, fill=None, data=None):
        n = int(np.prod(shape))
        fill = {torch.float32: float("nan"), torch.float64: float("nan")}.get(dtype, 0x5A) if fill is None else fill
        self.buf = torch.full((n + 2 * self.PAD,), fill, dtype=dtype, device=dev)
        self.t = self.buf[self.PAD:self.PAD + n].view(shape)
        if data is not None:
            self.t.copy_(torch.as_tensor(data).to(dtype).reshape(shape))
        self.bits = self.buf.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[self.buf.element_size()])
        self.initial = self.bits.clone()
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def check_guard(self, what=""):
        for sl in (slice(0, self.PAD), slice(self.PAD + self.n, None)):
            assert torch.equal(self.bits[sl], self.initial[sl]), f"{what}: stray write outside the operand"

    def check_unchanged(self, what=""):
        assert torch.equal(self.bits, self.initial), f"{what}: changed"


def P_(g):
    return VP(g.ptr) if g is not None else VP(None)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# =====================================================================================================================================
# 1. sampler
# =====================================================================================================================================
def dy_occ(rng, P):
    """Occupancies that are multiples of 2^-10 in (0, 1]: every fp64 running sum is exact in any order."""
    return (rng.integers(1, 1025, P) / 1024.0).astype(F)


def dy_occ_pow2(rng, P, last_kept=True):
    """Occupancies against min_occ = 0.25 whose kept total is a power of two: K = 2^k of the P points are kept, in pairs
    (0.5 + d, 0.5 - d) with d a multiple of 2^-10 below 0.25; the others are 0.25 (exactly min_occ: not kept) or 0.125.  Every
    running sum C_i is then a multiple of 2^-10 below 2^14 and u = C_i / C_last is exact in fp32: EVERY kept point offers a uniform
    that sits exactly on its CDF step."""
    K = 1 << int(np.log2(max(1, int(0.6 * P))))
    kept = np.sort(rng.choice(P - 1, K - 1, replace=False)) if last_kept else np.sort(rng.choice(P, K, replace=False))
    kept = np.append(kept, P - 1).astype(np.int64) if last_kept else kept
    occ = np.where(rng.random(P) < 0.5, F(0.25), F(0.125)).astype(F)
    d = rng.integers(0, 256, K // 2) / 1024.0
    v = np.full(K, 0.5)
    v[0:2 * (K // 2):2] += d
    v[1:2 * (K // 2):2] -= d
    occ[kept] = v.astype(F)
    total = float(occ[kept].astype(np.float64).sum())
    assert total == K / 2 and (occ[kept] > 0.25).all()
    return occ


def mixed_uniforms(rng, occ, min_occ, n):
    """n uniforms: 0, 0.99999994, values exactly on CDF steps (the last step, u = 1, among them), the rest random."""
    u = rng.uniform(0, 1, n).astype(F)
    fixed = [F(0.0), F(0.99999994)]
    if (occ > F(min_occ)).any():
        fixed += list(G.on_step_uniforms(occ, min_occ, 12)[0])
    k = min(n, len(fixed))
    u[:k] = fixed[:k]
    return u


def sampler_exact(occ):
    assert G.is_dyadic(occ, 10) and len(occ) * 1024 < 2 ** 52, "the fp64 sums of this case are not exact"


class SamplerCall:
    """One ctypes call of mcr_sample_proxy / _batched / _shared on guarded outputs and a guarded workspace of exactly the bytes the
    entry asks for.  tab [B, P, stride] holds the occupancies in column col."""

    def __init__(self, dev, X, tab, col, vh, u, min_occ, entry):
        self.dev, self.entry, self.min_occ = dev, entry, min_occ
        self.B, self.P, self.stride = tab.shape
        self.col, self.n = col, u.shape[-1]
        B, n = self.B, self.n
        self.X, self.tab, self.u = T(X, dev), T(tab, dev), T(u, dev)
        self.vh = T(vh, dev) if vh is not None else None
        self.res = Guarded((B, n, 4), torch.float32, dev)
        self.res_h = Guarded((B, n, 64), torch.float32, dev) if vh is not None else None
        self.uniq = Guarded((B, n), torch.int64, dev)
        self.inv = Guarded((B, n), torch.int64, dev)
        self.nu = Guarded((B,), torch.int32, dev)
        self.vol = Guarded((B,), torch.float64, dev)
        L = L_()
        self.ws_bytes = int(L.mcr_sample_proxy_workspace_bytes(I64(self.P), CI(n)) if entry == "single" else
                            L.mcr_sample_proxy_batched_workspace_bytes(I64(B), I64(self.P), CI(n)))
        self.ws = Workspace(self.ws_bytes, device=dev)

    def outs(self):
        return [o for o in (self.res, self.res_h, self.uniq, self.inv, self.nu, self.vol) if o is not None]

    def run(self, n_sample=None):
        L = L_()
        n = self.n if n_sample is None else n_sample
        pre = VP(self.tab.data_ptr() + 4 * self.col)
        tail = (CF(self.min_occ), VP(self.u.data_ptr()), CI(n), P_(self.res), P_(self.res_h), P_(self.uniq), P_(self.inv), P_(self.nu),
                P_(self.vol), VP(self.ws.ptr), SZ(self.ws_bytes), stream())
        vh = VP(self.vh.data_ptr()) if self.vh is not None else VP(None)
        if self.entry == "single":
            return L.mcr_sample_proxy(VP(self.X.data_ptr()), pre, I64(self.stride), vh, I64(self.P), *tail)
        fn = L.mcr_sample_proxy_shared if self.entry == "shared" else L.mcr_sample_proxy_batched
        return fn(VP(self.X.data_ptr()), pre, I64(self.stride), vh, I64(self.B), I64(self.P), *tail)

    def result(self):
        return (self.res.np(), self.res_h.np() if self.res_h is not None else None, self.inv.np(), self.uniq.np(), self.nu.np(),
                self.vol.np())

    def check_guards(self, what):
        for o in self.outs():
            o.check_guard(what)
        self.ws.check_guard(what + ": workspace")


def check_cloud(got, b, ref, what):
    """got: result() of a call, cloud b of it against the model's (res, res_h, inverse, uniq, n_unique, volume), bit for bit."""
    res, res_h, inv, uniq, nu, vol = ref
    assert int(got[4][b]) == nu, f"{what}: n_unique {int(got[4][b])} != {nu}"
    assert bits_equal(got[5][b], np.float64(vol)), f"{what}: volume {got[5][b]!r} != {vol!r}"
    assert np.array_equal(got[2][b], inv), f"{what}: inverse"
    assert np.array_equal(got[3][b], uniq), f"{what}: unique indices"
    assert bits_equal(got[0][b], res), f"{what}: res"
    if res_h is not None:
        assert bits_equal(got[1][b], res_h), f"{what}: res_harmonics"


def run_twice_and_check(call, refs, what):
    """The same call twice on the same workspace, not re-zeroed in between (the kernel leaves the ticket ready): bit-equal results,
    intact guards, every cloud equal to its model."""
    ok(call.run(), what)
    first = call.result()
    ok(call.run(), what + " (second call)")
    second = call.result()
    for a, b in zip(first, second):
        assert (a is None and b is None) or bits_equal(a, b), f"{what}: the second call on the same workspace differs"
    call.check_guards(what)
    for b, ref in enumerate(refs):
        check_cloud(second, b, ref, f"{what} cloud {b}")


SIZES = [(1, 1), (255, 2), (256, 3), (257, 1023), (2047, 1024), (2048, 1025), (2049, 4095), (65536, 4096), (65537, 1024), (65537, 3),
         (257, 4096)]


@pytest.mark.parametrize("P,n", SIZES, ids=[f"{p}-{n}" for p, n in SIZES])
def test_sampler_sizes(dev, P, n):
    """ops.sample_proxy with explicit samples over the sizes at which the block sums, the scan and the sort change shape."""
    from macarons_amd import ops
    rng = np.random.default_rng(1000 * P + n)
    occ = dy_occ_pow2(rng, P)                                    # the last point (the 257th block of 65537) is kept
    sampler_exact(occ)
    X = rng.integers(-512, 512, (P, 3)).astype(F) / 256
    vh = rng.integers(-64, 64, (P, 64)).astype(F) / 32
    u = mixed_uniforms(rng, occ, 0.25, n)
    assert n < 14 or P < 255 or len(G.on_step_uniforms(occ, 0.25, 12)[0]) == 12, "too few uniforms exactly on a CDF step"
    ref = G.sample_proxy(X, occ, vh, u, 0.25)
    got = ops.sample_proxy(T(X, dev), T(occ[:, None], dev), T(vh, dev), T(u, dev), 0.25, return_volume=True, padded=True)
    res, resh, inv, uniq, nu, vol = (t.cpu().numpy() for t in got)
    check_cloud((res[None], resh[None], inv[None], uniq[None], nu, vol), 0, ref, f"P {P} n {n}")
    if P == 65537 and not G.PERTURB:
        assert (ref[3][:ref[4]] >= 65536).any(), "no sample reaches the block behind the scan's first round"


def pattern(name):
    """-> (P, occ, min_occ, u, expectation checked on the model's result)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    mo = 0.25
    if name.startswith("nothing_kept"):
        P = 257 if name == "nothing_kept" else 1
        occ = np.where(rng.random(P) < 0.5, F(0.25), F(0.125)).astype(F)
        return P, occ, mo, mixed_uniforms(rng, occ, mo, 5), lambda r: r[4] == 0 and r[5] == 0.0 and not r[2].any() and not r[0].any()
    if name.startswith("one_kept_"):
        P = 600
        at = {"first": 0, "last": P - 1, "255": 255, "256": 256}[name[9:]]
        occ = np.where(rng.random(P) < 0.5, F(0.25), F(0.0625)).astype(F)
        occ[at] = F(0.75)
        return P, occ, mo, mixed_uniforms(rng, occ, mo, 5), lambda r: r[4] == 1 and r[3][0] == at and r[5] == 0.75
    if name == "equal_min_occ":
        P = 300
        occ = dy_occ(rng, P)
        occ[::2] = F(0.25)
        return P, occ, mo, mixed_uniforms(rng, occ, mo, 64), lambda r: (r[0][:r[4], 3] > 0.25).all() and (r[3][:r[4]] % 2 == 1).all()
    if name == "empty_chunk_between":
        P = 768
        occ = dy_occ(rng, P)
        occ[256:512] = np.where(rng.random(256) < 0.5, F(0.25), F(0.125))
        u = mixed_uniforms(rng, occ, mo, 257)
        return P, occ, mo, u, lambda r: not ((r[3][:r[4]] >= 256) & (r[3][:r[4]] < 512)).any() and (r[3][:r[4]] >= 512).any()
    if name == "first_chunk_only":
        P = 2049
        occ = np.full(P, F(0.125))
        occ[:256] = dy_occ(rng, 256)
        occ[255] = F(0.5)
        u = mixed_uniforms(rng, occ, mo, 33)
        assert u[1] == F(0.99999994) and F(1.0) in u
        return P, occ, mo, u, lambda r: (r[3][:r[4]] < 256).all() and r[3][r[4] - 1] == 255
    if name == "all_same":
        P = 1000
        occ = dy_occ(rng, P)
        return P, occ, 0.0, np.full(1025, F(0.5)), lambda r: r[4] == 1 and not r[2].any()
    if name == "all_distinct":
        P = 4096
        occ = np.full(P, F(0.5))
        u = ((rng.permutation(P) + 1) / 4096.0).astype(F)           # every u on its own step C_i / C_last = (i + 1) / 4096
        return P, occ, mo, u, lambda r: r[4] == 4096 and np.array_equal(r[3][r[2]], np.round(u * 4096).astype(np.int64) - 1)
    if name == "u0_first_not_kept":
        P = 300
        occ = dy_occ(rng, P)
        occ[:7] = F(0.25)
        occ[7] = F(0.5)
        u = np.array([0.0, 0.0, 0.5], F)
        return P, occ, mo, u, lambda r: r[3][0] == 7 and r[2][0] == 0 and r[2][1] == 0
    raise KeyError(name)


PATTERNS = ["nothing_kept", "nothing_kept_p1", "one_kept_first", "one_kept_last", "one_kept_255", "one_kept_256", "equal_min_occ",
            "empty_chunk_between", "first_chunk_only", "all_same", "all_distinct", "u0_first_not_kept"]


@pytest.mark.parametrize("name", PATTERNS)
def test_sampler_patterns(dev, name):
    """Kept patterns through the C entry on a guarded workspace of exactly the bytes it asks for, called twice."""
    P, occ, mo, u, expect = pattern(name)
    sampler_exact(occ)
    rng = np.random.default_rng(5)
    X = rng.integers(-512, 512, (P, 3)).astype(F) / 256
    vh = rng.integers(-64, 64, (P, 64)).astype(F) / 32
    ref = G.sample_proxy(X, occ, vh, u, mo, want_trace=True)
    tr = ref[-1]
    if not G.PERTURB:
        assert expect(ref), f"{name}: the case does not show what it is for"
        if name == "first_chunk_only":
            assert not tr.lo.any() and not tr.moved_on.any() and not tr.backward.any()
    call = SamplerCall(dev, X, occ.reshape(1, P, 1), 0, vh, u, mo, "single")
    run_twice_and_check(call, [ref[:6]], name)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_sampler_walks(dev, which):
    """The two walks of smp_search need a target that rounding puts past the kept points the block offsets promise: occupancies spread
    over 36 binades (kept from min_occ = 0), 1024 of them in the first four blocks of a 2049-point cloud, u = 1.  The seeds were found
    on the host with the model, whose fp64 additions are in the kernels' order; its trace proves the branch, the oracle the result."""
    seed = {"forward": 3, "backward": 0}[which]
    rng = np.random.default_rng(seed)
    P = 2049
    occ = np.zeros(P, F)
    occ[:1024] = (rng.uniform(0.5, 1.0, 1024) * 2.0 ** -rng.integers(0, 36, 1024)).astype(F)
    X = rng.uniform(-1, 1, (P, 3)).astype(F)
    u = np.array([1.0, 0.99999994, 0.0, 0.5], F)
    ref = G.sample_proxy(X, occ, None, u, 0.0, want_trace=True)
    tr = ref[-1]
    if not G.PERTURB:
        assert tr.moved_on[0] and tr.found_in[0] < 0 and ref[3][ref[2][0]] == 1023, "u = 1 must end on the last kept point by a walk"
        assert tr.backward[0] == (which == "backward") and (tr.lo[0] > 3) == (which == "backward")
    call = SamplerCall(dev, X, occ.reshape(1, P, 1), 0, None, u, 0.0, "single")
    run_twice_and_check(call, [ref[:6]], f"walk {which}")


@pytest.mark.parametrize("with_vh", [True, False])
def test_sampler_pred_stride_4(dev, with_vh):
    """Occupancies as column 3 of a [P, 4] table (pred_stride = 4), with and without view harmonics."""
    rng = np.random.default_rng(44)
    P, n = 700, 129
    tab = rng.integers(-8, 8, (1, P, 4)).astype(F)               # the other columns would change every pick
    occ = dy_occ_pow2(rng, P, last_kept=False)
    tab[0, :, 3] = occ
    sampler_exact(occ)
    X = rng.integers(-512, 512, (P, 3)).astype(F) / 256
    vh = rng.integers(-64, 64, (P, 64)).astype(F) / 32 if with_vh else None
    u = mixed_uniforms(rng, occ, 0.25, n)
    ref = G.sample_proxy(X, occ, vh, u, 0.25)
    run_twice_and_check(SamplerCall(dev, X, tab, 3, vh, u, 0.25, "single"), [ref], f"stride 4 vh {with_vh}")


def test_sampler_batched_and_shared(dev):
    """B = 3 clouds with three patterns (one empty): each equals its own single call and its model; the shared form equals the batched
    form on a repeated X and vh."""
    rng = np.random.default_rng(45)
    B, P, n = 3, 2049, 257
    occ = np.stack([dy_occ_pow2(rng, P), np.where(rng.random(P) < 0.5, F(0.25), F(0.125)).astype(F), dy_occ(rng, P)])
    occ[2, 256:1800] = F(0.125)
    for b in range(B):
        sampler_exact(occ[b])
    X = rng.integers(-512, 512, (B, P, 3)).astype(F) / 256
    vh = rng.integers(-64, 64, (B, P, 64)).astype(F) / 32
    u = np.stack([mixed_uniforms(rng, occ[b], 0.25, n) for b in range(B)])
    refs = [G.sample_proxy(X[b], occ[b], vh[b], u[b], 0.25) for b in range(B)]
    assert G.PERTURB or (refs[1][4] == 0 and refs[0][4] > 1 and refs[2][4] > 1)
    call = SamplerCall(dev, X, occ.reshape(B, P, 1), 0, vh, u, 0.25, "batched")
    run_twice_and_check(call, refs, "batched")
    batched = call.result()
    for b in range(B):
        single = SamplerCall(dev, X[b], occ[b].reshape(1, P, 1), 0, vh[b], u[b:b + 1], 0.25, "single")
        ok(single.run(), f"single {b}")
        for g1, g2 in zip(single.result(), batched):
            assert bits_equal(g1[0], g2[b]), f"cloud {b}: the batched call differs from the single call"
    Xr, vhr = np.repeat(X[:1], B, 0), np.repeat(vh[:1], B, 0)
    rep = SamplerCall(dev, Xr, occ.reshape(B, P, 1), 0, vhr, u, 0.25, "batched")
    sh = SamplerCall(dev, X[0], occ.reshape(B, P, 1), 0, vh[0], u, 0.25, "shared")
    ok(rep.run(), "batched on a repeated X")
    run_twice_and_check(sh, [G.sample_proxy(X[0], occ[b], vh[0], u[b], 0.25) for b in range(B)], "shared")
    for g1, g2 in zip(rep.result(), sh.result()):
        assert bits_equal(g1, g2), "the shared form differs from the batched form on a repeated X and vh"


def test_sampler_refuses_4097_samples(dev):
    rng = np.random.default_rng(46)
    P = 300
    occ = dy_occ(rng, P)
    u = rng.uniform(0, 1, (1, 4097)).astype(F)
    call = SamplerCall(dev, rng.standard_normal((P, 3)).astype(F), occ.reshape(1, P, 1), 0, rng.standard_normal((P, 64)).astype(F), u, 0.25,
                       "single")
    refused(call.run(), "n_sample 4097", "n_sample <= 4096", call.outs())
    refused(call.run(0), "n_sample 0", "n_sample <= 4096", call.outs())
    call.ws.check_unchanged("workspace of a refused call")


# =====================================================================================================================================
# 2. frustum mask and masked occupancy
# =====================================================================================================================================
def fov_cameras():
    """Five dyadic camera records.  ndc = (x, y) / pw with pw = z (0, 1), pw = 0.5 z + 0.5 (2, 4), pw = 1 (3)."""
    cams = np.zeros((5, 40), F)
    cams[:, 32:36] = [-1.0, 1.0, -0.5, 0.5]
    cams[:, :16] = np.eye(4, dtype=F).reshape(-1)
    base = np.zeros((4, 4), F)
    base[0, 0] = base[1, 1] = 1.0
    base[2, 2], base[2, 3], base[3, 2] = 1.0, 1.0, -0.5
    for c in range(5):
        cams[c, 16:32] = base.reshape(-1)
    cams[1, 14] = -0.5                                            # z_view = z - 0.5: zero on the plane z = 0.5
    cams[1, 36:40] = [1.0, -1.0, 0.0, 5.0]                        # range 5 around (1, -1, 0): 3-4-5 offsets sit exactly on it
    cams[2, 16 + 11], cams[2, 16 + 15] = 0.5, 0.5                 # pw = 0.5 z + 0.5: zero at z = -1
    cams[2, 39] = -3.0                                            # negative range: no range test
    cams[3, 16 + 11], cams[3, 16 + 15] = 0.0, 1.0                 # pw = 1
    cams[3, 32:36] = [0.5, -0.5, -2.0, 2.0]                       # empty frustum (max_x < min_x)
    cams[4, 16 + 0], cams[4, 16 + 4] = 0.5, -0.5                  # px = 0.5 x - 0.5 y
    cams[4, 16 + 11], cams[4, 16 + 15] = 0.5, 0.5
    cams[4, 32:36] = [-0.25, 0.25, -1.0, 1.0]
    cams[4, 36:40] = [0.0, 0.0, 0.0, 0.0]                         # range 0: no range test
    return cams


def fov_points():
    """A lattice of multiples of 1/4 (z from -2 to 4, including 0, 0.5 and -1), the 3-4-5 offsets of camera 1 first."""
    ax = np.arange(-12, 13) / 4.0
    zs = np.array([2.0, 1.0, 0.5, 0.0, -1.0, 4.0, -2.0, 0.25])
    g = np.stack(np.meshgrid(ax[::3], ax[::2], zs, indexing="ij"), -1).reshape(-1, 3)
    first = np.array([[2.0, 1.0, 2.0], [4.0, 3.0, 0.0], [1.0, 2.0, 4.0], [-2.0, -1.0, 2.0], [2.0, -1.0, 2.0], [1.0, 1.0, 2.0], [1.0, -1.0, 2.0],
                      [0.0, 0.0, 0.0], [0.5, 0.25, -1.0], [1.0, 1.0, -2.0], [1.0, 0.5, 1.0], [-1.0, -0.5, 1.0], [0.5, 0.25, 0.5]])
    rng = np.random.default_rng(7)
    return np.concatenate([first, g[rng.permutation(len(g))]]).astype(F)


@pytest.mark.parametrize("P,n_cam", [(1, 1), (255, 3), (256, 5), (257, 3), (257, 5), (255, 1)])
def test_fov_mask(dev, P, n_cam):
    """mcr_points_in_fov == oracle.macarons_regime.points_in_fov, and mcr_fov_mask_occ with occ_stride 1 and 4."""
    from macarons_amd import ops
    cams, pts = fov_cameras()[:n_cam], fov_points()[:P]
    assert len(pts) == P
    mask = ops.points_in_fov(T(pts, dev), T(cams, dev)).cpu().numpy()
    for c in range(n_cam):
        with np.errstate(divide="ignore", invalid="ignore"):
            assert G.fov_intermediates_exact(pts, cams[c]), f"camera {c}: an intermediate is not exact in fp32"
            ref = G.points_in_fov(pts, cams[c])
        assert np.array_equal(mask[c], ref), f"camera {c}: {np.flatnonzero(mask[c] != ref)[:8]}"
    if P >= 255 and not G.PERTURB:                                 # the edges are in the case
        p64 = pts.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            nx, ny = p64[:, 0] / p64[:, 2], p64[:, 1] / p64[:, 2]
        m0 = mask[0]
        for v, b in ((nx, -1.0), (nx, 1.0), (ny, -0.5), (ny, 0.5)):
            assert (m0 & (v == b)).any(), "no point ON an ndc bound inside the mask"
        assert (p64[:, 2] == 0).any() and not m0[p64[:, 2] == 0].any() and (p64[:, 2] < 0).any() and not m0[p64[:, 2] < 0].any()
        assert 0 < m0.sum() < P
        if n_cam >= 3:
            d = np.sqrt(((p64 - [1.0, -1.0, 0.0]) ** 2).sum(1))
            assert (mask[0] & (d == 5.0)).any() and not mask[1][d == 5.0].any() and mask[1].any(), "distance == range is outside"
            assert not mask[1][p64[:, 2] == 0.5].any() and mask[0][p64[:, 2] == 0.5].any(), "z_view == 0 is outside"
            assert mask[2].any() and (p64[:, 2] == -1).any()
        if n_cam == 5:
            assert not mask[3].any() and mask[4].any()
    # masked occupancy
    rng = np.random.default_rng(P)
    tab = rng.integers(1, 1025, (P, 4)).astype(F) / 1024
    got1 = ops.fov_mask_occ(T(mask, dev), T(tab[:, 0].copy(), dev)).cpu().numpy()
    assert bits_equal(got1, np.where(mask, tab[None, :, 0], F(0)).astype(F))
    out = Guarded((n_cam, P), torch.float32, dev)
    m8, tt = T(mask.astype(np.uint8), dev), T(tab, dev)
    ok(L_().mcr_fov_mask_occ(VP(m8.data_ptr()), VP(tt.data_ptr() + 12), I64(4), P_(out), I64(P), CI(n_cam), stream()), "fov_mask_occ")
    out.check_guard("fov_mask_occ stride 4")
    assert bits_equal(out.np(), np.where(mask, tab[None, :, 3], F(0)).astype(F))


# =====================================================================================================================================
# 3. signed distance and the single-frame update
# =====================================================================================================================================
def sd_camera(perspective):
    """M_view: z_view = (0.5 z + 0.25) / 2; projection: (x, y) / pw with pw = 1 or pw = z."""
    rec = np.zeros(40, F)
    Mv = np.eye(4, dtype=F)
    Mv[2, 2], Mv[3, 2], Mv[3, 3] = 0.5, 0.25, 2.0
    Mp = np.zeros((4, 4), F)
    Mp[0, 0] = Mp[1, 1] = 1.0
    if perspective:
        Mp[2, 3] = 1.0
    else:
        Mp[3, 3] = 1.0
    rec[:16], rec[16:32] = Mv.reshape(-1), Mp.reshape(-1)
    rec[32:36] = [-100.0, 100.0, -100.0, 100.0]
    return rec


def sd_points(H, W, perspective, n):
    """Points whose projections land on: every pixel centre, fx = 0 and fx = W - 1 exactly, outside the border on each side, halfway
    between pixels (all combinations of the x and y lists, shuffled, tiled to n)."""
    m = float(min(H, W))
    fxs = sorted(set([-1.5, -0.5, 0.0, 0.5, W - 1.5, W - 1.0, W - 0.5, W + 1.0] + [float(c) for c in range(W)]))
    fys = sorted(set([-1.5, -0.5, 0.0, 0.5, H - 1.5, H - 1.0, H - 0.5, H + 1.0] + [float(c) for c in range(H)]))
    g = np.stack(np.meshgrid(fxs, fys, indexing="ij"), -1).reshape(-1, 2)
    g = g[np.random.default_rng(H * 16 + W).permutation(len(g))]
    g = np.concatenate([g] * (n // len(g) + 1))[:n]
    px, py = (W - 2 * g[:, 0] - 1) / m, (H - 2 * g[:, 1] - 1) / m
    z = np.array([1.0, 2.0, 4.0, 0.5])[np.arange(n) % 4]
    s = z if perspective else 1.0
    return np.stack([px * s, py * s, z], 1).astype(F), g


def sd_depth(H, W, seed=0):
    return (np.random.default_rng(seed).integers(16, 80, (H, W)) / 16.0).astype(F)


SD_SHAPES = [(4, 8), (8, 4), (1, 5), (5, 1), (3, 3)]


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("H,W", SD_SHAPES, ids=[f"{h}x{w}" for h, w in SD_SHAPES])
def test_signed_distance_dyadic(dev, H, W, n):
    """mcr_signed_distance_to_depth == _frames_model.signed_distance on dyadic cameras, depths and points, with no mask and with a
    mask that clears each of the four taps in turn (and all of them)."""
    from macarons_amd import ops
    depth = sd_depth(H, W)
    for perspective in (False, True):
        rec = sd_camera(perspective)
        pts, want = sd_points(H, W, perspective, n)
        if (H, W) in ((4, 8), (8, 4)):                           # powers of two: the pixel coordinates are exact, the edges are hit
            fx32, fy32 = G.bilinear_coords(pts, rec, H, W, F)
            fx64, fy64 = G.bilinear_coords(pts, rec, H, W, np.float64)
            assert np.array_equal(fx32, fx64) and np.array_equal(fy32, fy64), "pixel coordinates not exact in fp32"
            assert np.array_equal(fx64, np.clip(want[:, 0], 0, W - 1)) and np.array_equal(fy64, np.clip(want[:, 1], 0, H - 1))
            if n >= 255:
                ux, uy = G.unclamped_coords(pts, rec, H, W)
                assert (ux < 0).any() and (ux > W - 1).any() and (uy < 0).any() and (uy > H - 1).any()
                assert (ux == 0).any() and (ux == W - 1).any() and (ux % 1 == 0.5).any() and (uy == H - 1).any()
        # (other shapes: -min(H, W) / W is not dyadic; equality there rests on glue.hip's -ffp-contract=off)
        masks = [None]
        if H > 1 and W > 1:
            for tap in ((1, 1), (1, 2), (2, 1), (2, 2)):         # the taps of the halfway point (1.5, 1.5)
                mk = np.ones((H, W), bool)
                mk[tap] = False
                masks.append(mk)
        masks.append(np.zeros((H, W), bool))
        for mk in masks:
            got = ops.signed_distance_to_depth(T(pts, dev), T(rec, dev), T(depth, dev), T(mk, dev) if mk is not None else None, 8.5)
            ref = G.signed_distance(pts, rec, depth, mk, 8.5)
            assert bits_equal(got.cpu().numpy(), ref), f"{H}x{W} n {n} perspective {perspective} mask {None if mk is None else (~mk).sum()}"


def test_signed_distance_border_column(dev):
    """At ix1 == W the east tap has weight 0 and must be SKIPPED, not multiplied: the pixel a stray read would find there (the next
    row's first one) is inf in this map, and every point sits on or beyond the right border."""
    from macarons_amd import ops
    H, W = 4, 8
    depth = sd_depth(H, W, 3)
    depth[:, 0] = np.inf
    rec = sd_camera(False)
    pts, want = sd_points(H, W, False, 257)
    pts = pts[want[:, 0] >= W - 1]
    got = ops.signed_distance_to_depth(T(pts, dev), T(rec, dev), T(depth, dev), None, 8.5).cpu().numpy()
    assert len(pts) > 40 and np.isfinite(got).all()
    assert bits_equal(got, G.signed_distance(pts, rec, depth, None, 8.5))


def real_camera(rng, rng_range=0.0):
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0].astype(F)
    Tt = rng.uniform(-1, 1, 3).astype(F) + np.array([0, 0, 6], F)
    Mv = np.eye(4, dtype=F)
    Mv[:3, :3], Mv[3, :3] = R, Tt
    f = 1.0 / np.tan(np.deg2rad(60) / 2)
    K = np.array([[f, 0, 0, 0], [0, f, 0, 0], [0, 0, 100 / 99, 1], [0, 0, -100 / 99, 0]], F)
    rec = np.zeros(40, F)
    rec[:16], rec[16:32] = Mv.reshape(-1), (Mv @ K).astype(F).reshape(-1)
    rec[32:36] = [-1.5, 1.5, -1.0, 1.0]
    rec[36:39] = -Tt @ R.T
    rec[39] = rng_range
    return rec


def test_signed_distance_real_valued(dev):
    """Real-valued camera, depth and points at the agreement tests/test_scone_step_gpu.py demands of the same device function: the
    frames entry (K = 1) and the single-frame entry give the same bits where the frustum bit is set, 0 elsewhere."""
    from macarons_amd import ops
    rng = np.random.default_rng(31)
    P, H, W = 2001, 37, 53
    pts = rng.uniform(-3, 3, (P, 3)).astype(F)
    rec = real_camera(rng)
    depth = rng.uniform(2, 9, (1, H, W)).astype(F)
    dmask = rng.random((1, H, W)) < 0.8
    bits, sgn, _ = ops.supervision_frames(T(pts, dev), T(rec[None], dev), T(depth, dev), T(dmask, dev), [110.0], 0.5)
    m = ops.points_in_fov(T(pts, dev), T(rec[None], dev))[0]
    assert torch.equal((bits & 1).bool(), m) and 100 < int(m.sum()) < P
    d = ops.signed_distance_to_depth(T(pts, dev)[m].contiguous(), T(rec, dev), T(depth[0], dev), T(dmask[0], dev), 110.0)
    assert torch.equal(sgn[0][m], d) and not sgn[0][~m].any()
    ref = FM.signed_distance(pts[m.cpu().numpy()], rec, depth[0], dmask[0], 110.0)
    print(f"ERR signed distance, real-valued, kernel vs the fp32 restatement: {float(np.abs(d.cpu().numpy() - ref).max()):.2e}")


@pytest.mark.parametrize("P", [1, 257])
def test_proxy_scene_update(dev, P):
    """mcr_proxy_scene_update == _frames_model.update_frames with K = 1 on all five tables, twice in a row (counters, the quotient
    exactly at the threshold), sgn bit-untouched where the frustum mask is clear, and the frames entry with K = 1 gives the same bits."""
    from macarons_amd import ops
    H, W, n_elev, n_azim = 4, 8, 7, 14
    rec, depth = sd_camera(False), sd_depth(H, W, 5)
    rng = np.random.default_rng(60 + P)
    # z chosen per point so that d = z_view - depth lands on -0.75, -0.5 (= -tol), 0.25 (|d| < tol), 1 (= distance_to_surface), 0.5
    pts, want = sd_points(H, W, False, P)
    ix, iy = np.clip(np.floor(want[:, 0] + 0.5), 0, W - 1).astype(int), np.clip(np.floor(want[:, 1] + 0.5), 0, H - 1).astype(int)
    px, py = (W - 2 * ix - 1) / 4.0, (H - 2 * iy - 1) / 4.0      # snapped to pixel centres: d is exactly what is asked for
    dwant = np.array([-0.75, -0.5, 0.25, 1.0, 0.5, -0.5, 0.25])[np.arange(P) % 7] if P > 1 else np.array([0.25])
    z = ((depth[iy, ix].astype(np.float64) + dwant) * 2 - 0.25) / 0.5
    pts = np.stack([px, py, z], 1).astype(F)
    sgn_ref = G.signed_distance(pts, rec, depth, None, 8.5)
    assert G.PERTURB or np.array_equal(sgn_ref.astype(np.float64), dwant), "the signed distances of this case are not the exact ones"
    X_cams = np.array([[0.5, 3.0, -2.0], [-4.0, -1.5, 9.0]], F)
    margin = np.minimum(*(G.decision_margin(pts[None], xc[None], n_elev, n_azim)[0, :, 0] for xc in X_cams))
    fov = ((rng.random(P) < 0.8) | (P == 1)) & (margin > 1e-3)     # the bins of the masked points do not depend on the libm at hand
    assert fov.sum() >= 0.6 * P
    tabs = [(rng.random((P, n_elev * n_azim)) < 0.05).astype(F), np.full(P, 3.0, F), np.where(rng.random(P) < 0.5, 2.0, 1.0).astype(F),
            (rng.random(P) < 0.5).astype(F), (rng.random(P) < 0.7).astype(F)]
    thr, tol, dts = 0.75, 0.5, 1.0                                 # (2 + 1) / (3 + 1) == 0.75: exactly at the threshold -> 1
    dev_tabs = [Guarded(t.shape, torch.float32, dev, data=t) for t in tabs]
    frames_tabs = [T(t, dev) for t in tabs]
    sgn = Arena(P, 1, device=dev)
    pp, fm, rc_, dd = T(pts, dev), T(fov.astype(np.uint8), dev), T(rec, dev), T(depth, dev)
    cur = tabs
    for it, xc in enumerate(X_cams):
        xcd = T(xc, dev)
        ok(L_().mcr_proxy_scene_update(VP(pp.data_ptr()), I64(P), VP(fm.data_ptr()), VP(rc_.data_ptr()), VP(dd.data_ptr()), VP(None), CI(H),
                                       CI(W), CF(8.5), VP(xcd.data_ptr()), CF(dts), CF(tol), CF(thr), CI(n_elev), CI(n_azim),
                                       *[P_(t) for t in dev_tabs], VP(sgn.ptr), stream()), "mcr_proxy_scene_update")
        cur = G.proxy_update(pts, fov, sgn_ref, xc, dts, tol, thr, n_elev, n_azim, cur)
        if it == 0 and P > 1 and not G.PERTURB:
            assert ((cur[2] / cur[1] == F(thr)) & (cur[3] == 1) & fov).any(), "no quotient exactly at the threshold"
        names = ("view_states", "n_inside", "n_behind", "supervision_occ", "out_of_field")
        for name, g, r in zip(names, dev_tabs, cur):
            g.check_guard(name)
            assert bits_equal(g.np(), r.astype(F)), f"call {it}: {name} rows {np.flatnonzero((g.np() != r).reshape(P, -1).any(1))[:8]}"
        sgn.check_guard("sgn")
        sb = sgn.packed().view(np.int32)[:, 0]
        assert (sb[~fov] == np.int32(FILL_BITS)).all(), "sgn written where the frustum mask is clear"
        assert bits_equal(sgn.packed()[fov, 0], sgn_ref[fov])
        for name, t0, r in zip(names, tabs, cur):
            assert bits_equal(np.asarray(r)[~fov], t0[~fov]), f"{name}: a row with a clear mask changed"
        # the frames entry, K = 1, from the same bits and distances
        s1 = T(np.where(fov, sgn_ref, F(0))[None], dev)
        ops.proxy_scene_update_frames_(pp, T(fov.astype(np.int32), dev), s1, T(xc[None], dev), dts, tol, thr, n_elev, n_azim, *frames_tabs)
        for name, g, f_ in zip(names, dev_tabs, frames_tabs):
            assert torch.equal(g.t, f_), f"call {it}: {name} differs between the single-frame and the frames entry"
    if P > 1 and not G.PERTURB:
        assert (fov & (sgn_ref == -0.5)).any() and (fov & (sgn_ref == 1.0)).any() and (fov & (sgn_ref == 0.25)).any()
    # ops.proxy_scene_update_ (the wrapper: its own zeroed sgn) on fresh tables gives the first call's tables
    t2 = [T(t, dev) for t in tabs]
    s = ops.proxy_scene_update_(pp, T(fov, dev), rc_, dd, None, 8.5, T(X_cams[0], dev), dts, tol, thr, n_elev, n_azim, *t2, return_sgn=True)
    first = G.proxy_update(pts, fov, sgn_ref, X_cams[0], dts, tol, thr, n_elev, n_azim, tabs)
    for g, r in zip(t2, first):
        assert bits_equal(g.cpu().numpy(), r.astype(F))
    assert bits_equal(s.cpu().numpy(), np.where(fov, sgn_ref, F(0)).astype(F))


# =====================================================================================================================================
# 4. view state
# =====================================================================================================================================
LATTICES = [(7, 14), (4, 6)]


@pytest.mark.parametrize("n_elev,n_azim", LATTICES)
@pytest.mark.parametrize("n_view", [1, 9])
def test_view_state_lattice_centres(dev, n_elev, n_azim, n_view):
    """One ray per bin of the lattice, a quarter step off the lattice angles in elevation and azimuth: far from every boundary AND from
    every bin centre (a discontinuity of upstream's fp32 formula too, see _glue_model.decision_margin), so array_equal with no
    exceptions."""
    from macarons_amd import ops
    d = G.lattice_rays(n_elev, n_azim, 1.5)
    pts = (-d).astype(F)                                          # ray = X_view - pts = d + X_view, X_view tiny
    rng = np.random.default_rng(n_view)
    Xv = (rng.integers(-1, 2, (n_view, 3)) * 2.0 ** -12).astype(F)
    margin = G.decision_margin(pts[None], Xv, n_elev, n_azim)
    assert margin.min() > 1e-3
    for dim in (3, 4):
        p = np.concatenate([pts, np.full((len(pts), dim - 3), 7.0, F)], 1)
        got = ops.view_state(T(p[None], dev), T(Xv, dev), n_elev, n_azim).cpu().numpy()[0]
        assert np.array_equal(got, G.compute_view_state(p, Xv, n_elev, n_azim))
        assert (got.sum(1) == 1).all()                            # the nine views of a point agree on its bin


# upstream's compute_view_state (scone_utils.py:799-860, with get_spherical_coords and floor_divide) evaluated with torch on the CPU on
# these rays (X_view = 0, point = -ray): the bins it sets.  +Y and -Y on the 4 x 6 lattice share bin 1: upstream's quirks, kept.
POLE_RAYS = np.array([[0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [-2.0 ** -20, 0, -1], [-2.0 ** -20, 0.5, -1],
                      [0, 2, 0], [3, 0, 0], [0, 0, -0.5]], F)
POLE_BINS_UPSTREAM = {(7, 14): [4, 88, 42, 49, 46, 52, 49, 63, 4, 46, 49], (4, 6): [1, 1, 12, 15, 13, 16, 15, 21, 1, 13, 15]}


@pytest.mark.parametrize("n_elev,n_azim", LATTICES)
def test_view_state_poles_and_axes(dev, n_elev, n_azim):
    from macarons_amd import ops
    pts, Xv = (-POLE_RAYS).astype(F), np.zeros((1, 3), F)
    got = ops.view_state(T(pts[None], dev), T(Xv, dev), n_elev, n_azim).cpu().numpy()[0]
    assert (got.sum(1) == 1).all()
    with np.errstate(all="ignore"):
        ref = G.view_state_indices(pts[None], Xv, n_elev, n_azim)[0, :, 0]
    print(f"view-state bins at the poles and axes, {n_elev} x {n_azim}: kernel {got.argmax(1).tolist()} model {ref.tolist()}")
    assert G.PERTURB or ref.tolist() == POLE_BINS_UPSTREAM[(n_elev, n_azim)], "the oracle left upstream's bins"
    assert got.argmax(1).tolist() == ref.tolist()
    if (n_elev, n_azim) == (4, 6):                                 # +-Y sits exactly on the elevation rounding threshold
        assert np.mod(F(np.pi / 2), F(np.pi / 5)) == F(np.pi / 5 / 2.)


def test_view_state_zero_length_ray(dev):
    """A point AT the camera: the direction is NaN, upstream defines no bin for it.  view_state_bin ends with `idx %= nb; if (idx < 0)
    idx += nb`, so whatever the NaN converts to, the written index is inside the row: one bin of that row is set, the guards and all
    other rows are intact (which bin is not asserted)."""
    n_elev, n_azim, P = 7, 14, 5
    nb = n_elev * n_azim
    rng = np.random.default_rng(3)
    pts = rng.integers(-8, 8, (P, 3)).astype(F) / 4
    Xv = (pts[2:3] + 0).astype(F)                                 # the camera sits on point 2
    other = np.delete(np.arange(P), 2)
    assert G.decision_margin(pts[None, other], Xv, n_elev, n_azim).min() > 1e-3
    prior = (rng.random((P, nb)) < 0.1).astype(F)
    prior[2] = 0
    table = Arena(P, nb, device=dev, data=prior)
    pd, xd = T(pts, dev), T(Xv, dev)
    ok(L_().mcr_view_state_batched(VP(pd.data_ptr()), CI(3), VP(xd.data_ptr()), VP(table.ptr), I64(1), I64(P), CI(1), CI(n_elev), CI(n_azim),
                                   VP(None), CI(1), stream()), "view state, zero-length ray")
    table.check_guard("zero-length ray")
    got = table.packed()
    ref = G.compute_view_state(pts[other], Xv, n_elev, n_azim, table=prior[other], rows=np.arange(P - 1))
    assert np.array_equal(got[other], ref), "a row other than the zero-length ray's changed wrongly"
    assert got[2].sum() == 1 and set(np.unique(got[2])) == {0.0, 1.0}


def safe_points(rng, n, Xv, n_elev, n_azim, dim=3):
    """n random points (multiples of 2^-8) whose rays to every view are more than 1e-3 rad from every place where the binning can
    change its answer (boundaries, the seam, bin centres)."""
    c = (rng.integers(-128, 129, (4 * n + 64, 3)) / 256.0).astype(F)
    m = np.minimum.reduce([G.decision_margin(c[None], x, n_elev, n_azim).min(-1)[0] for x in Xv.reshape(-1, Xv.shape[-2], 3)])
    c = c[m > 1e-3][:n]
    assert len(c) == n
    return np.concatenate([c, rng.standard_normal((n, dim - 3)).astype(F)], 1)


@pytest.mark.parametrize("P", [1, 255, 257])
@pytest.mark.parametrize("dim", [3, 4])
def test_view_state_shapes_and_batches(dev, P, dim):
    """n_view = 9, pts_dim 3 and 4, one cloud and three clouds with their own X_view each."""
    from macarons_amd import ops
    rng = np.random.default_rng(100 * P + dim)
    n_elev, n_azim, B = 7, 14, 3
    Xv = rng.integers(-6, 7, (B, 9, 3)).astype(F) / 4 + np.array([0, 0, 3], F)
    pts = np.stack([safe_points(rng, P, Xv, n_elev, n_azim, dim) for _ in range(B)])
    got1 = ops.view_state(T(pts[:1], dev), T(Xv[0], dev), n_elev, n_azim).cpu().numpy()[0]
    assert np.array_equal(got1, G.compute_view_state(pts[0], Xv[0], n_elev, n_azim))
    gotb = ops.view_state(T(pts, dev), T(Xv, dev), n_elev, n_azim).cpu().numpy()
    for b in range(B):
        assert np.array_equal(gotb[b], G.compute_view_state(pts[b], Xv[b], n_elev, n_azim)), f"cloud {b}"
    assert not np.array_equal(gotb[1], G.compute_view_state(pts[1], Xv[0], n_elev, n_azim)) or P == 1
    shared = ops.view_state(T(pts, dev), T(Xv[0], dev), n_elev, n_azim).cpu().numpy()           # mcr_view_state, B * P points
    for b in range(B):
        assert np.array_equal(shared[b], G.compute_view_state(pts[b], Xv[0], n_elev, n_azim))


def test_view_state_rows_and_accumulate(dev):
    """ops.view_state_update_: repeated target rows OR together, untouched rows keep their prior ones; accumulate = 0 zeroes first;
    a row index without accumulate is refused."""
    from macarons_amd import ops
    rng = np.random.default_rng(17)
    n_elev, n_azim, n, R = 7, 14, 257, 40
    nb = n_elev * n_azim
    Xv = rng.integers(-6, 7, (4, 3)).astype(F) / 4 + np.array([0, 0, 3], F)
    pts = safe_points(rng, n, Xv[None], n_elev, n_azim, 4)
    rows = rng.integers(0, R // 2, n).astype(np.int64) * 2          # even rows only, each several times
    prior = (rng.random((R, nb)) < 0.1).astype(F)
    table = T(prior, dev)
    ops.view_state_update_(table, T(rows, dev), T(pts, dev), T(Xv, dev), n_elev, n_azim)
    ref = G.compute_view_state(pts, Xv, n_elev, n_azim, table=prior, rows=rows)
    assert np.array_equal(table.cpu().numpy(), ref) and np.array_equal(ref[1::2], prior[1::2]) and not np.array_equal(ref, prior)
    before = (rng.random((n, nb)) < 0.1).astype(F)
    t2 = T(before, dev)
    ops.view_state_update_(t2, None, T(pts, dev), T(Xv, dev), n_elev, n_azim)                    # rows None: row i <- point i, OR'ed in
    assert np.array_equal(t2.cpu().numpy(), G.compute_view_state(pts, Xv, n_elev, n_azim, table=before, rows=np.arange(n)))
    # accumulate = 0 on a dirty table == a fresh one; with rows it is refused and nothing is written
    dirty = Arena(n, nb, device=dev, data=np.ones((n, nb), F))
    pd, xd, rd = T(pts, dev), T(Xv, dev), T(np.arange(n, dtype=np.int64), dev)
    args = lambda tab, r, acc: (VP(pd.data_ptr()), CI(4), VP(xd.data_ptr()), VP(tab.ptr), I64(1), I64(n), CI(4), CI(n_elev), CI(n_azim),   # noqa: E731
                                r, CI(acc), stream())
    ok(L_().mcr_view_state_batched(*args(dirty, VP(None), 0)), "accumulate 0")
    dirty.check_guard("accumulate 0")
    assert np.array_equal(dirty.packed(), G.compute_view_state(pts, Xv, n_elev, n_azim))
    keep = Arena(n, nb, device=dev, data=np.ones((n, nb), F))
    refused(L_().mcr_view_state_batched(*args(keep, VP(rd.data_ptr()), 0)), "rows without accumulate", "accumulate", [keep])


def test_view_state_random_rays_with_a_cap(dev):
    """The existing rule on random rays (a mismatch only within 2e-6 rad of a place where the binning decides) with a cap on how many
    rays may be excused.  SEED 2, P = 2000, 9 views: the closest ray is 3.1e-5 rad from a boundary and 2.9e-6 rad from a bin centre
    (_glue_model.decision_margin), so NO ray qualifies: CAP = 0, the comparison is array_equal.  (The oracle's fp32 and fp64 binnings
    cannot pick the seed: they differ on 21 of this seed's 18000 rays, the fewest of seeds 0..11, all far from every boundary --
    upstream's floor_divide quotient is not an integer in fp32, -6.0000005 for one, and the conversion truncates it.  Kernel and
    oracle reproduce that in fp32; those rays are not excused.)"""
    from macarons_amd import ops
    SEED, CAP = 2, 0
    rng = np.random.default_rng(SEED)
    pts = rng.uniform(-.5, .5, (1, 2000, 3)).astype(F)
    Xv = rng.standard_normal((9, 3)).astype(F)
    Xv = (1.5 * Xv / np.linalg.norm(Xv, axis=1, keepdims=True)).astype(F)
    margin = G.decision_margin(pts, Xv, 7, 14)
    assert int((margin < 2e-6).sum()) <= CAP and V.bin_boundary_margin(pts, Xv, 7, 14).min() > 2e-6
    vs = ops.view_state(T(pts, dev), T(Xv, dev), 7, 14).cpu().numpy()
    ref = G.compute_view_state(pts[0], Xv, 7, 14)[None]
    bad = np.argwhere((vs != ref).any(-1))
    for b in bad:
        assert margin[tuple(b)].min() < 2e-6
    assert len(bad) <= CAP


# =====================================================================================================================================
# 5. transform, unprojection, gains, arg-max records
# =====================================================================================================================================
def dyadic_transform(rng, K):
    M = rng.choice(np.array([0, 1, -1, 0.5, -0.5, 2], F), (K, 16))
    return M, (rng.integers(-8, 9, (K, 3)) / 4).astype(F), rng.choice(np.array([0.5, 0.25, 2, 1, 0.125], F), K)


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("dim", [3, 4])
def test_transform_points(dev, n, dim):
    from macarons_amd import ops
    rng = np.random.default_rng(10 * n + dim)
    K = 3
    M, center, inv = dyadic_transform(rng, K)
    pts = (rng.integers(-64, 65, (K, n, dim)) / 16).astype(F)
    if dim == 4:
        pts[..., 3] = rng.standard_normal((K, n)).astype(F)       # column 3: any bits
    # single
    ref = G.transform_points(pts[0], M[0], center[0], inv[0])
    assert np.array_equal(ref.astype(np.float64), G.transform_points(pts[0], M[0], center[0], inv[0], dt=np.float64)), "not exact in fp32"
    got = ops.transform_points_(T(pts[0], dev), T(M[0], dev), T(center[0], dev), float(inv[0])).cpu().numpy()
    assert bits_equal(got, ref)
    # batched == per-cloud single calls == the model
    gb = ops.transform_points_batched_(T(pts, dev), T(M.reshape(K, 4, 4), dev), T(center, dev), T(inv, dev)).cpu().numpy()
    for c in range(K):
        single = ops.transform_points_(T(pts[c], dev), T(M[c], dev), T(center[c], dev), float(inv[c])).cpu().numpy()
        assert bits_equal(gb[c], single) and bits_equal(single, G.transform_points(pts[c], M[c], center[c], inv[c])), f"cloud {c}"
    # cloud_of: the clouds interleaved
    cloud = rng.integers(0, K, n).astype(np.int32)
    flat = pts[0].copy()
    refc = G.transform_points(flat, M, center, inv, cloud=cloud)
    assert np.array_equal(refc.astype(np.float64), G.transform_points(flat, M, center, inv, cloud=cloud, dt=np.float64))
    gc = ops.transform_points_batched_(T(flat, dev), T(M.reshape(K, 4, 4), dev), T(center, dev), T(inv, dev), cloud_of=T(cloud, dev))
    assert bits_equal(gc.cpu().numpy(), refc)
    if dim == 4:
        assert bits_equal(gc.cpu().numpy()[:, 3], flat[:, 3]) and bits_equal(gb[..., 3], pts[..., 3])


def unproject_bar(depth, cam):
    """(fp64 reference, bar): the same formula in fp64 on the fp32 inputs, and four times the error of the fp32 restatement against
    it (the factor allows for fp32 rounding that depends on contraction and on the divide)."""
    ref = G.unproject_depth(depth, cam, np.float64)
    e = float(np.abs(G.unproject_depth(depth, cam, F).astype(np.float64) - ref).max())
    return ref, e, 4 * e


UNPROJ_SHAPES = [(2, 3), (3, 2), (24, 40), (40, 24)]


@pytest.mark.parametrize("n_cam", [1, 3])
@pytest.mark.parametrize("H,W", UNPROJ_SHAPES, ids=[f"{h}x{w}" for h, w in UNPROJ_SHAPES])
def test_unproject_depth(dev, H, W, n_cam):
    from macarons_amd import ops
    rng = np.random.default_rng(H * 100 + W + n_cam)
    # dyadic: Minv over {0, +-1, +-0.5}, k22 = 1, k32 = -1, depths that are powers of two (sdepth = 1 - 1 / d is exact)
    cam = np.zeros((n_cam, 18), F)
    cam[:, :16] = rng.choice(np.array([0, 1, -1, 0.5, -0.5], F), (n_cam, 16))
    cam[:, 15] = 4.0                                               # w stays away from 0
    cam[:, 3], cam[:, 7], cam[:, 11] = 0.0, 0.0, 0.5
    cam[:, 16], cam[:, 17] = 1.0, -1.0
    depth = (2.0 ** rng.integers(0, 6, (n_cam, H, W))).astype(F)
    got = ops.unproject_depth(T(depth, dev), T(cam, dev)).cpu().numpy()
    for c in range(n_cam):
        ref = G.unproject_depth(depth[c], cam[c], F)
        if min(H, W) == 2:                                         # j / (m - 1) is exact: so is every intermediate before the divide
            h32, h64 = G.unproject_depth(depth[c], cam[c], F, True), G.unproject_depth(depth[c], cam[c], np.float64, True)
            assert np.array_equal(h32.astype(np.float64), h64), "not exact in fp32"
        # (m = 24: j / 23 is not dyadic; equality there rests on glue.hip's -ffp-contract=off)
        assert bits_equal(got[c], ref), f"camera {c}"
    # real-valued: within four times the fp32 restatement's own error of the fp64 value
    f = 1.0 / np.tan(np.deg2rad(60) / 2)
    K = np.array([[f, 0, 0, 0], [0, f, 0, 0], [0, 0, 100 / 99, 1], [0, 0, -100 / 99, 0]], np.float64)
    cams, depths = [], rng.uniform(2, 50, (n_cam, H, W)).astype(F)
    for c in range(n_cam):
        Mv = np.eye(4)
        Mv[:3, :3], Mv[3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.uniform(-2, 2, 3)
        cams.append(np.concatenate([np.linalg.inv(Mv @ K).reshape(-1), [K[2, 2], K[3, 2]]]).astype(F))
    cams = np.stack(cams)
    got = ops.unproject_depth(T(depths, dev), T(cams, dev)).cpu().numpy()
    for c in range(n_cam):
        ref, e, bar = unproject_bar(depths[c], cams[c])
        err = float(np.abs(got[c].astype(np.float64) - ref).max())
        print(f"ERR unproject {H}x{W} camera {c}: kernel {err:.3e}, fp32 restatement {e:.3e}, bar {bar:.3e} (|world| max {np.abs(ref).max():.1f})")
        assert err <= bar


def call_multi(dev, vis, n_cam, out=None):
    B, C, N = vis.shape
    out = Guarded((B, C ** n_cam), torch.float32, dev) if out is None else out
    v = T(vis, dev)
    return L_().mcr_coverage_gain_multiple(VP(v.data_ptr()), P_(out), I64(B), I64(C), I64(N), CI(n_cam), stream()), out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_cam", [2, 3])
def test_coverage_gain_multiple(dev, n_cam, B):
    """mcr_coverage_gain_multiple on an arbitrary vis table == fp64 max then mean in torch.cartesian_prod's tuple order: the fp64 value
    rounded once to fp32 when vis holds multiples of 2^-12 (the sum is exact), within 1 ulp otherwise."""
    rng = np.random.default_rng(n_cam * 10 + B)
    for C in (1, 2, 5):
        for N in (1, 255, 256, 257, 1025):
            vis = (rng.integers(0, 4097, (B, C, N)) / 4096.0).astype(F)
            rc, out = call_multi(dev, vis, n_cam)
            ok(rc, f"multi C {C} N {N}")
            out.check_guard("multi gains")
            ref = G.coverage_gain_multiple(vis, n_cam)
            assert G.is_dyadic(vis, 12) and bits_equal(out.np(), ref.astype(F)), f"C {C} N {N}"
            vis = rng.random((B, C, N)).astype(F)
            rc, out = call_multi(dev, vis, n_cam)
            ok(rc, f"multi C {C} N {N} real")
            ref = G.coverage_gain_multiple(vis, n_cam)
            r32 = ref.astype(F)
            assert (np.abs(out.np().astype(np.float64) - ref) <= np.spacing(np.abs(r32)).astype(np.float64)).all(), f"C {C} N {N}: over 1 ulp"


@pytest.mark.parametrize("n_cam", [2, 3])
def test_coverage_gain_multiple_tuple_order(dev, n_cam):
    """Which cameras a column stands for.  The gain of a tuple does not depend on the order of its cameras (max is symmetric), so a
    reversed enumeration cannot show in the gains; it shows in the index table ops.coverage_gain_multiple hands out beside them:
    that table is torch.cartesian_prod's (the last index fastest) and column j of the gains is the mean-max over ITS cameras."""
    from macarons_amd import ops
    rng = np.random.default_rng(n_cam)
    B, N, C = 2, 33, 4
    pts = rng.uniform(-.5, .5, (B, N, 4)).astype(F)
    harm = (rng.standard_normal((B, N, 64)) * .5).astype(F)
    cams = rng.standard_normal((B, C, 3)).astype(F)
    args = (T(pts, dev), T(harm, dev), T(cams, dev))
    gains, idx = ops.coverage_gain_multiple(*args, n_cam)
    t = G.tuple_table(C, n_cam)
    assert np.array_equal(idx.numpy(), t)
    assert np.array_equal(idx.numpy(), torch.cartesian_prod(*([torch.arange(C)] * n_cam)).numpy()) and idx[1].tolist() == [0] * (n_cam - 1) + [1]
    vis = ops.sh_visibilities(*args).cpu().numpy()
    ref = np.stack([vis.astype(np.float64)[:, t[:, k], :] for k in range(n_cam)], 0).max(0).mean(-1)
    assert (np.abs(gains.cpu().numpy().astype(np.float64) - ref) <= np.spacing(np.abs(ref.astype(F))).astype(np.float64)).all()
    rc, out = call_multi(dev, vis, n_cam)
    ok(rc, "multi on the network's vis")
    assert bits_equal(out.np(), gains.cpu().numpy())


def test_coverage_gain_multiple_refuses_four_cameras(dev):
    vis = np.random.default_rng(1).random((1, 3, 10)).astype(F)
    out = Guarded((1, 81), torch.float32, dev)
    rc, _ = call_multi(dev, vis, 4, out)
    refused(rc, "n_cam 4", "n_cam is too large", [out])


@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("dim", [3, 4])
@pytest.mark.parametrize("smooth", [False, True])
def test_macarons_gain(dev, N, dim, smooth):
    """ops.macarons_gain_ on dyadic inputs: distances from Pythagorean offsets (0, 3, 4 = distance_th, 5, 7, 9, 13, 15, 25), th = 4 so
    d / th and its square are exact.  The scaled vis is array_equal to the fp32 restatement.  The gains: the fp64 sum of at most 257
    fp32 values between 2^-20 and 1 is exact in any order, so the kernel's (float)(sum / N) * volume is the fp64 mean rounded once,
    times the volume, rounded once -- array_equal too."""
    from macarons_amd import ops
    rng = np.random.default_rng(N * 8 + dim * 2 + smooth)
    B = 4
    offs = np.array([[0, 0, 0], [0, 0, 4], [1, 2, 2], [3, 4, 0], [2, 3, 6], [1, 4, 8], [5, 12, 0], [9, 12, 0], [7, 24, 0], [0, -4, 0]], F)
    pick = offs[np.arange(B * N) % len(offs)].reshape(B, N, 3) * rng.choice(np.array([1, -1], F), (B, N, 3))
    cam = (rng.integers(-8, 9, (B, 3)) / 2).astype(F)
    pts = np.concatenate([pick + cam[:, None], rng.standard_normal((B, N, dim - 3)).astype(F)], -1).astype(F)
    vis = (rng.integers(1, 257, (B, N)) / 256.0).astype(F)
    vol = np.array([0.0, -1.5, 3.25, 100.0], F)
    v_ref, g64 = G.macarons_gain(vis, pts, cam, vol, 4.0, int(smooth))
    import math
    assert all(math.fsum(r.astype(np.float64)) / N == g for r, g in zip(v_ref, g64)), "the fp64 sum of the scaled vis is not exact"
    d = np.sqrt(((pts[..., :3] - cam[:, None]) ** 2).sum(-1))
    assert (N == 1) or ((d == 4).any() and (d == 0).any() and (d > 4).any())
    vd = T(vis, dev)
    g = ops.macarons_gain_(vd, T(pts, dev), T(cam, dev), T(vol, dev), 4.0, smooth).cpu().numpy()
    assert bits_equal(vd.cpu().numpy(), v_ref)
    assert bits_equal(g, (g64.astype(F) * vol).astype(F))
    if not smooth:
        assert bits_equal(v_ref[d <= 4], vis[d <= 4])              # d == distance_th and d == 0: factor 1


def test_macarons_gain_refusals(dev):
    from macarons_amd import ops
    B, N = 2, 10
    vis, gains = Guarded((B, N), torch.float32, dev, data=np.ones((B, N), F)), Guarded((B,), torch.float32, dev)
    pts, cam, vol = T(np.ones((B, N, 3), F), dev), T(np.zeros((B, 3), F), dev), T(np.ones(B, F), dev)
    call = lambda th, mode: L_().mcr_macarons_gain(P_(vis), VP(pts.data_ptr()), CI(3), VP(cam.data_ptr()), VP(vol.data_ptr()), CF(th), CI(mode),   # noqa: E731
                                                   I64(B), I64(N), P_(gains), stream())
    refused(call(0.0, 0), "distance_th 0", "distance_th must be positive", [vis, gains])
    refused(call(-1.0, 1), "distance_th < 0", "distance_th must be positive", [vis, gains])
    refused(call(1.0, 2), "factor_mode 2", "factor_mode", [vis, gains])


def argmax_rows(rng, B, C):
    """Rows: random, all -inf, all equal, a NaN in the last lane's column only, two NaNs, a tie, +inf, the max in the last column."""
    g = rng.random((B, C)).astype(F)
    last_lane = max([c for c in range(C) if c % 64 == 63], default=C - 1)
    g[1] = -np.inf
    g[2] = 0.5
    g[3, last_lane] = np.nan
    g[4, C // 3], g[4, C - 1] = np.nan, np.nan
    g[5, C // 2], g[5, C - 1] = 2.0, 2.0
    g[6, C - 1] = np.inf
    g[7, C - 1] = 3.0
    return g


@pytest.mark.parametrize("C", [1, 63, 64, 65, 129])
def test_argmax_records(dev, C):
    """best_record / best_merge / nbv_decide against torch.max on the CPU."""
    from macarons_amd import ops
    rng = np.random.default_rng(C)
    B = 65                                                       # the merge's second block of 64 clouds
    g = argmax_rows(rng, B, C)
    tm = torch.max(torch.from_numpy(g), dim=1)
    val, idx = G.torch_max_rows(g)
    assert G.PERTURB or (np.array_equal(idx, tm.indices.numpy()) and bits_equal(np.nan_to_num(val, nan=-7), np.nan_to_num(tm.values.numpy(), nan=-7)))
    same = lambda a, b: bits_equal(np.nan_to_num(np.asarray(a, F), nan=-7.0), np.nan_to_num(np.asarray(b, F), nan=-7.0))      # noqa: E731
    # one record per cloud, with an offset
    for off in (0, 1000, 2 ** 24 - C):
        rec = ops.best_record(T(g, dev), off).cpu().numpy()
        assert same(rec[:, 0], val) and np.array_equal(rec[:, 1].astype(np.int64), idx + off), f"offset {off}"
    out = Guarded((B, 2), torch.float32, dev)
    gd = T(g, dev)
    refused(L_().mcr_best_record(VP(gd.data_ptr()), I64(B), I64(C), I64(2 ** 24 - C + 1), P_(out), stream()), "idx_offset + C > 2^24",
            "below 2^24", [out])
    # shards merged, an empty shard's record (-inf, 3e38) among them: it never wins, not even against a row of -inf
    cuts = sorted(set([0, C // 3, C // 2, C]))
    recs = [ops.best_record(T(g[:, lo:hi].copy(), dev), lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    empty = T(np.tile(np.array([-np.inf, 3e38], F), (B, 1)), dev)
    for order in ([empty] + recs, recs + [empty], recs[:1] + [empty] + recs[1:]):
        vals, ids = ops.best_merge(torch.stack(order, 0).contiguous())
        assert same(vals.cpu().numpy(), val) and np.array_equal(ids.cpu().numpy(), idx)
    # the single-rank decision: empty clouds, the record as doubles, the range flag given and NULL
    nu = rng.integers(1, 2049, B).astype(np.int32)
    nu[[0, 4, 9]] = 0
    flag = T(np.array([3], np.int32), dev)
    for n_unique, rf in ((nu, flag), (None, None), (nu, None)):
        gd = T(g, dev)
        mx, ids, rec = ops.nbv_decide(gd, T(n_unique, dev) if n_unique is not None else None, rf)
        e = (n_unique < 1) if n_unique is not None else np.zeros(B, bool)
        want_idx, want_val = np.where(e, -1, idx), np.where(e, F(np.nan), val)
        want_g = np.where(e[:, None], F(np.nan), g)
        assert np.array_equal(ids.cpu().numpy(), want_idx) and same(mx.cpu().numpy(), want_val)
        assert same(gd.cpu().numpy(), want_g), "the gains of an empty cloud are NaN in place, the others untouched"
        rec = rec.cpu().numpy()
        assert rec.dtype == np.float64 and rec.shape == (1 + 2 * B,) and rec[0] == (3.0 if rf is not None else 0.0)
        assert np.array_equal(rec[1:1 + B], want_idx.astype(np.float64))
        assert bits_equal(np.nan_to_num(rec[1 + B:], nan=-7.0), np.nan_to_num(want_val.astype(np.float64), nan=-7.0))
