"""Operands and expected outputs of the padded-sequence block tests (tests/test_padded_blocks_gpu.py), numpy only: neither torch nor
the library, so everything here is pinned without a GPU (tests/test_padded_cases_cpu.py).

A. Attention with `lens` (mcr_attention_lens -> attention_mfma_kernel).  The selector cases of tests/_attention_cases.py with
   lens: every query puts all of its weight on one key below lens[s]; key row lens[s], the first excluded one, is the super-selector
   (raw score C / 2 above every target): ONE key leaking past the length flips every answer of the sequence, and the wrong row
   decodes to the key it came from.  attention_mfma_kernel cuts its key-split parts at kmid of the CLAMPED length n = min(L, max(1,
   lens[s])), so the lengths below are derived from kmid_of(n): part 0 = keys [0, kmid_of(n)), part 1 = [kmid_of(n), n).
       n = 1: kmid = 0, part 0 is EMPTY (n / 2 = 0 tiles); n = 64: kmid = 64, part 1 is empty; n = 65: part 1 holds one key;
       n = 191 | 192 | 193: part 1 = [128, n) ends one key short of, on, and one key past its first tile edge; n = 128 | 129: the same
       for part 1 = [64, n); n = 576 | 577: kmid = 320.
B. Pools and the column max.  Integer operands in which every asserted number is exact in ANY summation order:
       valid rows (r < n) of column c come in pairs (2 i, 2 i + 1) holding v +- amp(i), the sign order alternating with i + c; an
       unpaired last row holds v.  The sum of the n rows is n v and the mean is exactly v whatever the division rounds like.
       amp(i) is 1 .. 11 but for two pairs p1 < p2 that hold the column's largest amplitude A = 12 .. 15: the maximum v + A appears at
       exactly two rows (n >= 4), so the lowest-row rule of the backward kernels can be cross-checked against the forward.
       v = 64 + c + 300 s names (sequence, column).
       Padding rows r >= n hold 2^20 + r: a padded row entering a max names itself, one entering a sum moves the mean by more than
       2^10 (at least 2^20 / n, n <= 600; below 256 rows: more than 2^12).
   Every partial sum of valid rows is an integer below n (v + A) < 2^24 (asserted on the host for the shapes listed).
C. `ex` columns: ex[row, j] = 1 + 16 row + j over EX_W = 17 columns: a copied element names its source row and column (divmod(value -
   1, 16); column 16, which only the copy launch behind ex_cols = 17 moves, shares its value with column 0 of the next row).
D. LayerNorm into planes: Gaussian rows with a per-row offset and scale; the expected planes are NOT computed here: the claim under
   test is that the fused kernel equals the library's own two-step form bit for bit.
"""
import functools

import numpy as np

import _attention_cases as ac
from _attention_cases import HEADS, TK, cdiv, kmid_of

# ---- A: attention ----------------------------------------------------------------------------------------------------------------------
def n_keys(L, n):
    return int(min(L, max(1, n)))


def lens_route(heads, S, L, split_mode, lens, variant=0, aligned=True, workspace=True):
    """The instantiation attention() of nn_kernels.hip launches for mcr_attention_lens, from its conditions; None: refused."""
    H, qk, v = HEADS[heads]
    dq, dv = qk // H, v // H
    if lens is None and L == 16 and (dq, dv) == (8, 32):
        return "attention_small_kernel<16,4,8,32,4>"
    if not aligned:
        return None if lens is not None else f"attention_flash_kernel<{dq},{dv},4>"
    split = workspace and L >= 512 and 2 * S <= 65535 and (split_mode == 1 or (split_mode < 0 and cdiv(L, 64) * H * S <= 256))
    qg = 2 if cdiv(L, 128) * H * (2 * S if split else S) >= 512 else 1
    form = "PVH" if variant in (0, 6, 7) else "F32"
    return f"attention_mfma_kernel<{dq},{dv},{'SPLIT' if split else 'WHOLE'},{form},QG{qg}>" + ("+attention_combine_kernel" if split else "")


def key_parts(L, n, split):
    """The key ranges [(first, end)] of the blocks of one (query tile, head, sequence): one, or two when split."""
    n = n_keys(L, n)
    return [(0, kmid_of(n)), (kmid_of(n), n)] if split else [(0, n)]


def whole_lens(L):
    """0 (clamps to 1), 1, either side of a 16-key fragment and of the 64-key tile, L - 1, L, L + 5 (clamps to L)."""
    return tuple(dict.fromkeys([0, 1, 15, 16, 17, TK - 1, TK, TK + 1, L - 1, L, L + 5]))


WHOLE_L = (65, 129)
SHORT_L, SHORT_LENS = 16, (1, 8, 16)                                 # (32,128): lens forces the MFMA kernel where attention_small_kernel would run
QG2_S, QG1_S, QG_L = 64, 63, 129                                     # cdiv(129, 128) * 4 * 64 = 512
SPLIT_L = 577
# two calls of six sequences: split_mode 1 and -1 split (cdiv(577, 64) * 4 * 6 = 240 <= 256), 0 does not; QG = 1 (5 * 4 * 12 = 240 < 512)
SPLIT_LENS = ((0, 1, TK, TK + 1, 2 * TK, 2 * TK + 1), (3 * TK - 1, 3 * TK, 3 * TK + 1, SPLIT_L - 1, SPLIT_L, SPLIT_L + 5))
SPLIT2_S, SPLIT2_L = 16, 512                                         # grid2 = cdiv(512, 128) * 4 * 2 * 16 = 512: QG = 2
SPLIT2_LENS = (0, 1, TK, TK + 1, 2 * TK, 2 * TK + 1, 3 * TK - 1, 3 * TK, 3 * TK + 1, 4 * TK - 1, 4 * TK, 4 * TK + 1, 320, 511, 512, 517)


def qg_lens(S):
    base = whole_lens(QG_L)
    return tuple(base[s % len(base)] for s in range(S))


# One row per attention_mfma_kernel instantiation mcr_attention_lens reaches: (instantiation, heads, S, L, split_mode, lens given, variant)
# at the smallest shape of the tests that reaches it.  Every row has exact (selector) cases.
def _routes():
    rows = []
    for h in HEADS:
        dq, dv = HEADS[h][1] // 4, HEADS[h][2] // 4
        for variant, form in ((0, "PVH"), (1, "F32")):
            rows += [(f"attention_mfma_kernel<{dq},{dv},WHOLE,{form},QG1>", h, 1, SHORT_L if h == "32x128" else WHOLE_L[0], 0, True, variant),
                     (f"attention_mfma_kernel<{dq},{dv},WHOLE,{form},QG2>", h, QG2_S, QG_L, 0, True, variant),
                     (f"attention_mfma_kernel<{dq},{dv},SPLIT,{form},QG1>+attention_combine_kernel", h, 6, SPLIT_L, 1, True, variant),
                     (f"attention_mfma_kernel<{dq},{dv},SPLIT,{form},QG2>+attention_combine_kernel", h, SPLIT2_S, SPLIT2_L, 1, True, variant)]
    return tuple(rows)


ROUTES = _routes()


def padded_selectors():
    """Every selector argument tuple (ac.selector) the GPU file uses, so that the host file checks exactly those."""
    r = [("32x128", 1, SHORT_L, 0, (n,)) for n in SHORT_LENS]
    for h in HEADS:
        r += [(h, 1, L, rot, (n,)) for L in WHOLE_L for n in whole_lens(L) for rot in (0, 4)]
        r += [(h, QG2_S, QG_L, 0, qg_lens(QG2_S))]
        r += [(h, len(ls), SPLIT_L, rot, ls) for ls in SPLIT_LENS for rot in (0, 4)]
        r += [(h, SPLIT2_S, SPLIT2_L, 0, SPLIT2_LENS), (h, SPLIT2_S, SPLIT2_L, 0)]
    return tuple(dict.fromkeys(ac._norm(a) for a in r))


# ---- B: pools and the column max ----------------------------------------------------------------------------------------------------------
PAD_BASE = 2 ** 20
POOL_E = (1, 63, 64, 65, 250)
POOL_SL = ((3, 1), (2, 17), (3, 129), (3, 511), (3, 512), (2, 600))
POOL_RL, POOL_LONG_RL, POOL_LONG_MIN = 16, 64, 512                   # nn_kernels.hip: row lanes of pool_kernel / pool_long_kernel


def pool_kernel_of(L):
    return "pool_long_kernel" if L >= POOL_LONG_MIN else "pool_kernel"


def unroll_edges(L):
    """Lengths at which the 8-rows-in-flight loop of the kernel that serves L changes its trip count for some row lane: a row lane g
    takes an unrolled step while r + 7 RL < n, r = g + 8 RL k: the first lane starts at n = 7 RL + 1, the last completes at 8 RL."""
    rl = POOL_LONG_RL if L >= POOL_LONG_MIN else POOL_RL
    e = []
    k = 0
    while 8 * rl * k + 7 * rl + 1 <= L + 1:
        e += [8 * rl * k + 7 * rl + 1, 8 * rl * (k + 1)]
        k += 1
    return [x for x in e if x <= L + 1]


def pool_lens_sets(S, L):
    """Vectors of S lengths that together cover 0, 1, every unroll edge and its neighbours, L - 1, L and L + 5."""
    cand = {0, 1, L - 1, L, L + 5}
    for e in unroll_edges(L):
        cand |= {e - 1, e, e + 1}
    cand = sorted(c for c in cand if 0 <= c <= L + 5)
    n = cdiv(len(cand), S)
    return [tuple(cand[(i * S + k) % len(cand)] for k in range(S)) for i in range(n)]


class PoolCase:
    """x [S, L, E] float32 (frozen); per (sequence, column): n [S], mx, mean [S, E] float32, arg [S, E] = the lowest row holding the max."""

    def __init__(self, S, L, E, lens):
        self.S, self.L, self.E = S, L, E
        self.lens = None if lens is None else np.asarray(lens, np.int32)
        self.n = np.full(S, L) if lens is None else np.array([n_keys(L, n) for n in lens])
        c = np.arange(E)
        x = np.empty((S, L, E), np.float64)
        x[:] = (PAD_BASE + np.arange(L))[None, :, None]
        self.v = np.empty((S, E))
        self.twice = np.zeros(S, bool)
        for s in range(S):
            n, v = int(self.n[s]), 64 + c + 300 * s
            self.v[s] = v
            x[s, :n] = v
            npair = n // 2
            if npair:
                i = np.arange(npair)[:, None]
                amp = 1 + (3 * i + c[None]) % 11
                if npair >= 2:
                    p1 = (5 * c + s) % (npair - 1)
                    p2 = p1 + 1 + (c + 2 * s) % (npair - 1 - p1)
                    A = 12 + c % 4
                    amp[p1, c] = A
                    amp[p2, c] = A
                    self.twice[s] = True
                sign = np.where((i + c[None]) % 2 == 0, 1, -1)
                x[s, 0:2 * npair:2] += sign * amp
                x[s, 1:2 * npair:2] -= sign * amp
        assert np.array_equal(x, np.round(x))
        self.x = x.astype(np.float32)
        self.mx = np.stack([self.x[s, :int(self.n[s])].max(0) for s in range(S)])
        self.arg = np.stack([self.x[s, :int(self.n[s])].argmax(0) for s in range(S)])       # numpy: first occurrence = lowest row
        self.mean = self.v.astype(np.float32)
        for a in (self.x, self.mx, self.arg, self.mean):
            a.flags.writeable = False

    def largest_partial_sum(self):
        """All valid values are positive: no partial sum of a column, in any order, exceeds the sum of its valid rows."""
        return max(float(self.x[s, :int(self.n[s])].astype(np.float64).sum(0).max()) for s in range(self.S))

    def describe(self, s, c, y):
        """What a wrong max / mean says about its source."""
        if y >= PAD_BASE:
            return f"padding row {int(y) - PAD_BASE} (n = {int(self.n[s])})"
        return f"expected column value v = {int(self.v[s, c])}, n = {int(self.n[s])}, lowest max row {int(self.arg[s, c])}"


@functools.lru_cache(maxsize=None)
def pool_case(S, L, E, lens):
    return PoolCase(S, L, E, None if lens is None else list(lens))


# ---- C: ex columns ---------------------------------------------------------------------------------------------------------------------------
EX_W = 17
EX_COLS = (0, 1, 4, 16, 17)                                          # 0: ex = NULL; 17 > 16 leaves the fused copy for copy2d
EX_SL = ((3, 511), (3, 512))                                         # either side of POOL_LONG_MIN
EX_E = (1, 65)


def ex_rows(rows):
    x = (1 + 16 * np.arange(rows)[:, None] + np.arange(EX_W)[None, :]).astype(np.float32)
    x.flags.writeable = False
    return x


def ex_decode(y):
    """(row, column) an ex value came from, or None."""
    if not (np.isfinite(y) and y == np.floor(y) and y >= 1):
        return None
    return divmod(int(y) - 1, 16)


def colmax_route(L, ex_cols):
    """launch_colmax_broadcast: the kernels of one call."""
    if L >= POOL_LONG_MIN and ex_cols <= 16:
        return "pool_long_kernel<true>" + ("+ex" if ex_cols else "")
    return "pool_kernel<true>" + ("+copy2d_kernel" if ex_cols else "")


# ---- D: LayerNorm into planes ------------------------------------------------------------------------------------------------------------------
LN_E = (4, 60, 64, 68, 128, 252, 256, 512)                           # EPL = 2 (E <= 128), 4 (<= 256), 8; partial last lanes at 60, 68, 252
LN_M = (1, 3, 4, 5, 1000)                                            # four rows per block


def ln_epl(E):
    epl = cdiv(E, 64)
    return 2 if epl <= 2 else 4 if epl <= 4 else 8


@functools.lru_cache(maxsize=None)
def ln_case(M, E):
    """(x [M, E], gamma [E], beta [E]) float32, frozen."""
    rng = np.random.default_rng(1000 * E + M)
    x = (rng.standard_normal((M, E)) * rng.uniform(0.1, 30.0, (M, 1)) + rng.uniform(-50, 50, (M, 1))).astype(np.float32)
    g = rng.uniform(0.5, 2.0, E).astype(np.float32) * np.where(rng.random(E) < 0.3, -1, 1).astype(np.float32)
    b = rng.standard_normal(E).astype(np.float32)
    for a in (x, g, b):
        a.flags.writeable = False
    return x, g, b


LN_BIG = {"M": 5, "E": 256, "row": 3, "col": 77, "gamma": 8192.0}


def ln_overflow_case():
    """Row LN_BIG.row is one-hot at LN_BIG.col: its normalised value is sqrt(E - 1) = 15.97, times gamma = 8192: |y| = 1.3e5 > 65504, the
    largest fp16; every other |y| stays below 6 * 8192 < 65504 (asserted on the host with the fp64 reference)."""
    M, E, r, c = LN_BIG["M"], LN_BIG["E"], LN_BIG["row"], LN_BIG["col"]
    rng = np.random.default_rng(7)
    x = rng.standard_normal((M, E)).astype(np.float32)
    x[r] = 0
    x[r, c] = 1
    g = np.ones(E, np.float32)
    g[c] = LN_BIG["gamma"]
    b = np.zeros(E, np.float32)
    return x, g, b
