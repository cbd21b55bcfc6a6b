"""Cases, expected values and bounds of the attention edge tests (tests/test_attention_edges_gpu.py), numpy only: neither torch nor
the library, so everything here is checked without a GPU (tests/test_attention_cases_cpu.py).

A. Selector cases.  A q | k | v in which every (sequence, head, query) puts ALL of its weight on one chosen key pi[s, h, q]: the output
   row must be that key's value row bit for bit, and a wrong row decodes to the key (and column) it came from.
   A key index is three base-16 digits j = (a, b, d), each moved to [-8, 7] (j' = digit - 8).  With c = C = 512 and per-head width dq:

       k_j = [c a', -c a'^2/2,  c b', -c b'^2/2,  c d', -c d'^2/2,  1,               0]     (dq = 16: eight more zeros)
       q_t = [  ta',         1,   tb',         1,   td',         1,  -(c/2) |t'|^2,   1]     for the target key t

   raw score(t, j) = -(c/2) |j' - t'|^2: 0 on the target, -c/2 = -256 on a runner-up (one digit off by one), which is 92 in units of
   log 2 at dq = 16 and 130 at dq = 8.  Every entry is an integer; max |k| = 16384 and max |q| = 49152 = 3 * 2^14 are exact in ONE
   fp16 plane (k, q and v have an all-zero low plane), and every tile stays below 32768, the limit above which attention_mfma_kernel
   leaves its fp16-pair path for the fp32 one.  Two things differ from the plain form [c a, -c a^2/2, ...] | [ta, 1, ...]:
     * the digits are centred, so that |k| < 32768 (the plain form has |k| = 57600 wherever a digit is 15, i.e. in every 16 keys: the
       fp16-pair forms would never run);
     * dimension 6 removes the per-query constant (c/2) |t|^2 of the plain form, so the target's raw score is exactly 0.
       attention_planes_kernel takes exp2(fma(s, c2, -m)) with m = fl(s c2): with s = 0 that is exp2(0) = 1, with s = 1e5 it is
       exp2(of a rounding residue) and no output bit would be known.
   FORM "plain" keeps the uncentred form without dimension 6 (|k| up to 57600: the fp32 fallback tiles of the fp16-pair kernel) for the entries whose
   kernels subtract the maximum from the score itself.
   The SUPER-SELECTOR (lens cases) is the key row lens[s], the first excluded one: k = [0 x 6, 0, c/2]: raw score +c/2 for EVERY
   query, c/2 above its target: one key leaking past the length flips every answer of the sequence.
   Values: v[s, j, col] = 1 + (j + 7 col + 13 s) mod 2047, integers in [1, 2047] (never 0: next to an expected 0 the 2^-92 leftovers
   are visible), distinct along j (L <= 2047) and along the columns.

B. Conditioning cases: integer q, k, v (raw dot products exact in fp32) with scores far from 0, compared with fp64 at a DERIVED bound:
       delta = (dq + 1) 2^-24 scale max_{q,j} sum_i |q_i k_ji|        (score error, units of log 2; scale = log2(e) / sqrt(dq))
       bound = (expm1(2 ln2 delta) + L 2^-24) max |v|                 (every weight moves by e^(+-ln2 delta), before and after the
                                                                        normalisation; the sums add L roundings)
C. Backward: the selector operands with an integer d_out in [1, 7].  P is one-hot, delta = rowsum(dO * O) and dP[target] are the same
   integer sum below 2^24, so dS[target] = 1 * (x - x) = 0: dv[j] = sum of d_out[q] over {q: pi(q) = j} exactly, and everything else
   is below 4 B, B = L max|d_out . v| max|k| w_off with w_off the fp64 reference's largest off-target weight.
"""
import functools
import math

import numpy as np

U24 = 2.0 ** -24
C = 512                                   # the selector's gain: runner-up at -C/2 raw
HEADS = {"32x128": (4, 32, 128), "64x256": (4, 64, 256)}          # name -> (H, qk_dim, v_dim)
TK = 64                                   # keys per tile of attention_mfma_kernel / attention_planes_kernel
AB_TILE = 32                              # keys (queries) per wave and step of attention_bwd.hip
SPB = 4                                   # sequences per block of attention_small_kernel
A16_WAVES = 4                             # sequences per block of a16_bwd_kernel
LOG2E = 1.4426950408889634
V_MOD = 2047
MAP_KINDS = ("identity", "reversal", "first", "last", "kmid-1", "kmid", "random")


def cdiv(a, b):
    return -(-a // b)


def kmid_of(n_keys):
    """The tile-aligned cut of the key-split forms (nn_kernels.hip / attention_planes.hip: kmid)."""
    return min(n_keys, cdiv(n_keys // 2, TK) * TK)


def n_keys_of(L, lens):
    """[S] number of keys: min(L, max(1, lens[s])), or L."""
    return None if lens is None else np.clip(np.asarray(lens, np.int64), 1, L)


# ---- the routes of the launchers, recomputed from their conditions ---------------------------------------------------------------------
def forward_route(entry, heads, S, L, aligned=True, variant=0, masked=False):
    """The kernel instantiation attention() of nn_kernels.hip launches for a C entry.  entry: mcr_attention (no workspace: never
    split), mcr_attention_ws / mcr_attention_masked with a workspace (split mode -1).  variant 0: the default (6: fp16-pair P V)."""
    H, qk, v = HEADS[heads]
    dq, dv = qk // H, v // H
    if L == 16 and (dq, dv) == (8, 32):
        return "attention_small_kernel<16,4,8,32,4>" + (" +mask" if masked else "")
    if not aligned:
        return None if masked else f"attention_flash_kernel<{dq},{dv},4>"
    with_ws = entry in ("mcr_attention_ws", "mcr_attention_masked")
    split = with_ws and L >= 512 and cdiv(L, 64) * H * S <= 256
    qg = 2 if (not masked and cdiv(L, 128) * H * (2 * S if split else S) >= 512) else 1
    form = "MASK" if masked else ("PVH" if variant in (0, 6, 7) else "F32")
    return f"attention_mfma_kernel<{dq},{dv},{'SPLIT' if split else 'WHOLE'},{form},QG{qg}>" + ("+attention_combine_kernel" if split else "")


def planes_route(heads, S, L, split_mode):
    H, qk, v = HEADS[heads]
    split = L >= 512 and (split_mode == 1 or (split_mode < 0 and cdiv(L, 64) * H * S <= 256))
    qg = 2 if cdiv(L, 128) * H * (2 * S if split else S) >= 512 else 1
    return f"attention_planes_kernel<{qk // H},{v // H},{'SPLIT' if split else 'WHOLE'},QG{qg},NP2>" + ("+attention_combine_kernel" if split else "")


def ab_nsplit(S, L, H=4):
    blocks = S * H * cdiv(L, 64)
    return 1 if blocks >= 512 else 2 if blocks >= 256 else 4


def backward_route(heads, S, L):
    H, qk, v = HEADS[heads]
    dq, dv = qk // H, v // H
    if dq == 8 and L == 16:
        return "a16_bwd_kernel"
    ns = ab_nsplit(S, L, H)
    r = f"ab_fwd_kernel<{dq},{dv}> ab_dq_kernel<{dq},{dv}> ab_dkdv_kernel<{dq},{dv}> nsplit={ns}"
    return r + (f" ab_fwd_merge_kernel<{dv}> ab_sum_parts_kernel" if ns > 1 else "")


# One row per template instantiation a building-block C entry can reach: (instantiation, entry, heads, S, L, how).  Smallest shapes the
# launchers' conditions allow: QG = 2 needs cdiv(L, 128) * 4 * S >= 512 (S = 64 at L = 129; S = 63 stays at QG = 1), SPLIT needs a
# workspace, L >= 512 and cdiv(L, 64) * 4 * S <= 256 (S <= 7 at L = 576; S = 8 is unsplit); planes with split_mode = 1 split whatever S
# is, so their SPLIT QG = 2 form is cdiv(512, 128) * 4 * 2 S >= 512: S = 16.
# NOT reachable from the entries of THIS table: attention_mfma_kernel's SPLIT forms at QG = 2 (mode -1 asks for cdiv(L, 64) * 4 * S <=
# 256 and cdiv(L, 128) * 8 * S >= 512 at once: no L >= 512 has both) and its `lens` argument -- mcr_attention_lens reaches both
# (tests/_padded_cases.py has their rows) -- and attention_planes_kernel's NP = 1 forms (variant 7: test_variant7_gpu.py).
def _route_table():
    rows = [("attention_small_kernel<16,4,8,32,4>", "mcr_attention", "32x128", 5, 16, "any alignment"),
            ("attention_small_kernel<16,4,8,32,4> +mask", "mcr_attention_masked", "32x128", 5, 16, "any alignment")]
    for h in HEADS:
        dq, dv = HEADS[h][1] // 4, HEADS[h][2] // 4
        rows += [(f"attention_flash_kernel<{dq},{dv},4>", "mcr_attention", h, 1, 65, "ldq odd or qkv + 4 bytes"),
                 (f"attention_mfma_kernel<{dq},{dv},WHOLE,PVH,QG1>", "mcr_attention", h, 1, 65, "default variant"),
                 (f"attention_mfma_kernel<{dq},{dv},WHOLE,F32,QG1>", "mcr_attention", h, 1, 65, "mcr_call_variant(1)"),
                 (f"attention_mfma_kernel<{dq},{dv},WHOLE,PVH,QG2>", "mcr_attention", h, 64, 129, "default variant"),
                 (f"attention_mfma_kernel<{dq},{dv},WHOLE,F32,QG2>", "mcr_attention", h, 64, 129, "mcr_call_variant(1)"),
                 (f"attention_mfma_kernel<{dq},{dv},SPLIT,PVH,QG1>+attention_combine_kernel", "mcr_attention_ws", h, 1, 513, "default variant"),
                 (f"attention_mfma_kernel<{dq},{dv},SPLIT,F32,QG1>+attention_combine_kernel", "mcr_attention_ws", h, 1, 513, "mcr_call_variant(1)"),
                 (f"attention_mfma_kernel<{dq},{dv},WHOLE,MASK,QG1>", "mcr_attention_masked", h, 1, 65, "aligned"),
                 (f"attention_mfma_kernel<{dq},{dv},SPLIT,MASK,QG1>+attention_combine_kernel", "mcr_attention_masked", h, 1, 513, "with a workspace"),
                 (f"attention_planes_kernel<{dq},{dv},WHOLE,QG1,NP2>", "mcr_attention_planes", h, 1, 513, "split_mode 0"),
                 (f"attention_planes_kernel<{dq},{dv},WHOLE,QG2,NP2>", "mcr_attention_planes", h, 64, 129, "split_mode 0"),
                 (f"attention_planes_kernel<{dq},{dv},SPLIT,QG1,NP2>+attention_combine_kernel", "mcr_attention_planes", h, 1, 513, "split_mode 1"),
                 (f"attention_planes_kernel<{dq},{dv},SPLIT,QG2,NP2>+attention_combine_kernel", "mcr_attention_planes", h, 16, 512, "split_mode 1")]
    rows += [("a16_bwd_kernel", "mcr_attention_backward_pct", "32x128", 5, 16, "NULL workspace"),
             (backward_route("32x128", 1, 17), "mcr_attention_backward_pct", "32x128", 1, 17, "nsplit 4"),
             (backward_route("64x256", 1, 65), "mcr_attention_backward", "64x256", 1, 65, "nsplit 4"),
             (backward_route("64x256", 16, 256), "mcr_attention_backward", "64x256", 16, 256, "nsplit 2"),
             (backward_route("64x256", 32, 256), "mcr_attention_backward", "64x256", 32, 256, "nsplit 1")]
    return tuple(rows)


ROUTES = _route_table()


def route_of(row):
    """The route the launchers' conditions give for a row of ROUTES (must equal row[0])."""
    name, entry, heads, S, L, how = row
    if entry.startswith("mcr_attention_backward"):
        return backward_route(heads, S, L)
    if entry == "mcr_attention_planes":
        return planes_route(heads, S, L, int(how.split()[-1]))
    return forward_route(entry, heads, S, L, aligned="odd" not in how, variant=1 if "variant(1)" in how else 0, masked="masked" in entry)


# ---- A: selector cases -----------------------------------------------------------------------------------------------------------------
def _digits(j, centred):
    j = np.asarray(j, np.int64)
    d = np.stack([(j >> 8) & 15, (j >> 4) & 15, j & 15], -1)
    return d - 8 if centred else d


def target_map(kind, L, n, rng):
    """pi [L]: the target key of every query row, inside the first n keys."""
    q = np.arange(L) % n
    km = min(kmid_of(n), n - 1)
    if kind.startswith("shift:"):                          # (q + N) mod n
        return ((q + int(kind[6:])) % n).astype(np.int64)
    if kind.startswith("const:"):                          # every query -> key N (negative: from the end)
        return np.full(L, int(kind[6:]) % n, np.int64)
    if kind == "random":
        return rng.integers(0, n, L).astype(np.int64)
    if kind == "permutation":                              # every key gets one query (n == L)
        return rng.permutation(n)[q].astype(np.int64)
    return {"identity": q, "reversal": n - 1 - q, "first": np.zeros(L, np.int64), "last": np.full(L, n - 1),
            "kmid-1": np.full(L, max(km - 1, 0)), "kmid": np.full(L, km)}[kind].astype(np.int64)


def value_rows(S, L, v_dim):
    s, j, c = np.arange(S)[:, None, None], np.arange(L)[None, :, None], np.arange(v_dim)[None, None, :]
    return (1 + (j + 7 * c + 13 * s) % V_MOD).astype(np.float32)


def decode_key(y, s, col):
    """The key a value came from (value_rows inverted), or -1 when y is not one of its integers."""
    if not (np.isfinite(y) and y == np.floor(y) and 1 <= y <= V_MOD):
        return -1
    return int((int(y) - 1 - 7 * col - 13 * s) % V_MOD)


class Selector:
    """qkv [S, L, 2 qk + v] (float32, frozen), pi [S, H, L], lens ([S] int32 or None), expected [S, L, v], kinds [S][H]."""

    def __init__(self, heads, S, L, rot=0, lens=None, form="centred", kinds=None, seed=0):
        assert L <= V_MOD and form in ("centred", "plain")
        H, qk, v = HEADS[heads]
        dq = qk // H
        self.heads, self.S, self.L, self.H, self.qk, self.v, self.form = heads, S, L, H, qk, v, form
        self.lens = None if lens is None else np.asarray(lens, np.int32)
        nk = np.full(S, L) if lens is None else n_keys_of(L, lens)
        rng = np.random.default_rng(1000 * L + 10 * S + rot + seed)
        kinds = kinds or MAP_KINDS
        self.kinds = [[kinds[(rot + h + H * s) % len(kinds)] for h in range(H)] for s in range(S)]
        self.pi = np.stack([np.stack([target_map(self.kinds[s][h], L, int(nk[s]), rng) for h in range(H)]) for s in range(S)])
        centred = form == "centred"
        jd = _digits(np.arange(L), centred).astype(np.float64)                      # [L, 3]
        k = np.zeros((L, dq))
        k[:, 0:6:2], k[:, 1:6:2] = C * jd, -C * jd * jd / 2
        if centred:
            k[:, 6] = 1
        qkv = np.zeros((S, L, 2 * qk + v))
        for s in range(S):
            for h in range(H):
                td = _digits(self.pi[s, h], centred).astype(np.float64)
                q = np.zeros((L, dq))
                q[:, 0:6:2], q[:, 1:6:2] = td, 1
                if centred:
                    q[:, 6], q[:, 7] = -(C / 2) * (td * td).sum(-1), 1
                qkv[s, :, h * dq:(h + 1) * dq] = q
                qkv[s, :, qk + h * dq:qk + (h + 1) * dq] = k
                if lens is not None and nk[s] < L:                                  # the super-selector: the first excluded key
                    assert centred
                    qkv[s, nk[s], qk + h * dq:qk + (h + 1) * dq] = 0
                    qkv[s, nk[s], qk + h * dq + 7] = C / 2
        self.values = value_rows(S, L, v)
        qkv[..., 2 * qk:] = self.values
        assert np.array_equal(qkv, np.round(qkv))
        self.qkv = qkv.astype(np.float32)
        self.n_keys = nk
        dv = v // H
        exp = np.empty((S, L, v), np.float32)
        for s in range(S):
            for h in range(H):
                exp[s, :, h * dv:(h + 1) * dv] = self.values[s, self.pi[s, h], h * dv:(h + 1) * dv]
        self.expected = exp
        for a in (self.qkv, self.pi, self.expected, self.values):
            a.flags.writeable = False

    def asserted_rows(self, s):
        """Query rows whose output is asserted: all without lens, the first n_keys[s] with (rows beyond still get an output)."""
        return self.L if self.lens is None else int(self.n_keys[s])

    def mismatches(self, y, keys=None, limit=6):
        """[(sequence, head, query, column, expected key, decoded key)] where y [S', L, v] (the first S' sequences) differs in any bit
        from the value rows of keys [S, H, L] (default: the target map)."""
        dv = self.v // self.H
        keys = self.pi if keys is None else keys
        expected = self.expected if keys is self.pi else expected_rows(self, keys)
        out = []
        for s in range(y.shape[0]):
            n = self.asserted_rows(s)
            bad = np.argwhere(y[s, :n].view(np.int32) != expected[s, :n].view(np.int32))
            for qi, col in bad[:limit]:
                h = int(col) // dv
                out.append((s, h, int(qi), int(col), int(keys[s, h, qi]), decode_key(float(y[s, qi, col]), s, int(col))))
        return out

    @functools.cached_property
    def w_off(self):
        """The fp64 reference's largest off-target weight."""
        return max(off_target_weight(reference_weights(self.qkv[s:s + 1], self.H, self.qk, None, None if self.lens is None else self.lens[s:s + 1]),
                                     self.pi[s:s + 1])[1] for s in range(self.S))


def neighbours(t, L):
    """Keys one digit step away from key t inside [0, L): the runner-ups of target t (raw score -C/2)."""
    out = []
    for sh in (0, 4, 8):
        dg = (t >> sh) & 15
        for step in (-1, 1):
            j = t + step * (1 << sh)
            if 0 <= dg + step <= 15 and 0 <= j < L:
                out.append(j)
    return out


def selector_mask(sel, kind):
    """A mask that removes every target and all but one of its runner-ups; -> (bytes, (seq, head, query) strides, bool mask
    broadcastable to [S, H, L, L], survivor [S, H, L]).  kind "head": a mask per head; "pair": one [L, L] mask per sequence shared by
    the heads; "key": one [L] mask per sequence shared by heads and queries (every map of the case must be constant)."""
    S, H, L = sel.S, sel.H, sel.L
    shape = {"head": (S, H, L, L), "pair": (S, 1, L, L), "key": (S, 1, 1, L)}[kind]
    keep = np.ones(shape, bool)
    surv = np.empty((S, H, L), np.int64)
    for s in range(S):
        for qi in range(L):
            if kind == "key" and qi:
                assert (sel.pi[s, :, qi] == sel.pi[s, :, 0]).all(), "a key mask needs constant maps"
                surv[s, :, qi] = surv[s, :, 0]
                continue
            gone = [set([int(sel.pi[s, h, qi])] + neighbours(int(sel.pi[s, h, qi]), L)) for h in range(H)]
            for h in range(H):
                others = set().union(*[gone[g] for g in range(H) if g != h]) if kind != "head" else set()
                free = [j for j in neighbours(int(sel.pi[s, h, qi]), L) if j not in others]
                assert free, f"no runner-up of head {h} is free of the other heads' removed keys (s {s}, query {qi})"
                surv[s, h, qi] = free[(qi + h) % len(free)]
            for h in range(H):
                rem = sorted(gone[h] - ({int(surv[s, h, qi])} if kind == "head" else set(int(x) for x in surv[s, :, qi])))
                keep[s, h if kind == "head" else 0, qi if kind != "key" else 0, rem] = False
    strides = {"head": (H * L * L, L * L, L), "pair": (L * L, 0, L), "key": (L, 0, 0)}[kind]
    return keep.astype(np.uint8), strides, keep, surv


def expected_rows(sel, keys):
    """[S, L, v]: the value rows of keys [S, H, L]."""
    dv = sel.v // sel.H
    out = np.empty((sel.S, sel.L, sel.v), np.float32)
    for s in range(sel.S):
        for h in range(sel.H):
            out[s, :, h * dv:(h + 1) * dv] = sel.values[s, keys[s, h], h * dv:(h + 1) * dv]
    return out


# ---- the documented order in fp32 ----------------------------------------------------------------------------------------------------
def emulate_fp32(qkv, H, qk, v, mask=None, lens=None):
    """q * (log2(e) / sqrt(dq)) rounded, an fp32 dot product, exp2(s - max), the sum, the divide, then P V -- every step rounded to
    fp32 (numpy float32 arithmetic; the order inside the two sums is numpy's).  -> (out [S, L, v] float32, weights [S, H, L, L] float32)."""
    S, L, _ = qkv.shape
    dq, dv = qk // H, v // H
    f = np.float32
    scale = f(LOG2E) / np.sqrt(f(dq))
    x = qkv.astype(f)
    out = np.empty((S, L, v), f)
    ws = np.empty((S, H, L, L), f)
    nk = np.full(S, L) if lens is None else n_keys_of(L, lens)
    for s in range(S):
        for h in range(H):
            q = x[s, :, h * dq:(h + 1) * dq] * scale
            k = x[s, :, qk + h * dq:qk + (h + 1) * dq]
            sc = np.zeros((L, L), f)
            for d in range(dq):
                sc = sc + q[:, d:d + 1] * k[None, :, d]
            if mask is not None:
                m = np.broadcast_to(np.asarray(mask).astype(bool), (S, H, L, L))[s, h]
                sc = np.where(m, sc, f(-1e3) * scale)
            sc[:, int(nk[s]):] = -np.inf
            p = np.exp2(sc - sc.max(-1, keepdims=True)).astype(f)
            p = p / p.sum(-1, dtype=f)[:, None]
            ws[s, h] = p
            out[s, :, h * dv:(h + 1) * dv] = p @ x[s, :, 2 * qk + h * dv:2 * qk + (h + 1) * dv]
    return out, ws


def reference_weights(qkv, H, qk, mask=None, lens=None):
    """The fp64 soft-max weights [S, H, L, L] of _strided.attention_ref's rule (masked score -1e3 BEFORE the division)."""
    S, L, _ = qkv.shape
    dq = qk // H
    x = qkv.astype(np.float64)
    hs = lambda t: t.reshape(S, L, H, dq).transpose(0, 2, 1, 3)
    sc = hs(x[..., :qk]) @ hs(x[..., qk:2 * qk]).transpose(0, 1, 3, 2)
    if mask is not None:
        sc = np.where(np.broadcast_to(np.asarray(mask).astype(bool), sc.shape), sc, -1e3)
    sc = sc / np.sqrt(dq)
    if lens is not None:
        sc = np.where(np.arange(L).reshape(1, 1, 1, L) < n_keys_of(L, lens).reshape(S, 1, 1, 1), sc, -np.inf)
    e = np.exp(sc - sc.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def off_target_weight(w, keys):
    """(arg-max key [S, H, L], the largest total weight outside `keys` [S, H, L])."""
    off = w.copy()
    np.put_along_axis(off, keys[..., None], 0.0, -1)
    return w.argmax(-1), float(off.sum(-1).max())


# ---- the cases of section A (shapes recomputed from the launchers' constants) ---------------------------------------------------------
SMALL_S = (1, SPB, SPB + 1)                                                           # a ragged last block at S = SPB + 1
MFMA_L = (17, TK - 1, TK, TK + 1, 2 * TK - 1, 2 * TK, 2 * TK + 1)
QG_CASE = {"L": 2 * TK + 1, "S_qg2": 512 // (4 * cdiv(2 * TK + 1, 128)), "S_qg1": 512 // (4 * cdiv(2 * TK + 1, 128)) - 1}
SPLIT_SL = tuple((1, L) for L in (512, 513, 575, 576, 577, 640)) + ((7, 576),)
UNSPLIT_SL = (8, 576)                                                                 # cdiv(576, 64) * 4 * 8 = 288 > 256
MASK_L = (16, 65, 129, 513)
PLANES_L = (512, 513, 577, 700)
PLANES_SHORT_L = 65                                                                   # the entry accepts L < 512 (never split)


def planes_lens(L):
    """The lengths of the `lens` cases: 0 (clamped to 1), 1, the tile edge, kmid of L and its neighbours, L - 1, L, L + 5 (clamped)."""
    km = kmid_of(L)
    return [0, 1, TK - 1, TK, TK + 1, km - 1, km, km + 1, L - 1, L, L + 5]


# ---- B: conditioning -------------------------------------------------------------------------------------------------------------------
COND_KINDS = ("common+", "common-", "growing", "equal")
COND_CASES = tuple((kind, L) for kind in COND_KINDS[:3] for L in (TK + 1, 513)) + (("equal", TK),)     # the mean of 64 integers is exact


def conditioning_case(kind, heads, L, S=1):
    """-> (qkv [S, L, W] float32 of integers, bound).  common+-: every raw score is +-Q0 K0 (about 2e4 units of log 2) plus an integer
    0..16; growing: the raw score of query row r grows (r % 3 == 0), falls (1) or stays (2) by about 40 units of log 2 per 64-key tile;
    equal: q = 0, the output is the mean of v."""
    H, qk, v = HEADS[heads]
    dq = qk // H
    rng = np.random.default_rng(len(kind) * 100 + L + dq)
    scale = LOG2E / math.sqrt(dq)
    x = np.zeros((S, L, 2 * qk + v))
    x[..., 2 * qk:] = rng.integers(-8, 9, (S, L, v))
    for h in range(H):
        q, k = np.zeros((S, L, dq)), np.zeros((S, L, dq))
        k[..., 1] = rng.integers(0, 17, (S, L))
        k[..., 2:dq] = rng.integers(-2, 3, (S, L, dq - 2))
        q[..., 1] = 1
        q[..., 2:dq] = rng.integers(-1, 2, (S, L, dq - 2))
        if kind in ("common+", "common-"):
            g = int(round(math.sqrt(2e4 / scale)))
            q[..., 0], k[..., 0] = (g if kind == "common+" else -g), g + h
        elif kind == "growing":
            q[..., 0] = np.array([1, -1, 0])[np.arange(L) % 3]
            k[..., 0] = (np.arange(L) // TK) * int(round(40 / scale))
        else:
            q[:] = 0
        x[..., h * dq:(h + 1) * dq], x[..., qk + h * dq:qk + (h + 1) * dq] = q, k
    hq = x[..., :qk].reshape(S, L, H, dq)
    hk = x[..., qk:2 * qk].reshape(S, L, H, dq)
    mag = max(float((np.abs(hq[s, :, h])[:, None, :] * np.abs(hk[s, :, h])[None, :, :]).sum(-1).max()) for s in range(S) for h in range(H))
    delta = (dq + 1) * U24 * scale * mag
    bound = (math.expm1(2 * math.log(2) * delta) + L * U24) * float(np.abs(x[..., 2 * qk:]).max())
    out = x.astype(np.float32)
    out.flags.writeable = False
    return out, bound


# ---- C: backward -----------------------------------------------------------------------------------------------------------------------
BWD_L = (17, AB_TILE, AB_TILE + 1, 2 * AB_TILE, 2 * AB_TILE + 1)
BWD_NSPLIT_SL = ((16, 256), (15, 256), (32, 256), (31, 256))          # 256 blocks: nsplit 2 | 240: 4 | 512: 1 | 496: 2
BWD_LENS = lambda L: [1, AB_TILE - 1, AB_TILE, AB_TILE + 1, L]
A16_S = (1, A16_WAVES - 1, A16_WAVES, A16_WAVES + 1, 64)


def d_out_rows(S, L, v_dim, seed=5):
    g = np.random.default_rng(seed + L).integers(1, 8, (S, L, v_dim)).astype(np.float32)
    g.flags.writeable = False
    return g


def expected_dv(sel, g):
    """dv[s, j, head h's columns] = sum of g[s, q, the same columns] over {q: pi[s, h, q] = j} -- integer sums, exact in fp32."""
    dv = sel.v // sel.H
    out = np.zeros((sel.S, sel.L, sel.v))
    for s in range(sel.S):
        for h in range(sel.H):
            np.add.at(out[s, :, h * dv:(h + 1) * dv], sel.pi[s, h], g[s, :, h * dv:(h + 1) * dv].astype(np.float64))
    assert np.abs(out).max() < 2 ** 24
    return out.astype(np.float32)


def backward_bound(sel, g, w_off):
    """B = L max|d_out . v| max|k| w_off (per head dot products of a d_out row with a value row)."""
    dv = sel.v // sel.H
    gv = max(float((np.abs(g[s, :, h * dv:(h + 1) * dv].astype(np.float64)) @ np.abs(sel.values[s, :, h * dv:(h + 1) * dv].astype(np.float64)).T).max())
             for s in range(sel.S) for h in range(sel.H))
    kmax = float(np.abs(sel.qkv[..., sel.qk:2 * sel.qk]).max())
    return sel.L * gv * kmax * w_off


@functools.lru_cache(maxsize=None)
def selector(heads, S, L, rot=0, lens=None, form="centred", kinds=None, seed=0):
    """Selector(...) built once per argument tuple (lens / kinds as tuples) and shared by the tests."""
    return Selector(heads, S, L, rot, None if lens is None else list(lens), form, kinds, seed)


# ---- the registry: every selector the GPU tests use, so that the CPU file checks exactly those --------------------------------------------
PAIR_KINDS = ("shift:0", "shift:4", "shift:8", "shift:12")        # one [L, L] mask serves four heads: their targets stay apart
KEY_KINDS = ("const:0", "const:5", "const:-2", "const:-7")        # one [L] mask serves every query: constant maps
BWD_KINDS = ("permutation", "first")
LENS_L = 577                                                      # ten tiles, kmid = 320: neither a tile count of 2^n nor a length on an edge


def _both_rots(S):
    return (0, 4) if S == 1 else (0,)                            # 4 heads x S slots must cover the 7 map kinds


def forward_selectors():
    r = [("32x128", S, 16, rot) for S in SMALL_S for rot in _both_rots(S)]
    for h in HEADS:
        r += [(h, 1, L, rot) for L in MFMA_L for rot in (0, 4)]
        r += [(h, 1, 2 * TK + 1, 0, None, "plain"), (h, 1, 513, 0, None, "plain")]
        r += [(h, QG_CASE["S_qg2"], QG_CASE["L"], 0)]
        r += [(h, S, L, rot) for S, L in SPLIT_SL + (UNSPLIT_SL,) for rot in _both_rots(S)]
        r += [(h, 1, L, 0) for L in PLANES_L + (PLANES_SHORT_L,)] + [(h, 16, 512, 0)]
        r += [(h, len(planes_lens(LENS_L)), LENS_L, 0, tuple(planes_lens(LENS_L)))]
    return tuple(dict.fromkeys(_norm(a) for a in r))


def mask_selectors():
    return tuple(_norm((h, 1, L, 0, None, "centred", kinds)) for h in HEADS for L in MASK_L for kinds in (None, PAIR_KINDS, KEY_KINDS))


def backward_selectors():
    r = [("64x256", S, L, 0, None, "centred", BWD_KINDS) for L in BWD_L for S in (1, 2)]
    r += [("64x256", S, L, 0, None, "centred", BWD_KINDS) for S, L in BWD_NSPLIT_SL]
    r += [("64x256", 5, 65, 0, tuple(BWD_LENS(65)), "centred", BWD_KINDS)]
    r += [("32x128", S, 16, 0, None, "centred", BWD_KINDS) for S in A16_S]
    for L in (17, 65):
        r += [("32x128", 2, L, 0, None, "centred", BWD_KINDS), ("32x128", 5, L, 0, tuple(BWD_LENS(L)), "centred", BWD_KINDS)]
    return tuple(_norm(a) for a in r)


def _norm(a):
    a = tuple(a) + (0, None, "centred", None)[len(a) - 3:]
    return a[:7]


def sel_id(a):
    h, S, L, rot, lens, form, kinds = a
    return f"{h}-S{S}-L{L}-rot{rot}" + ("-lens" if lens else "") + ("" if form == "centred" else "-" + form) + \
        ("" if kinds is None else "-" + kinds[0].split(":")[0])
