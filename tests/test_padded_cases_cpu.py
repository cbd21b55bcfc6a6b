"""The cases of tests/test_padded_blocks_gpu.py, pinned on the host (tests/_padded_cases.py).  Attention: the route table against the
launcher's conditions, the kmid values and key ranges of attention_mfma_kernel (cut at kmid of the CLAMPED length), and per selector
case, from the fp64 reference alone: the arg-max key is the target, the off-target weight is below 2^-60, the first excluded key
would win every query if it leaked.  Pools: the expected max / mean / lowest max row from plain numpy, the exactness headroom (every
partial sum below 2^24), padding rows that name themselves.  ex columns decode to their source.  LayerNorm: the EPL instantiations and
the overflow row."""
import numpy as np
import pytest

import _attention_cases as ac
import _padded_cases as pc
import _strided as st
from test_attention_cases_cpu import W_OFF_MAX, _check_formats, _check_selector


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def test_kmid_is_taken_from_the_clamped_length():
    km = {n: ac.kmid_of(n) for n in (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 511, 512, 576, 577)}
    assert km == {1: 0, 63: 63, 64: 64, 65: 64, 127: 64, 128: 64, 129: 64, 191: 128, 192: 128, 193: 128, 255: 128, 256: 128, 257: 128,
                  320: 192, 511: 256, 512: 256, 576: 320, 577: 320}
    L = pc.SPLIT_L
    assert ac.kmid_of(L) == 320                                        # what a cut taken from L instead of the length would use
    parts = {n: pc.key_parts(L, n, True) for ls in pc.SPLIT_LENS for n in ls}
    assert parts == {0: [(0, 0), (0, 1)], 1: [(0, 0), (0, 1)],          # part 0 EMPTY: n / 2 = 0 tiles
                     64: [(0, 64), (64, 64)],                           # part 1 empty
                     65: [(0, 64), (64, 65)],                           # one key in part 1
                     128: [(0, 64), (64, 128)], 129: [(0, 64), (64, 129)],
                     191: [(0, 128), (128, 191)], 192: [(0, 128), (128, 192)], 193: [(0, 128), (128, 193)],     # around part 1's tile edge
                     576: [(0, 320), (320, 576)], 577: [(0, 320), (320, 577)], 582: [(0, 320), (320, 577)]}
    for n in (128, 129, 191, 192, 193):                                 # a cut from L = 577 would leave all of these keys in part 0
        assert pc.n_keys(L, n) <= ac.kmid_of(L)
    for n in pc.SPLIT2_LENS:
        (a, b), (c, d) = pc.key_parts(pc.SPLIT2_L, n, True)
        assert a == 0 and b == c == ac.kmid_of(pc.n_keys(pc.SPLIT2_L, n)) and d == pc.n_keys(pc.SPLIT2_L, n) and b % ac.TK in (0, d % ac.TK)
    assert pc.key_parts(65, 70, False) == [(0, 65)] and pc.key_parts(65, 0, False) == [(0, 1)]
    assert pc.whole_lens(65) == (0, 1, 15, 16, 17, 63, 64, 65, 70) and pc.whole_lens(129) == (0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 134)


def test_route_table_against_the_launcher_conditions():
    names = [r[0] for r in pc.ROUTES]
    assert len(set(names)) == len(names) == 16
    for name, heads, S, L, mode, with_lens, variant in pc.ROUTES:
        assert pc.lens_route(heads, S, L, mode, (1,) * S if with_lens else None, variant) == name, name
    want = {f"attention_mfma_kernel<{dq},{dv},{sp},{form},QG{g}>" for dq, dv in ((8, 32), (16, 64)) for form in ("PVH", "F32") for g in (1, 2)
            for sp in ("WHOLE", "SPLIT")}
    assert {n.split("+")[0] for n in names} == want
    for h in ac.HEADS:
        one = (1,)
        # lens forces the matrix-pipe kernel at L = 16; without it the (32,128) layout runs attention_small_kernel
        assert pc.lens_route(h, 1, 16, 0, one).startswith("attention_mfma_kernel")
        assert pc.lens_route(h, 1, 16, 0, None).startswith("attention_small_kernel" if h == "32x128" else "attention_mfma_kernel")
        assert pc.lens_route(h, 1, 65, 0, one, aligned=False) is None and pc.lens_route(h, 1, 65, 0, None, aligned=False).startswith("attention_flash")
        for L in pc.WHOLE_L:
            assert "WHOLE" in pc.lens_route(h, 1, L, 1, one) and "QG1" in pc.lens_route(h, 1, L, 1, one)          # below 512: never split
        assert "WHOLE" in pc.lens_route(h, pc.QG2_S, pc.QG_L, 0, one) and "QG2" in pc.lens_route(h, pc.QG2_S, pc.QG_L, 0, one)
        assert "QG1" in pc.lens_route(h, pc.QG1_S, pc.QG_L, 0, one)
        for ls in pc.SPLIT_LENS:
            S = len(ls)
            assert "SPLIT" in pc.lens_route(h, S, pc.SPLIT_L, 1, ls) and "QG1" in pc.lens_route(h, S, pc.SPLIT_L, 1, ls)
            assert "WHOLE" in pc.lens_route(h, S, pc.SPLIT_L, 0, ls) and "SPLIT" in pc.lens_route(h, S, pc.SPLIT_L, -1, ls)
            assert "WHOLE" in pc.lens_route(h, S, pc.SPLIT_L, 1, ls, workspace=False)
        assert "WHOLE" in pc.lens_route(h, 7, pc.SPLIT_L, -1, one)                                                 # 10 * 4 * 7 = 280 > 256
        r = pc.lens_route(h, pc.SPLIT2_S, pc.SPLIT2_L, 1, one)
        assert "SPLIT" in r and "QG2" in r and "QG1" in pc.lens_route(h, pc.SPLIT2_S - 1, pc.SPLIT2_L, 1, one)
        assert "SPLIT" in pc.lens_route(h, 1, pc.SPLIT2_L, 1, None) and "QG1" in pc.lens_route(h, 1, pc.SPLIT2_L, 1, None)
    assert ac.cdiv(pc.SPLIT2_L, 128) * 4 * 2 * pc.SPLIT2_S == 512


@pytest.mark.parametrize("args", pc.padded_selectors(), ids=ac.sel_id)
def test_padded_selector(args):
    """The arg-max of the fp64 reference is the target, the off-target weight stays below 2^-60, the fp32 emulation is exact, and
    the super-selector at row lens[s] would take every query if one more key were read."""
    sel = ac.selector(*args)
    _check_formats(sel)
    assert _check_selector(sel) < W_OFF_MAX
    if sel.lens is not None:
        for s in range(sel.S):
            n = int(sel.n_keys[s])
            assert n == pc.n_keys(sel.L, int(sel.lens[s])) and sel.pi[s].max() < n
            if n < sel.L:                                              # the super-selector row: k = [0 .. 0, C / 2] in every head
                k = sel.qkv[s, n, sel.qk:2 * sel.qk].reshape(sel.H, -1)
                assert (k[:, -1 if sel.qk // sel.H == 8 else 7] == ac.C / 2).all() and np.count_nonzero(k) == sel.H


def test_split_cases_put_weight_on_both_sides_of_the_cut():
    """Among the maps of the split cases there are targets in part 0 and in part 1 wherever both parts hold keys, and the maps
    "kmid-1" / "kmid" sit on the cut of the clamped length."""
    for h in ac.HEADS:
        for ls in pc.SPLIT_LENS:
            for rot in (0, 4):
                sel = ac.selector(h, len(ls), pc.SPLIT_L, rot, ls)
                for s, n in enumerate(sel.n_keys):
                    km = min(ac.kmid_of(int(n)), int(n) - 1)                # (the last key where part 1 is empty)
                    for hh, kind in enumerate(sel.kinds[s]):
                        if kind == "kmid":
                            assert (sel.pi[s, hh] == km).all()
                        if kind == "kmid-1":
                            assert (sel.pi[s, hh] == max(km - 1, 0)).all()
        kinds = {k for ls in pc.SPLIT_LENS for rot in (0, 4) for row in ac.selector(h, len(ls), pc.SPLIT_L, rot, ls).kinds for k in row}
        assert kinds == set(ac.MAP_KINDS)
        sel = ac.selector(h, pc.SPLIT2_S, pc.SPLIT2_L, 0, pc.SPLIT2_LENS)
        for s, n in enumerate(sel.n_keys):
            km = ac.kmid_of(int(n))
            if 0 < km < n:
                assert (sel.pi[s] < km).any() and (sel.pi[s] >= km).any(), (s, n)


# ---- pools and the column max ---------------------------------------------------------------------------------------------------------------
def test_pool_lens_sets_cover_the_edges():
    assert pc.unroll_edges(1) == [] and pc.unroll_edges(17) == [] and pc.unroll_edges(129) == [113, 128]
    assert pc.unroll_edges(511) == [113, 128, 241, 256, 369, 384, 497, 512] and pc.unroll_edges(512) == [449, 512] == pc.unroll_edges(600)
    assert [pc.pool_kernel_of(L) for _, L in pc.POOL_SL] == ["pool_kernel"] * 4 + ["pool_long_kernel"] * 2
    for S, L in pc.POOL_SL:
        sets = pc.pool_lens_sets(S, L)
        seen = {n for ls in sets for n in ls}
        assert all(len(ls) == S for ls in sets)
        assert {0, 1, L - 1, L, L + 5} <= seen
        for e in pc.unroll_edges(L):
            assert {x for x in (e - 1, e, e + 1) if x <= L + 5} <= seen, (S, L, e)
    assert pc.pool_lens_sets(3, 1) == [(0, 1, 6)] and pc.pool_lens_sets(2, 17) == [(0, 1), (16, 17), (22, 0)]


@pytest.mark.parametrize("S,L", pc.POOL_SL)
def test_pool_cases_are_exact_in_any_order(S, L):
    for E in pc.POOL_E:
        for lens in [None, (L,) * S] + pc.pool_lens_sets(S, L):
            case = pc.pool_case(S, L, E, lens)
            x = case.x.astype(np.float64)
            assert np.array_equal(x, np.round(x)) and x.min() > 0
            assert case.largest_partial_sum() < 2 ** 24
            for s in range(S):
                n = int(case.n[s])
                assert n == (L if lens is None else pc.n_keys(L, lens[s]))
                valid = x[s, :n]
                assert np.array_equal(valid.sum(0), n * case.v[s]) and np.array_equal(case.mean[s].astype(np.float64), case.v[s])
                assert np.array_equal((valid.sum(0) / n).astype(np.float32), case.mean[s])          # fp64 mean, rounded once
                assert np.array_equal(np.float32(valid.sum(0)) / np.float32(n), case.mean[s])      # the kernel's fp32 division
                assert valid.max() < 1024 and np.array_equal(case.mx[s].astype(np.float64), valid.max(0))
                hits = (valid == valid.max(0)).sum(0)
                assert (hits == (2 if n >= 4 else 1)).all(), (s, n, hits)
                assert np.array_equal(case.arg[s], (valid == valid.max(0)).argmax(0))
                if n >= 4:                                              # the two max rows lie in different pairs: the later one is not the answer
                    last = n - 1 - (valid[::-1] == valid.max(0)).argmax(0)
                    assert (last // 2 > case.arg[s] // 2).all()
                assert np.array_equal(x[s, n:], np.broadcast_to((pc.PAD_BASE + np.arange(n, L))[:, None], (L - n, E)))
                # a mean over L rows instead of n, or one padded row in the sum, is far from v
                if n < L:
                    assert abs(valid.sum(0) / L - case.v[s]).min() >= 0.5 * case.v[s].min() / L and pc.PAD_BASE / L > 2 ** 10
            assert len(np.unique(case.v)) == S * E                      # v names (sequence, column)
            assert case.describe(0, 0, float(pc.PAD_BASE + 5)).startswith("padding row 5")


def test_ex_columns_name_their_source():
    x = pc.ex_rows(3 * 512)
    assert x.shape == (1536, pc.EX_W) and x.max() < 2 ** 24
    for r, j in ((0, 0), (5, 3), (1535, 15), (700, 16)):
        assert pc.ex_decode(float(x[r, j])) == ((r, j) if j < 16 else (r + 1, 0))
    assert pc.ex_decode(float("nan")) is None and pc.ex_decode(0.5) is None
    assert len(np.unique(x[:, :16])) == 1536 * 16
    assert pc.colmax_route(512, 16) == "pool_long_kernel<true>+ex" and pc.colmax_route(512, 17) == "pool_kernel<true>+copy2d_kernel"
    assert pc.colmax_route(511, 4) == "pool_kernel<true>+copy2d_kernel" and pc.colmax_route(512, 0) == "pool_long_kernel<true>"
    assert pc.colmax_route(511, 0) == "pool_kernel<true>"
    assert [L >= pc.POOL_LONG_MIN for _, L in pc.EX_SL] == [False, True]


# ---- LayerNorm into planes ----------------------------------------------------------------------------------------------------------------
def test_layernorm_cases():
    assert {pc.ln_epl(E) for E in pc.LN_E} == {2, 4, 8} and [pc.ln_epl(E) for E in pc.LN_E] == [2, 2, 2, 2, 2, 4, 4, 8]
    assert any(E % 64 for E in pc.LN_E) and all(E % 4 == 0 for E in pc.LN_E)
    assert any(M % 4 for M in pc.LN_M) and 4 in pc.LN_M
    for E in pc.LN_E:
        x, g, b = pc.ln_case(5, E)
        y = st.layernorm_ref(x, g, b)
        assert np.abs(y).max() < 60000 and np.abs(g).min() >= 0.5
    x, g, b = pc.ln_overflow_case()
    y = st.layernorm_ref(x, g, b)
    r, c = pc.LN_BIG["row"], pc.LN_BIG["col"]
    assert abs(y[r, c]) > 65504 * 1.5
    y[r, c] = 0
    assert np.abs(y).max() < 65504 * 0.9
