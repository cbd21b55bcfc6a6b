"""The padded-sequence forward block by block, through the C ABI on guarded arenas: mcr_attention_lens (attention_mfma_kernel with
`lens`, whole and key-split, QG 1 and 2, fp16-pair and fp32 P V), mcr_pool_max_avg_lens and mcr_colmax_broadcast_lens (pool_kernel /
pool_long_kernel over the first lens[s] rows, the `ex` column copy) and mcr_layernorm_planes (layernorm_planes_kernel).

Operands and expected outputs come from tests/_padded_cases.py (pinned on the host by tests/test_padded_cases_cpu.py) and are compared
BIT FOR BIT:
  * attention: selector cases; key row lens[s] is the super-selector, so one key past the length flips every answer of the sequence
    and the failure names (sequence, head, query, column, expected key, decoded key);
  * pools / column max: integer columns whose max and mean are exact in any order; padding rows name themselves; the forward's max is
    fed back through the backward entries, which must put their 1 on the lowest row holding it;
  * ex columns decode to (source row, source column);
  * LayerNorm into planes equals mcr_split_to_planes(mcr_layernorm(x)) in both planes.
Every call checks the output guard, that its inputs (lens included) are unchanged, and the guard of a NaN-filled workspace.

Measured, not asserted (printed with the ERR prefix): the query rows at and beyond lens[s] of mcr_attention_lens, which the kernel
documents as "still get an output": they must be finite and inside the guard.  Measured on an MI355X: 178 ERR lines, 129021 padding
rows in all, "0 of N differ from their target's value row, largest distance 0.000e+00" on every one: on the selector operands the
rows beyond the length are their own target's value rows too.  The LayerNorm planes need no fallback tolerance: both planes are
bit-equal to the two-step form at every shape below (after the fix this file led to: the fused kernel's conversion had been folded into
its affine fma, one rounding instead of two, and hi was an fp16 ulp off fp16(y) in 3 of 60000 elements at M = 1000, E = 60; NOTES.md)."""
import ctypes

import numpy as np
import pytest
import torch

import _attention_cases as ac
import _padded_cases as pc
from _strided import Arena, HalfArena, Workspace
from test_abi_strided_gpu import ATT_LAYOUTS, POOL_LAYOUTS, refused
from test_attention_edges_gpu import exact, forward

pytestmark = pytest.mark.gpu

I64, CI, VP, SZ = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t


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


def dev_lens(dev, lens):
    return None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).to(dev)


def LP(lt):
    return VP(lt.data_ptr() if lt is not None else None)


def lens_unchanged(lt, lens, what):
    if lt is not None:
        assert np.array_equal(lt.cpu().numpy(), np.asarray(lens, np.int32)), what + ": lens changed"


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# =====================================================================================================================================
# mcr_attention_lens
# =====================================================================================================================================
def attn(dev, qkv, heads, lens=None, split_mode=0, variant=0, layout="packed", tag=""):
    """One call on arenas; -> y [S, L, v].  A workspace of exactly mcr_attention_workspace_bytes is passed whenever the mode can split."""
    H, qk, v = ac.HEADS[heads]
    S, L, W = qkv.shape
    dq, do, oq, oo = ATT_LAYOUTS[layout]
    what = f"mcr_attention_lens {heads} S={S} L={L} lens={None if lens is None else list(lens)} split_mode={split_mode} variant={variant} {layout} {tag}"
    Q = Arena(S * L, W, W + dq, oq, qkv.reshape(S * L, W).copy(), dev)
    O = Arena(S * L, v, v + do, oo, device=dev)
    ws = Workspace(int(L_().mcr_attention_workspace_bytes(I64(S), I64(L), CI(H), CI(v))), dev) if split_mode != 0 and L >= 512 else None
    lt = dev_lens(dev, lens)
    if variant:
        assert L_().mcr_call_variant(CI(variant)) == 0
    rc = L_().mcr_attention_lens(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(S), I64(L), CI(H), CI(qk), CI(v), LP(lt), CI(split_mode), P(ws),
                                 SZ(ws.n_bytes if ws else 0), stream())
    sync_ok(rc, what)
    O.check_guard(what + " out")
    Q.check_unchanged(what + " qkv")
    if ws is not None:
        ws.check_guard(what + " workspace")
    lens_unchanged(lt, lens, what)
    return O.packed().reshape(S, L, v)


def check_lens_output(sel, y, what):
    """The asserted rows bit for bit; the rows at and beyond lens[s] finite (an unwritten element keeps the NaN fill), their distance
    from their own target's value rows measured."""
    assert np.isfinite(y).all(), f"{what}: rows beyond a length hold something non-finite (an unwritten element keeps the fill)"
    exact(sel, y, what)
    if sel.lens is not None:
        rows = differ = 0
        dist = 0.0
        for s in range(y.shape[0]):
            n = int(sel.n_keys[s])
            rows += sel.L - n
            differ += int((y[s, n:].view(np.int32) != sel.expected[s, n:].view(np.int32)).any(-1).sum())
            dist = max(dist, float(np.abs(y[s, n:].astype(np.float64) - sel.expected[s, n:]).max(initial=0.0)))
        if rows:
            print(f"ERR {what} rows beyond lens: {differ} of {rows} differ from their target's value row, largest distance {dist:.3e}")


@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("L", pc.WHOLE_L)
def test_attention_lens_whole(dev, heads, L):
    """Unsplit, QG = 1, one sequence per call: lengths around a 16-key fragment, the 64-key tile and L; 0 clamps to 1, L + 5 to L.  With
    lens = L (and with lens = NULL) the bits are mcr_attention's."""
    for variant in (0, 1):
        assert "WHOLE" in pc.lens_route(heads, 1, L, 0, (1,), variant) and "QG1" in pc.lens_route(heads, 1, L, 0, (1,), variant)
        for rot in (0, 4):
            base = forward(dev, ac.selector(heads, 1, L, rot).qkv, heads, variant=variant)
            for i, n in enumerate(pc.whole_lens(L)):
                sel = ac.selector(heads, 1, L, rot, (n,))
                lay = "pad4" if (i + rot) % 3 == 0 else "packed"
                y = attn(dev, sel.qkv, heads, sel.lens, variant=variant, layout=lay)
                check_lens_output(sel, y, f"whole {heads} L={L} lens={n} (keys {pc.key_parts(L, n, False)}) rot={rot} variant={variant} maps={sel.kinds}")
                if n >= L:                                             # the same operand as the lens-free selector: no key row replaced
                    assert same_bits(y, base), f"lens = {n} >= L = {L} must give mcr_attention's bits ({heads}, variant {variant})"
            none = attn(dev, ac.selector(heads, 1, L, rot).qkv, heads, None, variant=variant)
            assert same_bits(none, base), f"lens = NULL must give mcr_attention's bits ({heads}, L={L}, variant {variant})"


def test_attention_lens_forces_the_mfma_kernel_at_16_tokens(dev):
    """(32,128), L = 16: attention_small_kernel has no lens, so attention() sends the call to attention_mfma_kernel: one partial tile."""
    for variant in (0, 1):
        for n in pc.SHORT_LENS:
            assert pc.lens_route("32x128", 1, pc.SHORT_L, 0, (n,), variant).startswith("attention_mfma_kernel<8,32,WHOLE")
            sel = ac.selector("32x128", 1, pc.SHORT_L, 0, (n,))
            y = attn(dev, sel.qkv, "32x128", sel.lens, variant=variant)
            check_lens_output(sel, y, f"L=16 lens={n} variant={variant} maps={sel.kinds}")
            if n == pc.SHORT_L:
                assert same_bits(y, forward(dev, ac.selector("32x128", 1, pc.SHORT_L, 0).qkv, "32x128", variant=variant))


@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_attention_lens_two_query_groups(dev, heads):
    """QG = 2 at (64, 129) with a different length per sequence against the first 63 sequences at QG = 1: bit-equal, padding rows included."""
    L, s2, s1 = pc.QG_L, pc.QG2_S, pc.QG1_S
    lens = pc.qg_lens(s2)
    sel = ac.selector(heads, s2, L, 0, lens)
    for variant in (0, 1):
        assert "QG2" in pc.lens_route(heads, s2, L, 0, lens, variant) and "QG1" in pc.lens_route(heads, s1, L, 0, lens[:s1], variant)
        y2 = attn(dev, sel.qkv, heads, sel.lens, variant=variant)
        y1 = attn(dev, sel.qkv[:s1], heads, sel.lens[:s1], variant=variant)
        check_lens_output(sel, y2, f"QG=2 {heads} S={s2} L={L} variant={variant}")
        check_lens_output(sel, y1, f"QG=1 {heads} S={s1} L={L} variant={variant}")
        bad = np.argwhere((y2[:s1].view(np.int32) != y1.view(np.int32)).any(-1))
        assert bad.size == 0, f"{heads} variant {variant}: QG = 2 and QG = 1 differ at (sequence, query) {bad[:6].tolist()}, lens {[lens[s] for s, _ in bad[:6]]}"


@pytest.mark.parametrize("split_mode", [1, 0, -1])
@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_attention_lens_key_split(dev, heads, split_mode):
    """L = 577, six sequences per call: the two blocks of a (query tile, head, sequence) take keys [0, kmid) and [kmid, n) with kmid from
    the CLAMPED length n: part 0 empty (n = 1), part 1 empty (64), one key in part 1 (65), either side of a tile edge of part 1 (128 |
    129, 191 | 192 | 193), n = L.  split_mode 1 and -1 split, 0 runs the same lengths whole."""
    L = pc.SPLIT_L
    for ls in pc.SPLIT_LENS:
        for variant in (0, 1):
            route = pc.lens_route(heads, len(ls), L, split_mode, ls, variant)
            assert ("SPLIT" in route) == (split_mode != 0) and "QG1" in route
            for rot in (0, 4):
                sel = ac.selector(heads, len(ls), L, rot, ls)
                y = attn(dev, sel.qkv, heads, sel.lens, split_mode=split_mode, variant=variant)
                parts = [pc.key_parts(L, n, split_mode != 0) for n in ls]
                check_lens_output(sel, y, f"{route} lens={list(ls)} key parts={parts} rot={rot} maps={sel.kinds}")


@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_attention_lens_key_split_two_query_groups(dev, heads):
    """(16, 512), split_mode 1: grid2 = 4 * 4 * 32 = 512 blocks: the SPLIT form at QG = 2, with a length per sequence and without lens;
    the lens-free call equals, sequence by sequence, the split of one sequence at QG = 1."""
    S, L = pc.SPLIT2_S, pc.SPLIT2_L
    free = ac.selector(heads, S, L, 0)
    sel = ac.selector(heads, S, L, 0, pc.SPLIT2_LENS)
    for variant in (0, 1):
        route = pc.lens_route(heads, S, L, 1, pc.SPLIT2_LENS, variant)
        assert "SPLIT" in route and "QG2" in route and "QG1" in pc.lens_route(heads, 1, L, 1, None, variant)
        y = attn(dev, sel.qkv, heads, sel.lens, split_mode=1, variant=variant)
        check_lens_output(sel, y, f"{route} lens={list(pc.SPLIT2_LENS)} key parts={[pc.key_parts(L, n, True) for n in pc.SPLIT2_LENS]}")
        y2 = attn(dev, free.qkv, heads, None, split_mode=1, variant=variant)
        exact(free, y2, f"{route} without lens")
        for s in range(S):
            y1 = attn(dev, free.qkv[s:s + 1], heads, None, split_mode=1, variant=variant)
            assert same_bits(y2[s], y1[0]), f"{heads} variant {variant}: sequence {s} of the QG = 2 split differs from its own QG = 1 split"


@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_attention_lens_refusals(dev, heads):
    """lens off the matrix-pipe kernel (qkv + 4 bytes, odd ldq) is the launcher's refusal; a workspace too small for the split that the
    mode asks for, a missing one, and a split_mode outside {1, 0, -1} are the entry's.  Nothing is written."""
    H, qk, v = ac.HEADS[heads]
    W = 2 * qk + v
    sel = ac.selector(heads, 1, 65, 0, (17,))
    lt = dev_lens(dev, sel.lens)
    for lay, (dq, oq) in {"q+4 bytes": (0, 1), "ldq odd": (1, 0)}.items():
        assert pc.lens_route(heads, 1, 65, 0, (17,), aligned=False) is None
        Q, O = Arena(65, W, W + dq, oq, sel.qkv[0].copy(), dev), Arena(65, v, device=dev)
        rc = L_().mcr_attention_lens(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(1), I64(65), CI(H), CI(qk), CI(v), LP(lt), CI(0), VP(None), SZ(0), stream())
        refused(rc, f"mcr_attention_lens lens with {lay}", "per-sequence lengths", [O])
        assert rc == 3
        # ... and the same operand without lens is served (attention_flash_kernel)
        rc = L_().mcr_attention_lens(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(1), I64(65), CI(H), CI(qk), CI(v), VP(None), CI(0), VP(None), SZ(0), stream())
        sync_ok(rc, f"mcr_attention_lens without lens, {lay}")
        assert np.isfinite(O.packed()).all()
        O.check_guard(lay)
    L = 513
    x = ac.selector(heads, 1, L, 0).qkv
    Q, O = Arena(L, W, data=x[0].copy(), device=dev), Arena(L, v, device=dev)
    need = int(L_().mcr_attention_workspace_bytes(I64(1), I64(L), CI(H), CI(v)))
    lt = dev_lens(dev, (300,))
    for mode, nbytes, null in ((1, need - 4, False), (-1, need - 4, False), (1, 0, True)):
        ws = Workspace(max(nbytes, 4), dev)
        rc = L_().mcr_attention_lens(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(1), I64(L), CI(H), CI(qk), CI(v), LP(lt), CI(mode),
                                     VP(None) if null else P(ws), SZ(nbytes), stream())
        refused(rc, f"mcr_attention_lens split_mode {mode} with {nbytes} of {need} workspace bytes", "workspace too small", [O, ws])
    for mode in (2, -2):
        rc = L_().mcr_attention_lens(P(Q), I64(Q.ld), P(O), I64(O.ld), I64(1), I64(L), CI(H), CI(qk), CI(v), LP(lt), CI(mode), VP(None), SZ(0), stream())
        refused(rc, f"mcr_attention_lens split_mode {mode}", "split_mode", [O])
    Q.check_unchanged("refusals")


# =====================================================================================================================================
# mcr_pool_max_avg_lens, mcr_colmax_broadcast_lens
# =====================================================================================================================================
def _lens_and_layouts(S, L):
    """(lens, layout) pairs: NULL and [L] * S packed, the first length vector on every layout, the others on one layout each."""
    sets = pc.pool_lens_sets(S, L)
    lays = list(POOL_LAYOUTS)
    out = [(None, "packed"), ((L,) * S, "packed")] + [(sets[0], lay) for lay in lays]
    return out + [(ls, lays[i % len(lays)]) for i, ls in enumerate(sets[1:], 1)]


def _name_columns(case, got, want, limit=6):
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    return [(int(s), int(c), float(got[s, c]), case.describe(int(s), int(c), float(got[s, c]))) for s, c in bad[:limit]]


def _lowest_row_holding(case, mx):
    """[S, E]: the lowest valid row of every column that holds the forward's max."""
    return np.stack([(case.x[s, :int(case.n[s])] == mx[s]).argmax(0) for s in range(case.S)])


def _one_hot(case, rows, value):
    out = np.zeros((case.S, case.L, case.E), np.float32)
    for s in range(case.S):
        out[s, rows[s], np.arange(case.E)] = value
    return out


def _name_rows(got, want, limit=6):
    bad = np.argwhere(got != want)
    return [(int(s), int(r), int(c), float(got[s, r, c]), float(want[s, r, c])) for s, r, c in bad[:limit]]


@pytest.mark.parametrize("E", pc.POOL_E)
@pytest.mark.parametrize("S,L", pc.POOL_SL)
def test_pool_max_avg_lens(dev, S, L, E):
    """Max over the first n rows and mean = sum / n, both exact; then the forward's max through mcr_pool_max_avg_backward_lens with
    d_max = 1, d_avg = 0: the 1 lands on the lowest row holding it, everything else is zero."""
    ones = np.concatenate([np.ones((S, E), np.float32), np.zeros((S, E), np.float32)], 1)
    for lens, lay in _lens_and_layouts(S, L):
        case = pc.pool_case(S, L, E, lens)
        dx, dy, ox, oy = POOL_LAYOUTS[lay]
        tag = f"{pc.pool_kernel_of(L)}<false> S={S} L={L} E={E} lens={lens} {lay}"
        X = Arena(S * L, E, E + dx, ox, case.x.reshape(S * L, E).copy(), dev)
        Z = Arena(S, 2 * E, 2 * E + dy, oy, device=dev)
        lt = dev_lens(dev, lens)
        sync_ok(L_().mcr_pool_max_avg_lens(P(X), I64(X.ld), P(Z), I64(Z.ld), I64(S), I64(L), CI(E), LP(lt), stream()), tag)
        Z.check_guard(tag)
        X.check_unchanged(tag)
        lens_unchanged(lt, lens, tag)
        z = Z.packed()
        mx, mean = np.ascontiguousarray(z[:, :E]), np.ascontiguousarray(z[:, E:])
        assert same_bits(mx, case.mx), f"max {tag}: (sequence, column, got, meaning) {_name_columns(case, mx, case.mx)}"
        assert same_bits(mean, case.mean), f"mean {tag}: (sequence, column, got, meaning) {_name_columns(case, mean, case.mean)}"
        if lens is None or tuple(lens) == (L,) * S:
            Z0 = Arena(S, 2 * E, device=dev)
            sync_ok(L_().mcr_pool_max_avg(P(X), I64(X.ld), P(Z0), I64(Z0.ld), I64(S), I64(L), CI(E), stream()), "mcr_pool_max_avg " + tag)
            assert same_bits(Z0.packed(), z), f"{tag}: differs from mcr_pool_max_avg"
        if lay == "packed" or lens is None:
            bl = dev_lens(dev, (L,) * S if lens is None else lens)
            G = Arena(S, 2 * E, data=ones, device=dev)
            D = Arena(S * L, E, device=dev)
            sync_ok(L_().mcr_pool_max_avg_backward_lens(P(X), I64(X.ld), P(G), I64(G.ld), P(D), I64(D.ld), I64(S), I64(L), CI(E), LP(bl), stream()),
                    "backward " + tag)
            D.check_guard("backward " + tag)
            got = D.packed().reshape(S, L, E)
            want = _one_hot(case, _lowest_row_holding(case, mx), 1.0)
            assert np.array_equal(got, want), f"backward {tag}: (sequence, row, column, got, expected) {_name_rows(got, want)}"
            assert np.array_equal(_lowest_row_holding(case, mx), case.arg)


@pytest.mark.parametrize("E", pc.POOL_E)
@pytest.mark.parametrize("S,L", pc.POOL_SL)
def test_colmax_broadcast_lens(dev, S, L, E):
    """Every one of the L rows of a sequence, padding rows included, holds the max of its first n rows; mcr_colmax_backward with ones
    puts the sum L on the lowest row holding the forward's max."""
    for lens, lay in _lens_and_layouts(S, L):
        case = pc.pool_case(S, L, E, lens)
        dx, dy, ox, oy = POOL_LAYOUTS[lay]
        tag = f"{pc.colmax_route(L, 0)} S={S} L={L} E={E} lens={lens} {lay}"
        X = Arena(S * L, E, E + dx, ox, case.x.reshape(S * L, E).copy(), dev)
        Y = Arena(S * L, E, E + dy, oy, device=dev)
        lt = dev_lens(dev, lens)
        rc = L_().mcr_colmax_broadcast_lens(P(X), I64(X.ld), P(Y), I64(Y.ld), I64(S), I64(L), CI(E), LP(lt), VP(None), I64(0), CI(0), VP(None), stream())
        sync_ok(rc, tag)
        Y.check_guard(tag)
        X.check_unchanged(tag)
        lens_unchanged(lt, lens, tag)
        y = Y.packed().reshape(S, L, E)
        want = np.ascontiguousarray(np.broadcast_to(case.mx[:, None], y.shape))
        if not same_bits(y, want):
            s, r, c = (int(t) for t in np.argwhere(y.view(np.int32) != want.view(np.int32))[0])
            raise AssertionError(f"{tag}: row {r} of sequence {s}, column {c} holds {y[s, r, c]}: {case.describe(s, c, float(y[s, r, c]))}")
        if lens is None or tuple(lens) == (L,) * S:
            Y0 = Arena(S * L, E, device=dev)
            sync_ok(L_().mcr_colmax_broadcast(P(X), I64(X.ld), P(Y0), I64(Y0.ld), I64(S), I64(L), CI(E), stream()), "mcr_colmax_broadcast " + tag)
            assert same_bits(Y0.packed(), y.reshape(S * L, E)), f"{tag}: differs from mcr_colmax_broadcast"
        if lay == "packed":
            G = Arena(S * L, E, data=np.ones((S * L, E), np.float32), device=dev)
            D = Arena(S * L, E, data=np.zeros((S * L, E), np.float32), device=dev)
            sync_ok(L_().mcr_colmax_backward(P(X), I64(X.ld), P(G), I64(G.ld), P(D), I64(D.ld), I64(S), I64(L), CI(E), LP(lt), stream()), "backward " + tag)
            D.check_guard("backward " + tag)
            got = D.packed().reshape(S, L, E)
            bwd = _one_hot(case, _lowest_row_holding(case, y[:, 0]), float(L))
            assert np.array_equal(got, bwd), f"backward {tag}: (sequence, row, column, got, expected) {_name_rows(got, bwd)}"


# (ex_ld - EX_W, offset of ex, ldy - max(E, EX_W + 3), offset of Y and ex_dst).  ldy >= ex_ld in every layout: a kernel that mixed the two
# leading dimensions up would still write inside ex_dst's arena (and ldy != ex_ld in every layout: it would be seen)
EX_LAYOUTS = {"packed": (0, 0, 0, 0), "odd+1": (1, 1, 1, 1), "pad4": (3, 0, 4, 0)}


def EXA_LD(dex):
    return pc.EX_W + dex


@pytest.mark.parametrize("ex_cols", pc.EX_COLS)
@pytest.mark.parametrize("S,L", pc.EX_SL)
def test_colmax_broadcast_ex_columns(dev, S, L, ex_cols):
    """The raw-column copy: inside pool_long_kernel from 512 rows with ex_cols <= 16, by copy2d_kernel otherwise.  Every ex_dst element
    decodes to its own row and column, for all L rows whatever lens says; ex_dst has Y's leading dimension; columns from ex_cols on
    keep the fill."""
    ex = pc.ex_rows(S * L)
    sets = [None] + pc.pool_lens_sets(S, L)[:2]
    for E in pc.EX_E:
        for lens in sets:
            case = pc.pool_case(S, L, E, lens)
            for lay, (dex, oex, dy, oy) in EX_LAYOUTS.items():
                tag = f"{pc.colmax_route(L, ex_cols)} S={S} L={L} E={E} ex_cols={ex_cols} lens={lens} {lay}"
                X = Arena(S * L, E, data=case.x.reshape(S * L, E).copy(), device=dev)
                ldy = max(E, pc.EX_W + 3) + dy
                assert ldy >= EXA_LD(dex) and ldy != EXA_LD(dex)
                Y = Arena(S * L, E, ldy, oy, device=dev)
                EXA = Arena(S * L, pc.EX_W, pc.EX_W + dex, oex, ex.copy(), dev)
                D = Arena(S * L, max(ex_cols, 1), ldy, oy, device=dev)
                lt = dev_lens(dev, lens)
                rc = L_().mcr_colmax_broadcast_lens(P(X), I64(X.ld), P(Y), I64(Y.ld), I64(S), I64(L), CI(E), LP(lt), P(EXA) if ex_cols else VP(None),
                                                    I64(EXA.ld if ex_cols else 0), CI(ex_cols), P(D) if ex_cols else VP(None), stream())
                sync_ok(rc, tag)
                for a in (Y, D):
                    a.check_guard(tag)
                for a in (X, EXA):
                    a.check_unchanged(tag)
                y = Y.packed().reshape(S, L, E)
                assert same_bits(y, np.ascontiguousarray(np.broadcast_to(case.mx[:, None], y.shape))), "max " + tag
                if not ex_cols:
                    D.check_unchanged(tag + ": ex_dst without ex")
                    continue
                d = D.packed()
                bad = np.argwhere(d.view(np.int32) != ex[:, :ex_cols].view(np.int32))
                assert bad.size == 0, f"{tag}: ex_dst (row, column) -> decoded source (row, column): " \
                                      f"{[((int(r), int(c)), pc.ex_decode(float(d[r, c]))) for r, c in bad[:6]]}"


def test_colmax_broadcast_lens_refusals(dev):
    S, L, E = 2, 17, 8
    X, Y = Arena(S * L, E, data=pc.pool_case(S, L, E, None).x.reshape(S * L, E).copy(), device=dev), Arena(S * L, 32, device=dev)
    EXA, D = Arena(S * L, pc.EX_W, data=pc.ex_rows(S * L).copy(), device=dev), Arena(S * L, 32, device=dev)

    def call(ldx, ldy, ex, ex_ld, ex_cols, dst):
        return L_().mcr_colmax_broadcast_lens(P(X), I64(ldx), P(Y), I64(ldy), I64(S), I64(L), CI(E), VP(None), ex, I64(ex_ld), CI(ex_cols), dst, stream())
    for args, needle in (((E - 1, 32, VP(None), 0, 0, VP(None)), "leading dimension too small"), ((E, E - 1, VP(None), 0, 0, VP(None)), "leading dimension too small"),
                         ((E, 32, P(EXA), 17, 4, VP(None)), "ex without ex_dst"), ((E, 32, P(EXA), 3, 4, P(D)), "ex_cols"),
                         ((E, 16, P(EXA), 17, 17, P(D)), "ex_cols"), ((E, 32, P(EXA), 17, 0, P(D)), "ex_cols"), ((E, 32, P(EXA), 17, -1, P(D)), "ex_cols"),
                         ((E, 32, VP(None), 0, 4, VP(None)), "without ex"), ((E, 32, VP(None), 0, 0, P(D)), "without ex")):
        refused(call(*args), f"mcr_colmax_broadcast_lens {args[:2]} ex_ld {args[3]} ex_cols {args[4]}", needle, [Y, D])
    Z = Arena(S, 2 * E, device=dev)
    for ldx, ldy in ((E - 1, 2 * E), (E, 2 * E - 1)):
        refused(L_().mcr_pool_max_avg_lens(P(X), I64(ldx), P(Z), I64(ldy), I64(S), I64(L), CI(E), VP(None), stream()), "mcr_pool_max_avg_lens",
                "leading dimension too small", [Z])


# =====================================================================================================================================
# mcr_layernorm_planes
# =====================================================================================================================================
# (ldx - E, ldp - E): multiples of 4, as mcr_split_to_planes asks
LNP_LAYOUTS = {"packed": (0, 0), "pad": (4, 8)}


def _ln_two_step(dev, x, g, b, tag):
    """mcr_split_to_planes(mcr_layernorm(x)) -> (hi bits, lo bits) uint16 [M, E]."""
    M, E = x.shape
    X, Y = Arena(M, E, data=x.copy(), device=dev), Arena(M, E, device=dev)
    G, B = Arena(1, E, data=g[None].copy(), device=dev), Arena(1, E, data=b[None].copy(), device=dev)
    sync_ok(L_().mcr_layernorm(P(X), I64(X.ld), P(G), P(B), P(Y), I64(Y.ld), I64(M), CI(E), stream()), "mcr_layernorm " + tag)
    Ph, Pl = HalfArena(M, E, device=dev), HalfArena(M, E, device=dev)
    sync_ok(L_().mcr_split_to_planes(P(Y), I64(Y.ld), P(Ph), P(Pl), I64(Ph.ld), I64(M), CI(E), stream()), "mcr_split_to_planes " + tag)
    return Ph.packed_bits(), Pl.packed_bits(), Y.packed()


def _ln_planes(dev, x, g, b, lay, with_lo, tag):
    M, E = x.shape
    dx, dp = LNP_LAYOUTS[lay]
    X = Arena(M, E, E + dx, 0, x.copy(), dev)
    G, B = Arena(1, E, data=g[None].copy(), device=dev), Arena(1, E, data=b[None].copy(), device=dev)
    Yh, Yl = HalfArena(M, E, E + dp, device=dev), HalfArena(M, E, E + dp, device=dev)
    rc = L_().mcr_layernorm_planes(P(X), I64(X.ld), P(G), P(B), P(Yh), P(Yl) if with_lo else VP(None), I64(Yh.ld), I64(M), CI(E), stream())
    sync_ok(rc, tag)
    Yh.check_guard(tag + " hi")
    for a in (X, G, B):
        a.check_unchanged(tag)
    if with_lo:
        Yl.check_guard(tag + " lo")
    else:
        Yl.check_unchanged(tag + ": the low plane's arena of a single-plane call")
    return Yh.packed_bits(), Yl.packed_bits()


def _name_halves(got, want, y, limit=6):
    bad = np.argwhere(got != want)
    return [(int(r), int(c), hex(int(got[r, c])), hex(int(want[r, c])), float(y[r, c])) for r, c in bad[:limit]]


@pytest.mark.parametrize("E", pc.LN_E)
def test_layernorm_planes_equals_split_of_layernorm(dev, E):
    """Both planes bit for bit, at every EPL instantiation (2, 4, 8 elements per lane), partial last lanes and ragged last blocks; the
    single-plane form writes the same high plane and leaves the low plane's memory alone."""
    for M in pc.LN_M:
        x, g, b = pc.ln_case(M, E)
        tag = f"layernorm_planes_kernel<{pc.ln_epl(E)}> M={M} E={E}"
        hi, lo, y = _ln_two_step(dev, x, g, b, tag)
        for lay in LNP_LAYOUTS:
            h2, l2 = _ln_planes(dev, x, g, b, lay, True, f"{tag} {lay}")
            assert np.array_equal(h2, hi), f"{tag} {lay} hi: (row, column, got, expected, fp32 y) {_name_halves(h2, hi, y)}"
            assert np.array_equal(l2, lo), f"{tag} {lay} lo: (row, column, got, expected, fp32 y) {_name_halves(l2, lo, y)}"
            h1, _ = _ln_planes(dev, x, g, b, lay, False, f"{tag} {lay} Yl=NULL")
            assert np.array_equal(h1, hi), f"{tag} {lay} Yl=NULL hi: {_name_halves(h1, hi, y)}"
        assert np.isfinite(hi.view(np.float16)).all() and (lo != 0).any()


def test_layernorm_planes_overflow_row_is_non_finite(dev):
    """|y| > 65504 in one element: its hi is non-finite, which is what the range guard looks for; the planes still equal the two-step form."""
    x, g, b = pc.ln_overflow_case()
    r, c = pc.LN_BIG["row"], pc.LN_BIG["col"]
    hi, lo, y = _ln_two_step(dev, x, g, b, "overflow")
    assert abs(y[r, c]) > 65504
    for with_lo in (True, False):
        h2, l2 = _ln_planes(dev, x, g, b, "packed", with_lo, f"overflow with_lo={with_lo}")
        assert not np.isfinite(h2.view(np.float16)[r, c]), f"hi of y = {y[r, c]} is {h2.view(np.float16)[r, c]}"
        mask = np.ones(h2.shape, bool)
        mask[r, c] = False
        assert np.isfinite(h2.view(np.float16)[mask]).all()
        assert np.array_equal(h2, hi) and (not with_lo or np.array_equal(l2, lo))


def test_layernorm_planes_refusals(dev):
    M, E = 3, 64
    x, g, b = pc.ln_case(M, E)
    X = Arena(M, E, E + 4, 0, x.copy(), dev)
    X1 = Arena(M, E, E + 4, 1, x.copy(), dev)
    G, B = Arena(1, E, data=g[None].copy(), device=dev), Arena(1, E, data=b[None].copy(), device=dev)
    Yh, Yl = HalfArena(M, E, E + 4, device=dev), HalfArena(M, E, E + 4, device=dev)
    Yo = HalfArena(M, E, E + 4, 1, device=dev)

    def call(xa, ldx, yh, yl, ldp, e=E):
        return L_().mcr_layernorm_planes(P(xa), I64(ldx), P(G), P(B), P(yh), P(yl), I64(ldp), I64(M), CI(e), stream())
    for args, needle in (((X, E - 4, Yh, Yl, E + 4), "leading dimension too small"), ((X, E + 4, Yh, Yl, E - 4), "leading dimension too small"),
                         ((X, E + 1, Yh, Yl, E + 4), "ldx must be a multiple of 4"), ((X1, E + 4, Yh, Yl, E + 4), "X 16-byte aligned"),
                         ((X, E + 4, Yh, Yl, E + 2), "ldp must be a multiple of 4"), ((X, E + 4, Yo, Yl, E + 4), "8-byte aligned"),
                         ((X, E + 4, Yh, Yo, E + 4), "8-byte aligned"), ((X, E + 4, Yh, Yl, E + 4, 62), "multiple of 4")):
        refused(call(*args), f"mcr_layernorm_planes {needle}", needle, [Yh, Yl, Yo])
