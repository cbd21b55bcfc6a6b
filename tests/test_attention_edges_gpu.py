"""The attention kernels key by key (nn_kernels.hip, attention_planes.hip, attention_bwd.hip), through the C ABI on guarded arenas.

A. Selector cases (tests/_attention_cases.py, pinned on the host by tests/test_attention_cases_cpu.py): every (sequence, head, query)
   puts all of its weight on one key, so the output row is that key's value row BIT FOR BIT on every kernel form a building-block
   entry reaches (ROUTES): a mis-addressed, dropped or double-counted key, a head or column mix-up, a lost rescale or a wrong merge
   of two key parts changes bits, and the failure message names (sequence, head, query, column, expected key, decoded key).
B. Conditioning: integer operands with scores far from 0 against the fp64 reference at the bound derived in the cases module; the
   ratio error / bound is printed per call (prefix COND).
C. Backward: the selector operands with integer d_out: dv exact where it is non-zero, everything else below 4 B.
Every call checks the output guard, that its inputs are unchanged, and the guard of a NaN-filled workspace."""
import ctypes

import numpy as np
import pytest
import torch

import _attention_cases as ac
import _strided as st
from _strided import Arena, Workspace
from test_abi_strided_gpu import ATT_LAYOUTS

pytestmark = pytest.mark.gpu

I64, CI, VP, SZ = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
FLASH_LAYOUTS = ("q_odd", "q+1")                          # off the 16-byte grid: attention_flash_kernel (attention_small_kernel: any)


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


def forward(dev, qkv, heads, entry="mcr_attention", layout="packed", variant=0, mask=None, lens=None, split_mode=0, tag=""):
    """One forward call on arenas; -> y [S, L, v].  mask: (bytes, strides).  Guards and inputs are checked here."""
    H, qk, v = ac.HEADS[heads]
    S, L, W = qkv.shape
    dq, do, oq, oo = ATT_LAYOUTS[layout]
    what = f"{entry} {heads} S={S} L={L} {layout} variant={variant} {tag}"
    Q = Arena(S * L, W, W + dq, oq, qkv.reshape(S * L, W).copy(), dev)        # (the cases are read-only arrays)
    O = Arena(S * L, v, v + do, oo, device=dev)
    ws = None
    if entry == "mcr_attention_planes":
        ws = Workspace(int(L_().mcr_attention_planes_workspace_bytes(I64(S), I64(L), CI(H), CI(qk), CI(v))), dev)
    elif entry == "mcr_attention_ws" or (entry == "mcr_attention_masked" and L >= 512):
        ws = Workspace(int(L_().mcr_attention_workspace_bytes(I64(S), I64(L), CI(H), CI(v))), dev)
    lt = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).to(dev)
    if variant:
        assert L_().mcr_call_variant(CI(variant)) == 0
    head = (P(Q), I64(Q.ld), P(O), I64(O.ld), I64(S), I64(L), CI(H), CI(qk), CI(v))
    if entry == "mcr_attention":
        rc = L_().mcr_attention(*head, stream())
    elif entry == "mcr_attention_ws":
        rc = L_().mcr_attention_ws(*head, P(ws), SZ(ws.n_bytes), stream())
    elif entry == "mcr_attention_masked":
        mt = torch.from_numpy(mask[0].reshape(-1).copy()).to(dev)
        rc = L_().mcr_attention_masked(*head, VP(mt.data_ptr()), I64(mask[1][0]), I64(mask[1][1]), I64(mask[1][2]), P(ws),
                                       SZ(ws.n_bytes if ws else 0), stream())
    else:
        rc = L_().mcr_attention_planes(*head, VP(lt.data_ptr() if lt is not None else None), CI(split_mode), P(ws), SZ(ws.n_bytes), stream())
    sync_ok(rc, what)
    O.check_guard(what + " out")
    Q.check_unchanged(what + " qkv")
    if ws is not None:
        ws.check_guard(what + " workspace")
    if entry == "mcr_attention_masked":
        assert np.array_equal(mt.cpu().numpy(), mask[0].reshape(-1)), what + ": the mask changed"
    if lt is not None:
        assert np.array_equal(lt.cpu().numpy(), np.asarray(lens, np.int32)), what + ": lens changed"
    return O.packed().reshape(S, L, v)


def exact(sel, y, what, keys=None):
    bad = sel.mismatches(y, keys)
    assert not bad, f"{what}: (sequence, head, query, column, expected key, decoded key; -1 = no key's value): {bad}"


# =====================================================================================================================================
# A. forward, bit for bit
# =====================================================================================================================================
@pytest.mark.parametrize("S", ac.SMALL_S)
def test_small_kernel(dev, S):
    """attention_small_kernel: SPB = 4 sequences per block, S = 5 leaves a ragged last block; any alignment."""
    for rot in ac._both_rots(S):
        sel = ac.selector("32x128", S, 16, rot)
        assert ac.forward_route("mcr_attention", "32x128", S, 16).startswith("attention_small_kernel")
        for lay in ("packed",) + FLASH_LAYOUTS + ("o_odd+1",):
            exact(sel, forward(dev, sel.qkv, "32x128", layout=lay), f"small S={S} rot={rot} {lay}")


@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("L", ac.MFMA_L)
def test_mfma_whole_and_flash(dev, heads, L):
    """attention_mfma_kernel at QG = 1, unsplit, around its 64-key tile: fp16-pair P V (default variant) and fp32 P V (variant 1); the
    same cases through a misaligned qkv: attention_flash_kernel (128-key tiles, four waves' partial soft-maxes merged)."""
    for rot in (0, 4):
        sel = ac.selector(heads, 1, L, rot)
        for variant in (0, 1):
            exact(sel, forward(dev, sel.qkv, heads, variant=variant), f"mfma {heads} L={L} rot={rot} variant={variant} maps={sel.kinds}")
        for lay in FLASH_LAYOUTS:
            exact(sel, forward(dev, sel.qkv, heads, layout=lay), f"flash {heads} L={L} rot={rot} {lay} maps={sel.kinds}")


@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_plain_form_takes_the_fp32_fallback_tiles(dev, heads):
    """The plain selector form has |k| = 57600 in every 16 keys: under the default variant every tile of the fp16-pair kernel leaves
    for its fp32 path (|k| >= 32768); the split form merges two such parts."""
    for L, entry in ((2 * ac.TK + 1, "mcr_attention"), (513, "mcr_attention"), (513, "mcr_attention_ws")):
        sel = ac.selector(heads, 1, L, 0, None, "plain")
        for variant in (0, 1):
            exact(sel, forward(dev, sel.qkv, heads, entry=entry, variant=variant), f"plain {entry} {heads} L={L} variant={variant}")
    exact(sel, forward(dev, sel.qkv, heads, layout="q_odd"), f"plain flash {heads} L=513")


@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_mfma_two_query_groups(dev, heads):
    """QG = 2 from cdiv(L, 128) * 4 * S >= 512: S = 64 at L = 129; S = 63 stays at QG = 1; the common sequences agree bit for bit."""
    L, s2, s1 = ac.QG_CASE["L"], ac.QG_CASE["S_qg2"], ac.QG_CASE["S_qg1"]
    sel = ac.selector(heads, s2, L, 0)
    for variant in (0, 1):
        assert "QG2" in ac.forward_route("mcr_attention", heads, s2, L, variant=variant) and "QG1" in ac.forward_route("mcr_attention", heads, s1, L)
        y2 = forward(dev, sel.qkv, heads, variant=variant)
        y1 = forward(dev, sel.qkv[:s1], heads, variant=variant)
        exact(sel, y2, f"QG=2 {heads} variant={variant}")
        exact(sel, y1, f"QG=1 {heads} S={s1} variant={variant}")
        assert np.array_equal(y2[:s1].view(np.int32), y1.view(np.int32))


@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("S,L", ac.SPLIT_SL)
def test_mfma_key_split(dev, heads, S, L):
    """mcr_attention_ws: two blocks per (query tile, head, sequence) take keys [0, kmid) and [kmid, L), attention_combine_kernel merges
    them.  The maps "kmid-1" and "kmid" put all of the weight in one part and none in the other."""
    assert "SPLIT" in ac.forward_route("mcr_attention_ws", heads, S, L)
    for rot in ac._both_rots(S):
        sel = ac.selector(heads, S, L, rot)
        for variant in (0, 1):
            exact(sel, forward(dev, sel.qkv, heads, entry="mcr_attention_ws", variant=variant),
                  f"split {heads} S={S} L={L} kmid={ac.kmid_of(L)} rot={rot} variant={variant} maps={sel.kinds}")
    if L == 513:
        exact(sel, forward(dev, sel.qkv, heads, layout="q+1"), f"flash {heads} L=513")


@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_just_above_the_split_threshold_is_unsplit(dev, heads):
    S, L = ac.UNSPLIT_SL
    assert "WHOLE" in ac.forward_route("mcr_attention_ws", heads, S, L)
    sel = ac.selector(heads, S, L, 0)
    y = forward(dev, sel.qkv, heads, entry="mcr_attention_ws")
    exact(sel, y, f"unsplit {heads} S={S} L={L}")
    assert np.array_equal(y.view(np.int32), forward(dev, sel.qkv, heads).view(np.int32))


def _mask_kind(args):
    return "head" if args[6] is None else ("pair" if args[6] == ac.PAIR_KINDS else "key")


@pytest.mark.parametrize("args", ac.mask_selectors(), ids=ac.sel_id)
def test_masked(dev, args):
    """MASK form (and attention_small_kernel's mask at L = 16 of the (32,128) layout): an all-ones mask gives the unmasked answer; a mask
    that removes every target and all but one of its runner-ups moves the answer to that runner-up, exactly."""
    sel, kind = ac.selector(*args), _mask_kind(args)
    heads, L = args[0], args[2]
    ones = {"head": (np.ones((1, 4, L, L), np.uint8), (4 * L * L, L * L, L)), "pair": (np.ones((1, 1, L, L), np.uint8), (L * L, 0, L)),
            "key": (np.ones((1, 1, 1, L), np.uint8), (L, 0, 0))}[kind]
    exact(sel, forward(dev, sel.qkv, heads, entry="mcr_attention_masked", mask=ones), f"all-ones {kind} mask {heads} L={L}")
    mbytes, strides, _, surv = ac.selector_mask(sel, kind)
    for lay in ("packed", "o_odd+1"):
        exact(sel, forward(dev, sel.qkv, heads, entry="mcr_attention_masked", layout=lay, mask=(mbytes, strides)),
              f"{kind} mask {heads} L={L} {lay} ({ac.forward_route('mcr_attention_masked', heads, 1, L, masked=True)})", keys=surv)


@pytest.mark.parametrize("split_mode", [1, 0, -1])
@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("L", ac.PLANES_L + (ac.PLANES_SHORT_L,))
def test_planes(dev, heads, L, split_mode):
    """attention_planes_kernel: K rows reach LDS with their 16-byte chunks swapped for rows 8..15 of every 16 (DQ = 16), V as
    [DV / 16][64 keys][16] read transposed, partial tiles clamped to the last key: a row or column mix-up is a permutation of keys."""
    sel = ac.selector(heads, 1, L, 0)
    exact(sel, forward(dev, sel.qkv, heads, entry="mcr_attention_planes", split_mode=split_mode),
          f"planes {heads} L={L} split_mode={split_mode} ({ac.planes_route(heads, 1, L, split_mode)}) maps={sel.kinds}")


@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("S2,L,split_mode", [(64, 129, 0), (16, 512, 1)])
def test_planes_two_query_groups(dev, heads, S2, L, split_mode):
    """launch_attention_planes takes QG = 2 from cdiv(L, 128) * 4 * grid.z >= 512 (grid.z = 2 S when split): one sequence fewer stays at 1."""
    assert "QG2" in ac.planes_route(heads, S2, L, split_mode) and "QG1" in ac.planes_route(heads, S2 - 1, L, split_mode)
    sel = ac.selector(heads, S2, L, 0)
    y2 = forward(dev, sel.qkv, heads, entry="mcr_attention_planes", split_mode=split_mode)
    y1 = forward(dev, sel.qkv[:S2 - 1], heads, entry="mcr_attention_planes", split_mode=split_mode)
    exact(sel, y2, f"planes QG=2 {heads} S={S2} L={L}")
    exact(sel, y1, f"planes QG=1 {heads} S={S2 - 1} L={L}")


@pytest.mark.parametrize("split_mode", [1, 0, -1])
@pytest.mark.parametrize("heads", list(ac.HEADS))
def test_planes_lens(dev, heads, split_mode):
    """One sequence per length (0 and L + 5 are clamped): the targets lie below lens[s], and key lens[s], the first excluded one, scores
    C / 2 above every query's target: one key leaking past the length flips the answers.  Rows at or beyond lens[s] get an output
    that is not asserted (the guard is)."""
    lens = tuple(ac.planes_lens(ac.LENS_L))
    sel = ac.selector(heads, len(lens), ac.LENS_L, 0, lens)
    y = forward(dev, sel.qkv, heads, entry="mcr_attention_planes", lens=sel.lens, split_mode=split_mode)
    assert np.isfinite(y).all(), "rows beyond a length hold something non-finite (an unwritten element keeps the fill)"
    exact(sel, y, f"planes lens={list(lens)} kmid(L)={ac.kmid_of(ac.LENS_L)} {heads} split_mode={split_mode} maps={sel.kinds}")


# =====================================================================================================================================
# B. conditioning
# =====================================================================================================================================
@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("kind,L", ac.COND_CASES)
def test_conditioning(dev, kind, heads, L):
    H, qk, v = ac.HEADS[heads]
    x, bound = ac.conditioning_case(kind, heads, L)
    ref = st.attention_ref(x, H, qk, v)
    calls = [("mcr_attention", 0, 0), ("mcr_attention", 1, 0), ("mcr_attention_ws", 0, 0), ("mcr_attention_ws", 1, 0),
             ("mcr_attention_planes", 0, -1), ("mcr_attention_planes", 0, 0)]
    worst = []
    for entry, variant, split_mode in calls:
        y = forward(dev, x, heads, entry=entry, variant=variant, split_mode=split_mode, tag=kind)
        err = float(np.abs(y.astype(np.float64) - ref).max())
        same = " bit-equal to the fp64 mean" if kind == "equal" and np.array_equal(y.astype(np.float64), ref) else ""
        print(f"COND {kind} {heads} L={L} {entry} variant={variant} split_mode={split_mode}: error {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}{same}")
        worst.append((err, entry, variant, split_mode))
    assert all(np.isfinite(e[0]) and e[0] <= bound for e in worst), (bound, worst)


# =====================================================================================================================================
# C. backward
# =====================================================================================================================================
def _backward(dev, sel, g, tag):
    H, qk, v = sel.H, sel.qk, sel.v
    S, L, W = sel.S, sel.L, 2 * sel.qk + sel.v
    pct = qk // H == 8
    Q, G, D = Arena(S * L, W, data=sel.qkv.reshape(-1, W).copy(), device=dev), Arena(S * L, v, data=g.reshape(-1, v).copy(), device=dev), Arena(S * L, W, device=dev)
    lt = None if sel.lens is None else torch.from_numpy(sel.lens).to(dev)
    ws = None
    if not (pct and L == 16):                                           # a16_bwd_kernel touches no workspace: NULL
        nb = L_().mcr_attention_backward_pct_workspace_bytes(I64(S), I64(L)) if pct else L_().mcr_attention_backward_workspace_bytes(I64(S), I64(L), CI(H), CI(v))
        ws = Workspace(int(nb), dev)
    fn = L_().mcr_attention_backward_pct if pct else L_().mcr_attention_backward
    rc = fn(P(Q), I64(Q.ld), P(G), I64(G.ld), P(D), I64(D.ld), I64(S), I64(L), CI(H), CI(qk), CI(v), VP(lt.data_ptr() if lt is not None else None),
            P(ws), SZ(ws.n_bytes if ws else 0), stream())
    sync_ok(rc, tag)
    D.check_guard(tag)
    Q.check_unchanged(tag + " qkv")
    G.check_unchanged(tag + " d_out")
    if ws is not None:
        ws.check_guard(tag + " workspace")
    return D.packed().reshape(S, L, W)


@pytest.mark.parametrize("args", ac.backward_selectors(), ids=ac.sel_id)
def test_backward(dev, args):
    """dv is bit-equal wherever the expected entry is non-zero; there, and in all of dq and dk, |value| <= 4 B (one-hot P: dS of the
    target is 1 * (x - x) = 0 exactly, every other weight is below w_off).  With lens: key lens[s] is the super-selector, the rows of
    dk | dv from lens[s] on are exact zeros and no query moves."""
    sel = ac.selector(*args)
    g = ac.d_out_rows(sel.S, sel.L, sel.v)
    B = ac.backward_bound(sel, g, sel.w_off)
    assert B < 2.0 ** -30
    tag = f"{'mcr_attention_backward_pct' if sel.qk == 32 else 'mcr_attention_backward'} {ac.sel_id(args)} ({ac.backward_route(args[0], sel.S, sel.L)})"
    d = _backward(dev, sel, g, tag)
    qk, dvh = sel.qk, sel.v // sel.H
    want = ac.expected_dv(sel, g)
    got = d[..., 2 * qk:]
    assert np.isfinite(d).all(), tag
    hit = want != 0
    bad = np.argwhere(hit & (got.view(np.int32) != want.view(np.int32)))
    assert bad.size == 0, f"{tag}: dv differs at (sequence, key, column; head = column // {dvh}) {bad[:6].tolist()}: got {got[tuple(bad[:6].T)]}, expected {want[tuple(bad[:6].T)]}"
    rest = max(float(np.abs(got[~hit]).max(initial=0.0)), float(np.abs(d[..., :2 * qk]).max()))
    print(f"BWD {tag}: largest value outside the expected dv {rest:.3e}, 4 B = {4 * B:.3e}")
    assert rest <= 4 * B, f"{tag}: {rest:.3e} > 4 B = {4 * B:.3e}"
    if sel.lens is not None:
        for s in range(sel.S):
            assert not d[s, int(sel.n_keys[s]):, qk:].any(), f"{tag}: keys beyond lens[{s}] must get exact zeros"
