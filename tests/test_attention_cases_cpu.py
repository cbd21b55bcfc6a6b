"""The cases of tests/test_attention_edges_gpu.py, checked on the host (tests/_attention_cases.py): if the construction is tuned, these
conditions are what must keep holding.  Per selector case, from the fp64 reference alone: the arg-max key is pi[s, h, q]; the weight
outside it is below 2^-60; an fp32 emulation of the documented order returns the target's value row bit for bit; q, k and v survive a
round trip through fp16.  With lens: the first excluded key would win every query if it leaked.  Masked cases: the same for the
surviving runner-up, and the masked score stays 64 units of log 2 below it.  Backward cases: B < 2^-30.  Conditioning cases: the fp32
emulation stays within a quarter of the derived bound.  The route table names every instantiation the launchers' conditions give."""
import math

import numpy as np
import pytest

import _attention_cases as ac
import _strided as st

W_OFF_MAX = 2.0 ** -60


def _check_selector(sel, mask=None, keys=None):
    """-> the largest off-target weight of the fp64 reference."""
    keys = sel.pi if keys is None else keys
    H, qk, v = sel.H, sel.qk, sel.v
    expected = sel.expected if mask is None else ac.expected_rows(sel, keys)
    worst = 0.0
    for s in range(sel.S):
        x = sel.qkv[s:s + 1]
        m = None if mask is None else np.broadcast_to(mask, (sel.S, H, sel.L, sel.L))[s:s + 1]
        lens = None if sel.lens is None else sel.lens[s:s + 1]
        w = ac.reference_weights(x, H, qk, m, lens)
        arg, off = ac.off_target_weight(w, keys[s:s + 1])
        assert np.array_equal(arg, keys[s:s + 1]), f"sequence {s}: arg-max differs from the target map at {np.argwhere(arg != keys[s:s + 1])[:4]}"
        assert off < W_OFF_MAX, f"sequence {s}: off-target weight {off:.3e}"
        worst = max(worst, off)
        ref = st.attention_ref(x, H, qk, v, mask=m, lens=lens)
        assert np.abs(ref - expected[s:s + 1]).max() <= ac.V_MOD * W_OFF_MAX
        emu, _ = ac.emulate_fp32(x, H, qk, v, m, lens)
        assert np.array_equal(emu.view(np.int32), expected[s:s + 1].view(np.int32)), f"sequence {s}: the fp32 emulation is not exact"
        if sel.lens is not None and sel.n_keys[s] < sel.L:             # the super-selector: one leaked key flips every answer
            n = int(sel.n_keys[s])
            leak = ac.reference_weights(x, H, qk, None, np.array([n + 1]))
            arg, off = ac.off_target_weight(leak, np.full((1, H, sel.L), n))
            assert (arg == n).all() and off < W_OFF_MAX, f"sequence {s}: key {n} past the length would not win ({off:.3e})"
    return worst


def _check_formats(sel):
    x = sel.qkv
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x), "q | k | v must be exact in one fp16 plane"
    assert np.array_equal(x, np.round(x)) and sel.values.min() >= 1 and sel.values.max() <= ac.V_MOD
    k = np.abs(x[..., sel.qk:2 * sel.qk]).max()
    assert k < (32768 if sel.form == "centred" else 65504), k
    for s in range(sel.S):                                             # distinct along the keys and along the columns
        assert len(np.unique(sel.values[s, :, 0])) == sel.L and len(np.unique(sel.values[s, 0])) == sel.v


@pytest.mark.parametrize("args", ac.forward_selectors(), ids=ac.sel_id)
def test_forward_selector(args):
    sel = ac.selector(*args)
    _check_formats(sel)
    _check_selector(sel)
    heads_maps = {tuple(sel.pi[s, h]) for s in range(sel.S) for h in range(sel.H)}
    assert len(heads_maps) > 1 or sel.L == 1                          # pi differs per head


def test_forward_selectors_cover_every_map_kind():
    for h in ac.HEADS:
        for L in ac.MFMA_L:
            kinds = {k for rot in (0, 4) for row in ac.selector(h, 1, L, rot).kinds for k in row}
            assert kinds == set(ac.MAP_KINDS)
    assert ac.kmid_of(513) == 256 and ac.kmid_of(512) == 256 and ac.kmid_of(575) == 320 and ac.kmid_of(640) == 320   # (Lk / 2 is an integer division)
    for rot in (0, 4):
        sel = ac.selector("64x256", 1, 576, rot)
        for h, kind in enumerate(sel.kinds[0]):
            if kind == "kmid":
                assert (sel.pi[0, h] == ac.kmid_of(576)).all() and ac.kmid_of(576) == 320
            if kind == "kmid-1":
                assert (sel.pi[0, h] == ac.kmid_of(576) - 1).all()


@pytest.mark.parametrize("args", ac.mask_selectors(), ids=ac.sel_id)
def test_masked_selector(args):
    sel = ac.selector(*args)
    kind = "head" if args[6] is None else ("pair" if args[6] == ac.PAIR_KINDS else "key")
    _check_formats(sel)
    _check_selector(sel, mask=np.ones((1, 1, 1, sel.L), bool))        # an all-ones mask: the unmasked answer
    mbytes, strides, keep, surv = ac.selector_mask(sel, kind)
    assert mbytes.shape == {"head": (sel.S, sel.H, sel.L, sel.L), "pair": (sel.S, 1, sel.L, sel.L), "key": (sel.S, 1, 1, sel.L)}[kind]
    _check_selector(sel, mask=keep, keys=surv)
    kb = np.broadcast_to(keep, (sel.S, sel.H, sel.L, sel.L))
    assert not np.take_along_axis(kb, sel.pi[..., None], -1).any(), "every target is masked"
    assert np.take_along_axis(kb, surv[..., None], -1).all() and (surv != sel.pi).all()
    # the masked score -1e3 / sqrt(dq) against the survivor's -(C / 2) / sqrt(dq), in units of log 2
    dq = sel.qk // sel.H
    assert (1e3 - ac.C / 2) * ac.LOG2E / math.sqrt(dq) >= 64


@pytest.mark.parametrize("args", ac.backward_selectors(), ids=ac.sel_id)
def test_backward_selector(args):
    sel = ac.selector(*args)
    _check_formats(sel)
    w_off = _check_selector(sel)
    g = ac.d_out_rows(sel.S, sel.L, sel.v)
    assert g.min() >= 1 and g.max() <= 7 and np.array_equal(g, np.round(g))
    B = ac.backward_bound(sel, g, w_off)
    assert B < 2.0 ** -30, B
    dv = ac.expected_dv(sel, g)
    assert np.isclose(dv.astype(np.float64).sum(), g.astype(np.float64).sum())        # every query's d_out lands on one key
    kinds = {k for row in sel.kinds for k in row}
    assert kinds == set(ac.BWD_KINDS)
    for s in range(sel.S):
        for h, kind in enumerate(sel.kinds[s]):
            cols = slice(h * (sel.v // sel.H), (h + 1) * (sel.v // sel.H))
            if kind == "first":
                assert np.array_equal(dv[s, 0, cols], g[s, :, cols].astype(np.float64).sum(0).astype(np.float32)) and not dv[s, 1:, cols].any()
            elif sel.lens is None:
                assert (dv[s, :, cols] != 0).all()                                        # a permutation: every key gets one query
        if sel.lens is not None:
            assert not dv[s, int(sel.n_keys[s]):].any()
    # fp64 autograd agrees: dv to rounding, dq and dk below 4 B
    if sel.S * sel.L <= 130:
        ref = st.attention_backward_ref(sel.qkv, g, sel.H, sel.qk, sel.v, sel.lens)
        assert np.abs(ref[..., 2 * sel.qk:] - dv).max() <= 4 * B and np.abs(ref[..., :2 * sel.qk]).max() <= 4 * B


@pytest.mark.parametrize("heads", list(ac.HEADS))
@pytest.mark.parametrize("kind,L", ac.COND_CASES)
def test_conditioning_case(kind, heads, L):
    H, qk, v = ac.HEADS[heads]
    x, bound = ac.conditioning_case(kind, heads, L)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() < 2048
    ref = st.attention_ref(x, H, qk, v)
    emu, _ = ac.emulate_fp32(x, H, qk, v)
    err = float(np.abs(emu - ref).max())
    print(f"{kind} {heads} L={L}: emulation error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound / 4, (err, bound)
    sc = x[0, :, :qk // H].astype(np.float64) @ x[0, :, qk:qk + qk // H].astype(np.float64).T * ac.LOG2E / math.sqrt(qk // H)
    if kind == "common+":
        assert sc.min() > 1.9e4 and sc.max() - sc.min() < 40
    elif kind == "common-":
        assert sc.max() < -1.9e4
    elif kind == "growing" and L == 513:
        assert sc[0].max() - sc[0, :64].max() > 128                     # exp2 overflows fp32 without the running-max rescale
    elif kind == "equal":
        assert np.array_equal(ref, np.broadcast_to(x[..., 2 * qk:].astype(np.float64).mean(1, keepdims=True), ref.shape))


def test_route_table_names_every_reachable_instantiation():
    names = [r[0] for r in ac.ROUTES]
    assert len(set(names)) == len(names)
    for row in ac.ROUTES:
        assert ac.route_of(row) == row[0], row
    want = {"attention_small_kernel<16,4,8,32,4>", "attention_small_kernel<16,4,8,32,4> +mask", "a16_bwd_kernel"}
    for dq, dv in ((8, 32), (16, 64)):
        want.add(f"attention_flash_kernel<{dq},{dv},4>")
        for form, qgs in (("PVH", (1, 2)), ("F32", (1, 2)), ("MASK", (1,))):
            want |= {f"attention_mfma_kernel<{dq},{dv},WHOLE,{form},QG{g}>" for g in qgs}
            want.add(f"attention_mfma_kernel<{dq},{dv},SPLIT,{form},QG1>+attention_combine_kernel")
        for g in (1, 2):
            want |= {f"attention_planes_kernel<{dq},{dv},WHOLE,QG{g},NP2>", f"attention_planes_kernel<{dq},{dv},SPLIT,QG{g},NP2>+attention_combine_kernel"}
    assert want <= set(names), want - set(names)
    assert {ac.ab_nsplit(S, L) for S, L in ac.BWD_NSPLIT_SL} == {1, 2, 4} and [ac.ab_nsplit(S, L) for S, L in ac.BWD_NSPLIT_SL] == [2, 4, 1, 2]
    # the shapes of section A against the launchers' conditions
    L, s2, s1 = ac.QG_CASE["L"], ac.QG_CASE["S_qg2"], ac.QG_CASE["S_qg1"]
    assert (L, s2, s1) == (129, 64, 63) and "QG2" in ac.forward_route("mcr_attention", "64x256", s2, L) and "QG1" in ac.forward_route("mcr_attention", "64x256", s1, L)
    for S, L in ac.SPLIT_SL:
        assert "SPLIT" in ac.forward_route("mcr_attention_ws", "32x128", S, L)
    assert "WHOLE" in ac.forward_route("mcr_attention_ws", "32x128", *ac.UNSPLIT_SL)
    assert "WHOLE" in ac.forward_route("mcr_attention_ws", "32x128", 1, 511)
    assert ac.planes_lens(577) == [0, 1, 63, 64, 65, 319, 320, 321, 576, 577, 582]
