"""Ragged SconeOcc HIP backward (scone_occ_bwd.hip: mcr_scone_occ_backward_ragged; ops.scone_occ_backward_ragged,
autograd.SconeOccRaggedFunction, SconeOcc.forward_ragged(..., differentiable=True)) against the fp64 torch composite
(autograd.scone_occ_ragged on a float64 copy of the module; tests/test_scone_occ_ragged_grad_cpu.py ties that composite to J separate
calls), in the metric and on the bounds of tests/test_pct_backward_gpu.py: max |got - ref| / max |ref| per tensor < NET_TOL = 1e-4,
parameter denominators floored at 1e-4 x the largest parameter gradient; the mathematically zero mhsa.w_k.bias gradients are bounded as
in tests/test_scone_occ_backward_gpu.py (whose _check is used); between two fp32 results, which both carry that noise, their difference
is bounded by ZERO_TOL x the largest parameter gradient (`ez` below is that difference over the floor of 1e-4 x the
largest).  Inputs by that file's protocol: the first of eight seeds on which the fp32 TORCH composite agrees with the fp64 one to
WELL_POSED = 1e-5; no HIP result takes part in the choice.
The pooling backward with lengths has a block entry (mcr_pool_max_avg_backward_lens) and is tested on its own against torch (d).  The
other three new kernels (so_pad_global_kernel, so_bcast_rows_kernel, so_seg_colsum_kernel) have none: they are covered through the
network, (a) - (c).  Measured errors are printed with an ERR prefix."""
import numpy as np
import pytest
import torch

import test_pct_backward_gpu as P
import test_scone_occ_backward_gpu as O
from test_pct_backward_gpu import BLOCK_TOL, NET_TOL, WELL_POSED, ZERO_TOL, T, err

pytestmark = pytest.mark.gpu

LG = 48
CLOUDS = (300, 150, 75)                                   # points per job and scale of the entry-level cases


def _row_job(rows, dev):
    return torch.from_numpy(np.repeat(np.arange(len(rows)), rows).astype(np.int32)).to(dev)


def _composite(model, dtype, pcg, glen, offsets, x0, vq, row_job, up=None):
    """(param grads by name, d_x, d_vh) of sum(up * SconeOcc ragged) through the torch composite on `model` in `dtype`."""
    from macarons_amd import autograd as A
    x = x0.to(dtype, copy=True).requires_grad_(True)
    v = vq.to(dtype, copy=True).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    y = A.scone_occ_ragged(model, pcg.to(dtype), glen, [o.to(dtype) for o in offsets], x, v, row_job)
    (y if up is None else y * up.to(dtype)).sum().backward()
    return {n: q.grad.clone() for n, q in model.named_parameters()}, x.grad.clone(), v.grad.clone()


def _offsets(x, rows, rng, dev, sizes=CLOUDS):
    """per scale [T,16,3]: every job's rows against a cloud of its own (the jobs without rows take no part in the search)"""
    from macarons_amd import ops
    live = [q for q in rows if q > 0]
    out = []
    for M in sizes:
        pc = T(rng.uniform(-.3, .3, (M * len(live), 3)), dev)
        out.append(ops.knn_offsets_segmented(x, pc, [M] * len(live), live))
    return out


@pytest.fixture(scope="module")
def nets(dev):
    import os
    saved = os.environ.pop("MCR_SCONE_OCC_BWD", None)
    try:
        yield P._occ(dev), P._occ(dev, torch.float64)
    finally:
        if saved is not None:
            os.environ["MCR_SCONE_OCC_BWD"] = saved


def _well_posed(tag, nets, dev, make, first_seed):
    """the first of eight seeds on which the fp32 torch composite agrees with the fp64 one to WELL_POSED; make(rng) -> the composite's
    arguments behind the model and the dtype"""
    occ, od = nets
    for seed in range(first_seed, first_seed + 8):
        args = make(np.random.default_rng(seed))
        ref = _composite(od, torch.float64, *args)
        t32 = _composite(occ, torch.float32, *args)
        yard = P._worst(t32[:2], ref[:2]) + (err(t32[2], ref[2]),)
        print(f"ERR {tag} seed {seed}: fp32 torch composite vs fp64: params max {yard[0]:.2e}  d_x {yard[1]:.2e}  d_vh {yard[2]:.2e}")
        if max(yard[:2]) < WELL_POSED:
            print(f"ERR {tag}: seed {seed} taken, {seed - first_seed} draw(s) rejected before it")
            occ.zero_grad(set_to_none=True)
            return args, ref, t32
    pytest.fail("no well-posed draw among eight")


# ---- the entry-level case of (a), (b), (c): 4 jobs, one of a single row, one without rows ---------------------------------------------
ROWS_A, LEN_A = (50, 1, 0, 45), (48, 17, 33, 20)


@pytest.fixture(scope="module")
def case_a(dev, nets):
    def make(rng):
        n = sum(ROWS_A)
        pcg = T(rng.uniform(-.3, .3, (len(ROWS_A), LG, 3)), dev)
        x0 = T(rng.uniform(-.4, .4, (n, 3)), dev)
        vq = T(rng.standard_normal((n, 64)) * 0.3, dev)
        return (pcg, torch.tensor(LEN_A, dtype=torch.int32, device=dev), _offsets(x0, ROWS_A, rng, dev), x0, vq, _row_job(ROWS_A, dev))
    args, ref, t32 = _well_posed("scone_occ ragged (a)", nets, dev, make, 40)
    return dict(occ=nets[0], args=args, ref=ref, t32=t32, rows=ROWS_A)


def _call(c, pcg=None, keep=None, **kw):
    """ops.scone_occ_backward_ragged on case c with d_out = 1 (keep: the jobs that stay, in order -- none of the dropped may have rows)"""
    from macarons_amd import ops
    p, glen, offsets, x0, vq, row_job = c["args"]
    p = p if pcg is None else pcg
    rows = list(c["rows"])
    if keep is not None:
        assert all(rows[j] == 0 for j in range(len(rows)) if j not in keep)
        idx = torch.tensor(keep, device=p.device)
        p, glen, rows = p[idx].contiguous(), glen[idx].contiguous(), [rows[j] for j in keep]
        row_job = _row_job(rows, p.device)
    kw.setdefault("q_chunk", 32)
    return ops.scone_occ_backward_ragged(p, glen, offsets, x0, vq, row_job, rows, torch.ones(x0.shape[0], 1, device=p.device),
                                         c["occ"].weight_table(), **kw)


def _same(a, b):
    return all(torch.equal(s, t) for s, t in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- (a) the entry against the fp64 composite ------------------------------------------------------------------------------------------
def test_entry_against_fp64_composite(dev, case_a):
    c = case_a
    got = _call(c)                                   # 96 rows in chunks of 32: job 0 is cut twice, the last chunk spans jobs 0 - 3
    assert len(got[0]) == 140 and got[1].shape == (96, 3) and got[2].shape == (96, 64)
    O._check("scone_occ ragged (a) q_chunk=32", (O._by_name(c["occ"], got[0]), got[1], got[2]), c)
    assert _same(got, _call(c)), "two calls must give identical bits"
    assert _same(got, _call(c, keep=[0, 1, 3])), "a job without rows must contribute exact zeros"


# ---- (b) need --------------------------------------------------------------------------------------------------------------------------
def test_need(dev, monkeypatch, case_a):
    from macarons_amd import ops
    c = case_a
    full = _call(c)
    w_only, x_only, v_only = (_call(c, need=n) for n in ((True, False, False), (False, True, False), (False, False, True)))
    assert w_only[1] is None and w_only[2] is None and x_only[0] is None and x_only[2] is None and v_only[0] is None and v_only[1] is None
    assert all(torch.equal(a, b) for a, b in zip(full[0], w_only[0]))
    assert torch.equal(full[1], x_only[1]) and torch.equal(full[2], v_only[2])
    wx = _call(c, need=(True, True, False))
    assert wx[2] is None and all(torch.equal(a, b) for a, b in zip(full[0], wx[0])) and torch.equal(full[1], wx[1])
    entered, real = [], ops.check
    monkeypatch.setattr(ops, "check", lambda rc, what: (entered.append(what), real(rc, what))[1])
    assert _call(c, need=(False, False, False)) == (None, None, None) and not entered
    _call(c, need=(False, False, True))
    assert entered == ["mcr_scone_occ_backward_ragged"]


# ---- (c) the padding rows of pc_global are never used ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_padding(dev, case_a, fill):
    c = case_a
    pcg = c["args"][0].clone()
    for j, n in enumerate(LEN_A):
        pcg[j, n:] = fill
    got = _call(c, pcg=pcg)
    assert all(bool(torch.isfinite(t).all()) for t in (*got[0], got[1], got[2]))
    assert _same(got, _call(c))


# ---- (d) the pooling backward with lengths on its own -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S,L,E", [(1, 17, 128), (3, 150, 256)])
def test_pool_backward_with_lengths(dev, S, L, E):
    from macarons_amd import ops
    rng = np.random.default_rng(S * 100000 + L * 1000 + E)
    x = rng.standard_normal((S, L, E)).astype(np.float32)
    lens = [1, L, L // 2][-S:] if S > 1 else [L // 2]
    for s_, n in enumerate(lens):                    # a tie inside the valid rows: the lowest row wins; a larger value behind them: not seen
        if n >= 4:
            x[s_, n - 1, 5] = x[s_, 2, 5] = 9.0
        if n < L:
            x[s_, n:, 7] = 50.0
    g = rng.standard_normal((S, 2 * E)).astype(np.float32)
    xt, gt = T(x, dev), T(g, dev)
    for ln in (lens, [L] * S, [1] * S):
        got = ops.pool_max_avg_backward(xt, gt, torch.tensor(ln, dtype=torch.int32, device=dev)).cpu().numpy()
        ref = np.zeros((S, L, E))
        for s_, n in enumerate(ln):
            ref[s_, :n] = g[s_, None, E:].astype(np.float64) / n
            ref[s_, x[s_, :n].argmax(axis=0), np.arange(E)] += g[s_, :E]          # (numpy's argmax: the first of equal maxima)
        e = err(got, ref)
        print(f"ERR pool backward with lengths S={S} L={L} E={E} lens={ln}: {e:.2e}")
        assert e < BLOCK_TOL
        for s_, n in enumerate(ln):
            assert (got[s_, n:] == 0).all(), "rows beyond the length must be exact zeros"
            if n >= 4 and ln is lens:                # the tie went to the lower row alone
                avg = g[s_, E + 5] / np.float32(n)
                assert abs(got[s_, n - 1, 5] - avg) < 1e-7 and abs(got[s_, 2, 5] - (avg + g[s_, 5])) < 1e-6
    assert torch.equal(ops.pool_max_avg_backward(xt, gt, torch.tensor([L] * S, dtype=torch.int32, device=dev)), ops.pool_max_avg_backward(xt, gt))


# ---- (e) agreement with the uniform entry ----------------------------------------------------------------------------------------------
def test_agrees_with_uniform_entry(dev, nets):
    from macarons_amd import ops
    occ, od = nets
    B, Q, qc = 2, 48, 32                             # uniform: chunks 32 + 16 per cloud; ragged: 32 | 16 + 16 | 32, the middle one spans both

    def make(rng):
        pcg = T(rng.uniform(-.3, .3, (B, LG, 3)), dev)
        x0 = T(rng.uniform(-.4, .4, (B, Q, 3)), dev)
        vq = T(rng.standard_normal((B * Q, 64)) * 0.3, dev)
        make.scales = [T(rng.uniform(-.3, .3, (B, M, 3)), dev) for M in CLOUDS]
        make.idx = [ops.knn_points(x0, s_, 16)[2] for s_ in make.scales]
        offsets = [(torch.gather(s_[:, None].expand(-1, Q, -1, -1), 2, i_[..., None].expand(-1, -1, -1, 3)) - x0[:, :, None, :])
                   .reshape(B * Q, 16, 3).contiguous() for s_, i_ in zip(make.scales, make.idx)]
        return (pcg, torch.full((B,), LG, dtype=torch.int32, device=dev), offsets, x0.reshape(B * Q, 3), vq, _row_job([Q] * B, dev))
    args, ref, t32 = _well_posed("scone_occ ragged (e)", nets, dev, make, 50)
    pcg, glen, offsets, x0, vq, row_job = args
    g = torch.ones(B * Q, 1, device=dev)
    rag = ops.scone_occ_backward_ragged(pcg, glen, offsets, x0, vq, row_job, [Q] * B, g, occ.weight_table(), q_chunk=qc)
    uni = ops.scone_occ_backward(pcg, make.scales, x0.view(B, Q, 3), vq.view(B, Q, 64), make.idx, g.view(B, Q, 1), occ.weight_table(),
                                 q_chunk=qc)
    assert torch.equal(rag[1], uni[1].reshape(B * Q, 3)) and torch.equal(rag[2], uni[2].reshape(B * Q, 64))
    c = dict(ref=ref, t32=t32)
    O._check("scone_occ ragged (e) ragged entry", (O._by_name(occ, rag[0]), rag[1], rag[2]), c)
    O._check("scone_occ ragged (e) uniform entry", (O._by_name(occ, uni[0]), uni[1].reshape(B * Q, 3), uni[2].reshape(B * Q, 64)), c)
    ew, ez = O._between(O._by_name(occ, rag[0]), O._by_name(occ, uni[0]))
    print(f"ERR scone_occ ragged (e) ragged vs uniform entry: params max {ew:.2e} (zero gradients, floored: {ez:.2e})")


# ---- (f) the default chunk's boundary ---------------------------------------------------------------------------------------------------
def test_default_chunk_boundary(dev, nets):
    from macarons_amd import ops
    occ = nets[0]
    rows = (1500, 551)
    n = sum(rows)
    assert n == ops.scone_occ_backward_chunk(10 ** 6) + 3
    rng = np.random.default_rng(61)
    pcg = T(rng.uniform(-.3, .3, (2, LG, 3)), dev)
    glen = torch.tensor((48, 31), dtype=torch.int32, device=dev)
    x0 = T(rng.uniform(-.4, .4, (n, 3)), dev)
    vq = T(rng.standard_normal((n, 64)) * 0.3, dev)
    g = T(rng.standard_normal((n, 1)), dev)
    offsets = _offsets(x0, rows, rng, dev)
    call = lambda qc: ops.scone_occ_backward_ragged(pcg, glen, offsets, x0, vq, _row_job(rows, dev), rows, g, occ.weight_table(), q_chunk=qc)
    two, one, again = call(0), call((n + 15) // 16 * 16), call(0)
    assert _same(two, again)
    assert all(bool(torch.isfinite(t).all()) for t in (*two[0], *one[0], two[1], two[2], one[1], one[2]))
    assert torch.equal(two[1], one[1]) and torch.equal(two[2], one[2])
    ew, ez = O._between(O._by_name(occ, two[0]), O._by_name(occ, one[0]))
    print(f"ERR scone_occ ragged (f) T={n}: chunks of {n - 3} + 3 vs one chunk: params max {ew:.2e} (zero gradients, floored: {ez:.2e})")
    assert ew < NET_TOL and ez * 1e-4 < ZERO_TOL


# ---- (g), (h), (i): the module ----------------------------------------------------------------------------------------------------------
SIZES_G, ROWS_G = (65, 300, 2100), (20, 1, 30)      # the smallest cloud the reference admits, one below seq_len, one above it


@pytest.fixture(scope="module")
def case_g(dev, nets):
    from macarons_amd import ops
    occ, od = nets
    torch.manual_seed(6)
    perms = [occ.draw_perms(M) for M in SIZES_G]
    J, Lg, n = len(SIZES_G), occ.seq_len, sum(ROWS_G)
    row_job = _row_job(ROWS_G, dev)
    state = {}

    def make(rng):
        pc = T(rng.uniform(-.3, .3, (sum(SIZES_G), 3)), dev)
        x0 = T(rng.uniform(-.4, .4, (n, 3)), dev)
        vq = T(rng.standard_normal((n, 64)) * 0.3, dev)
        with torch.no_grad():
            y_ng = occ.forward_ragged(pc, list(SIZES_G), x0, vq, list(ROWS_G), perms=perms)
        ia = occ.last_ragged_perms
        pc1 = pc[ia["idx1"]]
        clouds = [pc, pc1, pc1[ia["idx2"]]]
        sz = [occ.scale_sizes(M) for M in SIZES_G]
        offsets = [ops.knn_offsets_segmented(x0, c_.contiguous(), [s_[i] for s_ in sz], list(ROWS_G)) for i, c_ in enumerate(clouds)]
        state.update(pc=pc, y_ng=y_ng)
        return (pc[ia["g_idx"]].view(J, Lg, 3), ia["g_len"], offsets, x0, vq, row_job)
    args, ref, t32 = _well_posed("scone_occ ragged (g)", nets, dev, make, 60)
    assert args[1].tolist() == [65, 300, 2048]
    return dict(occ=occ, perms=perms, args=args, ref=ref, t32=t32, **state)


def _module_grads(c, **kw):
    occ = c["occ"]
    x = c["args"][3].clone().requires_grad_(True)
    v = c["args"][4].clone().requires_grad_(True)
    occ.zero_grad(set_to_none=True)
    y = occ.forward_ragged(c["pc"], list(SIZES_G), x, v, list(ROWS_G), perms=c["perms"], differentiable=True, **kw)
    y.sum().backward()
    assert all(q.grad is not None for q in occ.parameters())
    return y, ({n_: q.grad.clone() for n_, q in occ.named_parameters()}, x.grad.clone(), v.grad.clone())


def test_module_under_autograd(dev, monkeypatch, case_g):
    from macarons_amd import ops
    c = case_g
    occ = c["occ"]
    assert len(list(occ.parameters())) == 172
    monkeypatch.delenv("MCR_SCONE_OCC_BWD", raising=False)
    n_bwd, real = [], ops.scone_occ_backward_ragged
    monkeypatch.setattr(ops, "scone_occ_backward_ragged", lambda *a, **k: (n_bwd.append(1), real(*a, **k))[1])
    y, first = _module_grads(c)
    assert y.grad_fn is not None and y.shape == (sum(ROWS_G), 1) and torch.equal(y.detach(), c["y_ng"])
    assert len(n_bwd) == 1
    O._check("scone_occ ragged (g) module", first, c)
    _, again = _module_grads(c)
    assert O._same(first + (None,), again + (None,)), "two backward passes over fresh graphs must give identical bits"
    # ... and the J per-job forward() calls (composite backward), summed over the jobs
    x0, vq = c["args"][3], c["args"][4]
    o0, r0 = np.concatenate(([0], np.cumsum(SIZES_G))), np.concatenate(([0], np.cumsum(ROWS_G)))
    occ.zero_grad(set_to_none=True)
    dx, dv = [], []
    for j in range(len(SIZES_G)):
        xj = x0[r0[j]:r0[j + 1]][None].clone().requires_grad_(True)
        vj = vq[r0[j]:r0[j + 1]][None].clone().requires_grad_(True)
        occ(c["pc"][o0[j]:o0[j + 1]][None], xj, vj, perms=c["perms"][j]).sum().backward()
        dx.append(xj.grad[0]); dv.append(vj.grad[0])
    per_job = {n_: q.grad.clone() for n_, q in occ.named_parameters()}
    ew, ez = O._between(first[0], per_job)
    ex, ev = err(first[1], torch.cat(dx)), err(first[2], torch.cat(dv))
    print(f"ERR scone_occ ragged (g) module vs {len(SIZES_G)} per-job forward() calls (composite, fp32): params max {ew:.2e} (zero gradients, "
          f"floored: {ez:.2e})  d_x {ex:.2e}  d_vh {ev:.2e}")
    assert max(ew, ex, ev) < NET_TOL and ez * 1e-4 < ZERO_TOL


def test_refusals(dev, case_g, case_a):
    from macarons_amd import _lib, ops
    c = case_g
    occ = c["occ"]
    x0, vq = c["args"][3], c["args"][4]
    call = lambda pc, **kw: occ.forward_ragged(pc, list(SIZES_G), x0, vq, list(ROWS_G), perms=c["perms"], differentiable=True, **kw)
    with pytest.raises(NotImplementedError):
        call(c["pc"].clone().requires_grad_())
    with pytest.raises(ValueError):
        call(c["pc"], out=torch.empty(sum(ROWS_G), 1, device=dev))
    x = x0.clone().requires_grad_(True)
    y = occ.forward_ragged(c["pc"], list(SIZES_G), x, vq, list(ROWS_G), perms=c["perms"], differentiable=True)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(y.sum(), [x] + list(occ.parameters()), create_graph=True)
    # the entry: global sequences of 16 tokens, a bad q_chunk
    for qc in (8, 40, -16):
        with pytest.raises(_lib.MacaronsHipError, match="q_chunk must be"):
            _call(case_a, q_chunk=qc)
    p, glen, offsets, xa, va, row_job = case_a["args"]
    with pytest.raises(_lib.MacaronsHipError, match="mcr_scone_occ_backward_ragged.*16 tokens"):
        ops.scone_occ_backward_ragged(p[:, :16].contiguous(), glen.clamp(max=16), offsets, xa, va, row_job, list(ROWS_A),
                                      torch.ones(xa.shape[0], 1, device=dev), occ.weight_table())
    with pytest.raises(ValueError):
        ops.scone_occ_backward_ragged(p, glen, offsets, xa, va, row_job, [50, 1, 0, 44], torch.ones(xa.shape[0], 1, device=dev),
                                      occ.weight_table())


def test_without_the_keyword_nothing_changes(dev, case_g):
    c = case_g
    occ = c["occ"]
    assert torch.is_grad_enabled() and all(q.requires_grad for q in occ.parameters())
    x = c["args"][3].clone().requires_grad_(True)
    y = occ.forward_ragged(c["pc"], list(SIZES_G), x, c["args"][4], list(ROWS_G), perms=c["perms"])
    assert not y.requires_grad and y.grad_fn is None and torch.equal(y, c["y_ng"])
    with torch.no_grad():
        y2 = occ.forward_ragged(c["pc"], list(SIZES_G), x, c["args"][4], list(ROWS_G), perms=c["perms"], differentiable=True)
    assert not y2.requires_grad and torch.equal(y2, c["y_ng"])
