"""SconeOcc HIP backward (scone_occ_bwd.hip: mcr_scone_occ_backward; autograd.SconeOccFunction, env MCR_SCONE_OCC_BWD=hip) against the
fp64 torch composite (autograd.scone_occ on a float64 copy of the module), in the metric and on the bounds of
tests/test_pct_backward_gpu.py: max |got - ref| / max |ref| per tensor < NET_TOL = 1e-4, parameter denominators floored at 1e-4 x the
largest parameter gradient; the mathematically zero mhsa.w_k.bias gradients are bounded absolutely, at ZERO_TOL x the largest parameter
gradient or 4 x what the fp32 torch composite leaves there on the same inputs, whichever is larger.  The inputs are chosen by that
file's protocol (pooled maxima make the gradient discontinuous at near-ties): the first seed of 22 + B ... 29 + B on which the fp32
TORCH composite agrees with the fp64 one to 1e-5; no HIP result takes part in the choice.  The gather and the query's share of the
offsets' gradient have no entry of their own: they are covered through the network (d_x, and every local transformer's gradients).
Measured errors are printed with an ERR prefix."""
import ctypes

import numpy as np
import pytest
import torch

import test_pct_backward_gpu as P
from test_pct_backward_gpu import NET_TOL, ZERO_GRAD, ZERO_TOL, WELL_POSED, T, err

pytestmark = pytest.mark.gpu

I64, CI, VP, SZ = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t


def _composite(model, dtype, dp, pc, x0, vq, scales, idx):
    """(param grads by name, d_x, d_vh) of sum(SconeOcc) through the torch composite on `model` in `dtype`."""
    from macarons_amd import autograd as A
    x = x0.to(dtype, copy=True).requires_grad_(True)
    v = vq.to(dtype, copy=True).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    A.scone_occ(model, pc[:, dp[0]].to(dtype), [s_.to(dtype) for s_ in scales], x, v, idx).sum().backward()
    return {n: q.grad.clone() for n, q in model.named_parameters()}, x.grad.clone(), v.grad.clone()


@pytest.fixture(scope="module")
def cases(dev):
    """B -> the module, the pinned draws, the well-posed inputs and both torch composites' gradients: computed once, shared, never changed."""
    import os
    from macarons_amd import ops
    out = {}

    def get(B):
        if B in out:
            return out[B]
        saved = os.environ.pop("MCR_SCONE_OCC_BWD", None)          # the references are the all-torch composite
        try:
            occ, od = P._occ(dev), P._occ(dev, torch.float64)
            torch.manual_seed(4)
            perms = occ.draw_perms(300)
            dp = [p.to(dev) for p in perms]
            for seed in range(22 + B, 30 + B):
                rng = np.random.default_rng(seed)
                pc = T(rng.uniform(-.3, .3, (B, 300, 3)), dev)
                x0 = T(rng.uniform(-.4, .4, (B, 50, 3)), dev)
                vq = T(rng.standard_normal((B, 50, 64)) * 0.3, dev)
                scales = [pc, pc[:, dp[1]].contiguous()]
                scales.append(scales[1][:, dp[2]].contiguous())
                idx = [ops.knn_points(x0.contiguous(), s_, 16)[2] for s_ in scales]
                ref = _composite(od, torch.float64, dp, pc, x0, vq, scales, idx)
                t32 = _composite(occ, torch.float32, dp, pc, x0, vq, scales, idx)
                yard = P._worst(t32[:2], ref[:2]) + (err(t32[2], ref[2]),)
                print(f"ERR scone_occ hip B={B} seed {seed}: fp32 torch composite vs fp64: params max {yard[0]:.2e}  d_x {yard[1]:.2e}  "
                      f"d_vh {yard[2]:.2e}")
                if max(yard[:2]) < WELL_POSED:
                    print(f"ERR scone_occ hip B={B}: seed {seed} taken, {seed - 22 - B} draw(s) rejected before it")
                    break
            else:
                pytest.fail("no well-posed draw among eight")
        finally:
            if saved is not None:
                os.environ["MCR_SCONE_OCC_BWD"] = saved
        occ.zero_grad(set_to_none=True)
        out[B] = dict(occ=occ, perms=perms, dp=dp, pc=pc, x0=x0, vq=vq, scales=scales, idx=idx, ref=ref, t32=t32)
        return out[B]
    return get


def _check(tag, got, c):
    """got = (param grads by name, d_x, d_vh) against the fp64 reference of case c, on the bounds of the module docstring."""
    ref, t32 = c["ref"], c["t32"]
    scale = max(float(t.abs().max()) for t in ref[0].values())
    worst = 0.0
    for n in ref[0]:
        if n.endswith(ZERO_GRAD):
            e = float((got[0][n].double() - ref[0][n]).abs().max()) / scale
            e32 = float((t32[0][n].double() - ref[0][n]).abs().max()) / scale
            print(f"ERR {tag}: {n} (zero gradient) {e:.2e} x the largest (fp32 composite: {e32:.2e})")
            assert e < max(ZERO_TOL, 4 * e32), (tag, n, e, e32)
            continue
        e = err(got[0][n], ref[0][n], 1e-4 * scale)
        worst = max(worst, e)
        assert e < NET_TOL, (tag, n, e)
    ex, ev = err(got[1], ref[1]), err(got[2], ref[2])
    print(f"ERR {tag}: params max {worst:.2e}  d_x {ex:.2e}  d_vh {ev:.2e}")
    assert ex < NET_TOL and ev < NET_TOL, (tag, ex, ev)


def _by_name(occ, d_w):
    """the 140 table gradients of ops.scone_occ_backward as the 172 parameters' gradients by name"""
    params, slots = occ._grad_slots()
    names = [n for n, _ in occ.named_parameters()]
    return {n: (d_w[k] if rows is None else d_w[k][rows[0]:rows[1]]) for n, (k, rows) in zip(names, slots)}


def _grads(c, pc_grad=False):
    occ = c["occ"]
    x = c["x0"].clone().requires_grad_(True)
    v = c["vq"].clone().requires_grad_(True)
    pc = c["pc"].clone().requires_grad_(True) if pc_grad else c["pc"]
    occ.zero_grad(set_to_none=True)
    occ(pc, x, v, perms=c["perms"]).sum().backward()
    return {n: q.grad.clone() for n, q in occ.named_parameters()}, x.grad.clone(), v.grad.clone(), (pc.grad.clone() if pc_grad else None)


def _same(a, b):
    return (all(torch.equal(a[0][n], b[0][n]) for n in a[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
            and (a[3] is None or torch.equal(a[3], b[3])))


def _between(a, b):
    """two HIP results by name, in the parameters' metric: (the largest error but the zero gradients', the zero gradients' -- noise
    over the floor of 1e-4 x the largest gradient)"""
    scale = max(float(t.abs().max()) for t in b.values())
    e = {n: err(a[n], b[n], 1e-4 * scale) for n in a}
    return (max(v for n, v in e.items() if not n.endswith(ZERO_GRAD)), max(v for n, v in e.items() if n.endswith(ZERO_GRAD)))


def _table_call(c, **kw):
    from macarons_amd import ops
    occ = c["occ"]
    g = torch.ones(c["x0"].shape[0], c["x0"].shape[1], 1, device=c["x0"].device)
    return ops.scone_occ_backward(c["pc"][:, c["dp"][0]].contiguous(), c["scales"], c["x0"], c["vq"], c["idx"], g, occ.weight_table(), **kw)


# ---- 2. the whole network under autograd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_network_under_autograd(dev, monkeypatch, cases, B):
    from macarons_amd import autograd as A, ops
    c = cases(B)
    occ = c["occ"]
    assert len(list(occ.parameters())) == 172
    monkeypatch.setenv("MCR_SCONE_OCC_BWD", "hip")
    n_bwd, n_comp, n_pct = [], [], []
    real_bwd, real_comp, real_pct = ops.scone_occ_backward, A.pc_transformer, A.PCTransformerFunction.backward
    monkeypatch.setattr(ops, "scone_occ_backward", lambda *a, **k: (n_bwd.append(1), real_bwd(*a, **k))[1])
    monkeypatch.setattr(A, "pc_transformer", lambda pct, t: (n_comp.append(1), real_comp(pct, t))[1])
    monkeypatch.setattr(A.PCTransformerFunction, "backward", staticmethod(lambda ctx, g: (n_pct.append(1), real_pct(ctx, g))[1]))
    with torch.no_grad():
        y_ng = occ(c["pc"], c["x0"], c["vq"], perms=c["perms"])
    x = c["x0"].clone().requires_grad_(True)
    v = c["vq"].clone().requires_grad_(True)
    occ.zero_grad(set_to_none=True)
    y = occ(c["pc"], x, v, perms=c["perms"])
    assert y.grad_fn is not None and torch.equal(y.detach(), y_ng)
    y.sum().backward(retain_graph=True)
    assert len(n_bwd) == 1 and not n_comp and not n_pct
    first = ({n: q.grad.clone() for n, q in occ.named_parameters()}, x.grad.clone(), v.grad.clone(), None)
    _check(f"scone_occ hip B={B}", first, c)
    occ.zero_grad(set_to_none=True)
    x.grad = v.grad = None
    y.sum().backward()
    again = ({n: q.grad.clone() for n, q in occ.named_parameters()}, x.grad.clone(), v.grad.clone(), None)
    assert _same(first, again)
    y = occ(c["pc"], x, v, perms=c["perms"])
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(y.sum(), [x] + list(occ.parameters()), create_graph=True)
    assert not n_comp and not n_pct


# ---- 3. chunks: a tail chunk and a cloud change between chunks ----------------------------------------------------------------------
def test_chunks(dev, cases):
    from macarons_amd import ops
    c = cases(2)
    occ = c["occ"]
    whole = _table_call(c)
    got = _table_call(c, q_chunk=32)                 # 50 queries per cloud: 32 + 18 rows, twice
    again = _table_call(c, q_chunk=32)
    assert all(torch.equal(a, b) for a, b in zip(got[0], again[0])) and torch.equal(got[1], again[1]) and torch.equal(got[2], again[2])
    _check("scone_occ hip q_chunk=32", (_by_name(occ, got[0]), got[1], got[2]), c)
    ew, ez = _between(_by_name(occ, got[0]), _by_name(occ, whole[0]))
    ex, ev = err(got[1], whole[1]), err(got[2], whole[2])
    print(f"ERR scone_occ hip q_chunk=32 vs q_chunk=0: params max {ew:.2e} (zero gradients, floored: {ez:.2e})  d_x {ex:.2e}  d_vh {ev:.2e}")
    assert max(ew, ez, ex, ev) < NET_TOL
    assert ops.scone_occ_backward_chunk(10 ** 6) == ops.pc_transformer_backward_chunk(10 ** 6, 16)
    assert ops.scone_occ_backward_chunk(50) == 50


# ---- 4. the default chunk's boundary, HIP against HIP: the staging ---------------------------------------------------------------------
def test_default_chunk_boundary(dev):
    from macarons_amd import ops
    chunk = ops.scone_occ_backward_chunk(10 ** 6)
    Q = chunk + 3
    occ = P._occ(dev)
    torch.manual_seed(5)
    dp = [p.to(dev) for p in occ.draw_perms(300)]
    rng = np.random.default_rng(61)
    pc = T(rng.uniform(-.3, .3, (1, 300, 3)), dev)
    x = T(rng.uniform(-.4, .4, (1, Q, 3)), dev)
    vq = T(rng.standard_normal((1, Q, 64)) * 0.3, dev)
    g = T(rng.standard_normal((1, Q, 1)), dev)
    scales = [pc, pc[:, dp[1]].contiguous()]
    scales.append(scales[1][:, dp[2]].contiguous())
    idx = [ops.knn_points(x, s_, 16)[2] for s_ in scales]
    call = lambda qc: ops.scone_occ_backward(pc[:, dp[0]].contiguous(), scales, x, vq, idx, g, occ.weight_table(), q_chunk=qc)
    two, one, again = call(0), call((Q + 15) // 16 * 16), call(0)
    assert all(torch.equal(a, b) for a, b in zip(two[0], again[0])) and torch.equal(two[1], again[1]) and torch.equal(two[2], again[2])
    for t in list(two[0]) + list(one[0]) + [two[1], two[2], one[1], one[2]]:
        assert bool(torch.isfinite(t).all())
    ew, ez = _between(_by_name(occ, two[0]), _by_name(occ, one[0]))
    ex, ev = err(two[1], one[1]), err(two[2], one[2])
    print(f"ERR scone_occ hip Q={Q}: chunks of {chunk} + 3 vs one chunk: params max {ew:.2e} (zero gradients, floored: {ez:.2e})  "
          f"d_x {ex:.2e}  d_vh {ev:.2e}")
    assert max(ew, ez, ex, ev) < NET_TOL


# ---- 5. need ---------------------------------------------------------------------------------------------------------------------------
def test_need(dev, monkeypatch, cases):
    from macarons_amd import ops
    c = cases(2)
    full = _table_call(c)
    w_only, x_only, v_only = (_table_call(c, need=n) for n in ((True, False, False), (False, True, False), (False, False, True)))
    assert w_only[1] is None and w_only[2] is None and x_only[0] is None and x_only[2] is None and v_only[0] is None and v_only[1] is None
    assert len(full[0]) == 140 and all(torch.equal(a, b) for a, b in zip(full[0], w_only[0]))
    assert torch.equal(full[1], x_only[1]) and torch.equal(full[2], v_only[2])
    entered, real = [], ops.check
    monkeypatch.setattr(ops, "check", lambda rc, what: (entered.append(what), real(rc, what))[1])
    assert _table_call(c, need=(False, False, False)) == (None, None, None) and not entered
    _table_call(c, need=(False, False, True))
    assert entered == ["mcr_scone_occ_backward"]


# ---- 6. a gradient for the surface points: the `pct` route ----------------------------------------------------------------------------
def test_pc_gradient_falls_back_to_pct(dev, monkeypatch, cases):
    c = cases(1)
    # torch scatters the points' gradient with float atomics unless told otherwise: both runs take its deterministic kernels where it has them
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        monkeypatch.setenv("MCR_SCONE_OCC_BWD", "pct")
        pct = _grads(c, pc_grad=True)
        monkeypatch.setenv("MCR_SCONE_OCC_BWD", "hip")
        hip = _grads(c, pc_grad=True)
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    assert hip[3] is not None and _same(pct, hip)


# ---- 7. the other modes are what they were ------------------------------------------------------------------------------------------
def test_other_modes_untouched(dev, monkeypatch, cases):
    c = cases(1)
    t32 = c["t32"] + (None,)
    monkeypatch.delenv("MCR_SCONE_OCC_BWD", raising=False)
    assert _same(t32, _grads(c))
    monkeypatch.setenv("MCR_SCONE_OCC_BWD", "composite")
    assert _same(t32, _grads(c))


# ---- 8. refusals through the C ABI ------------------------------------------------------------------------------------------------------
def test_refusals(dev, cases):
    from macarons_amd import _lib
    L = _lib.lib()
    who = "mcr_scone_occ_backward"
    c = cases(1)
    occ = c["occ"]
    B, Q, Lg = 1, 50, 300                               # (the 300-point cloud: the global sequence is all of it)
    pcg = c["pc"][:, c["dp"][0]].contiguous()
    assert pcg.shape[1] == Lg
    tab = occ.weight_table()
    FILL = 7.25
    d_w = [torch.full(tuple(t.shape), FILL, device=dev) for t in tab]
    d_x, d_v = torch.full((B, Q, 3), FILL, device=dev), torch.full((B, Q, 64), FILL, device=dev)
    g = torch.ones(B, Q, 1, device=dev)
    nb = int(L.mcr_scone_occ_backward_workspace_bytes(I64(B), I64(Q), I64(Lg), I64(0)))
    assert nb > 0 and nb == int(L.mcr_scone_occ_backward_workspace_bytes(I64(B), I64(Q), I64(Lg), I64(64)))   # (a chunk is capped at Q)
    assert int(L.mcr_scone_occ_backward_workspace_bytes(I64(B), I64(10 ** 5), I64(Lg), I64(0))) == \
        int(L.mcr_scone_occ_backward_workspace_bytes(I64(B), I64(10 ** 6), I64(Lg), I64(0)))                    # does not grow with Q
    ws = torch.full((nb + 64,), 93, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    ptr = lambda t: VP(t.data_ptr()) if t is not None else VP(None)

    def call(pc_global=pcg, scales=c["scales"], M=None, x=c["x0"], vh=c["vq"], idx=c["idx"], d_out=g, n_tab=len(tab), dw=d_w, dx=d_x,
             dv=d_v, q_chunk=0, B_=B, Q_=Q, wsp=ws.data_ptr(), n_bytes=nb):
        sc = (VP * 3)(*[p.data_ptr() if p is not None else None for p in scales])
        ms = (I64 * 3)(*(M or [p.shape[1] for p in c["scales"]]))
        ix = (VP * 3)(*[t.data_ptr() if t is not None else None for t in idx])
        wt = (VP * len(tab))(*[t.data_ptr() for t in tab])
        dt = (VP * len(dw))(*[t.data_ptr() if t is not None else None for t in dw]) if dw is not None else VP(None)
        return L.mcr_scone_occ_backward(ptr(pc_global), I64(Lg), sc, ms, ptr(x), ptr(vh), ix, ptr(d_out), I64(B_), I64(Q_), wt, CI(n_tab),
                                        dt, ptr(dx), ptr(dv), I64(q_chunk), VP(wsp), SZ(n_bytes), VP(torch.cuda.current_stream().cuda_stream))

    def refused(rc, what, needle):
        torch.cuda.synchronize()
        msg = L.mcr_last_error().decode()
        assert rc != 0, f"{what}: the call must be refused; it returned 0"
        assert who in msg and needle in msg, f"{what}: message {msg!r} lacks {who!r} or {needle!r}"
        for t in d_w + [d_x, d_v]:
            assert bool((t == FILL).all()), f"{what}: an output of a refused call was written"
        assert bool((ws == 93).all()), f"{what}: the workspace of a refused call was written"
        print(f"REFUSED {what}")

    off1 = lambda t: torch.cat((t.reshape(-1)[:1], t.reshape(-1)))[1:]                  # the same values, one element off the 16-byte grid
    refused(call(pc_global=None), "pc_global NULL", "null pointer")
    refused(call(x=None), "x NULL", "null pointer")
    refused(call(vh=None), "view_harmonics NULL", "null pointer")
    refused(call(d_out=None), "d_out NULL", "null pointer")
    refused(call(scales=[c["scales"][0], None, c["scales"][2]]), "pc_scale[1] NULL", "null pointer")
    refused(call(idx=[c["idx"][0], c["idx"][1], None]), "knn_idx[2] NULL", "null pointer")
    refused(call(dw=d_w[:77] + [None] + d_w[78:]), "d_weights[77] NULL", "d_weights[77] is null")
    refused(call(n_tab=139), "139 weights", "expected 140 weight pointers")
    refused(call(Q_=0), "Q = 0", "bad problem size")
    refused(call(B_=0), "B = 0", "bad problem size")
    refused(call(M=[300, 15, 16]), "M_scale[1] = 15", "< k = 16")
    for qc in (8, 40, -16):
        refused(call(q_chunk=qc), f"q_chunk = {qc}", "q_chunk must be")
    refused(call(x=off1(c["x0"])), "x off the 16-byte grid", "16-byte aligned")
    refused(call(dv=off1(d_v)), "d_view_harmonics off the 16-byte grid", "16-byte aligned")
    refused(call(idx=[c["idx"][0], off1(c["idx"][1]), c["idx"][2]]), "knn_idx[1] off the 16-byte grid (by 8 bytes)", "16-byte aligned")
    refused(call(scales=[c["scales"][0], c["scales"][1], off1(c["scales"][2])]), "pc_scale[2] off the 16-byte grid", "16-byte aligned")
    refused(call(wsp=ws.data_ptr() + 4, n_bytes=nb + 32), "workspace off the 16-byte grid", "16-byte aligned")
    refused(call(n_bytes=nb - 4), f"{nb - 4} bytes of workspace", "workspace too small")
    refused(call(wsp=None), "workspace NULL", "workspace too small")
    rc = call(dw=None, dx=None, dv=None)                # nothing asked: returns 0 at once
    torch.cuda.synchronize()
    assert rc == 0 and bool((ws == 93).all())
    rc = call()                                         # and the accepted call, in exactly the stated bytes
    torch.cuda.synchronize()
    assert rc == 0, L.mcr_last_error().decode()
    assert bool((ws[nb:] == 93).all())
    full = _table_call(c)
    assert all(torch.equal(a, b) for a, b in zip(d_w, full[0])) and torch.equal(d_x, full[1]) and torch.equal(d_v, full[2])
