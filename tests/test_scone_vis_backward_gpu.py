"""SconeVis HIP backward (scone_vis_bwd.hip: mcr_scone_vis_backward; its building blocks: bwd_blocks.hip, attention_bwd.hip) against fp64 torch autograd on the GPU,
the fp64 composite (autograd.scone_vis) and the reference's own fp64 gradients (scone_vis_grad*.npz, make_golden_scone_vis_grad.py).
Errors are max |got - ref| / max |ref| per tensor; parameter denominators are floored at 1e-4 x the largest parameter gradient
(w_k.bias has a mathematically zero gradient).  Measured errors are printed with an ERR prefix."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import weights  # noqa: E402
import make_golden_scone_vis_grad as G  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK_TOL = 2e-5
NET_TOL = 1e-4
# w_k.bias: its gradient is mathematically zero (softmax ignores a constant added to every key's score); what fp32 leaves there is
# rounding noise of sums of O(|dK|) terms, measured up to 3.1e-7 x the largest parameter gradient at 1 x 2048 -- bounded absolutely
ZERO_GRAD = "mhsa.w_k.bias"
ZERO_TOL = 2e-6


def _vis(dev, seed=1):
    from macarons_amd.networks import SconeVis
    m = SconeVis()
    sd = weights.make_state_dict(weights.shapes_of(m), seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(dev)


def T(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype)


def err(got, ref, floor=0.0):
    got = got.detach().double().cpu() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got, np.float64))
    ref = ref.detach().double().cpu() if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref, np.float64))
    return float((got - ref).abs().max() / max(float(ref.abs().max()), floor, 1e-30))


def hip_grads(m, pts, vh, g, lengths=None):
    """(param grads by name, d_pts, d_vh) through SconeVis.forward's autograd path (the HIP backward)."""
    p = pts.clone().requires_grad_(True)
    v = vh.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(p, view_harmonics=v, lengths=lengths)
    (y * g).sum().backward()
    return {n: q.grad.clone() for n, q in m.named_parameters()}, p.grad.clone(), v.grad.clone()


def _double(m):
    """A float64 copy of m (same parameters) for the composite."""
    from macarons_amd.networks import SconeVis
    md = SconeVis()
    md.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    return md.to(next(m.parameters()).device).double()


def composite_grads(m, pts, vh, g, lengths=None):
    """The same gradients through the fp64 composite (autograd.scone_vis on a float64 copy of the module)."""
    from macarons_amd import autograd as A
    md = _double(m)
    p = pts.double().requires_grad_(True)
    v = vh.double().requires_grad_(True)
    y = A.scone_vis(md, p, v, lengths)
    (y * g.double()).sum().backward()
    return {n: q.grad for n, q in md.named_parameters()}, p.grad, v.grad


def compare(tag, got, ref, tol):
    gp, gx, gv = got
    rp, rx, rv = ref
    scale = max(float(t.abs().max()) for t in rp.values())
    worst = 0.0
    for n in rp:
        if n.endswith(ZERO_GRAD):
            e = float((gp[n].double().cpu() - rp[n].double().cpu()).abs().max()) / scale
            print(f"ERR {tag}: {n} (zero gradient) {e:.2e} x the largest")
            assert e < ZERO_TOL, (tag, n, e)
            continue
        e = err(gp[n], rp[n], 1e-4 * scale)
        worst = max(worst, e)
        assert e < tol, (tag, n, e)
    ex, ev = err(gx, rx), err(gv, rv)
    print(f"ERR {tag}: params max {worst:.2e}  d_pts {ex:.2e}  d_vh {ev:.2e}")
    assert ex < tol and ev < tol, (tag, ex, ev)
    return max(worst, ex, ev)


# ---- 1. building blocks against fp64 torch autograd ---------------------------------------------------------------------------------
def _attn_ref(qkv, g, lens):
    S, L, _ = qkv.shape
    q, k, v = qkv[..., :64], qkv[..., 64:128], qkv[..., 128:]
    q = q.view(S, L, 4, 16).transpose(1, 2)
    k = k.view(S, L, 4, 16).transpose(1, 2)
    v = v.view(S, L, 4, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / 4.0
    if lens is not None:
        s = s.masked_fill(torch.arange(L, device=qkv.device)[None, None, None, :] >= lens.clamp(min=1).view(-1, 1, 1, 1).long(), float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(S, L, 256)
    (o * g).sum().backward()


@pytest.mark.parametrize("S,L", [(1, 2048), (4, 2048), (3, 333), (2, 17)])     # (4, 2048): enough blocks, no key / query split
@pytest.mark.parametrize("with_lens", [False, True])
def test_attention_backward(dev, S, L, with_lens):
    from macarons_amd import ops
    rng = np.random.default_rng(S * 1000 + L)
    qkv = T(rng.standard_normal((S, L, 384)), dev)
    g = T(rng.standard_normal((S, L, 256)), dev)
    lens = None
    if with_lens:
        lens = torch.tensor(([1] + [max(1, L // 2 - 3)] * (S - 1))[:S] if S > 1 else [L // 3], dtype=torch.int32, device=dev)
    got = ops.attention_backward(qkv, g, 4, lens)
    qd = qkv.double().requires_grad_(True)
    _attn_ref(qd, g.double(), lens)
    ref = qd.grad
    if lens is not None:            # keys beyond the length: zero gradient (torch gives exact zeros there as well)
        for s in range(S):
            n = int(lens[s])
            assert torch.count_nonzero(got[s, n:, 64:]) == 0
    e = [err(got[..., a:b], ref[..., a:b]) for a, b in ((0, 64), (64, 128), (128, 384))]
    print(f"ERR attention S={S} L={L} lens={with_lens}: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < BLOCK_TOL, e


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_linear_backward(dev, gelu, accumulate):
    from macarons_amd import ops
    rng = np.random.default_rng(5 + gelu + 2 * accumulate)
    M, N, K = 777, 192, 126
    x = T(rng.standard_normal((M, K)), dev)
    w = T(rng.standard_normal((N, K)) / np.sqrt(K), dev)
    b = T(rng.standard_normal(N) * 0.1, dev)
    g = T(rng.standard_normal((M, N)), dev)
    z = x @ w.t() + b
    base = T(rng.standard_normal((M, K)), dev) if accumulate else None
    d_x = base.clone() if accumulate else None
    dx, dw, db = ops.linear_backward(x, w, g, z=z if gelu else None, gelu=gelu, d_x=d_x)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = torch.nn.functional.linear(xd, wd, bd)
    if gelu:
        y = torch.nn.functional.gelu(y)
    (y * g.double()).sum().backward()
    rx = xd.grad + (base.double() if accumulate else 0)
    e = (err(dx, rx), err(dw, wd.grad), err(db, bd.grad))
    print(f"ERR linear gelu={gelu} acc={accumulate}: dx {e[0]:.2e} dw {e[1]:.2e} db {e[2]:.2e}")
    assert max(e) < BLOCK_TOL, e


@pytest.mark.parametrize("E", [64, 128, 256, 512])
def test_layernorm_backward(dev, E):
    from macarons_amd import ops
    rng = np.random.default_rng(9 + E)
    M = 1000
    x = T(rng.standard_normal((M, E)) * 2 + 0.5, dev)
    gm = T(1 + 0.1 * rng.standard_normal(E), dev)
    bt = T(0.05 * rng.standard_normal(E), dev)
    g = T(rng.standard_normal((M, E)), dev)
    base = T(rng.standard_normal((M, E)), dev)
    for acc in (False, True):
        dx, dg, db = ops.layernorm_backward(x, gm, g, d_x=base.clone() if acc else None)
        xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gm, bt))
        (torch.nn.functional.layer_norm(xd, (E,), gd, bd, 1e-5) * g.double()).sum().backward()
        rx = xd.grad + (base.double() if acc else 0)
        e = (err(dx, rx), err(dg, gd.grad), err(db, bd.grad))
        print(f"ERR layernorm E={E} acc={acc}: dx {e[0]:.2e} dgamma {e[1]:.2e} dbeta {e[2]:.2e}")
        assert max(e) < BLOCK_TOL, e


def test_colmax_backward_ties_go_to_lowest_row(dev):
    from macarons_amd import ops
    rng = np.random.default_rng(11)
    S, L, E = 2, 300, 126
    x = rng.standard_normal((S, L, E)).astype(np.float32)
    x[0, 7, 3] = x[0, 250, 3] = 10.0            # a deliberate tie: row 7 must win
    x[1, 40, 5] = x[1, 20, 5] = 9.0             # row 20 must win
    x[1, 200, 6] = 50.0                         # beyond the length of cloud 1: ignored
    lens = torch.tensor([L, 150], dtype=torch.int32, device=dev)
    g = T(rng.standard_normal((S, L, E)), dev)
    base = T(rng.standard_normal((S, L, E)), dev)
    got = ops.colmax_backward(T(x, dev), g, base.clone(), lens)
    xd = T(x, dev, torch.float64).requires_grad_(True)
    valid = torch.arange(L, device=dev)[None, :, None] < lens.view(-1, 1, 1)
    r = torch.where(valid, xd, torch.full_like(xd, float("-inf")))
    (r.max(dim=1, keepdim=True)[0].expand_as(xd) * g.double()).sum().backward()
    ref = xd.grad + base.double()
    e = err(got, ref)
    print(f"ERR colmax: {e:.2e}")
    assert e < BLOCK_TOL
    tot = g.double().sum(1)
    assert abs(float(got[0, 7, 3] - base[0, 7, 3]) - float(tot[0, 3])) < 1e-4 and float(got[0, 250, 3] - base[0, 250, 3]) == 0.0
    assert abs(float(got[1, 20, 5] - base[1, 20, 5]) - float(tot[1, 5])) < 1e-4 and float(got[1, 40, 5] - base[1, 40, 5]) == 0.0
    assert float(got[1, 200, 6] - base[1, 200, 6]) == 0.0


# ---- 2. whole network: against the reference fixture and the fp64 composite ----------------------------------------------------------
def _case_inputs(case, dev):
    src = golden("scone_vis")
    kp, kv = G.CASES[case]
    pts, vh = T(src[kp], dev), T(src[kv], dev)
    return pts, vh, T(G.upstream(case, tuple(vh.shape)), dev)


def _fixture(case):
    return golden("scone_vis_grad_2048" if case == "2048" else "scone_vis_grad"), golden("scone_vis_grad")


def _check_fixture(tag, case, got, tol):
    fx, idx_src = _fixture(case)
    gp, gx, gv = got
    scale = 0.0
    for n in gp:
        scale = max(scale, float(fx[f"m_{case}_{n}"]) if f"m_{case}_{n}" in fx else float(np.abs(fx[f"g_{case}_{n}"]).max()))
    worst = 0.0
    for n, t in gp.items():
        a = t.detach().double().cpu().numpy()
        if f"s_{case}_{n}" in fx:
            ref = fx[f"s_{case}_{n}"].astype(np.float64)
            a = a.reshape(-1)[idx_src[f"idx_{n}"]]
            den = max(float(fx[f"m_{case}_{n}"]), 1e-4 * scale)
        else:
            ref = fx[f"g_{case}_{n}"].astype(np.float64)
            den = max(float(np.abs(ref).max()), 1e-4 * scale)
        if n.endswith(ZERO_GRAD):
            e = float(np.abs(a - ref).max()) / scale
            assert e < ZERO_TOL, (tag, n, e)
            continue
        e = float(np.abs(a - ref).max() / den)
        worst = max(worst, e)
        assert e < tol, (tag, n, e)
    ex, ev = err(gx, fx[f"d_pts_{case}"]), err(gv, fx[f"d_vh_{case}"])
    print(f"ERR {tag} vs fixture: params max {worst:.2e}  d_pts {ex:.2e}  d_vh {ev:.2e}")
    assert ex < tol and ev < tol, (tag, ex, ev)


@pytest.mark.parametrize("variant", [6, 7])
@pytest.mark.parametrize("case", ["333", "b3", "2048"])
def test_network_against_fixture_and_composite(dev, case, variant):
    from macarons_amd import ops
    m = _vis(dev)
    pts, vh, g = _case_inputs(case, dev)
    with ops.variant(variant):
        got = hip_grads(m, pts, vh, g)
    _check_fixture(f"{case} v{variant}", case, got, NET_TOL)
    compare(f"{case} v{variant} vs composite", got, composite_grads(m, pts, vh, g), NET_TOL)


def test_network_small_batch_against_composite(dev):
    m = _vis(dev)
    rng = np.random.default_rng(21)
    pts = T(np.concatenate([rng.uniform(-.5, .5, (2, 60, 3)), rng.uniform(.1, 1, (2, 60, 1))], -1), dev)
    vh = T(rng.standard_normal((2, 60, 64)) * 0.3, dev)
    g = T(rng.standard_normal((2, 60, 64)), dev)
    compare("2x60", hip_grads(m, pts, vh, g), composite_grads(m, pts, vh, g), NET_TOL)


# ---- 3. no composite anywhere in the pretraining step ----------------------------------------------------------------------------------
def test_pretraining_step_without_composite(dev, monkeypatch):
    from macarons_amd import autograd as A
    from macarons_amd.networks.SconeVis import L1_loss
    m = _vis(dev)
    pts, vh, _ = _case_inputs("2048", dev)
    rng = np.random.default_rng(3)
    cams = T(rng.standard_normal((1, 9, 3)) * 2, dev)
    target = T(rng.uniform(0, 1, (1, 9)), dev)
    with torch.no_grad():
        y_ng = m(pts, view_harmonics=vh)

    def chain(p, v, net):
        h = net(p, v)
        gain = m.compute_coverage_gain(p, h, cams)
        return L1_loss()(gain, target)

    # the reference: the same chain through the fp64 composite and the scorer's torch composite
    md = _double(m)
    p64, v64 = pts.double().requires_grad_(True), vh.double().requires_grad_(True)
    h64 = A.scone_vis(md, p64, v64)
    L1_loss()(A.coverage_gain(p64, h64, cams.double()), target.double()).backward()
    ref = ({n: q.grad for n, q in md.named_parameters()}, p64.grad, v64.grad)

    def boom(*a, **k):
        raise AssertionError("the composite SconeVis backward ran")
    monkeypatch.setattr(A, "scone_vis", boom)
    p, v = pts.clone().requires_grad_(True), vh.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    h = m(p, view_harmonics=v)
    assert torch.equal(h.detach(), y_ng)                     # the forward under autograd: the no-grad bits
    L1_loss()(m.compute_coverage_gain(p, h, cams), target).backward()
    compare("pretraining step", ({n: q.grad for n, q in m.named_parameters()}, p.grad, v.grad), ref, NET_TOL)


# ---- 4. padded batch ----------------------------------------------------------------------------------------------------------------
def test_padded_batch_equals_sliced_clouds(dev):
    m = _vis(dev)
    rng = np.random.default_rng(8)
    B, N, lens = 3, 120, [120, 77, 1]
    pts = T(np.concatenate([rng.uniform(-.5, .5, (B, N, 3)), rng.uniform(.1, 1, (B, N, 1))], -1), dev)
    vh = T(rng.standard_normal((B, N, 64)) * 0.3, dev)
    g = T(rng.standard_normal((B, N, 64)), dev)
    for b, n in enumerate(lens):
        g[b, n:] = 0
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev)
    gp, gx, gv = hip_grads(m, pts, vh, g, lengths)
    acc = {n: torch.zeros_like(t) for n, t in gp.items()}
    rx, rv = torch.zeros_like(gx), torch.zeros_like(gv)
    for b, n in enumerate(lens):
        p_, x_, v_ = hip_grads(m, pts[b:b + 1, :n], vh[b:b + 1, :n], g[b:b + 1, :n])
        for k in acc:
            acc[k] += p_[k]
        rx[b, :n], rv[b, :n] = x_[0], v_[0]
    compare("padded batch", (gp, gx, gv), (acc, rx, rv), NET_TOL)


# ---- 5. trainer pattern: per-sample forwards, one summed loss, one backward ----------------------------------------------------------
def test_summed_loss_equals_sum_of_backwards(dev):
    m = _vis(dev)
    rng = np.random.default_rng(12)
    xs = [(T(np.concatenate([rng.uniform(-.5, .5, (1, n, 3)), rng.uniform(.1, 1, (1, n, 1))], -1), dev),
           T(rng.standard_normal((1, n, 64)) * 0.3, dev), T(rng.standard_normal((1, n, 64)), dev)) for n in (90, 130, 64)]
    m.zero_grad(set_to_none=True)
    loss = sum((m(p, view_harmonics=v) * g).sum() for p, v, g in xs)
    loss.backward()
    got = {n: q.grad.clone() for n, q in m.named_parameters()}
    ref = {n: torch.zeros_like(t) for n, t in got.items()}
    for p, v, g in xs:
        gp, _, _ = hip_grads(m, p, v, g)
        for k in ref:
            ref[k] += gp[k]
    scale = max(float(t.abs().max()) for t in ref.values())
    e = max(err(got[n], ref[n], 1e-4 * scale) for n in ref)
    print(f"ERR summed loss: {e:.2e}")
    assert e < 1e-5


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------
def test_backward_is_deterministic(dev):
    from macarons_amd import ops
    m = _vis(dev)
    pts, vh, g = _case_inputs("2048", dev)
    tab = m._table_cache.get(m, m.weight_table_with_planes)
    a = ops.scone_vis_backward(pts, vh, g, tab)
    b = ops.scone_vis_backward(pts, vh, g, tab)
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert torch.equal(x, y)


# ---- 7. peak memory ---------------------------------------------------------------------------------------------------------------
def test_backward_peak_memory(dev, monkeypatch):
    m = _vis(dev)
    pts, vh, _ = _case_inputs("2048", dev)
    B = 4
    pts, vh = pts.expand(B, -1, -1).contiguous(), vh.expand(B, -1, -1).contiguous()
    g = T(np.random.default_rng(4).standard_normal((B, 2048, 64)), dev)

    def rise():
        p = pts.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        y = m(p, view_harmonics=vh)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        (y * g).sum().backward()
        torch.cuda.synchronize(dev)
        return (torch.cuda.max_memory_allocated(dev) - base) / 2**20

    from macarons_amd import ops
    ops._ws_cache.clear()
    hip = rise()
    monkeypatch.setenv("MCR_SCONE_VIS_BWD", "composite")
    comp = rise()
    print(f"ERR peak memory rise during backward at {B}x2048: HIP {hip:.1f} MB ({hip / B:.1f} per cloud), composite {comp:.1f} MB")
    assert hip / B <= 96.0


# ---- 8. once only -------------------------------------------------------------------------------------------------------------------
def test_create_graph_raises(dev):
    m = _vis(dev)
    pts, vh, g = _case_inputs("333", dev)
    y = m(pts, view_harmonics=vh)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad((y * g).sum(), list(m.parameters()), create_graph=True)
