"""PCTransformer HIP backward (pct_bwd.hip: mcr_pc_transformer_backward; attention_bwd.hip: mcr_attention_backward_pct; bwd_blocks.hip: mcr_pool_max_avg_backward)
against fp64 torch autograd on the GPU, the fp64 composite (autograd.pc_transformer) and the reference's own fp64 gradients
(pct_grad.npz, make_golden_pct_grad.py).  Errors are max |got - ref| / max |ref| per tensor; parameter denominators are floored at
1e-4 x the largest parameter gradient.  mhsa.w_k.bias has a mathematically zero gradient: it is bounded absolutely, at 2e-6 x the
largest parameter gradient or 4 x what the fp32 torch composite leaves there on the same inputs, whichever is larger.  Measured errors
are printed with an ERR prefix."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import weights  # noqa: E402
import make_golden_pct_grad as G  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK_TOL = 2e-5
NET_TOL = 1e-4
ZERO_GRAD = "mhsa.w_k.bias"
ZERO_TOL = 2e-6


def T(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dtype)


def err(got, ref, floor=0.0):
    got = got.detach().double().cpu() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got, np.float64))
    ref = ref.detach().double().cpu() if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref, np.float64))
    return float((got - ref).abs().max() / max(float(ref.abs().max()), floor, 1e-30))


def _pct(dev, L=16, feature_dim=256, dtype=torch.float32):
    from macarons_amd.networks.SconeOcc import PCTransformer
    m = PCTransformer(seq_len=L, pts_embedding_dim=128, feature_dim=feature_dim)
    sd = weights.make_state_dict(weights.shapes_of(m), G.WEIGHT_SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(device=dev, dtype=dtype)


def _copy(m, dtype):
    """A copy of m (same parameters) in another precision, for the composites."""
    from macarons_amd.networks.SconeOcc import PCTransformer
    c = PCTransformer(seq_len=m.seq_len, pts_embedding_dim=128, feature_dim=m.feature_dim)
    c.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    return c.to(device=next(m.parameters()).device, dtype=dtype)


def hip_grads(m, pc, g):
    """(param grads by name, d_pc) through PCTransformer.forward's autograd path (the HIP backward)."""
    p = pc.detach().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(p)
    (y * g).sum().backward()
    return {n: q.grad.clone() for n, q in m.named_parameters()}, p.grad.clone()


def composite_grads(m, pc, g, dtype=torch.float64):
    """The same gradients through the composite (autograd.pc_transformer) on a copy of the module in `dtype`."""
    from macarons_amd import autograd as A
    md = _copy(m, dtype)
    p = pc.detach().to(dtype, copy=True).requires_grad_(True)
    (A.pc_transformer(md, p) * g.to(dtype)).sum().backward()
    return {n: q.grad for n, q in md.named_parameters()}, p.grad


def compare(tag, got, ref, tol, fp32=None, d_pc=True):
    """fp32: the fp32 torch composite's gradients on the same inputs (the yardstick of the zero gradient's noise)."""
    gp, gx = got
    rp, rx = ref
    scale = max(float(t.abs().max()) for t in rp.values())
    worst = 0.0
    for n in rp:
        if n.endswith(ZERO_GRAD):
            e = float((gp[n].double().cpu() - rp[n].double().cpu()).abs().max()) / scale
            e32 = float((fp32[0][n].double().cpu() - rp[n].double().cpu()).abs().max()) / scale if fp32 is not None else 0.0
            print(f"ERR {tag}: {n} (zero gradient) {e:.2e} x the largest (fp32 composite: {e32:.2e})")
            assert e < max(ZERO_TOL, 4 * e32), (tag, n, e, e32)
            continue
        e = err(gp[n], rp[n], 1e-4 * scale)
        worst = max(worst, e)
        assert e < tol, (tag, n, e)
    ex = err(gx, rx) if d_pc else 0.0
    print(f"ERR {tag}: params max {worst:.2e}  d_pc {ex:.2e}")
    assert ex < tol, (tag, ex)


# ---- 1. attention block, widths (8, 32) -------------------------------------------------------------------------------------------
def _attn_ref(qkv, g, lens):
    S, L, _ = qkv.shape
    q = qkv[..., :32].view(S, L, 4, 8).transpose(1, 2)
    k = qkv[..., 32:64].view(S, L, 4, 8).transpose(1, 2)
    v = qkv[..., 64:].view(S, L, 4, 32).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / np.sqrt(8.0)
    if lens is not None:
        s = s.masked_fill(torch.arange(L, device=qkv.device)[None, None, None, :] >= lens.clamp(min=1).view(-1, 1, 1, 1).long(), float("-inf"))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(S, L, 128)
    (o * g).sum().backward()


ATTN_CASES = [(1, 16), (5, 16), (1031, 16), (65537, 16), (2, 17), (3, 333), (1, 2048), (4, 2048)]


@pytest.mark.parametrize("S,L", ATTN_CASES)
def test_attention_backward_pct(dev, S, L):
    from macarons_amd import ops
    rng = np.random.default_rng(S * 1000 + L)
    qkv = T(rng.standard_normal((S, L, 192), dtype=np.float32), dev)
    g = T(rng.standard_normal((S, L, 128), dtype=np.float32), dev)
    for with_lens in ((False,) if L == 16 else (False, True)):
        lens = None
        if with_lens:
            lens = torch.tensor(([1] + [max(1, L // 2 - 3)] * (S - 1))[:S] if S > 1 else [L // 3], dtype=torch.int32, device=dev)
        got = ops.attention_backward_pct(qkv, g, lens)
        qd = qkv.double().requires_grad_(True)
        _attn_ref(qd, g.double(), lens)
        ref = qd.grad
        if lens is not None:            # keys beyond the length: exact zeros
            for s in range(S):
                assert torch.count_nonzero(got[s, int(lens[s]):, 32:]) == 0
        e = [err(got[..., a:b], ref[..., a:b]) for a, b in ((0, 32), (32, 64), (64, 192))]
        print(f"ERR attention_pct S={S} L={L} lens={with_lens}: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
        assert max(e) < BLOCK_TOL, e


def test_attention_backward_pct_refuses_lens_on_16_tokens(dev):
    from macarons_amd import ops, _lib
    qkv, g = torch.randn(3, 16, 192, device=dev), torch.randn(3, 16, 128, device=dev)
    with pytest.raises(_lib.MacaronsHipError, match="take no lens"):
        ops.attention_backward_pct(qkv, g, torch.full((3,), 9, dtype=torch.int32, device=dev))


# ---- 2. pool backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("L", [16, 150])
@pytest.mark.parametrize("E", [128, 256])
def test_pool_max_avg_backward(dev, S, L, E):
    from macarons_amd import ops
    rng = np.random.default_rng(S * 100000 + L * 1000 + E)
    x = T(rng.standard_normal((S, L, E)), dev)
    g = T(rng.standard_normal((S, 2 * E)), dev)
    got = ops.pool_max_avg_backward(x, g)
    xd = x.double().requires_grad_(True)
    (torch.cat((xd.max(dim=1)[0], xd.mean(dim=1)), dim=-1) * g.double()).sum().backward()
    e = err(got, xd.grad)
    print(f"ERR pool S={S} L={L} E={E}: {e:.2e}")
    assert e < BLOCK_TOL


def test_pool_max_avg_backward_ties_go_to_the_lower_row(dev):
    from macarons_amd import ops
    rng = np.random.default_rng(11)
    S, L, E = 2, 150, 128
    x = rng.standard_normal((S, L, E)).astype(np.float32)
    x[0, 140] = x[0, 7] = 10.0 + np.arange(E, dtype=np.float32)     # two identical rows hold every column's maximum: row 7 wins
    x[1, 20, 5] = x[1, 40, 5] = 9.0
    g = rng.standard_normal((S, 2 * E)).astype(np.float32)
    got = ops.pool_max_avg_backward(T(x, dev), T(g, dev)).cpu().numpy()
    avg = g[:, None, E:] / np.float32(L)
    assert np.allclose(got[0, 140], avg[0, 0], rtol=1e-6, atol=1e-9) and np.allclose(got[0, 7], avg[0, 0] + g[0, :E], rtol=1e-6, atol=1e-7)
    assert abs(got[1, 40, 5] - avg[1, 0, 5]) < 1e-8 and abs(got[1, 20, 5] - (avg[1, 0, 5] + g[1, 5])) < 1e-6
    xd = T(x, dev, torch.float64).requires_grad_(True)
    (torch.cat((xd.max(dim=1)[0], xd.mean(dim=1)), dim=-1) * T(g, dev, torch.float64)).sum().backward()
    assert err(got, xd.grad) < BLOCK_TOL            # torch.max(dim) makes the same choice


# ---- 3. the network against the fixture and the composite ---------------------------------------------------------------------------
def _check_fixture(tag, case, got, tol, zero_bound):
    fx = golden("pct_grad")
    gp, gx = got
    scale = max(float(fx[f"m_{case}_{n}"]) if f"m_{case}_{n}" in fx else float(np.abs(fx[f"g_{case}_{n}"]).max()) for n in gp)
    worst = 0.0
    for n, t in gp.items():
        a = t.detach().double().cpu().numpy()
        if f"s_{case}_{n}" in fx:
            ref = fx[f"s_{case}_{n}"]
            a = a.reshape(-1)[fx[f"idx_{case}_{n}"]]
            den = max(float(fx[f"m_{case}_{n}"]), 1e-4 * scale)
        else:
            ref = fx[f"g_{case}_{n}"]
            den = max(float(np.abs(ref).max()), 1e-4 * scale)
        if n.endswith(ZERO_GRAD):
            e = float(np.abs(a - ref).max()) / scale
            assert e < zero_bound, (tag, n, e)
            continue
        e = float(np.abs(a - ref).max() / den)
        worst = max(worst, e)
        assert e < tol, (tag, n, e)
    ex = err(gx, fx[f"d_pc_{case}"])
    print(f"ERR {tag} vs fixture: params max {worst:.2e}  d_pc {ex:.2e}")
    assert ex < tol, (tag, ex)


@pytest.fixture(scope="module")
def references(dev):
    """case -> (module, pc, upstream, fp64 composite gradients, fp32 composite gradients): computed once, shared, never changed."""
    out = {}

    def get(case):
        if case not in out:
            S, L, fd = G.CASES[case]
            m = _pct(dev, L, fd)
            pc, g = T(G.inputs(case), dev), T(G.upstream(case), dev)
            out[case] = (m, pc, g, composite_grads(m, pc, g), composite_grads(m, pc, g, torch.float32))
        return out[case]
    return get


@pytest.mark.parametrize("case", ["s16", "l150", "l2048"])
def test_network_against_fixture_and_composite(dev, case, references):
    from macarons_amd import ops
    m, pc, g, ref64, ref32 = references(case)
    got = {}
    for variant in (6, 7):
        with ops.variant(variant):
            got[variant] = hip_grads(m, pc, g)
        scale = max(float(t.abs().max()) for t in ref64[0].values())
        zero32 = max(float((ref32[0][n].double() - ref64[0][n]).abs().max()) / scale for n in ref64[0] if n.endswith(ZERO_GRAD))
        _check_fixture(f"{case} v{variant}", case, got[variant], NET_TOL, max(ZERO_TOL, 4 * zero32))
        compare(f"{case} v{variant} vs composite", got[variant], ref64, NET_TOL, ref32)
    for n in got[6][0]:                            # the fp32 network's gradient on every variant: the same bits
        assert torch.equal(got[6][0][n], got[7][0][n]), n
    assert torch.equal(got[6][1], got[7][1])
    # need = (params, pc): what overlaps agrees bit for bit
    tab = m.weight_table()
    both = ops.pc_transformer_backward(pc, g, tab, m.feature_dim, need=(True, True))
    w_only = ops.pc_transformer_backward(pc, g, tab, m.feature_dim, need=(True, False))
    p_only = ops.pc_transformer_backward(pc, g, tab, m.feature_dim, need=(False, True))
    assert w_only[1] is None and p_only[0] is None
    assert all(torch.equal(a, b) for a, b in zip(both[0], w_only[0])) and torch.equal(both[1], p_only[1])
    assert torch.equal(both[1], got[6][1])


def _worst(got, ref):
    """(largest parameter error but the zero gradient's, input error) in the metric of compare()."""
    scale = max(float(t.abs().max()) for t in ref[0].values())
    return max(err(got[0][n], ref[0][n], 1e-4 * scale) for n in ref[0] if not n.endswith(ZERO_GRAD)), err(got[1], ref[1])


# ---- 4. chunk boundary ------------------------------------------------------------------------------------------------------------
# The max's gradient goes to ONE row, and jumps to another where two rows of a column agree to within the forward's rounding: among
# the (2 chunk + 3) x 128 maxima of this test there are always a few such pairs, and whichever fp32 forward evaluates them (the fp32
# torch composite as well: 8 flips and 5e-4 on these inputs) then differentiates another branch than the fp64 reference.  That is
# a property of the function, not of a backward, so the upstream gradient of the max is set to zero wherever the reference's two
# largest rows lie closer than NEAR_TIE x the largest activation -- the flips sit below 1e-7, fp32's rounding; 1e-5 takes about three
# maxima in a thousand out (the tokens of a neighbourhood of offsets ~0.05 lie close together), after which the fp32 torch
# composite agrees with the reference to 3.1e-5 (parameters) and 7e-7 (points).
NEAR_TIE = 1e-5


def _near_ties(m, pc):
    """[S, half] bool: columns whose two largest rows nearly tie in the fp64 composite's activations in front of the pooling."""
    import torch.nn.functional as F
    from macarons_amd import autograd as A
    md = _copy(m, torch.float64)
    with torch.no_grad():
        x = A.embedding(md.embedding, pc.double())
        for enc in md.encoders:
            x = A.encoder(enc, x)
        y = F.linear(F.layer_norm(x, (x.shape[-1],), md.norm.weight, md.norm.bias), md.linear0.weight, md.linear0.bias)
        top = y.topk(2, dim=1)[0]
        return (top[:, 0] - top[:, 1]) < NEAR_TIE * y.abs().max()


def test_chunk_boundary_16_tokens(dev):
    from macarons_amd import ops
    chunk = ops.pc_transformer_backward_chunk(10 ** 6, 16)
    S = 2 * chunk + 3
    assert ops.pc_transformer_backward_chunk(S, 16) == chunk < S and ops.pc_transformer_backward_chunk(5, 150) == 5
    m = _pct(dev)
    rng = np.random.default_rng(44)
    pc = T(rng.uniform(-0.05, 0.05, (S, 16, 3)), dev)
    g = T(rng.standard_normal((S, 256)), dev)
    # the claim above, checked on every run: on the UNMASKED upstream gradient the fp32 torch composite misses the bound itself
    raw64, raw32 = composite_grads(m, pc, g), composite_grads(m, pc, g, torch.float32)
    raw = _worst(raw32, raw64)
    print(f"ERR chunks S={S}: unmasked, fp32 torch composite vs fp64: params max {raw[0]:.2e}  d_pc {raw[1]:.2e}")
    assert max(raw) > NET_TOL, raw
    ties = _near_ties(m, pc)
    assert 0 < int(ties.sum()) < 0.01 * ties.numel()
    g[:, :128][ties] = 0.0
    print(f"ERR chunks S={S}: {int(ties.sum())} of {ties.numel()} maxima nearly tied (no upstream gradient there)")
    masked = _worst(composite_grads(m, pc, g, torch.float32), composite_grads(m, pc, g))
    print(f"ERR chunks S={S}: masked, fp32 torch composite vs fp64: params max {masked[0]:.2e}  d_pc {masked[1]:.2e}")
    assert max(masked) < NET_TOL, masked
    got = hip_grads(m, pc, g)
    compare(f"chunks S={S}", got, composite_grads(m, pc, g), NET_TOL, composite_grads(m, pc, g, torch.float32))
    again = hip_grads(m, pc, g)
    assert all(torch.equal(got[0][n], again[0][n]) for n in got[0]) and torch.equal(got[1], again[1])


# ---- 5. a sequence with two identical points ---------------------------------------------------------------------------------------
def test_two_identical_points(dev):
    m = _pct(dev)
    rng = np.random.default_rng(45)
    pc = rng.uniform(-0.05, 0.05, (3, 16, 3)).astype(np.float32)
    pc[1, 11] = pc[1, 4]                            # identical tokens: identical rows in front of the pooling, every max tied
    pc, g = T(pc, dev), T(rng.standard_normal((3, 256)), dev)
    got, ref = hip_grads(m, pc, g), composite_grads(m, pc, g)
    compare("tied rows", got, ref, NET_TOL, composite_grads(m, pc, g, torch.float32), d_pc=False)
    gx, rx = got[1].double().clone(), ref[1].clone()
    for t in (gx, rx):                              # the two tied rows may share the max's gradient differently: compare their sum
        t[1, 4] += t[1, 11]
        t[1, 11] = 0
    e = err(gx, rx)
    print(f"ERR tied rows: d_pc (tied rows summed) {e:.2e}")
    assert e < NET_TOL


# ---- 6. PCTransformer.forward under autograd ----------------------------------------------------------------------------------------
def test_forward_under_autograd(dev):
    m, rng = _pct(dev), np.random.default_rng(46)
    pc = T(rng.uniform(-0.05, 0.05, (7, 16, 3)), dev)
    g = T(rng.standard_normal((7, 256)), dev)
    with torch.no_grad():
        y_ng = m(pc)
    p = pc.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    y = m(p)
    assert y.grad_fn is not None
    assert torch.equal(y.detach(), y_ng)
    (y * g).sum().backward(retain_graph=True)
    first = ({n: q.grad.clone() for n, q in m.named_parameters()}, p.grad.clone())
    compare("forward under autograd", first, composite_grads(m, pc, g), NET_TOL, composite_grads(m, pc, g, torch.float32))
    m.zero_grad(set_to_none=True)
    p.grad = None
    (y * g).sum().backward()
    assert all(torch.equal(first[0][n], q.grad) for n, q in m.named_parameters()) and torch.equal(first[1], p.grad)
    y = m(p)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad((y * g).sum(), list(m.parameters()), create_graph=True)


# ---- 7. SconeOcc with MCR_SCONE_OCC_BWD=pct ----------------------------------------------------------------------------------------
def _occ(dev, dtype=torch.float32):
    from macarons_amd.networks import SconeOcc
    m = SconeOcc()
    sd = weights.make_state_dict(weights.shapes_of(m), 2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(device=dev, dtype=dtype)


# The four transformers pool 128 maxima per sequence, and the gradient of a maximum jumps where two rows agree to within the forward's
# rounding (section 4): an fp32 forward then differentiates another branch than the fp64 reference, and the two differ by 1e-4 and
# more whatever the backward does.  The inputs are therefore the first draw (seeds 22 + B, 23 + B, ...) on which the fp32 TORCH
# composite -- the same function in the same precision, no code of the HIP backward -- agrees with the fp64 composite to
# WELL_POSED, ten times below the bound: a draw on which fp32 evaluation takes the reference's branch.
WELL_POSED = 1e-5


@pytest.mark.parametrize("B", [1, 2])
def test_scone_occ_backward_through_pct(dev, monkeypatch, B):
    from macarons_amd import autograd as A, ops
    occ, od = _occ(dev), _occ(dev, torch.float64)
    assert len(list(occ.parameters())) == 172
    torch.manual_seed(4)
    perms = occ.draw_perms(300)
    dp = [p.to(dev) for p in perms]
    monkeypatch.delenv("MCR_SCONE_OCC_BWD", raising=False)

    def composite(model, dtype, pc, x0, vq, scales, idx):
        x = x0.to(dtype, copy=True).requires_grad_(True)
        model.zero_grad(set_to_none=True)
        A.scone_occ(model, pc[:, dp[0]].to(dtype), [s_.to(dtype) for s_ in scales], x, vq.to(dtype), idx).sum().backward()
        return {n: q.grad.clone() for n, q in model.named_parameters()}, x.grad.clone()

    for seed in range(22 + B, 30 + B):
        rng = np.random.default_rng(seed)
        pc = T(rng.uniform(-.3, .3, (B, 300, 3)), dev)
        x0 = T(rng.uniform(-.4, .4, (B, 50, 3)), dev)
        vq = T(rng.standard_normal((B, 50, 64)) * 0.3, dev)
        scales = [pc, pc[:, dp[1]].contiguous()]
        scales.append(scales[1][:, dp[2]].contiguous())
        idx = [ops.knn_points(x0.contiguous(), s_, 16)[2] for s_ in scales]
        ref = composite(od, torch.float64, pc, x0, vq, scales, idx)
        torch32 = composite(occ, torch.float32, pc, x0, vq, scales, idx)
        yard = _worst(torch32, ref)
        print(f"ERR scone_occ B={B} seed {seed}: fp32 torch composite vs fp64: params max {yard[0]:.2e}  d_x {yard[1]:.2e}")
        if max(yard) < WELL_POSED:
            print(f"ERR scone_occ B={B}: seed {seed} taken, {seed - 22 - B} draw(s) rejected before it")
            break
    else:
        pytest.fail("no well-posed draw among eight")

    def grads():
        x = x0.clone().requires_grad_(True)
        occ.zero_grad(set_to_none=True)
        occ(pc, x, vq, perms=perms).sum().backward()
        return {n: q.grad.clone() for n, q in occ.named_parameters()}, x.grad.clone()

    # unset: today's path -- bit-equal to plain torch autograd through the all-torch composite, which is what it differentiates ...
    base = grads()
    assert all(torch.equal(base[0][n], torch32[0][n]) for n in base[0]) and torch.equal(base[1], torch32[1])
    # ... the composite's transformers are reached (counted), and any other value of the variable is the same path
    calls, real = [], A.pc_transformer
    monkeypatch.setattr(A, "pc_transformer", lambda pct, t: (calls.append(1), real(pct, t))[1])
    monkeypatch.setenv("MCR_SCONE_OCC_BWD", "composite")
    other = grads()
    assert len(calls) == 4
    assert all(torch.equal(base[0][n], other[0][n]) for n in base[0]) and torch.equal(base[1], other[1])
    monkeypatch.setenv("MCR_SCONE_OCC_BWD", "pct")
    got = grads()
    assert len(calls) == 4                          # the composite's transformers did not run again
    scale = max(float(t.abs().max()) for t in ref[0].values())
    for n in ref[0]:
        if n.endswith(ZERO_GRAD):
            e = float((got[0][n].double() - ref[0][n]).abs().max()) / scale
            e32 = float((base[0][n].double() - ref[0][n]).abs().max()) / scale
            print(f"ERR scone_occ pct B={B}: {n} (zero gradient) {e:.2e} x the largest (fp32 composite: {e32:.2e})")
            assert e < max(ZERO_TOL, 4 * e32), (n, e, e32)
    for n in ref[0]:
        if not n.endswith(ZERO_GRAD):
            assert err(got[0][n], ref[0][n], 1e-4 * scale) < NET_TOL, (n, err(got[0][n], ref[0][n], 1e-4 * scale))
    worst, ex = _worst(got, ref)
    print(f"ERR scone_occ pct B={B}: params max {worst:.2e}  d_x {ex:.2e}")
    assert ex < NET_TOL
