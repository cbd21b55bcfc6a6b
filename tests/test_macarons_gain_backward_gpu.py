"""HIP backward of the MACARONS-regime gain (macarons_gain_bwd.hip: mcr_macarons_gain_backward behind autograd.MacaronsGainFunction) and the
differentiable predict_coverage_gain_for_cameras built on it, against the fp64 composites (autograd.macarons_gain, autograd.visibilities,
autograd.scone_vis) under torch autograd.

Bounds.  Entry, d_vis: max |got - ref| <= 2e-6 x max |ref| per camera -- the value is a product of fewer than ten correctly rounded fp32
operations (<= 6e-7 relative), the bound is three times that; d_volume: 1e-6 relative.  Chain: the metric and bounds of
tests/test_scone_vis_backward_gpu.py (per-tensor max error over max reference, parameter denominators floored at 1e-4 x the largest
parameter gradient, NET_TOL = 1e-4; mhsa.w_k.bias by ZERO_TOL).  Measured errors are printed with an ERR prefix."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import golden
from test_macarons_regime_gpu import T, _models, _records
from test_scone_vis_backward_gpu import NET_TOL, ZERO_GRAD, ZERO_TOL, _double, err

pytestmark = pytest.mark.gpu

D_VIS_TOL = 2e-6
D_VOL_TOL = 1e-6
TH = 2.0
S_LIMIT = 8192


def _points(rng, cam, S, pts_dim, th=TH):
    """[K,S,pts_dim] fp32 points at distances on both sides of th from their cameras, none within 1e-3 th of it (asserted on the fp32
    values); the fourth column is a payload the gain must not read."""
    K = cam.shape[0]
    dirs = rng.standard_normal((K, S, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    r = np.where(rng.random((K, S)) < 0.5, rng.uniform(0.2, 0.95, (K, S)), rng.uniform(1.05, 4.0, (K, S))) * th
    if S > 1:
        r[:, 0], r[:, 1] = 0.5 * th, 2.0 * th
    world = (cam[:, None, :] + dirs * r[..., None]).astype(np.float32)
    if pts_dim > 3:
        world = np.concatenate([world, rng.uniform(0, 1, (K, S, pts_dim - 3)).astype(np.float32)], -1)
    d = np.linalg.norm(world[..., :3].astype(np.float64) - cam[:, None, :].astype(np.float64), axis=-1)
    assert np.abs(d - th).min() > 1e-3 * th
    if S > 1:
        assert (d > th).any() and (d < th).any()
    return world


def _reference(g, vis, world, inv, nu, cam, vol, th, smooth):
    """(d_vis, d_volume, gains) of the fp64 composite on the same fp32 inputs, under autograd."""
    from macarons_amd import autograd as A
    v = vis.double().requires_grad_(True)
    w = vol.double().requires_grad_(True)
    gains = A.macarons_gain(v, world.double(), inv, nu, cam.double(), w, th, smooth)
    (gains * g.double()).sum().backward()
    return v.grad, w.grad, gains.detach()


def _check(tag, got, ref, nu=None):
    d_vis, d_vol = got
    r_vis, r_vol, _ = ref
    worst = 0.0
    for k in range(d_vis.shape[0]):
        scale = float(r_vis[k].abs().max())
        e = float((d_vis[k].double() - r_vis[k]).abs().max())
        if scale > 0:
            worst = max(worst, e / scale)
        assert e <= D_VIS_TOL * scale, (tag, k, e, scale)
    ev = float(((d_vol.double() - r_vol).abs() / r_vol.abs().clamp(min=1e-300)).max()) if nu is None else \
        float(((d_vol.double() - r_vol).abs()[nu > 0] / r_vol.abs()[nu > 0]).max())
    print(f"ERR gain backward {tag}: d_vis {worst:.2e}  d_volume {ev:.2e}")
    assert ev <= D_VOL_TOL, (tag, ev)


# ---- (a) the entry against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [False, True])
def test_entry_against_fp64(dev, smooth):
    from macarons_amd import ops
    rng = np.random.default_rng(70 + smooth)
    K, S = 4, 70                                          # S: neither a multiple of 64 nor of 256
    cam = rng.uniform(-1, 1, (K, 3)).astype(np.float32)
    world = T(_points(rng, cam, S, 4), dev)
    nine = np.concatenate([np.arange(9), rng.integers(0, 9, S - 9)])
    inv = T(np.stack([rng.permutation(S),                 # 0: all samples distinct
                      rng.permutation(nine),              # 1: heavy duplicates, 70 samples over 9 rows
                      np.zeros(S, np.int64),              # 2: every sample on row 0
                      np.zeros(S, np.int64)]), dev)       # 3: empty frustum
    nu = torch.tensor([S, 9, 1, 0], dtype=torch.int32, device=dev)
    vis = T(rng.uniform(0.05, 1, (K, S)).astype(np.float32), dev)
    vol = T(rng.uniform(0.5, 30, K).astype(np.float32), dev)
    g = T(rng.standard_normal(K).astype(np.float32), dev)
    cam = T(cam, dev)
    got = ops.macarons_gain_backward(g, vis, world, inv, nu, cam, vol, TH, smooth, need_volume=True)
    ref = _reference(g, vis, world, inv, nu, cam, vol, TH, smooth)
    _check(f"4x70 smooth={smooth}", got, ref, nu)
    d_vis, d_vol = got
    for k, n in enumerate(nu.tolist()):
        assert torch.count_nonzero(d_vis[k, n:]) == 0, k                       # rows u >= n_unique[k]: exactly zero
    assert torch.count_nonzero(d_vis[3]) == 0 and float(d_vol[3]) == 0.0
    assert torch.count_nonzero(d_vis[0]) == S and torch.count_nonzero(d_vis[1]) == 9 and torch.count_nonzero(d_vis[2]) == 1
    # d_volume / g is the forward's mean: gains / volume to fp32 rounding
    gains = ops.macarons_gain_indexed(vis, world, inv, nu, cam, vol, TH, smooth)
    assert float(((d_vol / g)[:3] / (gains / vol)[:3] - 1).abs().max()) < 4e-7
    again = ops.macarons_gain_backward(g, vis, world, inv, nu, cam, vol, TH, smooth, need_volume=True)
    assert torch.equal(again[0], d_vis) and torch.equal(again[1], d_vol)
    only_vis, none = ops.macarons_gain_backward(g, vis, world, inv, nu, cam, vol, TH, smooth)
    assert none is None and torch.equal(only_vis, d_vis)


# ---- (b) the factor is the forward's factor ---------------------------------------------------------------------------------------------
def test_factor_is_the_forwards_factor(dev):
    """Identity form, grad_gains = S, volume = 1: (g * vol) / S is exactly 1 and every count is 1, so d_vis is the distance factor itself,
    bit for bit what get_distance_factor_threshold / get_distance_factor_smooth (macarons_gain_kernel) return for the same points."""
    from macarons_amd import ops
    from macarons_amd.utility import macarons_utils as mu
    rng = np.random.default_rng(64)
    K, S = 2, 64
    cam = rng.uniform(-1, 1, (K, 3)).astype(np.float32)
    params, fc = NS(image_height=256, image_width=456), NS(fov=torch.tensor([60.0]))
    th_s = mu.sensor_distance_threshold(params, fc, 0.1)
    g = torch.full((K,), float(S), device=dev)
    one = torch.ones(K, device=dev)
    vis = T(rng.uniform(0.05, 1, (K, S)).astype(np.float32), dev)
    for smooth, th in ((False, TH), (True, th_s), (False, th_s)):
        world = T(_points(rng, cam, S, 4, th), dev)
        d_vis, _ = ops.macarons_gain_backward(g, vis, world, None, None, T(cam, dev), one, th, smooth)
        for k in range(K):
            xc = T(cam[k:k + 1], dev)
            if smooth:
                want = mu.get_distance_factor_smooth(params, world[k], xc, fc, 0.1)
            elif th == TH:
                want = mu.get_distance_factor_threshold(world[k], xc, TH)
            else:
                want = mu.get_distance_factor(params, world[k], xc, fc, 0.1)
            assert torch.equal(d_vis[k], want.view(-1)), (smooth, th, k)
            assert float(want.min()) < 1.0


# ---- (c) edges ----------------------------------------------------------------------------------------------------------------------
def _edge_case(dev, K, S, pts_dim, indexed, seed):
    rng = np.random.default_rng(seed)
    cam = rng.uniform(-1, 1, (K, 3)).astype(np.float32)
    world = T(_points(rng, cam, S, pts_dim), dev)
    inv = nu = None
    if indexed:
        n_u = max(1, S // 3)
        inv = T(rng.integers(0, n_u, (K, S)), dev)
        nu = torch.full((K,), n_u, dtype=torch.int32, device=dev)
    vis = T(rng.uniform(0.05, 1, (K, S)).astype(np.float32), dev)
    vol = T(rng.uniform(0.5, 30, K).astype(np.float32), dev)
    g = T(rng.standard_normal(K).astype(np.float32), dev)
    return g, vis, world, inv, nu, T(cam, dev), vol


@pytest.mark.parametrize("K,S,pts_dim,indexed", [(3, 1, 4, True), (3, 1, 4, False), (1, S_LIMIT, 4, True), (2, 300, 3, False)])
@pytest.mark.parametrize("smooth", [False, True])
def test_edges(dev, K, S, pts_dim, indexed, smooth):
    from macarons_amd import ops
    g, vis, world, inv, nu, cam, vol = _edge_case(dev, K, S, pts_dim, indexed, 1000 + S)
    got = ops.macarons_gain_backward(g, vis, world, inv, nu, cam, vol, TH, smooth, need_volume=True)
    _check(f"{K}x{S} pts_dim={pts_dim} indexed={indexed} smooth={smooth}", got, _reference(g, vis, world, inv, nu, cam, vol, TH, smooth))
    if indexed:                                           # rows no sample maps to: exactly zero
        assert torch.count_nonzero(got[0][:, int(nu[0]):]) == 0


def test_more_samples_than_counters_is_an_error(dev):
    """Argument validation on the host: nothing is launched."""
    from macarons_amd import _lib, ops
    S = S_LIMIT + 1
    z = torch.zeros(1, S, device=dev)
    with pytest.raises(_lib.MacaronsHipError, match=str(S_LIMIT)) as e:
        ops.macarons_gain_backward(torch.ones(1, device=dev), z, torch.zeros(1, S, 4, device=dev), torch.zeros(1, S, dtype=torch.int64, device=dev),
                                   torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, 3, device=dev), torch.ones(1, device=dev), TH)
    assert "mcr_macarons_gain_backward" in str(e.value)
    assert str(S_LIMIT) in _lib.lib().mcr_last_error().decode()


def test_function_identity_form(dev):
    """MacaronsGainFunction without a map: the bits of ops.macarons_gain_, its input left alone, gradients to vis and volume."""
    from macarons_amd import autograd as A, ops
    g, vis, world, _, _, cam, vol = _edge_case(dev, 2, 300, 4, False, 77)
    v, w = vis.clone().requires_grad_(True), vol.clone().requires_grad_(True)
    gains = A.MacaronsGainFunction.apply(v, world, None, None, cam, w, TH, False)
    assert torch.equal(v.detach(), vis)
    assert torch.equal(gains.detach(), ops.macarons_gain_(vis.clone(), world, cam, vol, TH, False))
    (gains * g).sum().backward()
    _check("Function, identity form", (v.grad, w.grad), _reference(g, vis, world, None, None, cam, vol, TH, False))
    with pytest.raises(RuntimeError, match="differentiable once"):
        gains = A.MacaronsGainFunction.apply(v, world, None, None, cam, w, TH, False)
        torch.autograd.grad((gains * g).sum(), [v], create_graph=True)


# ---- (d) the chain: predict_coverage_gain_for_cameras -> loss -> backward ---------------------------------------------------------------
SEQ = 160
W = (0.7, -1.3, 0.4, 2.0)


def _scene(dev):
    g = golden("single_camera")
    P_ = len(g["X_world"])
    vh = (g["vh_u"][:, None] * g["vh_v"][None, :] + g["vh_w"][np.arange(P_) % 16]).astype(np.float32)
    recs = _records(g, float(g["sensor_range"])).to(dev)
    u = torch.zeros(4, 2048, device=dev)
    for c in range(3):
        u[c] = T(g[f"u_{c}"], dev)
    Mpred = T(np.repeat(g["Mpred"], 4, 0), dev)
    return [T(g["X_world"], dev), T(vh, dev), T(g["occ"], dev), recs, T(g["eyes"], dev), Mpred, float(g["box_diag"])], u[:, :SEQ].contiguous()


def _cams(args, u, sel):
    """The scene with the cameras `sel` only."""
    return [a[sel] if i in (3, 4, 5) else a for i, a in enumerate(args)], u[sel]


def _hip_step(vis_model, args, u, w, **kw):
    from macarons_amd.utility import macarons_utils as mu
    vis_model.zero_grad(set_to_none=True)
    rec = {}
    out = mu.predict_coverage_gain_for_cameras(vis_model, *args, seq_len=SEQ, samples=u, record=rec, differentiable=True, **kw)
    gains = out[0] if kw.get("return_parts") else out
    (gains * w).sum().backward()
    return gains, {n: (None if p.grad is None else p.grad.clone()) for n, p in vis_model.named_parameters()}, rec, out


def _composite_step(vis_model, args, samples, w):
    """The same step through the fp64 composites; the sampled sets are recomputed by the same ops calls and used as constants."""
    from macarons_amd import autograd as A, ops
    X_world, vh, occ, recs, eyes, Mpred, box_diag = args
    K, dev = recs.shape[0], X_world.device
    mask = ops.points_in_fov(X_world, recs)
    occ_k = ops.fov_mask_occ(mask, occ.reshape(-1).contiguous())
    res, res_h, inv, _, nu, vol = ops.sample_proxy_batched(X_world, occ_k, vh, samples.contiguous(), 0.1)
    Mv, xc, inv_d = Mpred.float().contiguous(), eyes.reshape(K, 3).contiguous(), 1.0 / box_diag
    center, cam_view = ops.camera_boxes(res, nu, Mv, xc, inv_d)
    pts = res.clone()
    ops.transform_points_batched_(pts, Mv, center, torch.full((K,), inv_d, dtype=torch.float32, device=dev))
    md = _double(vis_model)
    harm = A.scone_vis(md, pts.double(), res_h.double(), nu)
    vis = A.visibilities(pts.double(), harm, cam_view.view(K, 1, 3).double(), True).view(K, SEQ)
    gains = A.macarons_gain(vis, res.double(), inv, nu, xc.double(), vol.double(), 17., False)
    (gains * w.double()).sum().backward()
    return gains.detach(), {n: q.grad for n, q in md.named_parameters()}, nu


def _compare_params(tag, got, ref):
    scale = max(float(t.abs().max()) for t in ref.values())
    worst = 0.0
    for n in ref:
        if n.endswith(ZERO_GRAD):
            e = float((got[n].double().cpu() - ref[n].double().cpu()).abs().max()) / scale
            print(f"ERR {tag}: {n} (zero gradient) {e:.2e} x the largest")
            assert e < ZERO_TOL, (tag, n, e)
            continue
        e = err(got[n], ref[n], 1e-4 * scale)
        worst = max(worst, e)
        assert e < NET_TOL, (tag, n, e)
    print(f"ERR {tag}: params max {worst:.2e}  (largest parameter gradient {scale:.3e})")


@pytest.fixture(scope="module")
def chain(dev):
    m = _models(dev).visibility
    assert all(p.requires_grad for p in m.parameters())
    args, u = _scene(dev)
    w = torch.tensor(W, device=dev)
    gains, grads, rec, _ = _hip_step(m, args, u, w)
    return NS(model=m, args=args, u=u, w=w, gains=gains, grads=grads, rec=rec)


def test_chain_against_fp64_composite(dev, chain):
    assert chain.gains.requires_grad and chain.gains.shape == (4,)
    assert float(chain.gains.detach()[3]) == 0.0 and float(chain.gains.detach()[:3].min()) > 0
    for n, t in chain.grads.items():
        assert t is not None and bool(torch.isfinite(t).all()), n
    assert torch.equal(chain.rec["samples"], chain.u)
    ref_gains, ref, nu = _composite_step(chain.model, chain.args, chain.rec["samples"], chain.w)
    assert nu.tolist()[3] == 0 and min(nu.tolist()[:3]) > 0
    eg = err(chain.gains, ref_gains)
    print(f"ERR chain 4x{SEQ}: gains {eg:.2e}")
    assert eg < NET_TOL
    _compare_params(f"chain 4x{SEQ}", chain.grads, ref)
    gains2, grads2, _, _ = _hip_step(chain.model, chain.args, chain.u, chain.w)       # a fresh graph: identical bits
    assert torch.equal(gains2.detach(), chain.gains.detach())
    for n, t in chain.grads.items():
        assert torch.equal(grads2[n], t), n


# ---- (e) nothing moved ------------------------------------------------------------------------------------------------------------------
def test_no_grad_and_return_parts_keep_the_bits(dev, chain):
    from macarons_amd.utility import macarons_utils as mu
    with torch.no_grad():
        plain = mu.predict_coverage_gain_for_cameras(chain.model, *chain.args, seq_len=SEQ, samples=chain.u, differentiable=True)
        _, vis_ng, world_ng = mu.predict_coverage_gain_for_cameras(chain.model, *chain.args, seq_len=SEQ, samples=chain.u, return_parts=True)
    assert not plain.requires_grad and torch.equal(plain, chain.gains.detach())
    unasked = mu.predict_coverage_gain_for_cameras(chain.model, *chain.args, seq_len=SEQ, samples=chain.u)     # no keyword: no graph
    assert not unasked.requires_grad and torch.equal(unasked, plain)
    gains, grads, _, out = _hip_step(chain.model, chain.args, chain.u, chain.w, return_parts=True)
    assert gains.requires_grad and torch.equal(gains.detach(), plain)
    for n, t in chain.grads.items():                       # the same graph behind it
        assert torch.equal(grads[n], t), n
    _, vis, world = out
    assert vis[3] is None and world[3] is None
    for c in range(3):                                     # the lists: detached values, today's bits
        assert not vis[c].requires_grad and torch.equal(vis[c], vis_ng[c]) and torch.equal(world[c], world_ng[c])


def test_all_cameras_empty(dev, chain):
    """K = 1, the empty frustum alone: gain 0, every parameter gets a finite all-zero gradient tensor."""
    args, u = _cams(chain.args, chain.u, slice(3, 4))
    gains, grads, _, _ = _hip_step(chain.model, args, u, chain.w[3:4])
    assert gains.requires_grad and gains.shape == (1,) and float(gains.detach()[0]) == 0.0
    for n, t in grads.items():
        assert t is not None, n
        assert bool(torch.isfinite(t).all()) and torch.count_nonzero(t) == 0, n
