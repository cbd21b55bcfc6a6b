"""The scorer's HIP backward (mcr_sh_scorer_backward): ops.sh_scorer_backward against the reference's fp64 gradients
(tests/golden/scorer_grad.npz) and against the fp64 composite (autograd.coverage_gain / autograd.visibilities) on the GPU; the
differentiable torch.ops.macarons.sh_coverage_gain / sh_visibilities and the SconeVis / Macarons entry points that use them.
Errors are per tensor: max |got - ref| / max |ref|.  Measured errors are printed (run with -s to see them)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import weights  # noqa: E402

pytestmark = pytest.mark.gpu
# proposed from fp32 summation depth; measured values in NOTES.md
TOL_H, TOL_DIR = 1e-5, 1e-4
WRT = ("harm", "pts", "cams")


def T(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)


def composite_grads(pts, harm, cams, w, per_pair, sig, need=(True, True, True)):
    """fp64 autograd through the composite; w [B,C] (gains) or [B,C,N] (per pair)."""
    from macarons_amd import autograd as A
    p, h, c = (t.detach().double().requires_grad_(n) for t, n in zip((pts, harm, cams), (need[1], need[0], need[2])))
    out = A.visibilities(p, h, c, sig) if per_pair else A.coverage_gain(p, h, c, sig)
    (out * w.double()).sum().backward()
    return h.grad, p.grad, c.grad


def check(got, ref, tag, need=(True, True, True)):
    errs = []
    for name, g, r, n, tol in zip(WRT, got, ref, need, (TOL_H, TOL_DIR, TOL_DIR)):
        if not n:
            assert g is None, (tag, name)
            continue
        assert g is not None and torch.isfinite(g).all(), (tag, name)
        e = rel_err(g.cpu().numpy(), r.cpu().numpy() if torch.is_tensor(r) else r)
        errs.append(f"{name} {e:.2e}")
        assert e <= tol, (tag, name, e)
    print("ERR", tag, " ".join(errs))


@pytest.mark.parametrize("case", ["4", "3"])
@pytest.mark.parametrize("kind", ["gain", "vis"])
@pytest.mark.parametrize("act", ["sig", "relu"])
def test_backward_matches_reference_gradients(dev, case, kind, act):
    from macarons_amd import ops
    f = golden("scorer_grad")
    pts, harm, cams = (T(f[k + case], dev) for k in ("pts", "harm", "cams"))
    w = T(f[("w_gain" if kind == "gain" else "w_pair") + case], dev)
    got = ops.sh_scorer_backward(pts, harm, cams, w, kind == "vis", act == "sig")
    assert got[1].shape == pts.shape
    check(got, [f[f"g_{kind}_{act}_{wrt}{case}"] for wrt in WRT], f"golden case{case} {kind} {act}")
    if case == "4":
        assert torch.all(got[1][..., 3] == 0)


def _inputs(rng, B, N, C, dev, pts_dim=4, sigma=0.5):
    pts = np.concatenate([rng.uniform(-.5, .5, (B, N, 3)), rng.uniform(.1, 1, (B, N, pts_dim - 3))], -1).astype(np.float32)
    harm = (rng.standard_normal((B, N, 64)) * sigma).astype(np.float32)
    cams = rng.standard_normal((B, C, 3))
    cams = (1.5 * cams / np.linalg.norm(cams, axis=-1, keepdims=True)).astype(np.float32)
    return T(pts, dev), T(harm, dev), T(cams, dev)


def _weights(rng, pts, harm, cams, per_pair, sig, dev):
    """Upstream gradient; for relu per pair, pairs with |z| < 1e-3 (fp64) get weight 0 so that no pair near the kink can take the
    other side in fp32."""
    B, N, C = pts.shape[0], pts.shape[1], cams.shape[1]
    w = T(rng.standard_normal((B, C, N) if per_pair else (B, C)), dev)
    if per_pair and not sig:
        from macarons_amd import autograd as A
        with torch.no_grad():
            rays = cams.double()[:, :, None, :] - pts.double()[:, None, :, :3]
            z = (A.sh_basis(rays / torch.linalg.norm(rays, dim=-1, keepdim=True)) * harm.double()[:, None]).sum(-1)
        w = torch.where(z.abs() < 1e-3, torch.zeros_like(w), w)
    return w


def test_backward_pretraining_shape_and_edges(dev):
    """B = 3, N = 2048, C = 52 (pretrain_scone_vis.py) and edge shapes, both kinds of upstream gradient."""
    from macarons_amd import ops
    rng = np.random.default_rng(5)
    shapes = [(3, 2048, 52)] + [(2, n, c) for n in (1, 63, 65, 500) for c in (1, 7, 200)]
    for i, (B, N, C) in enumerate(shapes):
        pts, harm, cams = _inputs(rng, B, N, C, dev)
        for per_pair, sig in ((False, True), (True, False)) if i % 2 else ((False, True), (True, True), (True, False)):
            w = _weights(rng, pts, harm, cams, per_pair, sig, dev)
            got = ops.sh_scorer_backward(pts, harm, cams, w, per_pair, sig)
            check(got, composite_grads(pts, harm, cams, w, per_pair, sig), f"B{B} N{N} C{C} per_pair={per_pair} sig={sig}")


def test_backward_rays_along_the_polar_axis(dev):
    """Cameras straight above and below points (rays along +-Y exactly: n_x = n_z = 0)."""
    from macarons_amd import ops
    rng = np.random.default_rng(6)
    pts, harm, cams = _inputs(rng, 1, 130, 8, dev, pts_dim=3)
    cams = cams.clone()
    for c, (n, dy) in enumerate([(0, 1.2), (0, -1.2), (64, 0.7), (129, -0.9)]):
        cams[0, c] = pts[0, n, :3] + torch.tensor([0., dy, 0.], device=dev)
    rays = cams[0, :4] - pts[0, [0, 0, 64, 129], :3]
    assert torch.all(rays[:, 0] == 0) and torch.all(rays[:, 2] == 0)
    for per_pair, sig in ((False, True), (True, True), (True, False)):
        w = _weights(rng, pts, harm, cams, per_pair, sig, dev)
        got = ops.sh_scorer_backward(pts, harm, cams, w, per_pair, sig)
        check(got, composite_grads(pts, harm, cams, w, per_pair, sig), f"polar axis per_pair={per_pair} sig={sig}")


def test_backward_every_need_subset(dev):
    """Each non-empty subset of (d_harm, d_pts, d_cams): the others are None (null outputs: never written), the rest as with all three."""
    from macarons_amd import ops
    rng = np.random.default_rng(7)
    for B, N, C in ((3, 2048, 52), (1, 300, 9)):
        pts, harm, cams = _inputs(rng, B, N, C, dev)
        for per_pair in (False, True):
            w = _weights(rng, pts, harm, cams, per_pair, True, dev)
            ref = composite_grads(pts, harm, cams, w, per_pair, True)
            for need in itertools.product((False, True), repeat=3):
                if any(need):
                    got = ops.sh_scorer_backward(pts, harm, cams, w, per_pair, True, need=need)
                    check(got, ref, f"need={need} B{B} N{N} C{C} per_pair={per_pair}", need)


def test_backward_headline_shape(dev):
    """100 000 points x 200 cameras: d_harm on sampled points (first and last wave-tile included) against the fp64 composite on those
    points with the per-pair weight g / N; d_cams against the fp64 composite accumulated over point chunks; everything finite."""
    from macarons_amd import ops
    rng = np.random.default_rng(8)
    B, N, C = 1, 100_000, 200
    pts, harm, cams = _inputs(rng, B, N, C, dev)
    g = T(rng.standard_normal((B, C)), dev)
    d_harm, d_pts, d_cams = ops.sh_scorer_backward(pts, harm, cams, g, False, True)
    assert all(torch.isfinite(t).all() for t in (d_harm, d_pts, d_cams))
    d_harm_only = ops.sh_scorer_backward(pts, harm, cams, g, False, True, need=(True, False, False))[0]
    idx = np.unique(np.concatenate([np.arange(64), np.arange(N - 64, N), rng.choice(N, 4096, replace=False)]))
    it = torch.from_numpy(idx).to(dev)
    w = (g.double() / N)[:, :, None].expand(B, C, len(idx))
    ref_h = composite_grads(pts[:, it], harm[:, it], cams, w, True, True, need=(True, False, False))[0]
    e_h = rel_err(d_harm[:, it].cpu().numpy(), ref_h.cpu().numpy())
    e_h1 = rel_err(d_harm_only[:, it].cpu().numpy(), ref_h.cpu().numpy())
    ref_c = torch.zeros((B, C, 3), dtype=torch.float64, device=dev)
    for lo in range(0, N, 5000):
        sl = slice(lo, min(N, lo + 5000))
        wc = (g.double() / N)[:, :, None].expand(B, C, sl.stop - sl.start)
        ref_c += composite_grads(pts[:, sl], harm[:, sl], cams, wc, True, True, need=(False, False, True))[2]
    e_c = rel_err(d_cams.cpu().numpy(), ref_c.cpu().numpy())
    print(f"ERR headline 100000x200 harm {e_h:.2e} harm(d_harm only) {e_h1:.2e} cams {e_c:.2e}")
    # d_harm bound loosened from 1e-5: measured 1.77e-5.  Here one camera chunk covers all 200 cameras, so each point's 200 pairs are
    # summed in monomial space and transformed once; the transform's large alternating coefficients amplify that sum's rounding (an
    # fp32 emulation of the kernel gives 1.75e-5 for one transform per point, 1.9e-6 for one per 4 cameras, the chunked shapes above).
    assert e_h <= 3e-5 and e_h1 <= 3e-5 and e_c <= TOL_DIR, (e_h, e_h1, e_c)


def test_backward_is_deterministic(dev):
    from macarons_amd import ops
    rng = np.random.default_rng(9)
    for B, N, C in ((3, 2048, 52), (1, 100_000, 200)):
        pts, harm, cams = _inputs(rng, B, N, C, dev)
        for per_pair in (False, True):
            w = _weights(rng, pts, harm, cams, per_pair, True, dev) if per_pair else T(rng.standard_normal((B, C)), dev)
            a = ops.sh_scorer_backward(pts, harm, cams, w, per_pair, True)
            b = ops.sh_scorer_backward(pts, harm, cams, w, per_pair, True)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (B, N, C, per_pair)


def _vis_module(dev, use_sigmoid=True):
    from macarons_amd.networks import SconeVis
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = SconeVis(use_sigmoid=use_sigmoid)
    sd = weights.make_state_dict(weights.shapes_of(m), 1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def test_entry_points_backpropagate_through_the_hip_backward(dev, monkeypatch):
    """SconeVis.compute_coverage_gain / compute_visibilities and Macarons.compute_visibility_gains differentiate without the composite
    (autograd.coverage_gain / visibilities raise here); torch.ops.macarons.sh_coverage_gain / sh_visibilities are differentiable."""
    from macarons_amd import autograd as A
    from macarons_amd import ops, torch_ops  # noqa: F401
    from macarons_amd.networks.Macarons import Macarons
    rng = np.random.default_rng(10)
    pts, harm, cams = _inputs(rng, 2, 300, 11, dev)
    wg = T(rng.standard_normal((2, 11)), dev)
    wv = T(rng.standard_normal((2, 11, 300)), dev)
    refs = {k: composite_grads(pts, harm, cams, w, k == "vis", True) for k, w in (("gain", wg), ("vis", wv))}

    ref_ones = composite_grads(pts, harm, cams, torch.ones_like(wg), False, True, need=(True, False, False))[0]

    def boom(*a, **k):
        raise AssertionError("the composite must not run")
    monkeypatch.setattr(A, "coverage_gain", boom)
    monkeypatch.setattr(A, "visibilities", boom)
    vis = _vis_module(dev)
    mac = Macarons(None, None, vis)
    calls = {
        "SconeVis.compute_coverage_gain": ("gain", vis.compute_coverage_gain),
        "SconeVis.compute_visibilities": ("vis", vis.compute_visibilities),
        "Macarons.compute_visibility_gains": ("vis", mac.compute_visibility_gains),
        "torch.ops.macarons.sh_coverage_gain": ("gain", lambda p, h, c: torch.ops.macarons.sh_coverage_gain(p, h, c, True)),
        "torch.ops.macarons.sh_visibilities": ("vis", lambda p, h, c: torch.ops.macarons.sh_visibilities(p, h, c, True)),
    }
    for name, (kind, fn) in calls.items():
        p, h, c = (t.clone().requires_grad_(True) for t in (pts, harm, cams))
        out = fn(p, h, c)
        with torch.no_grad():
            plain = fn(pts, harm, cams)
        assert torch.equal(out.detach(), plain) and out.requires_grad, name
        (out * (wg if kind == "gain" else wv)).sum().backward()
        check((h.grad, p.grad, c.grad), refs[kind], name)
    # only the inputs that require a gradient get one; x.sum().backward() hands in an expanded, zero-stride gradient
    h = harm.clone().requires_grad_(True)
    vis.compute_coverage_gain(pts, h, cams).sum().backward()
    assert rel_err(h.grad.cpu().numpy(), ref_ones.cpu().numpy()) <= TOL_H


def test_backward_peak_memory(dev):
    """N = 20 000, C = 200: backward() raises the peak allocation by at most 64 MB (the composite held about 1 GB here)."""
    rng = np.random.default_rng(11)
    pts, harm, cams = _inputs(rng, 1, 20_000, 200, dev)
    vis = _vis_module(dev)
    p, h, c = (t.clone().requires_grad_(True) for t in (pts, harm, cams))
    gains = vis.compute_coverage_gain(p, h, c)
    loss = (gains * T(rng.standard_normal((1, 200)), dev)).sum()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    loss.backward()
    torch.cuda.synchronize()
    rise = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    print(f"ERR peak memory rise during backward at 20000x200: {rise:.1f} MB")
    assert rise <= 64, rise
    assert all(torch.isfinite(t.grad).all() for t in (p, h, c))


def test_pretraining_chain_gradients(dev):
    """pretrain_scone_vis.py:168-224: SconeVis forward -> gather with duplicate sample indices (true_monte_carlo_sampling) ->
    compute_coverage_gain -> L1_loss -> backward; parameter gradients against the all-composite fp64 chain."""
    from macarons_amd import autograd as A
    from macarons_amd.networks.SconeVis import L1_loss
    rng = np.random.default_rng(12)
    vis = _vis_module(dev)
    N, C = 2048, 52
    pts = T(np.concatenate([rng.uniform(-.5, .5, (1, N, 3)), rng.uniform(.1, 1, (1, N, 1))], -1), dev)
    vh = T(rng.standard_normal((1, N, 64)) * 0.3, dev)
    cams = T(1.5 * rng.standard_normal((1, C, 3)), dev)
    sample_idx = torch.from_numpy(rng.integers(0, N, N)).to(dev)          # with replacement: duplicates
    assert len(torch.unique(sample_idx)) < N
    gt = T(rng.uniform(0, 1, (1, C, 1)), dev)
    loss_fn = L1_loss()

    def chain(model, p, v, c, coverage):
        h = model(p, view_harmonics=v) if coverage is None else A.scone_vis(model, p, v)
        g = (model.compute_coverage_gain if coverage is None else coverage)(p[:, sample_idx], h[:, sample_idx], c)
        return loss_fn(g[..., None], gt.to(g.dtype))

    for q in vis.parameters():
        q.grad = None
    chain(vis, pts, vh, cams, None).backward()
    got = {n: q.grad.clone() for n, q in vis.named_parameters()}
    vis64 = _vis_module(dev).double()                          # the same weights (the module's host caches do not deep-copy)
    for q in vis64.parameters():
        q.grad = None
    chain(vis64, pts.double(), vh.double(), cams.double(), A.coverage_gain).backward()
    scale = max(float(q.grad.abs().max()) for q in vis64.parameters())
    worst = 0.0
    for n, q in vis64.named_parameters():
        ref = q.grad.cpu().numpy()
        floor = max(np.abs(ref).max(), 1e-4 * scale)          # as in the trainer test of test_networks_gpu.py
        e = np.abs(got[n].double().cpu().numpy() - ref).max() / floor
        worst = max(worst, e)
        assert e < 1e-3, (n, e)
    print(f"ERR pretraining chain: worst parameter gradient {worst:.2e}")
