"""The SH scorer (sh_scorer.hip, sh_mono.h, sh_scorer_bwd.hip) basis function by basis function, and bit for bit at the edges of its work
split.  Cases, expected values and bounds: tests/_scorer_cases.py (checked on the CPU by tests/test_scorer_cases_cpu.py).

A. Forward, one basis function at a time: harm = +-e_k at the origin, the cameras the direction set D, against the fp64 basis within
   E_k(d) = 32 * 2^-24 * max(A_k(d), 1) (relu), E_k / 4 + 4 * 2^-24 (sigmoid, the SCALED table); the gains within the mean of the bounds.
B. Exact operands: saturating coefficients on lattice points, every visibility exactly 0, 0.5 or 1, every gain and the arg-max record
   (ties to the lower index) bit for bit, outputs poisoned with -7 beforehand, at the shapes of EXACT_SHAPES and under every
   waves_per_simd override.
C. Backward, one basis function at a time: d_harm rows are the 64 basis values of one direction (within E_k), or their sum over the
   cameras (within the sum of E_k); d_pts and d_cams of each basis function alone against fp64 autograd through autograd.sh_basis,
   at TOL_DIR = 1e-4 of that basis function's own largest gradient.

Every measured distance is printed with an ERR prefix before it is asserted (run with -s).

Measured on an MI355X, error / (2^-24 * max(A, 1)), worst over D per degree l = 0 .. 7 (the bound is 32; the CPU emulation of the
documented operation order gives 0.25 0.82 2.34 3.33 4.45 4.68 6.06 6.90):
  forward relu, visibilities:         0.25 0.71 2.47 2.76 4.45 4.71 7.93 8.21   (3.7e-6 absolute at worst)
  backward d_harm, one pair per point: 0.25 1.12 2.60 3.31 4.77 6.20 6.39 8.94   (3.4e-6 absolute at worst)
The sigmoid path reaches 0.19 of its bound, the gains 0.02 (relu) and 0.08 (sigmoid) of theirs, d_harm summed over 200 cameras 0.06 of
the summed bound; d_pts and d_cams of a single basis function 1.1e-6 of its largest gradient at worst (l = 6), d_cams against the
negated sum of the d_pts rows 5.5e-8.  v_rcp_f32(1.0) returned exactly 1 in every exact case; no exact case differed in any bit.
"""
import numpy as np
import pytest
import torch

import _scorer_cases as sc

pytestmark = pytest.mark.gpu
TOL_DIR = 1e-4                       # the project's bound on the direction gradients (tests/test_scorer_backward_gpu.py)


def T(x, dev):
    return torch.from_numpy(np.array(x)).to(dev)                        # a copy: the case file's arrays are read-only


def fmt(v):
    return " ".join(f"{x:.2f}" for x in v)


# ---- A. forward, one basis function at a time ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basis_reference():
    """Y [|D|,64] and E [|D|,64] in fp64, computed once and never changed."""
    D = sc.directions()
    Y, E = sc.basis(D), sc.bound(D)
    Y.flags.writeable = E.flags.writeable = False
    return Y, E


@pytest.mark.parametrize("pts_dim", [3, 4])
def test_forward_relu_one_basis_function_at_a_time(dev, basis_reference, pts_dim):
    from macarons_amd import ops
    Y, E = basis_reference
    pts, harm, cams = (T(a, dev) for a in sc.basis_operands(pts_dim))
    vis = ops.sh_visibilities(pts, harm, cams, use_sigmoid=False)[0].cpu().numpy().astype(np.float64)
    gains = ops.sh_coverage_gain(pts, harm, cams, use_sigmoid=False)[0].cpu().numpy().astype(np.float64)
    assert vis.shape == (len(Y), sc.N_BASIS_POINTS) and np.isfinite(vis).all()
    plus, minus = vis[:, :64], vis[:, 64:128]
    err = (plus - minus) - Y
    ratios = sc.ratio_per_degree(err, sc.directions())
    print(f"ERR forward relu pts_dim {pts_dim}: error / (2^-24 max(A, 1)) per l: {fmt(ratios)}; absolute worst {np.abs(err).max():.2e}")
    bad = np.argwhere(np.abs(err) > E)
    assert len(bad) == 0, [(int(c), int(sc.L_OF[k]), int(sc.M_OF[k]), err[c, k], E[c, k]) for c, k in bad[:8]]      # (camera, l, m, error, bound)
    assert np.all(plus * minus == 0) and np.all(plus >= 0) and np.all(minus >= 0)
    assert np.all(vis[:, 128] == 0)
    want = np.abs(Y).sum(1) / sc.N_BASIS_POINTS
    g_bound = 2 * E.sum(1) / sc.N_BASIS_POINTS                       # the mean of the points' bounds: E_k for k and for 64 + k, 0 for point 128
    e_g = np.abs(gains - want)
    print(f"ERR forward relu pts_dim {pts_dim}: gains {e_g.max():.2e} (bound at that camera {g_bound[e_g.argmax()]:.2e}), worst share {(e_g / g_bound).max():.3f}")
    assert np.all(e_g <= g_bound)


@pytest.mark.parametrize("pts_dim", [3, 4])
def test_forward_sigmoid_one_basis_function_at_a_time(dev, basis_reference, pts_dim):
    """The SCALED path: -log2(e) folded into the table, 1 / (1 + 2^zs).  The sigmoid's slope is at most 1/4; 4 * 2^-24 covers the
    scale's, v_exp_f32's and v_rcp_f32's roundings of a value below 1."""
    from macarons_amd import ops
    Y, E = basis_reference
    pts, harm, cams = (T(a, dev) for a in sc.basis_operands(pts_dim))
    vis = ops.sh_visibilities(pts, harm, cams, use_sigmoid=True)[0].cpu().numpy().astype(np.float64)
    gains = ops.sh_coverage_gain(pts, harm, cams, use_sigmoid=True)[0].cpu().numpy().astype(np.float64)
    tol = E / 4 + 4 * sc.U24
    e_p, e_m = np.abs(vis[:, :64] - sc.sigmoid(Y)), np.abs(vis[:, 64:128] - sc.sigmoid(-Y))
    print(f"ERR forward sigmoid pts_dim {pts_dim}: +e_k {e_p.max():.2e} (share of the bound {(e_p / tol).max():.3f}), -e_k {e_m.max():.2e} ({(e_m / tol).max():.3f})")
    for e in (e_p, e_m):
        bad = np.argwhere(e > tol)
        assert len(bad) == 0, [(int(c), int(sc.L_OF[k]), int(sc.M_OF[k]), e[c, k], tol[c, k]) for c, k in bad[:8]]
    assert np.all(vis[:, 128] == 0.5)
    want = (sc.sigmoid(Y).sum(1) + sc.sigmoid(-Y).sum(1) + 0.5) / sc.N_BASIS_POINTS
    e_g = np.abs(gains - want)
    g_bound = 2 * tol.sum(1) / sc.N_BASIS_POINTS
    print(f"ERR forward sigmoid pts_dim {pts_dim}: gains {e_g.max():.2e}, worst share of the bound {(e_g / g_bound).max():.3f}")
    assert np.all(e_g <= g_bound)


# ---- B. exact operands -----------------------------------------------------------------------------------------------------------------------------
def poisoned_empty(monkeypatch, ops):
    """Every float32 tensor that ops allocates with torch.empty holds -7 (as in tests/test_expansion_layer_gpu.py)."""
    poisoned, real_empty = [], torch.empty

    def empty(*size, **kw):
        if kw.get("dtype") is not torch.float32:
            return real_empty(*size, **kw)
        out = torch.full(*size, -7.0, **kw)
        poisoned.append(out)
        return out

    monkeypatch.setattr(ops.torch, "empty", empty)
    return poisoned


def one_value(x, what):
    """v_rcp_f32(1.0) is expected to be exactly 1; were it not, the entries are compared with the single value it returns."""
    v = np.unique(x)
    assert len(v) == 1, (what, v[:4])
    return v[0]


@pytest.mark.parametrize("B,N,C,wps,edge", sc.EXACT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in sc.EXACT_SHAPES])
def test_exact_operands_bit_for_bit(dev, monkeypatch, B, N, C, wps, edge):
    from macarons_amd import ops
    pts, harm, cams, vis_w, gains_w, record_w, min_abs_z, halves = sc.exact_case(B, N, C)
    assert min_abs_z >= sc.MIN_ABS_Z and halves < 2 ** 24
    p, h, c = T(pts, dev), T(harm, dev), T(cams, dev)
    poisoned = poisoned_empty(monkeypatch, ops)
    vis = ops.sh_visibilities(p, h, c, use_sigmoid=True)
    gains, record = ops.sh_coverage_gain_best(p, h, c, use_sigmoid=True, waves_per_simd=wps)
    plain = ops.sh_coverage_gain(p, h, c, use_sigmoid=True, waves_per_simd=wps)
    monkeypatch.undo()
    assert all(any(q is t for q in poisoned) for t in (vis, gains, record, plain))
    vis, gains, record, plain = (t.cpu().numpy() for t in (vis, gains, record, plain))
    assert vis.shape == (B, C, N) and gains.shape == (B, C) and record.shape == (B, 2)
    assert set(np.unique(vis).tolist()) <= {0.0, 0.5, 1.0}, np.unique(vis)[:8]
    if (vis_w == 1).any():
        high = one_value(vis[vis_w == 1], "saturated high")
        print(f"ERR exact {B}x{N}x{C}: v_rcp_f32(1.0) = {high!r}")
        assert high == 1.0
    wrong = np.argwhere(vis != vis_w)
    print(f"ERR exact {B}x{N}x{C} waves_per_simd {wps} ({edge}): {len(wrong)} visibilities, {(gains != gains_w).sum()} gains differ")
    assert len(wrong) == 0, wrong[:8]
    assert np.array_equal(gains, gains_w), np.argwhere(gains != gains_w)[:8]
    assert np.array_equal(plain, gains_w)
    assert np.array_equal(record, record_w), (record, record_w)


@pytest.mark.parametrize("wps", sc.SAME_BITS_WAVES)
def test_exact_operands_under_every_override(dev, wps):
    from macarons_amd import ops
    B, N, C = sc.SAME_BITS_SHAPE
    pts, harm, cams, vis_w, gains_w, record_w = sc.exact_case(B, N, C)[:6]
    gains, record = ops.sh_coverage_gain_best(T(pts, dev), T(harm, dev), T(cams, dev), use_sigmoid=True, waves_per_simd=wps)
    assert np.array_equal(gains.cpu().numpy(), gains_w) and np.array_equal(record.cpu().numpy(), record_w)


@pytest.mark.parametrize("C", [1, 65, 257])             # 257: the stride loop of the record's kernel and its four-wave merge
@pytest.mark.parametrize("row", ["random", "zeros", "nan", "nan_cameras"])
def test_record_is_best_record_of_the_gains(dev, row, C):
    """The scorer's record and ops.best_record decide by one rule (best_before / wave_best of csrc/wave.h): the record of
    sh_coverage_gain_best equals best_record of sh_coverage_gain's gains on the same inputs, bit for bit, and both say what torch.max
    says on the CPU.  zeros: the second cloud's harmonics are all zero, every camera ties and index 0 wins.  nan: the second cloud's
    harmonics hold a NaN; the first NaN camera wins.  nan_cameras: cameras C // 2 and C - 1 of the second cloud are NaN, so only their
    gains are: a NaN beats every number, and of the two the lower index wins (at C = 257 they sit in different waves and strides)."""
    from macarons_amd import ops
    B, N = 2, 64
    rng = np.random.default_rng(1000 + C)
    pts = rng.uniform(-.5, .5, (B, N, 3)).astype(np.float32)
    harm = (rng.standard_normal((B, N, 64)) * .5).astype(np.float32)
    cams = rng.standard_normal((B, C, 3))
    cams = (1.5 * cams / np.linalg.norm(cams, axis=-1, keepdims=True)).astype(np.float32)
    if row == "zeros":
        harm[1] = 0
    if row == "nan":
        harm[1, 17, 5] = np.nan
    if row == "nan_cameras":
        cams[1, [C // 2, C - 1]] = np.nan
    p, h, c = T(pts, dev), T(harm, dev), T(cams, dev)
    gains_b, record = ops.sh_coverage_gain_best(p, h, c)
    gains = ops.sh_coverage_gain(p, h, c)
    want = ops.best_record(gains)
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    assert np.array_equal(bits(gains_b), bits(gains))
    assert np.array_equal(bits(record), bits(want)), (record, want)
    gains, record = gains.cpu(), record.cpu()
    top = torch.max(gains, dim=1)
    assert np.array_equal(record[:, 0].numpy(), top.values.numpy(), equal_nan=True) and torch.equal(record[:, 1].long(), top.indices)
    if row == "zeros":
        assert bool((gains[1] == gains[1, 0]).all()) and record[1, 1] == 0
    if row == "nan_cameras":
        assert torch.isnan(gains[1]).nonzero().flatten().tolist() == sorted({C // 2, C - 1})
    if row in ("nan", "nan_cameras"):
        first = int(torch.isnan(gains[1]).nonzero()[0])
        assert bool(torch.isnan(record[1, 0])) and record[1, 1] == first and not bool(torch.isnan(gains[0]).any())


def test_exact_operands_relu_and_stride_4(dev):
    """The same split with relu and a point stride of 4: z itself is not exact, its sign is; a zero row gives exactly 0."""
    from macarons_amd import ops
    B, N, C = 3, 130, 200
    pts, harm, cams = sc.exact_operands(B, N, C, pts_dim=4)
    z = sc.exact_z(pts, harm, cams)
    vis = ops.sh_visibilities(T(pts, dev), T(harm, dev), T(cams, dev), use_sigmoid=False).cpu().numpy()
    assert np.array_equal(vis > 0, z > 0) and np.all(vis[z == 0] == 0)
    e = np.abs(vis - np.maximum(z, 0)).max() / np.abs(z).max()
    print(f"ERR exact relu 3x130x200, stride 4: {e:.2e} of the largest |z|")
    assert e <= sc.ROUNDINGS * sc.U24


# ---- C. backward, one basis function at a time ---------------------------------------------------------------------------------------------------
def test_backward_d_harm_one_pair_per_point(dev):
    from macarons_amd import ops
    pts, harm, cams, w, rays = sc.one_camera_per_point(3)
    d_harm = ops.sh_scorer_backward(T(pts, dev), T(harm, dev), T(cams, dev), T(w, dev), True, False, need=(True, False, False))[0]
    got = d_harm[0].cpu().numpy().astype(np.float64)
    err = got - sc.basis(rays)
    ratios = sc.ratio_per_degree(err, rays)
    print(f"ERR backward d_harm, one pair per point: error / (2^-24 max(A, 1)) per l: {fmt(ratios)}; absolute worst {np.abs(err).max():.2e}")
    E = sc.bound(rays)
    bad = np.argwhere(np.abs(err) > E)
    assert len(bad) == 0, [(int(n), int(sc.L_OF[k]), int(sc.M_OF[k]), err[n, k], E[n, k]) for n, k in bad[:8]]        # (point, l, m, error, bound)


def test_backward_d_harm_many_cameras_per_point(dev):
    """A point's 200 cameras are split over several chunks, which the second pass adds: the sum of the basis over the cameras."""
    from macarons_amd import ops
    pts, harm, cams, w, rays = sc.many_cameras_per_point()
    d_harm = ops.sh_scorer_backward(T(pts, dev), T(harm, dev), T(cams, dev), T(w, dev), True, False, need=(True, False, False))[0]
    got = d_harm[0].cpu().numpy().astype(np.float64)
    C, N = rays.shape[:2]
    flat = rays.reshape(C * N, 3)
    want = sc.basis(flat).reshape(C, N, 64).sum(0)
    E = sc.bound(flat).reshape(C, N, 64).sum(0)
    err = np.abs(got - want)
    share = err / E
    print(f"ERR backward d_harm, 200 cameras per point: {err.max():.2e}, worst share of the summed bound per l:",
          fmt([share[:, sc.L_OF == l].max() for l in range(8)]))
    bad = np.argwhere(err > E)
    assert len(bad) == 0, [(int(n), int(sc.L_OF[k]), int(sc.M_OF[k]), err[n, k], E[n, k]) for n, k in bad[:8]]


def per_basis_reference(pts, cams, w):
    """fp64 autograd through autograd.sh_basis: z[k, n] = Y_k(dir_n) + 8 Y_0 for the one pair of point n; (d_pts [64,N,3], d_cams [64,C,3])."""
    from macarons_amd import autograd as A
    c_of = torch.from_numpy(w[0].argmax(0))
    p = torch.from_numpy(pts[0, :, :3]).double()[None].repeat(64, 1, 1).requires_grad_(True)
    c = torch.from_numpy(cams[0]).double()[None].repeat(64, 1, 1).requires_grad_(True)
    rays = c[:, c_of] - p
    Y = A.sh_basis(rays / torch.linalg.norm(rays, dim=-1, keepdim=True))
    z = Y[torch.arange(64), :, torch.arange(64)] + 8 * Y[..., 0]
    assert float(z.detach().min()) > 0                                             # relu is the identity
    z.sum().backward()
    return p.grad.numpy(), c.grad.numpy()


@pytest.mark.parametrize("pts_dim", [3, 4])
def test_backward_direction_gradients_per_basis_function(dev, pts_dim):
    """Cloud k carries harm = e_k + 8 e_0: its d_pts and d_cams are the direction gradients of Y_k alone, each held to TOL_DIR of that
    basis function's own largest gradient.  Y_0 is a constant: cloud 0's gradients are exactly 0."""
    from macarons_amd import ops
    pts, harm, cams, w = sc.per_basis_clouds(pts_dim)
    _, d_pts, d_cams = ops.sh_scorer_backward(T(pts, dev), T(harm, dev), T(cams, dev), T(w, dev), True, False, need=(False, True, True))
    d_pts, d_cams = d_pts.cpu().numpy().astype(np.float64), d_cams.cpu().numpy().astype(np.float64)
    ref_p, ref_c = per_basis_reference(pts, cams, w)
    assert d_pts.shape == pts.shape and np.isfinite(d_pts).all() and np.isfinite(d_cams).all()
    if pts_dim == 4:
        assert np.all(d_pts[..., 3] == 0)
    assert np.all(d_pts[0] == 0) and np.all(d_cams[0] == 0) and not ref_p[0].any() and not ref_c[0].any()
    c_of = w[0].argmax(0)
    worst = np.zeros((3, 64))
    for k in range(1, 64):
        scale_p, scale_c = np.abs(ref_p[k]).max(), np.abs(ref_c[k]).max()
        summed = np.zeros_like(d_cams[k])
        np.add.at(summed, c_of, -d_pts[k, :, :3])
        worst[:, k] = (np.abs(d_pts[k, :, :3] - ref_p[k]).max() / scale_p, np.abs(d_cams[k] - ref_c[k]).max() / scale_c,
                       np.abs(d_cams[k] - summed).max() / scale_c)
    per_l = lambda r: " ".join(f"{r[sc.L_OF == l].max():.1e}" for l in range(1, 8))
    print(f"ERR backward per basis function, pts_dim {pts_dim}, worst per l = 1 .. 7 over the largest gradient of that function: d_pts {per_l(worst[0])};"
          f" d_cams {per_l(worst[1])}; d_cams + sum d_pts {per_l(worst[2])}")
    bad = np.argwhere(worst > TOL_DIR)
    assert len(bad) == 0, [(("d_pts", "d_cams", "d_cams + sum d_pts")[t], int(sc.L_OF[k]), int(sc.M_OF[k]), worst[t, k]) for t, k in bad[:8]]
