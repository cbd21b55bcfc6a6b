"""The cases, expected values and bounds of the scorer's edge tests (tests/_scorer_cases.py), checked on the CPU: the polynomial behind
the bound is the right polynomial, the bound covers the values it bounds, the exact operands saturate with a wide margin, the
vectorised expectation equals a plain loop bit for bit, the library's table is the polynomial forms, and an fp32 emulation of the
documented operation order meets the bound with a margin (so it is not a bound that only the kernel as built could meet; the reference's
C port does not meet it, for a stated reason).  Prints (with -s) the reference-alone figures."""
import numpy as np
import pytest

from conftest import golden
from oracle import sh

import _scorer_cases as sc


def test_direction_set_is_what_it_is_called():
    D = sc.directions()
    assert D.dtype == np.float32 and D.shape == (274, 3) and not D.flags.writeable
    assert sc.directions() is D
    r = np.sqrt((D.astype(np.float64) ** 2).sum(-1))
    assert r.min() >= 1.0 - 1e-6 and r.max() <= 2.0 + 1e-6
    n = D / r[:, None]
    rho = np.hypot(n[:, 0], n[:, 2])
    poles, equator, axes, octants = n[200:240], n[240:260], D[260:266], D[266:]
    assert rho[200:240].max() < 0.1 and rho[200:240].min() < 1e-6 and (poles[:, 1] > 0).any() and (poles[:, 1] < 0).any()
    assert np.abs(equator[:, 1]).max() < 1e-5 and np.abs(equator[:, 1]).min() > 0
    assert sorted(map(tuple, axes.tolist())) == sorted([(1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0), (0, -1.5, 0), (0, 0, 1.5), (0, 0, -1.5)])
    assert np.all(np.abs(octants) == 1.0) and len({tuple(o) for o in octants.tolist()}) == 8


def test_polynomial_form_is_the_oracles_basis():
    """The signed form whose term magnitudes make A reproduces oracle.sh.sh_basis_trigfree on D and on random rays, and the reference's
    own Y_f64 golden on its angle grid, to 1e-12; and the oracle's trig-free form equals its literal trig form away from the poles."""
    D = sc.directions().astype(np.float64)
    rays = np.concatenate([D, np.random.default_rng(1).standard_normal((2000, 3))])
    e = np.abs(sc.sh_basis_polynomial(rays) - sc.basis(rays)).max()
    g = golden("sh_basis")
    th, ph = g["theta"], g["phi"]
    grid = np.stack([np.sin(th) * np.sin(ph), np.cos(th), np.sin(th) * np.cos(ph)], axis=1)
    e_g = np.abs(sc.sh_basis_polynomial(grid) - g["Y_f64"]).max()
    e_t = np.abs(sc.basis(grid) - g["Y_f64"]).max()
    away = np.abs(rays[:, 1]) < 0.99 * np.linalg.norm(rays, axis=1)
    _, elev, azim = sh.spherical_coords(rays[away])
    e_l = np.abs(sh.sh_basis_literal(np.pi / 2 - elev, azim, np.float64) - sc.basis(rays[away])).max()
    print(f"ERR polynomial form vs trig-free oracle {e:.2e}, vs Y_f64 {e_g:.2e}; trig-free vs Y_f64 {e_t:.2e}, vs literal {e_l:.2e}")
    assert e < 1e-12 and e_g < 1e-12 and e_t < 1e-12 and e_l < 1e-11


def test_sum_of_magnitudes_covers_the_basis():
    D = sc.directions()
    A, Y = sc.sum_of_magnitudes(D), sc.basis(D)
    assert np.all(A >= np.abs(Y) - 1e-13)
    assert np.all(A[:, 0] == A[0, 0]) and abs(A[0, 0] - 0.28209479177387814) < 1e-15
    per_l = [float(A[:, sc.L_OF == l].max()) for l in range(8)]
    print("ERR largest A over D per l:", " ".join(f"{v:.1f}" for v in per_l), "; largest |Y|", f"{np.abs(Y).max():.3f}")
    assert 50 < max(per_l) < 200 and per_l == sorted(per_l)             # about 100, at l = 7
    E = sc.bound(D)
    assert E.min() == sc.ROUNDINGS * sc.U24 and E.max() == sc.ROUNDINGS * sc.U24 * max(per_l) and sc.ROUNDINGS <= 64


def test_basis_operands():
    for P in (3, 4):
        pts, harm, cams = sc.basis_operands(P)
        assert pts.shape == (1, 129, P) and not pts.any() and np.array_equal(cams[0], sc.directions())
        assert np.array_equal(harm[0, :64], np.eye(64, dtype=np.float32)) and np.array_equal(harm[0, 64:128], -np.eye(64, dtype=np.float32))
        assert not harm[0, 128].any()


@pytest.mark.parametrize("B,N,C,wps,edge", sc.EXACT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in sc.EXACT_SHAPES])
def test_exact_shapes_saturate(B, N, C, wps, edge):
    """Every listed shape: lattice operands, |z| >= 256 on the non-zero rows, sums below 2^24 halves, all three visibility values and
    (from two cameras on) tied gains."""
    pts, harm, cams, vis, gains, record, min_abs_z, halves = sc.exact_case(B, N, C)
    assert sc.exact_case(B, N, C)[0] is pts and not vis.flags.writeable
    assert np.array_equal(pts * 16, np.round(pts * 16)) and np.abs(pts).max() <= 0.5
    odd = (cams * 32).astype(np.int64)
    assert np.array_equal(cams * 32, odd) and np.all(odd % 2 != 0)
    nz = harm != 0
    assert np.all(nz.sum(-1) <= 1) and np.all(np.abs(harm[nz]) == sc.SATURATING) and not nz[..., 0].any() and not nz[..., 4:].any()
    assert np.array_equal(~nz.any(-1), np.broadcast_to(np.arange(N) % 5 == 4, (B, N)))
    print(f"ERR exact {B}x{N}x{C} ({edge}): U = {sc.units(B, N, C)}, min |z| = {min_abs_z:.0f}, largest sum {halves:.0f} halves")
    assert min_abs_z >= sc.MIN_ABS_Z and halves < 2 ** 24
    assert set(np.unique(vis).tolist()) <= {0.0, 0.5, 1.0}
    if N >= 5:
        assert set(np.unique(vis).tolist()) == {0.0, 0.5, 1.0}
    # the fp64 z of the case file is the oracle's: the full basis on a sample of the pairs
    b, c = B - 1, C - 1
    n = np.unique(np.concatenate([np.arange(min(N, 70)), np.arange(max(0, N - 70), N)]))
    Y = sc.basis(cams[b, c].astype(np.float64)[None] - pts[b, n, :3].astype(np.float64))
    assert np.abs((Y * harm[b, n]).sum(-1) - sc.exact_z(pts, harm, cams)[b, c, n]).max() < 1e-9
    if C >= 2:
        assert np.array_equal(gains[:, C // 2:2 * (C // 2)], gains[:, :C // 2])
        tied = [(gains[k] == record[k, 0]).sum() > 1 for k in range(B)]
        assert any(tied) and all(record[k, 1] == np.flatnonzero(gains[k] == record[k, 0])[0] for k in range(B))


def test_exact_shape_list_is_the_stated_one():
    assert [s[:4] for s in sc.EXACT_SHAPES] == [(1, 1, 1, 0), (2, 63, 3, 0), (2, 64, 1, 0), (3, 65, 7, 1), (3, 130, 200, 1),
                                                (2, 44801, 2, 1), (1, 16449, 3, 0), (3, 2561, 150, 0)]
    U = {s[:3]: sc.units(*s[:3]) for s in sc.EXACT_SHAPES}
    assert U[(3, 130, 200)] == 1800 and U[(2, 44801, 2)] == 2804 and U[(3, 2561, 150)] == 18450 > 256 * 4 * 8 * 2
    assert 2804 / 1024 > 2 and -(-16449 // 64) == 258 and 16449 % 64 == 1 and 65 % 64 == 1
    assert sc.SAME_BITS_SHAPE == (3, 130, 200) and sc.SAME_BITS_WAVES == (2, 3, 8)


@pytest.mark.parametrize("B,N,C", [s[:3] for s in sc.EXACT_SHAPES[:3]])
def test_expected_gains_from_a_plain_loop(B, N, C):
    """The smallest three shapes, pair by pair through the oracle's full basis, give the vectorised expectation bit for bit."""
    pts, harm, cams, vis, gains, record = sc.exact_case(B, N, C)[:6]
    for b in range(B):
        best, best_c = None, None
        for c in range(C):
            halves = 0
            for n in range(N):
                ray = cams[b, c].astype(np.float64) - pts[b, n, :3].astype(np.float64)
                z = float((sc.basis(ray[None])[0] * harm[b, n].astype(np.float64)).sum())
                v = 0.5 if not harm[b, n].any() else (1.0 if z > 0 else 0.0)
                assert vis[b, c, n] == np.float32(v)
                halves += int(2 * v)
            g = np.float32(halves / 2.0) * (np.float32(1.0) / np.float32(N))
            assert g.dtype == np.float32 and gains[b, c] == g
            if best is None or g > best:
                best, best_c = g, c
        assert record[b, 0] == best and record[b, 1] == np.float32(best_c)


def test_backward_operands():
    pts, harm, cams, w, rays = sc.one_camera_per_point(4)
    N, C = sc.N_BWD, cams.shape[1]
    assert N > 64 and N % 64 and N > C and pts.shape == (1, N, 4) and np.array_equal(cams[0], sc.directions())
    assert np.all(w.sum(1) == 1) and np.all(w[0, np.arange(N) % C, np.arange(N)] == 1)
    assert np.all(harm[..., 0] == 8) and not harm[..., 1:].any()
    assert np.array_equal(rays, (cams[0, np.arange(N) % C] - pts[0, :, :3]).astype(np.float64))
    z = 8 * sc.basis(rays)[:, 0]
    assert abs(z[0] - 2.2567583341910251) < 1e-12 and np.all(z == z[0])
    pts, harm, cams, w, rays = sc.many_cameras_per_point()
    assert pts.shape == (1, 65, 3) and cams.shape == (1, 200, 3) and np.all(w == 1) and rays.shape == (200, 65, 3)
    assert np.array_equal(cams[0, -74:], sc.directions()[-74:])
    pts, harm, cams, w = sc.per_basis_clouds(3)
    assert harm.shape == (64, N, 64) and np.all(harm[0, :, 0] == 9) and np.all(harm[5, :, 5] == 1) and np.all(harm[5, :, 0] == 8)
    assert np.all(harm.sum(-1) == 9) and np.all((harm != 0).sum(-1) <= 2)
    # relu stays the identity with the basis function added: z = Y_k + 2.26 > 0 for every pair
    Y = sc.basis(sc.one_camera_per_point(3)[4])
    assert (Y + 8 * Y[:, :1]).min() > 0.5


def _sh_mono_of_the_library():
    """SH_MONO[m][l][k] as written in macarons_amd/csrc/sh_consts.inc (the text of the table, not the library)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "macarons_amd", "csrc", "sh_consts.inc")
    with open(path) as f:
        txt = f.read().split("SH_MONO[8][8][8]")[1]
    vals = [float(v) for v in re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f", txt)]
    assert len(vals) == 512
    return np.array(vals).reshape(8, 8, 8)


def test_library_table_is_the_polynomial_forms():
    """Every entry of SH_MONO equals K_lm (-1)^m c_{l,m,j} from numpy.polynomial.legendre to a relative 1e-12 (the table is written in
    fp64 digits and rounded to fp32 by the compiler), zeros where the form has none: 70 non-zero entries (120 counting
    the cos and sin channels of m != 0 apart, as the transform's products do)."""
    lib, want = _sh_mono_of_the_library(), sc.mono_table()
    assert np.count_nonzero(want) == 70 and 2 * 70 - np.count_nonzero(want[0]) == 120 and np.array_equal(lib != 0, want != 0)
    nz = want != 0
    assert np.abs(lib[nz] / want[nz] - 1).max() < 1e-12


def test_fp32_emulation_meets_the_forward_bound():
    """sh_mono.h's documented operation order, emulated on the CPU with the library's own table (each product-and-add in fp64, then
    rounded to fp32; v_rsq_f32 taken as correctly rounded, the one instruction this does not model): an emulation, not a measurement
    on a GPU.  On D it stays below 8.4 * 2^-24 max(A, 1), which is the margin of ROUNDINGS = 32: a factor of 3.8."""
    D = sc.directions()
    err = sc.emulate_basis_fp32(D, _sh_mono_of_the_library()) - sc.basis(D)
    ratios = sc.ratio_per_degree(err, D)
    print("ERR fp32 emulation, error / (2^-24 max(A, 1)) per l:", " ".join(f"{r:.2f}" for r in ratios), f"; absolute worst {np.abs(err).max():.2e}")
    assert np.all(np.abs(err) <= sc.bound(D)) and max(ratios) <= 8.4


def test_c_port_against_the_forward_bound():
    """The reference's C port (relu visibilities) on the operands of section A, away from the poles (|n_y| < 0.99).  It does NOT stay
    within E_k: it restates upstream's fp32 asin -> cos -> acos -> cos(m azimuth) chain, and acos is as ill-conditioned at azimuth 0
    and pi (n_x = 0, every m != 0 term times m) as asin is at the poles.  Measured, error / (2^-24 max(A, 1)) per l = 0 .. 7:
    0.25 94 204 326 290 404 472 562, 4.6e-5 absolute at worst, i.e. up to 17.6 times the bound.  So the bound's margin is stated against
    the fp32 emulation alone (test_fp32_emulation_meets_the_forward_bound): 32 against 8.4.  What is asserted here is the part of the
    C port that the conditioning does not touch: the m = 0 channels, polynomials in n_y = sin(asin(n_y)) alone, stay within E_k."""
    from oracle import cport
    pts, harm, cams = sc.basis_operands(3)
    D = sc.directions().astype(np.float64)
    away = np.abs(sc._unit(D)[:, 1]) < 0.99
    vis = cport.visibilities(pts, harm, cams, use_sigmoid=False)[0].astype(np.float64)
    err = (vis[:, :64] - vis[:, 64:128]) - sc.basis(D)
    ratios = sc.ratio_per_degree(err[away], D[away])
    zonal = sc.M_OF == 0
    print("ERR C port, |n_y| < 0.99, error / (2^-24 max(A, 1)) per l:", " ".join(f"{r:.2f}" for r in ratios),
          f"; absolute worst {np.abs(err[away]).max():.2e}; at the poles {np.abs(err[~away]).max():.2e}; m = 0 channels alone",
          f"{(np.abs(err[away]) / sc.bound(D[away]))[:, zonal].max() * sc.ROUNDINGS:.2f}")
    assert away.sum() > 200 and np.all(vis[:, 128] == 0) and np.isfinite(err).all()
    assert np.all(np.abs(err[away][:, zonal]) <= sc.bound(D[away])[:, zonal])
