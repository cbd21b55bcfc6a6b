"""Cases, expected values and error bounds of the scorer's edge tests (tests/test_scorer_edges_gpu.py), host only: numpy and oracle.sh,
neither torch nor the library, so everything here is checked without a GPU (tests/test_scorer_cases_cpu.py).

A. One basis function at a time.  One cloud of 129 points at the origin (rays = cams exactly): point k carries harm = +e_k, point
   64 + k carries -e_k, point 128 zeros.  The cameras are the direction set D: random directions, directions near the poles and the
   equator, the axes and the octant diagonals.  The expected value is the fp64 basis Y_k(d) of oracle.sh.sh_basis_trigfree.
   The bound is derived, not measured:  E_k(d) = ROUNDINGS * 2^-24 * max(A_k(d), 1), where
       A_{l,+-m}(d) = K_lm * sum_j |c_{l,m,j}| |n_y|^j * (n_x^2 + n_z^2)^(m/2)
   is the sum of the magnitudes of the monomial terms that sh_mono.h adds (c_{l,m,.}: the monomial coefficients of d^m P_l / dx^m from
   numpy.polynomial.legendre; K_lm: the real-SH normalisation), and ROUNDINGS = 32 is at least the number of roundings on the longest
   path of sh_mono.h (coefficient transform 4, Horner in x 7, six complex steps 12, last real part 2, normalisation 3 = 28).
B. Exact operands.  Points on the lattice j/16, cameras on j/16 + 1/32, one coefficient of +-2^17 in an l = 1 channel per point (every
   fifth point zeros): the sigmoid saturates, every visibility is exactly 0, 0.5 or 1, every sum is exact in fp32, and the gains and
   the arg-max record are known bit for bit.  The second half of a cloud's cameras repeats the first half, so that the largest gain
   is (almost always) tied and the record's "ties go to the lower index" is exercised.
C. Backward, one basis function at a time: operands and the same bound E_k for d_harm.
"""
import functools
import math

import numpy as np
from numpy.polynomial import Polynomial
from numpy.polynomial.legendre import Legendre

from oracle import sh

MAX_RANK = sh.MAX_RANK
U24 = 2.0 ** -24
ROUNDINGS = 32                       # see the module docstring; the issue's ceiling without a found cause is 64
L_OF = np.array([l for l in range(MAX_RANK) for _ in range(2 * l + 1)])       # degree of channel k = l*l + l + m
M_OF = np.array([m for l in range(MAX_RANK) for m in range(-l, l + 1)])       # order of channel k


def _frozen(a):
    a.flags.writeable = False
    return a


# ---- the polynomial form behind A ----------------------------------------------------------------------------------------------------------
def sh_k(l, m_abs):
    """K_lm: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), times sqrt(2) for m != 0."""
    k = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m_abs) / math.factorial(l + m_abs))
    return k * math.sqrt(2.0) if m_abs else k


@functools.lru_cache(maxsize=None)
def legendre_deriv_coeffs(l, m_abs):
    """c_{l,m,j}, j = 0 .. l-m: d^m P_l / dx^m = sum_j c_j x^j (fp64)."""
    p = Legendre.basis(l)
    if m_abs:
        p = p.deriv(m_abs)
    c = p.convert(kind=Polynomial).coef
    return tuple(float(v) for v in c)


def _unit(d):
    d = np.asarray(d, np.float64)
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def sh_basis_polynomial(d):
    """The signed form: Y_{l,+-m}(d) = K_lm (-1)^m (sum_j c_j n_y^j) {Re, Im} (n_z + i n_x)^m, fp64, d [K,3] -> [K,64].
    P_l^m(x) = (-1)^m (1 - x^2)^(m/2) d^m P_l / dx^m (Condon-Shortley) and sin^m(polar) e^(i m azimuth) = (n_z + i n_x)^m."""
    n = _unit(d)
    w = n[:, 2] + 1j * n[:, 0]
    out = np.empty((n.shape[0], MAX_RANK * MAX_RANK))
    for l in range(MAX_RANK):
        for m in range(l + 1):
            c = legendre_deriv_coeffs(l, m)
            poly = sum(cj * n[:, 1] ** j for j, cj in enumerate(c))
            wm = w ** m
            out[:, l * l + l + m] = sh_k(l, m) * (-1) ** m * poly * wm.real
            if m:
                out[:, l * l + l - m] = sh_k(l, m) * (-1) ** m * poly * wm.imag
    return out


def sum_of_magnitudes(d):
    """A_k(d) [K,64]: the magnitudes of the same terms added, with |{Re, Im} w^m| replaced by |w|^m."""
    n = _unit(d)
    rho2 = n[:, 0] ** 2 + n[:, 2] ** 2
    out = np.empty((n.shape[0], MAX_RANK * MAX_RANK))
    for l in range(MAX_RANK):
        for m in range(l + 1):
            c = legendre_deriv_coeffs(l, m)
            a = sh_k(l, m) * sum(abs(cj) * np.abs(n[:, 1]) ** j for j, cj in enumerate(c)) * rho2 ** (m / 2)
            out[:, l * l + l + m] = a
            out[:, l * l + l - m] = a
    return out


def bound(d):
    """E_k(d) [K,64] = ROUNDINGS * 2^-24 * max(A_k(d), 1)."""
    return ROUNDINGS * U24 * np.maximum(sum_of_magnitudes(d), 1.0)


def basis(d):
    """The expected values: oracle.sh.sh_basis_trigfree in fp64."""
    return sh.sh_basis_trigfree(np.asarray(d, np.float64), np.float64)


def ratio_per_degree(err, d):
    """max over directions and orders of |err| / (2^-24 max(A, 1)), one figure per l: what the docstrings record."""
    r = np.abs(err) / (U24 * np.maximum(sum_of_magnitudes(d), 1.0))
    return [float(r[:, L_OF == l].max()) for l in range(MAX_RANK)]


# ---- the documented fp32 operation order of sh_mono.h, emulated (every product-and-add in fp64, then rounded once to fp32) ----------------
def mono_table():
    """MONO[m][l][j] = K_lm (-1)^m c_{l,m,j} in fp64: what SH_MONO of sh_consts.inc holds, rounded to fp32."""
    t = np.zeros((MAX_RANK, MAX_RANK, MAX_RANK))
    for l in range(MAX_RANK):
        for m in range(l + 1):
            c = legendre_deriv_coeffs(l, m)
            t[m, l, :len(c)] = sh_k(l, m) * (-1) ** m * np.array(c)
    return t


def _r(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _fma(a, b, c):
    return _r(a * b + c)


def emulate_basis_fp32(d, table=None):
    """z of sh_dot for harm = e_k, every k: d [K,3] float32 -> [K,64] (fp32 values held in fp64).  The coefficient transform of e_k is
    the table's row; then Horner in x = n_y, the complex Horner steps in w = n_z + i n_x and the last real part, in sh_dot's order.
    v_rsq_f32 is modelled as a correctly rounded 1 / sqrt."""
    t = _r(mono_table() if table is None else table)
    d = np.asarray(d, np.float32).astype(np.float64)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ir = _r(1.0 / np.sqrt(_fma(dz, dz, _fma(dy, dy, _r(dx * dx)))))
    nx, ct, nz = _r(dx * ir), _r(dy * ir), _r(dz * ir)
    zero = np.zeros_like(ct)
    out = np.empty((d.shape[0], MAX_RANK * MAX_RANK))
    for l in range(MAX_RANK):
        for m in range(l + 1):
            p = zero + t[m, l, MAX_RANK - 1 - m]                       # the chain starts at a[shk(7, m)]: power 7 - m
            for j in range(MAX_RANK - 2 - m, -1, -1):
                p = _fma(ct, p, t[m, l, j])
            if m == 0:
                out[:, l * l + l] = _fma(nz, zero, _fma(nx, zero, p))
                continue
            for sign in (1, -1):
                ar, bi = (p, zero) if sign > 0 else (zero, p)          # A_m = P_m = U_m - i V_m
                for _ in range(m - 1):
                    ar, bi = _fma(ar, nz, _fma(bi, nx, zero)), _fma(bi, nz, _fma(-ar, nx, zero))
                out[:, l * l + l + sign * m] = _fma(nz, ar, _fma(nx, bi, zero))
    return out


# ---- the direction set D ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def directions():
    """D [274,3] float32, lengths in [1, 2]: 200 random directions, 40 near the poles (x and z scaled by 1e-2, 1e-4, 1e-7), 20 near the
    equator (y scaled by 1e-6), the six axis directions exactly, the eight octant diagonals."""
    rng = np.random.default_rng(20260)
    rand = _unit(rng.standard_normal((200, 3)))
    poles = _unit(rng.standard_normal((40, 3)))
    poles[:, [0, 2]] *= np.array([1e-2, 1e-4, 1e-7])[np.arange(40) % 3, None]
    poles[:, 1] = np.where(np.arange(40) % 2, -1.0, 1.0) * np.maximum(np.abs(poles[:, 1]), 0.1)           # both poles
    equator = _unit(rng.standard_normal((20, 3)))
    equator[:, 1] *= 1e-6
    lengths = rng.uniform(1.0, 2.0, 260)[:, None]
    body = np.concatenate([rand, _unit(poles), _unit(equator)]) * lengths
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 1.5
    octants = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)      # length sqrt(3)
    return _frozen(np.concatenate([body, axes, octants]).astype(np.float32))


N_BASIS_POINTS = 129


def basis_operands(pts_dim):
    """Section A: (pts [1,129,pts_dim] zeros, harm [1,129,64], cams [1,|D|,3] = D)."""
    harm = np.zeros((1, N_BASIS_POINTS, 64), np.float32)
    harm[0, np.arange(64), np.arange(64)] = 1.0
    harm[0, 64 + np.arange(64), np.arange(64)] = -1.0
    return np.zeros((1, N_BASIS_POINTS, pts_dim), np.float32), harm, directions()[None].copy()


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---- B: exact operands ---------------------------------------------------------------------------------------------------------------------------
# (B, N, C, waves_per_simd of the gains (0: the default), the edge)
EXACT_SHAPES = (
    (1, 1, 1, 0, "one unit"),
    (2, 63, 3, 0, "a single tile, ragged"),
    (2, 64, 1, 0, "a full tile, one camera"),
    (3, 65, 7, 1, "a last tile of one point"),
    (3, 130, 200, 1, "U = 1800 over W = 1024 waves: ranges start mid-camera-range and cross tiles and clouds"),
    (2, 44801, 2, 1, "U = 2804: a wave's range exceeds C, so it walks whole tiles and a cloud boundary"),
    (1, 16449, 3, 0, "258 wave-tiles: the reduce's strided loop runs twice and the last tile holds one point"),
    (3, 2561, 150, 0, "U = 18450, above any possible resident count (256 x 4 x 8 x 2): W < U for the visibilities"),
)
SAME_BITS_SHAPE = (3, 130, 200)              # at waves_per_simd 2, 3 and 8: the bits of waves_per_simd = 1
SAME_BITS_WAVES = (2, 3, 8)
SATURATING = 2.0 ** 17
MIN_ABS_Z = 256.0                            # asserted over the non-zero rows; fp32 needs 89 for 2^zs to reach infinity
K1 = math.sqrt(3.0 / (4.0 * math.pi))        # Y_{1,-1} = -K1 n_x,  Y_{1,0} = K1 n_y,  Y_{1,1} = -K1 n_z


def units(B, N, C):
    return B * (-(-N // 64)) * C


def exact_operands(B, N, C, pts_dim=3):
    """(pts [B,N,pts_dim], harm [B,N,64], cams [B,C,3]) float32.  pts on j/16 (j = -8 .. 8), cams on j/16 + 1/32 (j = -24 .. 23), so
    every coordinate difference is an odd multiple of 1/32; cameras C//2 .. 2 (C//2) - 1 of a cloud repeat cameras 0 .. C//2 - 1."""
    rng = np.random.default_rng(1000003 * B + 1009 * N + C)
    pts = np.zeros((B, N, pts_dim), np.float32)
    pts[..., :3] = rng.integers(-8, 9, (B, N, 3)) / 16.0
    if pts_dim > 3:
        pts[..., 3:] = rng.integers(1, 9, (B, N, pts_dim - 3)) / 8.0          # never read by the scorer
    cams = (rng.integers(-24, 24, (B, C, 3)) / 16.0 + 1.0 / 32.0).astype(np.float32)
    h = C // 2
    cams[:, h:2 * h] = cams[:, :h]
    n, b = np.arange(N)[None, :], np.arange(B)[:, None]
    chan = 1 + (n + b) % 3
    sign = np.where((n // 3) % 2 == 0, 1.0, -1.0) * np.ones((B, 1))
    sign[:, np.arange(N) % 5 == 4] = 0.0
    harm = np.zeros((B, N, 64), np.float32)
    np.put_along_axis(harm, chan[..., None], (sign * SATURATING).astype(np.float32)[..., None], axis=2)
    return pts, harm, cams


def exact_z(pts, harm, cams):
    """fp64 z [B,C,N] of exact_operands: only the l = 1 channels are occupied, z = K1 (-n_x h_1 + n_y h_2 - n_z h_3)."""
    d = cams.astype(np.float64)[:, :, None, :] - pts.astype(np.float64)[:, None, :, :3]
    n = d / np.sqrt((d * d).sum(-1, keepdims=True))
    h = harm.astype(np.float64)[:, None, :, 1:4]
    return K1 * (-n[..., 0] * h[..., 0] + n[..., 1] * h[..., 1] - n[..., 2] * h[..., 2])


def exact_expected(pts, harm, cams):
    """(vis [B,C,N] float32 in {0, 0.5, 1}, gains [B,C] float32, record [B,2] float32, min |z| over the non-zero rows, the largest sum in
    halves).  gains = float32(S) * (float32(1) / float32(N)), the expression of sh_reduce_kernel; record = (max, first arg-max)."""
    z = exact_z(pts, harm, cams)
    zero_row = ~harm.any(-1)[:, None, :]
    vis = np.where(z > 0, 1.0, 0.0)
    vis = np.where(zero_row & (z == 0), 0.5, vis).astype(np.float32)
    live = np.abs(z)[np.broadcast_to(~zero_row, z.shape)]
    min_abs_z = float(live.min()) if live.size else math.inf
    S = vis.astype(np.float64).sum(-1)                                            # multiples of 0.5: exact
    gains = (S.astype(np.float32) * (np.float32(1.0) / np.float32(pts.shape[1]))).astype(np.float32)
    idx = np.argmax(gains, axis=1)                                                # the first of equal maxima
    record = np.stack([gains[np.arange(len(idx)), idx], idx.astype(np.float32)], axis=1).astype(np.float32)
    return vis, gains, record, min_abs_z, float(2.0 * S.max())


@functools.lru_cache(maxsize=None)
def exact_case(B, N, C):
    """The operands and expected values of one shape, computed once and never changed."""
    ops = exact_operands(B, N, C)
    return tuple(_frozen(a) for a in ops) + tuple(_frozen(a) if isinstance(a, np.ndarray) else a for a in exact_expected(*ops))


# ---- C: backward -----------------------------------------------------------------------------------------------------------------------------------
N_BWD = 301                                  # > 64 points, a ragged last tile (45), and more points than directions in D


def lattice_points(N, pts_dim, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros((1, N, pts_dim), np.float32)
    pts[..., :3] = rng.integers(-8, 9, (1, N, 3)) / 16.0
    if pts_dim > 3:
        pts[..., 3:] = rng.integers(1, 9, (1, N, pts_dim - 3)) / 8.0
    return pts


def rays_f32(pts, cams):
    """cams - pts as the kernel forms it: one fp32 subtraction per coordinate.  [C,N,3] of the first cloud, as fp64."""
    return (cams[0][:, None, :] - pts[0][None, :, :3]).astype(np.float32).astype(np.float64)


def one_camera_per_point(pts_dim=3):
    """d_harm, one pair per point: harm = 8 e_0 (z = 2.26: relu is the identity), w[c, n] = 1 where c == n % C.
    Returns (pts, harm, cams, w [1,C,N], rays [N,3] fp64 of the chosen pairs)."""
    cams = directions()[None].copy()
    C = cams.shape[1]
    pts = lattice_points(N_BWD, pts_dim, 77)
    harm = np.zeros((1, N_BWD, 64), np.float32)
    harm[..., 0] = 8.0
    n = np.arange(N_BWD)
    w = np.zeros((1, C, N_BWD), np.float32)
    w[0, n % C, n] = 1.0
    return pts, harm, cams, w, rays_f32(pts, cams)[n % C, n]


def many_cameras_per_point():
    """d_harm, N = 65 points and the last 200 directions of D (126 random ones and every special one), w = 1 everywhere.
    Returns (pts, harm, cams, w, rays [C,N,3] fp64)."""
    cams = directions()[None, -200:].copy()
    pts = lattice_points(65, 3, 78)
    harm = np.zeros((1, 65, 64), np.float32)
    harm[..., 0] = 8.0
    return pts, harm, cams, np.ones((1, 200, 65), np.float32), rays_f32(pts, cams)


def per_basis_clouds(pts_dim):
    """d_pts and d_cams per basis function: cloud k of 64 carries harm = e_k + 8 e_0 (cloud 0: 9 e_0); the points, cameras and weights
    of one_camera_per_point in every cloud."""
    pts, harm, cams, w, _ = one_camera_per_point(pts_dim)
    harm = np.repeat(harm, 64, axis=0)
    harm[np.arange(64), :, np.arange(64)] += 1.0
    return np.repeat(pts, 64, axis=0), harm, np.repeat(cams, 64, axis=0), np.repeat(w, 64, axis=0)
