"""numpy restatement of what the existing host models do not cover of the decision-glue kernels (csrc/glue.hip), for
tests/test_decision_glue_gpu.py.  TEST INFRASTRUCTURE ONLY.

What is reused, not restated: oracle/view_state.py (sample_proxy_points(exact=True), compute_view_state, view_state_indices,
bin_boundary_margin), oracle/macarons_regime.py (points_in_fov), oracle/scene.py (ndc_tabs; its unproject_depth mixes fp32 and fp64 and
is neither the fp32 restatement nor the fp64 reference needed here), tests/_frames_model.py (signed_distance, update_frames).  Every function here that has such an oracle returns the ORACLE's value, or a restatement that is
asserted equal to it on the spot, whenever PERTURB is empty: the restatements exist to say which branch of a kernel an input reaches
and to carry the planted mistakes below.

  sample_proxy          the sampler as the kernels run it: 256-point block sums (wave butterfly, then (s0 + s1) + (s2 + s3)), the
                        Hillis-Steele scan of the block sums in rounds of 256 with a carry, per sample the binary search on the
                        exclusive offsets, the in-block wave scan, the walk to later blocks and the backward walk; fp64 additions in
                        the kernels' order, so the trace (which walk a sample took) holds for real-valued occupancies too
  points_in_fov, signed_distance, proxy_update, view_state_indices / compute_view_state
                        the oracles above, behind the switch
  transform_points, unproject_depth, macarons_gain, coverage_gain_multiple, torch_max_rows
                        fp32 restatements in the kernels' order / fp64 references

PERTURB (a set of names, empty in every test) switches ONE documented mistake into the model: the sensitivity record of the suite --
which test notices which mistake -- is made by running the GPU tests with one name set (env GLUE_MODEL_PERTURB).  Neither a kernel
nor the package reads it.  Names:
  admit_nonstrict     the sampler keeps occ >= min_occ                     (kernel and upstream: occ > min_occ)
  cdf_strict          a sample picks the first i with C_i > u C_last       (>=)
  carry_dropped       the block-offset scan forgets its carry after the first 256 block sums
  ndc_exclusive       the frustum's max_x bound is exclusive               (all four are inclusive)
  border_tap          the east tap of the bilinear sample is not skipped at ix1 == W (it reads the next row's first pixel)
  tol_sign            n_behind counts d >= tol                             (d >= -tol)
  elev_ge             the elevation index rounds up at mod >= half a step  (>)
  cartesian_reversed  camera tuples with the FIRST index fastest           (torch.cartesian_prod: the last)
  last_nan            of two NaN gains the last one wins the arg-max       (torch.max: the first)
"""
import os

import numpy as np

import _frames_model as FM
from oracle import macarons_regime as R
from oracle import scene as S
from oracle import sh
from oracle import view_state as V

F = np.float32
PERTURB = set(os.environ.get("GLUE_MODEL_PERTURB", "").split())
KNOWN = {"admit_nonstrict", "cdf_strict", "carry_dropped", "ndc_exclusive", "border_tap", "tol_sign", "elev_ge", "cartesian_reversed",
         "last_nan"}
assert PERTURB <= KNOWN, PERTURB - KNOWN

SMP_BLOCK = 256


def is_dyadic(a, bits):
    """Every value is an integer multiple of 2^-bits."""
    a = np.asarray(a, np.float64) * float(2 ** bits)
    return bool(np.all(a == np.round(a)))


# ---- sampler ------------------------------------------------------------------------------------------------------------------------
def _hillis_steele(s):
    """Inclusive scan along the last axis in the kernels' order: s[i] += s[i - o] for o = 1, 2, 4, ..."""
    s = s.copy()
    o = 1
    while o < s.shape[-1]:
        t = np.zeros_like(s)
        t[..., o:] = s[..., :-o]
        s = s + t
        o <<= 1
    return s


class SamplerTrace:
    """What the search did per sample: the block the binary search chose, the block the pick was found in (-1: none), whether the
    loop moved past its first block, whether the backward walk ran."""

    def __init__(self, n):
        self.lo = np.zeros(n, np.int64)
        self.found_in = np.full(n, -1, np.int64)
        self.moved_on = np.zeros(n, bool)
        self.backward = np.zeros(n, bool)


def sampler_scan(occ, min_occ):
    """-> (kept [nb,256] bool, cum [nb,256] fp64 = what `base + v[e]` is at every position, off [nb] exclusive block offsets, total)."""
    occ = np.asarray(occ, F).reshape(-1)
    P = len(occ)
    nb = -(-P // SMP_BLOCK)
    o = np.zeros(nb * SMP_BLOCK, F)
    o[:P] = occ
    valid = np.arange(nb * SMP_BLOCK) < P
    kept = valid & ((o >= F(min_occ)) if "admit_nonstrict" in PERTURB else (o > F(min_occ)))
    w = np.where(kept, o.astype(np.float64), 0.0)
    # smp_block_sums: thread t of a chunk holds occupancy t; a wave's butterfly, then the four wave sums as (s0 + s1) + (s2 + s3)
    v = w.reshape(nb, 4, 64)
    h = 32
    while h > 0:
        v = v[..., :h] + v[..., h:2 * h]
        h >>= 1
    bs = (v[:, 0, 0] + v[:, 1, 0]) + (v[:, 2, 0] + v[:, 3, 0])
    # the last block's scan: rounds of 256 block sums, `carry + s - x`, carry += s[255]
    off = np.zeros(nb, np.float64)
    carry = 0.0
    for base in range(0, nb, SMP_BLOCK):
        x = np.zeros(SMP_BLOCK, np.float64)
        n = min(SMP_BLOCK, nb - base)
        x[:n] = bs[base:base + n]
        s = _hillis_steele(x)
        c = 0.0 if "carry_dropped" in PERTURB else carry
        off[base:base + n] = ((c + s) - x)[:n]
        carry = carry + s[SMP_BLOCK - 1]
    total = carry
    # smp_search inside a block: lane l holds occupancies 4l .. 4l+3, sums them in order, the lane totals are scanned across the wave
    q = w.reshape(nb, 64, 4)
    vq = np.zeros_like(q)
    run = np.zeros((nb, 64), np.float64)
    for e in range(4):
        run = run + q[:, :, e]
        vq[:, :, e] = run
    incl = _hillis_steele(run)
    base_l = off[:, None] + (incl - run)
    cum = (base_l[:, :, None] + vq).reshape(nb, SMP_BLOCK)
    return kept.reshape(nb, SMP_BLOCK), cum, off, total


def sample_proxy(X, occ, vh, u, min_occ, want_trace=False):
    """One cloud, as mcr_sample_proxy leaves its outputs: res [n,4], res_h [n,64] or None, inverse [n] int64, uniq [n] int64 (rows
    beyond n_unique zero), n_unique, volume (fp64 sum of the kept occupancies).  X [P,3], occ [P], vh [P,64] or None, u [n]."""
    X, occ, u = np.asarray(X, F), np.asarray(occ, F).reshape(-1), np.asarray(u, F).reshape(-1)
    n = len(u)
    kept, cum, off, total = sampler_scan(occ, min_occ)
    nb = len(off)
    tr = SamplerTrace(n)
    picked = np.full(n, -1, np.int64)
    last_in = np.where(kept.any(1), SMP_BLOCK - 1 - np.argmax(kept[:, ::-1], axis=1), -1)      # last kept position of every block
    for s in range(n):
        target = np.float64(u[s]) * total
        lo, hi = 0, nb - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if off[mid] < target:
                lo = mid
            else:
                hi = mid - 1
        tr.lo[s] = lo
        ans = last_kept = -1
        for blk in range(lo, nb):
            hit = kept[blk] & ((cum[blk] > target) if "cdf_strict" in PERTURB else (cum[blk] >= target))
            if hit.any():
                ans = blk * SMP_BLOCK + int(np.argmax(hit))
                tr.found_in[s] = blk
            if last_in[blk] >= 0:
                last_kept = blk * SMP_BLOCK + int(last_in[blk])
            if ans >= 0:
                break
            tr.moved_on[s] = tr.moved_on[s] or blk + 1 < nb
        if ans < 0:
            if last_kept < 0:
                tr.backward[s] = lo > 0
                for blk in range(lo - 1, -1, -1):
                    if last_in[blk] >= 0:
                        last_kept = blk * SMP_BLOCK + int(last_in[blk])
                        break
            ans = last_kept
        picked[s] = ans
    res = np.zeros((n, 4), F)
    res_h = np.zeros((n, 64), F) if vh is not None else None
    uniq = np.zeros(n, np.int64)
    if (picked < 0).any():                                       # nothing above min_occ: every sample is invalid
        assert (picked < 0).all()
        inverse, nu = np.zeros(n, np.int64), 0
    else:
        un, inverse = np.unique(picked, return_inverse=True)
        nu = len(un)
        uniq[:nu] = un
        res[:nu, :3], res[:nu, 3] = X[un], occ[un]
        if vh is not None:
            res_h[:nu] = np.asarray(vh, F)[un]
    out = (res, res_h, inverse.astype(np.int64), uniq, nu, float(total))
    if not PERTURB and nu > 0:                                    # the restatement IS the oracle's convention
        ro, ho, io, uo = V.sample_proxy_points(X, occ[:, None], np.zeros((len(occ), 64), F) if vh is None else vh, u, min_occ, exact=True)
        assert len(uo) == nu and np.array_equal(uo, uniq[:nu]) and np.array_equal(io, inverse) and np.array_equal(ro, res[:nu]), \
            "the sampler restatement left the oracle's exact-CDF convention"
        assert vh is None or np.array_equal(ho, res_h[:nu])
    return out + (tr,) if want_trace else out


def on_step_uniforms(occ, min_occ, want):
    """Uniforms that sit EXACTLY on a CDF step: u = C_i / C_last as fp32 with fp64(u) * C_last == C_i, for up to `want` kept points
    spread over the cloud (the last step, u = 1, included).  -> (u fp32, the kept indices i)."""
    occ = np.asarray(occ, F).reshape(-1)
    idx = np.nonzero(occ > F(min_occ))[0]
    C = np.cumsum(occ[idx].astype(np.float64))
    us, at = [], []
    for j in np.unique(np.linspace(0, len(idx) - 1, 4 * want).astype(int))[::-1]:
        uu = F(C[j] / C[-1])
        if np.float64(uu) * C[-1] == C[j]:
            us.append(uu)
            at.append(int(idx[j]))
        if len(us) == want:
            break
    return np.array(us, F), np.array(at, np.int64)


# ---- frustum mask -------------------------------------------------------------------------------------------------------------------
def points_in_fov(pts, rec):
    if "ndc_exclusive" not in PERTURB:
        return R.points_in_fov(pts, rec)
    r2 = np.array(rec, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = R.points_in_fov(pts, r2)
        r2[33] = np.nextafter(r2[33], F(-np.inf))                 # nx <= pred(max_x)  ==  nx < max_x
        return m & R.points_in_fov(pts, r2)


def fov_intermediates_exact(pts, rec):
    """The products and sums of point_in_fov in fp32 equal their fp64 values (so a contraction into fma cannot change them), and the
    two quotients are exact too."""
    ok = True
    p64, r64 = np.asarray(pts, np.float64), np.asarray(rec, np.float64)
    p32, r32 = np.asarray(pts, F), np.asarray(rec, F)
    for cols, M in (((2,), 0), ((0, 1, 3), 16)):
        for j in cols:
            a = ((p32[:, 0] * r32[M + j] + p32[:, 1] * r32[M + 4 + j]) + p32[:, 2] * r32[M + 8 + j]) + r32[M + 12 + j]
            b = ((p64[:, 0] * r64[M + j] + p64[:, 1] * r64[M + 4 + j]) + p64[:, 2] * r64[M + 8 + j]) + r64[M + 12 + j]
            ok = ok and np.array_equal(a.astype(np.float64), b)
    d32, d64 = p32 - r32[36:39], p64 - r64[36:39]
    ok = ok and np.array_equal(((d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2]).astype(np.float64),
                               (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2])
    return bool(ok)


# ---- signed distance and the single-frame update ------------------------------------------------------------------------------------
def signed_distance(pts, rec, depth, dmask, fill):
    if "border_tap" not in PERTURB:
        return FM.signed_distance(pts, rec, depth, dmask, fill)
    # the mistake: `if (ix1 < W)` dropped from the east tap.  Its weight is 0 there, and pixel (iy0, W) is the next row's first one
    # (NaN behind the last row): the sum changes where that pixel is not finite.
    H, W = depth.shape
    good = FM.signed_distance(pts, rec, depth, dmask, fill)
    d = np.where(dmask, depth, F(fill)).astype(F) if dmask is not None else depth.astype(F)
    flat = np.concatenate([d.reshape(-1), np.full(W + 1, np.nan, F)])
    fx, fy = bilinear_coords(pts, rec, H, W)
    ix0, iy0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    with np.errstate(invalid="ignore"):
        extra = flat[iy0 * W + ix0 + 1] * ((fx - np.floor(fx)) * (np.floor(fy) + F(1) - fy))
    return np.where(ix0 + 1 == W, (good + extra).astype(F), good).astype(F)


def bilinear_coords(pts, rec, H, W, dt=F):
    """(fx, fy): the clamped pixel coordinates signed_distance samples the depth map at, in the kernel's order, in dtype dt."""
    pts, rec = np.asarray(pts, dt), np.asarray(rec, dt)
    Mp = rec[16:32].reshape(4, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    lin = lambda j: ((x * Mp[0, j] + y * Mp[1, j]) + z * Mp[2, j]) + Mp[3, j]       # noqa: E731
    pw = lin(3)
    px, py = lin(0) / pw, lin(1) / pw
    factor = -dt(min(H, W))
    gx, gy = factor / dt(W) * px, factor / dt(H) * py
    fx = ((gx + dt(1)) * dt(W) - dt(1)) / dt(2)
    fy = ((gy + dt(1)) * dt(H) - dt(1)) / dt(2)
    return np.minimum(dt(W - 1), np.maximum(fx, dt(0))), np.minimum(dt(H - 1), np.maximum(fy, dt(0)))


def unclamped_coords(pts, rec, H, W):
    """fp64 pixel coordinates before the clamp (which side of the border a projection falls on)."""
    pts, rec = np.asarray(pts, np.float64), np.asarray(rec, np.float64)
    Mp = rec[16:32].reshape(4, 4)
    h = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ Mp
    px, py = h[:, 0] / h[:, 3], h[:, 1] / h[:, 3]
    m = float(min(H, W))
    return ((-m / W * px + 1) * W - 1) / 2, ((-m / H * py + 1) * H - 1) / 2


def proxy_update(pts, fov_mask, sgn, X_cam, distance_to_surface, tol, score_threshold, n_elev, n_azim, tables):
    """mcr_proxy_scene_update from the signed distances: _frames_model.update_frames with K = 1.  tables = (view_states, n_inside,
    n_behind, sup_occ, out_of_field) -> new copies."""
    t = -tol if "tol_sign" in PERTURB else tol
    bits = np.asarray(fov_mask, bool).astype(np.uint32)
    s = np.where(bits.astype(bool), np.asarray(sgn, F), F(0))[None]
    return FM.update_frames(pts, bits, s, np.asarray(X_cam, F).reshape(1, 3), distance_to_surface, t, score_threshold, n_elev, n_azim,
                            *tables)


# ---- view state ---------------------------------------------------------------------------------------------------------------------
def view_state_indices(pts, X_view, n_elev, n_azim):
    """pts [n_clouds, P, >=3], X_view [n_view, 3] -> bin index [n_clouds, P, n_view] (oracle/view_state.py, behind the switch)."""
    if "elev_ge" not in PERTURB:
        return V.view_state_indices(pts, X_view, n_elev, n_azim)
    pts, X_view = np.asarray(pts, F), np.asarray(X_view, F)
    n_clouds, seq_len, _ = pts.shape
    es, az = F(np.pi / (n_elev + 1)), F(2 * np.pi / n_azim)
    rays = (X_view[None, None, :, :] - pts[:, :, None, :3]).reshape(-1, 3)
    _, elev, azim = sh.spherical_coords(rays)
    ie, ia = V.floor_divide(elev, es), V.floor_divide(azim, az)
    ie[np.mod(elev, es) >= F(np.pi / (n_elev + 1) / 2.)] += 1                 # the mistake: >= for >
    ia[np.mod(azim, az) > F(2 * np.pi / n_azim / 2.)] += 1
    ie[ie >= n_elev] = n_elev - 1
    ie[ie < -n_elev // 2] = -n_elev // 2
    ia[ia > n_azim // 2] = -n_azim // 2
    ie += n_elev // 2
    ia[ia < 0] += n_azim
    idx = ie.astype(np.int64) * n_azim + ia.astype(np.int64)
    idx %= n_elev * n_azim
    return idx.reshape(n_clouds, seq_len, X_view.shape[0])


def compute_view_state(pts, X_view, n_elev, n_azim, table=None, rows=None):
    """pts [P, >=3] of ONE cloud -> [P, n_bins]; with table / rows: a copy of `table` with the bins OR'ed into row rows[p]."""
    pts = np.asarray(pts, F)
    idx = view_state_indices(pts[None], X_view, n_elev, n_azim)[0]
    out = np.zeros((len(pts), n_elev * n_azim), F) if table is None else np.array(table, F)
    r = np.arange(len(pts)) if rows is None else np.asarray(rows)
    out[np.repeat(r, idx.shape[1]), idx.reshape(-1)] = 1.0
    if not PERTURB and table is None:
        assert np.array_equal(out, V.compute_view_state(pts[None], X_view, n_elev, n_azim)[0])
    return out


def decision_margin(pts, X_view, n_elev, n_azim):
    """fp64 distance (radians) of every (point, view) ray to the nearest place where upstream's fp32 binning can change its answer:
    the half-step boundaries and the +-pi seam (oracle.view_state.bin_boundary_margin) AND the bin centres.  At a centre the angle
    crosses a multiple of the step, mod() jumps from ~step to 0, and the index is `trunc((angle - mod) / step) [+ 1]`: that quotient
    is not an integer in fp32 for every bin (F(3 step) / F(step) = 2.9999998), so the two sides of a centre can land in different
    bins.  -> [n_clouds, P, n_view]"""
    b = V.bin_boundary_margin(pts, X_view, n_elev, n_azim)
    p, x = np.asarray(pts, np.float64), np.asarray(X_view, np.float64)
    rays = (x[None, None, :, :] - p[:, :, None, :3]).reshape(-1, 3)
    r = np.linalg.norm(rays, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        elev = np.arcsin(np.clip(rays[:, 1] / r, -1, 1))
    azim = np.arctan2(rays[:, 0], rays[:, 2])
    es, az = np.pi / (n_elev + 1), 2 * np.pi / n_azim
    ce = np.minimum(np.mod(elev, es), es - np.mod(elev, es))
    ca = np.minimum(np.mod(azim, az), az - np.mod(azim, az))
    return np.minimum(b, np.minimum(ce, ca).reshape(b.shape))


def lattice_rays(n_elev, n_azim, radius=1.0):
    """One direction per bin of the lattice: the lattice angles (scone_utils.py:723-727) moved a quarter of a step in elevation and in
    azimuth, i.e. a quarter step from the bin's centre AND from its rounding boundary (see decision_margin; for an even n_elev the
    lattice elevations themselves are half-steps).  fp64 angles -> fp32 vectors of length `radius`."""
    es, az = np.pi / (n_elev + 1), 2 * np.pi / n_azim
    e = np.array([-np.pi / 2 + (i + 1) * es + es / 4 for i in range(n_elev) for j in range(n_azim)])
    a = np.array([j * az + az / 4 for i in range(n_elev) for j in range(n_azim)])
    d = np.stack((np.cos(e) * np.sin(a), np.sin(e), np.cos(e) * np.cos(a)), 1) * radius
    return d.astype(F)


# ---- transform, unprojection, gains -------------------------------------------------------------------------------------------------
def transform_points(pts, M, center, inv_diag, cloud=None, dt=F):
    """pts [n,d]; M [K,16], center [K,3], inv_diag [K]; cloud [n] (the cloud of every row; None: cloud 0) -> new [n,d]: columns 0..2
    as transform_points_kernel computes them in dtype dt, the others untouched."""
    out = np.array(pts, dt)
    M, center, inv_diag = np.asarray(M, dt).reshape(-1, 16), np.asarray(center, dt).reshape(-1, 3), np.asarray(inv_diag, dt).reshape(-1)
    c = np.zeros(len(out), np.int64) if cloud is None else np.asarray(cloud, np.int64)
    x, y, z = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
    for j in range(3):
        out[:, j] = ((((x * M[c, j] + y * M[c, 4 + j]) + z * M[c, 8 + j]) + M[c, 12 + j]) - center[c, j]) * inv_diag[c]
    return out


def unproject_depth(depth, cam, dt=F, homogeneous=False):
    """depth [H,W], cam [18] = Minv[16], k22, k32 -> [H*W, 3] as unproject_depth_kernel computes it in dtype dt (the inputs are the
    fp32 values either way); homogeneous: the [H*W, 4] coordinates before the divide instead."""
    H, W = depth.shape
    m = dt(min(H, W))
    i = np.arange(H, dtype=dt)[:, None].repeat(W, 1).reshape(-1)
    j = np.arange(W, dtype=dt)[None, :].repeat(H, 0).reshape(-1)
    nx = dt(W) / m - (j / (m - dt(1))) * dt(2)
    ny = dt(H) / m - (i / (m - dt(1))) * dt(2)
    if dt is F:
        tx, ty = S.ndc_tabs(H, W)
        assert np.array_equal(nx, tx.reshape(-1)) and np.array_equal(ny, ty.reshape(-1))
    K = np.asarray(cam, F).astype(dt)
    d = np.asarray(depth, F).astype(dt).reshape(-1)
    sd = (K[16] * d + K[17]) / d
    lin = lambda c: ((nx * K[c] + ny * K[4 + c]) + sd * K[8 + c]) + K[12 + c]       # noqa: E731
    w = lin(3)
    if homogeneous:
        return np.stack([lin(0), lin(1), lin(2), w], 1).astype(dt)
    return np.stack([lin(0) / w, lin(1) / w, lin(2) / w], 1).astype(dt)


def tuple_table(C, n_cam):
    """[C^n_cam, n_cam]: the cameras of every output column, in torch.cartesian_prod's order (the last index fastest)."""
    import torch
    t = torch.cartesian_prod(*([torch.arange(C)] * n_cam)).numpy().reshape(-1, n_cam)
    if "cartesian_reversed" in PERTURB:
        t = t[:, ::-1]
    return t


def coverage_gain_multiple(vis, n_cam):
    """vis [B,C,N] fp32 -> fp64 [B, C^n_cam]: mean over n of the max over the tuple's cameras."""
    vis = np.asarray(vis, F).astype(np.float64)
    t = tuple_table(vis.shape[1], n_cam)
    return np.stack([vis[:, t[:, k], :] for k in range(n_cam)], 0).max(0).mean(-1)


def macarons_gain(vis, pts, cam, volume, th, mode, dt=F):
    """-> (vis scaled in place [B,N] in dtype dt in the kernel's order, gains [B] fp64 from those scaled values)."""
    vis, p, cam = np.asarray(vis, F).astype(dt), np.asarray(pts, F).astype(dt), np.asarray(cam, F).astype(dt)
    th = dt(F(th))
    dx, dy, dz = (p[..., k] - cam[:, None, k] for k in range(3))
    d = np.sqrt((dx * dx + dy * dy) + dz * dz).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == 1:
            q = d / th
            f = dt(1) / (dt(1) + q * q)
        else:
            f = np.where(d > th, (th * th) / (d * d), dt(1))
    v = (vis * f).astype(dt)
    g = v.astype(np.float64).mean(-1)
    return v, g


def torch_max_rows(g):
    """torch.max(g, dim=1) in numpy: a NaN beats every number (the first NaN), else the largest value, ties to the lowest index.
    -> (values fp32 [B], indices int64 [B])."""
    import torch
    g = np.asarray(g, F)
    isn = np.isnan(g)
    idx = np.where(isn.any(1), np.argmax(isn, 1), np.argmax(np.where(isn, -np.inf, g), 1))
    if "last_nan" in PERTURB:
        idx = np.where(isn.any(1), g.shape[1] - 1 - np.argmax(isn[:, ::-1], 1), idx)
    else:
        ref = torch.max(torch.from_numpy(g), dim=1)
        assert np.array_equal(ref.indices.numpy(), idx)
    return g[np.arange(len(g)), idx], idx.astype(np.int64)
