"""numpy restatement of the trainer's two K-frame kernels (csrc/glue.hip: supervision_frames_kernel, proxy_update_frames_kernel),
fp32 step by step in the kernels' order of operations.  TEST INFRASTRUCTURE ONLY.

  supervision_frames   train_macarons.py:402-415: frustum bits (Camera.get_points_in_fov), signed distances to each frame's depth map
                       (Camera.get_signed_distance_to_depth_maps, macarons_utils.py:2451-2500: grid_sample bilinear / border /
                       align_corners=False on the depth with masked pixels at `fill`), the close mask with upstream's overwrite rule
  update_frames        :476-487: view-state bins, the two counters, the supervision occupancy and the out-of-field flags
"""
import numpy as np

from oracle import macarons_regime as R
from oracle import view_state as V

F = np.float32


def signed_distance(pts, rec, depth, dmask, fill):
    """pts [n,3], rec: M_view[16] | M_full_projection[16] | ..., depth [H,W], dmask [H,W] bool or None -> [n] fp32."""
    pts = np.asarray(pts, F)
    H, W = depth.shape
    Mv, Mp = rec[:16].reshape(4, 4).astype(F), rec[16:32].reshape(4, 4).astype(F)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    lin = lambda M, j: ((x * M[0, j] + y * M[1, j]) + z * M[2, j]) + M[3, j]       # noqa: E731
    zv = lin(Mv, 2) / lin(Mv, 3)
    pw = lin(Mp, 3)
    px, py = lin(Mp, 0) / pw, lin(Mp, 1) / pw
    factor = -F(min(H, W))
    gx, gy = factor / F(W) * px, factor / F(H) * py
    fx = ((gx + F(1)) * F(W) - F(1)) / F(2)
    fy = ((gy + F(1)) * F(H) - F(1)) / F(2)
    fx = np.minimum(F(W - 1), np.maximum(fx, F(0)))
    fy = np.minimum(F(H - 1), np.maximum(fy, F(0)))
    x0, y0 = np.floor(fx), np.floor(fy)
    ix0, iy0 = x0.astype(np.int64), y0.astype(np.int64)
    ix1, iy1 = ix0 + 1, iy0 + 1
    d = np.where(dmask, depth, F(fill)).astype(F) if dmask is not None else depth.astype(F)
    w_nw, w_ne = (x0 + F(1) - fx) * (y0 + F(1) - fy), (fx - x0) * (y0 + F(1) - fy)
    w_sw, w_se = (x0 + F(1) - fx) * (fy - y0), (fx - x0) * (fy - y0)
    at = lambda ix, iy: d[np.minimum(iy, H - 1), np.minimum(ix, W - 1)]              # noqa: E731
    acc = at(ix0, iy0) * w_nw
    acc = np.where(ix1 < W, acc + at(ix1, iy0) * w_ne, acc).astype(F)
    acc = np.where(iy1 < H, acc + at(ix0, iy1) * w_sw, acc).astype(F)
    acc = np.where((ix1 < W) & (iy1 < H), acc + at(ix1, iy1) * w_se, acc).astype(F)
    return (zv - acc).astype(F)


def supervision_frames(pts, recs, depths, dmasks, fills, surface_distance):
    """-> fov_bits [P] uint32, sgn [K,P] fp32 (0 where the bit is clear), close [P] bool (the LAST frame holding the point decides)."""
    pts = np.asarray(pts, F)
    K, P = len(recs), len(pts)
    bits = np.zeros(P, np.uint32)
    sgn = np.zeros((K, P), F)
    close = np.zeros(P, bool)
    for k in range(K):
        m = R.points_in_fov(pts, recs[k].astype(F))
        d = signed_distance(pts[m], recs[k], depths[k], None if dmasks is None else dmasks[k], fills[k])
        sgn[k, m] = d
        bits[m] |= np.uint32(1) << np.uint32(k)
        close[m] = np.abs(d) < F(surface_distance)
    return bits, sgn, close


def update_frames(pts, bits, sgn, X_cam, distance_to_surface, tol, score_threshold, n_elev, n_azim, view_states, n_inside, n_behind,
                  sup_occ, out_of_field):
    """Returns new copies of the five state tables ([P, n_bins] and four [P])."""
    pts = np.asarray(pts, F)
    vs, ni, nb = view_states.copy(), n_inside.astype(F).copy(), n_behind.astype(F).copy()
    so, oof = sup_occ.astype(F).copy(), out_of_field.astype(F).copy()
    for k in range(sgn.shape[0]):
        m = ((bits >> np.uint32(k)) & np.uint32(1)).astype(bool)
        rows = np.nonzero(m & (sgn[k] < F(distance_to_surface)))[0]
        if len(rows):
            idx = V.view_state_indices(pts[rows][None], np.asarray(X_cam[k], F).reshape(1, 3), n_elev, n_azim)[0, :, 0]
            vs[rows, idx] = 1.0
        ni[m] = ni[m] + F(1)
        nb[m] = nb[m] + (sgn[k][m] >= -F(tol)).astype(F)
        so[m] = (nb[m] / ni[m] >= F(score_threshold)).astype(F)
    oof[bits != 0] = 0.0
    return vs, ni, nb, so, oof
