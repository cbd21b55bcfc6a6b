"""Synthetic frames for the trainer's K-frame passes: perspective cameras on a ring around an ellipsoid, looking at it (or away from
it), their 40-float frustum records and 18-float depth records, and the analytic depth map of the ellipsoid per camera.
TEST INFRASTRUCTURE ONLY (numpy; the conventions are those of oracle/scene.py and oracle/macarons_regime.py: row-vector matrices)."""
import numpy as np

from oracle import scene as S

AXES = np.array([5.5, 2.8, 5.0])
BOX = np.array([8.0, 4.0, 8.0], np.float32)            # the scene box is [-BOX, BOX], a 2 x 1 x 2 grid in the tests
ZFAR = 500.0
RANGE = 24.0


def look_at(eye, at):
    """World -> view rotation (columns = camera axes) and translation of a camera at `eye` looking at `at`, up = +Y."""
    eye, at = np.asarray(eye, np.float64), np.asarray(at, np.float64)
    z = (at - eye) / np.linalg.norm(at - eye)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], -1)
    return R.astype(np.float32), (-(R.T @ eye)).astype(np.float32)


def projection(fov_deg=60.0, znear=1.0, zfar=ZFAR):
    s = 1.0 / np.tan(np.deg2rad(fov_deg) / 2)
    return np.array([[s, 0, 0, 0], [0, s, 0, 0], [0, 0, zfar / (zfar - znear), 1], [0, 0, -zfar * znear / (zfar - znear), 0]], np.float32)


def ndc_bounds(H, W):
    nx, ny = S.ndc_tabs(H, W)
    return np.array([nx.min(), nx.max(), ny.min(), ny.max()], np.float32)


def ellipsoid_depth(H, W, eye, R, axes=AXES, fov_deg=60.0):
    """View-space depth of the ellipsoid along every pixel's ray (-1 where the ray misses) and the hit mask."""
    nx, ny = S.ndc_tabs(H, W)
    s = 1.0 / np.tan(np.deg2rad(fov_deg) / 2)
    d = np.stack([nx.astype(np.float64) / s, ny.astype(np.float64) / s, np.ones((H, W))], -1) @ R.astype(np.float64).T
    o, ax = np.asarray(eye, np.float64), np.asarray(axes, np.float64)
    A, B, C = ((d / ax) ** 2).sum(-1), 2 * ((o / ax) * (d / ax)).sum(-1), ((o / ax) ** 2).sum() - 1
    disc = B * B - 4 * A * C
    hit = disc > 0
    tt = (-B - np.sqrt(np.where(hit, disc, 0.0))) / (2 * A)
    hit &= tt > 0
    return np.where(hit, tt, -1.0).astype(np.float32), hit


def make_frames(K, H, W, seed, away=()):
    """K cameras at radius ~10 on a wavy ring; the ones listed in `away` look away from the scene (empty frustum over the box).
    -> dict(recs [K,40], cam18 [K,18], depths [K,H,W], dmasks [K,H,W] bool, eyes [K,3], zfar, sensor_range)."""
    rng = np.random.default_rng(seed)
    P1 = projection()
    recs, cam18, depths, dmasks, eyes = [], [], [], [], []
    for k in range(K):
        th = 2 * np.pi * k / max(K, 3) + 0.13 + 0.05 * rng.standard_normal()
        eye = np.array([10.0 * np.cos(th), 3.0 * np.sin(3 * th + 0.4), 10.0 * np.sin(th)], np.float32)
        at = (4.0 * eye if k in away else np.array([3.0 * np.sin(3 * k + 0.4), 0.3, 3.0 * np.cos(2 * k + 0.2)])).astype(np.float32)
        R, T = look_at(eye, at)
        Mv = np.zeros((4, 4), np.float32)
        Mv[:3, :3], Mv[3, :3], Mv[3, 3] = R, T, 1.0
        Mf = (Mv @ P1).astype(np.float32)
        recs.append(np.concatenate((Mv.reshape(-1), Mf.reshape(-1), ndc_bounds(H, W), eye, [RANGE])).astype(np.float32))
        cam18.append(np.concatenate((np.linalg.inv(Mf.astype(np.float64)).astype(np.float32).reshape(-1), [P1[2, 2], P1[3, 2]])).astype(np.float32))
        dd, hh = ellipsoid_depth(H, W, eye, R)
        depths.append(dd); dmasks.append(hh); eyes.append(eye)
    return dict(recs=np.stack(recs), cam18=np.stack(cam18), depths=np.stack(depths), dmasks=np.stack(dmasks), eyes=np.stack(eyes),
                zfar=ZFAR, sensor_range=RANGE)


def proxy_points(P, seed):
    """P points of the box on the 2^-6 grid, off the cell faces (x = 0, z = 0) -- Cell.fill's box tests are strict."""
    rng = np.random.default_rng(seed)
    q = (np.round(rng.uniform(-1, 1, (P, 3)) * (BOX - 0.1) * 64) / 64).astype(np.float32)
    q[q == 0] = 1.0 / 64
    return q


def load_scone_step(g):
    """tests/golden/scone_step.npz (make_golden_scone_step.py) decoded: the K = 3 frames as records, the inputs and every recorded table."""
    P, (H, W), G = len(g["proxy"]), [int(v) for v in g["hw"]], np.float32(g["G"])
    K = len(g["eyes"])
    bits = lambda a, n: np.unpackbits(a)[:n].astype(bool)                                    # noqa: E731
    out = dict(P=P, H=H, W=W, K=K, proxy=g["proxy"].astype(np.float32) / G, eyes=g["eyes"],
               recs=np.stack([np.concatenate((g["Mview"][k].reshape(-1), g["Mfull"][k].reshape(-1), g["ndc"], g["eyes"][k],
                                              [g["sensor_range"]])).astype(np.float32) for k in range(K)]),
               cam18=np.stack([np.concatenate((np.linalg.inv(g["Mfull"][k].astype(np.float64)).astype(np.float32).reshape(-1),
                                               [g["P"][2, 2], g["P"][3, 2]])).astype(np.float32) for k in range(K)]),
               depth=g["depth"], dmask=bits(g["dmask"], K * H * W).reshape(K, H, W), error_mask=bits(g["error_mask"], K * H * W).reshape(K, H, W),
               fov_masks=np.unpackbits(g["fov_masks"], axis=-1)[:, :P].astype(bool), close_mask=bits(g["close_mask"], P),
               prediction_mask=bits(g["prediction_mask"], P), pseudo_gt=bits(g["pseudo_gt"], P).astype(np.float32),
               X_world=(g["proxy"].astype(np.float32) / G)[g["X_idx"]], view_harmonics=g["vh_q"].astype(np.float32) / np.float32(512.),
               occ=g["occ"].astype(np.float32))
    for tag in ("before", "after"):
        out[tag] = dict(view_states=np.unpackbits(g[f"{tag}_view_states"], axis=-1)[:, :98].astype(np.float32),
                        n_inside=g[f"{tag}_n_inside"].astype(np.float32), n_behind=g[f"{tag}_n_behind"].astype(np.float32),
                        sup_occ=bits(g[f"{tag}_sup_occ"], P).astype(np.float32), oof=bits(g[f"{tag}_oof"], P).astype(np.float32))
    return out
