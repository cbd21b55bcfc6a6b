#!/usr/bin/env python3
"""Golden vectors of the depth module's plane sweep: the REFERENCE's own CostVolumeBuilder.forward(..., return_cost_volume=True)
(macarons/networks/ManyDepth.py:207-305) on the CPU, this container only.

    python tests/golden/make_golden_cost_volume.py        # writes tests/golden/cost_volume.npz (data only)

PyTorch3D is not installed here: the module's FoVPerspectiveCameras name is bound to a stand-in built on make_golden._StandInCameras
(explicit row-vector matrices; unproject_points and Transform3d.transform_points as published, the latter with its eps rule
sign(w) * max(|w|, eps)).  Stored per case: the inputs, the reference's conv_reduce parameters, `cost_volume` and `res`.

Cases (the smallest that reach every branch of the fused kernel):
  a  B 2, A 2, D 5,  26x42 -> 6x10   resize ratios 4.33 / 4.2 (fractional cubic weights), general target poses, one source ahead of the
                                     target along the view axis (the nearest plane falls behind it, w < 0), one source looking away with
                                     every sample outside its map
  b  B 1, A 1, D 96, 24x40 -> 6x10   upstream's plane count and bins (0.5 .. 750), target R = I, T = 0 as apply_depth_model sets them
  c  B 1, A 3, D 3,  32x64 -> 8x16   n_alpha != 2
Asserted here (conditions on the drawn poses, not tolerances): no projected point of any case has |w| < 1e-3; in case a at least half of
the output positions have a sample inside some source map and at least 5 % have none.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402

_ref_import.install_stubs()
import torch  # noqa: E402
from make_golden import _StandInCameras, _fov_projection  # noqa: E402

MD = importlib.import_module("macarons.networks.ManyDepth")
torch.set_num_threads(8)

_min_abs_w = [float("inf")]


class _Cameras(_StandInCameras):
    class _T(_StandInCameras._T):
        def transform_points(self, p, eps=None):
            p4 = torch.cat((p, torch.ones_like(p[..., :1])), -1) @ self.M
            w = p4[..., 3:4]
            _min_abs_w[0] = min(_min_abs_w[0], float(w.abs().min()))
            if eps is not None:                          # Transform3d.transform_points as published
                sign = torch.sign(w) + (w == 0.0).type_as(w)
                w = sign * torch.clamp(w.abs(), eps)
            return p4[..., :3] / w

    def get_full_projection_transform(self):
        return self._T(self.Mv @ self.P)


def _factory(device=None, R=None, T=None, zfar=None):
    P = torch.stack([torch.from_numpy(_fov_projection(60.0, 1.0, float(z))) for z in zfar.reshape(-1)])
    return _Cameras(R, T, P)


MD.FoVPerspectiveCameras = _factory


def rot(axis, angle):
    """Rotation matrix about `axis` by `angle` (Rodrigues), float32."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return torch.tensor(np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K, dtype=torch.float32)


def run_case(tag, seed, H, W, Hf, Wf, D, d_min, d_max, out_ch, R, T, Ra, Ta):
    torch.manual_seed(seed)
    B, A, C = Ra.shape[0], Ra.shape[1], 64
    cvb = MD.CostVolumeBuilder(H, W, Hf, Wf, C, A, d_min, d_max, D, out_ch)
    x, xa = torch.randn(B, C, Hf, Wf), torch.randn(B, A, C, Hf, Wf)
    zf, zfa = torch.full((B,), 750.0), torch.full((B, A), 750.0)
    grids = []
    real_gs = torch.nn.functional.grid_sample

    def capture(input, grid, **kw):
        grids.append(grid.clone())
        return real_gs(input, grid, **kw)

    MD.torch.nn.functional.grid_sample = capture
    try:
        with torch.no_grad():
            res, cv = cvb(x, R, T, zf, xa, Ra, Ta, zfa, device="cpu", return_cost_volume=True)
    finally:
        MD.torch.nn.functional.grid_sample = real_gs
    g = grids[0].reshape(B, D, A, Hf, Wf, 2)                              # the reference's batch order: b, plane, source
    px, py = ((g[..., 0] + 1) * Wf - 1) / 2, ((g[..., 1] + 1) * Hf - 1) / 2
    inside = (px > -1) & (px < Wf) & (py > -1) & (py < Hf)                # some bilinear corner inside the source map
    sd = cvb.state_dict()
    out = {f"{tag}_x": x, f"{tag}_x_alpha": xa, f"{tag}_R": R, f"{tag}_T": T, f"{tag}_R_alpha": Ra, f"{tag}_T_alpha": Ta,
           f"{tag}_dims": np.array([H, W, D, out_ch], np.int64), f"{tag}_d_range": np.array([d_min, d_max], np.float64),
           f"{tag}_depth_bins": cvb.depth_bins, f"{tag}_cost_volume": cv, f"{tag}_res": res,
           f"{tag}_state_keys": np.array(list(sd.keys())), f"{tag}_state_shapes": np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()]),
           f"{tag}_conv_reduce_weight": sd["conv_reduce.weight"], f"{tag}_conv_reduce_bias": sd["conv_reduce.bias"]}
    print(f"case {tag}: cost volume {tuple(cv.shape)} max {float(cv.max()):.3f}; positions with a sample inside "
          f"{float(inside.any(2).float().mean()):.3f}; min |w| so far {_min_abs_w[0]:.3e}")
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, inside


def main():
    data = {}
    # ---- a: general poses; source (0, 0) sits 2 units ahead along the view axis (plane 0.5 is behind it), source (1, 1) looks away
    R = torch.stack([rot([0, 1, 0], 0.1), rot([1, 0, 0], -0.05)])
    T = torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]])
    Ra = torch.stack([torch.stack([rot([0, 1, 0], 0.12), rot([0.2, 1, 0], -0.07)]),
                      torch.stack([rot([1, 0.3, 0], 0.06), rot([0, 1, 0], np.deg2rad(150.0))])])
    Ta = torch.tensor([[[0.5, 0.0, -2.0], [-0.3, 0.1, 0.2]], [[0.0, 0.4, 0.1], [40.0, 0.0, 0.0]]])
    d, inside = run_case("a", 0, 26, 42, 6, 10, 5, 0.5, 12.0, 8, R, T, Ra, Ta)
    data.update(d)
    data["a_away"] = np.array([1, 1], np.int64)                          # (b, a) of the source that looks away
    frac = float(inside.any(2).float().mean())
    assert frac >= 0.5, frac
    assert 1.0 - frac >= 0.05, frac
    assert not bool(inside[1, :, 1].any()), "the source that looks away has a sample inside"
    assert bool((torch.from_numpy(d["a_depth_bins"])[0] - 2.0 < 0)), "no plane behind source (0, 0)"
    # ---- b: upstream's planes, the target at the origin as apply_depth_model sets it
    d, _ = run_case("b", 1, 24, 40, 6, 10, 96, 0.5, 750.0, 8, torch.eye(3)[None], torch.zeros(1, 3),
                    rot([0.1, 1, 0], 0.05)[None, None], torch.tensor([[[0.4, -0.1, 0.15]]]))
    data.update(d)
    # ---- c: three sources
    d, _ = run_case("c", 2, 32, 64, 8, 16, 3, 1.0, 9.0, 8, rot([0, 1, 0.1], -0.08)[None], torch.tensor([[0.05, -0.1, 0.2]]),
                    torch.stack([rot([0, 1, 0], 0.1), rot([1, 0, 0], 0.08), rot([0, 0, 1], 0.2)])[None],
                    torch.tensor([[[0.3, 0.0, 0.1], [-0.2, 0.2, -0.3], [0.0, -0.3, 0.4]]]))
    data.update(d)
    assert _min_abs_w[0] >= 1e-3, _min_abs_w[0]
    path = os.path.join(HERE, "cost_volume.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
