#!/usr/bin/env python3
"""Golden vectors of the depth module's photometric reconstruction loss: the REFERENCE's own reconstruction_loss_fn
(macarons/utility/macarons_utils.py:1091-1187, which calls CostVolumeBuilder.reproject_depth_map / warp and the SSIM layer of
macarons/networks/ManyDepth.py) on the CPU, this container only.

    python tests/golden/make_golden_reconstruction_loss.py     # writes tests/golden/reconstruction_loss.npz (data only)

Cameras: the stand-ins of make_golden_cost_volume.py.  `macarons` is a SimpleNamespace holding an upstream CostVolumeBuilder.  Stored per
case: the inputs, and per variant (padding mode, mask on / off) `loss`, `d_depth` from loss.backward(), and the per-pixel selected loss
and index, captured by wrapping torch.min during the call; once, the parameter names of upstream's inner function.

Inputs are smooth (noise makes every bilinear gradient a kink lottery): images 0.5 + four sinusoids of amplitude 0.12 with spatial
frequencies in 0.1 .. 0.6 rad/pixel, clamped to [0, 1]; depth 3 + 1.5 sin(0.3 x + 0.2 y), + 0.7 on the second image; the target poses of
cost-volume case a, sources offset by a few tenths of a unit; one rectangular hole in each mask.

Cases:  a  B 2, A 2, S 2, 20x28  both paddings x mask on / off; the second scale a 4x nearest-upsampled coarse depth
        b  B 2, A 2, S 1, 19x37  no axis a multiple of a tile, several tiles each way
        c  B 1, A 3, S 1, 12x40
        d  B 1, A 1, S 1, 2x3    the smallest legal image: every pixel is an edge
Asserted here (conditions on the drawn inputs, not tolerances; a draw that fails one gets another seed): no |w| < 1e-3; upstream fp32
and the fp64 model (tests/_reconstruction_model.py) pick the same source at every pixel; at most 5 % of the pixels have their two best
sources within 1e-3 of the map's maximum; each source is selected on at least 25 % of the pixels (every case of more than one source);
at least 10 % of the samples lie outside each source; no SSIM value sits at the clamp.  Printed: the reference's distance to the model.
"""
import importlib
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402

_ref_import.install_stubs()
import torch  # noqa: E402
from make_golden import _fov_projection  # noqa: E402
from make_golden_cost_volume import MD, _Cameras, _min_abs_w, rot  # noqa: E402
import _reconstruction_model as model  # noqa: E402

MU = importlib.import_module("macarons.utility.macarons_utils")
ZFAR, SSIM_FACTOR = 50.0, 0.85


def _cams(R, T):
    n = R.shape[0]
    return _Cameras(R, T, torch.from_numpy(np.broadcast_to(_fov_projection(60.0, 1.0, ZFAR), (n, 4, 4)).copy()))


def smooth_images(rng, shape_prefix, H, W):
    """[..., H, W, 3]: 0.5 + four sinusoids of amplitude 0.12 per image and channel, clamped to [0, 1]."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    n = int(np.prod(shape_prefix)) * 3
    out = np.full((n, H, W), 0.5)
    for i in range(n):
        for _ in range(4):
            k, th, ph = rng.uniform(0.1, 0.6), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
            out[i] += 0.12 * np.sin(k * (np.cos(th) * xx + np.sin(th) * yy) + ph)
    out = out.reshape(*shape_prefix, 3, H, W)
    return torch.from_numpy(np.clip(np.moveaxis(out, -3, -1), 0.0, 1.0).astype(np.float32)).contiguous()


def run_variant(fn, c, padding, masked):
    B, A, H, W, _ = c["alpha_images"].shape
    params = SimpleNamespace(jz=False, ddp=False, use_depth_mask=masked, zfar=ZFAR, ssim_factor=SSIM_FACTOR)
    cvb = MD.CostVolumeBuilder(H, W, H // 2, W // 2, 64, A, 0.5, 10.0, 4, 8)
    macarons = SimpleNamespace(depth=SimpleNamespace(depth_decoder=SimpleNamespace(cost_volume_builder=cvb)))
    cameras, alpha_cameras = _cams(c["R"], c["T"]), _cams(c["R_alpha"].reshape(-1, 3, 3), c["T_alpha"].reshape(-1, 3))
    res = dict(loss=[], d_depth=[], map=[], index=[])
    real_min = torch.min
    for k in range(c["depth"].shape[0]):
        d = c["depth"][k].clone().reshape(B, H, W, 1).requires_grad_(True)
        got = []

        def capture(*a, **kw):
            r = real_min(*a, **kw)
            if kw.get("dim") == 1:
                got.append((r[0].detach().clone(), r[1].clone()))
            return r

        torch.min = capture
        try:
            loss = fn(params=params, input_images=c["images"], input_alpha_images=c["alpha_images"], mask=c["mask"][..., None],
                      cameras=cameras, alpha_cameras=alpha_cameras, predicted_depth=d, macarons=macarons, ssim_loss_fn=MD.SSIM(),
                      channel_is_at_the_end=True, padding_mode=padding)
        finally:
            torch.min = real_min
        loss.backward()
        assert len(got) == 1
        res["loss"].append(loss.detach()), res["d_depth"].append(d.grad.reshape(B, H, W))
        res["map"].append(got[0][0].reshape(B, H, W)), res["index"].append(got[0][1].reshape(B, H, W).to(torch.uint8))
    return {k: torch.stack(v) for k, v in res.items()}


def check_variant(tag, c, padding, masked, res):
    """The conditions of the module docstring, and the printed distances."""
    mask = c["mask"] if masked else None
    args = (c["images"], c["alpha_images"], mask, c["R"], c["T"], c["R_alpha"], c["T_alpha"])
    with torch.no_grad():
        m = model.reconstruction(*args, c["depth"], ZFAR, SSIM_FACTOR, padding)
    grad = model.gradient(*args, c["depth"], ZFAR, SSIM_FACTOR, padding, force_index=res["index"])
    A = c["alpha_images"].shape[1]
    w_min = min(float(p["w"].abs().min()) for p in m["parts"])
    diff_idx = int((m["index"] != res["index"].long()).sum())
    near = float((m["margin"] < 1e-3 * float(m["map"].max())).double().mean()) if A > 1 else 0.0
    shares = [float((res["index"] == a).double().mean()) for a in range(A)]
    outside = [min(float(1 - p["inside"][:, a].double().mean()) for p in m["parts"]) for a in range(A)]
    raw = torch.stack([p["ssim_raw"] for p in m["parts"]])
    e_map, e_loss, e_grad = model.rel(res["map"], m["map"]), model.rel(res["loss"], m["loss"]), model.rel(res["d_depth"], grad)
    print(f"case {tag} {padding:6s} mask={int(masked)}: min|w| {w_min:.2f}; index differences {diff_idx}; near ties {100 * near:.2f} %; "
          f"selected {['%.0f %%' % (100 * s) for s in shares]}; outside {['%.0f %%' % (100 * o) for o in outside]}; "
          f"ssim in [{float(raw.min()):.3f}, {float(raw.max()):.3f}]; reference vs model: loss {e_loss:.1e} map {e_map:.1e} d_depth {e_grad:.1e}")
    assert w_min >= 1e-3 and _min_abs_w[0] >= 1e-3
    assert diff_idx == 0
    assert near <= 0.05
    assert float(raw.min()) > 0 and float(raw.max()) < 1
    if A > 1:
        assert min(shares) >= 0.25, shares
    assert min(outside) >= 0.10, outside
    return dict(map=e_map, loss=e_loss, d_depth=e_grad)


def make_case(tag, seed, H, W, S, R, T, Ra, Ta, hole):
    rng = np.random.default_rng(seed)
    B, A = Ra.shape[0], Ra.shape[1]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    base = 3.0 + 1.5 * np.sin(0.3 * xx + 0.2 * yy)
    depth = np.stack([base + 0.7 * (b == 1) for b in range(B)])[None].repeat(S, 0)
    if S > 1:                                              # the second scale: a coarse depth, 4x nearest-upsampled
        coarse = (depth[0][:, ::4, ::4] + 0.15 * np.cos(0.5 * xx[::4, ::4]))
        depth[1] = coarse.repeat(4, 1).repeat(4, 2)[:, :H, :W]
    mask = np.ones((B, H, W), bool)
    y0, y1, x0, x1 = hole
    mask[:, y0:y1, x0:x1] = False
    return dict(images=smooth_images(rng, (B,), H, W), alpha_images=smooth_images(rng, (B, A), H, W), mask=torch.from_numpy(mask),
                R=R, T=T, R_alpha=Ra, T_alpha=Ta, depth=torch.from_numpy(depth.astype(np.float32)))


def main():
    fn = MU.get_reconstruction_loss_fn(SimpleNamespace())
    data = {"parameter_names": np.array(list(inspect.signature(fn).parameters))}
    # the target poses of cost-volume case a; sources a few tenths of a unit away, turned enough to look past the target's frame
    R = torch.stack([rot([0, 1, 0], 0.1), rot([1, 0, 0], -0.05)])
    T = torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.0, 0.0]])
    Ra = torch.stack([torch.stack([rot([0, 1, 0], 0.1 + 0.33), rot([0.2, 1, 0], 0.1 - 0.3)]),
                      torch.stack([rot([1, 0.3, 0], -0.05 + 0.3), rot([0, 1, 0], -0.3)])])
    Ta = torch.tensor([[[0.4, 0.0, 0.1], [-0.3, 0.1, 0.2]], [[0.0, 0.4, 0.1], [0.3, -0.2, 0.0]]])
    cases = {
        "a": make_case("a", 0, 20, 28, 2, R, T, Ra, Ta, (5, 11, 8, 17)),
        "b": make_case("b", 1, 19, 37, 1, R, T, Ra, Ta, (3, 9, 20, 31)),
        "c": make_case("c", 11, 12, 40, 1, R[:1], T[:1], torch.stack([rot([0, 1, 0], 0.3), rot([1, 0, 0], 0.2), rot([0, 0, 1], 0.2)])[None],
                       torch.tensor([[[0.3, 0.0, 0.1], [-0.2, 0.2, -0.3], [0.0, -0.3, 0.4]]]), (2, 7, 10, 22)),
        "d": make_case("d", 3, 2, 3, 1, R[:1], T[:1], rot([0, 1, 0], 0.15)[None, None], torch.tensor([[[0.2, -0.1, 0.1]]]), (0, 1, 1, 2)),
    }
    for tag, c in cases.items():
        for k, v in c.items():
            data[f"{tag}_{k}"] = v.numpy()
        data[f"{tag}_zfar"], data[f"{tag}_ssim_factor"] = np.float64(ZFAR), np.float64(SSIM_FACTOR)
        for padding, masked in model.VARIANTS[tag]:
            res = run_variant(fn, c, padding, masked)
            dist = check_variant(tag, c, padding, masked, res)
            pre = f"{tag}_out_{padding}_{'mask' if masked else 'nomask'}_"
            for k, v in res.items():
                data[pre + k] = v.numpy()
            data[pre + "distance"] = np.array([dist["loss"], dist["map"], dist["d_depth"]])
    path = os.path.join(HERE, "reconstruction_loss.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
