#!/usr/bin/env python3
"""Generate tests/golden/scorer_grad.npz: the reference's own fp64 autograd gradients of the SH scorer (this container only).

    python tests/golden/make_golden_scorer_grad.py

SconeVis.compute_coverage_gain (weighted by w_gain [B,C]) and SconeVis.compute_visibilities (weighted by w_pair [B,C,N]) are
differentiated with respect to pts, harmonics and X_cam, for sigmoid and relu, on two inputs cut from scorer_b2_n500_c7.npz:
  case "4": the first 128 points of both clouds (pts_dim 4: the fourth channel gets a zero gradient);
  case "3": points 256..315 of cloud 1, xyz only (pts_dim 3), with that cloud's cameras.
Keys: {pts,harm,cams,w_gain,w_pair}{3,4} (float32 inputs) and g_{kind}_{act}_{wrt}{case} (float64), kind in gain / vis,
act in sig / relu, wrt in pts / harm / cams.  No pair sits on the relu kink: min |z| > 1e-4 is asserted.
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402

ref = _ref_import.load_reference()
import torch  # noqa: E402

from macarons_amd import autograd as A  # noqa: E402  (the fp64 z of every pair, for the kink check)


def cases():
    src = np.load(os.path.join(HERE, "scorer_b2_n500_c7.npz"))
    pts, harm, cams = src["pts"], src["harmonics"], src["cams"]
    rng = np.random.default_rng(21)
    out = {}
    for case, (p, h, c) in {"4": (pts[:, :128], harm[:, :128], cams),
                            "3": (pts[1:, 256:316, :3], harm[1:, 256:316], cams[1:])}.items():
        B, N, C = p.shape[0], p.shape[1], c.shape[1]
        out[case] = dict(pts=np.ascontiguousarray(p, np.float32), harm=np.ascontiguousarray(h, np.float32),
                         cams=np.ascontiguousarray(c, np.float32),
                         w_gain=rng.standard_normal((B, C)).astype(np.float32),
                         w_pair=rng.standard_normal((B, C, N)).astype(np.float32))
    return out


def main():
    SconeVis = ref["SconeVis"].SconeVis
    arrays = {}
    for case, d in cases().items():
        t = {k: torch.from_numpy(v).to(torch.float64) for k, v in d.items()}
        with torch.no_grad():
            rays = t["cams"][:, :, None, :] - t["pts"][:, None, :, :3]
            z = (A.sh_basis(rays / torch.linalg.norm(rays, dim=-1, keepdim=True)) * t["harm"][:, None]).sum(-1)
        zmin = float(z.abs().min())
        assert zmin > 1e-4, f"case {case}: a pair sits on the relu kink (min |z| = {zmin:.3e})"
        print(f"case {case}: B,N,C = {tuple(d['pts'].shape[:2]) + (d['cams'].shape[1],)}, min |z| = {zmin:.3e}")
        for k, v in d.items():
            arrays[f"{k}{case}"] = v
        for use_sigmoid in (True, False):
            m = SconeVis(use_sigmoid=use_sigmoid)
            act = "sig" if use_sigmoid else "relu"
            for kind in ("gain", "vis"):
                p, h, c = (t[k].clone().requires_grad_(True) for k in ("pts", "harm", "cams"))
                if kind == "gain":
                    loss = (m.compute_coverage_gain(p, h, c) * t["w_gain"]).sum()
                else:
                    loss = (m.compute_visibilities(p, h, c) * t["w_pair"]).sum()
                loss.backward()
                for wrt, g in (("pts", p.grad), ("harm", h.grad), ("cams", c.grad)):
                    arrays[f"g_{kind}_{act}_{wrt}{case}"] = g.numpy()
    path = os.path.join(HERE, "scorer_grad.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
