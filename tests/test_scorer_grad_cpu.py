"""The scorer's gradient oracle against the reference: autograd.coverage_gain / autograd.visibilities in fp64 reproduce the reference's
own fp64 autograd gradients (tests/golden/scorer_grad.npz, made by make_golden_scorer_grad.py) with respect to pts, harmonics and
X_cam.  The GPU backward (tests/test_scorer_backward_gpu.py) is checked against the same fixture and this oracle."""
import os

import numpy as np
import pytest
import torch

from macarons_amd import autograd as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scorer_grad.npz")
# Measured worst 1.1e-10 (relu, per-pair weights, d_pts, case "4"); every other tensor is within 6e-11.  The reference differentiates
# through its angle route (acos / atan2, then the Legendre recurrences), this oracle through the Cartesian polynomials: two fp64 paths.
BOUND = 2e-10


@pytest.mark.parametrize("case", ["4", "3"])
@pytest.mark.parametrize("kind", ["gain", "vis"])
@pytest.mark.parametrize("act", ["sig", "relu"])
def test_oracle_gradients_match_reference(case, kind, act):
    f = np.load(GOLDEN)
    t = {k: torch.from_numpy(f[k + case]).to(torch.float64) for k in ("pts", "harm", "cams", "w_gain", "w_pair")}
    p, h, c = (t[k].clone().requires_grad_(True) for k in ("pts", "harm", "cams"))
    if kind == "gain":
        loss = (A.coverage_gain(p, h, c, act == "sig") * t["w_gain"]).sum()
    else:
        loss = (A.visibilities(p, h, c, act == "sig") * t["w_pair"]).sum()
    loss.backward()
    assert p.shape[-1] == int(case)
    for wrt, g in (("pts", p.grad), ("harm", h.grad), ("cams", c.grad)):
        ref = f[f"g_{kind}_{act}_{wrt}{case}"]
        err = float(np.abs(g.numpy() - ref).max() / np.abs(ref).max())
        assert err <= BOUND, (wrt, err)
    if case == "4":
        assert np.all(f[f"g_{kind}_{act}_pts4"][..., 3] == 0)
