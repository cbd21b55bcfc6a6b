"""The SconeVis gradient oracle against the reference: autograd.scone_vis in fp64 reproduces the reference SconeVis's own fp64 autograd
gradients (tests/golden/scone_vis_grad.npz, made by make_golden_scone_vis_grad.py) for every parameter, pts and view_harmonics.  The
GPU backward (tests/test_scone_vis_backward_gpu.py) is checked against the same fixture and this oracle.  The 2048-token case is
left to the GPU tests (its fp64 run takes too long here)."""
import os
import sys

import numpy as np
import pytest
import torch

from macarons_amd import autograd as A

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import weights  # noqa: E402
import make_golden_scone_vis_grad as G  # noqa: E402

BOUND = 1e-10


@pytest.mark.parametrize("case", ["333", "b3"])
def test_composite_matches_reference_gradients(case):
    from macarons_amd.networks import SconeVis
    m = SconeVis()
    sd = weights.make_state_dict(weights.shapes_of(m), 1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.double()
    src = np.load(os.path.join(HERE, "golden", "scone_vis.npz"))
    fx = np.load(os.path.join(HERE, "golden", "scone_vis_grad.npz"))
    kp, kv = G.CASES[case]
    p = torch.from_numpy(src[kp].astype(np.float64)).requires_grad_(True)
    v = torch.from_numpy(src[kv].astype(np.float64)).requires_grad_(True)
    y = A.scone_vis(m, p, v)
    (y * torch.from_numpy(G.upstream(case, tuple(y.shape)).astype(np.float64))).sum().backward()
    worst = 0.0
    for n, prm in m.named_parameters():
        g = prm.grad.numpy()
        if f"s_{case}_{n}" in fx:
            got, ref, den = g.reshape(-1)[fx[f"idx_{n}"]], fx[f"s_{case}_{n}"], float(fx[f"m_{case}_{n}"])
            assert abs(np.abs(g).max() - den) <= BOUND * den, n
        else:
            got, ref, den = g, fx[f"g_{case}_{n}"], float(np.abs(fx[f"g_{case}_{n}"]).max())
        e = float(np.abs(got - ref).max() / max(den, 1e-30))
        worst = max(worst, e)
        assert e < BOUND, (n, e)
    for name, t in (("pts", p.grad), ("vh", v.grad)):
        ref = fx[f"d_{name}_{case}"]
        e = float(np.abs(t.numpy() - ref).max() / np.abs(ref).max())
        worst = max(worst, e)
        assert e < BOUND, (name, e)
    print(f"ERR composite vs reference, case {case}: {worst:.2e}")
