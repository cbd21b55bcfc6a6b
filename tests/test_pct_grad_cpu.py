"""The PCTransformer gradient oracle against the reference: autograd.pc_transformer in fp64 reproduces the reference PCTransformer's own
fp64 autograd gradients (tests/golden/pct_grad.npz, made by make_golden_pct_grad.py) for every parameter and the points, in all
three cases.  The GPU backward (tests/test_pct_backward_gpu.py) is checked against the same fixture and this oracle."""
import os
import sys

import numpy as np
import pytest
import torch

from macarons_amd import autograd as A

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import weights  # noqa: E402
import make_golden_pct_grad as G  # noqa: E402

BOUND = 1e-9


@pytest.mark.parametrize("case", ["s16", "l150", "l2048"])
def test_composite_matches_reference_gradients(case):
    from macarons_amd.networks.SconeOcc import PCTransformer
    S, L, fd = G.CASES[case]
    m = PCTransformer(seq_len=L, pts_embedding_dim=128, feature_dim=fd)
    sd = weights.make_state_dict(weights.shapes_of(m), G.WEIGHT_SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.double()
    fx = np.load(os.path.join(HERE, "golden", "pct_grad.npz"))
    p = torch.from_numpy(G.inputs(case).astype(np.float64)).requires_grad_(True)
    y = A.pc_transformer(m, p)
    assert tuple(y.shape) == (S, fd)
    (y * torch.from_numpy(G.upstream(case).astype(np.float64))).sum().backward()
    worst = 0.0
    scale = max(float(fx[f"m_{case}_{n}"]) if f"m_{case}_{n}" in fx else float(np.abs(fx[f"g_{case}_{n}"]).max()) for n, _ in m.named_parameters())
    for n, prm in m.named_parameters():
        g = prm.grad.numpy()
        if f"s_{case}_{n}" in fx:
            got, ref, den = g.reshape(-1)[fx[f"idx_{case}_{n}"]], fx[f"s_{case}_{n}"], float(fx[f"m_{case}_{n}"])
            assert abs(np.abs(g).max() - den) <= BOUND * den, n
        else:
            got, ref, den = g, fx[f"g_{case}_{n}"], float(np.abs(fx[f"g_{case}_{n}"]).max())
        e = float(np.abs(got - ref).max() / max(den, 1e-30))
        if n.endswith("mhsa.w_k.bias"):             # mathematically zero: rounding noise that follows the summation order (threads);
            e = float(np.abs(got - ref).max() / scale)     # measured against the largest parameter gradient
        worst = max(worst, e)
        assert e < BOUND, (n, e)
    ref = fx[f"d_pc_{case}"]
    e = float(np.abs(p.grad.numpy() - ref).max() / np.abs(ref).max())
    worst = max(worst, e)
    assert e < BOUND, ("pc", e)
    print(f"ERR composite vs reference, case {case}: {worst:.2e}")
