"""The oracle of the ragged occupancy pass: autograd.scone_occ_ragged (J jobs in one call: padded global sequences with key masking and
masked pooling, one gather of the global features per row) in fp64 on the CPU against J separate autograd.scone_occ calls, each on its
own unpadded global sequence and its own rows, with the same neighbourhoods expressed as indices.  Outputs and all gradients (the
parameters' summed over the jobs, x, view_harmonics) agree to 1e-9 -- the two are the same arithmetic but for the order of a few sums --
and nothing changes when the padding rows of pc_global hold other values, NaN included.  The GPU backward
(tests/test_scone_occ_ragged_backward_gpu.py) is checked against this composite."""
import os
import sys

import numpy as np
import pytest
import torch

from macarons_amd import autograd as A

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import weights  # noqa: E402

BOUND = 1e-9
LG, GLOBAL_LEN, ROWS, CLOUD = 48, (48, 17, 33), (5, 1, 9), (40, 24, 16)


def _err(got, ref):
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


@pytest.fixture(scope="module")
def case():
    from macarons_amd.networks import SconeOcc
    saved = os.environ.pop("MCR_SCONE_OCC_BWD", None)          # (autograd.scone_occ: the all-torch composite)
    try:
        m = SconeOcc()
        sd = weights.make_state_dict(weights.shapes_of(m), 2)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m = m.double()
        rng = np.random.default_rng(7)
        J, T = len(ROWS), sum(ROWS)
        pcg = torch.from_numpy(rng.uniform(-.3, .3, (J, LG, 3)))
        x = torch.from_numpy(rng.uniform(-.4, .4, (T, 3)))
        vh = torch.from_numpy(rng.standard_normal((T, 64)) * 0.3)
        up = torch.from_numpy(rng.standard_normal((T, 1)))
        row_job = torch.from_numpy(np.repeat(np.arange(J), ROWS))
        r0 = np.concatenate(([0], np.cumsum(ROWS)))
        # per job and scale: a cloud and, per row, 16 indices into it (any 16 distinct points: the selection carries no gradient)
        clouds = [[torch.from_numpy(rng.uniform(-.3, .3, (1, M, 3))) for M in CLOUD] for _ in range(J)]
        idx = [[torch.from_numpy(np.stack([rng.permutation(M)[:16] for _ in range(ROWS[j])])[None]) for M in CLOUD] for j in range(J)]
        offsets = [torch.cat([clouds[j][i][0][idx[j][i][0]] - x[r0[j]:r0[j + 1], None, :] for j in range(J)]) for i in range(3)]
        # ---- the J separate calls
        ref_out, ref_dx, ref_dv = [], [], []
        m.zero_grad(set_to_none=True)
        for j in range(J):
            xj = x[r0[j]:r0[j + 1]][None].clone().requires_grad_(True)
            vj = vh[r0[j]:r0[j + 1]][None].clone().requires_grad_(True)
            y = A.scone_occ(m, pcg[j:j + 1, :GLOBAL_LEN[j]], clouds[j], xj, vj, idx[j])
            (y[0] * up[r0[j]:r0[j + 1]]).sum().backward()                # parameter gradients accumulate over the jobs
            ref_out.append(y[0].detach()); ref_dx.append(xj.grad[0]); ref_dv.append(vj.grad[0])
        ref = (torch.cat(ref_out), {n: p.grad.clone() for n, p in m.named_parameters()}, torch.cat(ref_dx), torch.cat(ref_dv))
    finally:
        if saved is not None:
            os.environ["MCR_SCONE_OCC_BWD"] = saved

    def ragged(pc_global):
        xr, vr = x.clone().requires_grad_(True), vh.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        y = A.scone_occ_ragged(m, pc_global, torch.tensor(GLOBAL_LEN, dtype=torch.int32), offsets, xr, vr, row_job)
        (y * up).sum().backward()
        return y.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}, xr.grad.clone(), vr.grad.clone()
    return dict(pcg=pcg, ref=ref, ragged=ragged, first=ragged(pcg))


def test_ragged_composite_matches_separate_calls(case):
    got, ref = case["first"], case["ref"]
    assert got[0].shape == (sum(ROWS), 1) and len(got[1]) == 172
    e_out, e_x, e_v = _err(got[0], ref[0]), _err(got[2], ref[2]), _err(got[3], ref[3])
    scale = max(float(t.abs().max()) for t in ref[1].values())
    e_w = max(float((got[1][n] - ref[1][n]).abs().max()) / max(float(ref[1][n].abs().max()), 1e-4 * scale) for n in ref[1])
    print(f"ERR scone_occ_ragged composite vs {len(ROWS)} separate calls (fp64): out {e_out:.2e}  params max {e_w:.2e}  d_x {e_x:.2e}  "
          f"d_vh {e_v:.2e}")
    assert max(e_out, e_w, e_x, e_v) < BOUND
    assert float(ref[2].abs().max()) > 0 and all(float(t.abs().max()) > 0 for n, t in ref[1].items() if not n.endswith("mhsa.w_k.bias"))


@pytest.mark.parametrize("fill", [float("nan"), 1e30, -3.0])
def test_padding_rows_are_never_read(case, fill):
    pcg = case["pcg"].clone()
    for j, n in enumerate(GLOBAL_LEN):
        pcg[j, n:] = fill
    got, first = case["ragged"](pcg), case["first"]
    assert torch.equal(got[0], first[0]) and torch.equal(got[2], first[2]) and torch.equal(got[3], first[3])
    assert all(torch.equal(got[1][n], first[1][n]) for n in first[1])
    assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[2], got[3], *got[1].values()))
