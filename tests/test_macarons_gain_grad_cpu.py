"""The composite of the MACARONS-regime gain (autograd.macarons_gain, the reference of the HIP backward's tests) on the CPU in fp64: a
case worked by hand and torch.autograd.gradcheck with respect to the per-point gains and the volumes, both distance factors."""
import pytest
import torch

from macarons_amd import autograd as A


def test_hand_case():
    """K = 1, S = 3, inverse = [0, 0, 1], n_unique = 2: d gains / d vis_u = g * vol / 3 * [2 f0, f1, 0]."""
    th, vol, g = 2.0, 1.7, 0.6
    vis = torch.tensor([[0.3, 0.8, 0.5]], dtype=torch.float64, requires_grad=True)
    world = torch.tensor([[[1.0, 0.0, 0.0, 9.0], [0.0, 3.0, 4.0, 9.0], [50.0, 50.0, 50.0, 9.0]]], dtype=torch.float64)    # d = 1, 5, (unused)
    inv = torch.tensor([[0, 0, 1]])
    nu = torch.tensor([2], dtype=torch.int32)
    cam = torch.zeros(1, 3, dtype=torch.float64)
    volume = torch.tensor([vol], dtype=torch.float64, requires_grad=True)
    for smooth, f0, f1 in ((False, 1.0, (th / 5.0) ** 2), (True, 1.0 / (1.0 + (1.0 / th) ** 2), 1.0 / (1.0 + (5.0 / th) ** 2))):
        vis.grad = volume.grad = None
        gains = A.macarons_gain(vis, world, inv, nu, cam, volume, th, smooth)
        mean = (2 * 0.3 * f0 + 0.8 * f1) / 3
        assert abs(float(gains.detach()[0]) - vol * mean) < 1e-14
        (gains * g).sum().backward()
        want = torch.tensor([[2 * f0, f1, 0.0]], dtype=torch.float64) * (g * vol / 3)
        assert torch.allclose(vis.grad, want, rtol=0, atol=1e-14), (vis.grad, want)
        assert float(vis.grad[0, 2]) == 0.0
        assert abs(float(volume.grad[0]) - g * mean) < 1e-14


def _gradcheck_inputs():
    K, S, th = 3, 11, 2.0
    gen = torch.Generator().manual_seed(5)
    cam = torch.rand(K, 3, generator=gen, dtype=torch.float64) - 0.5
    dirs = torch.randn(K, S, 3, generator=gen, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    radius = torch.tensor([0.4, 0.9, 1.5, 1.9, 2.2, 2.7, 3.5, 5.0, 1.2, 4.1, 0.7], dtype=torch.float64) * (th / 2.0)   # both sides of th
    world = torch.cat((cam[:, None, :] + dirs * radius[None, :, None], torch.rand(K, S, 1, generator=gen, dtype=torch.float64)), -1)
    inv = torch.stack((torch.randint(0, 7, (S,), generator=gen),       # camera 0: duplicates over 7 rows
                       torch.zeros(S, dtype=torch.int64),              # camera 1: n_unique = 0 (its map is not read for the value)
                       torch.full((S,), 4)))                           # camera 2: every sample on row 4
    nu = torch.tensor([7, 0, 5], dtype=torch.int32)
    vis = torch.rand(K, S, generator=gen, dtype=torch.float64, requires_grad=True)
    volume = (torch.rand(K, generator=gen, dtype=torch.float64) + 0.5).requires_grad_(True)
    return vis, world, inv, nu, cam, volume, th


@pytest.mark.parametrize("smooth", [False, True])
def test_gradcheck(smooth):
    vis, world, inv, nu, cam, volume, th = _gradcheck_inputs()
    d = (world[..., :3] - cam[:, None, :]).norm(dim=-1)
    assert float((d - th).abs().min()) > 1e-3 * th          # the threshold factor has a kink at d = th: stay away from it
    assert bool((d > th).any()) and bool((d < th).any())
    gains = A.macarons_gain(vis, world, inv, nu, cam, volume, th, smooth).detach()
    assert float(gains[1]) == 0.0 and float(gains[0]) > 0 and float(gains[2]) > 0
    assert torch.autograd.gradcheck(lambda v, w: A.macarons_gain(v, world, inv, nu, cam, w, th, smooth), (vis, volume),
                                    eps=1e-6, atol=1e-9, rtol=1e-7)
    # the identity form: no map, every camera counts
    assert torch.autograd.gradcheck(lambda v, w: A.macarons_gain(v, world, None, None, cam, w, th, smooth), (vis, volume),
                                    eps=1e-6, atol=1e-9, rtol=1e-7)
