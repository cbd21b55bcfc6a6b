"""Seeded plane-sweep cases at the sizes the goldens do not have (tests/golden/cost_volume.npz holds three shapes): built on the CPU, in
the shape of _cost_volume_model.load_case's dicts, with the conditions on the inputs that make the fp64 model a fair reference for an
fp32 kernel.  The conditions are properties of the inputs, not measurements of a kernel: tests/test_cost_volume_cpu.py asserts them for
every case below and tests/test_cost_volume_edges_gpu.py relies on them.  If a seed misses a condition, the seed changes, never the
condition.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cost_volume_model as model                                     # noqa: E402

C = 64
MARGIN = 1e-5                    # the sign margin of tests/test_cost_volume_backward_gpu.py
MIN_ABS_W = 1e-3                 # the golden generator's own bound on the smallest |w| of a bicubic tap
MIN_INSIDE = 0.5                 # share of (b,a,k,p) samples with a corner inside the source map
MIN_GOOD = 0.99                  # share of (b,k,p) positions that keep their weight

# tag -> (seed, B, A, H, W, Hf, Wf, D)
SHAPES = {
    "min":   (101, 1, 1, 2, 2, 1, 1, 1),        # the smallest sizes the entry admits; D = 1
    "row":   (102, 1, 2, 8, 12, 1, 5, 4),       # Hf = 1
    "col":   (103, 2, 1, 12, 8, 6, 1, 5),       # Wf = 1, portrait image, D = 4 + 1
    "full":  (104, 1, 3, 5, 7, 5, 7, 3),        # Hf = H, Wf = W (bicubic fraction 0), odd sizes
    "tile1": (105, 3, 2, 20, 28, 5, 13, 9),     # P = 65: one layout tile + 1, four sweep workgroups + 1; D = 2*4 + 1; B = 3
    "wide":  (106, 1, 8, 16, 24, 4, 6, 2),      # A = 8
    "scan":  (107, 3, 3, 36, 68, 9, 17, 6),     # n_dest = 1377: scan chunks of 2, one of 1, then empty ones; P = 153 = 2 tiles + 25
    "full2": (108, 1, 1, 24, 40, 24, 40, 5),    # ratio 1 at P = 960 = 15 whole layout tiles
}
TAGS = tuple(SHAPES)

# the stride loop of the backward's maximum: D*P = 66 048 elements per batch, one pass of 256 x 256 threads covers 65 536.  The
# weighted plane is the last one, whose first element is number 171*384 = 65 664; the planes MAXABS_SUB hold its quadruple.
MAXABS_SHAPE = (109, 2, 1, 16, 24, 16, 24, 172)
MAXABS_SUB = (168, 172)


def _rotations(n, gen, max_angle=0.1):
    """n rotations about random axes by angles in [-max_angle, max_angle] (Rodrigues, fp64)."""
    axis = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    th = ((torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * max_angle).view(n, 1, 1)
    K = torch.zeros(n, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


def inputs(seed, B, A, H, W, Hf, Wf, D):
    """The case dict (float32 CPU tensors + H, W, D): normal features, small rotations about random axes, translations within +-0.3,
    depth_bins = linspace(1, 9, D)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, Hf, Wf, generator=g)
    xa = torch.randn(B, A, C, Hf, Wf, generator=g)
    R = _rotations(B, g).float()
    Ra = _rotations(B * A, g).float().view(B, A, 3, 3)
    T = (torch.rand(B, 3, generator=g) * 2 - 1) * 0.3
    Ta = (torch.rand(B, A, 3, generator=g) * 2 - 1) * 0.3
    return dict(x=x, x_alpha=xa, R=R, T=T, R_alpha=Ra, T_alpha=Ta, depth_bins=torch.linspace(1.0, 9.0, D), H=H, W=W, D=D)


def sub_planes(c, lo, hi):
    """The same case on the planes lo..hi-1 only."""
    return dict(c, depth_bins=c["depth_bins"][lo:hi].clone(), D=hi - lo)


def conditions(c, seed):
    """dict(min_abs_w, inside_share, good [B,D,Hf,Wf] bool, good_share, lw [B,D,Hf,Wf] float32 seeded normal)."""
    Hf, Wf = c["x"].shape[-2:]
    cam = (c["R"], c["T"], c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"], Hf, Wf)
    with torch.no_grad():
        min_abs_w = float(model.tap_min_abs_w(*cam).min())
        g, _ = model.grid_coordinates(*cam)
        px, py = ((g[..., 0] + 1) * Wf - 1) / 2, ((g[..., 1] + 1) * Hf - 1) / 2
        inside = (px > -1) & (px < Wf) & (py > -1) & (py < Hf)                  # some corner of the bilinear cell lies in the map
        d = (model.sample(c["x_alpha"], g).mean(1) - c["x"].double()[:, :, None]).abs()    # [B,C,D,Hf,Wf]
    good = ~((d > 0) & (d <= MARGIN)).any(1)
    lw = torch.randn(good.shape, generator=torch.Generator().manual_seed(seed + 1000))
    return dict(min_abs_w=min_abs_w, inside_share=float(inside.double().mean()), good=good, good_share=float(good.double().mean()), lw=lw)


def holds(cond):
    return cond["min_abs_w"] >= MIN_ABS_W and cond["inside_share"] >= MIN_INSIDE and cond["good_share"] >= MIN_GOOD


def build_case(seed, B, A, H, W, Hf, Wf, D):
    """(case, conditions)."""
    c = inputs(seed, B, A, H, W, Hf, Wf, D)
    return c, conditions(c, seed)


def maxabs_case():
    """(the D = 172 case, its D = 4 sub-problem, the sub-problem's conditions)."""
    c = inputs(*MAXABS_SHAPE)
    sub = sub_planes(c, *MAXABS_SUB)
    return c, sub, conditions(sub, MAXABS_SHAPE[0])


def reference_gradients(c, weight):
    """fp64 autograd through the model: the gradients of sum(cost volume * weight) for x and x_alpha."""
    x6, xa6 = c["x"].double().requires_grad_(True), c["x_alpha"].double().requires_grad_(True)
    cv = model.cost_volume(x6, c["R"], c["T"], xa6, c["R_alpha"], c["T_alpha"], c["depth_bins"], c["H"], c["W"])
    return torch.autograd.grad((cv * weight.double()).sum(), (x6, xa6))
