#!/usr/bin/env python3
"""Golden vectors of the disparity-scales step of a depth-training step: the REFERENCE's own compute_depth_from_disparity,
compute_disparity_from_depth, get_regularity_loss_fn and regularity_tab (macarons/utility/depth_model_utils.py) on the CPU in fp32, this
container only, chained the way apply_depth_model (macarons_utils.py:959-1031) chains them -- that glue (the nearest upsampling, the mean
normalisation and mask zeroing, the reflection padding, the mean-plus-std threshold) is written here in this file's own words.

    python tests/golden/make_golden_disparity_scales.py     # writes tests/golden/disparity_scales.npz (data only)

Stored per case: the inputs (tests/_disparity_model.py draws them: smooth images, disparities of a ramp plus sinusoids at each scale's
own resolution, a rectangular mask hole), and per variant (mask on / off) depth [S,B,H,W], reg [S], tab, thr, error_mask and the
disparity gradients of sum_s c_s reg[s] + sum(g * depth) with the fixed c and g stored beside them, and the reference's distance to the
fp64 model.  Cases: see CASES in tests/_disparity_model.py (a .. e; f is GPU-only and has no golden).
Asserted here (conditions on the drawn inputs, not tolerances; a draw that fails one gets another seed): in the model, every block border
and mask-free neighbour pair of every scale differs by at least 1e-4 in n; at most 1 % of an image's pixels are undecided
(|tab - thr| < 1e-4 thr); the error mask of every image that is not fully masked holds both values.  And of the reference's fp32 results:
its error mask equals the model's at every pixel that is not undecided, and every sign it differentiates through is the model's (its
gradient lies within 1e-4 of the model's).
"""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402

_ref_import.install_stubs()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import _disparity_model as model  # noqa: E402

DMU = importlib.import_module("macarons.utility.depth_model_utils")
PARAMS = SimpleNamespace(znear=model.ZNEAR, zfar=model.ZFAR)


def reference(inp, masked, c, g):
    """The reference's functions on fp32 CPU tensors, glued as apply_depth_model glues them."""
    images = torch.from_numpy(inp["images"])
    B, H, W, _ = images.shape
    img = images.permute(0, 3, 1, 2)
    keep = torch.from_numpy(inp["mask"])[:, None] if masked else torch.ones(B, 1, H, W, dtype=torch.bool)
    leaves = [torch.from_numpy(d)[:, None].clone().requires_grad_(True) for d in inp["disps"]]
    reg_fn = DMU.get_regularity_loss_fn(PARAMS)
    depths, regs, first = [], [], None
    for leaf in leaves:
        depth = DMU.compute_depth_from_disparity(PARAMS, leaf)
        if depth.shape[-2:] != (H, W):
            depth = F.interpolate(depth, size=(H, W), mode="nearest")
        disparity = DMU.compute_disparity_from_depth(PARAMS, depth)
        normed = disparity / (disparity.mean((2, 3), keepdim=True) + 1e-7) * keep
        depths.append(depth[:, 0]), regs.append(reg_fn(disp=normed, img=img))
        if first is None:
            first = normed.detach()
    tab = DMU.regularity_tab(disp=F.pad(first, (1, 1, 1, 1), mode="reflect"), img=F.pad(img, (1, 1, 1, 1), mode="reflect"))[:, 0]
    thr = tab.reshape(B, -1).mean(1) + tab.reshape(B, -1).std(1)
    depth, reg = torch.stack(depths), torch.stack(regs)
    ((reg * torch.from_numpy(c)).sum() + (depth * torch.from_numpy(g)).sum()).backward()
    res = dict(depth=depth.detach().numpy(), reg=reg.detach().numpy(), tab=tab.numpy(), thr=thr.numpy(),
               error_mask=(tab < thr.view(B, 1, 1)).numpy())
    res.update({f"d_disp{s}": leaf.grad[:, 0].numpy() for s, leaf in enumerate(leaves)})
    return res


def check(tag, inp, masked, res, c, g):
    mask = inp["mask"] if masked else None
    gap, undecided_share, both, undecided = model.conditions(inp["disps"], inp["images"], mask)
    m = model.forward(inp["disps"], inp["images"], mask)
    grads = model.gradient(inp["disps"], inp["images"], mask, g, c)
    dist = [model.rel(res[k], m[k]) for k in ("depth", "reg", "tab", "thr")]
    dist.append(max(model.rel(res[f"d_disp{s}"], gm) for s, gm in enumerate(grads)))
    wrong = int(((res["error_mask"] != m["error_mask"]) & ~undecided).sum())
    print(f"case {tag} mask={int(masked)}: least pair gap {gap:.2e}; undecided {100 * undecided_share:.2f} %; error mask set on "
          f"{100 * m['error_mask'].mean():.1f} %; reference vs model: depth {dist[0]:.1e} reg {dist[1]:.1e} tab {dist[2]:.1e} thr {dist[3]:.1e} "
          f"d_disp {dist[4]:.1e}; decided error-mask pixels that differ {wrong}")
    assert gap >= 1e-4, gap
    assert undecided_share <= 0.01, undecided_share
    assert both
    assert wrong == 0
    assert dist[4] < 1e-4
    return np.array(dist)


def main():
    data = {}
    for tag in model.GOLDEN_TAGS:
        case = model.CASES[tag]
        inp = model.make_inputs(tag)
        S, (B, H, W) = len(inp["disps"]), inp["mask"].shape
        for s, d in enumerate(inp["disps"]):
            data[f"{tag}_disp{s}"] = d
        data[f"{tag}_images"], data[f"{tag}_mask"] = inp["images"], inp["mask"]
        c, g = model.upstream_weights(np.random.default_rng(100 + case["seed"]), S, B, H, W)
        for masked in case["variants"]:
            res = reference(inp, masked, c, g)
            pre = f"{tag}_out_{'mask' if masked else 'nomask'}_"
            data[pre + "distance"] = check(tag, inp, masked, res, c, g)
            data[pre + "c"], data[pre + "g"] = c, g
            for k, v in res.items():
                data[pre + k] = v
    # the fp32 identity the entry relies on: the depth -> disparity round trip, measured on case c's finest map
    d = torch.from_numpy(model.make_inputs("c")["disps"][0])
    back = DMU.compute_disparity_from_depth(PARAMS, DMU.compute_depth_from_disparity(PARAMS, d))
    print(f"round trip disparity -> depth -> disparity in fp32: max |difference| {float((back - d).abs().max()):.1e}")
    # and the conditions of the GPU-only case, on its seeded inputs
    inp = model.make_inputs("f")
    gap, share, both, _ = model.conditions(inp["disps"], inp["images"], inp["mask"])
    print(f"case f (no golden): least pair gap {gap:.2e}; undecided {100 * share:.2f} %; both values {both}")
    assert gap >= 1e-4 and share <= 0.01 and both
    path = os.path.join(HERE, "disparity_scales.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
