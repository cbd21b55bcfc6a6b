#!/usr/bin/env python3
"""Golden vectors of the disparity head: the REFERENCE's own DisparityLayer (macarons/networks/ManyDepth.py:366-384) on the CPU in fp32,
this container only.

    python tests/golden/make_golden_disparity_head.py     # writes tests/golden/disparity_head.npz (data only)

Stored per case (GOLDEN_TAGS of tests/_disparity_head_model.py, the cases small enough to commit; their seeded inputs are drawn there):
x, the layer's weight [1,C,3,3] and bias [1] (the seeded ones, loaded into the layer), g_out, the layer's y [B,1,Hs,Ws], the gradients
of sum(y * g_out) for x, weight and bias, the reference's distance to the fp64 model (y, d_x, d_weight, d_bias), and, from case a's
layer, the names and shapes of the reference's state_dict.  Asserted here: every distance is below 1e-5.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402

_ref_import.install_stubs()
import torch  # noqa: E402
import _disparity_head_model as model  # noqa: E402

REF = importlib.import_module("macarons.networks.ManyDepth")


def main():
    data = {}
    for tag in model.GOLDEN_TAGS:
        inp = model.make_inputs(tag)
        B, C, Hs, Ws = model.CASES[tag]["shape"]
        layer = REF.DisparityLayer(input_channels=C)
        layer.load_state_dict({"conv.weight": torch.from_numpy(inp["weight"])[None], "conv.bias": torch.from_numpy(inp["bias"])}, strict=True)
        x = torch.from_numpy(inp["x"]).requires_grad_(True)
        y = layer(x)
        (y[:, 0] * torch.from_numpy(inp["g_out"])).sum().backward()
        res = dict(y=y.detach().numpy(), d_x=x.grad.numpy(), d_weight=layer.conv.weight.grad.numpy(), d_bias=layer.conv.bias.grad.numpy())
        _, ym = model.forward(inp["x"], inp["weight"], inp["bias"])
        grads = model.backward(inp["x"], inp["weight"], ym, inp["g_out"])
        dist = np.array([model.rel(res["y"], ym)] + [model.rel(res[k], g) for k, g in zip(("d_x", "d_weight", "d_bias"), grads)])
        print(f"case {tag} {(B, C, Hs, Ws)}: reference vs model: y {dist[0]:.1e} d_x {dist[1]:.1e} d_weight {dist[2]:.1e} d_bias {dist[3]:.1e}")
        assert dist.max() < 1e-5, dist
        data[f"{tag}_x"], data[f"{tag}_g_out"] = inp["x"], inp["g_out"]
        data[f"{tag}_weight"], data[f"{tag}_bias"] = layer.conv.weight.detach().numpy(), layer.conv.bias.detach().numpy()
        data[f"{tag}_distance"] = dist
        for k, v in res.items():
            data[f"{tag}_{k}"] = v
        if tag == "a":
            sd = layer.state_dict()
            data["state_dict_names"] = np.array(sorted(sd))
            data["state_dict_shapes"] = np.array([",".join(str(n) for n in sd[k].shape) for k in sorted(sd)])
    path = os.path.join(HERE, "disparity_head.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
