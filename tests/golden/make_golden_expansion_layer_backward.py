#!/usr/bin/env python3
"""Golden vectors of the expansion layer's backward: the REFERENCE's own ExpansionLayer (macarons/networks/ManyDepth.py:308-363) on the CPU
in fp32 under autograd, this container only.

    python tests/golden/make_golden_expansion_layer_backward.py     # writes tests/golden/expansion_layer_backward.npz (data only)

Per case of GOLDEN_TAGS (tests/_expansion_layer_model.py), with the seeded inputs of make_inputs(tag) loaded into the layer and the seeded
d_y of tests/_expansion_layer_backward_model.py: d_y, the six gradients of sum(d_y * layer(x, x_add)) -- d_x, d_x_add (where the case has
an x_add), d_up_weight, d_up_bias, d_i_weight, d_i_bias -- and each one's distance to the fp64 model.  The inputs are not stored again:
they are regenerated from the seeds.  Asserted here: every distance is below 1e-5.
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
import _expansion_layer_backward_model as bmodel  # noqa: E402

REF = importlib.import_module("macarons.networks.ManyDepth")


def main():
    data = {}
    for tag in bmodel.GOLDEN_TAGS:
        inp, d_y = bmodel.make_inputs(tag), bmodel.make_d_y(tag)
        B, Cin, Cmid, Cadd, Cout, h, w, H, W = bmodel.sizes(tag)
        layer = REF.ExpansionLayer(input_channels=Cin, inner_channels=Cmid, output_channels=Cout, output_size=(H, W), additional_channels=Cadd)
        layer.load_state_dict({"upconv.weight": torch.from_numpy(inp["up_weight"]), "upconv.bias": torch.from_numpy(inp["up_bias"]),
                               "iconv.weight": torch.from_numpy(inp["i_weight"]), "iconv.bias": torch.from_numpy(inp["i_bias"])}, strict=True)
        x = torch.from_numpy(inp["x"]).requires_grad_(True)
        x_add = None if inp["x_add"] is None else torch.from_numpy(inp["x_add"]).requires_grad_(True)
        layer(x, x_add).backward(torch.from_numpy(d_y))
        got = dict(d_x=x.grad, d_x_add=None if x_add is None else x_add.grad, d_up_weight=layer.upconv.weight.grad,
                   d_up_bias=layer.upconv.bias.grad, d_i_weight=layer.iconv.weight.grad, d_i_bias=layer.iconv.bias.grad)
        want = bmodel.backward(*bmodel.args_of(inp), d_y)
        data[f"{tag}_d_y"] = d_y
        line = []
        for k in bmodel.NAMES:
            if got[k] is None:
                continue
            g = got[k].numpy()
            dist = bmodel.rel(g, want[k])
            assert g.shape == want[k].shape and dist < 1e-5, (tag, k, dist)
            data[f"{tag}_{k}"], data[f"{tag}_{k}_distance"] = g, np.array(dist)
            line.append(f"{k} {dist:.1e}")
        print(f"case {tag} {bmodel.CASES[tag]['shape']}: reference vs model: " + " ".join(line))
    path = os.path.join(HERE, "expansion_layer_backward.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
