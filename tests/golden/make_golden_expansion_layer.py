#!/usr/bin/env python3
"""Golden vectors of the expansion layer: the REFERENCE's own ExpansionLayer (macarons/networks/ManyDepth.py:308-363) on the CPU in fp32,
this container only.

    python tests/golden/make_golden_expansion_layer.py     # writes tests/golden/expansion_layer.npz (data only)

Stored per case (GOLDEN_TAGS of tests/_expansion_layer_model.py; their seeded inputs are drawn there): x, x_add (where the case has one),
the layer's upconv.weight [Cin,Cmid,3,3], upconv.bias, iconv.weight [Cout,Cmid+Cadd,3,3], iconv.bias (the seeded ones, loaded into the
layer), output_size, the layer's y [B,Cout,H,W], the reference's distance to the fp64 model, and, from case b's layer, the names and shapes
of the reference's state_dict.  Asserted here: every distance is below 1e-5.
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
import _expansion_layer_model as model  # noqa: E402

REF = importlib.import_module("macarons.networks.ManyDepth")


def main():
    data = {}
    for tag in model.GOLDEN_TAGS:
        inp = model.make_inputs(tag)
        B, Cin, Cmid, Cadd, Cout, h, w, H, W = model.sizes(tag)
        layer = REF.ExpansionLayer(input_channels=Cin, inner_channels=Cmid, output_channels=Cout, output_size=(H, W), additional_channels=Cadd)
        layer.load_state_dict({"upconv.weight": torch.from_numpy(inp["up_weight"]), "upconv.bias": torch.from_numpy(inp["up_bias"]),
                               "iconv.weight": torch.from_numpy(inp["i_weight"]), "iconv.bias": torch.from_numpy(inp["i_bias"])}, strict=True)
        with torch.no_grad():
            y = layer(torch.from_numpy(inp["x"]), None if inp["x_add"] is None else torch.from_numpy(inp["x_add"])).numpy()
        dist = model.rel(y, model.forward(*model.args_of(inp))["y"])
        print(f"case {tag} {model.CASES[tag]['shape']}: reference vs model: y {dist:.1e}")
        assert y.shape == (B, Cout, H, W) and dist < 1e-5, dist
        for k in ("x", "up_weight", "up_bias", "i_weight", "i_bias"):
            data[f"{tag}_{k}"] = inp[k]
        if inp["x_add"] is not None:
            data[f"{tag}_x_add"] = inp["x_add"]
        data[f"{tag}_output_size"] = np.array([H, W])
        data[f"{tag}_y"], data[f"{tag}_distance"] = y, np.array(dist)
        if tag == "b":
            sd = layer.state_dict()
            data["state_dict_names"] = np.array(sorted(sd))
            data["state_dict_shapes"] = np.array([",".join(str(n) for n in sd[k].shape) for k in sorted(sd)])
    path = os.path.join(HERE, "expansion_layer.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
