"""Helper of tests/test_call_numerics_gpu.py: the three SconeOcc forwards on the smallest SconeOcc golden (scone_occ.npz, tag
m1024_q300, its recorded draws) -- the dense forward as a single call, the dense forward as phase 1 + phase 2, and the ragged
forward on the same data as one job.

Run as a script (a fresh process, so that it reads its own MCR_OCC_OVERLAP) it writes the three outputs as <dir>/<name>.npy:
    python tests/_occ_forwards.py DIR"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from conftest import golden  # noqa: E402
import weights  # noqa: E402

NAMES = ("dense", "two_phase", "ragged")
TAG = "m1024_q300"


def dense_two_phase(m, pc, x, vh, perms, phases=None):
    """The dense forward as mcr_scone_occ_forward_phase 1, then 2, through ops.scone_occ_forward itself.  Not through
    forward_begin / forward(begun=...): SconeOcc.forward honours a handle only for a global down-sample of seq_len = 2048 points,
    so on a cloud of 1024 points it would drop the handle and run the single call again.  phases (a list): the `phase` argument
    of every call that reaches mcr_scone_occ_forward_phase from here is appended."""
    from macarons_amd import _lib, ops
    table, blobs, head = m._images(ops.current_variant())
    sizes = m.scale_sizes(pc.shape[1])
    pc_global = m._take(pc, perms[0])                                    # the draws and down-samples of SconeOcc.forward
    scales = [pc.contiguous()]
    for p in perms[1:]:
        scales.append(m._take(scales[-1], p))
    assert [s.shape[1] for s in scales] == sizes
    x, vh, Lg = x.contiguous(), vh.contiguous(), pc_global.shape[1]
    L = _lib.lib()
    entry = L.mcr_scone_occ_forward_phase

    def spy(*args):                                                      # what reaches the C entry: `phase` is its argument 17
        if phases is not None:
            phases.append(args[17].value)
        return entry(*args)

    L.mcr_scone_occ_forward_phase = spy
    try:
        assert ops.scone_occ_forward(None, [scales[0], None, None], x, None, table, blobs, head, None, phase=1, M_scale=sizes, Lg=Lg) is None
        return ops.scone_occ_forward(pc_global, scales, x, vh, table, blobs, head, None, phase=2)
    finally:
        L.mcr_scone_occ_forward_phase = entry


def occ_forwards(dev):
    """{name: numpy [Q, 1]} for NAMES."""
    from macarons_amd.networks import SconeOcc
    m = SconeOcc()
    sd = weights.make_state_dict(weights.shapes_of(m), 2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    g = golden("scone_occ")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    perms = [torch.from_numpy(g[f"{TAG}_perm{i}"].astype(np.int64)) for i in range(3)]
    pc, x, vh = T(g[f"{TAG}_pc"]), T(g[f"{TAG}_x"]), T(g[f"{TAG}_vh"])
    M, Q = pc.shape[1], x.shape[1]
    with torch.no_grad():
        dense = m(pc, x, vh, perms=perms).clone()
        phases = []
        two = dense_two_phase(m, pc, x, vh, perms, phases).clone()
        assert phases == [1, 2], phases
        ragged = m.forward_ragged(pc[0].contiguous(), [M], x[0].contiguous(), vh[0].contiguous(), [Q], perms=[perms]).clone()
    torch.cuda.synchronize()
    return {"dense": dense.cpu().numpy().reshape(Q, 1), "two_phase": two.cpu().numpy().reshape(Q, 1), "ragged": ragged.cpu().numpy().reshape(Q, 1)}


if __name__ == "__main__":
    for name, y in occ_forwards(torch.device("cuda:0")).items():
        np.save(os.path.join(sys.argv[1], name + ".npy"), y)
    print("OCC_FORWARDS_OK", flush=True)
