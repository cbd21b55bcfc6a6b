"""The HIP backward of the plane sweep without a GPU: the route switch, the host layer's refusal of CPU tensors, and the C ABI's two
symbols (declared, exported, and the workspace size's arithmetic, which is plain host code)."""
import ctypes

import pytest
import torch

from macarons_amd import _lib, autograd, build, ops


def test_backward_mode_follows_the_environment(monkeypatch):
    monkeypatch.delenv("MCR_COST_VOLUME_BWD", raising=False)
    assert autograd.cost_volume_backward_mode() == "hip"
    for value, mode in (("composite", "composite"), ("COMPOSITE", "composite"), ("hip", "hip"), ("", "hip"), ("something", "hip")):
        monkeypatch.setenv("MCR_COST_VOLUME_BWD", value)
        assert autograd.cost_volume_backward_mode() == mode, value


def test_ops_entry_refuses_cpu_tensors():
    x, xa = torch.zeros(1, 64, 2, 3), torch.zeros(1, 1, 64, 2, 3)
    with pytest.raises(_lib.MacaronsHipError, match="HIP device"):
        ops.cost_volume_backward(x, xa, torch.zeros(1, 2, 12), torch.ones(2), torch.zeros(1, 2, 2, 3), 8, 12)


def test_symbols_are_declared_and_exported():
    names = _lib.declared_symbols()
    assert "mcr_cost_volume_backward" in names and "mcr_cost_volume_backward_workspace_bytes" in names
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "mcr_cost_volume_backward") and hasattr(L, "mcr_cost_volume_backward_workspace_bytes")


def test_workspace_size():
    L = ctypes.CDLL(build.build())
    f = L.mcr_cost_volume_backward_workspace_bytes
    f.restype = ctypes.c_size_t
    i64 = ctypes.c_int64

    def size(B=1, A=2, C=64, Hf=64, Wf=114, D=96):
        return int(f(i64(B), i64(A), i64(C), i64(Hf), i64(Wf), i64(D)))

    for name in ("B", "A", "C", "Hf", "Wf", "D"):
        assert size(**{name: 0}) == 0 and size(**{name: -3}) == 0, name
    sizes = [size(D=d) for d in (1, 2, 5, 96, 97)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert size() % 16 == 0
    # it holds the sign states (16 bytes per (b,k,p)) and 8 bytes for each of the four corners of every (b,a,k,p), and nothing with a
    # channel axis per (source, plane, position): upstream's warped tensor alone is B*D*A*C*Hf*Wf*4 bytes
    P = 64 * 114
    assert size() >= 96 * P * 16 + 4 * 2 * 96 * P * 8
    assert size() < 2 * 96 * 64 * P * 4 // 4
    # more corner contributions than the lists can index: refused by the entry, so no size
    assert size(B=64, A=8, Hf=512, Wf=512, D=96) == 0
