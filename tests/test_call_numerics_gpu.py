"""The numerics variant is a property of a CALL (csrc/numerics.h: the scoped entries fix it when they open their VariantScope), and
the SconeOcc forwards give the same bits with and without their side streams (csrc/side_stream.h).

The probe of the first two tests is ops.attention_packed at heads (32, 128), S = 2, L = 65: one tile plus one key, the smallest shape
that runs attention_mfma_kernel, whose P V product is fp16 hi/lo on variant 6 and fp32 on variant 1.  It needs no parameter blob, so a
numerics mix-up can only give other bits, never an out-of-range read."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, QK, V, S, L = 4, 32, 128, 2, 65


@pytest.fixture(scope="module")
def probe(dev):
    """(qkv, the other variant, its single-thread bits, the default's single-thread bits); the two outputs differ, else the tests
    below would prove nothing."""
    from macarons_amd import ops
    qkv = torch.randn(S, L, 2 * QK + V, generator=torch.Generator().manual_seed(7)).to(dev)
    other = 1 if ops.current_variant() in (6, 7) else 6                  # (1 unless a whole suite runs on MCR_LOCAL_PCT_VARIANT = 1 or 5)
    with ops.variant(other):
        y_other = ops.attention_packed(qkv, H, QK, V)
    y_default = ops.attention_packed(qkv, H, QK, V)
    assert ops.attention_packed(qkv, H, QK, V).equal(y_default)
    assert not torch.equal(y_other, y_default), "the probe does not tell the two variants apart: pick another seed"
    return qkv, other, y_other, y_default


def test_a_failed_call_consumes_the_one_shot(dev, probe):
    """mcr_call_variant(v), then a scoped entry that fails validation before any launch: the next, plain call runs on the default."""
    from macarons_amd import ops
    from macarons_amd._lib import lib
    qkv, other, y_other, y_default = probe
    i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    out = torch.zeros(S, L, V, device=dev)
    assert lib().mcr_call_variant(i32(other)) == 0
    rc = lib().mcr_attention(vp(qkv.data_ptr()), i64(2 * QK + V), vp(out.data_ptr()), i64(V), i64(0), i64(L), i32(H), i32(QK), i32(V), ops._stream())
    assert rc == 1 and not out.any()                                     # "empty problem": nothing launched
    y = ops.attention_packed(qkv, H, QK, V)
    assert torch.equal(y, y_default) and not torch.equal(y, y_other)


def test_two_host_threads_keep_their_own_variant(dev, probe):
    """Thread A inside ops.variant(other), thread B on the default, ~50 probe calls each at the same time (ctypes releases the GIL):
    every output of A has the other variant's single-thread bits, every output of B the default's."""
    from macarons_amd import ops
    qkv, other, y_other, y_default = probe
    n, outs, errors = 50, {"a": [], "b": []}, []
    start = threading.Barrier(2, timeout=60)

    def work(name, variant):
        try:
            start.wait()
            if variant:
                with ops.variant(variant):
                    outs[name] = [ops.attention_packed(qkv, H, QK, V) for _ in range(n)]
            else:
                outs[name] = [ops.attention_packed(qkv, H, QK, V) for _ in range(n)]
        except BaseException as e:                                       # noqa: BLE001  (reported by the main thread)
            errors.append((name, repr(e)))

    threads = [threading.Thread(target=work, args=("a", other), daemon=True), threading.Thread(target=work, args=("b", 0), daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive(), "a probe thread did not finish"
    assert not errors, errors
    torch.cuda.synchronize()
    assert len(outs["a"]) == n and len(outs["b"]) == n
    for i in range(n):
        assert torch.equal(outs["a"][i], y_other), f"thread A, call {i}"
        assert torch.equal(outs["b"][i], y_default), f"thread B, call {i}"


def test_occ_forwards_without_side_streams_give_the_same_bits(dev, tmp_path):
    """MCR_OCC_OVERLAP=0 (read once per process, so: a fresh child) puts the global transformer, the early x embedding and the cloud
    build back on the caller's stream: the same kernels in the same per-stream order, so the dense forward (single call, and
    phase 1 + phase 2: _occ_forwards.dense_two_phase, which checks that phases 1 and 2 reach the entry) and the ragged forward on
    m1024_q300 return the bits of the default, side streams on."""
    import _occ_forwards as helper
    env = dict(os.environ, MCR_OCC_OVERLAP="0")
    r = subprocess.run([sys.executable, os.path.abspath(helper.__file__), str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "OCC_FORWARDS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.environ.get("MCR_OCC_OVERLAP", "1")[:1] != "0", "this process must run with the side streams on"
    mine = helper.occ_forwards(dev)
    for name in helper.NAMES:
        theirs = np.load(os.path.join(str(tmp_path), name + ".npy"))
        assert theirs.shape == mine[name].shape and np.isfinite(theirs).all(), name
        assert np.array_equal(theirs, mine[name]), name
