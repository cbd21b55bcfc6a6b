"""The arena helper of the strided C-ABI tests (tests/_strided.py) on the CPU: window placement, and that a one-element overwrite
in each guard region -- before the first row, a padding column, behind the last row -- is found and named."""
import numpy as np
import pytest
import torch

from _strided import FILL_BITS, GUARD, LEAD, Arena, Workspace, attention_ref, colmax_backward_ref


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_window_placement(offset, pad):
    rows, cols = 5, 7
    data = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
    a = Arena(rows, cols, ld=cols + pad, offset=offset, data=data)
    assert a.ptr == a.bits.data_ptr() + 4 * (LEAD + offset)
    assert a.n == LEAD + offset + rows * (cols + pad) + GUARD
    flat = a.floats.numpy()
    for r in range(rows):
        for c in range(cols):
            assert flat[LEAD + offset + r * (cols + pad) + c] == data[r, c]
    assert np.array_equal(a.packed(), data)
    assert int(a.outside_mask().sum()) == a.n - rows * cols
    bits = a.bits.numpy()
    assert (bits[a.outside_mask()] == np.int32(FILL_BITS)).all() and np.isnan(flat[a.outside_mask()]).all()
    a.check_guard()
    a.check_unchanged()
    a.window()[2, 3] = -1.0                     # inside the window: the guard does not care, the input check does
    a.check_guard()
    with pytest.raises(AssertionError):
        a.check_unchanged()


@pytest.mark.parametrize("where,index", [("before the first row", lambda a: a.start - 1), ("before the first row", lambda a: 0),
                                         ("padding row 2 col 7", lambda a: a.start + 2 * a.ld + 7),
                                         ("padding row 4 col 10", lambda a: a.start + 4 * a.ld + 10),   # the last row's padding
                                         ("guard +0", lambda a: a.start + a.rows * a.ld),
                                         ("guard +4095", lambda a: a.n - 1)])
@pytest.mark.parametrize("value", [0.0, float("nan")])      # a plain NaN has other bits than the fill: compared as int32
def test_planted_overwrite_is_found(where, index, value):
    a = Arena(5, 7, ld=11, offset=1, data=np.zeros((5, 7), np.float32))
    i = index(a)
    a.floats[i] = value
    bad = a.guard_violations()
    assert bad == [(i, where)]
    with pytest.raises(AssertionError, match="stray write"):
        a.check_guard("planted")
    with pytest.raises(AssertionError):
        a.check_unchanged()


def test_empty_output_and_workspace():
    out = Arena(3, 4, ld=8)                      # no data: the window holds the fill as well -- an unwritten output is visible
    assert (out.bits == FILL_BITS).all()
    out.check_unchanged()
    w = Workspace(1024)
    assert w.ptr % 4 == 0 and w.rows == 1 and w.cols == 256 and w.n == LEAD + 256 + GUARD
    w.window()[0, 255] = 1.0                     # the last float of the scratch is the entry's to write
    w.check_guard()
    w.floats[LEAD + 256] = 1.0                   # the one behind it is not
    assert w.guard_violations() == [(LEAD + 256, "guard +0")]


def test_references_handle_masks_and_lengths():
    rng = np.random.default_rng(0)
    S, L, H, qk, v = 2, 5, 4, 32, 128
    qkv = rng.standard_normal((S, L, 2 * qk + v)).astype(np.float32)
    full = attention_ref(qkv, H, qk, v)
    assert np.allclose(attention_ref(qkv, H, qk, v, mask=np.ones((S, 1, L, L), bool)), full, atol=1e-12)
    assert np.allclose(attention_ref(qkv, H, qk, v, lens=[L, 99]), full, atol=1e-12)
    # a fully masked query attends uniformly (-1e3, not -inf); a length of 1 (or 0: clamped) returns the first value row
    m = np.ones((S, 1, L, L), bool)
    m[0, 0, 3, :] = False
    y = attention_ref(qkv, H, qk, v, mask=m)
    assert np.allclose(y[0, 3], qkv[0, :, 2 * qk:].astype(np.float64).mean(0), atol=1e-9)
    y = attention_ref(qkv, H, qk, v, lens=[1, 0])
    assert np.allclose(y[0], np.broadcast_to(qkv[0, 0, 2 * qk:], (L, v)), atol=1e-12)
    assert np.allclose(y[1], np.broadcast_to(qkv[1, 0, 2 * qk:], (L, v)), atol=1e-12)
    x = np.zeros((1, 4, 2), np.float32)
    x[0, 1, 0] = x[0, 3, 0] = 5.0                # tie: row 1 wins; column 1 is all equal: row 0 wins
    g = np.ones((1, 4, 2), np.float32)
    d = colmax_backward_ref(x, g)
    assert d[0, 1, 0] == 4.0 and d[0, 0, 1] == 4.0 and d.sum() == 8.0
    d = colmax_backward_ref(x, g, lens=[1])
    assert d[0, 0, 0] == 4.0 and d[0, 0, 1] == 4.0
