"""The fp16 arena of the planes-GEMM tests (tests/_strided.py: HalfArena) on the CPU: the same placement and guard rules as the float
arena counted in halves, and a fill that is a NaN in EVERY half, so that a guard half reaching an accumulator poisons the result."""
import numpy as np
import pytest

from _strided import FILL_BITS, HALF_FILL_BITS, HALF_GUARD, HALF_LEAD, Arena, HalfArena


def test_fill_is_nan_in_every_half():
    a = HalfArena(3, 8, ld=16, offset=4)
    h = a.floats.numpy()
    assert h.dtype == np.float16 and np.isnan(h).all()
    assert (a.bits.numpy().view(np.uint16) == HALF_FILL_BITS).all()
    # the reason the float fill would not do: one of its two halves is an ordinary number
    assert np.isfinite(np.array([FILL_BITS], np.uint32).view(np.float16)).sum() == 1
    # a dot product over a row that runs into the padding is poisoned
    assert np.isnan(np.dot(h[a.start:a.start + 9].astype(np.float32), np.ones(9, np.float32)))


@pytest.mark.parametrize("offset", [0, 1, 4, 7])
@pytest.mark.parametrize("pad", [0, 4, 8])
def test_window_placement(offset, pad):
    rows, cols = 5, 8
    data = (np.arange(rows * cols).reshape(rows, cols) - 17).astype(np.float16)
    a = HalfArena(rows, cols, ld=cols + pad, offset=offset, data=data)
    assert a.ptr == a.bits.data_ptr() + 2 * (HALF_LEAD + offset)
    assert a.n == HALF_LEAD + offset + rows * (cols + pad) + HALF_GUARD
    assert 2 * HALF_LEAD == 4 * Arena.LEAD_N and 2 * HALF_GUARD == 4 * Arena.GUARD_N      # the same bytes as the float arena
    flat = a.floats.numpy()
    for r in range(rows):
        assert np.array_equal(flat[a.start + r * a.ld:a.start + r * a.ld + cols], data[r])
    assert np.array_equal(a.packed(), data) and a.packed().dtype == np.float16
    assert np.array_equal(a.packed_bits(), data.view(np.uint16))
    assert int(a.outside_mask().sum()) == a.n - rows * cols
    assert np.isnan(flat[a.outside_mask()]).all()
    a.check_guard()
    a.check_unchanged()
    a.window()[2, 3] = -1.0
    a.check_guard()
    with pytest.raises(AssertionError):
        a.check_unchanged()


@pytest.mark.parametrize("where,index", [("before the first row", lambda a: a.start - 1), ("before the first row", lambda a: 0),
                                         ("padding row 2 col 8", lambda a: a.start + 2 * a.ld + 8),
                                         ("padding row 4 col 15", lambda a: a.start + 4 * a.ld + 15),
                                         ("guard +0", lambda a: a.start + a.rows * a.ld),
                                         (f"guard +{HALF_GUARD - 1}", lambda a: a.n - 1)])
@pytest.mark.parametrize("value", [0.0, float("nan")])      # a plain NaN has other bits than the fill: compared as int16
def test_planted_overwrite_is_found(where, index, value):
    a = HalfArena(5, 8, ld=16, offset=4, data=np.zeros((5, 8), np.float16))
    i = index(a)
    a.floats[i] = value
    assert a.guard_violations() == [(i, where)]
    with pytest.raises(AssertionError, match="stray write"):
        a.check_guard("planted")
    with pytest.raises(AssertionError):
        a.check_unchanged()


def test_empty_output_keeps_the_fill():
    out = HalfArena(3, 4, ld=8)
    assert (out.bits.numpy().view(np.uint16) == HALF_FILL_BITS).all() and np.isnan(out.packed()).all()
    out.check_unchanged()
