"""The cases and bounds of the direct local-transformer tests (tests/_local_pct_cases.py), checked on the CPU: every bound that
tests/test_local_pct_gpu.py asserts comes from the oracle alone, and these are the conditions under which such a bound cannot hide a
failure.  Prints (with -s) the reference-alone numbers: the worst whole(r32), dep(r32) and dep(rsplit) of every case."""
import numpy as np
import pytest

import _local_pct_cases as lc


def test_case_builder_is_deterministic():
    """Two builds of a case are bit-equal and distinct cases differ; the shared arrays are read-only; the shapes are the stated ones."""
    for case in lc.CASES:
        a, b = lc.build_offsets(case), lc.build_offsets(case)
        assert a is not b and a.dtype == np.float32 and a.tobytes() == b.tobytes(), case
        assert a.shape == ((64 if case == "knn" else lc.S_SMALL), 16, 3), case
        assert lc.offsets(case).tobytes() == a.tobytes() and not lc.offsets(case).flags.writeable
    blobs = {lc.offsets(c).tobytes() for c in lc.CASES}
    assert len(blobs) == len(lc.CASES)
    r = lc.reference(2, 1.0, 0, "g0.05")
    assert lc.reference(2, 1.0, 0, "g0.05") is r and not r.ref.flags.writeable
    again = lc.Reference(2, 1.0, 0, "g0.05")
    assert again.ref.tobytes() == r.ref.tobytes() and again.r32.tobytes() == r.r32.tobytes()


def test_cases_are_what_they_are_called():
    o = lc.offsets("equal16")
    assert (o == o[:, :1]).all() and np.abs(o).min() > 0
    o = lc.offsets("pairs")
    assert (o[:, 0::2] == o[:, 1::2]).all() and len({r.tobytes() for r in o[0, 0::2]}) == 8
    assert not lc.offsets("zero").any()
    o = lc.offsets("mixed")
    assert np.abs(o[:, :8]).max() < 1e-2 and np.abs(o[:, 8:]).max() > 1.0
    for (name, scale) in lc.GAUSS:
        s = lc.offsets(name).std()
        assert 0.8 * scale < s < 1.2 * scale, (name, s)
    o = lc.offsets("knn")                                   # neighbours in ascending distance, inside the golden cloud's extent
    d = np.linalg.norm(o.astype(np.float64), axis=-1)
    assert (np.diff(d, axis=1) >= -1e-6).all() and d.max() < 1.0
    # the split of variant 6 reproduces x to max(2^-22 |x|, 2^-25)
    for case in lc.CASES:
        x = lc.offsets(case).astype(np.float64)
        assert (np.abs(lc.split_fp16(x) - x) <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25)).all(), case


def test_metrics_on_known_errors():
    """whole and dep measure what their names say: an error planted in one sequence and half shows there and nowhere else."""
    r = lc.reference(2, 1.0, 1, "g0.05")
    got = r.ref.copy()
    got[3, 128 + 5] += 1e-3
    w, d = r.whole(got), r.dep(got)
    assert w[3, 1] == pytest.approx(1e-3 / np.abs(r.ref[3, 128:]).max()) and np.count_nonzero(w) == 1
    assert d[3] == pytest.approx(1e-3 / np.abs(r.ref[3] - r.ref0[0]).max()) and np.count_nonzero(d) == 1
    z = lc.reference(2, 1.0, 1, "zero")
    assert not z.live.any() and np.isnan(z.dep(z.r32)).all() and z.bound_dep(6) is None and z.dep_r32 is None
    assert np.array_equal(z.ref, np.broadcast_to(z.ref0, z.ref.shape))


@pytest.mark.parametrize("seed,local_scale", lc.WEIGHT_SETS)
def test_conditions_hold_for_every_case(seed, local_scale):
    """8 * whole(r32) <= 1e-4 and max|ref - ref0| >= 1e-3 max|ref| wherever dep is asserted: for every transformer and case."""
    for t in range(3):
        for case in lc.CASES:
            r = lc.reference(seed, local_scale, t, case)
            r.check_conditions()
            assert r.live.all() or case in ("zero", "knn"), case
            if r.live.any():
                assert r.bound_dep(1) == r.bound_dep(5) == 8 * r.dep_r32 and r.bound_dep(6) == 8 * r.dep_r32 + 2 * r.dep_rsplit
                assert 0 < r.bound_dep(5) < r.bound_dep(6) < 0.05, (seed, local_scale, t, case, r.bound_dep(6))
            assert r.bound_whole == 8 * r.whole_r32 > 0


def test_print_reference_alone_table():
    """The worst reference-alone numbers per case over the weight sets and transformers (the figures NOTES.md records)."""
    print("\nREF case      whole(r32)  dep(r32)   dep(rsplit)  min dependence   [worst over 4 weight sets x 3 transformers]")
    worst_whole = {}
    for case in lc.CASES:
        rs = [lc.reference(s, k, t, case) for (s, k) in lc.WEIGHT_SETS for t in range(3)]
        w = max(r.whole_r32 for r in rs)
        live = [r for r in rs if r.live.any()]
        d32 = max((r.dep_r32 for r in live), default=float("nan"))
        dsp = max((r.dep_rsplit for r in live), default=float("nan"))
        dmin = min((float(r.dependence()[r.live].min()) for r in live), default=float("nan"))
        print(f"REF {case:9s} {w:10.2e} {d32:10.2e} {dsp:10.2e} {dmin:12.2e}")
        worst_whole[case] = w
    for (s, k) in lc.WEIGHT_SETS:
        w = max(lc.reference(s, k, t, c).whole_r32 for t in range(3) for c in lc.CASES)
        print(f"REF weights seed {s} x{k:g}: worst whole(r32) {w:.2e}")
    assert max(worst_whole.values()) * lc.MARGIN <= lc.CONTRACT
