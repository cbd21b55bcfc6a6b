"""Cases, references, metrics and bounds for the direct tests of the fused local transformers (csrc/local_pct{,5,6,7}.hip).
TEST INFRASTRUCTURE ONLY, CPU only: nothing here touches a GPU or a kernel's output.

WEIGHT SETS  (seed, local_scale) as tests/test_variant7_gpu.py::_occ builds them: SconeOcc() with weights.make_state_dict(seed); for
local_scale 4 every 2-D weight of the three local transformers is multiplied by 4 (soft-max logits 16x larger).

OFFSET CASES  [S, 16, 3] float32 from default_rng([KEY, index of the case]):
    g1e-3 .. g2   Gaussian at scales 1e-3, 1e-2, 0.05, 0.5, 2.0 (S = 9): from neighbours almost on the query to a query in empty space
    equal16       one token (scale 0.05) sixteen times: a cloud of duplicated points
    pairs         8 tokens (scale 0.05), each twice
    zero          all zeros: the query lies on sixteen copies of a surface point
    mixed         tokens 0..7 at scale 1e-3, tokens 8..15 at scale 1.0 in the same sequence
    knn           64 real neighbourhoods: oracle.knn.knn_offsets of the first 64 queries of scone_occ.npz's m1024_q300 cloud

REFERENCES per (weight set, transformer, case), all from oracle.nets.pc_transformer, read-only and cached:
    ref     fp64 output                       ref0    fp64 output of all-zero offsets (one row: it is the same for every sequence)
    r32     the oracle evaluated in float32   rsplit  fp64 oracle on the offsets as variant 6 carries them: hi = fp16(x),
                                                      lo = fp16(x - hi), value hi + lo

METRICS, both PER SEQUENCE:
    whole(got)  [S, 2]  max|got - ref| / max|ref| inside the sequence and the half (columns 0..127 max pool, 128..255 average pool)
    dep(got)    [S]     max|got - ref| / max|ref - ref0| over the sequence's 256 columns: the error relative to the part of the output
                        that depends on the offsets at all (at scale 1e-3 that part is 1e-3 .. 2e-3 of the output; the rest is bias, and a
                        max-norm over the whole output cannot see it).  NaN for a sequence whose offsets are all zero (0 / 0).

BOUNDS, from the reference alone, never from a kernel.  A bound belongs to a (weight set, transformer, case): the WORST sequence of the
reference's own float32 evaluation is the scale of fp32-class rounding on these inputs and weights, and every sequence of a kernel's
output must stay inside a fixed multiple of it (the rounding error of one single sequence is a random draw; its worst over the case is
the estimate of the scale).
    bound_whole = 8 * max whole(r32)
    bound_dep   = 8 * max dep(r32)                         variants 1 and 5
    bound_dep   = 8 * max dep(r32) + 2 * max dep(rsplit)   variant 6
8 = 4 (variant 6 carries 22 operand bits against fp32's 24) x 2 (a summation order that differs from numpy's); the 2 on the split term:
the kernel splits every activation as well as the input (local_pct6.hip now splits 2^8 x, which is finer than rsplit's plain split; the
term stays as the allowance it was set as).  check_conditions() asserts what keeps a bound from hiding a failure:
8 * whole(r32) <= 1e-4 (the project's contract) and max|ref - ref0| >= 1e-3 max|ref| for every sequence that gets a dep check.
"""
import contextlib
import functools
import io
import os
import sys

import numpy as np

from conftest import golden

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import weights  # noqa: E402
from oracle import knn, nets  # noqa: E402

WEIGHT_SETS = ((2, 1.0), (7, 1.0), (11, 1.0), (2, 4.0))
GAUSS = (("g1e-3", 1e-3), ("g1e-2", 1e-2), ("g0.05", 0.05), ("g0.5", 0.5), ("g2", 2.0))
CASES = tuple(n for n, _ in GAUSS) + ("equal16", "pairs", "zero", "mixed", "knn")
S_SMALL = 9
# The key of the draws.  On the x4 weight set the oracle's own float32 evaluation is 5e-6 .. 3e-5 from its float64 one depending on the
# draw (a sharp soft-max on paired tokens is the worst), and about one key in three has a sequence beyond the 1.25e-5 that the condition
# 8 * whole(r32) <= 1e-4 allows.  The keys 1 .. 12 were scanned ON THE ORACLE ALONE (no kernel involved); 2 meets the conditions in every
# case with room to spare (worst whole(r32) 8.7e-6), so a BLAS with another summation order does not flip them.
KEY = 2
CONTRACT = 1e-4          # the project's accuracy contract for variants 1, 5, 6
MARGIN = 8.0             # 4 (22 operand bits vs 24) x 2 (summation order)
MARGIN_SPLIT = 2.0       # the kernel splits every activation as well as the input
MIN_DEPENDENCE = 1e-3    # max|ref - ref0| / max|ref| of every sequence with a dep check


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def module(seed, local_scale):
    """(SconeOcc on the CPU with the weight set loaded, its state dict as float32 numpy arrays)."""
    import torch
    from macarons_amd.networks import SconeOcc
    with contextlib.redirect_stdout(io.StringIO()):
        m = SconeOcc()
    sd = weights.make_state_dict(weights.shapes_of(m), seed)
    if local_scale != 1.0:
        sd = {k: (v * np.float32(local_scale) if (k.startswith("local_transformers.") and k.endswith("weight") and v.ndim == 2) else v)
              for k, v in sd.items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval(), sd


def build_offsets(case):
    """A fresh [S, 16, 3] float32 array of the case (a function of the case's name alone)."""
    rng = np.random.default_rng([KEY, CASES.index(case)])
    S = S_SMALL
    gauss = dict(GAUSS)
    if case in gauss:
        o = rng.standard_normal((S, 16, 3)) * gauss[case]
    elif case == "equal16":
        o = np.repeat(rng.standard_normal((S, 1, 3)) * 0.05, 16, axis=1)
    elif case == "pairs":
        o = np.repeat(rng.standard_normal((S, 8, 3)) * 0.05, 2, axis=1)
    elif case == "zero":
        o = np.zeros((S, 16, 3))
    elif case == "mixed":
        o = rng.standard_normal((S, 16, 3)) * np.where(np.arange(16) < 8, 1e-3, 1.0)[None, :, None]
    elif case == "knn":
        g = golden("scone_occ")
        o = knn.knn_offsets(g["m1024_q300_x"][:, :64], g["m1024_q300_pc"], 16)[0][0]
    else:
        raise KeyError(case)
    o = np.ascontiguousarray(o, dtype=np.float32)
    assert o.shape[1:] == (16, 3)
    return o


@functools.lru_cache(maxsize=None)
def offsets(case):
    return _ro(build_offsets(case))


def split_fp16(x):
    """x as variant 6 carries an operand: hi = fp16(x), lo = fp16(x - hi); the value is hi + lo (float64, exact)."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64)


def whole(got, ref):
    """[S, 2]: max|got - ref| / max|ref| per sequence and half (max pool, average pool)."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 2, 128), np.asarray(ref, np.float64).reshape(-1, 2, 128)
    return np.abs(got - ref).max(-1) / np.abs(ref).max(-1)


def dep(got, ref, ref0, live):
    """[S]: max|got - ref| / max|ref - ref0| per sequence; NaN where `live` is False (an all-zero sequence)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    num, den = np.abs(got - ref).max(-1), np.abs(ref - ref0).max(-1)
    out = np.full(len(ref), np.nan)
    out[live] = num[live] / den[live]
    return out


class Reference:
    """The references of one (weight set, transformer, case) and the bounds that follow from them."""

    def __init__(self, seed, local_scale, t, case):
        _, sd = module(seed, local_scale)
        pre = f"local_transformers.{t}."
        offs = offsets(case)
        self.key = (seed, local_scale, t, case)
        self.offsets = offs
        self.live = _ro(np.abs(offs).reshape(len(offs), -1).max(-1) > 0)              # sequences that get a dep check
        self.ref = _ro(nets.pc_transformer(sd, pre, offs, np.float64))
        self.ref0 = _ro(nets.pc_transformer(sd, pre, np.zeros((1, 16, 3), np.float32), np.float64))
        self.r32 = _ro(nets.pc_transformer(sd, pre, offs, np.float32))
        self.rsplit = _ro(nets.pc_transformer(sd, pre, split_fp16(offs), np.float64))
        assert self.r32.dtype == np.float32 and self.ref.dtype == np.float64
        self.whole_r32 = float(self.whole(self.r32).max())
        self.dep_r32 = float(np.nanmax(self.dep(self.r32))) if self.live.any() else None
        self.dep_rsplit = float(np.nanmax(self.dep(self.rsplit))) if self.live.any() else None
        self.bound_whole = MARGIN * self.whole_r32

    def whole(self, got):
        return whole(got, self.ref)

    def dep(self, got):
        return dep(got, self.ref, self.ref0, self.live)

    def dependence(self):
        """[S]: max|ref - ref0| / max|ref|, the offset-dependent share of every sequence's output."""
        return np.abs(self.ref - self.ref0).max(-1) / np.abs(self.ref).max(-1)

    def bound_dep(self, variant):
        if self.dep_r32 is None:
            return None
        if variant in (1, 5):
            return MARGIN * self.dep_r32
        if variant == 6:
            return MARGIN * self.dep_r32 + MARGIN_SPLIT * self.dep_rsplit
        raise ValueError(f"no dep bound for variant {variant}")

    def check_conditions(self):
        assert np.isfinite(self.ref).all() and np.isfinite(self.r32).all() and np.isfinite(self.rsplit).all(), self.key
        assert self.bound_whole <= CONTRACT, (self.key, self.whole_r32)
        d = self.dependence()[self.live]
        assert d.size == 0 or d.min() >= MIN_DEPENDENCE, (self.key, float(d.min()))


@functools.lru_cache(maxsize=None)
def reference(seed, local_scale, t, case):
    return Reference(seed, local_scale, t, case)
