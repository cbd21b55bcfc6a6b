"""The range guard of the default numerics, shared by SconeOcc and SconeVis: THE place that says who reads the fp16 range flag and when.

Variant 6 (and the opt-in 7) runs the matrix products on fp16 hi/lo planes, valid for |activation| < 65504; the reference is plain fp32
(Attention.py:98-128) and cannot overflow there.  The kernels OR a device flag when an output comes out non-finite -- what an
out-of-range activation turns into -- and the forward can be repeated on variant 5 (bf16 hi/mid/lo, the whole fp32 range).
`range_guard` says who looks at the flag:
  "sync"  (default: correct for a drop-in caller -- the reference never returns NaN here) read the flag after every forward (one
          4-byte read-back = a pipeline drain) and repeat that forward at once on variant 5: the FIRST overflowed stand-alone forward
          already returns finite values within the 1e-4 contract;
  "defer" leave it in range_flag() for the caller: nbv_step / macarons_nbv_decision switch both networks to this for their duration
          (range_scope), make SconeVis report into SconeOcc's flag and check that ONE flag once, at the end of the decision (the
          performance paths never pay the per-forward read-back).  Whoever deferred owns the clearing;
  "async" (opt-in) never stalls: after every forward the flag is copied to pinned host memory behind the kernels; the NEXT forward (or
          check_range()) looks at copies that have landed.  A set flag means an earlier forward returned non-finite values (visible as
          such to the caller): it is reported once (RuntimeWarning) and every later forward of this module runs on variant 5 -- for a
          caller that keeps upstream's chunk loop, cannot afford a device->host round trip per chunk, and checks
          check_range(wait=True) at its own boundaries;
  "off"   no check.
Under stream capture "sync" / "async" act as "defer": the flag kernel stays in the graph, the read-back does not.

A guarded forward is: _range_reenter() (the preamble) -> _arm_range() -> the kernels, which write the flag -> _settle_range().
"""
import contextlib
import warnings

import torch

from .. import ops


class RangeGuard:
    """Mixin in front of nn.Module: the guard's state and protocol (see the module docstring for the four modes)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.range_guard = "sync"
        self._range_flag = None
        self._range_pending = []            # (pinned host int32 [1], event) of forwards whose flag has not been looked at yet
        self._range_pool = []               # pinned buffers whose copy was looked at: taken again by _post_range_check
        self._full_range = False            # True once an overflow was seen ("async"): variant 5 from then on

    def range_flag(self):
        """int32 device tensor [1]: 1 if a forward since clear_range_flag() produced a non-finite occupancy (None before the first
        guarded forward)."""
        return self._range_flag

    def _effective_guard(self):
        """range_guard, except under stream capture: a read-back ("sync") or a host copy ("async") cannot be part of a graph, so a
        captured forward leaves the flag in range_flag() ("defer") for whoever replays the graph to look at."""
        g = self.range_guard
        if g in ("sync", "async") and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return "defer"
        return g

    def _range_reenter(self):
        """Preamble of a forward: under "async" look at the copies that have landed; -> True when this forward has to re-enter on
        variant 5 (an earlier forward overflowed the fp16 split: full range from then on)."""
        if self._effective_guard() == "async" and (self._range_pending or self._full_range):
            self.check_range(_stacklevel=4)             # (the warning names the caller of forward, as a direct call from forward would)
        return self._full_range and ops.current_variant() in (6, 7)

    def _arm_range(self, device, guard):
        """The flag a guarded forward on `device` hands to its kernels (guard: _effective_guard(), not "off"): created when missing or
        on another device, else zeroed under "sync" / "async" and left alone under "defer" (the decision that deferred clears it)."""
        if self._range_flag is None or self._range_flag.device != device:
            self._range_flag = torch.zeros(1, dtype=torch.int32, device=device)
        elif guard in ("sync", "async"):
            self._range_flag.zero_()
        return self._range_flag

    def _settle_range(self, flag, guard, rerun):
        """After the kernels that write `flag` were queued (flag None: an unguarded forward, nothing to do).  "sync" with the flag set
        (the read-back): -> rerun() on variant 5, the full-range result; "async": the pinned copy is posted.  -> None otherwise."""
        if flag is not None and guard == "sync" and int(flag):
            with ops.variant(5):
                return rerun()
        if flag is not None and guard == "async":
            self._post_range_check(flag)
        return None

    @contextlib.contextmanager
    def range_scope(self, mode, device=None, peer=None):
        """One decision's guard: this module runs in `mode` for the duration, with its flag cleared on entry (device: created there
        first if need be, see clear_range_flag).  peer (SconeVis -- its encoders run on the same fp16 planes -- or any object; one
        without a guard is left untouched) takes the same mode and reports into THIS module's flag: one read-back covers both
        networks.  On every exit, an exception included, this module's mode and the peer's mode and flag are what they were (this
        module's own flag stays: it is what the decision hands out as `range_flag`)."""
        prev = self.range_guard
        peer_prev = (peer.range_guard, peer._range_flag) if hasattr(peer, "range_guard") else None
        try:
            self.range_guard = mode
            if peer_prev is not None:
                peer.range_guard = mode
            self.clear_range_flag(device)
            if peer_prev is not None:
                peer._range_flag = self._range_flag
            yield self
        finally:
            self.range_guard = prev
            if peer_prev is not None:
                peer.range_guard, peer._range_flag = peer_prev

    def _post_range_check(self, flag):
        """"async" guard: queue a copy of the flag to pinned host memory behind the forward's kernels (no stall)."""
        host = self._range_pool.pop() if self._range_pool else torch.empty(1, dtype=torch.int32).pin_memory()
        host.copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(flag.device))
        self._range_pending.append((host, ev))

    def check_range(self, wait=False, _stacklevel=3):
        """Look at the range flags of earlier forwards ("async" guard).  wait=False: only copies that have already landed (never stalls);
        wait=True: wait for all of them.  -> True if an overflow of the fp16-split path was seen (now or earlier); from then on this
        module runs on the full-range variant 5.  The forward that overflowed returned non-finite occupancies."""
        keep = []
        for host, ev in self._range_pending:
            if wait:
                ev.synchronize()
            if wait or ev.query():
                if int(host[0]) and not self._full_range:
                    warnings.warn(type(self).__name__ + ": an activation left the fp16 range of the default matrix path (variant 6) -- that forward "
                                  "returned non-finite values; this module runs on the full-range variant 5 from now on "
                                  "(range_guard='sync' repeats the forward itself at the price of a read-back per call)", RuntimeWarning, stacklevel=_stacklevel)
                    self._full_range = True
                self._range_pool.append(host)
            else:
                keep.append((host, ev))
        self._range_pending = keep
        return self._full_range

    def clear_range_flag(self, device=None):
        """Zero the flag; with `device`, create it there first if this module has not run a guarded forward on it yet (a rank whose
        query shard is empty never runs one, yet has to bring a flag to the step's all-reduce)."""
        if device is not None and (self._range_flag is None or self._range_flag.device != torch.device(device)):
            self._range_flag = torch.zeros(1, dtype=torch.int32, device=device)
        elif self._range_flag is not None:
            self._range_flag.zero_()
