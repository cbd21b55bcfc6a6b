"""The host layer of the network modules, on the CPU: the shared slot map and planes tail (packing.table_slots / planes_tail) against
the frozen per-class statements, the range guard's operations (networks/range_guard.py) on CPU tensors, and the one native-op probe
(utility/host.native_op)."""
import builtins
import contextlib
import io

import pytest
import torch

import _weight_tables_frozen as frozen


@pytest.fixture(scope="module")
def modules():
    """Default-architecture modules with random weights: PCTransformer at both feature widths, SconeOcc, SconeVis."""
    from macarons_amd.networks import SconeOcc, SconeVis
    from macarons_amd.networks.SconeOcc import PCTransformer
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        built = {"pct256": PCTransformer(seq_len=16, pts_embedding_dim=128, feature_dim=256),
                 "pct512": PCTransformer(seq_len=2048, pts_embedding_dim=128, feature_dim=512), "occ": SconeOcc(), "vis": SconeVis()}
    with torch.no_grad():
        for m in built.values():
            for p in m.parameters():                        # (LayerNorm's ones and zeros too: every tensor of a table is its own)
                p.copy_(torch.randn_like(p) * 0.3)
    assert all(m._is_default_arch() for m in built.values())
    return built


FROZEN = {"pct256": (frozen.pct_grad_slots, frozen.pct_planes), "pct512": (frozen.pct_grad_slots, frozen.pct_planes),
          "occ": (frozen.occ_grad_slots, frozen.occ_planes), "vis": (frozen.vis_grad_slots, frozen.vis_planes)}


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_grad_slots_are_the_frozen_slot_map(modules, name):
    m = modules[name]
    params, slots = m._grad_slots()
    want_params, want_slots = FROZEN[name][0](m)
    assert len(params) == len(want_params) and all(a is b for a, b in zip(params, want_params))
    assert slots == want_slots and isinstance(slots, tuple)
    assert len(params) == len(list(m.parameters())) > 30
    table = m.weight_table()
    for p, (k, rows) in zip(params, slots):                 # ... and a slot is where the parameter's values sit in the table
        entry = table[k] if rows is None else table[k][rows[0]:rows[1]]
        assert torch.equal(entry, p.detach())


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_weight_table_with_planes_is_the_frozen_table(modules, name):
    m = modules[name]
    got, want = m.weight_table_with_planes(), FROZEN[name][1](m)
    n = len(m.weight_table())
    assert isinstance(got, list) and len(got) == len(want) == n + 4 * len((m.global_transformer if name == "occ" else m).encoders) + \
        (5 if name == "vis" else 3)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (name, k)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got[:n], m.weight_table()))       # the table itself: the live tensors


@pytest.mark.parametrize("name", ["pct256", "occ", "vis"])
def test_a_parameter_outside_the_weight_table_is_refused(name):
    from macarons_amd.networks import SconeOcc, SconeVis
    from macarons_amd.networks.SconeOcc import PCTransformer
    with contextlib.redirect_stdout(io.StringIO()):
        m = {"pct256": lambda: PCTransformer(seq_len=16, pts_embedding_dim=128, feature_dim=256), "occ": SconeOcc, "vis": SconeVis}[name]()
    m.extra = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(NotImplementedError) as new:
        m._grad_slots()
    with pytest.raises(NotImplementedError) as old:
        FROZEN[name][0](m)
    assert str(new.value) == str(old.value) and "parameters outside the weight table: ['extra']" in str(new.value)


# ---- the range guard's operations ----------------------------------------------------------------------------------------------------
def _guarded_module():
    from macarons_amd.networks.range_guard import RangeGuard

    class Net(RangeGuard, torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 2)
    return Net()


def test_guard_state_is_per_instance_plain_lists():
    a, b = _guarded_module(), _guarded_module()
    assert a.range_guard == "sync" and a.range_flag() is None and a._full_range is False
    assert type(a._range_pending) is list and type(a._range_pool) is list
    assert a._range_pending is not b._range_pending and a._range_pool is not b._range_pool
    assert a.check_range() is False and a.check_range(wait=True) is False


def test_arm_creates_zeroes_or_leaves_the_flag():
    m, cpu = _guarded_module(), torch.device("cpu")
    for guard in ("sync", "async", "defer"):                # missing: created, zero, whatever the mode
        m._range_flag = None
        f = m._arm_range(cpu, guard)
        assert f is m.range_flag() and f.dtype == torch.int32 and f.shape == (1,) and f.device == cpu and int(f) == 0
    for guard in ("sync", "async"):                         # there: the same tensor, zeroed
        f.fill_(1)
        assert m._arm_range(cpu, guard) is f and int(f) == 0
    f.fill_(1)                                              # deferred: whoever deferred owns the clearing
    assert m._arm_range(cpu, "defer") is f and int(f) == 1
    for guard in ("sync", "defer"):                         # on another device: a new one where the forward runs
        m._range_flag = other = torch.ones(1, dtype=torch.int32, device="meta")
        f = m._arm_range(cpu, guard)
        assert f is not other and f is m.range_flag() and f.device == cpu and int(f) == 0


def test_settle_repeats_on_variant_5_only_under_sync_with_the_flag_set():
    from macarons_amd import ops
    m = _guarded_module()
    calls = []

    def rerun():
        calls.append(ops.current_variant())
        return "full range"
    with ops.variant(6):
        flag = torch.ones(1, dtype=torch.int32)
        assert m._settle_range(flag, "defer", rerun) is None and calls == [] and int(flag) == 1       # deferred: not looked at
        assert m._settle_range(flag, "off", rerun) is None and calls == []
        assert m._settle_range(None, "sync", rerun) is None and calls == []                           # an unguarded forward
        assert m._settle_range(torch.zeros(1, dtype=torch.int32), "sync", rerun) is None and calls == []
        assert m._settle_range(flag, "sync", rerun) == "full range" and calls == [5]                  # once, with variant 5 in scope
        assert ops.current_variant() == 6 and int(flag) == 1
    assert m._range_pending == [] and m._full_range is False


def test_reenter_only_after_an_overflow_was_seen():
    from macarons_amd import ops
    m = _guarded_module()
    with ops.variant(6):
        assert m._range_reenter() is False
        m._full_range = True
        assert m._range_reenter() is True
    with ops.variant(5):
        assert m._range_reenter() is False                  # already on the full-range variant


def test_overflow_warning_names_the_caller_of_forward():
    """The "async" guard's RuntimeWarning, raised from the preamble, points where it pointed when forward called check_range itself: at
    the line that called forward (and at the caller of check_range's caller when a user calls check_range directly)."""
    from macarons_amd import ops

    class Landed:
        def query(self):
            return True

        def synchronize(self):
            pass
    m = _guarded_module()
    m.range_guard = "async"

    def forward():
        return m._range_reenter()

    def caller():
        return forward()
    for call, code in ((caller, caller.__code__), (lambda: m.check_range(), None)):
        m._full_range = False
        m._range_pending.append((torch.ones(1, dtype=torch.int32), Landed()))
        with ops.variant(6), pytest.warns(RuntimeWarning, match="left the fp16 range") as seen:
            assert call() is True
        assert len(seen) == 1 and seen[0].filename == __file__
        if code is not None:
            assert seen[0].lineno == code.co_firstlineno + 1
    assert m._range_pending == [] and len(m._range_pool) == 2


@pytest.mark.parametrize("raises", [False, True])
def test_range_scope_restores_both_modules(raises):
    occ, vis = _guarded_module(), _guarded_module()
    occ.range_guard, vis.range_guard = "async", "sync"
    vis._range_flag = own = torch.ones(1, dtype=torch.int32)
    occ._range_flag = flag = torch.ones(1, dtype=torch.int32)
    try:
        with occ.range_scope("defer", torch.device("cpu"), peer=vis) as scope:
            assert scope is occ and occ.range_guard == vis.range_guard == "defer"
            assert occ.range_flag() is flag and int(flag) == 0          # cleared on entry
            assert vis.range_flag() is flag                             # the peer reports into this module's flag
            flag.fill_(1)
            if raises:
                raise KeyError("inside the decision")
    except KeyError:
        assert raises
    assert (occ.range_guard, vis.range_guard) == ("async", "sync")
    assert vis.range_flag() is own and int(own) == 1                    # the peer's own flag is back, untouched
    assert occ.range_flag() is flag and int(flag) == 1                  # what the decision reported stays readable


def test_range_scope_flag_creation_follows_the_device_argument():
    occ, vis = _guarded_module(), _guarded_module()
    with occ.range_scope("off", None, peer=vis):                        # no device: nothing is created, the peer shares "nothing"
        assert occ.range_guard == vis.range_guard == "off" and occ.range_flag() is None and vis.range_flag() is None
    assert occ.range_guard == vis.range_guard == "sync" and occ.range_flag() is None
    with occ.range_scope("defer", "cpu", peer=vis):                     # a device: the flag exists before the first forward
        assert occ.range_flag() is not None and int(occ.range_flag()) == 0 and vis.range_flag() is occ.range_flag()
    assert vis.range_flag() is None and occ.range_flag() is not None


@pytest.mark.parametrize("peer", [None, torch.nn.Linear(2, 2), object()])
def test_range_scope_leaves_a_peer_without_a_guard_untouched(peer):
    occ = _guarded_module()
    before = dict(vars(peer)) if hasattr(peer, "__dict__") else None
    with occ.range_scope("defer", "cpu", peer=peer):
        assert occ.range_guard == "defer"
        assert not hasattr(peer, "range_guard") and not hasattr(peer, "_range_flag")
    assert occ.range_guard == "sync" and not hasattr(peer, "range_guard") and not hasattr(peer, "_range_flag")
    assert before is None or dict(vars(peer)) == before


def test_the_networks_take_their_guard_from_the_one_class():
    from macarons_amd.networks import SconeOcc, SconeVis, packing
    from macarons_amd.networks.range_guard import RangeGuard
    assert issubclass(SconeOcc, RangeGuard) and issubclass(SconeVis, RangeGuard) and not hasattr(packing, "RangeGuard")
    with contextlib.redirect_stdout(io.StringIO()):
        vis = SconeVis()
    assert vis.range_guard == "sync" and vis._range_pending == [] and "_range_pending" in vars(vis)


# ---- the native-op probe --------------------------------------------------------------------------------------------------------------
def _spy_on_extension_imports(monkeypatch):
    seen, real = [], builtins.__import__

    def spy(name, globals=None, locals=None, fromlist=(), level=0):
        if "torch_ops" in name or "torch_ops" in (fromlist or ()):
            seen.append(name)
        return real(name, globals, locals, fromlist, level)
    monkeypatch.setattr(builtins, "__import__", spy)
    return seen


def test_probe_opt_out_answers_without_loading_the_extension(monkeypatch):
    from macarons_amd.utility import host
    monkeypatch.setattr(host, "_NATIVE_OPS", {})
    seen = _spy_on_extension_imports(monkeypatch)
    monkeypatch.setenv("MCR_PROBE_TEST", "0")
    assert host.native_op("ragged_tables", "MCR_PROBE_TEST") is False and seen == []
    monkeypatch.delenv("MCR_PROBE_TEST")
    host.native_op("h2d", "MCR_PROBE_TEST")                             # not opted out: the extension is asked (built or not)
    assert len(seen) == 1
    assert host.native_op("no_such_operator", "MCR_PROBE_TEST") is False      # loaded or missing, an operator it lacks is not there


def test_probe_is_memoised_per_operator(monkeypatch):
    from macarons_amd.utility import host
    monkeypatch.setattr(host, "_NATIVE_OPS", {})
    seen = _spy_on_extension_imports(monkeypatch)
    first = host.native_op("h2d", "MCR_PROBE_TEST")
    monkeypatch.setenv("MCR_PROBE_TEST", "0")
    assert host.native_op("h2d", "MCR_PROBE_TEST") is first and len(seen) == 1        # asked once: the later opt-out is not seen ...
    assert host.native_op("field_jobs", "MCR_PROBE_TEST") is False and len(seen) == 1   # ... but another operator asks for itself
    assert host._NATIVE_OPS == {"h2d": first, "field_jobs": False}


def test_the_four_probes_name_their_operator_and_variable(monkeypatch):
    import importlib
    from macarons_amd import ops
    from macarons_amd.utility import host, macarons_utils as mu, scone_utils as su
    so = importlib.import_module("macarons_amd.networks.SconeOcc")
    for probe, op, env in ((ops._native_h2d, "h2d", "MCR_NATIVE_H2D"), (su._native_bins, "view_space_bins", "MCR_NATIVE_BINS"),
                           (mu._native_field_jobs, "field_jobs", "MCR_NATIVE_FIELD_JOBS"),
                           (so._native_ragged_tables, "ragged_tables", "MCR_NATIVE_RAGGED_TABLES")):
        monkeypatch.setattr(host, "_NATIVE_OPS", {})
        monkeypatch.setenv(env, "0")
        assert probe() is False and host._NATIVE_OPS == {op: False}
