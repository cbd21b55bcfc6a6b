"""The range guard of the 16-bit matrix paths (networks/range_guard.py) end to end.

Variant 6 (the default) and variant 7 feed the large GEMMs, the long-sequence attention and the fused local transformers fp16 operands,
valid for |activation| < 65504; the reference is plain fp32.  The kernels OR a device flag when an output comes out non-finite
(mcr_nonfinite_flag, the flag arguments of the network entry points) and the Python layer repeats the forward, or the whole decision,
on the full-range variant 5.  Tested here: the flag kernel itself against numpy; the flag of both networks under a user's stream
capture and inside GraphedNbvStep; the fallback of every decision entry point when SconeVis overflows, against the fp64 oracle;
variant 7's fallback; and no false alarm with activations right below the limit.

Overflow recipe (the one of test_networks_gpu.py): one layer's weight and bias scaled by 2^16 or 2^17.  The overflow is numeric (inf /
NaN in fp16 operands), never a memory fault."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import weights  # noqa: E402
from oracle import nets  # noqa: E402
from oracle import nbv as onbv  # noqa: E402
from test_variant7_gpu import AMPLIFICATION, OCC_TOL_BY_WEIGHTS, VIS_TOL  # noqa: E402  (variant 7's stated bounds)

pytestmark = pytest.mark.gpu
TOL = 1e-4
HALF_MAX = 65504.0
EDGE = 0.75 * HALF_MAX          # the largest activation entering a product in the no-false-alarm tests: in [2^14, 65504)

# name -> (network, weight seed, layers scaled, factor)
SITES = {
    "vis_encoder": ("SconeVis", 1, ["encoders.1.ff.linear1"], 2.0 ** 17),
    "occ_head": ("SconeOcc", 2, ["linear1", "x_embedding.linear2"], 2.0 ** 16),
    "occ_global": ("SconeOcc", 2, ["global_transformer.encoders.0.ff.linear1"], 2.0 ** 17),
    "occ_local_ff": ("SconeOcc", 2, ["local_transformers.1.encoders.0.ff.linear1"], 2.0 ** 16),
}


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.fixture(autouse=True)
def _default_variant_6():
    from macarons_amd import _lib
    if _lib.lib().mcr_get_local_pct_variant() != 6:
        pytest.skip("the range guard belongs to variant 6 (suite running on another variant)")


def _state(net, seed):
    from macarons_amd import networks
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(networks, net)()
    return weights.make_state_dict(weights.shapes_of(m), seed)


def _load(net, sd, dev):
    from macarons_amd import networks
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(networks, net)()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def _scaled(sd, layers, factor):
    out = {k: v.copy() for k, v in sd.items()}
    for layer in layers:
        for k in (layer + ".weight", layer + ".bias"):
            out[k] = (out[k] * np.float32(factor)).astype(np.float32)
    return out


def _site(name, scaled=True):
    """-> (network class name, state dict: the site's layers scaled when `scaled`)."""
    net, seed, layers, factor = SITES[name]
    sd = _state(net, seed)
    return net, (_scaled(sd, layers, factor) if scaled else sd)


def _inputs(net, name):
    """Host inputs of a stand-alone forward: SconeVis 700 points (>= 512: the planes encoders); SconeOcc the scone_occ.npz case with
    Lg = 2048 for the global transformer, m1024_q300 otherwise."""
    if net == "SconeVis":
        rng = np.random.default_rng(3)
        pts = np.concatenate([rng.uniform(-.5, .5, (1, 700, 3)), rng.uniform(.1, 1., (1, 700, 1))], -1).astype(np.float32)
        return {"pts": pts, "vh": (rng.standard_normal((1, 700, 64)) * 0.3).astype(np.float32)}
    g = golden("scone_occ")
    tag = "m4096_q512" if name == "occ_global" else "m1024_q300"
    return {"pc": g[f"{tag}_pc"], "x": g[f"{tag}_x"], "vh": g[f"{tag}_vh"], "perms": [g[f"{tag}_perm{i}"].astype(np.int64) for i in range(3)]}


def _on(inp, dev):
    """The inputs as device tensors (uploaded before any capture: a graph cannot hold a copy from pageable host memory)."""
    return {k: ([T(p, dev) for p in v] if k == "perms" else T(v, dev)) for k, v in inp.items()}


def _forward(m, d):
    if "pts" in d:
        return m(d["pts"], view_harmonics=d["vh"])
    return m(d["pc"], d["x"], d["vh"], perms=d["perms"])


def _oracle(sd, inp):
    if "pts" in inp:
        return nets.scone_vis_forward(sd, inp["pts"], inp["vh"], np.float64)
    return nets.scone_occ_forward(sd, inp["pc"], inp["x"], inp["vh"], inp["perms"], np.float64)


# ---- 1. the flag kernel -------------------------------------------------------------------------------------------------------
FLT_MAX = np.finfo(np.float32).max
CLEAN_SPECIALS = np.array([FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1e-40, -1e-40, 0.0, -0.0], np.float32)     # +-max, +-subnormals, +-0
BAD_BITS = {"+inf": 0x7F800000, "-inf": 0xFF800000, "quiet NaN": 0x7FC00000, "NaN payload": 0xFFC0BEEF, "signalling NaN": 0x7F800001}
PASS = 1024 * 256               # launch cap: element PASS is the first one of the second grid-stride pass


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, PASS - 1, PASS, PASS + 1, 3 * PASS + 17, 50_000_000])
def test_nonfinite_flag_kernel_against_numpy(dev, n):
    """ops.nonfinite_flag_ (mcr_nonfinite_flag) against numpy's isfinite: finite data with +-FLT_MAX, +-subnormals and +-0 leaves the
    flag as it was (0 stays 0, 1 stays 1: the kernel ORs, never clears); one inf / NaN (payload and signalling NaNs included) at the
    first element, the last one, the first of the second grid-stride pass and a random one sets it."""
    from macarons_amd import ops
    rng = np.random.default_rng(n % 9973)
    xh = rng.standard_normal(n, dtype=np.float32)
    bits = xh.view(np.uint32)
    spots = [0, n - 1, 63, 64, 255, 256, PASS - 1, PASS] + list(rng.integers(0, n, 8))
    spots = sorted({s for s in spots if s < n})
    x = T(xh, dev)

    def flag_after(start):
        f = torch.full((1,), start, dtype=torch.int32, device=dev)
        ops.nonfinite_flag_(x, f)
        return int(f)

    for shift in range(len(CLEAN_SPECIALS) if n < 64 else 1):         # (tiny sizes: every special value at every position)
        for j, s in enumerate(spots):
            xh[s] = CLEAN_SPECIALS[(j + shift) % len(CLEAN_SPECIALS)]
        x.copy_(T(xh, dev))
        assert np.isfinite(xh).all()
        assert flag_after(0) == 0 and flag_after(1) == 1, (n, shift)
    where = sorted({0, n - 1, int(rng.integers(0, n))} | ({PASS} if n > PASS else set()))
    for name, b in BAD_BITS.items():
        for i in where:
            old = bits[i]
            bits[i] = b
            x[i:i + 1].copy_(torch.from_numpy(xh[i:i + 1].copy()))     # (a byte copy: the NaN payload arrives as it is)
            assert not np.isfinite(xh).all()
            assert flag_after(0) == 1 and flag_after(1) == 1, (n, name, i)
            bits[i] = old
            x[i:i + 1].copy_(torch.from_numpy(xh[i:i + 1].copy()))
    assert flag_after(0) == 0


# ---- 2. stand-alone forwards under a user's capture ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vis_encoder", "occ_head", "occ_global"])
def test_captured_forward_leaves_the_overflow_in_the_flag(dev, name):
    """Under stream capture the default guard ("sync") and "async" act as "defer": the flag kernel is part of the graph, no read-back
    and no host copy is.  An overflowing model's replay raises its flag (range_flag() reads 1 after the replay; the graph returns what
    the 16-bit path computed, for the caller to repeat); an in-range model captured beside it replays the eager bits and leaves its own
    flag at 0."""
    net, sd_ok = _site(name, scaled=False)
    _, sd_bad = _site(name)
    ok, bad = _load(net, sd_ok, dev), _load(net, sd_bad, dev)
    assert ok.range_guard == "sync" and bad.range_guard == "sync"
    d = _on(_inputs(net, name), dev)
    with torch.no_grad():
        y_e = _forward(ok, d)
        yb_e = _forward(bad, d)                           # eager "sync": already repeated on variant 5
        assert torch.isfinite(yb_e).all() and int(bad.range_flag()) == 1
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _forward(ok, d), _forward(bad, d)      # warm-up on the capture stream
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        for guard in ("sync", "async"):
            ok.range_guard = bad.range_guard = guard
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                y_g, yb_g = _forward(ok, d), _forward(bad, d)
            assert len(ok._range_pending) == 0 and len(bad._range_pending) == 0, guard     # no host copy queued in the graph
            ok.clear_range_flag(); bad.clear_range_flag()
            graph.replay()
            torch.cuda.synchronize()
            assert int(bad.range_flag()) == 1, (name, guard)
            assert int(ok.range_flag()) == 0, (name, guard)
            assert torch.equal(y_g, y_e), (name, guard)
            assert not torch.isfinite(yb_g).all(), (name, guard)
            assert len(bad._range_pending) == 0 and bad._full_range is False and ok._full_range is False
            del graph


# ---- 3. GraphedNbvStep ---------------------------------------------------------------------------------------------------------
def _decision_models(dev, overflow=None):
    """The models of the NBV tests (seeds 2 / 1, occupancy bias + 0.5 so that untrained occupancies pass min_occ); overflow: "head"
    scales the SconeOcc head, "vis" the SconeVis encoders.  -> (occ, vis, sdo, sdv)."""
    sdo, sdv = _state("SconeOcc", 2), _state("SconeVis", 1)
    sdo["linear3.bias"] = sdo["linear3.bias"] + np.float32(0.5)
    if overflow == "head":
        sdo = _scaled(sdo, SITES["occ_head"][2], SITES["occ_head"][3])
    elif overflow == "vis":
        sdv = _scaled(sdv, SITES["vis_encoder"][2], SITES["vis_encoder"][3])
    return _load("SconeOcc", sdo, dev), _load("SconeVis", sdv, dev), sdo, sdv


def _grid_scene(dev):
    g = golden("e2e_grid_config1")
    from macarons_amd.nbv import ViewStateGrid
    args = (T(g["pc"], dev), T(g["X"], dev), T(g["X_view"], dev), T(g["X_cam"], dev), ViewStateGrid(dev))
    perms = [g[f"perm{i}"].astype(np.int64) for i in range(3)]
    return g, args, perms, g["samples"].astype(np.float32)


def _v(variant):
    from macarons_amd import ops
    return ops.variant(variant) if variant != 6 else contextlib.nullcontext()


@pytest.mark.parametrize("variant", [6, 7])
@pytest.mark.parametrize("where", ["head", "vis"])
def test_graphed_step_reports_an_overflow(dev, where, variant):
    """A decision captured from overflowing models (the SconeOcc head, or SconeVis's encoders) returns range_flag = 1 after the replay,
    in out["range_flag"] and in the flag word of the decision record: the caller sees that the decision must be repeated eagerly."""
    from macarons_amd.nbv import GraphedNbvStep
    occ, vis, _, _ = _decision_models(dev, where)
    g, (pc, X, X_view, X_cam, grid), perms, u = _grid_scene(dev)
    with _v(variant):
        step = GraphedNbvStep(occ, vis, pc, X, X_view, X_cam, grid)
    out = step(occ_perms=[torch.from_numpy(p) for p in perms], samples=T(u, dev))
    torch.cuda.synchronize()
    assert int(out["range_flag"]) == 1, (where, variant)
    assert float(out["record"][0]) == 1.0, (where, variant)
    assert occ.range_guard == "sync" and vis.range_guard == "sync"


@pytest.mark.parametrize("variant", [6, 7])
def test_graphed_step_clears_its_own_flag(dev, variant):
    """A step captured from in-range models zeroes its flag inside the graph: set to 1 by hand, it reads 0 again after the next replay."""
    from macarons_amd.nbv import GraphedNbvStep
    occ, vis, _, _ = _decision_models(dev)
    g, (pc, X, X_view, X_cam, grid), perms, u = _grid_scene(dev)
    with _v(variant):
        step = GraphedNbvStep(occ, vis, pc, X, X_view, X_cam, grid)
    kw = dict(occ_perms=[torch.from_numpy(p) for p in perms], samples=T(u, dev))
    out = step(**kw)
    torch.cuda.synchronize()
    assert int(out["range_flag"]) == 0 and float(out["record"][0]) == 0.0
    out["range_flag"].fill_(1)
    out = step(**kw)
    torch.cuda.synchronize()
    assert int(out["range_flag"]) == 0 and float(out["record"][0]) == 0.0
    assert torch.isfinite(out["gains"]).all() and int(out["nbv_idx"]) == int(g["nbv_idx"])


# ---- 4. eager decisions with SconeVis overflow ---------------------------------------------------------------------------------
def test_nbv_step_falls_back_when_scone_vis_overflows(dev):
    """nbv_step with SconeVis's encoders out of the fp16 range: the deferred check repeats the decision on variant 5 with the same
    draws -- the same occupancies, gains and camera as a run on variant 5 from the start, the gains within 1e-4 of the fp64 oracle."""
    from macarons_amd.nbv import nbv_step
    occ, vis, sdo, sdv = _decision_models(dev, "vis")
    g, a, perms, u = _grid_scene(dev)
    kw = dict(occ_perms=[torch.from_numpy(p) for p in perms], samples=T(u, dev))
    r0 = nbv_step(occ, vis, *a, range_guard=False, **kw)
    assert int(r0["range_flag"]) == 1 and "fallback_variant" not in r0          # the overflow is there ...
    r = nbv_step(occ, vis, *a, **kw)
    assert r.get("fallback_variant") == 5                                      # ... and the guarded step repeated the decision
    with _v(5):
        r5 = nbv_step(occ, vis, *a, **kw)
    assert "fallback_variant" not in r5
    assert torch.equal(r["occ"], r5["occ"]) and torch.equal(r["gains"], r5["gains"]) and int(r["nbv_idx"]) == int(r5["nbv_idx"])
    ref = onbv.nbv_step(sdo, sdv, g["pc"], g["X"], g["X_view"], g["X_cam"], perms, u, dtype=np.float64)
    err = rel_err(r["gains"].cpu().numpy(), ref["gains"])
    print(f"[range guard] nbv_step, SconeVis overflow, fallback gains vs fp64: {err:.2e}")
    assert int(r["n_unique"]) == ref["n_unique"] and err < TOL and int(r["nbv_idx"]) == ref["nbv_idx"]


def test_nbv_step_batch_falls_back_as_a_whole(dev):
    """nbv_step_batch (B = 3) with SconeVis overflowing: the whole batch is repeated on variant 5 and equals a batch run on variant 5
    from the start with the same draws."""
    from macarons_amd.nbv import nbv_step_batch, draw_batch
    occ, vis, _, _ = _decision_models(dev, "vis")
    g, (pc, X, X_view, X_cam, grid), _, _ = _grid_scene(dev)
    B = 3
    pcb = torch.cat([pc, pc * 0.9, pc.flip(1)]).contiguous()
    Xb = X.expand(B, -1, -1).contiguous()
    torch.manual_seed(7)
    perms, u = draw_batch(occ, B, pc.shape[1], 2048, dev)
    r = nbv_step_batch(occ, vis, pcb, Xb, X_view, X_cam, grid, occ_perms=perms, samples=u)
    assert r.get("fallback_variant") == 5
    with _v(5):
        r5 = nbv_step_batch(occ, vis, pcb, Xb, X_view, X_cam, grid, occ_perms=perms, samples=u)
    assert torch.isfinite(r["gains"]).all() and torch.isfinite(r["occ"]).all()
    assert torch.equal(r["occ"], r5["occ"]) and torch.equal(r["gains"], r5["gains"]) and torch.equal(r["nbv_idx"], r5["nbv_idx"])


def test_sharded_step_falls_back_on_the_all_reduced_flag(dev, monkeypatch):
    """The exchange path of nbv_step over a one-rank RCCL group (MCR_FORCE_DIST_PATH): the flag is all-reduced and the decision is
    repeated on variant 5, bit for bit the answer of the local guarded step."""
    import socket
    import torch.distributed as dist
    from macarons_amd.nbv import nbv_step
    occ, vis, _, _ = _decision_models(dev, "vis")
    g, a, perms, u = _grid_scene(dev)
    kw = dict(occ_perms=[torch.from_numpy(p) for p in perms], samples=T(u, dev))
    loc = nbv_step(occ, vis, *a, **kw)
    assert loc.get("fallback_variant") == 5
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    monkeypatch.setenv("MCR_FORCE_DIST_PATH", "1")
    try:
        r = nbv_step(occ, vis, *a, group=dist.group.WORLD, **kw)
        assert r.get("fallback_variant") == 5
        assert torch.equal(r["occ"], loc["occ"]) and torch.equal(r["gains"], loc["gains"])
        assert int(r["nbv_idx"]) == int(loc["nbv_idx"]) and torch.isfinite(r["gains"]).all()
    finally:
        dist.destroy_process_group()


def test_macarons_decision_falls_back_when_scone_vis_overflows(dev):
    """macarons_nbv_decision on the macarons_decision golden with SconeVis's encoders out of range: fallback_variant = 5 and, bit for
    bit, the decision of a model that runs on variant 5 from the start (the checks of the SconeOcc-overflow test)."""
    import ctypes
    from types import SimpleNamespace as NS
    from macarons_amd import _lib
    from macarons_amd.utility import macarons_utils as mu
    from test_macarons_regime_gpu import _decision_scenes, _models as _macarons
    g = golden("macarons_decision")
    H, W = int(g["hw"][0]), int(g["hw"][1])
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=16,
                prediction_neighborhood_size=3, n_view_state_cameras=98, sensor_range=40., min_occ_for_proxy_points=0.1, seq_len=2048,
                distance_factor_th=17., image_height=H, image_width=W, carving_tolerance=0.05)
    dmask = np.unpackbits(g["dmask"])[:2 * H * W].reshape(2, H, W).astype(bool)
    L = _lib.lib()

    def decide(force_variant):
        m = _macarons(dev)
        with torch.no_grad():
            lin = m.visibility.encoders[1].ff.linear1
            lin.weight.mul_(131072.); lin.bias.mul_(131072.)
        surface, proxy = _decision_scenes(g, dev)
        cam = mu.SceneCamera(mu.camera_record(g["Mview"][0], g["Mfull"][0], g["ndc"], g["eyes"][0], params.sensor_range).to(dev),
                             T(g["eyes"][0:1], dev), float(g["zfar"]))
        nrec = torch.stack([mu.camera_record(g["nMview_0"][k], g["nMfull_0"][k], g["ndc"], g["n_eyes"][0, k], params.sensor_range)
                            for k in range(5)]).to(dev)
        v0 = L.mcr_get_local_pct_variant()
        if force_variant:
            L.mcr_set_local_pct_variant(ctypes.c_int(force_variant))
        try:
            torch.manual_seed(5100)
            with torch.no_grad():
                r = mu.macarons_nbv_decision(params, m, proxy, surface, cam, T(g["depth"][0], dev), T(dmask[0], dev), nrec,
                                             T(g["n_eyes"][0], dev), dev, samples=T(g["u_0"], dev))
            assert m.occupancy.range_guard == "sync" and m.visibility.range_guard == "sync"      # restored
        finally:
            L.mcr_set_local_pct_variant(ctypes.c_int(v0))
        return r

    a, b = decide(None), decide(5)
    assert a.get("fallback_variant") == 5 and "fallback_variant" not in b
    assert torch.equal(a["occ_probs"], b["occ_probs"]) and torch.equal(a["gains"], b["gains"]) and int(a["next_idx"]) == int(b["next_idx"])
    assert torch.isfinite(a["gains"]).all()


# ---- 5. variant 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["occ_local_ff", "occ_head", "vis_encoder"])
def test_variant7_overflow_falls_back_to_the_full_fp32_contract(dev, name):
    """Under ops.variant(7) an overflow in the fused local transformer's FF, the SconeOcc head or SconeVis's encoders: the default guard
    returns finite values within 1e-4 of the fp64 oracle (the fallback gives variant 5's contract, not variant 7's looser bound);
    "defer" returns what variant 7 computed and leaves the flag at 1."""
    from macarons_amd import ops
    net, sd = _site(name)
    inp = _inputs(net, name)
    ref = _oracle(sd, inp)
    m = _load(net, sd, dev)
    with ops.variant(7), torch.no_grad():
        y = _forward(m, _on(inp, dev)).cpu().numpy()
    err = rel_err(y, ref)
    print(f"[range guard] variant 7, {name} overflow, fallback vs fp64: {err:.2e}")
    assert np.isfinite(y).all() and err < TOL
    assert int(m.range_flag()) == 1 and m._full_range is False
    dd = _load(net, sd, dev)
    dd.range_guard = "defer"
    dd.clear_range_flag(dev)
    with ops.variant(7), torch.no_grad():
        yd = _forward(dd, _on(inp, dev))
    assert int(dd.range_flag()) == 1 and not torch.isfinite(yd).all()


# ---- 6. no false alarm right below the limit ----------------------------------------------------------------------------------
def _recorded(monkeypatch, names):
    """Record the fp64 oracle's outputs of the named layers (`_lin` / `layernorm` calls) of the next oracle pass."""
    seen = {}
    lin, ln = nets._lin, nets.layernorm

    def lin_rec(sd, name, x):
        y = lin(sd, name, x)
        if name in names:
            seen[name] = y
        return y

    def ln_rec(sd, name, x, eps=1e-5):
        y = ln(sd, name, x, eps)
        if name in names:
            seen[name] = y
        return y
    monkeypatch.setattr(nets, "_lin", lin_rec)
    monkeypatch.setattr(nets, "layernorm", ln_rec)
    return seen


def _edge_model(monkeypatch, name):
    """(net, state dict, inputs, fp64 reference, largest activation entering the planes product): the scaled layer's output -- the
    input of the next planes GEMM -- peaks at EDGE (in [2^14, 65504)).  occ_head: linear1 (weight and bias) scaled, its GELU output
    enters linear2's product; vis_encoder: encoders.1.norm2 scaled, its output enters ff.linear1's product and ff.linear1's GELU output
    ff.linear2's (the weights' own planes stay in range: a LayerNorm has no matrix)."""
    net, sd = _site(name, scaled=False)
    inp = _inputs(net, name)
    if name == "occ_head":
        probe, layers = ["linear1"], ["linear1"]
        peak = lambda s: float(np.abs(nets.gelu(s["linear1"])).max())
    else:
        probe, layers = ["encoders.1.norm2", "encoders.1.ff.linear1"], ["encoders.1.norm2"]
        peak = lambda s: max(float(np.abs(s["encoders.1.norm2"]).max()), float(np.abs(nets.gelu(s["encoders.1.ff.linear1"])).max()))
    seen = _recorded(monkeypatch, probe)
    factor = 1.0
    for _ in range(3):                       # the peak is (close to) linear in the factor: a fixed point in a few passes
        sd_s = _scaled(sd, layers, factor)
        ref = _oracle(sd_s, inp)
        a = peak(seen)
        factor *= EDGE / a
    monkeypatch.undo()
    assert 2.0 ** 14 <= a < HALF_MAX, (name, a)
    return net, sd_s, inp, ref, a


@pytest.mark.parametrize("name", ["occ_head", "vis_encoder"])
def test_no_false_alarm_right_below_the_fp16_limit(dev, monkeypatch, name):
    """Activations entering a planes product up to 0.75 x 65504 (in [2^14, 65504)): the flag stays 0 on variants 6 and 7, variant 6
    stays within 1e-4 of fp64 and variant 7 within its stated bound (test_variant7_gpu.py).  The documented range is usable right up to
    its limit, not only as a rough bound."""
    from macarons_amd import ops
    net, sd, inp, ref, peak = _edge_model(monkeypatch, name)
    m = _load(net, sd, dev)
    m.range_guard = "defer"                  # (what the 16-bit path itself computed: no silent repeat on variant 5)
    errs = {}
    for v in (6, 7):
        m.clear_range_flag(dev)
        with _v(v), torch.no_grad():
            y = _forward(m, _on(inp, dev)).cpu().numpy()
        assert int(m.range_flag()) == 0, (name, v)
        assert np.isfinite(y).all()
        errs[v] = rel_err(y, ref)
    print(f"[range guard] {name}: peak activation {peak:.0f}; vs fp64: variant 6 {errs[6]:.2e}, variant 7 {errs[7]:.2e}")
    assert errs[6] < TOL
    bound = VIS_TOL if net == "SconeVis" else max(OCC_TOL_BY_WEIGHTS.values())
    assert errs[7] < bound and errs[7] < AMPLIFICATION * max(errs[6], 2.0 ** -22)
