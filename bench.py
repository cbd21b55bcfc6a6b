#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X-native SCONE coverage-gain hot path.

Metric (BASELINE.json): candidate-camera coverage-gain evals/sec (100k pts, 200 cams); NBV step p50 latency.

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run measures (A) alone and prints its line.  `--dump-outputs DIR` writes what the last timed step of (A) returned, as
DIR/gains.npy (float32 [1, C], the gains of rank 0's cameras) and DIR/record.npy (float32 [1, 2]: the decision, max gain and arg-max
camera); the inputs are seeded, so two builds given the same arguments can be compared output for output.

What a `--full` run reports, at any N:
  (A)  `value` — the contract line: scorer throughput, WEAK scaling.  A "step" = one pass of the scorer
       (SconeVis.compute_coverage_gain semantics) over one synthetic cloud of 100 000 points x 200 candidate cameras per GPU,
       inputs resident in HBM, followed by the arg-max decision record (N > 1: the all-gather of every rank's record).
       One (cloud, camera) pair scored = one eval.
  (A') `scorer_strong` — BASELINE config 4: the same cloud x 512 cameras IN TOTAL, block-partitioned over the ranks
       (512 / N per rank), same decision exchange: strong scaling of the scorer.
  (B)  `nbv_step` — p50 latency of the full SCONE NBV decision (macarons_amd.nbv.nbv_step: view state + harmonics on Q = 100k
       proxy points -> SconeOcc vs M = 10 240 surface points -> sample 2048 -> SconeVis -> gains over C = 200 cameras -> arg-max),
       device-synchronised per iteration, random-init weights; with N GPUs the queries and the cameras are sharded over the ranks
       (strong scaling of one decision) and the occupancies / records travel over RCCL.
  `ranks_seen` — how many distinct ranks an RCCL all-gather of the rank ids returned (proof the collective path ran at N).

Rank 0 prints ONE JSON line (contract in the task statement); under --full with extra objects:
  roofline              dominant kernel of (A), sh_gain_kernel, timed ALONE with HIP events (K launches of the first stage only):
                        algorithmic flop per launch / its mean duration vs the fp32 vector peak; the step-level figure
                        (gain + reduce + decision record per step) sits beside it as `step_*`
  roofline_nbv_dominant dominant kernel of (B), the fused local transformer: executed matrix-pipe rate vs the fp16 dense peak
                        (`frac`) and the algorithmic fp32-equivalent rate vs the same pipe (`frac_algorithmic`)
  cpu_baseline          the plain-C port of the reference scorer (oracle/csrc, pinned to the reference's goldens) on the host cores
  cpu_baseline_nbv      the numpy restatement of the NBV step (oracle/nbv.py, pinned likewise) on a bounded sample of the queries
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_PAIR = 370.0          # algorithmic flop per (point, camera) pair IN THE REFERENCE'S FORMULATION (trig + lpmv recurrences)
# flop the kernel EXECUTES per pair: the camera loop of sh_gain_kernel<true> is 94 vector instructions -- 77 fused multiply-adds
# (2 flop), 14 single-flop ones (mul / add / max), 3 transcendentals (1) -- counted on the compiled ISA (the loop between the
# scalar camera load and its back branch; 30.7 M wave-instructions per launch in profiles/r05_scorer_pmc.json = 94 x 100k x 200 / 64
# + the per-tile prologue).  The trig-free complex-Horner form needs fewer operations than the formulation SURVEY 8(d) counts, so a
# roofline fraction on the 370 can exceed 1; the one on the 171 cannot (it is <= the vector pipe's issue-slot utilisation).
FLOP_PER_PAIR_EXECUTED = 171.0
BYTES_PER_POINT = 268.0        # 12 B xyz + 256 B coefficients, read once per cloud
PEAK_FP32_TFLOPS = 157.3       # MI355X fp32 vector (= fp32 MFMA) peak, MI355X_MICROARCH.md
PEAK_F16_TFLOPS = 2500.0       # dense fp16 / bf16 MFMA peak
PEAK_HBM_GBS = 8000.0


def make_inputs(N, C, seed, device, cam_offset=0, n_cam_total=None):
    """Synthetic workload of SURVEY §8d: uniform points in [-0.5,0.5]^3 + occupancy U(0.1,1), coefficients
    N(0,0.5^2), cameras on the radius-1.5 sphere."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pts = torch.cat([torch.rand(1, N, 3, generator=g) - 0.5, 0.1 + 0.9 * torch.rand(1, N, 1, generator=g)], -1)
    harm = torch.randn(1, N, 64, generator=g) * 0.5
    n_tot = n_cam_total or C
    cams = torch.randn(1, n_tot, 3, generator=g)
    cams = 1.5 * cams / cams.norm(dim=-1, keepdim=True)
    cams = cams[:, cam_offset:cam_offset + C].contiguous()
    return pts.to(device), harm.to(device), cams.to(device)


def cpu_baseline(pts, harm, cams):
    """Time the C port of the reference scorer on the host cores for a bounded sample of the workload
    (the same cloud, the first cams.shape[1] cameras)."""
    from oracle import cport
    p, h, c = pts.cpu().numpy(), harm.cpu().numpy(), cams.cpu().numpy()
    N, C_sample = p.shape[1], c.shape[1]
    cport.coverage_gain(p[:, :256], h[:, :256], c)        # warm-up / build
    # every host core, one thread per physical core (SMT siblings share the FP units: 256 threads measured SLOWER than 128 on
    # the 2 x 64-core host) and the CPUs the container's quota lets the process burn (16 on the pool's boxes: more threads than
    # that only get the process throttled); ~5 s of CPU work each, the best one is the baseline, all are reported
    from macarons_amd.utility.host import effective_cpus
    runs = []
    for nt_req in sorted({os.cpu_count() or 1, max(1, (os.cpu_count() or 2) // 2), effective_cpus()}, reverse=True):
        cport.set_threads(nt_req)
        reps, t0 = 0, time.perf_counter()
        while True:
            g, nthreads = cport.coverage_gain(p, h, c)
            reps += 1
            dt = time.perf_counter() - t0
            if dt > 5.0 or reps >= 50:
                break
        runs.append({"threads": int(nthreads), "evals_per_s": reps * C_sample / dt, "passes": reps, "wall_s": dt})
    best = max(runs, key=lambda r_: r_["evals_per_s"])
    reps, dt, nthreads = best["passes"], best["wall_s"], best["threads"]
    return {"value": best["evals_per_s"], "unit": "evals/s", "cores": int(nthreads), "thread_sweep": runs, "kind": "port",
            "sample": f"C port (oracle/csrc/scorer_port.c, OpenMP) of the reference scorer on the same cloud: "
                      f"N={N} points x {C_sample} cameras x {reps} passes, {dt:.2f} s wall; "
                      f"`cores` = omp_get_num_threads() inside the parallel region of the fastest of the thread counts tried; "
                      f"host has {os.cpu_count()} cores, the container's quota is {effective_cpus()} CPUs"}, g


def cpu_baseline_nbv(C):
    """The numpy restatement of one NBV decision (oracle/nbv.py) on a bounded sample: the same surface cloud (M = 10 240), the
    same C cameras, Q_s = 6000 of the 100 000 proxy points.  The occupancy pass is linear in Q (every query is independent), so
    the full-size figure is extrapolated from two sample sizes and labelled as such."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import io, contextlib
    import weights
    from oracle import nbv as onbv
    from macarons_amd.networks import SconeVis, SconeOcc
    with contextlib.redirect_stdout(io.StringIO()):
        occ, vis = SconeOcc(), SconeVis()
    sdo = weights.make_state_dict(weights.shapes_of(occ), 2)
    sdv = weights.make_state_dict(weights.shapes_of(vis), 1)
    sdo["linear3.bias"] = sdo["linear3.bias"] + np.float32(0.5)
    rng = np.random.default_rng(4321)
    M = 10_240
    d = rng.standard_normal((M, 3))
    pc = (d / np.linalg.norm(d, axis=1, keepdims=True) * [0.35, 0.25, 0.3]).astype(np.float32)[None]
    cams = rng.standard_normal((C, 3)).astype(np.float32)
    cams = (1.5 * cams / np.linalg.norm(cams, axis=1, keepdims=True)).astype(np.float32)
    u = rng.uniform(0, 1, 2048).astype(np.float32)
    torch.manual_seed(11)
    perms = [p.numpy() for p in occ.draw_perms(M)]
    times = {}
    # numpy's BLAS / OpenMP pools: ask for every host core and report what the pools say they run with
    blas_threads = None
    try:
        from threadpoolctl import threadpool_limits, threadpool_info
        from macarons_amd.utility.host import effective_cpus
        threadpool_limits(limits=effective_cpus())
        blas_threads = {i.get("internal_api", i.get("user_api", "?")): int(i.get("num_threads", 0)) for i in threadpool_info()}
    except Exception:
        pass
    for Q in (1500, 6000):
        X = rng.uniform(-.5, .5, (1, Q, 3)).astype(np.float32)
        t0 = time.perf_counter()
        onbv.nbv_step(sdo, sdv, pc, X, cams[:3], cams, perms, u)
        times[Q] = time.perf_counter() - t0
    per_q = (times[6000] - times[1500]) / 4500.0
    fixed = max(times[1500] - 1500 * per_q, 0.0)
    full = fixed + 100_000 * per_q
    cores = max(blas_threads.values()) if blas_threads else int(torch.get_num_threads())
    return {"value": C / times[6000], "unit": "evals/s", "cores": int(cores), "thread_pools": blas_threads, "kind": "port",
            "sample": f"numpy restatement of the NBV step (oracle/nbv.py; `cores` = the largest thread pool numpy's BLAS / OpenMP "
                      f"libraries report after asking for the {effective_cpus()} CPUs of the container's quota; the host has {os.cpu_count()} cores): M=10240 surface points, C={C} cameras, Q_s=6000 of the 100000 proxy points: "
                      f"{times[6000]:.2f} s (Q_s=1500: {times[1500]:.2f} s)",
            "sample_step_s": times[6000], "per_query_ms": per_q * 1e3, "fixed_s": fixed,
            "extrapolated_full_step_s": full, "extrapolated_full_evals_per_s": C / full,
            "note": "extrapolation = fixed + 100000 x per-query cost from the two sample sizes; not a measurement of the full step"}


def measure_scorer_traffic(N, C, timeout_s=90):
    """HBM read bytes of ONE sh_gain_kernel launch at the headline size, measured in THIS run when rocprofv3 is on the box: a separate
    process runs the scorer under `rocprofv3 --pmc FETCH_SIZE` (counters only, no tracing, as MI355X_MICROARCH.md prescribes), the
    per-dispatch mean of the kernel is read from the counter csv and corrected x2 (gfx950: FETCH_SIZE counts 64-byte units of 128-byte
    requests, KiB as reported).  -> (bytes or None, how it was obtained)."""
    import glob, shutil, subprocess, tempfile, csv
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not on this box"
    out = tempfile.mkdtemp(prefix="mcr_pmc_")
    code = ("import sys; sys.path.insert(0, %r); import torch, bench; from macarons_amd import ops; d = torch.device('cuda:0'); "
            "p, h, c = bench.make_inputs(%d, %d, 1234, d); [ops.sh_coverage_gain(p, h, c) for _ in range(40)]; torch.cuda.synchronize()" % (ROOT, N, C))
    try:
        env = dict(os.environ, TMPDIR="/tmp")
        for k_ in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k_, None)
        # its own session: on a time-out the WHOLE tree (rocprofv3 -> python) is killed, nothing is left holding the GPU
        pr = subprocess.Popen([exe, "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", out, "-o", "p", "--", sys.executable, "-c", code],
                              cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, stdin=subprocess.DEVNULL,
                              start_new_session=True)
        try:
            pr.wait(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            import signal
            os.killpg(pr.pid, signal.SIGKILL)
            pr.wait()
            return None, f"in-run PMC pass exceeded {timeout_s} s"
        vals = []
        for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "sh_gain_kernel" in r.get("Kernel_Name", "") and r.get("Counter_Name") == "FETCH_SIZE":
                    vals.append(float(r["Counter_Value"]))
        if len(vals) < 8:
            return None, f"rocprofv3 --pmc FETCH_SIZE returned {len(vals)} dispatches of the kernel"
        vals = vals[len(vals) // 4:]                          # (the first launches warm the caches / page tables)
        return float(np.mean(vals)) * 1024.0 * 2.0, f"measured in this run: rocprofv3 --pmc FETCH_SIZE (own process, counters only), mean of {len(vals)} launches, x2 per MI355X_MICROARCH.md"
    except Exception as e:
        return None, f"in-run PMC pass failed: {repr(e)[:120]}"
    finally:
        shutil.rmtree(out, ignore_errors=True)


def pmc_profile(name):
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return json.load(f)
    except Exception:
        return None


def build_models(dev):
    from macarons_amd.networks import SconeVis, SconeOcc
    import io, contextlib
    torch.manual_seed(7)                                   # identical random-init weights on every rank
    with contextlib.redirect_stdout(io.StringIO()):
        occ, vis = SconeOcc(), SconeVis()
    with torch.no_grad():
        occ.linear3.bias += 0.5                            # untrained occupancies must pass min_occ
    occ, vis = occ.to(dev).eval(), vis.to(dev).eval()
    occ.freeze_weight_caches(); vis.freeze_weight_caches()    # inference: the weights are loaded once (no per-call fingerprint walk, ~70 us)
    return occ, vis


def measure_nbv_step(dev, rank, world, args):
    """(B) p50 latency of one NBV decision at Q=100k / M=10240 / C=cams, queries and cameras sharded over `world` GPUs."""
    from macarons_amd.nbv import nbv_step, ViewStateGrid
    occ, vis = build_models(dev)
    g = torch.Generator(device="cpu").manual_seed(4321)
    Q, M, C = 100_000, 10_240, args.cams
    d = torch.randn(M, 3, generator=g)
    pc = (d / d.norm(dim=1, keepdim=True) * torch.tensor([0.35, 0.25, 0.3]) + 0.002 * torch.randn(M, 3, generator=g))[None].to(dev)
    X = (torch.rand(1, Q, 3, generator=g) - 0.5).to(dev)
    cams = torch.randn(C, 3, generator=g)
    cams = (1.5 * cams / cams.norm(dim=1, keepdim=True)).to(dev)
    X_view = cams[:3].contiguous()
    u = torch.rand(2048, generator=g).to(dev)
    grid = ViewStateGrid(dev)
    torch.manual_seed(11)
    perms = [p.to(dev) for p in occ.draw_perms(M)]       # the three randperm draws of SconeOcc.forward, pinned and resident
    group = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None     # shards Q and C over the ranks
    n_warm = 10
    times = []
    for it in range(n_warm + args.nbv_iters):
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        t0 = time.perf_counter()
        r = nbv_step(occ, vis, pc, X, X_view, cams, grid, occ_perms=perms, samples=u, group=group)
        int(r["host"]["nbv_idx"][0]) if "host" in r else int(r["nbv_idx"])     # the decision reaches the host (with the range flag: one read-back)
        torch.cuda.synchronize()
        dt = max_over_ranks(time.perf_counter() - t0, dev, torch.distributed if world > 1 else None)
        if it >= n_warm:
            times.append(dt)
    p50 = float(np.median(times))
    graph = None
    if world == 1:
        # the same decision replayed as ONE hipGraph (nbv.GraphedNbvStep): removes the launch gaps between its ~70 kernels
        from macarons_amd.nbv import GraphedNbvStep
        try:
            gs = GraphedNbvStep(occ, vis, pc, X, X_view, cams, grid)
            gt = []
            for it in range(n_warm + args.nbv_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rg = gs(occ_perms=perms, samples=u)
                int(rg["nbv_idx"])
                torch.cuda.synchronize()
                if it >= n_warm:
                    gt.append(time.perf_counter() - t0)
            graph = {"p50_ms": float(np.median(gt)) * 1e3, "same_decision_as_eager": int(rg["nbv_idx"]) == int(r["nbv_idx"]),
                     "same_gains_as_eager": bool(torch.equal(rg["gains"], r["gains"]))}
        except Exception as e:                               # capture is an optimisation: report, never fail the bench on it
            graph = {"error": repr(e)[:200]}
    # what ONE rank of an 8-GPU job computes for this decision, measured here (N = 1 only): its 1/8 of the queries, then the part every
    # rank repeats (sampling, SconeVis, decision) and its 1/8 of the cameras, the two exchanges replaced by local stand-ins of the same
    # size -- the per-rank critical path apart from collective latency, so that the projected strong scaling is a measurement
    shard8 = None
    if world == 1:
        from macarons_amd import ops
        from macarons_amd.nbv import nbv_step_one_rank_of, GraphedNbvStep

        def one_rank(variant, n=20):
            te = []
            with ops.variant(variant):
                for it in range(5 + n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    re_ = nbv_step_one_rank_of(8, occ, vis, pc, X, X_view, cams, grid, perms, u)
                    int(re_["nbv_idx"])
                    torch.cuda.synchronize()
                    if it >= 5:
                        te.append(time.perf_counter() - t0)
                eager = float(np.median(te))
                # the same share replayed as ONE hipGraph: the GPU-side critical path without the host's launch rate (a 1/8-size step is
                # ~60 short launches: eager it is bound by the host)
                try:
                    gs8 = GraphedNbvStep(occ, vis, pc, X, X_view, cams, grid, one_rank_of=8)
                    tg = []
                    for it in range(5 + n):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rg8 = gs8(occ_perms=perms, samples=u)
                        int(rg8["nbv_idx"])
                        torch.cuda.synchronize()
                        if it >= 5:
                            tg.append(time.perf_counter() - t0)
                    graph8 = float(np.median(tg))
                except Exception as e:
                    graph8 = None
                    sys.stderr.write(f"bench.py: one_rank_of_8 graph capture failed: {e!r}\n")
            return eager, graph8

        def part_ms(fn, n=20):                              # device time of one component, back to back (HIP events on the current stream)
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        p50_e, p50_g = one_rank(6)
        # replicated vs sharded: the components of a rank's share timed alone (variant 6).  Sharded = SconeOcc on Q/8 queries (its global
        # transformer -- replicated work -- runs on a side stream beside the local path) + the scorer on C/8 cameras; replicated = the part
        # every rank repeats on the full sampled set
        from macarons_amd.utility import scone_utils as su
        q8, c8 = Q // 8, C // 8
        Xs, vhs = X[:, :q8].contiguous(), torch.zeros(1, q8, 64, device=dev)
        prev_guard = (occ.range_guard, vis.range_guard)
        occ.range_guard = vis.range_guard = "off"
        try:
            with torch.no_grad():
                t_occ = part_ms(lambda: occ(pc, Xs, vhs, perms=perms))
                t_glob = part_ms(lambda: occ.global_transformer(pc[:, perms[0]].contiguous()))
                pp = torch.cat((X[0, :2048], torch.rand(2048, 1, device=dev)), 1)
                vs = su.compute_view_harmonics(su.compute_view_state(pp[None, :, :3].contiguous(), X_view, grid.n_elev, grid.n_azim),
                                               grid.base_harmonics, grid.h_polar, grid.h_azim, grid.n_elev, grid.n_azim)
                t_vis = part_ms(lambda: vis(pp[None], view_harmonics=vs))
                occ_full = torch.rand(Q, device=dev) * 0.8 + 0.15
                t_smp = part_ms(lambda: ops.sample_proxy(X[0].contiguous(), occ_full, None, u.reshape(-1), 0.1, padded=True))
                hm = torch.randn(1, 2048, 64, device=dev) * 0.3
                t_sc = part_ms(lambda: vis.compute_coverage_gain(pp[None], hm, cams[:c8].contiguous().view(1, -1, 3)))
        finally:
            occ.range_guard, vis.range_guard = prev_guard
        shard8 = {"world": 8, "rank": 0, "p50_ms": p50_e * 1e3, "p50_ms_hipgraph": None if p50_g is None else p50_g * 1e3,
                  "full_step_p50_ms": p50 * 1e3, "speedup_before_collective_latency": p50 / p50_e,
                  "speedup_hipgraph_before_collective_latency": None if p50_g is None else (graph["p50_ms"] * 1e-3 if graph and "p50_ms" in graph else p50) / p50_g,
                  "split_device_ms": {"sharded": {"scone_occ_on_Q_over_8": t_occ, "scorer_on_C_over_8": t_sc},
                                      "replicated": {"global_transformer_inside_scone_occ_side_stream": t_glob, "sampler": t_smp, "scone_vis_2048": t_vis},
                                      "note": "components timed alone, back to back (HIP events); the global transformer's time is INSIDE scone_occ's "
                                              "(side stream, beside the local path): replicated work that does not add to the path unless it "
                                              "outlasts the sharded local part"},
                  "note": "one rank's critical path of an 8-rank step emulated on one GPU (its query shard + the redundant sampling / "
                          "SconeVis / decision + its camera shard; exchanges = local copies of the same size): the 8-GPU step costs this "
                          "plus the latency of one occupancy all-gather (50 KB per rank) and one 8-byte record all-gather.  Eager, a 1/8-size "
                          "step is ~60 short launches and host-bound; p50_ms_hipgraph is the same share replayed as one hipGraph"}
        try:
            e7, g7 = one_rank(7, n=12)
            shard8["variant_7"] = {"p50_ms": e7 * 1e3, "p50_ms_hipgraph": None if g7 is None else g7 * 1e3}
        except Exception as e:
            shard8["variant_7"] = {"error": repr(e)[:200]}
    # the same step on the other numerics of the matrix path (1: exact fp32 MFMA, 5: bf16 hi/mid/lo x6, 6: fp16 hi/lo x3 = default) and on
    # the OPT-IN 16-bit matrix path (7: one fp16 plane per operand, BASELINE config 3's "bf16"; its own tolerance, never the default)
    by_variant = None
    if world == 1:
        from macarons_amd import ops
        by_variant = {}
        for v in (1, 5, 6, 7):
            tv = []
            with ops.variant(v):                            # per-call selection, scoped to this thread: the process default is not touched
                for it in range(3 + (20 if v == 7 else 8)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rv = nbv_step(occ, vis, pc, X, X_view, cams, grid, occ_perms=perms, samples=u)
                    int(rv["host"]["nbv_idx"][0]) if "host" in rv else int(rv["nbv_idx"])
                    torch.cuda.synchronize()
                    if it >= 3:
                        tv.append(time.perf_counter() - t0)
            pv = float(np.median(tv))
            by_variant[str(v)] = {"p50_ms": pv * 1e3, "evals_per_s": C / pv, "same_decision_as_default": int(rv["nbv_idx"]) == int(r["nbv_idx"]),
                                  "max_rel_gain_diff_vs_default": float((rv["gains"] - r["gains"]).abs().max() / r["gains"].abs().max()),
                                  "max_rel_occ_diff_vs_default": float((rv["occ"] - r["occ"]).abs().max() / r["occ"].abs().max()),
                                  "fell_back_to_variant": rv.get("fallback_variant")}
        try:                                                # the variant-7 step replayed as ONE hipGraph (captured inside the variant's scope)
            from macarons_amd.nbv import GraphedNbvStep
            with ops.variant(7):
                gs7 = GraphedNbvStep(occ, vis, pc, X, X_view, cams, grid)
                tg7 = []
                for it in range(5 + 20):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rg7 = gs7(occ_perms=perms, samples=u)
                    int(rg7["nbv_idx"])
                    torch.cuda.synchronize()
                    if it >= 5:
                        tg7.append(time.perf_counter() - t0)
            by_variant["7"]["hipgraph_replay"] = {"p50_ms": float(np.median(tg7)) * 1e3, "same_decision_as_eager": int(rg7["nbv_idx"]) == int(rv["nbv_idx"]),
                                                  "same_gains_as_eager": bool(torch.equal(rg7["gains"], rv["gains"]))}
        except Exception as e:
            by_variant["7"]["hipgraph_replay"] = {"error": repr(e)[:200]}
        by_variant["7"].update({
            "dtype": "f16 matrix operands, ONE plane (1 MFMA per product, fp32 accumulation) in the local transformers and the SconeOcc head; "
                     "LayerNorm statistics, soft-max, GELU, pooling, SH scorer, reductions fp32",
            "tolerance": "opt-in, NOT the 1e-4 contract: occupancies within 2e-3 relative on the golden weights (measured 0.7-1.2e-3; "
                         "tests/test_variant7_gpu.py states the bound per weight set), same arg-max camera on every golden decision",
            "selected_by": "ops.variant(7) / mcr_call_variant(7) per call; never a process default"})
    return {"p50_ms": p50 * 1e3, "p90_ms": float(np.percentile(times, 90)) * 1e3, "evals_per_s": C / p50, "iters": len(times),
            "hipgraph_replay": graph, "scaling": "strong", "by_variant": by_variant, "one_rank_of_8": shard8,
            "config": {"proxy_points": Q, "surface_points": M, "cams": C, "seq_len": 2048, "weights": "frozen (freeze_weight_caches: inference mode)",
                       "dtype": "f32 (matrix products of the local transformers and the head as fp16 hi/lo split, 22-bit significands, "
                                "fp32 accumulation; everything else fp32); by_variant: 1 = exact fp32 MFMA, 5 = bf16 x6",
                       "parallelism": f"query+camera shard x{world}"},
            "algorithmic_TFLOP": 26.5e6 * Q / 1e12 + 0.0037 + 0.0137, "nbv_idx": int(r["nbv_idx"]), "n_unique": int(r["n_unique"])}


def measure_nbv_batch(dev, rank, world, args, variant=None):
    """variant (optional): run on that numerics variant (7 = the opt-in 16-bit matrix path: the leg `nbv_batch_16bit`).
    BASELINE config 3: a scene batch of 8 objects x 32 768 proxy points (M = 4096 surface points each) x 200 cameras as ONE
    launch sequence (nbv.nbv_step_batch); with N >= 2 GPUs the clouds are sharded over the ranks (8 / N each, no data-path
    collective, one all-gather of the 8-byte records).  p50 latency of the 8 decisions, evals/s = 8 x 200 / p50."""
    from macarons_amd.nbv import nbv_step_batch, draw_batch, ViewStateGrid
    occ, vis = build_models(dev)
    B, M, Q, C = 8, 4096, 32768, args.cams
    g = torch.Generator(device="cpu").manual_seed(977)
    d = torch.randn(B, M, 3, generator=g)
    pc = (d / d.norm(dim=-1, keepdim=True) * torch.tensor([0.35, 0.25, 0.3]) + 0.002 * torch.randn(B, M, 3, generator=g)).to(dev)
    X = (torch.rand(B, Q, 3, generator=g) - 0.5).to(dev)
    cams = torch.randn(C, 3, generator=g)
    cams = (1.5 * cams / cams.norm(dim=1, keepdim=True)).to(dev)
    X_view = torch.stack([cams[torch.randperm(C, generator=g)[:3]] for _ in range(B)]).contiguous()
    grid = ViewStateGrid(dev)
    torch.manual_seed(13)
    perms, u = draw_batch(occ, B, M, 2048, dev)
    group = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
    import contextlib
    from macarons_amd import ops
    times = []
    with (ops.variant(variant) if variant else contextlib.nullcontext()):
        for it in range(3 + 15):
            torch.cuda.synchronize()
            if world > 1:
                torch.distributed.barrier()
            t0 = time.perf_counter()
            r = nbv_step_batch(occ, vis, pc, X, X_view, cams, grid, occ_perms=perms, samples=u, group=group)
            r["nbv_idx"].tolist()                              # the 8 decisions reach the host
            torch.cuda.synchronize()
            dt = max_over_ranks(time.perf_counter() - t0, dev, torch.distributed if world > 1 else None)
            if it >= 3:
                times.append(dt)
    p50 = float(np.median(times))
    extra = {}
    if variant == 7:                                       # beside the default numerics on the same inputs and draws
        rd = nbv_step_batch(occ, vis, pc, X, X_view, cams, grid, occ_perms=perms, samples=u, group=group)
        extra = {"variant": 7, "fell_back_to_variant": r.get("fallback_variant"),
                 "same_decisions_as_default_numerics": r["nbv_idx"].tolist() == rd["nbv_idx"].tolist(),
                 "max_rel_occ_diff_vs_default": float((r["occ"] - rd["occ"]).abs().max() / rd["occ"].abs().max()),
                 "max_rel_gain_diff_vs_default": float((r["gains"] - rd["gains"]).abs().max() / rd["gains"].abs().max()),
                 "dtype": "f16 matrix operands, ONE plane (1 MFMA per product, fp32 accumulation): BASELINE config 3's 16-bit matrix path",
                 "tolerance": "opt-in, NOT the 1e-4 contract: occupancies within 2e-3 relative on the golden weights, same arg-max camera on "
                              "every golden decision (tests/test_variant7_gpu.py)"}
    return {**extra, "p50_ms": p50 * 1e3, "evals_per_s": B * C / p50, "decisions_per_s": B / p50, "iters": len(times), "scaling": "strong",
            "config": {"workload": "BASELINE config 3: batch of 8 objects x 32768 proxy points (4096 surface points) x 200 cameras",
                       "clouds": B, "proxy_points": Q, "surface_points": M, "cams": C,
                       "dtype": "f16 single plane (variant 7, opt-in)" if variant == 7 else "f32 (fp16 hi/lo split matrix path)",
                       "parallelism": f"cloud shard x{world}" if world <= B else f"query+camera shard x{world}"},
            "nbv_idx": r["nbv_idx"].tolist()}


def measure_macarons_step(dev, rank=0, world=1):
    """BASELINE config 5 minus the depth network: p50 latency of one MACARONS next-best-view decision
    (macarons_utils.macarons_nbv_decision = testers/scene.py:391-454) on a synthetic scene of liberty's proportions: 3 x 8 x 3
    grid, 100 000 proxy points, surface = an ellipsoid shell (capacity 1000 points per cell), 256 x 456 analytic depth maps,
    30 neighbour cameras, seq_len 2048.  The poses cycle through three positions (the state keeps evolving as in a trajectory).
    With N ranks every rank holds a replica of the scene and the decision is sharded (query rows of the occupancy field and neighbour
    cameras block-partitioned); the time of an iteration is the max over the ranks.  After the clock of every iteration
    has stopped, invariants of the decision are checked at this size (nothing of this size has a golden): see `checks`."""
    from types import SimpleNamespace as NS
    from macarons_amd.networks import Macarons
    from macarons_amd.utility import macarons_utils as mu
    from macarons_amd.utility.scene import Scene
    occ, vis = build_models(dev)
    m = Macarons(None, occ, vis).to(dev).eval()
    H, W, zfar, P, K = 256, 456, 500., 100_000, 30
    rng = np.random.default_rng(55)
    x_min, x_max = torch.tensor([-21., -40., -21.], device=dev), torch.tensor([21., 40., 21.], device=dev)
    axes = np.array([9., 30., 9.])
    surface = Scene(x_min, x_max, 3, 8, 3, cell_capacity=1000, cell_resolution=0.5, n_proxy_points=P, device=dev, feature_dim=1)
    proxy = Scene(x_min, x_max, 3, 8, 3, cell_capacity=100000, cell_resolution=0.001, n_proxy_points=P, device=dev, feature_dim=1,
                  score_threshold=0.95)
    d = rng.standard_normal((60000, 3))
    surf = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True) * axes).astype(np.float32)).to(dev)
    torch.manual_seed(3)
    # the replicas of the surface scene are filled by ONE set of draws: rank 0's, through the group passed explicitly (group=None is a
    # local fill whatever process groups exist -- Scene.fill_cells)
    surface.fill_cells(surf, features=torch.zeros(len(surf), 1, device=dev),
                       **({"group": torch.distributed.group.WORLD} if world > 1 else {}))
    proxy.initialize_proxy_points()
    params = NS(n_harmonics=64, harmonic_degree=8, view_state_n_elev=7, view_state_n_azim=14, k_for_knn=16,
                prediction_neighborhood_size=3, n_view_state_cameras=98, sensor_range=70., min_occ_for_proxy_points=0.1, seq_len=2048,
                distance_factor_th=17., image_height=H, image_width=W, carving_tolerance=10.0)
    s = 1.0 / np.tan(np.deg2rad(60.0) / 2)
    Pm = np.array([[s, 0, 0, 0], [0, s, 0, 0], [0, 0, zfar / (zfar - 1), 1], [0, 0, -zfar / (zfar - 1), 0]], np.float32)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    ndc_x = W / H - jj / (H - 1) * 2.0                      # the reference Camera's NDC tables (macarons_utils.py:1921-1928)
    ndc_y = 1.0 - ii / (H - 1) * 2.0
    ndc = np.array([ndc_x[-1, -1], ndc_x[0, 0], ndc_y[-1, -1], ndc_y[0, 0]], np.float32)

    def look_at(eye, at):
        z = (at - eye) / np.linalg.norm(at - eye); x = np.cross([0., 1., 0.], z); x /= np.linalg.norm(x); y = np.cross(z, x)
        R = np.stack([x, y, z], -1)
        Mv = np.eye(4); Mv[:3, :3] = R; Mv[3, :3] = -(R.T @ eye)
        return R, Mv.astype(np.float32)

    def pose(eye, at):
        R, Mv = look_at(np.asarray(eye, float), np.asarray(at, float))
        dv = np.stack([ndc_x / s, ndc_y / s, np.ones_like(ndc_x)], -1) @ R.T
        o = np.asarray(eye, float)
        A = ((dv / axes) ** 2).sum(-1); Bq = 2 * ((o / axes) * (dv / axes)).sum(-1); Cq = ((o / axes) ** 2).sum() - 1
        disc = Bq * Bq - 4 * A * Cq
        hit = disc > 0
        tt = (-Bq - np.sqrt(np.where(hit, disc, 0))) / (2 * A)
        hit &= tt > 0
        # (a pose is host data: the camera's record stays on the host -- the decision uploads it without a stall and does its host-side
        # geometry on it without a read-back)
        cam = mu.SceneCamera(mu.camera_record(Mv, Mv @ Pm, ndc, eye, params.sensor_range), torch.tensor([eye], dtype=torch.float32), zfar)
        ne = np.asarray(eye, float) + rng.uniform(-6, 6, (K, 3))
        recs = torch.stack([mu.camera_record(mv_, mv_ @ Pm, ndc, e_, params.sensor_range)
                            for e_, mv_ in ((e_, look_at(e_, np.asarray(at, float) + rng.uniform(-4, 4, 3))[1]) for e_ in ne)]).to(dev)
        return (cam, torch.from_numpy(np.where(hit, tt, -1.0).astype(np.float32)).to(dev), torch.from_numpy(hit).to(dev), recs,
                torch.from_numpy(ne.astype(np.float32)).to(dev))
    poses = [pose([34., 10., -30.], [0., 5., 0.]), pose([-36., -8., -26.], [0., -10., 0.]), pose([30., 25., 32.], [0., 20., 0.])]
    times, info = [], None
    group = torch.distributed.group.WORLD if world > 1 else None
    dist = torch.distributed if world > 1 else None
    checks = {"iterations": 0, "n_inside_grows_by_fov_count": True, "fov_subset_of_in_field": True, "stored_proxy_indices_unique": True,
              "stored_points_inside_their_cell": True, "occupancies_finite_in_range": True, "field_rows_equal_selected_plus_out_of_field": True,
              "next_idx_is_first_strict_max": True, "gains_finite_nonnegative": True}
    # timed decisions first, back to back (as a trajectory runs them); THEN a few more decisions with the invariants checked after
    # each -- the checks read tensors back and leave the GPU idle for milliseconds, which cost the next timed decision 0.4 ms when
    # they sat between the timed ones
    n_timed, n_checked = 2 + 9, 4
    for it in range(n_timed + n_checked):
        cam, depth, dmask, recs, ne = poses[it % 3]
        n_in_before = float(proxy.proxy_n_inside_fov.sum()) if it >= n_timed else 0.0
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        with torch.no_grad():
            r = mu.macarons_nbv_decision(params, m, proxy, surface, cam, depth, dmask, recs, ne, dev, group=group)
        nxt = r["host"]["next_idx"] if "host" in r else int(r["next_idx"])     # (the decision rides on the range-flag read-back)
        torch.cuda.synchronize()
        dt = max_over_ranks(time.perf_counter() - t0, dev, dist)
        if 2 <= it < n_timed:
            times.append(dt)
        info = {"field_points": int(r["X_world"].shape[0]), "next_idx": nxt}
        if it < n_timed or os.environ.get("MCR_BENCH_NO_CHECKS"):      # (NO_CHECKS: kernel traces of the decision alone, tools/trace_macarons_step.sh)
            continue
        # ---- invariants at full size (outside the timed region)
        fm = r["fov_mask"]
        n_fov = int(fm.sum())
        checks["iterations"] += 1
        checks["n_inside_grows_by_fov_count"] &= float(proxy.proxy_n_inside_fov.sum()) - n_in_before == float(n_fov)
        checks["fov_subset_of_in_field"] &= bool((proxy.out_of_field[fm] == 0).all())
        stored = torch.cat([c.cell_features[:, 0] for c in proxy.cells.values() if c.cell_pts.shape[0] > 0]).long()
        checks["stored_proxy_indices_unique"] &= int(torch.unique(stored).numel()) == int(stored.numel())
        for c in proxy.cells.values():
            if c.cell_pts.shape[0] > 0:
                checks["stored_points_inside_their_cell"] &= bool(((c.cell_pts > c.x_min) & (c.cell_pts < c.x_max)).all()) and \
                    bool(torch.equal(proxy.proxy_points[c.cell_features[:, 0].long()], c.cell_pts))
        occ_p = r["occ_probs"]
        checks["occupancies_finite_in_range"] &= bool(torch.isfinite(occ_p).all()) and float(occ_p.min()) > -0.2
        n_sel = int(((proxy.proxy_supervision_occ > 0)[:, 0] & (proxy.out_of_field < 1)[:, 0]).sum())
        n_oof = int((proxy.out_of_field > 0).sum())
        checks["field_rows_equal_selected_plus_out_of_field"] &= r["X_world"].shape[0] == n_sel + n_oof == r["view_harmonics"].shape[0] == occ_p.shape[0]
        g_all = r["gains"]
        if world > 1:                                       # the ranks' camera shards, gathered for the check only
            from macarons_amd import dist as mdist
            g_all = mdist.allgather_rows(g_all.view(-1, 1), K, group).view(-1)
        g_h = g_all.cpu().numpy()
        checks["gains_finite_nonnegative"] &= bool(np.isfinite(g_h).all() and (g_h >= 0).all())
        checks["next_idx_is_first_strict_max"] &= nxt == int(np.argmax(g_h)) and abs(float(r["max_gain"]) - float(g_h.max())) == 0.0
        info = {"field_points": int(r["X_world"].shape[0]), "proxy_in_fov": n_fov, "next_idx": nxt}
    p50 = float(np.median(times)) if times else float("nan")
    checks["all_hold"] = all(v for k_, v in checks.items() if k_ != "iterations")
    # the same decision on the opt-in 16-bit matrix path (variant 7: its own tolerance, never the default)
    from macarons_amd import ops
    times_7 = []
    with ops.variant(7):
        for it in range(2 + 9):
            cam, depth, dmask, recs, ne = poses[it % 3]
            torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()
            t0 = time.perf_counter()
            with torch.no_grad():
                r = mu.macarons_nbv_decision(params, m, proxy, surface, cam, depth, dmask, recs, ne, dev, group=group)
            r["host"]["next_idx"] if "host" in r else int(r["next_idx"])
            torch.cuda.synchronize()
            dt = max_over_ranks(time.perf_counter() - t0, dev, dist)
            if it >= 2:
                times_7.append(dt)
    p50_7 = float(np.median(times_7))
    return {"p50_ms": p50 * 1e3, "evals_per_s": K / p50, "iters": len(times), "last": info, "checks": checks, "scaling": "strong",
            "variant_7": {"p50_ms": p50_7 * 1e3, "evals_per_s": K / p50_7, "fell_back_to_variant": r.get("fallback_variant"),
                          "note": "the opt-in 16-bit matrix path (ops.variant(7): one fp16 plane per operand in the local transformers and "
                                  "the SconeOcc head); p50_ms above is the default numerics (variant 6, the 1e-4 contract)"},
            "config": {"workload": "MACARONS decision (BASELINE config 5 minus the depth network): 100000 proxy points, 3x8x3 grid, "
                                   "30 neighbour cameras, 256x456 depth map, seq_len 2048", "cams": K, "proxy_points": P,
                       "parallelism": f"field-row + neighbour-camera shard x{world}" if world > 1 else "1 GPU"}}


def measure_local_pct(dev):
    """Roofline of the dominant kernel of the NBV step (fused local transformer): HIP events around back-to-back
    launches on the launch stream.  Default kernel = two-term fp16 split (local_pct6.hip): every algorithmic fp32 multiply-add
    runs as 3 fp16 MFMA multiply-adds, so the matrix pipe executes 3x the algorithmic GEMM flops; both the executed rate and the
    algorithmic (fp32-equivalent) rate are priced against the dense fp16 MFMA peak.  The exact-fp32-MFMA kernel is timed beside."""
    import ctypes
    from macarons_amd import ops, _lib
    from macarons_amd.networks import SconeOcc
    from macarons_amd.networks.packing import pack_local_pct
    import io, contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        occ = SconeOcc().to(dev)
    S = 16384
    offs = torch.randn(S, 16, 3, device=dev) * 0.05
    gemm_flops = S * 16 * 0.49e6                            # 0.49 MFLOP per token in linear layers
    alg_flops = gemm_flops + S * 0.164e6                    # + 16x16 attention per query
    L = _lib.lib()
    default_variant = L.mcr_get_local_pct_variant()
    out = {}
    for v in sorted({1, default_variant, 7}):
        blob = pack_local_pct(occ.local_transformers[0], v)
        with ops.variant(v):
            for _ in range(3):
                ops.local_pct_forward(offs, blob)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 20
            e0.record()
            for _ in range(n):
                ops.local_pct_forward(offs, blob)
            e1.record()
            torch.cuda.synchronize()
        out[v] = e0.elapsed_time(e1) / n
    # variant 7 runs three workgroups per CU: 16 384 queries = 4096 workgroups = 5.33 rounds of 768 (a third of the last round is tail);
    # a launch of 3 x 16 384 queries is 16 whole rounds -- the figure per 16 384 queries without the quantisation (the NBV step launches 100k)
    offs3 = torch.randn(3 * S, 16, 3, device=dev) * 0.05
    blob7 = pack_local_pct(occ.local_transformers[0], 7)
    with ops.variant(7):
        for _ in range(3):
            ops.local_pct_forward(offs3, blob7)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.local_pct_forward(offs3, blob7)
        e1.record()
        torch.cuda.synchronize()
    ms7_per_16k = e0.elapsed_time(e1) / 10 / 3
    ms = out[default_variant]
    mult = {6: 3.0, 5: 6.0}.get(default_variant, 1.0)
    if default_variant in (5, 6):
        peak = PEAK_F16_TFLOPS
        kern = f"local_pct{default_variant}_kernel"
        note = (f"dense fp16/bf16 MFMA peak 2.5 PFLOP/s; {int(mult)} MFMAs per fp32 product (split precision): `frac` = executed "
                f"matrix-pipe flops / peak, `frac_algorithmic` = algorithmic fp32-equivalent flops / the same peak")
    else:
        peak, kern, note = PEAK_FP32_TFLOPS, "local_pct_kernel", "fp32 MFMA (v_mfma_f32_32x32x2_f32) peak = 157.3 TFLOP/s"
    executed = mult * gemm_flops / (ms * 1e-3) / 1e12
    alg = alg_flops / (ms * 1e-3) / 1e12
    # what the fp16 matrix pipe sustains on this part with non-zero operands: every SIMD issuing v_mfma_f32_32x32x16_f16 back to
    # back reaches 2.43 PFLOP/s (2.40 GHz) on all-zero operands but 1.79 PFLOP/s on random ones -- the clock is managed down to
    # 1.76 GHz by the operand data (tools/experiments/mfma_power.hip)
    sustained = 1790.0 if default_variant in (5, 6) else None
    return {"kernel": kern, "bound": "mfma", "achieved": executed, "peak": peak, "unit": "TFLOP/s", "frac": executed / peak,
            "peak_sustained_random_operands": sustained, "frac_of_sustained": (executed / sustained) if sustained else None,
            "achieved_algorithmic": alg, "frac_algorithmic": alg / peak, "algorithmic_vs_fp32_mfma_peak": alg / PEAK_FP32_TFLOPS,
            "traffic": None, "device_ms_per_launch": ms, "queries_per_launch": S, "note": note,
            "single_fp16_plane_variant_7": {"kernel": "local_pct7_kernel (opt-in 16-bit matrix path)", "device_ms_per_launch": out[7],
                                            "device_ms_per_16384_queries_in_a_49152_query_launch": ms7_per_16k,
                                            "achieved": gemm_flops / (out[7] * 1e-3) / 1e12, "peak": PEAK_F16_TFLOPS,
                                            "frac": gemm_flops / (out[7] * 1e-3) / 1e12 / PEAK_F16_TFLOPS,
                                            "frac_of_sustained": gemm_flops / (out[7] * 1e-3) / 1e12 / 1790.0,
                                            "note": "one MFMA per product: executed = algorithmic GEMM flops; bound by vector issue and the "
                                                    "board's power limit (profiles/r06_local_pct7_pmc.txt, r06_power_local_pct7.txt)"},
            "exact_fp32_mfma_variant": {"kernel": "local_pct_kernel", "device_ms_per_launch": out[1],
                                        "achieved": gemm_flops / (out[1] * 1e-3) / 1e12, "peak": PEAK_FP32_TFLOPS,
                                        "frac": gemm_flops / (out[1] * 1e-3) / 1e12 / PEAK_FP32_TFLOPS}}


def max_over_ranks(dt, dev, dist):
    """MAX of a host float over the ranks (RCCL: a device tensor; the gloo test mode: a host tensor)."""
    if dist is None:
        return dt
    tw = torch.tensor([dt], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(tw, op=dist.ReduceOp.MAX)
    return float(tw.item())


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under torch.distributed.run on this node and hand
    rank 0's JSON line through as the LAST line of stdout (everything else the ranks print goes to stderr)."""
    import socket
    import subprocess
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MCR_BENCH_CHILD="1")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = r.stdout.splitlines()
    last_json = max((i for i, ln in enumerate(lines) if ln.startswith('{"metric"')), default=None)
    for i, ln in enumerate(lines):
        if i != last_json:
            print(ln, file=sys.stderr)
    sys.stderr.flush()
    if last_json is not None:
        print(lines[last_json], flush=True)
    sys.exit(r.returncode if last_json is not None or r.returncode else 3)


def timed_scorer_loop(step, finish, steps, warmup, dev, dist, streams=None):
    """W untimed + exactly `steps` timed calls of step(), bracketed by barrier + synchronize on both sides; returns
    (wall seconds = max over ranks, device ms between HIP events on the launch stream)."""
    # The W warm-up steps of a short run (the driver's --steps 20 --warmup 5 = 0.3 ms of GPU work) end before the shader clock has
    # left its idle state: 1000 more UNTIMED steps (>= 50 ms of GPU work) come first, so that the K timed steps measure the kernel and
    # not the clock ramp.  A FIXED count: every rank must submit the same number of decisions to the exchange (a time-based loop ran a
    # different number of steps on each rank, their record batches fell out of step and the ranks met in different collectives).
    for _ in range(1000):
        step()
    torch.cuda.synchronize()
    # ... and the W warm-up steps proper run LAST, behind that burst's synchronize: the FIRST operation submitted after the synchronize
    # that ends a long burst costs the host 250-350 us, once, whatever it is (a step, a lone event record: tools/time_scorer_short2.py).
    # That is the untimed burst's cost; with the burst last it landed on the first timed launch (60 us per step at 20 steps instead
    # of 47-49).  (W = 0: an event record takes the place of the warm-up steps.)
    torch.cuda.Event(enable_timing=True).record()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    finish(None)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    out = None
    for _ in range(steps):
        out = step()
    out = finish(out)
    # steps issued on side streams: one closing event per stream (a join on the current stream costs a cross-stream wait of tens of
    # microseconds after the last kernel); the device time of the region ends with the latest of them
    ends = [ev1]
    ev1.record()
    for st in streams or ():
        e = torch.cuda.Event(enable_timing=True)
        e.record(st)
        ends.append(e)
    if os.environ.get("MCR_BENCH_SPIN_SYNC", "1") != "0":
        # hipDeviceSynchronize may put the host thread to sleep and be woken by an interrupt tens of microseconds after the last kernel
        # retired -- 5 us per step of a 20-step run; polling the events notices the end within a microsecond, the synchronize behind it
        # (still there: the contract's bracket) then returns at once
        while not all(e.query() for e in ends):
            pass
    torch.cuda.synchronize()
    if dist is not None:                                    # (one rank: the synchronize above already is the closing bracket)
        dist.barrier()
        torch.cuda.synchronize()
    wall = max_over_ranks(time.perf_counter() - t0, dev, dist)
    return wall, max(ev0.elapsed_time(e) for e in ends), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--strong-cams", type=int, default=512, help="total cameras of the strong-scaling scorer run (config 4)")
    ap.add_argument("--waves-per-simd", type=int, default=0)
    ap.add_argument("--streams", type=int, default=2, help="streams the scorer steps are issued on, round-robin (1: every step on the current stream)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the in-run rocprofv3 --pmc FETCH_SIZE pass (roofline.traffic then comes from profiles/)")
    ap.add_argument("--no-nbv", action="store_true", help="skip the NBV-step latency measurement")
    ap.add_argument("--no-strong", action="store_true", help="skip the config-4 strong-scaling scorer leg (profiling the headline size alone)")
    ap.add_argument("--nbv-iters", type=int, default=50)
    ap.add_argument("--watchdog", type=int, default=0, help="seconds after which every rank dumps its Python stacks to stderr and exits (0 = off): "
                                                            "a rank stuck in a collective reports where, instead of hanging the job")
    ap.add_argument("--legs-deadline", type=int, default=None, help="seconds the extra legs (NBV step, scene batch, MACARONS decision, CPU baselines) "
                                                                    "may take together before every rank leaves and rank 0 prints the contract line without them "
                                                                    "(default: 240 on one GPU -- they take ~25 s -- and 120 on several)")
    ap.add_argument("--full", action="store_true", help="besides the headline (A): the strong-scaling leg, the kernel-alone roofline, the "
                                                        "in-run PMC traffic pass, the NBV / scene-batch / MACARONS legs and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the outputs of the last timed step of (A) as DIR/<name>.npy")
    args = ap.parse_args()

    if args.watchdog > 0:
        import faulthandler
        faulthandler.dump_traceback_later(args.watchdog, exit=True)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.legs_deadline is None:
        args.legs_deadline = 240 if max(world, args.gpus) == 1 else 120
    if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
        self_launch(args)                                  # plain `python bench.py --gpus N`: become the launcher of N ranks (never returns)
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: running with WORLD_SIZE", file=sys.stderr)
    # MCR_TEST_BACKEND=gloo: every rank on cuda:0 of a one-GPU box with host-staged collectives (RCCL refuses duplicate devices) --
    # the mode the test suite uses to run the N = 2 path end to end on one GPU; the product path is RCCL
    backend = os.environ.get("MCR_TEST_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    use_dist = world > 1 or bool(os.environ.get("MCR_BENCH_FORCE_DIST"))      # the env knob exercises the RCCL path on one GPU
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))

    from macarons_amd import ops
    from macarons_amd import dist as mdist
    N, C = args.points, args.cams

    ranks_seen = 1
    if dist is not None:                                   # every rank's id through an RCCL all-gather
        ids = torch.empty(world, dtype=torch.int32, device=dev)
        mdist.all_gather_into(ids, torch.tensor([rank], dtype=torch.int32, device=dev))
        ranks_seen = int(torch.unique(ids).numel())

    # the scorer as the product exposes it: torch.ops.macarons.sh_coverage_gain of the C++ TORCH_LIBRARY extension (what
    # SconeVis.compute_coverage_gain calls); the ctypes wrapper of the same C entry point when a non-default occupancy is asked for
    scorer_entry = "torch.ops.macarons.sh_coverage_gain (libmacarons_torch.so -> mcr_sh_coverage_gain)"
    # one step = the gains of every camera + the decision (torch.max over them): torch.ops.macarons.sh_coverage_gain_best -- ONE
    # dispatcher call for the three launches (gain kernel, deterministic reduce, arg-max record)
    scorer_entry = ("torch.ops.macarons.sh_coverage_gain_best (libmacarons_torch.so -> mcr_sh_coverage_gain_best = mcr_sh_coverage_gain, "
                    "what SconeVis.compute_coverage_gain calls, + the arg-max record)")
    if args.waves_per_simd == 0:
        import macarons_amd.torch_ops  # noqa: F401
        score_best = lambda p_, h_, c_: torch.ops.macarons.sh_coverage_gain_best(p_, h_, c_, True)
    else:
        scorer_entry = "macarons_amd.ops.sh_coverage_gain_best (ctypes -> mcr_sh_coverage_gain_best)"
        score_best = lambda p_, h_, c_: ops.sh_coverage_gain_best(p_, h_, c_, True, args.waves_per_simd)

    scorer_streams = []
    last_gains = [None]                                    # the gains of the latest step (what --dump-outputs writes)

    def scorer_run(pts, harm, cams, cam_offset, steps, warmup):
        # --streams S (default 2): consecutive steps are independent batches and are issued round-robin on S streams, each step whole
        # and stream-ordered on its own stream (fresh outputs and scratch from the stream-aware allocator): the reduce / record launch of
        # one step runs beside the gain kernel of the next, and two gain kernels fill each other's ramp and tail (43 us per step against
        # 56 on one stream; --streams 1 is the one-stream figure)
        # (side streams only: with the current -- default -- stream as one of the two, short runs measured erratically; ONE set of
        # streams for every leg: a second pair, created for the strong leg, shared a hardware queue and its steps did not overlap)
        if args.streams > 1 and not scorer_streams:
            scorer_streams.extend(torch.cuda.Stream(device=dev) for _ in range(args.streams))
        streams = scorer_streams if args.streams > 1 else None
        pipe = mdist.PipelinedBest(1, dev, batch=16, depth=3, producers=streams or ()) if dist is not None else None
        issued = [0]

        def step():
            def one():
                gains, record = score_best(pts, harm, cams)    # record [B,2] = (max gain, arg-max camera): the decision (torch.max semantics)
                last_gains[0] = gains
                if pipe is not None:                           # records of 16 decisions per all-gather, on a side stream
                    return pipe.submit(gains, cam_offset)      # (the record kernel on the step's own stream; the exchange waits for all of them)
                return record
            if streams is None:
                return one()
            st = streams[issued[0] % len(streams)]
            issued[0] += 1
            with torch.cuda.stream(st):
                return one()

        def finish(handle):
            if pipe is None:
                return handle
            pipe.flush()
            return pipe.result(handle) if handle is not None else None    # the last decision (and all earlier ones) is complete
        return timed_scorer_loop(step, finish, steps, warmup, dev, dist, streams)

    # ---- (A) weak scaling: every rank its own shard of C cameras out of world*C -------------------------------------------
    pts, harm, cams = make_inputs(N, C, 1234, dev, cam_offset=rank * C, n_cam_total=world * C)
    wall, dev_ms, decision = scorer_run(pts, harm, cams, rank * C, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_gains[0], decision)

    def headline():
        """The contract line: the fields of (A), all that a plain run prints."""
        return {
            "metric": "candidate-camera coverage-gain evals/sec (100k pts, 200 cams)",
            "value": world * C * args.steps / wall, "unit": "evals/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": wall * 1e3 / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"scorer: B=1 cloud x N={N} points x C={C} cameras per GPU "
                                   f"(BASELINE headline 100k pts / 200 cams), inputs resident in HBM",
                       "points": N, "cams_per_gpu": C, "parallelism": f"camera-shard x{world}", "entry": scorer_entry,
                       "streams": args.streams, "untimed_clock_ramp_steps": 1000,
                       "timing_note": "1000 untimed clock-ramp steps precede the --warmup steps (a warm-clock number by construction: the "
                                      "driver's --warmup 5 alone ends before the shader clock has left idle); steps are independent batches "
                                      f"issued round-robin on {args.streams} stream(s): roofline.ms_per_step_one_stream (--full) is the "
                                      "one-stream step"},
            "ranks_seen": ranks_seen,
        }

    if not args.full:
        leave(dist, rank, lambda: print(json.dumps(headline()), flush=True))
        return

    # ---- (A') strong scaling, BASELINE config 4: strong_cams cameras in total, block-partitioned ---------------------------
    Cs = args.strong_cams
    c0, c1 = mdist.shard_range(Cs, rank, world)
    _, _, cams_s = make_inputs(N, Cs, 1234, dev)
    cams_s = cams_s[:, c0:c1].contiguous()
    s_steps, s_warm = max(20, min(args.steps, 500)), max(5, min(args.warmup, 50))
    strong = None
    if args.no_strong:
        wall_s = float("nan")
    elif c1 > c0:
        wall_s, _, _ = scorer_run(pts, harm, cams_s, c0, s_steps, s_warm)
    else:                                                  # more ranks than cameras cannot happen at 512 cameras; keep the barriers aligned
        wall_s, _, _ = timed_scorer_loop(lambda: None, lambda h: h, s_steps, s_warm, dev, dist)
    strong = None if args.no_strong else {"metric": f"coverage-gain evals/s, N={N} points x {Cs} cameras in total (BASELINE config 4), strong scaling",
              "value": Cs * s_steps / wall_s, "unit": "evals/s", "steps": s_steps, "warmup": s_warm,
              "ms_per_step": wall_s * 1e3 / s_steps, "cams_total": Cs, "cams_this_rank": c1 - c0, "scaling": "strong"}

    # ---- dominant kernel alone: sh_gain_kernel (first stage of the scorer), HIP events around back-to-back launches -------
    kern_ms, one_stream = None, {}
    if rank == 0:
        for _ in range(20):
            ops.sh_coverage_gain_partials(pts, harm, cams, True, args.waves_per_simd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        nk = 300
        e0.record()
        for _ in range(nk):
            ops.sh_coverage_gain_partials(pts, harm, cams, True, args.waves_per_simd)
        e1.record()
        torch.cuda.synchronize()
        kern_ms = e0.elapsed_time(e1) / nk
        # the same step with every launch on ONE stream (what one NBV loop sees): 50 untimed + 300 timed steps on the current stream,
        # clocks warm from the loops above; wall time between synchronizes and device time between HIP events
        for _ in range(50):
            score_best(pts, harm, cams)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        e0.record()
        for _ in range(300):
            score_best(pts, harm, cams)
        e1.record()
        torch.cuda.synchronize()
        one_stream = {"ms_per_step_one_stream": (time.perf_counter() - t1) * 1e3 / 300, "step_device_ms_one_stream": e0.elapsed_time(e1) / 300}
    if dist is not None:
        dist.barrier()

    # ---- (B) the extra legs (NBV step, scene batch, MACARONS decision), sharded over the ranks -------------------------------
    # The contract line (the scorer loop above) is complete at this point.  The extra legs run under a deadline on EVERY rank: a leg
    # that raises is reported in its field; if the legs hang (a rank that left a collective) every rank leaves at the deadline and
    # rank 0 still prints the contract line with what was measured -- a secondary leg must not cost the job its record.
    import threading
    legs = {}
    legs_done = threading.Event()
    state = {"emit": None}

    def on_deadline():
        if legs_done.is_set():
            return
        sys.stderr.write(f"bench.py: rank {rank}: the extra legs did not finish within {args.legs_deadline} s -- leaving with the contract line\n")
        try:
            import faulthandler
            faulthandler.dump_traceback(file=sys.stderr)
        except Exception:
            pass
        sys.stderr.flush()
        if rank == 0 and state["emit"] is not None:
            state["emit"](f"extra legs stopped at the {args.legs_deadline} s deadline; finished: {sorted(legs)}")
        os._exit(0)

    leg_seconds = {}

    def run_leg(name, fn):
        t_leg = time.perf_counter()
        try:
            legs[name] = fn()
        except Exception as e:                              # reported in the leg's field, never fatal for the contract line
            legs[name] = {"error": repr(e)[:300]}
            sys.stderr.write(f"bench.py: rank {rank}: leg {name} failed: {e!r}\n")
        leg_seconds[name] = round(time.perf_counter() - t_leg, 2)

    if rank == 0:
        step_ms = dev_ms / args.steps              # device time of one whole step (gain + reduce + decision record)
        alg_flop = N * C * FLOP_PER_PAIR
        exe_flop = N * C * FLOP_PER_PAIR_EXECUTED
        achieved = exe_flop / (kern_ms * 1e-3) / 1e12
        achieved_ref = alg_flop / (kern_ms * 1e-3) / 1e12
        pmc_name = next((n_ for n_ in ("r05_scorer_pmc.json", "r04_scorer_pmc.json", "r03_scorer_pmc.json", "r02_scorer_pmc.json", "r01_scorer_pmc.json") if pmc_profile(n_)), None)
        pmc = pmc_profile(pmc_name) if pmc_name else {}
        valu = (pmc.get("per_dispatch_mean") or {}).get("SQ_INSTS_VALU")
        traffic, traffic_source = ((None, "skipped (--no-pmc / N > 1)") if (args.no_pmc or world > 1 or os.environ.get("MCR_BENCH_NO_PMC"))
                                   else measure_scorer_traffic(N, C))
        if traffic is None:                                # no rocprofv3 / pass failed: the committed profile's figure, labelled as such
            traffic_source = f"static: profiles/{pmc_name} ({traffic_source})"
            traffic = pmc.get("hbm_read_bytes_per_launch_corrected")
        roof = {"bound": "valu-fp32", "achieved": achieved, "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
                "frac": achieved / PEAK_FP32_TFLOPS, "kernel": "sh_gain_kernel<true>", "device_ms_per_launch": kern_ms,
                "flop_per_pair_executed": FLOP_PER_PAIR_EXECUTED, "flop_per_pair_reference_formulation": FLOP_PER_PAIR,
                "frac_meaning": "flop the kernel EXECUTES (171 per pair: 77 FMA x 2 + 14 + 3 of its 94 vector instructions per pair, counted on "
                                "the ISA) / kernel time / fp32 vector peak: cannot exceed the pipe's issue-slot utilisation (executed_valu_frac). "
                                "The SURVEY 8(d) figure -- 370 flop per pair of the REFERENCE's formulation -- is kept as "
                                "achieved_reference_formulation / frac_reference_formulation: it measures how much faster than a literal "
                                "restatement the trig-free form is and may pass 1",
                "achieved_reference_formulation": achieved_ref, "frac_reference_formulation": achieved_ref / PEAK_FP32_TFLOPS,
                "timing": "HIP events around 300 back-to-back launches of the kernel alone (mcr_sh_coverage_gain_partials)",
                "executed_flop_per_launch": exe_flop, "algorithmic_flop_per_launch": alg_flop, "algorithmic_bytes": N * BYTES_PER_POINT,
                "traffic": traffic, "traffic_source": traffic_source,
                "hbm_algorithmic_GBs": N * BYTES_PER_POINT / (kern_ms * 1e-3) / 1e9,
                "step_device_ms": step_ms, "step_achieved": exe_flop / (step_ms * 1e-3) / 1e12,
                "step_frac": exe_flop / (step_ms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS,
                "step_frac_reference_formulation": alg_flop / (step_ms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS,
                "step_meaning": f"device time of the timed region / steps, with the steps issued on {args.streams} stream(s): with two steps in "
                                "flight the gain kernels overlap each other's ramp and tail and the reduce launches, so a step costs less than "
                                "the kernel ALONE (device_ms_per_launch, what `achieved` / `frac` price); ms_per_step_one_stream is the same "
                                "step with every launch on ONE stream (kernel alone <= that step)"}
        roof.update(one_stream)
        if valu:
            # wave-level vector instructions issued per launch (PMC) x 2 cycles each (a SIMD retires 32 fp32 lanes per cycle:
            # 157.3 TFLOP/s = 1024 SIMDs x 2.4 GHz x 64 flop) / (SIMDs x kernel cycles at 2.4 GHz)
            roof["executed_valu_frac"] = valu * 2.0 / (1024 * kern_ms * 1e-3 * 2.4e9)
            roof["executed_valu_frac_meaning"] = (f"vector instructions the kernel EXECUTES (SQ_INSTS_VALU per launch from profiles/{pmc_name}: a "
                                                  "static property of the code at this size) x 2 issue cycles / (1024 SIMDs x kernel cycles at "
                                                  "2.4 GHz): how busy the vector pipe is, as opposed to `frac`")
            roof["valu_insts_per_launch"] = valu
        res = dict(headline(), roofline=roof, scorer_strong=strong)
    else:
        res = None

    def emit(note=None):
        out = dict(res)
        for k_, v_ in (("nbv_step", legs.get("nbv")), ("nbv_batch", legs.get("nbv_batch")), ("nbv_batch_16bit", legs.get("nbv_batch_16bit")),
                       ("macarons_step", legs.get("mac")),
                       ("roofline_nbv_dominant", legs.get("lp"))):
            if v_ is not None:
                out[k_] = v_
        for k_ in ("cpu_baseline", "cpu_baseline_nbv"):
            if k_ in legs:
                out[k_] = legs[k_]
        # the strong-scaling numbers north_star asks for (fixed total work, N GPUs), side by side with the contract's weak-scaling value
        summ = {"weak_scorer_evals_per_s": out.get("value"), "n_gpus": out.get("n_gpus")}
        if out.get("scorer_strong"):
            summ["strong_scorer_config4_evals_per_s"] = out["scorer_strong"]["value"]
        for key, leg in (("nbv_step", "nbv_step"), ("nbv_batch", "nbv_batch"), ("nbv_batch_16bit_variant7", "nbv_batch_16bit"),
                         ("macarons_decision", "macarons_step")):
            if out.get(leg):
                summ[f"strong_{key}_p50_ms"] = out[leg]["p50_ms"]
                summ[f"strong_{key}_evals_per_s"] = out[leg]["evals_per_s"]
        if out.get("nbv_step") and out["nbv_step"].get("one_rank_of_8"):
            summ["nbv_step_one_rank_of_8_p50_ms"] = out["nbv_step"]["one_rank_of_8"]["p50_ms"]
        out["scaling_summary"] = summ
        out["leg_seconds"] = dict(leg_seconds)
        if note:
            out["legs_incomplete"] = note
        sys.stdout.flush()
        print(json.dumps(out), flush=True)
    if rank == 0:
        state["emit"] = emit
    timer = threading.Timer(args.legs_deadline, on_deadline)
    timer.daemon = True
    timer.start()
    if not args.no_nbv:
        run_leg("nbv", lambda: measure_nbv_step(dev, rank, world, args))
        run_leg("nbv_batch", lambda: measure_nbv_batch(dev, rank, world, args))
        run_leg("nbv_batch_16bit", lambda: measure_nbv_batch(dev, rank, world, args, variant=7))
        if rank == 0:
            run_leg("lp", lambda: measure_local_pct(dev))
        run_leg("mac", lambda: measure_macarons_step(dev, rank, world))   # every rank: the decision is sharded over the ranks
    if dist is not None:
        dist.barrier()
    if rank == 0 and not args.no_cpu_baseline and world == 1:
        def cpu_leg():
            n_s = min(C, max(24, os.cpu_count() or 1))
            cb, g_cpu = cpu_baseline(pts, harm, cams[:, :n_s].contiguous())
            g_gpu = ops.sh_coverage_gain(pts, harm, cams[:, :n_s].contiguous()).cpu().numpy()
            cb["max_rel_diff_vs_gpu"] = float(np.abs(g_gpu - g_cpu).max() / np.abs(g_cpu).max())
            return cb
        run_leg("cpu_baseline", cpu_leg)
        if not args.no_nbv:
            run_leg("cpu_baseline_nbv", lambda: cpu_baseline_nbv(C))
    legs_done.set()
    timer.cancel()
    leave(dist, rank, emit)


def dump_outputs(path, gains, decision):
    """--dump-outputs: the last timed step's gains [B, C] and decision record [B, 2] = (max gain, arg-max camera), float32."""
    if isinstance(decision, tuple):                        # N > 1: the exchanged decision (max gains, global camera indices)
        decision = torch.stack([decision[0].float(), decision[1].float()], -1)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "gains.npy"), gains.float().cpu().numpy())
    np.save(os.path.join(path, "record.npy"), decision.float().cpu().numpy())


def leave(dist, rank, emit):
    """End of a run: rank 0 prints its JSON line (emit) as the LAST line of stdout."""
    if dist is not None:
        dist.destroy_process_group()       # RCCL prints its version banner to stdout on the way out: keep the JSON the LAST line
    sys.stdout.flush()
    if rank == 0:
        emit()
    if dist is not None:
        # librccl prints its version banner to stdout when the process winds down (after destroy_process_group, on every rank):
        # leave without running the exit handlers so that rank 0's JSON stays the LAST line of the job's output
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()
