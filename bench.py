#!/usr/bin/env python
"""bench.py — query images/s of the Gen6D tensor hot path (detect + select + 3x refine, 64 reference views) on
N MI355X, one process per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A step = one BATCH of `--batch` queries (default 4) through the whole path in one set of launches — the reference API is batched
([qn,H,W,3] queries, network/detector.py:291-304, selector.py:165-175) — each query: detector on a synthetic 480x640 frame
against 32 reference views, selector on a synthetic 128x128 crop against 64 views x 5 in-plane rotations, 3 refiner steps with 6
reference crops (weights: seeded synthetic state_dicts; no checkpoint/dataset exists offline).  Queries are independent, so the
path shards by query: every rank holds a replica of the reference state and runs its own K steps (weak scaling, no
collective on the data path); value = N*K*batch / max-over-ranks time; `single_query_ms` = latency of one query alone (batch 1).

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit, ms_per_step, dtype, ...).
`--dump-outputs DIR` writes what the timed path returned in its last step (rank 0) as DIR/rows.npy.  Everything else below
is measured only with `--full`.

Extra objects on the JSON line (--full):
  roofline     — the dominant MFMA-bound kernel family by serialised time (since round 2 the Winograd kernel: own VGG trunk +
                 the conv layers routed to it): FLOPs EXECUTED by every launch divided by its HIP-event duration (events
                 recorded on the launch stream), against 157.3 TFLOP/s; for the Winograd family the direct-form equivalent
                 (x2.25) is given beside it.  roofline_conv / roofline_winograd — the other family, same fields.
  cpu_baseline — the CPU oracle (a port of the reference's PyTorch-CPU path) timed on this host for one query: physical
                 cores, 1 warm-up + min of 3, per-stage seconds, torch.std share.
  parity_vs_reference — every timed row against the rows the reference's own modules produce (tests/golden/pipeline_rows.npz).
  lowp         — the same launch mode with bf16 / fp16 matrix-core operands (opt-in speed mode, graded separately).
  chained      — (--chained) the device-resident predict chain with real data flow between the stages.
  hbm_kernels  — the HBM-bound kernels of the path (selector scan, refiner volume, FC weight stream): algorithmic
                 bytes / HIP-event time against 8 TB/s.
  stages_ms    — per-stage GPU time of one query (eager launches).
"""
import argparse
import json
import os
import sys
import time

# Four queries in flight on four streams need four hardware queues of their own: ROCm maps a process's streams onto 4 queues by
# default (the null stream included), where the fourth lane collides (measured: 3 lanes 142.7, 4 lanes 113-135, 4 lanes with 8
# queues 147.2 images/s).  Read by the HIP runtime at initialisation, i.e. before torch is imported; an explicit setting wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3       # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32
LOWP_MFMA_PEAK_TFLOPS = 2500.0      # dense 16-bit MFMA peak (same guide; AMD's 5 PFLOP/s figure is 2:1 sparse)


def stage_times(pipe, full, crop, reps=5):
    """Per-stage GPU time of ONE query alone (ms, HIP events on the current stream, eager launches)."""
    r = pipe.ref_dev
    stages = {
        "detector": lambda: pipe.detector.detect_impl(full),
        "selector": lambda: pipe.selector.compute_view_point_feats(crop),
        "refiner_step": lambda: pipe.refiner._step(crop, r["Ks_in"][0], pipe.iter_poses[0][0], r["ref_imgs"][0],
                                                   r["ref_Ks"][0], r["ref_poses"][0]),
    }
    out = {}
    with torch.no_grad():
        for name, fn in stages.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            out[name] = e0.elapsed_time(e1) / reps
    return out


def ref_sweep(dev, B, lanes, steps, warmup):
    """north_star's reference-view sweep on the current code: the full pipeline (detector 480x640 vs 32 refs + selector + 3 refiner
    steps) at 32 / 128 selector reference views x 5 rotations, timed like the headline (hipGraph replay, `lanes` batches of B in
    flight), plus BASELINE configs[1] — the selector alone at 64 views x 36 rotations (reference network/selector.py:13-15,97-104 is
    parametric in the rotation count; configs/gen6d_pretrain.yaml:10 uses 5).  Each entry: images/s, the Winograd family's executed
    TFLOP/s and fraction of the fp32 MFMA peak from a serialised eager pass, and the selector logits against the reference's own
    (tests/golden/sel_128x5.npz, sel_64x36.npz) where such a fixture exists."""
    from gen6d_amd import ops, synth
    from gen6d_amd.pipeline import TensorPipeline
    fulls = synth.imgs_to_tensor(synth.synth_images(4, 480, 640, seed=100)).to(dev)
    crops = synth.imgs_to_tensor(synth.synth_images(4, 128, 128, seed=200)).to(dev)
    out = {}

    def logits_parity(pipe, tag):
        gp = os.path.join(ROOT, "tests", "golden", tag + ".npz")
        if not os.path.exists(gp):
            return None
        g = np.load(gp)
        with torch.no_grad():
            lg = pipe.selector.compute_view_point_feats(pipe.sel_case["que_imgs"].to(dev))[0].cpu().numpy()
        return {"source": f"tests/golden/{tag}.npz (the reference's own module)", "logits_max_abs_diff": float(np.abs(lg - g["logits"]).max()),
                "argmax_equal": bool((lg.argmax(1) == g["logits"].argmax(1)).all()), "bar": 1e-4}

    def wino_frac(fn):
        ops.SERIAL = True
        with torch.no_grad():
            fn(); torch.cuda.synchronize()
            ops.PROFILE, ops.PROFILE_HBM = [], {}
            fn(); torch.cuda.synchronize()
        prof, ops.PROFILE, ops.PROFILE_HBM = ops.PROFILE, None, None
        r = {}
        for key, sel in (("winograd", lambda p: p[3].startswith("wino3x3")), ("all_mfma", lambda p: True)):
            pp = [p for p in prof if sel(p)]
            fl, ms = sum(p[0] for p in pp), sum(p[1].elapsed_time(p[2]) for p in pp)
            r[key] = {"achieved_TFLOPs_executed": fl / (ms * 1e-3) / 1e12, "frac_of_fp32_mfma_peak": fl / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                      "ms_per_batch": ms}
        return r

    for sel_refs in (32, 128):
        pipe = TensorPipeline(dev, sel_rfn=sel_refs, det_rfn=32); pipe.build()
        ops.SERIAL = True
        pipe.capture(lanes=lanes, batch=B)
        busy = [None] * lanes
        def run(n):
            for i in range(n):
                idx = torch.tensor([(i * B + b + i // lanes) % 4 for b in range(B)], device=dev)
                lane = i % lanes
                if busy[lane] is not None: busy[lane].synchronize()
                _, stream = pipe.query_graph(fulls[idx], crops[idx], lane)
                ev = torch.cuda.Event(); ev.record(stream); busy[lane] = ev
            torch.cuda.synchronize()
        run(warmup)
        t0 = time.perf_counter(); run(steps); dt = time.perf_counter() - t0
        idx = torch.arange(B, device=dev) % 4
        out[f"{sel_refs}x5"] = {"workload": f"full pipeline, selector {sel_refs} refs x 5 rotations, detector 32 refs, 3 refine steps",
                                "value": steps * B / dt, "unit": "images/s", "ms_per_step": dt / steps * 1e3, "batch": B, "lanes": lanes,
                                "roofline": wino_frac(lambda: pipe.query(fulls[idx], crops[idx])),
                                "parity_vs_reference": logits_parity(pipe, f"sel_{sel_refs}x5")}
        del pipe; torch.cuda.empty_cache()
    # BASELINE configs[1]: selector only, 64 views x 36 rotations (D = 2304 hypotheses per query)
    pipe = TensorPipeline(dev, sel_rfn=64, det_rfn=32, an=36); pipe.build()
    ops.SERIAL = True
    idx = torch.arange(B, device=dev) % 4
    g_in = crops[idx].clone()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream), torch.no_grad():
        for _ in range(2): pipe.selector.compute_view_point_feats(g_in)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"), torch.no_grad():
        g_out = pipe.selector.compute_view_point_feats(g_in)
    for _ in range(2): graph.replay()
    torch.cuda.synchronize()
    n = max(10, steps)
    t0 = time.perf_counter()
    for _ in range(n): graph.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["64x36_selector_only"] = {"workload": "BASELINE configs[1]: selector only, 64 refs x 36 rotations, 128x128 queries", "value": n * B / dt,
                                  "unit": "queries/s", "ms_per_step": dt / n * 1e3, "batch": B, "lanes": 1,
                                  "roofline": wino_frac(lambda: pipe.selector.compute_view_point_feats(g_in)),
                                  "parity_vs_reference": logits_parity(pipe, "sel_64x36")}
    del pipe, graph, g_out; torch.cuda.empty_cache()
    return out


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: re-exec under torch.distributed.run
    (one process per GPU, rendezvous on 127.0.0.1) and exit with its return code.  On a box with fewer than N GPUs
    (e.g. a 1-GPU lease) the ranks share the visible GPUs and the collectives go over gloo — RCCL refuses two ranks
    on one device — which still exercises the whole multi-rank path; the JSON line names the backend."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sel-refs", type=int, default=64)
    ap.add_argument("--det-refs", type=int, default=32)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--lowp", default="fp16,fp16ref32,bf16",
                    help="comma list of reduced-precision schemes measured AFTER the fp32 headline (same launch mode, same steps) and "
                         "reported in the `lowp` object, each with its ALL-ROWS parity bar (gen6d_amd/bars.py) on the 4 bench queries + 16 held-out "
                         "ones; '' = skip.  fp16 = every stage on fp16 operands (selector query trunk / tail on fp32: cfg lowp_keep_fp32) — "
                         "BASELINE configs[4]; fp16ref32 = the same with the refiner on fp32 operands (the scheme that holds the all-rows bar on "
                         "the synthetic weights); bf16 = every stage on bf16 operands — BASELINE configs[2] as it reads; also: bf16mix (detector / "
                         "refiner bf16, selector fp16), fp16all (nothing kept on fp32), fp16sel32 (selector fp32)")
    ap.add_argument("--lowp-lanes", type=int, default=3,
                    help="batches in flight during the reduced-precision passes (their kernels are ~2x shorter, so replay gaps weigh "
                         "more: 342 images/s with 2, 357 with 3; fp32 gains 1 %% from a third lane and keeps the 2 of --lanes)")
    ap.add_argument("--no-cached", action="store_true", help="skip the reference-feature-cache side measurement (`cached` object)")
    ap.add_argument("--no-chained", action="store_true", help="skip the `chained` measurement")
    ap.add_argument("--no-sweep", action="store_true", help="skip the reference-view sweep (`sweep` object: 32 / 128 refs x 5 full pipeline, "
                                                            "64 x 36 selector only)")
    ap.add_argument("--chained", action="store_true",
                    help="(default since round 4; kept for old command lines) additionally time the device-resident predict chain (gen6d_amd/chain.py: detection -> crop -> selection "
                         "-> pose -> 3 x refine with every inter-stage warp and the pose algebra on the GPU, one captured graph "
                         "per lane) on a procedural 480x640 database with REAL data flow between the stages; reported as `chained`")
    ap.add_argument("--chain-batch", type=int, default=8, help="queries per captured graph of the --chained measurement")
    ap.add_argument("--cpu-reps", type=int, default=3, help="timed CPU-oracle runs after one warm-up (min is reported)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="torch CPU threads for the baseline (0 = best of {8,16,32,64,physical cores})")
    ap.add_argument("--no-graph", action="store_true", help="time the eager launch path instead of hipGraph replay")
    ap.add_argument("--batch", type=int, default=16,
                    help="queries per step: they go through every launch together (M dimension of the conv / correlation grids, one "
                         "pass over the selector's reference cache, one FC weight stream), 1..32 (the detector cuts at 16)")
    ap.add_argument("--lanes", type=int, default=3,
                    help="independent hipGraph copies (one batch each) kept in flight on separate streams (round 5, batches of 16: 2 lanes "
                         "247.7, 3 lanes 251.5, 4 lanes 251.4 images/s; 32 x 2: 251.1 — profiles/r05_batch_lanes.md)")
    ap.add_argument("--serial", action="store_true",
                    help="profiling aid: no stream fork/join and no graph, so that per-kernel durations in a rocprofv3 "
                         "trace are not inflated by overlap (this is how the roofline pass itself runs)")
    ap.add_argument("--fork", action="store_true",
                    help="graph mode: also fork the independent branches of ONE query (4 detector scales, 3 selector levels, "
                         "3 refiner feature branches) onto side streams inside each graph.  Off by default: measured, the "
                         "chip is filled better by whole queries in flight on separate streams (89 vs 69 images/s)")
    ap.add_argument("--force-dist", action="store_true",
                    help="create the process group at world size 1 as well (RCCL accepts every collective on one rank): the multi-rank "
                         "plumbing of the query-replica mode — barrier, MAX-reduce of the time, all-gather of the rows, graph capture next to the "
                         "process group's watchdog thread — then runs on a 1-GPU box exactly as it does on N (tests/test_rccl_world1_gpu.py)")
    ap.add_argument("--shard-refs", action="store_true",
                    help="strong-scaling variant: all ranks work on the SAME query stream, the selector's reference cache "
                         "is sharded over the ranks (RCCL statistics all-reduces + feature all-gather); default is query replicas")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement after the headline: rooflines, per-stage and single-query times, parity against "
                         "the reference's rows, reduced-precision modes, reference-feature cache, chained path, reference-view sweep, CPU "
                         "baseline, collective log of --shard-refs.  Off by default: a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write rank 0's result rows of the LAST timed step to DIR/rows.npy (float32 [batch, 26]: "
                         "position(2), scale, ref_idx, angle, then quaternion(4), offset(2), log2-scale of each of the 3 refine steps)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    self_launch(args)

    from gen6d_amd import lib, ops, parallel, synth
    from gen6d_amd.pipeline import TensorPipeline
    lib.load()                                           # no HIP library -> hard failure
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    n_dev = torch.cuda.device_count()
    want_world = int(os.environ.get("WORLD_SIZE", "1"))
    backend = os.environ.get("G6D_DIST_BACKEND") or ("nccl" if n_dev >= want_world else "gloo")   # nccl = RCCL over xGMI
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % n_dev)
    # `--shard-refs --gpus 1`: a one-rank RCCL process group — the sharded path issues its 9 + 1 collectives per batch on it
    rank, world, local = parallel.init_from_env(backend=backend, force=(args.shard_refs or args.force_dist) and want_world == 1)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    local = local % n_dev                            # (fewer GPUs than ranks: several ranks share a device, gloo)
    dev = torch.device("cuda", local)
    ranks_seen = int(parallel.sum_over_ranks(1, dev))

    shard_refs = args.shard_refs
    pipe = TensorPipeline(dev, sel_rfn=args.sel_refs, det_rfn=args.det_refs, shard=(rank, world) if shard_refs else (0, 1),
                          force_collectives=shard_refs and world == 1)
    torch.cuda.synchronize()
    tb = time.perf_counter()
    pipe.build()
    torch.cuda.synchronize()
    build_s = time.perf_counter() - tb            # one-time reference state: detector filters 32 refs, selector cache 64 x 5 (+R1/R2)
    qseed = 0 if shard_refs else rank           # same queries on every rank when the references are sharded
    fulls = synth.imgs_to_tensor(synth.synth_images(4, 480, 640, seed=100 + qseed)).to(dev)
    crops = synth.imgs_to_tensor(synth.synth_images(4, 128, 128, seed=200 + qseed)).to(dev)
    B = max(1, min(32, args.batch))               # sharded references: the batch also shares every collective (round 4)

    # reference-sharded runs: under RCCL the collectives are enqueued on device tensors on the launch stream and are captured into the
    # batch's hipGraph with the kernels around them; under gloo (ranks sharing one GPU) they are host-staged, i.e. eager only
    use_graph = not args.no_graph and not args.serial and (not shard_refs or parallel.backend_name() == "nccl")
    no_fork = args.serial or (use_graph and not args.fork)
    if no_fork:
        ops.SERIAL = True
    # (sharded: every lane's graph enqueues its collectives on its OWN communicator — parallel.lane_groups — so several batches can be in
    # flight; collectives only have to be issued in the same order on every rank WITHIN a communicator, and lane i's replays are)
    lanes = max(1, args.lanes) if use_graph else 1
    if use_graph:
        pipe.capture(lanes=lanes, batch=B)
    main_stream = torch.cuda.current_stream(dev)
    lane_busy = [None] * lanes

    def images_of(i):
        """The 4 synthetic images a step's batch draws: rotated against batch rows AND lanes from step to step, so that a lane's
        static output rows never receive the image they already hold (a skipped replay would fail `parity_vs_reference`)."""
        return [(i * B + b + i // lanes) % 4 for b in range(B)]

    def step(i, eager=False):
        idx = torch.tensor(images_of(i), device=dev)
        qf, qc = fulls[idx], crops[idx]
        if eager or not use_graph:
            return pipe.query(qf, qc)
        lane = i % lanes
        if lane_busy[lane] is not None:
            lane_busy[lane].synchronize()            # the lane's static buffers are free again
        out, stream = pipe.query_graph(qf, qc, lane)
        ev = torch.cuda.Event(); ev.record(stream)
        lane_busy[lane] = ev
        return out

    def drain():
        for ev in lane_busy:
            if ev is not None:
                main_stream.wait_event(ev)

    for i in range(args.warmup):
        step(i)
    drain()
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    coll_log = None
    if shard_refs and args.full:
        # per-collective log of ONE extra query (outside the timed region: logging synchronises the stream around every collective)
        parallel.COLLECTIVE_LOG = []
        step(0, eager=True)
        torch.cuda.synchronize()
        coll_log, parallel.COLLECTIVE_LOG = parallel.COLLECTIVE_LOG, None
        parallel.barrier()
    if not use_graph and args.full:
        ops.PROFILE, ops.PROFILE_HBM = [], {}
    ops.marker(1)
    t0 = time.perf_counter()
    rows = [step(args.warmup + i) for i in range(args.steps)]
    drain()
    ops.marker(2)
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dt = parallel.max_over_ranks(dt, dev)
    last_rows = rows[-1]                             # what the timed path returned in its last step
    if use_graph and args.full:
        # per-kernel HIP events cannot be recorded inside a graph replay: the roofline pass re-runs the same K steps
        # through the eager launch path (identical kernels, shapes and order) right after the timed region
        ops.SERIAL = True                      # branches back to back: per-kernel durations without stream overlap
        step(0, eager=True)
        torch.cuda.synchronize()
        ops.PROFILE, ops.PROFILE_HBM = [], {}
        for i in range(args.steps):
            step(args.warmup + i, eager=True)
        torch.cuda.synchronize()
        ops.SERIAL = no_fork
    prof, ops.PROFILE = ops.PROFILE or [], None
    prof_hbm, ops.PROFILE_HBM = ops.PROFILE_HBM or {}, None
    stages = stage_times(pipe, fulls[0:1], crops[0:1]) if (rank == 0 and not shard_refs and args.full) else None   # (sharded stages hold collectives)
    rows = (parallel.gather_rows(torch.cat(rows, 0), world * args.steps * B) if ((world > 1 or args.force_dist) and not shard_refs and args.full)
            else torch.cat(rows, 0))
    n_queries = args.steps * B if shard_refs else world * args.steps * B
    # latency of ONE query alone: a batch-1 graph on one lane, replays back to back (what a single camera stream would see); measured
    # without and with the query's independent branches (selector levels, refiner feature branches) forked onto side streams
    single_ms, single_detail = None, None
    if rank == 0 and use_graph and not shard_refs and args.full:
        single_detail = {}
        for tag, serial in (("one_stream", True), ("branches_forked", False)):
            ops.SERIAL = serial
            pipe.capture(lanes=1, batch=1)
            for i in range(3):
                pipe.query_graph(fulls[i % 4:i % 4 + 1], crops[i % 4:i % 4 + 1], 0)
            torch.cuda.synchronize()
            ts = time.perf_counter()
            for i in range(10):
                pipe.query_graph(fulls[i % 4:i % 4 + 1], crops[i % 4:i % 4 + 1], 0)
            torch.cuda.synchronize()
            single_detail[tag] = (time.perf_counter() - ts) / 10 * 1e3
        ops.SERIAL = no_fork
        single_ms = min(single_detail.values())
        pipe.capture(lanes=lanes, batch=B)            # back to the timed configuration (the lowp passes re-capture anyway)
        lane_busy[:] = [None] * lanes

    if rank != 0:
        return
    # HBM traffic of the dominant kernel family cannot be read without rocprofv3: it is taken from the committed PMC
    # summary of the same command (profiles/rNN_pmc_conv_traffic.json, newest round first; tools/pmc_conv_traffic.py), else null
    traffic_json, traffic_src = {}, None
    # (the CURRENT round's file or null: an older round's ratio printed beside this round's kernels would be stale — VERDICT r04 weak #4)
    for name in ("r06_pmc_conv_traffic.json",):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                traffic_json = json.load(f)
            traffic_src = "profiles/" + name
            break
        except (OSError, ValueError):
            pass
    tr_note = (f"STATIC, not measured in this run: {traffic_src} (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
               "`bench.py --no-graph`, tools/profile_round.sh); HBM-side bytes per launch = (2 x FETCH_SIZE + WRITE_SIZE) x 1024"
               if traffic_src else "null: no PMC summary of this round's kernels is committed (profiles/r06_pmc_conv_traffic.json)")
    # two MFMA-bound kernel families, both measured with HIP events around every launch (serialised eager re-run of the same
    # steps after the graph-replay timed region when graphs are used):
    #   conv      conv_igemm / conv_patch / corr_patch (split launches finish inside the kernel); executed = direct-form FLOPs
    #   winograd  wino_conv3x3_kernel (own VGG trunk + the conv layers g6d_conv_igemm routes to it); the matrix cores
    #             execute 1/2.25 of the direct-form FLOPs: `achieved` / `frac` are the EXECUTED rate, the direct-form equivalent
    #             is given beside it
    how = "HIP events around every launch, " + ("serialised eager re-run of the same steps after the graph-replay timed region"
                                                if use_graph else "inside the timed region")
    fams = {}
    for key, sel, kname in (("conv", lambda p: not p[3].startswith("wino3x3") and not p[3].startswith("conv16"),
                             "g6d_conv_igemm family: conv_igemm / conv_patch / corr_patch kernels (fp32 v_mfma_f32_32x32x2_f32); split "
                             "launches add their partial tiles inside the kernel"),
                            ("split16", lambda p: p[3].startswith("conv16"),
                             "conv16w_kernel<3, *> / corr16_kernel<3> (g6d_conv16_direct_multi, g6d_corr16_multi, math mode 3): direct convolution / "
                             "correlation on the 16-bit matrix cores with every operand an fp16 hi / lo pair — fp32-class results, THREE "
                             "v_mfma_f32_32x32x16_f16 per product: the VGG trunks of detector pyramid and refiner crops, the detector's 15x15 and 7x7 "
                             "correlations, the selector's product layers and InstanceNorm stacks"),
                            ("winograd", lambda p: p[3].startswith("wino3x3"),
                             "Winograd kernels on the fp32 matrix cores: wino_conv3x3_kernel (F(2x2,3x3), v_mfma_f32_32x32x2_f32) and wino43_kernel "
                             "(F(4x4,3x3), v_mfma_f32_16x16x4_f32): own VGG trunks + the stride-1 3x3 / 3x3x3 layers g6d_conv_igemm routes to "
                             "them + the detector's 15x15 correlation; the detector's pyramid runs each layer as one launch")):
        pp = [p for p in prof if sel(p)]
        if not pp:
            continue
        # (split16: the launches are booked with their direct-form FLOPs; the matrix cores execute three times that)
        fl = sum(p[0] for p in pp) * (3.0 if key == "split16" else 1.0)
        ms = sum(p[1].elapsed_time(p[2]) for p in pp)
        ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        tj = traffic_json if key == "conv" else traffic_json.get("winograd_family" if key == "winograd" else "split16_family", {})
        peak = LOWP_MFMA_PEAK_TFLOPS if key == "split16" else FP32_MFMA_PEAK_TFLOPS
        fams[key] = {"bound": "mfma", "kernel": kname, "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                     "frac": ach / peak, "traffic": tj.get("hbm_bytes_per_launch"), "traffic_source": tr_note if tj else None,
                     "launches_per_step": len(pp) / args.steps, "launches_per_query": len(pp) / args.steps / B,
                     "gflop_per_launch": fl / len(pp) / 1e9, "avg_launch_ms": ms / len(pp), "ms_per_step": ms / args.steps,
                     "ms_per_query": ms / args.steps / B, "measured": how}
        # algorithmic bytes of a launch = every operand once (input, multiplier map, filters, output); traffic / that = re-reads
        ab = sum(p[4] for p in pp if len(p) > 4) / len(pp)
        fams[key]["algorithmic_bytes_per_launch"] = ab
        if tj.get("hbm_bytes_per_launch") and ab > 0:
            fams[key]["traffic_over_algorithmic"] = tj["hbm_bytes_per_launch"] / ab
        if key == "conv":
            fams[key]["conv_ms_per_step"] = ms / args.steps
        elif key == "split16":
            fams[key].update(flops_counted="EXECUTED on the 16-bit matrix cores: 3 x the direct-form FLOPs (hi x hi + hi x lo + lo x hi)",
                             achieved_direct_form_equivalent=ach / 3.0, gflop_direct_form_per_step=fl / 3.0 / args.steps / 1e9,
                             sustained_mfma_note="a bare stream of v_mfma_f32_32x32x16_f16 on random operands sustains 1780 TFLOP/s on this chip "
                                                 "(0.71 of the 2500 nominal; small-integer operands 2250-2400: the clock follows the power the "
                                                 "operand bits draw) — tools/ubench/mfma16_peak.hip, profiles/r06_mfma16_peak.md")
        else:
            # per-launch factor: the F(2x2,3x3) kernel executes direct-form / 2.25 multiplications, the F(4x4,3x3) kernel direct-form / 4
            direct = sum((p[5] if len(p) > 5 else 2.25 * p[0]) for p in pp)
            by = {}
            for tag, sel43 in (("F(2x2,3x3) wino_conv3x3_kernel, direct / 2.25", False), ("F(4x4,3x3) wino43_kernel, direct / 4", True)):
                qq = [p for p in pp if p[3].startswith("wino3x3 F43") == sel43]
                if qq:
                    f_, m_ = sum(p[0] for p in qq), sum(p[1].elapsed_time(p[2]) for p in qq)
                    by[tag] = {"launches_per_step": len(qq) / args.steps, "ms_per_step": m_ / args.steps, "gflop_executed_per_step": f_ / args.steps / 1e9,
                               "achieved": f_ / (m_ * 1e-3) / 1e12, "frac": f_ / (m_ * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS}
            fams[key].update(flops_counted="EXECUTED in the Winograd domain, per launch: direct-form / 2.25 on the F(2x2,3x3) kernel (selector and "
                                           "refiner InstanceNorm stacks, reference-side trunks), direct-form / 4 on the F(4x4,3x3) kernel (detector "
                                           "pyramid trunk, 15x15 correlation, refiner volume layers)",
                             by_transform=by, achieved_direct_form_equivalent=direct / (ms * 1e-3) / 1e12,
                             gflop_direct_form_per_step=direct / args.steps / 1e9)
    dominant = max(fams, key=lambda k: fams[k]["ms_per_step"]) if fams else None
    result = {
        "metric": "query images/sec (detect+select+3x refine), 64 ref views",
        "value": n_queries / dt, "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "strong" if shard_refs else "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "arithmetic": "fp32 inputs, accumulation, statistics and results.  Since round 6 the VGG trunks of detector / refiner, the detector's 15x15 and 7x7 "
                      "correlations and the selector's 3x3 stacks form every product from fp16 hi / lo PAIRS of both fp32 operands on the 16-bit matrix "
                      "cores (three v_mfma_f32_32x32x16_f16 per product, fp32 accumulators; <= 2e-6 of a layer's output range against the float64 "
                      "convolution of the fp32 operands: below the fp32 Winograd kernels they replaced); everything else on the fp32 matrix cores / "
                      "vector ALUs.  Module switches restore round 5's all-fp32-core path (INTEGRATION.md section 4)",
        "batch": B, "images_per_step": B, "single_query_ms": single_ms, "single_query_ms_detail": single_detail,
        "config": {"workload": f"full tensor pipeline: detector 480x640 query vs {args.det_refs} refs (4 scales) + selector "
                               f"128x128 crop vs {args.sel_refs} refs x 5 rotations + 3 refiner steps (6 refs, 32^3 volume); "
                               "seeded synthetic weights", "sharding": (f"selector and detector references sharded x{world} (RCCL all-reduce/all-gather), refiner replicated" if shard_refs
                                else f"query-replicas x{world}"),
                   "launch": (f"hipGraph replay (1 graph = 1 batch of {B} queries sharing every launch{', branches forked' if args.fork else ''}), "
                              f"{lanes} batches in flight on separate streams") if use_graph else f"eager, batches of {B}"},
    }
    if dominant:
        result["roofline"] = dict(fams[dominant], family=dominant,
                                  note="dominant kernel family by serialised time; the other family follows as roofline_<name>")
        for k, v in fams.items():
            if k != dominant:
                result["roofline_" + k] = v
    # HBM-bound kernels of the path (K5/K6 scan, K12/K13 volume, K15 FC): algorithmic bytes / HIP-event time
    hbm = {}
    for name, recs in prof_hbm.items():
        if name.endswith("_small"):
            continue
        t_ms = sum(r[1].elapsed_time(r[2]) for r in recs)
        nb = sum(r[0] for r in recs)
        hbm[name] = {"launches_per_step": len(recs) / args.steps, "mbytes_per_launch": nb / len(recs) / 1e6,
                     "avg_launch_us": t_ms / len(recs) * 1e3, "achieved_GBps": nb / (t_ms * 1e-3) / 1e9,
                     "frac_of_8TBps": nb / (t_ms * 1e-3) / 8e12}
    if args.full:
        result["hbm_kernels"] = hbm
        result["stages_ms"] = stages
    result["ranks_seen"], result["backend"] = ranks_seen, parallel.backend_name()
    if coll_log is not None:
        kinds = {}
        for kind, nb, sec, enq in coll_log:
            k = kinds.setdefault(kind, {"count": 0, "bytes": 0, "us": 0.0, "enq": 0.0})
            k["count"] += 1; k["bytes"] += nb; k["us"] += sec * 1e6; k["enq"] += enq * 1e6
        result["collectives_per_query"] = {
            "total": len(coll_log) / B, "per_batch": len(coll_log), "batch": B, "total_us_per_batch": sum(c[2] for c in coll_log) * 1e6,
            "captured": bool(use_graph), "enqueue_us_mean": sum(c[3] for c in coll_log) * 1e6 / max(1, len(coll_log)),
            "by_kind": {k: {"count": v["count"], "mean_bytes": v["bytes"] / v["count"], "mean_us": v["us"] / v["count"],
                            "mean_enqueue_us": v["enq"] / v["count"]} for k, v in kinds.items()},
            "how": "one extra EAGER batch with a stream synchronisation around every data-path collective (rank 0's view; selector 9 + "
                   "detector 1 per batch of queries): mean_us = enqueue + execution on an idle stream, mean_enqueue_us = host time of the "
                   "call alone; `captured`: the timed region replays ONE hipGraph per batch that holds the kernels AND the collectives; "
                   + ("RCCL: enqueued on device tensors, no host staging" if parallel.backend_name() == "nccl" else
                      "gloo: every collective is staged through host memory (ranks share one GPU on this lease; RCCL refuses that)")}
    if shard_refs and world == 1 and args.full:
        # the forced-collective path against the plain one on the same four images (same kernels apart from the InstanceNorm
        # finalisation, which moves from the producers' last blocks into g6d_stats_finalize behind the all-reduce)
        idx4 = torch.arange(4, device=dev)
        with torch.no_grad():
            sh_rows = pipe.query(fulls[idx4], crops[idx4])
            for net in (pipe.selector, pipe.detector):
                net.set_shard(rank, world, force_collectives=False)
            un_rows = pipe.query(fulls[idx4], crops[idx4])
            for net in (pipe.selector, pipe.detector):
                net.set_shard(rank, world, force_collectives=True)
        dd = (sh_rows - un_rows).abs()
        result["sharded_vs_unsharded"] = {"max_abs_diff_row": float(dd.max()), "max_rel_diff_row": float((dd / un_rows.abs().clamp(min=1.0)).max()),
                                          "ref_idx_equal": bool((sh_rows[:, 3] == un_rows[:, 3]).all()),
                                          "what": "world-size-1 RCCL group, force_collectives: 9 selector + 1 detector collectives per batch, "
                                                  "rows of 4 queries vs the same pipeline without collectives"}
    result["build_s"] = {"value": build_s, "what": "TensorPipeline.build: detector reference filters + selector reference cache "
                                                   "(trunk over 32 + 320 crops, R1/R2 sums, viewpoint embedding), incl. first-use "
                                                   "library initialisation; reference: 0.57 s + 9.8 s on 8 CPU threads (BASELINE.md §2)"}
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "rows.npy"), last_rows.cpu().numpy().astype(np.float32))
    if not args.full:
        print(json.dumps(result))
        return
    got_rows = rows.cpu()
    # fp32 row of every synthetic image (rank 0's rows, headline lane count): side passes with another lane count draw the images in
    # another order, so they are compared per image
    row32 = {}
    for i in range(min(args.steps, got_rows.shape[0] // B)):
        for b, j in enumerate(images_of(args.warmup + i)):
            row32.setdefault(j, got_rows[i * B + b])
    gpath = os.path.join(ROOT, "tests", "golden", "pipeline_rows.npz")

    # ---- reduced-precision speed modes (BASELINE configs[2] "bf16", configs[4] "fp16 MFMA convs"): separately graded, never
    #      the headline.  Same pipeline, same launch mode, matrix-core operands rounded to bf16 / fp16 in the conv / correlation
    #      kernels (fp32 accumulation, fp32 InstanceNorm statistics, fp32 trunk).
    lowp, headline_lanes = {}, lanes
    # name -> (matrix-core operand type of the enclosing context, selector override, selector keep-list (None = cfg default), refiner override)
    LOWP_SCHEMES = {
        "fp16": ("fp16", None, None, None),            # BASELINE configs[4]: every stage on fp16 operands (selector trunk / tail kept on fp32)
        "fp16ref32": ("fp16", None, None, "fp32"),     # detector + selector fp16, refiner fp32: the scheme that holds the all-rows bar
        "bf16": ("bf16", None, None, None),            # BASELINE configs[2] as it reads: every stage on bf16 operands
        "bf16mix": ("bf16", "fp16", None, None),       # detector + refiner bf16, selector fp16
        "fp16all": ("fp16", None, (), None),           # nothing kept on fp32 anywhere
        "fp16sel32": ("fp16", "fp32", None, None),
    }
    SCHEME_TEXT = {
        "fp16": "detector, selector, refiner on fp16 operands; selector parts on fp32 operands: {kept} (profiles/r05_lowp_selector_sensitivity.md)",
        "fp16ref32": "detector and selector on fp16 operands (selector parts on fp32: {kept}), refiner on fp32 operands — every part of the synthetic "
                     "refiner ALONE moves the pose heads by 0.6-1.6e-2 in fp16 (profiles/r06_lowp_refiner_sensitivity.md), so the all-rows bar needs it on fp32",
        "bf16": "detector, selector, refiner on bf16 operands (selector parts on fp32: {kept}) — BASELINE configs[2] as it reads",
        "bf16mix": "detector and refiner bf16, selector fp16 with {kept} on fp32 operands",
        "fp16all": "every matrix-core launch on fp16 operands, nothing kept on fp32",
        "fp16sel32": "detector fp16, selector fp32, refiner fp16"}

    def set_scheme(name):
        mode, sel_mode, keep, ref_mode = LOWP_SCHEMES.get(name, (name, None, None, None))
        pipe.selector.cfg["math_mode"] = sel_mode
        pipe.selector.cfg["lowp_keep_fp32"] = pipe.selector.default_cfg["lowp_keep_fp32"] if keep is None else keep
        pipe.refiner.cfg["math_mode"] = ref_mode
        return mode

    def reset_scheme():
        pipe.selector.cfg["math_mode"] = None
        pipe.selector.cfg["lowp_keep_fp32"] = pipe.selector.default_cfg["lowp_keep_fp32"]
        pipe.refiner.cfg["math_mode"] = None

    # the gate queries of the reduced-precision modes (gen6d_amd/bars.py): the 4 bench queries + 16 HELD-OUT queries nothing was tuned on
    # (tests/golden/pipeline_rows_heldout.npz: rows and logits of the reference's own modules), with the fp32 path's rows of the same queries
    from gen6d_amd import bars
    gate = {}
    try:
        if (args.sel_refs, args.det_refs) == (64, 32) and world == 1 and not shard_refs:
            for tag, n, fs, cs, fn in (("bench4", 4, 100, 200, "pipeline_rows.npz"), ("heldout16", 16, 300, 400, "pipeline_rows_heldout.npz")):
                gp = os.path.join(ROOT, "tests", "golden", fn)
                if not os.path.exists(gp):
                    continue
                g_ = np.load(gp)
                gf = fulls if n == 4 else synth.imgs_to_tensor(synth.synth_images(n, 480, 640, seed=fs)).to(dev)
                gc = crops if n == 4 else synth.imgs_to_tensor(synth.synth_images(n, 128, 128, seed=cs)).to(dev)
                with torch.no_grad():
                    r32_, l32_ = pipe.query(gf, gc).cpu(), pipe.selector.compute_view_point_feats(gc)[0].cpu()
                gate[tag] = (gf, gc, torch.from_numpy(g_["rows"]).float(), torch.from_numpy(g_["logits"]).float(), r32_, l32_)
            if "heldout16" in gate:
                _, _, gr_, gl_, r32_, l32_ = gate["heldout16"]
                e_ = bars.row_errors(r32_, gr_)
                result["parity_vs_reference_heldout"] = {
                    "rows_checked": 16, "ref_idx_equal": e_["ref_idx_equal"], "max_rel_diff_row": e_["max_rel"],
                    "logits_max_abs_diff": float((l32_ - gl_).abs().max()), "argmax_equal": bool((l32_.argmax(1) == gl_.argmax(1)).all()),
                    "ok": bool(e_["ref_idx_equal"] and e_["max_rel"] <= bars.FP32_REL and float((l32_ - gl_).abs().max()) <= bars.FP32_REL),
                    "source": "tests/golden/pipeline_rows_heldout.npz: 16 more synthetic queries (frames seed 300, crops seed 400) through the reference's "
                              "own modules (tests/golden/make_golden_r06.py); fp32 path, eager batch of 16"}
    except Exception as e:
        result.setdefault("side_leg_errors", {})["gate_queries"] = f"{type(e).__name__}: {e}"[:600]

    try:
        modes = [m for m in args.lowp.split(",") if m] if (use_graph and world == 1 and not shard_refs) else []
        # the first re-captured pass after the serialised eager roofline pass measures ~15 % low whatever its type (bf16 first: 169 /
        # fp16 205; fp16 first: fp16 low, bf16 205): one throwaway pass of the first mode precedes the reported ones
        if modes:
            lanes = max(1, args.lowp_lanes)               # (step / images_of read `lanes` when they run)
        LOWP_PEAK_TFLOPS = 2500.0                          # dense 16-bit MFMA peak (MI355X_MICROARCH.md; AMD's 5 PFLOP/s figure is 2:1 sparse)
        gold_npz = np.load(gpath) if ((args.sel_refs, args.det_refs) == (64, 32) and os.path.exists(gpath)) else None
        for pi, mode_name in enumerate(modes[:1] + modes):
            mode = set_scheme(mode_name)
            with ops.math_mode(mode):
                pipe.capture(lanes=lanes, batch=B)
            lane_busy[:] = [None] * lanes
            for i in range(args.warmup):
                step(i)
            drain(); torch.cuda.synchronize()
            nl = 3 * args.steps                            # side measurement: three times the headline's queries for a steadier number
            t1 = time.perf_counter()
            lrows = [step(args.warmup + i) for i in range(nl)]
            drain(); torch.cuda.synchronize()
            ldt = time.perf_counter() - t1
            lrows = torch.cat(lrows[:args.steps], 0).cpu()
            entry = {"dtype": mode_name, "value": nl * B / ldt, "unit": "images/s", "ms_per_step": ldt / nl * 1e3, "queries": nl * B, "batch": B,
                     "lanes": lanes}
            kept = ", ".join(pipe.selector.cfg["lowp_keep_fp32"]) or "nothing"
            entry["scheme"] = SCHEME_TEXT.get(mode_name, mode_name).format(kept=kept)
            entry["default_scheme"] = mode_name == "fp16"
            if pi > 0:
                # roofline of the mode: serialised eager pass of the same steps with HIP events around every MFMA-family launch
                ops.SERIAL = True
                with ops.math_mode(mode), torch.no_grad():
                    step(0, eager=True); torch.cuda.synchronize()
                    ops.PROFILE, ops.PROFILE_HBM = [], {}
                    for i in range(args.steps):
                        step(args.warmup + i, eager=True)
                    torch.cuda.synchronize()
                    lp, ops.PROFILE, ops.PROFILE_HBM = ops.PROFILE, None, None
                    # the ALL-ROWS bar (gen6d_amd/bars.py) on the 4 bench queries and the 16 held-out ones, eager, in this mode
                    gate_out = {}
                    for tag, (gf, gc, gr_, gl_, r32_, l32_) in gate.items():
                        mrows, mlog = pipe.query(gf, gc).cpu(), pipe.selector.compute_view_point_feats(gc)[0].cpu()
                        gate_out[tag] = bars.lowp_all_rows(mrows, gr_, r32_, mlog, gl_)
                ops.SERIAL = no_fork
                # (pair launches of parts kept on the fp32 path: three 16-bit MFMAs per product)
                fl = sum(p[0] * (3.0 if p[3].startswith("conv16x3") else 1.0) for p in lp); ms = sum(p[1].elapsed_time(p[2]) for p in lp)
                wino = [p for p in lp if p[3].startswith("wino3x3")]
                c16 = [p for p in lp if p[3].startswith("conv16")]
                entry["roofline"] = {"bound": "mfma", "achieved": fl / (ms * 1e-3) / 1e12, "peak": LOWP_PEAK_TFLOPS, "unit": "TFLOP/s",
                                     "frac": fl / (ms * 1e-3) / 1e12 / LOWP_PEAK_TFLOPS, "traffic": None,
                                     "kernel": "all MFMA-family launches of a step (conv16 direct implicit-GEMM kernels on 16-bit activations, 16-bit "
                                               "Winograd conv family, corr16_patch, conv_igemm / conv_patch with 16-bit operands)",
                                     "flops_counted": "EXECUTED (Winograd launches: direct-form / 2.25)",
                                     "mfma_ms_per_step": ms / args.steps, "gflop_executed_per_step": fl / args.steps / 1e9,
                                     "winograd_share_of_ms": sum(p[1].elapsed_time(p[2]) for p in wino) / ms if ms > 0 else None,
                                     "conv16_direct": ({"ms_per_step": sum(p[1].elapsed_time(p[2]) for p in c16) / args.steps,
                                                        "achieved": sum(p[0] * (3.0 if p[3].startswith("conv16x3") else 1.0) for p in c16) / (sum(p[1].elapsed_time(p[2]) for p in c16) * 1e-3) / 1e12,
                                                        "launches_per_step": len(c16) / args.steps} if c16 else None),
                                     "measured": "HIP events around every launch, serialised eager re-run of the same steps"}
                if gate_out:
                    entry["all_rows"] = gate_out
                    entry["ok"] = bool(all(v["ok"] for v in gate_out.values()))
                    worst = max(gate_out.values(), key=lambda v: v["logits"]["worst_err_over_own_margin"])["logits"]
                    entry["selector_logits"] = {"max_abs_err": max(v["logits"]["max_abs_err"] for v in gate_out.values()),
                                                "worst_err_over_own_margin": worst["worst_err_over_own_margin"], "bar": bars.LOWP_MARGIN_FRAC,
                                                "ok": bool(all(v["ok_logits"] for v in gate_out.values())),
                                                "argmax_equal": bool(all(v["logits"]["argmax_equal"] for v in gate_out.values())),
                                                "queries": sum(v["queries"] for v in gate_out.values())}
            if gold_npz is not None:
                gold = torch.from_numpy(gold_npz["rows"]).float()
                ref = torch.stack([gold[j] for i in range(args.steps) for j in images_of(args.warmup + i)])
                r32 = torch.stack([row32[j] for i in range(args.steps) for j in images_of(args.warmup + i)])
                d = (lrows - ref).abs()
                entry["parity_vs_reference"] = {
                    "what": "the timed rows of this mode (graph replay) against the reference's golden rows of the 4 bench queries",
                    "ref_idx_equal": bool((lrows[:, 3].long() == ref[:, 3].long()).all()),
                    "detection_cell_px": float(d[:, 0:2].max()), "max_abs_diff_row": float(d.max()),
                    "max_rel_diff_row": float((d / ref.abs().clamp(min=1.0)).max()),
                    "vs_fp32_path_max_rel": float(((lrows - r32).abs() / r32.abs().clamp(min=1.0)).max())}
            if pi > 0:
                lowp[mode_name] = entry
        reset_scheme()
        if lowp:
            # the scheme to use: the fastest one whose all-rows bar holds on the 4 bench + 16 held-out queries (None: none of the measured ones)
            okd = [k for k, v in lowp.items() if isinstance(v, dict) and v.get("ok")]
            lowp["recommended"] = max(okd, key=lambda k: lowp[k]["value"]) if okd else None
            result["lowp"] = lowp
        lanes = headline_lanes
    except Exception as e:                 # a side measurement must not take the headline line with it
        result.setdefault("side_leg_errors", {})["lowp"] = f"{type(e).__name__}: {e}"[:600]
    finally:
        reset_scheme()
        lanes = headline_lanes
        if lowp:
            result["lowp"] = lowp

    # ---- reference-feature caching: the refiner's 6 reference crops per step skip the trunk + feature net when
    #      their (view, angle bucket) key repeats; in this workload the canned crops repeat in every step of every query (hit rate 1 after
    #      the first step), so this is the upper bound of what the cache buys.  Side number: the headline stays uncached.
    try:
        if use_graph and world == 1 and not args.no_cached and not shard_refs:
            pipe.capture(lanes=lanes, batch=B, cached_refs=True)
            lane_busy[:] = [None] * lanes
            for i in range(args.warmup):
                step(i)
            drain(); torch.cuda.synchronize()
            nl = 2 * args.steps
            t1 = time.perf_counter()
            crows = [step(args.warmup + i) for i in range(nl)]
            drain(); torch.cuda.synchronize()
            cdt = time.perf_counter() - t1
            crows = torch.cat(crows[:args.steps], 0).cpu()
            r_ = pipe.ref_dev
            def t_step(cached):
                qc = crops[0:1]
                fn = lambda: pipe.refiner._step(qc, r_["Ks_in"][0], pipe.iter_poses[0][0], r_["ref_imgs"][0], r_["ref_Ks"][0], r_["ref_poses"][0],
                                                ref_feats=pipe.ref_feats if cached else None)
                with torch.no_grad():
                    fn(); fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(); e0.record()
                    for _ in range(5): fn()
                    e1.record(); torch.cuda.synchronize()
                return e0.elapsed_time(e1) / 5
            result["cached"] = {
                "value": nl * B / cdt, "unit": "images/s", "ms_per_step": cdt / nl * 1e3, "queries": nl * B, "hit_rate": 1.0,
                "what": "same launch mode with the refiner's reference-crop features cached per (view, in-plane angle bucket): only the query "
                        "crop passes the trunk + feature net in each of the 3 steps; upper bound (every key repeats in this workload)",
                "refiner_step_ms_single_query": {"uncached": t_step(False), "cached": t_step(True)},
                "rows_vs_uncached_max_rel": float(((crows - got_rows[:crows.shape[0]]).abs() / got_rows[:crows.shape[0]].abs().clamp(min=1.0)).max())}
    except Exception as e:                 # a side measurement must not take the headline line with it
        result.setdefault("side_leg_errors", {})["cached"] = f"{type(e).__name__}: {e}"[:600]

    try:
        if not args.no_chained and world == 1 and rank == 0 and not shard_refs:
            # the estimator-level path: the crop fed to the selector comes from the detection, the refiner inputs from the pose of
            # the previous stage (bench headline: canned crops / poses)
            from gen6d_amd.estimator import Gen6DEstimator
            from gen6d_amd.synth_db import SyntheticDatabase
            tb = time.perf_counter()
            db = SyntheticDatabase(n_views=88, size=(480, 640), focal=560.0)
            # the refiner of this leg has its pose heads damped towards the identity update (synth.damp_refiner_head), as a trained
            # refiner's are: with the seeded random heads a single grey level of a crop moves the pose by 1e-2 and step-to-step
            # comparisons say nothing.  Same layers, same launches, same cost.
            from gen6d_amd.network import name2network
            ref_d = name2network["refiner"]({"name": "refiner_synth_damped"})
            ref_d.load_state_dict(synth.damp_refiner_head(pipe.state_dicts["refiner"]))
            ref_d.to(dev).eval()
            est = Gen6DEstimator({"ref_view_num": args.sel_refs, "det_ref_view_num": args.det_refs, "refine_iter": 3},
                                 modules={"detector": pipe.detector, "selector": pipe.selector, "refiner": ref_d})
            est.build(db, "all")
            torch.cuda.synchronize()
            cbuild = time.perf_counter() - tb
            _, qids = db.get_split("all")
            imgs = [torch.from_numpy(db.get_image(i)).to(dev) for i in qids[:8]]
            Ks = [db.get_K(i) for i in qids[:8]]
            n_c = max(3 * args.steps, 24)
            qi = [imgs[i % 8] for i in range(n_c + lanes)]
            qk = [Ks[i % 8] for i in range(n_c + lanes)]
            chain = est.device_chain()
            clanes = min(lanes, 3)
            cb = min(B, args.chain_batch, 8)  # queries per captured chain graph (they share every launch)
            n_c = max(n_c, 6 * cb * clanes)
            qi = [imgs[i % 8] for i in range(n_c)]
            qk = [Ks[i % 8] for i in range(n_c)]
            chain.predict_many(qi[:cb * clanes], qk[:cb * clanes], clanes, batch=cb)              # capture + warm-up
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = chain.predict_many(qi[:n_c], qk[:n_c], clanes, batch=cb)
            cdt = time.perf_counter() - t1
            _, inter_h = est.predict(imgs[0], Ks[0])                      # the host-driven path (numpy pose algebra, 5+ syncs per query)
            _, inter_d = est.predict_device(imgs[0], Ks[0])               # the same query through the eager device chain
            # every refine step of the device chain on the HOST path's input pose of that step (the chain's tracking entry: pose_init,
            # one step): per-step agreement without the free-running accumulation — the crops are uint8 (rint of the bilinear warp, as
            # cv2 returns them), so a 1e-6 pose difference flips single grey levels of the next crops and the randomly initialised
            # feature net answers a flipped grey level with 1e-4 ... 1e-3 on the pose even behind damped heads
            forced = []
            K0 = torch.from_numpy(np.ascontiguousarray(Ks[0], dtype=np.float32)).to(dev)
            for k_ in range(len(inter_h["refine_poses"]) - 1):
                o_ = chain.query(imgs[0], K0, pose_init=torch.from_numpy(np.ascontiguousarray(inter_h["refine_poses"][k_], dtype=np.float32)), refine_iter=1)
                forced.append(float(np.abs(o_["pose"].cpu().numpy() - inter_h["refine_poses"][k_ + 1]).max()))
            result["chained"] = {"value": n_c / cdt, "unit": "images/s", "ms_per_query": cdt / n_c * 1e3, "queries": n_c, "lanes": clanes, "batch": cb,
                                 "database": "procedural sphere, 66 reference views 480x640, 64/32 selected; build incl. rendering "
                                             f"{cbuild:.1f} s", "finite": bool(all(np.isfinite(p).all() for p, _ in res)),
                                 "vs_host_driven_predict": {
                                     "same_viewpoint": bool(inter_d["sel_ref_idx"] == inter_h["sel_ref_idx"]),
                                     "pose_from_detection_and_selection_maxabs": float(np.abs(inter_d["refine_poses"][0] - inter_h["refine_poses"][0]).max()),
                                     "after_refine_step_maxabs": [float(np.abs(inter_d["refine_poses"][i] - inter_h["refine_poses"][i]).max())
                                                                  for i in range(1, len(inter_h["refine_poses"]))],
                                     "final_pose_maxabs": float(np.abs(inter_d["refine_poses"][-1] - inter_h["refine_poses"][-1]).max()),
                                     "each_step_on_the_host_paths_input_pose_maxabs": forced, "each_step_ok": bool(max(forced) <= 1e-4),
                                     "graph_replay_vs_eager_chain_maxabs": float(np.abs(res[0][0] - inter_d["refine_poses"][-1]).max()),
                                     "bar": 1e-4, "note": "pose heads damped towards the identity (synth.damp_refiner_head); `each_step_...` holds the bar (every step on "
                                     "identical inputs); the free-running `after_refine_step_maxabs` grows from step 2 on because uint8 crops turn a 1e-6 pose "
                                     "difference into flipped grey levels, which the random feature net amplifies (the graph-replayed batch differs from the "
                                     "eager single query by the same mechanism: other split choices, 1e-6, flipped pixels)"}}
    except Exception as e:                 # a side measurement must not take the headline line with it
        result.setdefault("side_leg_errors", {})["chained"] = f"{type(e).__name__}: {e}"[:600]

    try:
        if not args.no_sweep and world == 1 and use_graph and not shard_refs and (args.sel_refs, args.det_refs) == (64, 32):
            sw = ref_sweep(dev, B, headline_lanes, max(10, args.steps // 2), max(2, args.warmup // 2))
            sw["64x5"] = {"workload": "the headline of this line", "value": result["value"], "unit": "images/s",
                          "roofline": {"winograd": {"achieved_TFLOPs_executed": fams.get("winograd", {}).get("achieved"),
                                                    "frac_of_fp32_mfma_peak": fams.get("winograd", {}).get("frac")}}}
            result["sweep"] = sw
            ops.SERIAL = no_fork
    except Exception as e:                 # a side measurement must not take the headline line with it
        result.setdefault("side_leg_errors", {})["sweep"] = f"{type(e).__name__}: {e}"[:600]
    finally:
        ops.SERIAL = no_fork

    def row_diff(got, ref):
        """Row layout: position(2, px), scale, ref_idx, angle, quaternion(4), offset(2), log2-scale."""
        d = (got - ref).abs()
        return {"ref_idx_equal": bool(int(got[3]) == int(ref[3])), "max_abs_diff_row": float(d.max()),
                "max_rel_diff_row": float((d / ref.abs().clamp(min=1.0)).max())}

    # parity of EVERY timed row (graph replay, `lanes` queries in flight) against the reference's own modules: the rows of
    # the four synthetic queries were produced from /root/reference by tests/golden/make_golden_r02.py (pipeline_rows.npz)
    # (reference-sharded runs draw the same four queries on every rank: their rows are held to the same golden rows — the sharded sums
    # differ from the unsharded ones by fp reassociation only)
    default_cfg = (args.sel_refs, args.det_refs) == (64, 32)
    if default_cfg and os.path.exists(gpath):
        gold = torch.from_numpy(np.load(gpath)["rows"]).float()
        worst = {"ref_idx_equal": True, "max_abs_diff_row": 0.0, "max_rel_diff_row": 0.0}
        per_rank = args.steps * B
        for i in range(got_rows.shape[0]):
            r_i, s_i = divmod(i, per_rank)             # (rank, row): every rank >0 draws its own query seeds -> rank 0 only
            if r_i != 0:
                break
            dct = row_diff(got_rows[i], gold[images_of(args.warmup + s_i // B)[s_i % B]])
            worst = {"ref_idx_equal": worst["ref_idx_equal"] and dct["ref_idx_equal"],
                     "max_abs_diff_row": max(worst["max_abs_diff_row"], dct["max_abs_diff_row"]),
                     "max_rel_diff_row": max(worst["max_rel_diff_row"], dct["max_rel_diff_row"])}
        worst["rows_checked"] = min(got_rows.shape[0], per_rank)
        worst["source"] = "tests/golden/pipeline_rows.npz (outputs of the reference's own PyTorch-CPU modules)"
        result["parity_vs_reference"] = worst

    try:
        if world == 1 and not args.no_cpu_baseline and not shard_refs:
            # BASELINE.md §3 protocol: threads = physical cores, 1 warm-up + min of >= 3 runs, torch.std share split out
            from oracle import gen6d_oracle as GO
            from oracle import pipeline_oracle as PO
            try:
                import psutil
                cores = psutil.cpu_count(logical=False) or torch.get_num_threads()
            except ImportError:
                cores = torch.get_num_threads()
            st = PO.build_state(pipe.state_dicts, pipe.det_refs, pipe.sel_case)
            iter_poses = [p.cpu() for p in pipe.iter_poses]
            j0 = images_of(args.warmup)[0]                # the image of the first timed row
            qf, qc = fulls[j0:j0 + 1].cpu(), crops[j0:j0 + 1].cpu()

            def one_run():
                GO.TIMERS = {}
                stage_s = {}
                t1 = time.perf_counter()
                r_, _ = PO.query(pipe.state_dicts, st, pipe.ref_case, iter_poses, qf, qc, stage_s)
                return time.perf_counter() - t1, stage_s, GO.TIMERS.get("refiner_std", 0.0), r_

            # The oracle is a PORT of the reference's PyTorch-CPU path (the reference itself is not on this box).  torch's CPU kernels
            # do not scale to every core of a large host (round 2: 128 threads were SLOWER than 8), so the baseline is the best thread
            # count of a short sweep: one run per candidate after a common warm-up, then min of `--cpu-reps` runs at the winner.
            cands = [args.cpu_threads] if args.cpu_threads > 0 else sorted({t for t in (8, 16, 32, 64, cores) if t <= cores})
            torch.set_num_threads(cands[-1])
            one_run()                                     # warm-up (allocator, oneDNN primitive caches)
            sweep = {}
            for t in cands:
                torch.set_num_threads(t)
                sweep[t] = one_run()[0]
            best_t = min(sweep, key=sweep.get)
            torch.set_num_threads(best_t)
            runs, stage_runs, std_runs = [], [], []
            row = None
            for rep in range(max(1, args.cpu_reps - 1)):
                dt_rep, stage_s, std_s, row = one_run()
                runs.append(dt_rep); stage_runs.append(stage_s); std_runs.append(std_s)
            GO.TIMERS = None
            best = min(range(len(runs)), key=lambda i: runs[i])
            cpu_dt = min(runs[best], sweep[best_t])
            result["cpu_baseline"] = {
                "value": 1.0 / cpu_dt, "unit": "images/s", "cores": best_t, "kind": "port",
                "sample": f"1 query of the same workload (image {j0}) through oracle/ (torch CPU fp32, a port of the reference's PyTorch-CPU "
                          f"path: the reference itself is not on this box), reference state prebuilt; 1 warm-up, one run per thread count "
                          f"{cands}, then min of {len(runs) + 1} runs at the best count ({best_t} of {cores} physical cores)",
                "seconds": cpu_dt, "thread_sweep_s": {str(k): v for k, v in sweep.items()}, "physical_cores": cores, "runs": len(runs) + 1,
                "stages_s": stage_runs[best], "torch_std_s": std_runs[best],
                "value_without_torch_std": 1.0 / max(cpu_dt - std_runs[best], 1e-9),
                "note": "reported baseline, not the target: the GPU/CPU ratio says nothing about kernel quality (see roofline)"}
            result["parity_vs_cpu"] = row_diff(got_rows[0], row[0])
    except Exception as e:                 # a side measurement must not take the headline line with it
        result.setdefault("side_leg_errors", {})["cpu_baseline"] = f"{type(e).__name__}: {e}"[:600]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
