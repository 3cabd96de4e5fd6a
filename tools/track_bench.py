"""Tracked frames/s of gen6d_amd.tracking.StreamTracker on the synthetic database and weights (bench.py's chained leg: 480x640 frames,
the refiner's pose heads damped towards the identity update).

For S streams x F frames: every stream's first frame (detection + selection + refine_iter steps) and one tracked tick (lazy graph
capture) are excluded; the remaining F - 2 ticks are timed between two device synchronisations.  Frames are on the device before the
clock starts (the upload of a user's numpy frames is not part of the tick).  Graphs and eager ticks run alternately, `--repeats` times
each; the table gives the median and the spread (max - min) / median.

  python tools/track_bench.py [--streams 1,8,32] [--frames 30] [--repeats 3] [--out profiles/r08_track_bench.md]
  python tools/track_bench.py --streams 32 --ingest none,same,nv12-1080p[,nv12-1080p-lens][,nv12-1080p-area,nv12-1080p-lens-area]   (graphs only, the variants alternated)
  python tools/track_bench.py --streams 32 --emit nv12 [--emit-host]            (graphs only: no sinks / device sinks / pinned host sinks
                                                                                 of the working-resolution picture, alternated)
  python tools/track_bench.py --streams 32 --ingest nv12-1080p --emit nv12 --emit-source [--emit-host]   (the same plus one SOURCE-view sink
                                                                                 per stream: the camera's own 1080x1920 frame, NV12 pass-through)
  python tools/track_bench.py --streams 32 --health off,lax,verify10 [--lens 10000]   (graphs only: no HealthPolicy / every soft
                                                     gate off / the same with the detector's check every 10th tick; --lens: see health_policy)
  rocprofv3 --kernel-trace --stats -d DIR -o track -- python tools/track_bench.py --profile 32      (one configuration, graphs)
  python tools/track_bench.py --stats-csv DIR/.../track_kernel_stats.csv --ticks N --tick-ms T --out profiles/r08_track_kernel_stats.md
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(dev):
    import torch
    from gen6d_amd import synth
    from gen6d_amd.estimator import Gen6DEstimator
    from gen6d_amd.network import name2network
    from gen6d_amd.synth_db import SyntheticDatabase
    mods = {}
    for k in ("detector", "selector", "refiner"):
        net = name2network[k]({"name": k + "_synth"}).eval()
        sd = synth.synth_state_dict(k)
        net.load_state_dict(synth.damp_refiner_head(sd) if k == "refiner" else sd)
        mods[k] = net.to(dev)
    db = SyntheticDatabase(n_views=88, size=(480, 640), focal=560.0)
    est = Gen6DEstimator({"ref_view_num": 64, "det_ref_view_num": 32, "refine_iter": 3}, modules=mods)
    est.build(db, "all")
    _, que = db.get_split("all")
    frames = [torch.from_numpy(np.ascontiguousarray(db.get_image(i))).to(dev) for i in que]
    K = db.get_K(que[0])
    torch.cuda.synchronize()
    return est, frames, K


def native_frames(frames, K, mode):
    """The frames a tracker with frame_size is fed -> (Frame list, canvas).
    same: the device-resident 480x640 RGB frames with their K, through the ingest launch (the computation of the plain path).
    nv12-1080p: host-resident 1080x1920 NV12 frames (numpy) into a 540x960 canvas: each synthetic
    frame enlarged 2.25x (nearest) into the left 1440 columns of a grey full-HD picture, BT.601; intrinsics: predict.py's pseudo K.
    nv12-1080p-lens: the same frames as pictures of a camera with f = 1000 and the lens brown (-0.35, 0.12, 0.001, -0.0005, -0.02),
    undistorted by the ingest launch (one mesh for all streams, built and uploaded in the first tick).
    nv12-1080p-area / nv12-1080p-lens-area: the nv12-1080p / nv12-1080p-lens frames for a tracker with minify="area" (`run` sets it), the
    lens with minify="area": n x n sub-samples per canvas pixel through the mesh."""
    import torch
    from gen6d_amd.ingest import Frame, Lens
    cam = {}
    if mode in ("nv12-1080p-lens", "nv12-1080p-lens-area"):
        cam = dict(K=np.array([[1000.0, 0, 959.5], [0, 1000.0, 539.5], [0, 0, 1]]),
                   lens=Lens("brown", (-0.35, 0.12, 0.001, -0.0005, -0.02), minify="area" if mode.endswith("-area") else "point"))
    if mode == "same":
        return [Frame(f, K=K) for f in frames], tuple(frames[0].shape[:2])
    out = []
    yi, xi = (np.arange(1080) / 2.25).astype(int), (np.arange(1440) / 2.25).astype(int)
    for f in frames[:8]:
        g = f.cpu().numpy()[yi][:, xi].astype(np.int64)
        buf = np.full((1620, 1920), 128, np.uint8)
        buf[:1080, :1440] = ((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16
        c = g[::2, ::2]
        buf[1080:, 0:1440:2] = ((-38 * c[..., 0] - 74 * c[..., 1] + 112 * c[..., 2] + 128) >> 8) + 128
        buf[1080:, 1:1440:2] = ((112 * c[..., 0] - 94 * c[..., 1] - 18 * c[..., 2] + 128) >> 8) + 128
        out.append(Frame(buf, "nv12", **cam))
    return out, (540, 960)


def make_sinks(S, hw, fmt, host, view="canvas"):
    """One sink per stream for the smoothed picture, in device memory or in pinned host memory; reused every tick (a lane's emits are
    ordered on its stream).  hw: the working resolution for canvas sinks, the camera frame's size for source-view sinks."""
    import torch
    from gen6d_amd.emit import Sink
    h, w = hw
    shape = (h * 3 // 2, w) if fmt == "nv12" else (h, w, 3)
    mk = (lambda: torch.zeros(shape, dtype=torch.uint8).pin_memory()) if host else (lambda: torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    return [Sink(mk(), fmt, view=view) for _ in range(S)]


def health_policy(mode):
    """off: no policy.  lax: the health launches with every soft gate off.  verify10: the same plus the detector's check on every 10th
    tick.  The synthetic weights put the object centre at a depth of ~3e-5 focal lengths, i.e. ~0 with the database's intrinsics, where
    about a third of all frames fall behind the camera, which no policy forgives: every such loss of a live stream costs one acquisition
    (detection, selection, refine_iter steps) at the push where the host learns of it, and the run measures those.  `--lens MUL` feeds
    every variant of a --health run (off included) intrinsics of MUL times the focal length, which keeps the centre in front: the
    table's `lost` column counts the streams that are LOST at the end of a run."""
    from gen6d_amd.tracking import HealthPolicy
    if mode in (None, "off"):
        return {}
    return {"health": HealthPolicy.lax(verify_every={"lax": 0, "verify10": 10}[mode])}


def run(est, frames, K, S, F, batch, graphs, ingest=None, emit=None, emit_host=False, health=None, lost=None, emit_view="canvas"):
    """-> (seconds of the timed ticks, timed ticks).  lost: a list that receives the number of LOST streams at the end of a health run.  ingest: None (plain frames, the tracker without frame_size) or a mode of
    native_frames.  emit: None, or the format of one sink per stream filled on every push (emit_host: pinned host sinks; emit_view
    "source": the camera's own frame at its own size, which needs an ingest mode).  health: a mode of health_policy."""
    import torch
    from gen6d_amd.tracking import StreamTracker
    ids = list(range(S))
    hk = health_policy(health)
    if ingest in (None, "none"):
        tr = StreamTracker(est, S, batch=batch, graphs=graphs, **hk)
        Ks = [K] * S
        canvas = tuple(frames[0].shape[:2])
    else:
        frames, canvas = native_frames(frames, K, ingest)
        tr = StreamTracker(est, S, batch=batch, graphs=graphs, frame_size=canvas, minify="area" if ingest.endswith("-area") else "point", **hk)
        Ks = None
    frame = lambda s, t: frames[(7 * s + t) % len(frames)]
    if emit and emit_view == "source":
        if ingest in (None, "none"):
            sys.exit("track_bench: source-view sinks need camera frames (--ingest same / nv12-1080p)")
        kw = {"sinks": make_sinks(S, (frames[0].height, frames[0].width), emit, emit_host, "source")}
    else:
        kw = {"sinks": make_sinks(S, canvas, emit, emit_host)} if emit else {}
    for t in range(2):                                  # first frames, then the tick that captures the lanes' graphs
        tr.push(ids, [frame(s, t) for s in ids], Ks, **kw)
    tr.result()
    t0 = time.perf_counter()
    for t in range(2, F):
        tr.push(ids, [frame(s, t) for s in ids], Ks, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.result()
    if hk and lost is not None:
        lost.append(sum(h.status == 3 for h in tr.health().values()))
    return dt, F - 2


def sweep(est, frames, K, args, configs, variants, label, title, text, lanes=False):
    """Every (streams, batch) configuration x every variant [(name, keywords of `run`)] (graphs unless a variant says otherwise),
    `--repeats` times, alternated -> one table row each, printed as it is known; `--out` receives the table under `title` and `text`.
    label: the heading of the variants' column.  lanes: the plain table, with a lanes column and without the list of runs.  Variants with
    a health policy add the `lost` column."""
    health = any("health" in kw for _, kw in variants)
    cols = ["streams", "batch"] + ["lanes"] * lanes + [label, "tracked frames/s (median)", "ms per tick", "spread"]
    cols += ["runs (frames/s)"] * (not lanes) + ["lost"] * health
    lines = ["| " + " | ".join(cols) + " |", "|" + "|".join("---" if c in (label, "runs (frames/s)", "lost") else "---:" for c in cols) + "|"]
    for S, B in configs:
        res, lost = {name: [] for name, _ in variants}, {name: [] for name, _ in variants}
        for _ in range(args.repeats):
            for name, kw in variants:                 # alternated
                dt, n = run(est, frames, K, S, args.frames, B, **{"graphs": True, "lost": lost[name], **kw})
                res[name].append((S * n / dt, dt / n * 1e3))
        for name, _ in variants:
            fps, ms = np.array([r[0] for r in res[name]]), np.array([r[1] for r in res[name]])
            med = float(np.median(fps))
            cells = [str(S), str(B)] + ["2"] * lanes + [name, f"{med:.1f}", f"{float(np.median(ms)):.3f}", f"{(fps.max() - fps.min()) / med:.1%}"]
            cells += [", ".join(f"{v:.1f}" for v in fps)] * (not lanes) + [", ".join(str(v) for v in lost[name]) or "-"] * health
            lines.append("| " + " | ".join(cells) + " |")
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"# {title}\n\n{text}\n\n" + "\n".join(lines) + "\n")


def stats_table(csv_path, ticks, tick_ms):
    """rocprofv3 kernel stats CSV -> markdown rows (name, calls, total ms, per tick us, share of a tick)."""
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    out = ["| kernel | calls | total ms | per tick us | share of tick |", "|---|---:|---:|---:|---:|"]
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    for r in rows:
        tot = float(r["TotalDurationNs"]) / 1e6
        per = tot / ticks * 1e3
        out.append(f"| `{r['Name'][:90]}` | {r['Calls']} | {tot:.3f} | {per:.1f} | {per / (tick_ms * 1e3):.2%} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,32")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0, help="one graphs run of this many streams (for a rocprofv3 trace)")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--ticks", type=int, default=0)
    ap.add_argument("--ingest", default=None, help="comma list of none / same / nv12-1080p / nv12-1080p-lens / nv12-1080p-area / nv12-1080p-lens-area: graphs runs of these frame "
                    "sources, alternated (with --profile: the one source of the profiled run)")
    ap.add_argument("--batch", type=int, default=0, help="--profile: slots per lane (default min(streams, 8))")
    ap.add_argument("--emit", default=None, choices=["nv12", "rgb24"], help="graphs runs without sinks and with one device sink of this "
                    "format per stream, alternated (with --profile: the profiled run emits)")
    ap.add_argument("--emit-host", action="store_true", help="--emit: pinned host sinks as a third variant (--profile: instead of device sinks)")
    ap.add_argument("--emit-source", action="store_true", help="--emit: one source-view sink per stream (the camera's own frame at its own "
                    "size; needs --ingest) as further variants (--profile: instead of the canvas sinks)")
    ap.add_argument("--tick-ms", type=float, default=0.0)
    ap.add_argument("--health", default=None, help="comma list of off / lax / verify10: graphs runs "
                    "with these health policies, alternated (with --profile: the one policy of the profiled run)")
    ap.add_argument("--lens", type=float, default=1.0, help="--health: every variant runs behind intrinsics of this many focal lengths")
    args = ap.parse_args()
    if args.stats_csv:
        txt = stats_table(args.stats_csv, args.ticks, args.tick_ms)
        print(txt)
        if args.out:
            with open(args.out, "w") as f:
                f.write(f"# Kernel time of the tracker (rocprofv3 --kernel-trace --stats)\n\n{args.ticks} ticks timed and profiled; tick time "
                        f"{args.tick_ms:.3f} ms (unprofiled run of the same configuration).  The table includes the setup (first frames, "
                        f"graph warm-up and capture) in `calls`/`total`; per-tick figures divide the totals by the ticks.\n\n{txt}\n")
        return
    import torch
    dev = torch.device("cuda", 0)
    est, frames, K = build(dev)
    if args.health and args.lens != 1.0:
        K = (np.asarray(K, np.float32) * np.array([[args.lens, 1, 1], [1, args.lens, 1], [1, 1, 1]])).astype(np.float32)
    if args.profile:
        S = args.profile
        dt, n = run(est, frames, K, S, args.frames, args.batch or min(S, 8), True, args.ingest, args.emit, args.emit_host, args.health,
                    emit_view="source" if args.emit_source else "canvas")
        print(f"profile S={S} ingest={args.ingest} emit={args.emit}{' (host)' if args.emit and args.emit_host else ''}"
              f"{' (source view)' if args.emit and args.emit_source else ''} "
              f"health={args.health}: {n} ticks, "
              f"{dt / n * 1e3:.3f} ms/tick")
        return
    configs = [(int(s), min(int(s), 8)) for s in args.streams.split(",")]
    if 32 in [c[0] for c in configs]:
        configs.append((32, 32))
    graphs = "Synthetic database and weights, graphs, "
    each = f"{args.frames} frames per stream, the first two excluded, {args.repeats} repeats of each "
    if args.health:
        sweep(est, frames, K, args, configs, [(m, {"ingest": args.ingest, "health": m}) for m in args.health.split(",")], "health",
              "Tracked frames/s by health policy (tools/track_bench.py --health)",
              graphs + each + f"policy, alternated, intrinsics of {args.lens:g} x the database's focal length.  off: no HealthPolicy; lax: "
              "gate, health, the status mirror and the host's routing with every soft gate off; verify10: the same with the detector's "
              "check on every 10th tick; lost: streams LOST at the end of each run.")
    elif args.emit:
        dev = {"ingest": args.ingest, "emit": args.emit}
        src = dict(dev, emit_view="source")
        sweep(est, frames, K, args, configs,
              [("none", {"ingest": args.ingest}), ("device", dev)] + ([("host", dict(dev, emit_host=True))] if args.emit_host else []) +
              ([("source", src)] + ([("source-host", dict(src, emit_host=True))] if args.emit_host else []) if args.emit_source else []), "sinks",
              f"Tracked frames/s with annotated frame output (tools/track_bench.py --emit {args.emit})",
              graphs + each + f"variant, alternated.  none: no sinks; device: one {args.emit} device sink per stream and frame (the smoothed "
              "picture at working resolution); host: the same into pinned host memory, copy included; source / source-host: one "
              "source-view sink per stream instead (the camera's own frame at its own size with the box in source pixels).")
    elif args.ingest:
        sweep(est, frames, K, args, configs, [(m, {"ingest": m}) for m in args.ingest.split(",")], "frames",
              "Tracked frames/s by frame source (tools/track_bench.py --ingest)",
              graphs + each + "source, alternated.  none: plain 480x640 device frames (tracker without frame_size); same: the same frames "
              "through the ingest launch; nv12-1080p: host-resident 1080x1920 NV12 frames into a 540x960 canvas, upload included; "
              "nv12-1080p-lens: those frames with a strong brown lens, undistorted in the same launch.")
    else:
        sweep(est, frames, K, args, configs, [("graphs", {}), ("eager", {"graphs": False})], "mode", "Tracked frames/s (tools/track_bench.py)",
              f"Synthetic database and weights, 480x640 frames, {args.frames} frames per stream, the first two excluded (first frames "
              f"and the graph-capturing tick), {args.repeats} repeats of each mode, alternated.  One tracked frame = one refinement "
              "step from the stream's previous pose + the box smoothing.", lanes=True)

if __name__ == "__main__":
    main()
