"""Tracked frames/s of gen6d_amd.tracking.StreamTracker on the synthetic database and weights (bench.py's chained leg: 480x640 frames,
the refiner's pose heads damped towards the identity update).

For S streams x F frames: every stream's first frame (detection + selection + refine_iter steps) and one tracked tick (lazy graph
capture) are excluded; the remaining F - 2 ticks are timed between two device synchronisations.  Frames are on the device before the
clock starts (the upload of a user's numpy frames is not part of the tick).  Graphs and eager ticks run alternately, `--repeats` times
each; the table gives the median and the spread (max - min) / median.

  python tools/track_bench.py [--streams 1,8,32] [--frames 30] [--repeats 3] [--out profiles/r08_track_bench.md]
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


def run(est, frames, K, S, F, batch, graphs):
    """-> (seconds of the timed ticks, timed ticks)."""
    import torch
    from gen6d_amd.tracking import StreamTracker
    tr = StreamTracker(est, S, batch=batch, graphs=graphs)
    ids = list(range(S))
    Ks = [K] * S
    frame = lambda s, t: frames[(7 * s + t) % len(frames)]
    for t in range(2):                                  # first frames, then the tick that captures the lanes' graphs
        tr.push(ids, [frame(s, t) for s in ids], Ks)
    tr.result()
    t0 = time.perf_counter()
    for t in range(2, F):
        tr.push(ids, [frame(s, t) for s in ids], Ks)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.result()
    return dt, F - 2


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
    ap.add_argument("--tick-ms", type=float, default=0.0)
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
    if args.profile:
        S = args.profile
        dt, n = run(est, frames, K, S, args.frames, min(S, 8), True)
        print(f"profile S={S}: {n} ticks, {dt / n * 1e3:.3f} ms/tick")
        return
    configs = [(int(s), min(int(s), 8)) for s in args.streams.split(",")]
    if 32 in [c[0] for c in configs]:
        configs.append((32, 32))
    lines = ["| streams | batch | lanes | mode | tracked frames/s (median) | ms per tick | spread |", "|---:|---:|---:|---|---:|---:|---:|"]
    for S, B in configs:
        res = {True: [], False: []}
        for _ in range(args.repeats):
            for g in (True, False):                   # alternated
                dt, n = run(est, frames, K, S, args.frames, B, g)
                res[g].append((S * n / dt, dt / n * 1e3))
        for g in (True, False):
            fps = np.array([r[0] for r in res[g]])
            ms = np.array([r[1] for r in res[g]])
            med = float(np.median(fps))
            lines.append(f"| {S} | {B} | 2 | {'graphs' if g else 'eager'} | {med:.1f} | {float(np.median(ms)):.3f} | "
                         f"{(fps.max() - fps.min()) / med:.1%} |")
            print(lines[-1], flush=True)
    txt = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Tracked frames/s (tools/track_bench.py)\n\n"
                    f"Synthetic database and weights, 480x640 frames, {args.frames} frames per stream, the first two excluded (first frames "
                    f"and the graph-capturing tick), {args.repeats} repeats of each mode, alternated.  One tracked frame = one refinement "
                    "step from the stream's previous pose + the box smoothing.\n\n" + txt + "\n")


if __name__ == "__main__":
    main()
