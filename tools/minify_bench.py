"""minify="area"  beside the point-sampled default, on device-resident frames into a 540x960 canvas.  Four parts:

  ingest     g6d_frame_ingest against g6d_frame_ingest_area on 8 NV12 3840x2160 frames and on 8 bgr24 1920x1080 frames (noise), the table
             already on the device; both against the byte floor: source bytes + canvas bytes over the HBM rate of tools/ingest_bench.py
  crop       g6d_frame_crop against g6d_frame_crop_area for 8 slots of 128x128 cut from 4K BGRA frames, under maps whose footprint makes
             n = 1, 4 and 8
  tick       a tracker tick (8 streams, batch 8, graphs, crops="source") with minify="point" and "area" on tools/frame_crop_bench.py's
             sources, and the ingest call of such a tick alone (table upload included), whose share of the tick is quoted
  aliasing   RMS error in grey levels of both ingest rules against a float64 box filter at 4:1, on noise and on a zone plate

Device events around `--launches` back-to-back calls, the two variants alternated `--repeats` times.

  python tools/minify_bench.py [--launches 100] [--repeats 3] [--frames 30] [--skip-ticks] [--out profiles/r28_minify.md]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ingest_bench import HBM_BPS, SRC_BYTES, frame_array  # noqa: E402

CANVAS = (540, 960)
CROP = 128
N = 8
INGEST_CASES = {"nv12-4k": ((2160, 3840), "nv12"), "bgr24-1080p": ((1080, 1920), "bgr24")}


def timed(calls, launches, repeats):
    """name -> call, alternated -> name -> [us per call of each repeat]."""
    import torch
    us = {k: [] for k in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    return us


def runs(v):
    return ", ".join(f"{x:.1f}" for x in v)


def ingest_rows(args):
    import torch
    from gen6d_amd import ops
    from gen6d_amd.ingest import Frame, ingest_frames_keep
    rng = np.random.RandomState(0)
    rows = []
    for name, ((h, w), fmt) in INGEST_CASES.items():
        frames = [Frame(torch.from_numpy(frame_array(rng, fmt, h, w)).cuda(), fmt) for _ in range(N)]
        out, K = torch.zeros((N,) + CANVAS + (3,), dtype=torch.uint8, device="cuda"), torch.zeros((N, 3, 3), device="cuda")
        table = ingest_frames_keep(frames, out, K)[1].table
        us = timed({"point": lambda: ops.frame_ingest(table, N, out, K), "area": lambda: ops.frame_ingest_area(table, None, N, out, K)},
                   args.launches, args.repeats)
        b = N * (int(h * w * SRC_BYTES[fmt]) + CANVAS[0] * CANVAS[1] * 3)
        floor = b / HBM_BPS * 1e6
        p, a = np.median(us["point"]), np.median(us["area"])
        rows.append(f"| {name} | {h / CANVAS[0]:.0f}:1 | {b / 1e6:.1f} MB | {floor:.1f} | {p:.1f} | {p / floor:.1f}x | {a:.1f} | {a / floor:.1f}x | "
                    f"{b / a / 1e6:.2f} | {runs(us['point'])} | {runs(us['area'])} |")
        print(rows[-1], flush=True)
        del frames, table
    return ["| case | ratio | source + canvas bytes | floor us | point us (median) | point / floor | area us (median) | area / floor | area TB/s | "
            "point runs | area runs |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|---|---|"] + rows


def crop_maps(rng, B, step):
    """Crop -> canvas maps of one scale: a crop pixel steps `step` canvas pixels; centred inside the picture's left three quarters."""
    H = []
    for _ in range(B):
        a = rng.uniform(-0.5, 0.5)
        R = step * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        t = np.array([rng.uniform(250, 470), rng.uniform(200, 340)]) - R @ [CROP / 2, CROP / 2]
        H.append(np.array([[R[0, 0], R[0, 1], t[0]], [R[1, 0], R[1, 1], t[1]], [0, 0, 1.0]]).reshape(9))
    return np.asarray(H, np.float32)


def crop_rows(frames, args):
    import torch
    from frame_crop_bench import device_frames
    from gen6d_amd import ops
    from gen6d_amd.ingest import SourceTable, ingest_frames_keep
    rng = np.random.RandomState(1)
    cam = device_frames(frames, "bgra-4k")
    imgs = torch.zeros((N,) + CANVAS + (3,), dtype=torch.uint8, device="cuda")
    src = SourceTable.of(ingest_frames_keep([cam[b % len(cam)] for b in range(N)], imgs, torch.zeros((N, 3, 3), device="cuda"))[1])
    out = torch.empty((N, 3, CROP, CROP), device="cuda")
    rows = []
    for n in (1, 4, 8):                                # the 4K source is 4x the canvas: a step of n / 4 canvas pixels covers n source pixels
        hinv = torch.from_numpy(crop_maps(rng, N, n / 4)).cuda()
        us = timed({"point": lambda: ops.frame_crop(src.table, src.rec, imgs, hinv, CROP, CROP, out=out),
                    "area": lambda: ops.frame_crop_area(src.table, src.rec, imgs, hinv, CROP, CROP, 8, out=out)}, args.launches, args.repeats)
        rows.append(f"| {n} | {n * n * 4} | {np.median(us['point']):.1f} | {np.median(us['area']):.1f} | {runs(us['point'])} | {runs(us['area'])} |")
        print(rows[-1], flush=True)
    return ["| n | taps per crop pixel | frame_crop us (median) | frame_crop_area us (median) | frame_crop runs | frame_crop_area runs |",
            "|---:|---:|---:|---:|---|---|"] + rows


def tick_rows(est, frames, args):
    import torch
    from frame_crop_bench import device_frames
    from gen6d_amd.ingest import ingest_frames_keep
    from gen6d_amd.tracking import StreamTracker
    rows = []
    for kind in ("nv12-1080p", "bgra-4k"):
        cam = device_frames(frames, kind)
        ids = list(range(N))
        frame = lambda s, t: cam[(7 * s + t) % len(cam)]
        ms = {"point": [], "area": []}
        for _ in range(args.repeats):
            for mode in ms:                            # alternated
                tr = StreamTracker(est, N, batch=N, frame_size=CANVAS, crops="source", minify=mode)
                for t in range(2):                     # first frames, then the tick that captures the lane's graph
                    tr.push(ids, [frame(s, t) for s in ids])
                tr.result()
                t0 = time.perf_counter()
                for t in range(2, args.frames):
                    tr.push(ids, [frame(s, t) for s in ids])
                torch.cuda.synchronize()
                ms[mode].append((time.perf_counter() - t0) / (args.frames - 2) * 1e3)
                tr.result()
        out, K = torch.zeros((N,) + CANVAS + (3,), dtype=torch.uint8, device="cuda"), torch.zeros((N, 3, 3), device="cuda")
        us = timed({m: (lambda m=m: ingest_frames_keep([cam[b % len(cam)] for b in range(N)], out, K, minify=m)) for m in ms}, args.launches, args.repeats)
        p, a = np.median(ms["point"]), np.median(ms["area"])
        ip, ia = np.median(us["point"]), np.median(us["area"])
        rows.append(f"| {kind} | {p:.3f} | {a:.3f} | {ip:.1f} | {ia:.1f} | {ip / (p * 1e3):.2%} | {ia / (a * 1e3):.2%} | "
                    f"{', '.join(f'{v:.3f}' for v in ms['point'])} | {', '.join(f'{v:.3f}' for v in ms['area'])} |")
        print(rows[-1], flush=True)
        del cam
    return ["| source | point ms per tick (median) | area ms per tick (median) | point ingest call us | area ingest call us | point ingest share | "
            "area ingest share | point tick runs | area tick runs |", "|---|---:|---:|---:|---:|---:|---:|---|---|"] + rows


def aliasing_rows():
    import torch
    from gen6d_amd import ops
    from gen6d_amd.ingest import Frame, ingest_frames_keep
    h, w = 4 * CANVAS[0], 4 * CANVAS[1]
    y, x = np.meshgrid(np.arange(h) - h / 2, np.arange(w) - w / 2, indexing="ij")
    pictures = {"noise": np.random.RandomState(2).randint(0, 256, (h, w)).astype(np.uint8),
                # a zone plate: the local frequency grows with the radius and reaches 0.5 cycles per source pixel at the picture's edge
                "zone plate": np.rint(127.5 + 127.5 * np.cos(np.pi * (x * x + y * y) / (2 * (w / 2)))).astype(np.uint8)}
    rows = []
    for name, pic in pictures.items():
        box = pic.astype(np.float64).reshape(CANVAS[0], 4, CANVAS[1], 4).mean((1, 3))
        out, K = torch.zeros((1,) + CANVAS + (3,), dtype=torch.uint8, device="cuda"), torch.zeros((1, 3, 3), device="cuda")
        table = ingest_frames_keep([Frame(torch.from_numpy(pic).cuda(), "gray8")], out, K)[1].table
        rms = {}
        for mode, op in (("point", lambda: ops.frame_ingest(table, 1, out, K)), ("area", lambda: ops.frame_ingest_area(table, None, 1, out, K))):
            op()
            rms[mode] = float(np.sqrt(np.mean((out[0, :, :, 0].cpu().numpy().astype(np.float64) - box) ** 2)))
        rows.append(f"| {name} | {rms['point']:.2f} | {rms['area']:.2f} |")
        print(rows[-1], flush=True)
    return ["| picture (gray8 2160x3840 -> 540x960) | point rule RMS error, grey levels | area rule RMS error, grey levels |", "|---|---:|---:|"] + rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--skip-ticks", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("minify_bench: needs the GPU (the kernels have no CPU fallback)")
    from track_bench import build
    est, frames, _ = build(torch.device("cuda", 0))
    text = ["## Ingest: the point rule and the area rule against the byte floor (tools/minify_bench.py)", "",
            f"{N} device-resident noise frames per launch into {CANVAS[0]}x{CANVAS[1]} canvases, the table on the device, device events around "
            f"{args.launches} back-to-back launches, {args.repeats} repeats of each rule, alternated.  Floor: source bytes + canvas bytes over "
            f"{HBM_BPS / 1e12:.1f} TB/s.  The point rule reads about a quarter of the source at 4:1 and half of it at 2:1; the area rule reads all of it.", ""]
    text += ingest_rows(args)
    text += ["", "## Crops: g6d_frame_crop and g6d_frame_crop_area", "",
             f"{N} slots of {CROP}x{CROP} cut from 2160x3840 BGRA frames under maps whose footprint gives n = 1, 4 and 8 (max_n = 8).", ""]
    text += crop_rows(frames, args)
    if not args.skip_ticks:
        text += ["", "## A tracker tick with crops=\"source\" in both modes", "",
                 f"Synthetic database and weights, graphs, {N} streams at batch {N}, device-resident frames, {args.frames} frames per stream, the "
                 f"first two excluded, {args.repeats} repeats of each mode, alternated.  Ingest call: `ingest_frames_keep` of the tick's {N} frames "
                 "alone (table upload included), its share of the same mode's tick.", ""] + tick_rows(est, frames, args)
    text += ["", "## Aliasing at 4:1 against a float64 box filter", "",
             "The mean of every 4 x 4 block in float64, unrounded, is the reference; RMS of (rule - reference) over the canvas.  The area rule's "
             "error is its rounding to 8 bits (a uniform error of +-1/2: 0.29).", ""] + aliasing_rows()
    print("\n".join(text))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
