"""g6d_frame_crop (csrc/frame_crop.hip) against the g6d_warp_batch call it replaces, and a tracker tick with crops="source" against
crops="canvas", on device-resident camera frames (what a hardware decoder leaves): 8 and 32 slots of

  nv12-1080p   1080x1920 NV12 (tools/track_bench.py's frames: the synthetic picture enlarged 2.25x in a grey full-HD frame)
  bgra-4k      2160x3840 BGRA (the same picture enlarged 4.5x)

both into a 540x960 canvas; --formats a,b,.. adds <format>-1080p for each named pixel format (ingest.FORMATS): the nv12-1080p picture
in that format (its BT.601 samples re-laid; bgr24 and the other packed RGB formats from the picture itself).  Kernel part: one launch of each op fills B 128x128 crops under look-at-sized homographies (a crop pixel
steps 0.4 to 1.0 canvas pixels: an object of 50 to 130 canvas pixels, i.e. small in the frame); device events around `--launches`
back-to-back calls, the two ops alternated `--repeats` times.  Tick part: tools/track_bench.py's timing (first frames and the capturing
tick excluded, the rest between two synchronisations), the two modes alternated `--repeats` times.

  python tools/frame_crop_bench.py [--slots 8,32] [--launches 200] [--frames 30] [--repeats 3] [--out profiles/r19_frame_crop.md]
  python tools/frame_crop_bench.py --skip-ticks            (the kernel part alone)
  python tools/frame_crop_bench.py --skip-ticks --slots 32 --formats nv12,bgr24,yuyv422,uyvy422,i420,yv12,p010,gray8
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CANVAS = (540, 960)
SOURCES = {"nv12-1080p": (1080, 1920, 2.25), "bgra-4k": (2160, 3840, 4.5)}
CROP = 128


def device_frames(frames, kind):
    """The synthetic 480x640 device frames -> device-resident camera Frames of `kind`, the picture enlarged (nearest) into the left
    three quarters of a grey frame; intrinsics: predict.py's pseudo K of the ingested picture."""
    import torch
    from gen6d_amd.ingest import Frame
    h, w, mul = SOURCES[kind]
    yi = (torch.arange(h, device="cuda") / mul).long().clamp_(max=479)
    xi = (torch.arange(int(640 * mul), device="cuda") / mul).long().clamp_(max=639)
    out = []
    fmt = kind[:-6] if kind.endswith("-1080p") else None      # a --formats source
    for f in frames[:8]:
        g = f[yi][:, xi]
        if fmt in ("rgb24", "bgr24", "rgba32", "bgra32"):
            buf = torch.full((h, w, 4 if fmt.endswith("32") else 3), 128, dtype=torch.uint8, device="cuda")
            buf[:, :g.shape[1], :3] = g.flip(-1) if fmt.startswith("bgr") else g
            out.append(Frame(buf, fmt))
            continue
        if kind == "bgra-4k":
            buf = torch.full((h, w, 4), 128, dtype=torch.uint8, device="cuda")
            buf[:, :g.shape[1], :3] = g.flip(-1)
            out.append(Frame(buf, "bgra32"))
            continue
        g = g.long()
        buf = torch.full((h * 3 // 2, w), 128, dtype=torch.uint8, device="cuda")
        buf[:h, :g.shape[1]] = (((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16).to(torch.uint8)
        c = g[::2, ::2]
        buf[h:, 0:g.shape[1]:2] = (((-38 * c[..., 0] - 74 * c[..., 1] + 112 * c[..., 2] + 128) >> 8) + 128).to(torch.uint8)
        buf[h:, 1:g.shape[1]:2] = (((112 * c[..., 0] - 94 * c[..., 1] - 18 * c[..., 2] + 128) >> 8) + 128).to(torch.uint8)
        if fmt in (None, "nv12"):
            out.append(Frame(buf, "nv12"))
            continue
        Y, U, V = buf[:h], buf[h:, 0::2], buf[h:, 1::2]   # the same samples in the format's layout
        if fmt == "gray8":
            out.append(Frame(Y.contiguous(), fmt))
        elif fmt == "p010":
            out.append(Frame((buf.to(torch.int32) << 8).to(torch.uint16), fmt))
        elif fmt in ("i420", "yv12"):
            first, second = (U, V) if fmt == "i420" else (V, U)
            out.append(Frame(torch.cat([Y.reshape(-1), first.reshape(-1), second.reshape(-1)]).reshape(h * 3 // 2, w), fmt))
        else:
            c = torch.stack([U, V], -1).repeat_interleave(2, 0).reshape(h, w // 2, 2)     # a chroma row per picture row
            pair = torch.stack([Y[:, 0::2], c[..., 0], Y[:, 1::2], c[..., 1]], -1) if fmt == "yuyv422" else \
                torch.stack([c[..., 0], Y[:, 0::2], c[..., 1], Y[:, 1::2]], -1)
            out.append(Frame(pair.reshape(h, w, 2).contiguous(), fmt))
    return out


def look_at_maps(rng, B):
    """Crop -> canvas homographies the size of the refiner's look-at crops of a small object: rotation, 0.4 to 1.0 canvas pixels per crop
    pixel, centred inside the picture's left three quarters."""
    H = []
    for _ in range(B):
        a, s = rng.uniform(-0.5, 0.5), rng.uniform(0.4, 1.0)
        cx, cy = rng.uniform(150, 570), rng.uniform(120, 420)
        R = np.array([[s * np.cos(a), -s * np.sin(a)], [s * np.sin(a), s * np.cos(a)]])
        t = np.array([cx, cy]) - R @ [CROP / 2, CROP / 2]
        H.append(np.array([[R[0, 0], R[0, 1], t[0]], [R[1, 0], R[1, 1], t[1]], [rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]]).reshape(9))
    return np.asarray(H, np.float32)


def kernel_rows(frames, args):
    import torch
    from gen6d_amd import ops
    from gen6d_amd.ingest import SourceTable, ingest_frames_keep
    rng = np.random.RandomState(0)
    rows = []
    for kind in SOURCES:
        cam = device_frames(frames, kind)
        for B in args.slots:
            imgs = torch.zeros((B,) + CANVAS + (3,), dtype=torch.uint8, device="cuda")
            staged = ingest_frames_keep([cam[b % len(cam)] for b in range(B)], imgs, torch.zeros((B, 3, 3), device="cuda"))[1]
            src = SourceTable.of(staged)
            hinv = torch.from_numpy(look_at_maps(rng, B)).cuda()
            ar = torch.arange(B, dtype=torch.int32, device="cuda")
            out = torch.empty((B, 3, CROP, CROP), device="cuda")
            calls = {"warp_batch": lambda: ops.warp_batch(imgs, None, ar, hinv, CROP, CROP, out=out),
                     "frame_crop": lambda: ops.frame_crop(src.table, src.rec, imgs, hinv, CROP, CROP, out=out)}
            us = {k: [] for k in calls}
            for _ in range(args.repeats):
                for name, call in calls.items():       # alternated
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    us[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
            w, c = np.array(us["warp_batch"]), np.array(us["frame_crop"])
            rows.append(f"| {kind} | {B} | {np.median(w):.1f} | {np.median(c):.1f} | {B * 3 * CROP * CROP * 4 / 1e6:.2f} MB | "
                        f"{', '.join(f'{v:.1f}' for v in w)} | {', '.join(f'{v:.1f}' for v in c)} |")
            print(rows[-1], flush=True)
        del cam
    return ["| source | slots | warp_batch us per call (median) | frame_crop us per call (median) | written per call | warp_batch runs | frame_crop runs |",
            "|---|---:|---:|---:|---:|---|---|"] + rows


def tick_rows(est, frames, args):
    import torch
    from gen6d_amd.tracking import StreamTracker
    rows = []
    for kind in SOURCES:
        cam = device_frames(frames, kind)
        for S in args.slots:
            ids = list(range(S))
            frame = lambda s, t: cam[(7 * s + t) % len(cam)]
            ms = {"canvas": [], "source": []}
            for _ in range(args.repeats):
                for mode in ms:                        # alternated
                    tr = StreamTracker(est, S, batch=min(S, 8), frame_size=CANVAS, crops=mode)
                    for t in range(2):                 # first frames, then the tick that captures the lanes' graphs
                        tr.push(ids, [frame(s, t) for s in ids])
                    tr.result()
                    t0 = time.perf_counter()
                    for t in range(2, args.frames):
                        tr.push(ids, [frame(s, t) for s in ids])
                    torch.cuda.synchronize()
                    ms[mode].append((time.perf_counter() - t0) / (args.frames - 2) * 1e3)
                    tr.result()
            cv, so = np.array(ms["canvas"]), np.array(ms["source"])
            rows.append(f"| {kind} | {S} | {min(S, 8)} | {np.median(cv):.3f} | {np.median(so):.3f} | {(cv.max() - cv.min()) / np.median(cv):.1%} | "
                        f"{(so.max() - so.min()) / np.median(so):.1%} | {', '.join(f'{v:.3f}' for v in cv)} | {', '.join(f'{v:.3f}' for v in so)} |")
            print(rows[-1], flush=True)
        del cam
    return ["| source | streams | batch | canvas ms per tick (median) | source ms per tick (median) | canvas spread | source spread | canvas runs | source runs |",
            "|---|---:|---:|---:|---:|---:|---:|---|---|"] + rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-ticks", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--formats", default=None, help="comma list of pixel formats: adds the source <format>-1080p for each")
    args = ap.parse_args()
    for f in (args.formats.split(",") if args.formats else []):
        SOURCES.setdefault(f"{f}-1080p", (1080, 1920, 2.25))
    args.slots = [int(s) for s in args.slots.split(",")]
    import torch
    if not torch.cuda.is_available():
        sys.exit("frame_crop_bench: needs the GPU (the kernels have no CPU fallback)")
    from track_bench import build
    est, frames, _ = build(torch.device("cuda", 0))
    text = ["## The crop launch (tools/frame_crop_bench.py)", "",
            f"{CROP}x{CROP} crops of device-resident frames in a {CANVAS[0]}x{CANVAS[1]} canvas, device events around {args.launches} back-to-back "
            f"calls, {args.repeats} repeats of each op, alternated.", ""] + kernel_rows(frames, args)
    if not args.skip_ticks:
        text += ["", "## A tracker tick in both modes", "",
                 f"Synthetic database and weights, graphs, device-resident frames, {args.frames} frames per stream, the first two excluded, "
                 f"{args.repeats} repeats of each mode, alternated; spread = (max - min) / median.", ""] + tick_rows(est, frames, args)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
