"""The frame-emit kernels alone (csrc/emit.hip, csrc/emit_source.hip): 32 device-resident images per launch into 32 device sinks of
the same size, with a valid box on every image, four canvas cases and three source-view cases (device-resident camera frames):

  540p-nv12  / 540p-rgb24     32 x (540x960 RGB  -> NV12 / rgb24)
  1080p-nv12 / 1080p-rgb24    32 x (1080x1920 RGB -> NV12 / rgb24)
  src-1080p-nv12-pass / src-540p-nv12-pass    32 x (NV12 frame -> NV12 sink of the same matrix: the pass-through)
  src-1080p-rgb24-nv12                        32 x (1080x1920 rgb24 frame -> NV12 sink)

--formats a,b,.. adds full-HD cases for the named pixel formats (ingest.FORMATS): 1080p-<f> (canvas -> a sink of f), src-1080p-<f>-pass (a
frame of f into a sink of f and the same matrix) and src-1080p-rgb24-<f> for every f a sink can have, src-1080p-<f>-nv12 (a frame of f
converted into an NV12 sink) for every f.

Bytes are counted from shapes: the image bytes a launch reads plus the sink bytes it writes (pixel bytes only).  Timing: device events
around `--launches` back-to-back calls (includes the table upload of each call), or, under the profiler, the kernel's own durations:

  python tools/emit_bench.py [--launches 50] [--formats nv12,bgr24,yuyv422,uyvy422,i420,yv12,p010,gray8]
  rocprofv3 --kernel-trace -d DIR -o emit --output-format csv -- python tools/emit_bench.py
  python tools/emit_bench.py --trace-csv DIR/.../emit_kernel_trace.csv [--tick-ms T] [--out FILE.md]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.3e12          # achievable HBM rate the shares are quoted against
CASES = {"540p-nv12": ((540, 960), "nv12"), "540p-rgb24": ((540, 960), "rgb24"), "1080p-nv12": ((1080, 1920), "nv12"),
         "1080p-rgb24": ((1080, 1920), "rgb24"),
         # source view: (size, sink format, source format)
         "src-1080p-nv12-pass": ((1080, 1920), "nv12", "nv12"), "src-1080p-rgb24-nv12": ((1080, 1920), "nv12", "rgb24"),
         "src-540p-nv12-pass": ((540, 960), "nv12", "nv12")}
N = 32
WARM = 3


# bytes per pixel: every sample of every plane (a canvas is rgb24)
PIX_BYTES = {"rgb24": 3, "bgr24": 3, "rgba32": 4, "bgra32": 4, "nv12": 1.5, "yuyv422": 2, "uyvy422": 2, "i420": 1.5, "yv12": 1.5, "p010": 3, "gray8": 1}
READ_ONLY = ("p010", "gray8")


def case_bytes(c):
    (h, w), fmt = c[:2]
    return N * (int(h * w * PIX_BYTES[c[2] if c[2:] else "rgb24"]) + int(h * w * PIX_BYTES[fmt]))


def picture_array(rng, fmt, h, w):
    """A noise picture of the format as the array ingest.Frame / emit.Sink take: [H,W,C] packed, [H*3/2, W] for the 4:2:0 formats."""
    if fmt == "p010":
        return (rng.randint(0, 1024, (h * 3 // 2, w)) << 6).astype(np.uint16)
    shape = {"nv12": (h * 3 // 2, w), "i420": (h * 3 // 2, w), "yv12": (h * 3 // 2, w), "yuyv422": (h, w, 2), "uyvy422": (h, w, 2),
             "gray8": (h, w), "rgba32": (h, w, 4), "bgra32": (h, w, 4)}.get(fmt, (h, w, 3))
    return rng.randint(0, 256, shape).astype(np.uint8)


def trace_table(path, launches, tick_ms, CASES=CASES):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "frame_emit" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = ["| case | launches | kernel us (median) | min | max | bytes per launch | TB/s (median) | share of 6.3 TB/s | share of a tick |",
           "|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    per = WARM + launches
    for i, (name, c) in enumerate(CASES.items()):
        d = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * per + WARM:(i + 1) * per]])
        if not len(d):
            continue
        b, med = case_bytes(c), float(np.median(d))
        tick = f"{med / (tick_ms * 1e3):.2%}" if tick_ms else "-"
        out.append(f"| {name} | {len(d)} | {med:.1f} | {d.min():.1f} | {d.max():.1f} | {b / 1e6:.1f} MB | {b / med / 1e6:.2f} | "
                   f"{b / med / 1e6 / (HBM_BPS / 1e12):.1%} | {tick} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--tick-ms", type=float, default=0.0, help="tick time of the 32-stream tracker the kernel time is set against")
    ap.add_argument("--out", default=None)
    ap.add_argument("--formats", default=None, help="comma list of pixel formats: adds their full-HD cases (see above)")
    args = ap.parse_args()
    cases = dict(CASES)
    for f in (args.formats.split(",") if args.formats else []):
        if f not in READ_ONLY:
            cases.setdefault(f"1080p-{f}", ((1080, 1920), f))
            if PIX_BYTES[f] < 3:
                cases.setdefault(f"src-1080p-{f}-pass", ((1080, 1920), f, f))
            cases.setdefault(f"src-1080p-rgb24-{f}", ((1080, 1920), f, "rgb24"))
        if f != "nv12":
            cases.setdefault(f"src-1080p-{f}-nv12", ((1080, 1920), "nv12", f))
    if args.trace_csv:
        txt = trace_table(args.trace_csv, args.launches, args.tick_ms, cases)
        print(txt)
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n## The emit kernel (rocprofv3 --kernel-trace, tools/emit_bench.py)\n\n32 device-resident images and sinks per launch, a "
                        "box on every image; bytes = image bytes read + sink bytes written, from shapes.\n\n" + txt + "\n")
        return
    import torch
    from gen6d_amd.emit import Sink, emit_frames, emit_source_frames
    from gen6d_amd.ingest import Frame, ingest_frames_keep
    if not torch.cuda.is_available():
        sys.exit("emit_bench: needs the GPU (the kernel has no CPU fallback)")
    rng = np.random.RandomState(0)
    for name, ((h, w), fmt, *src) in cases.items():
        shape = picture_array(np.random.RandomState(0), fmt, 2, 2).shape[2:]
        shape = ((h * 3 // 2, w) if PIX_BYTES[fmt] == 1.5 else (h, w)) + shape
        sinks = [Sink(torch.zeros(shape, dtype=torch.uint8, device="cuda"), fmt, view="source" if src else "canvas") for _ in range(N)]
        q = np.stack([rng.randint(w // 8, w - w // 8, (N, 8)), rng.randint(h // 8, h - h // 8, (N, 8))], -1).astype(np.int32)
        pts, valid = torch.from_numpy(q).cuda(), torch.ones(N, dtype=torch.int32, device="cuda")
        if src:                                  # device-resident camera frames; their table comes from one ingest into a small canvas
            imgs = [Frame(torch.from_numpy(picture_array(rng, src[0], h, w)).cuda(), src[0]) for _ in range(N)]
            _, staged = ingest_frames_keep(imgs, torch.zeros((N, 16, 32, 3), dtype=torch.uint8, device="cuda"),
                                           torch.zeros((N, 3, 3), device="cuda"))
            call = lambda: emit_source_frames(staged, pts, valid, sinks)
        else:
            imgs = torch.from_numpy(rng.randint(0, 256, (N, h, w, 3)).astype(np.uint8)).cuda()
            call = lambda: emit_frames(imgs, pts, valid, sinks)
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.launches
        b = case_bytes(cases[name])
        print(f"{name}: {us:.1f} us per call (events, table upload included), {b / 1e6:.1f} MB -> {b / us / 1e6:.2f} TB/s", flush=True)
        del imgs, sinks


if __name__ == "__main__":
    main()
