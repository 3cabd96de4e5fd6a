"""The frame-ingest kernels alone (csrc/ingest.hip): 32 device-resident frames per launch, two cases:

  nv12-1080p   32 x (1080x1920 NV12 -> 540x960 canvas)
  rgb-same     32 x (480x640 rgb24 -> 480x640 canvas)

and with --lens two more, the same frames with a strong lens (brown -0.35 0.12 0.001 -0.0005 -0.02, f = 1000 / 333) through the mesh path
of g6d_frame_ingest_mesh (nv12-1080p-lens, rgb-same-lens), and nv12-1080p-mixed: 31 plain frames and one lens frame, so that the plain
frames take the plain tile of the lens kernel; and the cases of g6d_frame_ingest_area (minify="area") side by side:
nv12-1080p-area and nv12-2160p-area (32 x 2160x3840 NV12 -> 540x960) without a lens, nv12-1080p-lens-in-area (the lens with its default
setting inside an area call: the mesh rule), nv12-2160p-lens (the mesh rule at 4:1) and, with Lens(minify="area"), nv12-1080p-lens-area
(n = 2) and nv12-2160p-lens-area (n = 4).  G6D_LIB_PATH selects another build of the library (tools/toolenv.py).  --formats a,b,.. adds one case per named pixel format (any of ingest.FORMATS):
<format>-1080p, 32 x (1080x1920 frames of that format -> 540x960 canvas).  --rounds R runs the cases R times in turn (variants alternate; the table gives the
spread of the rounds' medians).

Bytes are counted from shapes: the source rows a launch touches (every row of every plane, pixel bytes only) plus the canvas bytes it
writes.  Timing: device events around `--launches` back-to-back launches (includes the table upload of each call), or, under the profiler,
the kernel's own durations:

  python tools/ingest_bench.py [--launches 50] [--lens] [--rounds 3] [--formats nv12,bgr24,yuyv422,uyvy422,i420,yv12,p010,gray8]
  rocprofv3 --kernel-trace -d DIR -o ingest --output-format csv -- python tools/ingest_bench.py [--lens] [--rounds 3]
  python tools/ingest_bench.py --trace-csv DIR/.../ingest_kernel_trace.csv [--lens] [--rounds 3] [--tick-ms T] [--out FILE.md]
"""
import argparse
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 32
HBM_BPS = 6.3e12          # achievable HBM rate the shares are quoted against
CASES = {"nv12-1080p": dict(src=(1080, 1920), fmt="nv12", canvas=(540, 960)), "rgb-same": dict(src=(480, 640), fmt="rgb24", canvas=(480, 640))}
UHD = dict(src=(2160, 3840), fmt="nv12", canvas=(540, 960))
# minify: the call's setting; lens_minify: the setting of the frames' Lens
LENS_CASES = {"nv12-1080p-lens": dict(CASES["nv12-1080p"], lens=N), "rgb-same-lens": dict(CASES["rgb-same"], lens=N),
              "nv12-1080p-mixed": dict(CASES["nv12-1080p"], lens=1),
              "nv12-1080p-area": dict(CASES["nv12-1080p"], minify="area"),
              "nv12-1080p-lens-in-area": dict(CASES["nv12-1080p"], lens=N, minify="area"),
              "nv12-1080p-lens-area": dict(CASES["nv12-1080p"], lens=N, minify="area", lens_minify="area"),
              "nv12-2160p-area": dict(UHD, minify="area"), "nv12-2160p-lens": dict(UHD, lens=N),
              "nv12-2160p-lens-area": dict(UHD, lens=N, minify="area", lens_minify="area")}
BROWN = (-0.35, 0.12, 0.001, -0.0005, -0.02)
WARM = 3


# source bytes per pixel: every sample of every plane
SRC_BYTES = {"rgb24": 3, "bgr24": 3, "rgba32": 4, "bgra32": 4, "nv12": 1.5, "yuyv422": 2, "uyvy422": 2, "i420": 1.5, "yv12": 1.5, "p010": 3, "gray8": 1}


def case_bytes(c):
    (h, w), (H, W) = c["src"], c["canvas"]
    return N * (int(h * w * SRC_BYTES[c["fmt"]]) + H * W * 3)


def frame_array(rng, fmt, h, w):
    """A noise picture of the format as the array ingest.Frame takes: [H,W,C] packed, [H*3/2, W] for the 4:2:0 formats (uint16 for p010)."""
    if fmt == "p010":
        return (rng.randint(0, 1024, (h * 3 // 2, w)) << 6).astype(np.uint16)
    shape = {"nv12": (h * 3 // 2, w), "i420": (h * 3 // 2, w), "yv12": (h * 3 // 2, w), "yuyv422": (h, w, 2), "uyvy422": (h, w, 2),
             "gray8": (h, w), "rgba32": (h, w, 4), "bgra32": (h, w, 4)}.get(fmt, (h, w, 3))
    return rng.randint(0, 256, shape).astype(np.uint8)


def trace_table(path, cases, launches, rounds, tick_ms):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "frame_ingest" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []                                           # one entry per call: g6d_frame_ingest_area with a mesh table is two kernels
    for r in rows:
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        name = re.search(r"frame_ingest\w*", r["Kernel_Name"]).group(0)
        if name == "frame_ingest_lens_area_kernel" and calls:
            calls[-1] = (calls[-1][0] + d, calls[-1][1] + " + " + name)
        else:
            calls.append((d, name))
    rows = calls
    out = ["| case | kernel | calls | kernel us per call (median) | min | max | medians of the rounds | bytes per launch | TB/s (median) | share of 6.3 TB/s | share of a tick |",
           "|---|---|---:|---:|---:|---:|---|---:|---:|---:|---:|"]
    per = WARM + launches
    for i, (name, c) in enumerate(cases.items()):
        mine = [rows[(r * len(cases) + i) * per + WARM:(r * len(cases) + i + 1) * per] for r in range(rounds)]
        if not all(len(m) == launches for m in mine):
            continue
        d = [np.array([r[0] for r in m]) for m in mine]
        kernels = sorted({r[1] for m in mine for r in m})
        alld = np.concatenate(d)
        b, med = case_bytes(c), float(np.median(alld))
        tick = f"{med / (tick_ms * 1e3):.2%}" if tick_ms else "-"
        out.append(f"| {name} | {' '.join(kernels)} | {len(alld)} | {med:.1f} | {alld.min():.1f} | {alld.max():.1f} | "
                   f"{' '.join(f'{np.median(x):.1f}' for x in d)} | {b / 1e6:.1f} MB | {b / med / 1e6:.2f} | "
                   f"{b / med / 1e6 / (HBM_BPS / 1e12):.1%} | {tick} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--lens", action="store_true", help="add the lens cases (g6d_frame_ingest_mesh) and the area cases (g6d_frame_ingest_area)")
    ap.add_argument("--only", default=None, help="comma list of case names: run (and parse) these alone, in this order")
    ap.add_argument("--rounds", type=int, default=1, help="run the cases this many times in turn")
    ap.add_argument("--formats", default=None, help="comma list of pixel formats: adds the case <format>-1080p for each")
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--tick-ms", type=float, default=0.0, help="tick time of the 32-stream tracker the kernel time is set against")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = dict(CASES, **LENS_CASES) if args.lens else dict(CASES)
    for fmt in (args.formats.split(",") if args.formats else []):
        cases.setdefault(f"{fmt}-1080p", dict(src=(1080, 1920), fmt=fmt, canvas=(540, 960)))
    if args.only:
        cases = {name: cases[name] for name in args.only.split(",")}
    if args.trace_csv:
        txt = trace_table(args.trace_csv, cases, args.launches, args.rounds, args.tick_ms)
        print(txt)
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n## The ingest kernel (rocprofv3 --kernel-trace, tools/ingest_bench.py)\n\n32 device-resident frames per launch; bytes = "
                        "source rows touched + canvas bytes, from shapes.\n\n" + txt + "\n")
        return
    import toolenv  # noqa: F401  (G6D_LIB_PATH)
    import torch
    from gen6d_amd.ingest import Frame, Lens, ingest_frames, ingest_frames_keep, plan
    if not torch.cuda.is_available():
        sys.exit("ingest_bench: needs the GPU (the kernel has no CPU fallback)")
    rng = np.random.RandomState(0)
    work = {}
    for name, c in cases.items():
        (h, w), (H, W) = c["src"], c["canvas"]
        f = 1000.0 * w / 1920
        K = np.array([[f, 0, w / 2 - 0.5], [0, f, h / 2 - 0.5], [0, 0, 1]])
        lens = Lens("brown", BROWN, minify=c.get("lens_minify", "point"))
        frames = [Frame(torch.from_numpy(frame_array(rng, c["fmt"], h, w)).cuda(), c["fmt"],
                        **(dict(K=K, lens=lens) if i < c.get("lens", 0) else {})) for i in range(N)]
        if c.get("lens_minify") == "area":
            out_h, out_w, _ = plan(frames[0], (H, W))
            nodes, lg = lens.mesh(K, w, h, 0, out_w, out_h)
            print(f"{name}: mesh step {1 << lg}, n = {1 << Lens.samples_log2(nodes, lg, w, h)}", flush=True)
        call = (lambda fr, o, k: ingest_frames_keep(fr, o, k, minify="area")) if c.get("minify") == "area" else ingest_frames
        work[name] = (frames, torch.zeros((N, H, W, 3), dtype=torch.uint8, device="cuda"), torch.zeros((N, 3, 3), device="cuda"), call)
    for _ in range(args.rounds):
        for name, (frames, out, K, call) in work.items():
            for _ in range(WARM):
                call(frames, out, K)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call(frames, out, K)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.launches
            b = case_bytes(cases[name])
            print(f"{name}: {us:.1f} us per call (events, table upload included), {b / 1e6:.1f} MB -> {b / us / 1e6:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
