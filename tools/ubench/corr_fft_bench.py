"""The frequency-domain correlation (gen6d_amd/csrc/corr_fft.hip) launch by launch beside the corr16_multi launch it replaces, on the
headline's pyramid (88x116 + 60x80 + 44x60 + 32x40 x 512 channels, 32 references, k = 15) at batches 1, 2, 4, 8, 16; then the whole route
at batch 16 against the query chunk.  Random ReLU'd maps; every figure is the mean of `reps` back-to-back launches between two events,
after one warm-up, repeated `rounds` times with the two routes alternated: min .. max over the rounds.
python tools/ubench/corr_fft_bench.py [reps] [rounds] [chunk]      (chunk: queries per launch in the per-launch table, default ops.CORR_FFT_CHUNK)"""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import toolenv  # noqa
from gen6d_amd import lib, ops
lib.load()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
chunk = int(sys.argv[3]) if len(sys.argv) > 3 else ops.CORR_FFT_CHUNK
sizes = [(88, 116), (60, 80), (44, 60), (32, 40)]
Cin = 512


def timed(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def span(v):
    return f"{min(v):.0f} .. {max(v):.0f}"


g = torch.Generator().manual_seed(1)
w = (torch.rand((32, 225, Cin), generator=g) * 2 - 1) * (3.0 / (225 * Cin)) ** 0.5
f3 = ops.corr16_pack(w.cuda(), 3)
sp = ops.corr_fft_spectra(w.cuda())
bins = 32 * 17
print("| batch | chunk | corr16_multi us | fwd us | gemm us | inv us | corr_fft sum us | fwd GB/s | gemm GB/s (TFLOP/s) | inv GB/s |\n|---|---|---|---|---|---|---|---|---|---|")
for B in (1, 2, 4, 8, 16):
    xs = [torch.relu(torch.rand((B, h, ww, Cin), generator=g) * 2 - 1) for h, ww in sizes]
    xg = [x.cuda() for x in xs]
    xp = [torch.stack([x.half(), (x - x.half().float()).half()], -2).contiguous().cuda() for x in xs]
    o16 = [torch.empty((B, 1, h, ww, 32), device="cuda") for h, ww in sizes]
    of = [torch.empty((B, 1, h, ww, 32), device="cuda") for h, ww in sizes]
    qc = min(B, chunk)
    tiles = 73 * qc
    X = torch.empty(bins * tiles * 2 * Cin, device="cuda")
    Y = torch.empty(bins * tiles * 64, device="cuda")
    t = {k: [] for k in ("c16", "fwd", "gemm", "inv")}
    for _ in range(rounds):
        t["c16"].append(timed(lambda: ops.corr16_multi(xp, f3, o16)))
        # one chunk of qc queries per launch; B / qc chunks make the call
        nch = -(-B // qc)
        t["fwd"].append(nch * timed(lambda: ops.corr_fft_fwd([x[:qc] for x in xg], X)))
        t["gemm"].append(nch * timed(lambda: ops.corr_fft_gemm(X, sp.data, Y, tiles, Cin)))
        t["inv"].append(nch * timed(lambda: ops.corr_fft_inv(Y, [o[:qc] for o in of])))
    tot = [a + b + c for a, b, c in zip(t["fwd"], t["gemm"], t["inv"])]
    nch = -(-B // qc)
    xb, yb = 4.0 * bins * tiles * 2 * Cin * nch, 4.0 * bins * tiles * 64 * nch
    inb = sum(x.numel() for x in xs) * 4.0
    m = lambda v: sum(v) / len(v)
    print(f"| {B} | {qc} | {span(t['c16'])} | {span(t['fwd'])} | {span(t['gemm'])} | {span(t['inv'])} | {span(tot)} | {(xb + inb) / m(t['fwd']) / 1e3:.0f} | "
          f"{(xb + yb + nch * sp.data.numel() * 4.0) / m(t['gemm']) / 1e3:.0f} ({2.0 * bins * tiles * nch * 2 * Cin * 64 / m(t['gemm']) / 1e6:.0f}) | "
          f"{(yb + inb / Cin * 32) / m(t['inv']) / 1e3:.0f} |", flush=True)
    if B == 16:
        err = max(float((a - b).abs().max()) for a, b in zip(ops.corr_fft_multi(xg, sp, of), o16)) / max(float(o.abs().max()) for o in o16)
        print(f"\nbatch 16: corr_fft_multi against corr16_multi {err:.2e} of range\n\n| chunk | corr_fft_multi us (batch 16) |\n|---|---|")
        for ch in (2, 4, 8, 13):
            print(f"| {ch} | {span([timed(lambda: ops.corr_fft_multi(xg, sp, of, chunk=ch)) for _ in range(rounds)])} |", flush=True)
