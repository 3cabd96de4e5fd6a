"""Per-layer times of the halo-patch kernel alone (conv16w_kernel through g6d_conv16_direct_multi): the 14 trunk layers of
tools/conv16_bench.py (detector pyramid, refiner crops) and the selector's stack layers with their statistics epilogue, which no other
tool times.   python tools/conv16w_layers.py [batch=16] [pairs|fp16|bf16]
G6D_LIB_PATH=<ablation build> (tools/conv16w_ablate.sh) times that library instead: C16W_ABLATE=8 gives what a block costs outside its K loop."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import toolenv                                                  # noqa: E402,F401  (G6D_LIB_PATH / KNOBS)
from gen6d_amd import lib, ops                                  # noqa: E402


def timed(fn, reps=10):
    fn(); fn(); torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):                                          # the best of three rounds of `reps` launches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


def main():
    lib.load()
    lib.set_knob("conv16_halo", 1)
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    mode = sys.argv[2] if len(sys.argv) > 2 else "pairs"
    mm = {"pairs": 3, "fp16": 2, "bf16": 1}[mode]
    t16 = torch.bfloat16 if mm == 1 else torch.float16
    dev = torch.device("cuda", 0)
    pyr = [(352, 464), (240, 320), (176, 240), (128, 160)]          # the four scales of a 480x640 query after the first layer's pool
    # (tag, maps, Cin, Cout, full, pool, statistics: images per group or 0)
    specs = []
    for tag, div, ci, co, full, pool in [("pyr/2", 1, 64, 128, False, True), ("pyr/4", 2, 128, 256, True, False), ("pyr/4", 2, 256, 256, False, True),
                                         ("pyr/8", 4, 256, 512, True, False), ("pyr/8", 4, 512, 512, True, True), ("pyr/16", 8, 512, 512, True, False),
                                         ("pyr/16", 8, 512, 512, True, True)]:
        specs.append((tag, [(B, h // div, w // div) for h, w in pyr], ci, co, "t16" if full else None, "t16" if pool else None, 0))
    for tag, hw, ci, co, full, pool in [("crop/2", 64, 64, 128, False, True), ("crop/4", 32, 128, 256, True, False), ("crop/4", 32, 256, 256, True, True),
                                        ("crop/8", 16, 256, 512, True, False), ("crop/8", 16, 512, 512, True, True), ("crop/16", 8, 512, 512, True, False),
                                        ("crop/16", 8, 512, 512, True, False)]:
        specs.append((tag, [(7 * B, hw, hw)], ci, co, "t16" if full else None, "t16" if pool else None, 0))
    D = 320                                                          # hypothesis maps per query (64 references x 5 angles)
    for hw, ci, co in [(16, 64, 64), (8, 64, 128), (8, 128, 128), (4, 128, 256)]:
        specs.append(("sel", [(B * D, hw, hw)], ci, co, torch.float32, None, D))
    g = torch.Generator().manual_seed(1)
    print(f"# batch {B}, {mode}: conv16w_kernel per layer, us per launch (direct-form TFLOP/s); library {os.environ.get('G6D_LIB_PATH') or 'product build'}")
    print("| layer | maps | Cin -> Cout | outputs | us | TFLOP/s |\n|---|---|---|---|---|---|")
    tot = {"pyr": 0.0, "crop": 0.0, "sel": 0.0}
    for tag, shapes, ci, co, full, pool, gi in specs:
        w = (torch.rand((co, 9, ci), generator=g) * 2 - 1) * (1.0 / (9 * ci)) ** 0.5 * 3
        filt = ops.conv16_pack(w.to(dev), mm, 1)
        bias = torch.zeros(co, device=dev)
        xs = []
        for n, h, ww in shapes:
            x = torch.rand((n, h, ww, ci), device=dev)
            xs.append(torch.stack([x.half(), (x - x.half().float()).half()], -2).contiguous() if mm == 3 else x.to(t16))
            del x
        stats = torch.zeros((shapes[0][0] // gi, co, 2), dtype=torch.float64, device=dev) if gi else None
        rpg = gi * shapes[0][1] * shapes[0][2] if gi else 0
        outs = None
        if gi:                                                       # (the selector writes into one caller-held map)
            outs = [torch.empty((n, h, ww, co), device=dev) for n, h, ww in shapes]
        us = timed(lambda: ops.conv16_direct_multi(xs, filt, bias, relu=not gi, full=full, pool=pool, stats=stats, rows_per_group=rpg, out_full=outs))
        flops = sum(2.0 * n * h * ww * co * 9 * ci for n, h, ww in shapes)
        tot[tag.split("/")[0]] += us
        what = " ".join(k for k, on in (("full", full == "t16"), ("fp32", full is torch.float32), ("pool", pool), ("stats", gi)) if on)
        print(f"| {tag} | {'+'.join(f'{n}x{h}x{ww}' for n, h, ww in shapes)} | {ci} -> {co} | {what} | {us:.0f} | {flops / us / 1e6:.0f} |", flush=True)
        del xs, outs, stats
        torch.cuda.empty_cache()
    print(f"| **total us** | trunk (pyramid + crops) {tot['pyr'] + tot['crop']:.0f} | selector stacks {tot['sel']:.0f} | | {sum(tot.values()):.0f} | |")


if __name__ == "__main__":
    main()
