"""The refiner's 2-D feature net per branch and per layer: today's fp32-core routes (F(4x4,3x3) / F(2x2,3x3) / implicit GEMM with the
InstanceNorm affine in the operand prologue and the finalisation fused into the producing launch) against the fp16 hi / lo pair route
(conv16w_kernel<3,.> + its hand-over passes), the launches of VolumeRefiner.run_feature_net timed one by one and as whole branches — each
through the product's own layer runner, hand-over pass and join (VolumeRefiner.run_layer / to_pairs / join) on the shapes of refiner.FEATNET.
    python tools/featnet_layers.py [crops=112]
us per launch, the best of three rounds of 10; a branch's time is its whole launch sequence back to back on one stream (what the step pays
when the kernels serialise).  The table decides the feature net's "pair" entries of refiner.ROUTES (profiles/r16_featnet_pairs.md); run it with 7 crops for the
single-query times (recorded for a later decision, not routed on)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import toolenv                                                  # noqa: E402,F401  (G6D_LIB_PATH / KNOBS)
from gen6d_amd import lib, ops, synth                           # noqa: E402
from gen6d_amd.network import name2network, refiner             # noqa: E402


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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 112
    dev = torch.device("cuda", 0)
    ops.USE_ARENA = False
    net = name2network["refiner"]({"name": "featnet_layers"}).eval()
    net.load_state_dict(synth.synth_state_dict("refiner"))
    net.to(dev)
    size = (128, 128)
    big = n >= refiner.F43_MIN_QUERIES * 7
    cores = refiner.resolve_routes(refiner.FEATNET, refiner.ROUTES, size, big, False, False, {})      # the fp32 cores' kernel per layer
    table = net.range_table()
    rng = lambda name: (table, table.slot(name))
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    reader = refiner.FEATNET.reader("featnet.cat")
    cat32 = f32(n, 1, *reader.edge(size), reader.cin)
    cat16 = ops.new_map16(n, *reader.edge(size), reader.cin, 3, dev, rng=rng("cat"))
    print(f"# {n} crops of 128x128: the feature net's launches, us per launch (best of 3 rounds of 10); convs with direct-form TFLOP/s")
    print("| branch | launch | fp32-core route | us | TFLOP/s | pair route | us | TFLOP/s |\n|---|---|---|---|---|---|---|---|")
    total = [0.0, 0.0]
    for l0, l1 in refiner.FEATNET.chains():                     # a branch: its two layers; the second one's dst = (c_off in cat, up-sampling factor)
        name, hw, ci, cm, co = l0.key.split(".")[1], l0.edge(size)[0], l0.cin, l0.cout, l1.cout
        c_off, factor = l1.dst or (0, 0)
        x32 = torch.rand((n, 1, hw, hw, ci), device=dev) - 0.5
        y0, y1 = f32(n, 1, hw, hw, cm), f32(n, 1, hw, hw, co)
        s0, s1 = ops.new_stats(n, cm, dev), ops.new_stats(n, co, dev)             # (taken once: no zero-fill inside the timed launches)
        aff = {}

        def old_c0():
            aff["a0"] = net.run_layer(l0, cores[l0.key], x32, y0, None, s0)

        def old_c1():
            aff["a1"] = net.run_layer(l1, cores[l1.key], y0, y1, aff["a0"], s1)

        def conv16(layer, xin, y, st, key):
            aff[key] = net.run_layer(layer, "pair", xin, y, None, st)

        x16 = {}

        def new_in():
            # (the tap's pass is run_feature_net's own, not a layer's: spelled out)
            x16["x"] = ops.l2norm_split16(x32[:, 0], 3, rng=rng(name + ".in")) if factor else cat16

        def new_mid():
            x16["mid"] = net.to_pairs(y0, aff["a0"], l1.pass_slot)

        def old_end():
            net.join(y1, aff["a1"], cat32, c_off, factor)

        def new_end():
            net.join(y1, aff["a1"], cat16, c_off, factor)

        fl0, fl1 = 2.0 * n * hw * hw * cm * 9 * ci, 2.0 * n * hw * hw * co * 9 * cm
        kern = lambda l: "F(4x4)" if cores[l.key] == "f43" else "F(2x2) / igemm"
        rows = [("tap", "l2norm_rows (in place)" if factor else "-", (lambda: ops.l2norm_rows(x32)) if factor else None, 0.0,
                 "l2norm_split16" if factor else "-", new_in if factor else None),
                (f"{name}.0 {ci}->{cm} @{hw}", kern(l0) + " +stats +finalize", old_c0, fl0, "conv16x3 +stats, stats_finalize",
                 lambda: conv16(l0, x16["x"], y0, s0, "a0")),
                ("IN affine + ReLU", "(operand prologue of .3)", None, 0.0, "affine_split16", new_mid),
                (f"{name}.3 {cm}->{co} @{hw}", kern(l1) + " aff +stats +finalize", old_c1, fl1, "conv16x3 +stats, stats_finalize",
                 lambda: conv16(l1, x16["mid"], y1, s1, "a1")),
                ("branch end", ("affine_act_pool" if factor == 1 else f"upsample_bilinear x{factor}") if factor else "-", old_end if factor else None, 0.0,
                 ("affine_split16_to" if factor == 1 else f"upsample_bilinear_split16 x{factor}") if factor else "-", new_end if factor else None)]
        new_in()                                                # (conv_out: the pair `cat`)
        olds, news = [r[2] for r in rows if r[2]], [r[5] for r in rows if r[5]]
        for what, on, of, fl, nn, nf in rows:
            to, tn = (timed(of) if of else None), (timed(nf) if nf else None)
            cell = lambda t, f: f"{t:.0f} | {f / t / 1e6:.0f}" if (t and f) else (f"{t:.0f} | " if t else "- | ")
            print(f"| {name} | {what} | {on} | {cell(to, fl)} | {nn} | {cell(tn, fl)} |", flush=True)
        to, tn = timed(lambda: [f() for f in olds]), timed(lambda: [f() for f in news])
        total[0] += to; total[1] += tn
        print(f"| **{name}** | **whole branch** | | **{to:.0f}** | | | **{tn:.0f}** | {'pairs faster' if tn < to else 'fp32 cores faster'} ({to / tn:.2f}x) |", flush=True)
        del x32, y0, y1
    print(f"| **sum of the branches** | | | **{total[0]:.0f}** | | | **{total[1]:.0f}** | {total[0] / total[1]:.2f}x |")


if __name__ == "__main__":
    main()
