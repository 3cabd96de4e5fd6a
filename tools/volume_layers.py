"""The 32^3 stage of the refiner's volume net launch by launch: today's fp32-core route (F(4x4,3x3) with the depth taps folded, the
InstanceNorm affine in the operand prologue and the finalisation fused into the producing launch) against the fp16 hi / lo pair route
(conv16w_kernel<3, ., 1, 3> with depth-folded filters + its hand-over passes), with the volume construction in front of both and conv2
(16^3) as a candidate — every layer through the product's own layer runner, hand-over pass and join (VolumeRefiner.run_layer / to_pairs /
join) on the shapes of refiner.VOLUME.
    python tools/volume_layers.py [volumes=16]
us per launch, the best of three rounds of 10, convs with direct-form TFLOP/s.  The table decides the volume net's "pair" entries of
refiner.ROUTES (profiles/r17_volume_pairs.md); run it with 1 volume for the single-query times (recorded, not routed on)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import toolenv                                                  # noqa: E402,F401  (G6D_LIB_PATH / KNOBS)
from gen6d_amd import lib, ops, synth                           # noqa: E402
from gen6d_amd.network import name2network, refiner             # noqa: E402
from featnet_layers import timed                                # noqa: E402


def main():
    lib.load()
    qn = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    sn = 32
    dev = torch.device("cuda", 0)
    ops.USE_ARENA = False
    net = name2network["refiner"]({"name": "volume_layers"}).eval()
    net.load_state_dict(synth.synth_state_dict("refiner"))
    net.to(dev)
    V = refiner.VOLUME
    big = qn >= refiner.F43_MIN_QUERIES
    cores = refiner.resolve_routes(V, refiner.ROUTES, (sn,) * 3, big, False, False, {})               # the fp32 cores' kernel per layer
    table = net.range_table()
    rng = lambda name: (table, table.slot(name))
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    vox = sn ** 3
    c = synth.refiner_case()
    rep = lambda t: t.expand(qn, *t.shape[1:]).contiguous().to(dev)
    feats = torch.rand((qn, c["ref_imgs"].shape[1] + 1, 32, 32, 128), device=dev) - 0.5
    views = (feats, rep(c["ref_Ks"]), rep(c["ref_poses"]), rep(c["Ks_in"]), rep(c["poses_in"]), refiner._linspace(sn, dev), 128, 128)
    mean32, std32 = f32(qn, vox, 256), f32(qn, vox, 128)
    cat32 = f32(qn, sn, sn, sn, 128)
    cat16 = ops.new_map16(qn * sn, sn, sn, 128, 3, dev, rng=rng("cat"))
    v16 = {}
    print(f"# {qn} volumes of 32^3: the launches of the volume net's 32^3 stage, us per launch (best of 3 rounds of 10); convs with direct-form TFLOP/s")
    print("| part | launch | fp32-core route | us | TFLOP/s | pair route | us | TFLOP/s |\n|---|---|---|---|---|---|---|---|")
    cell = lambda t, f: f"{t:.0f} | {f / t / 1e6:.0f}" if (t and f) else (f"{t:.0f} | " if t else "- | ")
    total = [0.0, 0.0]

    def row(part, what, on, of, fl, nn, nf):
        to, tn = (timed(of) if of else None), (timed(nf) if nf else None)
        print(f"| {part} | {what} | {on} | {cell(to, fl)} | {nn} | {cell(tn, fl)} |", flush=True)
        return to or 0.0, tn or 0.0

    def new_volumes():
        v16["mean"], v16["std"] = ops.refiner_volume_kp_pairs(*views, rng_mean=rng("mean_in"), rng_std=rng("std"))

    to, tn = row("volumes", "mean_in, std", "refiner_volume_kp (fp32)", lambda: ops.refiner_volume_kp(*views, mean32, std32), 0.0,
                 "refiner_volume_kp_pairs", new_volumes)
    total[0] += to; total[1] += tn
    mean32.uniform_(-0.5, 0.5); std32.uniform_(0.0, 0.5)

    def conv32(x, layer, y, st=None, aff=None):                # (st: taken once, no zero-fill inside the timed launches)
        return net.run_layer(layer, cores[layer.key], x, y, aff, st)

    def conv16(x, layer, y, st=None):
        return net.run_layer(layer, "pair", x, y, None, st)

    kern = "F(4x4)" if big else "F(2x2)"
    for (l0, l1), x32, key in zip(V.chains(), (mean32, std32), ("mean", "std")):           # the two embeds; l1.dst = (c_off in cat, 1)
        name, ci, c_off = l0.key.split(".")[1], l0.cin, l1.dst[0]
        x32 = x32.view(qn, sn, sn, sn, ci)
        y0, y1 = f32(qn, sn, sn, sn, l0.cout), f32(qn, sn, sn, sn, l1.cout)
        s0 = ops.new_stats(qn, l0.cout, dev)
        aff = {}

        def old_c0():
            aff["a"] = conv32(x32, l0, y0, st=s0)

        def old_c1():
            conv32(y0, l1, cat32[..., c_off:c_off + 64], aff=aff["a"])

        def new_c0():
            aff["b"] = conv16(v16[key].view(qn, sn, sn, sn, 2, ci), l0, y0, st=s0)

        def new_mid():
            v16["mid"] = net.to_pairs(y0, aff["b"], l1.pass_slot)

        def new_c1():
            conv16(v16["mid"].view(qn, sn, sn, sn, 2, 64), l1, y1)

        def new_c1_f32cat():
            conv16(v16["mid"].view(qn, sn, sn, sn, 2, 64), l1, cat32[..., c_off:c_off + 64])

        def new_end():
            net.join(y1, None, cat16, c_off, 1)

        fl0, fl1 = 2.0 * qn * vox * 64 * 27 * ci, 2.0 * qn * vox * 64 * 27 * 64
        rows = [(f"{name}.0 {ci}->64", f"{kern} +stats +finalize", old_c0, fl0, "conv16x3 folded +stats, stats_finalize", new_c0),
                ("IN affine + ReLU", "(operand prologue of .3)", None, 0.0, "affine_split16", new_mid),
                (f"{name}.3 64->64", f"{kern} aff, into fp32 cat", old_c1, fl1, "conv16x3 folded -> fp32", new_c1),
                ("slice of pair cat", "-", None, 0.0, "affine_split16_to", new_end)]
        for what, on, of, fl, nn, nf in rows:
            row(name, what, on, of, fl, nn, nf)
        row(name, f"{name}.3 64->64 (variant)", "-", None, fl1, "conv16x3 folded -> slice of the fp32 cat (conv0 not on pairs)", new_c1_f32cat)
        to = timed(lambda: [old_c0(), old_c1()])
        tn = timed(lambda: [new_c0(), new_mid(), new_c1(), new_end()])
        tv = timed(lambda: [new_c0(), new_mid(), new_c1_f32cat()])
        total[0] += to; total[1] += tn
        print(f"| **{name}** | **both layers** | | **{to:.0f}** | | | **{tn:.0f}** | {'pairs faster' if tn < to else 'fp32 cores faster'} ({to / tn:.2f}x); "
              f"into the fp32 cat: {tv:.0f} |", flush=True)
        del y0, y1

    l = V.layer("volume.conv0")
    y, st = f32(qn, sn, sn, sn, 64), ops.new_stats(qn, 64, dev)
    cat32.uniform_(-0.5, 0.5)
    net.join(cat32, None, cat16, 0, 1)
    fl = 2.0 * qn * vox * 64 * 27 * 128
    to, tn = row("conv0", "conv0 128->64", f"{kern} +stats +finalize", lambda: conv32(cat32, l, y, st=st), fl, "conv16x3 folded +stats, stats_finalize",
                 lambda: conv16(cat16.view(qn, sn, sn, sn, 2, 128), l, y, st=st))
    total[0] += to; total[1] += tn
    print(f"| **32^3 stage with its volumes** | | | **{total[0]:.0f}** | | | **{total[1]:.0f}** | {total[0] / total[1]:.2f}x |", flush=True)

    # candidate: conv2 (128 -> 128 at 16^3) — today it takes conv1's affine in its operand prologue; on pairs that is one more pass
    s2 = sn // 2
    l = V.layer("volume.conv2")
    x2, y2 = torch.rand((qn, s2, s2, s2, 128), device=dev) - 0.5, f32(qn, s2, s2, s2, 128)
    st1, st2 = ops.new_stats(qn, 128, dev), ops.new_stats(qn, 128, dev)
    sc = torch.rand((qn, 128), device=dev) + 0.5
    sh = torch.rand((qn, 128), device=dev) - 0.5
    fl = 2.0 * qn * s2 ** 3 * 128 * 27 * 128
    N, H, W, ci, co, rows, D = refiner.admission_shapes(V, {l.key: ("pair",)}, qn, (sn,) * 3)[l.key]
    if ops.conv16_direct_plan(N, H, W, ci, co, 3, stats_rows=rows, D=D) == 1:
        def old2():
            conv32(x2, l, y2, st1, (sc, sh))

        def new2_in():
            v16["x2"] = net.to_pairs(x2, (sc, sh), l.pass_slot)

        def new2():
            conv16(v16["x2"], l, y2, st2)
        row("conv2 (candidate)", "IN affine + ReLU", "(operand prologue)", None, 0.0, "affine_split16", new2_in)
        to, tn = row("conv2 (candidate)", "conv2 128->128 @16^3", "F(2x2) aff +stats +finalize", old2, fl, "conv16x3 folded +stats, stats_finalize", new2)
        tb = timed(lambda: [new2_in(), new2()])
        print(f"| **conv2 (candidate)** | **with its pass** | | **{to:.0f}** | | | **{tb:.0f}** | {'pairs faster' if tb < to else 'fp32 cores faster'} ({to / tb:.2f}x) |", flush=True)
    else:
        print("| conv2 (candidate) | the pair kernel does not tile 16^3 planes at this batch | | | | | | |")


if __name__ == "__main__":
    main()
