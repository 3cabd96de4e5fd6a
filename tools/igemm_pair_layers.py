"""The layers the halo-patch pair kernel cannot express — stride 2, small volumes that need split-K, 1x1 — launch by launch: today's
fp32-core route (g6d_conv_igemm: conv_igemm_kernel<., MM = 0>, or F(2x2,3x3) for conv4) against the implicit-GEMM kernel's own fp16
hi / lo pair mode (conv_igemm_kernel<., MM = 3>, ops.conv(pairs=...)), at the bench's shapes — the volume layers (those of refiner.VOLUME
the halo-patch kernel cannot express) through the product's own layer runner, VolumeRefiner.run_layer, with the route forced.
    python tools/igemm_pair_layers.py [volumes / queries = 16]
us per launch, the best of three rounds of 10, with direct-form TFLOP/s.  The table decides the "igemmV" entries of refiner.ROUTES and
selector.SELECTOR_IGEMM_PAIR_LAYERS (profiles/r18_igemm_pairs.md): a layer is listed only where it is faster at 16; run it with 1 for
the single-query times (recorded, not routed on).
The five volume layers get a second table: the pair mode's three loader variants (ops.conv(pairs=(table, slot, variant))) — 3 splits both
operands in the loader, 4 copies filters the weight pack split, 5 copies both operands behind ONE affine_split16 pass, whose time is
included — each with the spread (max - min) of its three rounds.  A layer takes the fastest variant that beats its current route (the
one refiner.ROUTES names, else the fp32-core route) by more than the spread of the current route's rounds
(profiles/r22_igemm_presplit.md)."""
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


def timed3(fn, reps=10):
    """featnet_layers.timed with the spread: (best, max - min) of three rounds of `reps` launches, us per launch."""
    fn(); fn(); torch.cuda.synchronize()
    t = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / reps * 1e3)
    return min(t), max(t) - min(t)


def main():
    lib.load()
    qn = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    dev = torch.device("cuda", 0)
    ops.USE_ARENA = False
    net = name2network["refiner"]({"name": "igemm_pair_layers"}).eval()
    net.load_state_dict(synth.synth_state_dict("refiner"))
    net.to(dev)
    pn = 1 if qn > 1 else 0
    table = ops.RangeTable(dev)
    print(f"# {qn} volumes / queries: us per launch (best of 3 rounds of 10), direct-form TFLOP/s")
    print("| layer | shape | fp32-core route | us | TFLOP/s | pair route | us | TFLOP/s | |\n|---|---|---|---|---|---|---|---|---|")

    variants = []            # (name, {route: (us, spread)}) of the volume layers, printed as the second table

    def row(name, shape, on, of, nf, fl):
        to, tn = timed(of), timed(nf)
        print(f"| {name} | {shape} | {on} | {to:.1f} | {fl / to / 1e6:.0f} | conv_igemm pairs | {tn:.1f} | {fl / tn / 1e6:.0f} | "
              f"{'pairs faster' if tn < to else 'fp32 cores faster'} ({to / tn:.2f}x) |", flush=True)

    # the volume net's candidates (stride 2, or 8^3 and below); every layer takes the previous InstanceNorm's affine + ReLU in its operand
    # prologue (a table per volume) and adds its own sums with the fused finalize, as run_volume_net launches it
    for L in (L for L in refiner.VOLUME.layers if L.igemm):
        name, ci, co, stride, stats = L.key.split(".", 1)[1], L.cin, L.cout, L.stride, L.norm
        s, so = L.edge((32,) * 3)[0], L.edge((32,) * 3, out=True)[0]
        x = torch.rand((qn, s, s, s, ci), device=dev) - 0.5
        y = torch.empty((qn, so, so, so, co), dtype=torch.float32, device=dev)
        sc, sh = torch.rand((qn if pn else 1, ci), device=dev) + 0.5, torch.rand((qn if pn else 1, ci), device=dev) - 0.5
        st = ops.new_stats(qn, co, dev) if stats else None          # (taken once: no zero-fill inside the timed launches)

        def launch(pairs, L=L, x=x, y=y, sc=sc, sh=sh, st=st):
            net.run_layer(L, f"igemm{pairs}" if pairs else "cores", x, y, (sc, sh), st)
        fl = 2.0 * qn * so ** 3 * co * 27 * ci
        old = "F(2x2,3x3)" if L.wino else "conv_igemm fp32"
        row(name, f"{s}^3 -> {so}^3, {ci} -> {co}, s{stride}, aff{' stats' if stats else ''}", old, lambda: launch(False), lambda: launch(3), fl)
        variants.append((name, old, {r: timed3(lambda r=r: launch(r)) for r in (0, 3, 4, 5)}))
        del x, y

    routed = {k.split(".", 1)[1]: int(r[5:]) for k, rs in refiner.ROUTES.items() for r in rs if r.startswith("igemm")}
    print(f"\n# {qn} volumes: loader variants of the pair mode, us per launch (best of 3 rounds of 10) +- spread (max - min of the rounds); "
          "variant 5 includes its affine_split16 pass")
    print("| layer | fp32-core route | us | pairs 3 (split in the loader) | pairs 4 (filters pre-split) | pairs 5 (both pre-split, + pass) | "
          "current route | decision |\n|---|---|---|---|---|---|---|---|")
    total = {"current": 0.0, "chosen": 0.0}
    for name, old, t in variants:
        cur = routed.get(name, 0)
        best = min((4, 5, 3, 0), key=lambda r: t[r][0])
        take = best if (best != cur and t[cur][0] - t[best][0] > t[cur][1]) else cur
        total["current"] += t[cur][0]; total["chosen"] += t[take][0]
        label = {0: old, 3: "pairs 3", 4: "pairs 4", 5: "pairs 5"}
        print(f"| {name} | {old} | {t[0][0]:.1f} +- {t[0][1]:.1f} | {t[3][0]:.1f} +- {t[3][1]:.1f} | {t[4][0]:.1f} +- {t[4][1]:.1f} | "
              f"{t[5][0]:.1f} +- {t[5][1]:.1f} | {label[cur]} | {'stays on ' + label[cur] if take == cur else label[take] + f' ({t[cur][0] / t[take][0]:.2f}x)'} |")
    print(f"\nsum of the five layers: current routes {total['current']:.1f} us, table's choice {total['chosen']:.1f} us", flush=True)

    # the selector: fuse0, a 1x1 conv 768 -> 512 over qn * D hypothesis maps of 4x4 with per-query sums and the fused finalize; sp0 (516 ->
    # 512 over qn * D rows) as a candidate of the tail
    sel = name2network["selector"]({"name": "igemm_pair_layers", "selector_angle_num": 5}).eval()
    sel.load_state_dict(synth.synth_state_dict("selector", an=5))
    sel.to(dev)
    sp = sel._pack()
    D = 64 * 5
    grp = D if qn > 1 else 0
    cat = torch.rand((qn * D, 1, 4, 4, 768), device=dev) - 0.5
    y = torch.empty((qn * D, 1, 4, 4, 512), dtype=torch.float32, device=dev)
    st = ops.new_stats(qn, 512, dev)

    def fuse0(pairs):
        kw = {"pairs": (table, table.slot("fuse0"))} if pairs else {}
        ops.conv(cat, sp["fuse0"][0], sp["fuse0"][1], y, stats=st, finalize=D * 16, rows_per_group=grp * 16, **kw)
    row("fuse0", f"1x1 768 -> 512, {qn * D * 16} rows, stats", "conv_igemm fp32", lambda: fuse0(False), lambda: fuse0(True), 2.0 * qn * D * 16 * 512 * 768)
    from gen6d_amd.network.selector import FEAT_LD
    feats = torch.rand((qn * D, FEAT_LD), device=dev) - 0.5
    t0 = torch.empty((1, 1, 1, qn * D, 512), dtype=torch.float32, device=dev)
    if FEAT_LD % 8 == 0:
        def sp0(pairs):
            kw = {"pairs": (table, table.slot("sp0"))} if pairs else {}
            ops.conv(feats.view(1, 1, 1, qn * D, FEAT_LD), sp["sp0"][0], sp["sp0"][1], t0, out_act=1, **kw)
        row("sp0 (candidate)", f"1x1 {FEAT_LD} -> 512, {qn * D} rows", "conv_igemm fp32", lambda: sp0(False), lambda: sp0(True), 2.0 * qn * D * 512 * FEAT_LD)
    else:
        print(f"| sp0 (candidate) | 1x1 {FEAT_LD} -> 512 | the pair mode takes Cin % 8 == 0: stays | | | | | | |")


if __name__ == "__main__":
    main()
