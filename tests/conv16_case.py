"""Operands, float64 reference, CPU restatement and grading of the cases of tests/conv16_sweep.py (no GPU here: tests/test_conv16_sweep_cpu.py
grades the restatement, tests/test_conv16_sweep_gpu.py the kernels, both through grade()).

Operands are drawn as tests/test_conv16w_edges_gpu.py draws them (uniform activations, filters scaled by 3 / sqrt(taps Cin), bias up to
0.2); every image carries its own scale, so a sum filed under a neighbour's statistics group or a row read from the next image shows.  In
a 16-bit mode the operands are rounded first and the reference convolves the rounded values; pairs are split from the fp32 operands and
the reference convolves those (the bars' own tests do the same)."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import conv16_sweep as S
import ref_ops

T16 = {1: torch.bfloat16, 2: torch.float16, 3: torch.float16}


def build_shims(tmp):
    """The host builds of the two geometry headers (tests/conv16w_geom_shim.cpp, tests/corr16_geom_shim.cpp) -> {"conv", "corr"} ctypes libraries."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    libs = {}
    for key, src in (("conv", "conv16w_geom_shim.cpp"), ("corr", "corr16_geom_shim.cpp")):
        so = os.path.join(tmp, src.replace(".cpp", ".so"))
        subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(here, src), "-o", so], check=True)
        libs[key] = C.CDLL(so)
    libs["conv"].g_halo_tiling.argtypes = [C.c_int] * 5 + [C.c_void_p, C.POINTER(C.c_int)]
    libs["corr"].g_pick_grid.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)]
    return libs


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def split(x):
    hi = x.to(torch.float16)
    return torch.stack([hi, (x - hi.float()).to(torch.float16)], -2).contiguous()


def operands(case):
    c = case
    corr = c["fam"] == "C"
    taps = c["kd"] ** 2 if corr else 9 * c["kd"]
    g = torch.Generator().manual_seed(c["seed"])
    w = _rand(g, c["Cout"], taps, c["Cin"], scale=(3.0 / (taps * c["Cin"])) ** 0.5 if corr else (1.0 / (taps * c["Cin"])) ** 0.5 * 3)
    b = None if corr else _rand(g, c["Cout"], scale=0.2)
    xs = []
    for N, D, H, W in c["segs"]:
        x = _rand(g, N, D, H, W, c["Cin"])
        xs.append(x * (1.0 + 0.5 * torch.arange(N) / N).view(N, 1, 1, 1, 1))
    mode = c["mode"]
    if mode != 3:
        w, xs = w.to(T16[mode]).float(), [x.to(T16[mode]).float() for x in xs]
    # the inputs in the kernel's format: [N, D, H, W, Cin] of the 16-bit type, pairs [N, D, H, W, 2, Cin]
    x16 = [split(x) if mode == 3 else x.to(T16[mode]) for x in xs]
    return SimpleNamespace(case=c, corr=corr, taps=taps, w=w, b=b, xs=xs, x16=x16, mode=mode, pair=mode == 3)


def _conv(o, x, dt):
    c = o.case
    if o.corr:
        k = c["kd"]
        w = o.w.to(dt).reshape(c["Cout"], k, k, c["Cin"]).permute(0, 3, 1, 2)
        return F.conv2d(x[:, 0].to(dt).permute(0, 3, 1, 2), w, None, padding=k // 2).permute(0, 2, 3, 1)[:, None]
    if c["kd"] == 1:
        w = o.w.to(dt).reshape(c["Cout"], 3, 3, c["Cin"]).permute(0, 3, 1, 2)
        return F.conv2d(x[:, 0].to(dt).permute(0, 3, 1, 2), w, o.b.to(dt), padding=1).permute(0, 2, 3, 1)[:, None]
    w = o.w.to(dt).reshape(c["Cout"], 3, 3, 3, c["Cin"]).permute(0, 4, 1, 2, 3)
    return F.conv3d(x.to(dt).permute(0, 4, 1, 2, 3), w, o.b.to(dt), padding=1).permute(0, 2, 3, 4, 1)


def reference(o):
    """float64: per segment the full map [N, D, H, W, Cout] (after the ReLU) and its 2x2 max-pool, the statistics table [G, Cout, 2] of the
    launch (every segment adds to the groups of its own pixel indices), the range of each segment and of the launch."""
    c = o.case
    fulls, pools = [], []
    G = S.stat_groups(c)
    stats = torch.zeros((G, c["Cout"], 2), dtype=torch.float64) if G else None
    for x in o.xs:
        y = _conv(o, x, torch.float64)
        if c["relu"]:
            y = F.relu(y)
        fulls.append(y)
        pools.append(F.max_pool2d(y[:, 0].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)[:, None] if c["pool"] else None)
        if G:
            flat = y.reshape(-1, c["Cout"])
            grp = (torch.arange(flat.shape[0]) // c["rpg"]) if c["rpg"] else torch.zeros(flat.shape[0], dtype=torch.long)
            stats[:, :, 0].index_add_(0, grp, flat)
            stats[:, :, 1].index_add_(0, grp, flat * flat)
    rngs = [float(y.abs().max()) for y in fulls]
    return SimpleNamespace(fulls=fulls, pools=pools, stats=stats, rngs=rngs, rng=max(rngs), count=c["rpg"] or S.pixels(c))


def restatement(o):
    """The kernel's own arithmetic on the CPU: tests/ref_ops.py conv16_direct_multi / corr16_multi on the values of the rounded or split
    operands, outputs coded as the launch codes them -> (fulls, pools, stats) as the launch returns them.  ref_ops convolves in the
    filters' dtype.  16-bit modes: fp32, the kernels' accumulator type.  Pairs: float64 taps, i.e. the split operands' products summed
    exactly — torch's fp32 convolution adds the K = taps x Cin products of an output in one or a few chains and is 1.0e-6 .. 2.8e-6 of
    range off at K = 576 .. 21600 (measured: profiles/r35_conv16_sweep.md), above what the matrix cores lose (they add 16 products at a
    time before the fp32 accumulator sees them) and above the pair bar itself, so it restates nothing of the pair kernels; the suite's
    earlier sweep (tests/test_conv_sweep_cpu.py) leaves its pair family out of the fp32 grading for the same reason."""
    c = o.case
    wt = o.w.double() if o.pair else o.w
    if o.corr:
        filt = ref_ops.corr16_pack(wt, o.mode)
        outs = [torch.empty(x.shape[:4] + (32,), dtype=torch.float32) for x in o.xs]
        ref_ops.corr16_multi([x[:, 0] for x in o.x16], filt, [t[:, 0] for t in outs])
        return outs, [None] * len(outs), None
    filt = ref_ops.conv16_pack(wt, o.mode, c["layout"])
    G = S.stat_groups(c)
    stats = torch.zeros((G, c["Cout"], 2), dtype=torch.float64) if G else None
    kind = {None: None, "t16": "t16", "f32": torch.float32}
    xs = [x[:, 0] for x in o.x16] if c["kd"] == 1 else o.x16
    fulls, pools = ref_ops.conv16_direct_multi(xs, filt, o.b, relu=bool(c["relu"]), full=kind[c["full"]], pool=kind[c["pool"]], kd=c["kd"], stats=stats,
                                               rows_per_group=c["rpg"])
    return fulls, pools, stats


def value(t, kind, pair, Cout):
    """An output as the launch coded it -> float64 values [..., Cout]."""
    t = t.detach().cpu()
    if pair and kind == "t16":
        if t.shape[-1] == 2 * Cout:                      # rows [hi plane | lo plane]
            return t[..., :Cout].double() + t[..., Cout:].double()
        return t[..., 0, :].double() + t[..., 1, :].double()
    return t.double()


def bars_of(case):
    if case["fam"] == "C":
        return S.BARS["corr-pairs" if case["mode"] == 3 else "corr-b16"]
    return S.BARS["pairs" if case["mode"] == 3 else "b16"]


def grade(case, ref, fulls, pools, stats, arith=1.0):
    """-> (worst error / bar, [failures]).  arith scales the ARITHMETIC part of every bar (the conditioning check halves it); the half
    ulp a 16-bit output format adds on top stays whole — an exact result rounded once already uses all of it."""
    bar = bars_of(case)
    mode, Cout = case["mode"], case["Cout"]
    ulp = bar.get("ulp", 0.0)
    ulp = ulp[mode] if isinstance(ulp, dict) else ulp
    worst, bad = 0.0, []

    def check(what, e, tol):
        nonlocal worst
        ratio = e / tol
        worst = max(worst, ratio) if ratio == ratio else float("inf")
        if not e <= tol:                                     # (NaN — an output pixel never written — fails here)
            bad.append(f"{case['id']}: {what} error {e:.3e} > {tol:.3e}")
    for i, rng in enumerate(ref.rngs):
        for name, kind, got, want in (("full", case["full"], fulls[i], ref.fulls[i]), ("pool", case["pool"], pools[i], ref.pools[i])):
            if kind is None:
                continue
            v = value(got, kind, mode == 3, Cout).reshape(want.shape)
            check(f"segment {i} {name}", float((v - want).abs().max()) / rng, bar["map"] * arith + (ulp if kind == "t16" else 0.0))
    if ref.stats is not None:
        got = stats.detach().cpu()
        check("statistics: sums", float((got[..., 0] - ref.stats[..., 0]).abs().max()) / ref.count / ref.rng, bar["stat1"] * arith)
        check("statistics: squares", float((got[..., 1] - ref.stats[..., 1]).abs().max()) / ref.count / ref.rng ** 2, bar["stat2"] * arith)
    return worst, bad
