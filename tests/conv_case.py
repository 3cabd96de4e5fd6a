"""One convolution case in the vocabulary of CONV_CASES (tests/test_kernels_gpu.py), shared by the hand-picked tables there and by the
descriptor sweep (tests/conv_sweep.py): the operands from a seeded generator, the float64 reference (tests/ref_ops.py), and the launch
through gen6d_amd.ops.conv with the checks of the per-kernel parity tests.

A case is a dict: N, D, H, W, Cin, Cout, k, s, p and optionally ld_in / ld_out (channel slices of wider rows; an input row wider than
Cin + 64 puts the view at channel 64), aff, relu, per_n, mul, mul_group, in_mod, act, stats, rpg, split.

Operand scaling (the bars of the callers were set on it): inputs, multipliers U(-1, 1); filters U(-1, 1) / sqrt(taps * Cin); bias
0.1 U(-1, 1); affine scale 0.5 + U(0, 1), shift 0.3 U(-1, 1)."""
from types import SimpleNamespace

import torch

import ref_ops

SENTINEL = -777.0


def rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def f64(t):
    return t.detach().cpu().double() if t is not None else None


def rel_err(got, want):
    """max |got - want| / max |want|: the metric of the per-kernel parity tests."""
    got, want = got.detach().cpu().double(), want.double()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def check(got, want, tol, what=""):
    err = rel_err(got, want)
    assert err <= tol, f"{what}: rel-to-max error {err:.3e} > {tol}"
    return err


def out_dims(c):
    return [(i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((c["D"], c["H"], c["W"]), c["k"], c["s"], c["p"])]


def operands(case, seed=17):
    """The CPU fp32 operands of a case (drawn in the order _run_conv_case always drew them) and its derived sizes."""
    g = torch.Generator().manual_seed(seed)
    c = case
    N, D, H, W, Cin, Cout = c["N"], c["D"], c["H"], c["W"], c["Cin"], c["Cout"]
    k = c["k"]
    ld_in, ld_out = c.get("ld_in", Cin), c.get("ld_out", Cout)
    Do, Ho, Wo = out_dims(c)
    in_mod, mul_group, per_n = c.get("in_mod", 0), c.get("mul_group", 0), int(c.get("per_n", 0))
    xbuf = rand(g, in_mod or N, D, H, W, ld_in)
    off = 64 if ld_in >= Cin + 64 else 0
    T = k[0] * k[1] * k[2]
    w = rand(g, Cout, T, Cin, scale=(1.0 / (T * Cin)) ** 0.5)
    bias = rand(g, Cout, scale=0.1)
    mul = (rand(g, (N + mul_group - 1) // mul_group, H, W, Cin) if mul_group else rand(g, H, W, Cin)) if c.get("mul") else None
    groups_in = (N + per_n - 1) // per_n if per_n else 1
    sc = (0.5 + torch.rand((groups_in, Cin), generator=g)) if c.get("aff") else None
    sh = rand(g, groups_in, Cin, scale=0.3) if c.get("aff") else None
    M = N * Do * Ho * Wo
    rpg = c.get("rpg", 0)
    return SimpleNamespace(case=c, N=N, Cin=Cin, Cout=Cout, ld_in=ld_in, ld_out=ld_out, Do=Do, Ho=Ho, Wo=Wo, in_mod=in_mod, mul_group=mul_group,
                           per_n=per_n, xbuf=xbuf, off=off, x=xbuf[..., off:off + Cin], w=w, bias=None if c.get("no_bias") else bias, mul=mul,
                           sc=sc, sh=sh, M=M, rpg=rpg, G=M // rpg if rpg else 1, count=float(rpg if rpg else M), stats=bool(c.get("stats")))


def reference(o, dtype=torch.float64):
    """ref_ops.conv of the operands in `dtype` -> (map [N,Do,Ho,Wo,Cout], statistics [G,Cout,2] float64 or None)."""
    c = o.case
    cast = (lambda t: None if t is None else t.detach().cpu().to(dtype))
    ref = torch.empty((o.N, o.Do, o.Ho, o.Wo, o.Cout), dtype=dtype)
    rstats = torch.zeros((o.G, o.Cout, 2), dtype=torch.float64) if o.stats else None
    ref_ops.conv(cast(o.x), cast(o.w), cast(o.bias), ref, ksize=c["k"], stride=c["s"], pad=c["p"], mul=cast(o.mul), in_scale=cast(o.sc),
                 in_shift=cast(o.sh), in_relu=bool(c.get("relu")), per_n=o.per_n, out_act=c.get("act", 0), stats=rstats,
                 rows_per_group=o.rpg, in_mod=o.in_mod, mul_group=o.mul_group)
    return ref, rstats


def wino_u(w_taps, k):
    from gen6d_amd.network.backbone import winograd_filters_taps
    return winograd_filters_taps(w_taps, k[0])


def device_operands(o, dev="cuda"):
    """The operands on the device, the output as a channel slice of a sentinel-filled buffer."""
    to = (lambda t: None if t is None else t.to(dev))
    xg = o.xbuf.to(dev)
    outbuf = torch.full((o.N, o.Do, o.Ho, o.Wo, o.ld_out), SENTINEL, device=dev)
    return SimpleNamespace(x=xg[..., o.off:o.off + o.Cin], w=to(o.w), bias=to(o.bias), mul=to(o.mul), sc=to(o.sc), sh=to(o.sh), outbuf=outbuf,
                           out=outbuf[..., :o.Cout])


def launch(ops, o, dv, stats, finalize=True, **extra):
    """ops.conv of the case on the device operands `dv` (extra: w_wino / w_wino43 / pairs)."""
    c = o.case
    return ops.conv(dv.x, dv.w, dv.bias, dv.out, ksize=c["k"], stride=c["s"], pad=c["p"], mul=dv.mul, in_scale=dv.sc, in_shift=dv.sh,
                    in_relu=bool(c.get("relu")), per_n=o.per_n, out_act=c.get("act", 0), stats=stats, rows_per_group=o.rpg,
                    split_k=c.get("split", 0), finalize=o.count if (stats is not None and finalize) else None,
                    in_mod=o.in_mod, mul_group=o.mul_group, **extra)


def run_conv_case(ops, case, wino):
    """The check of test_conv_igemm / test_conv_on_winograd_kernel and their kin: map and statistics against float64 within 2e-5 (4e-5
    with the Winograd filters), the sentinel columns of the output rows, the fused finalisation against the stand-alone kernel."""
    o = operands(case)
    dv = device_operands(o)
    stats = ops.new_stats(o.G, o.Cout, "cuda") if o.stats else None
    res = launch(ops, o, dv, stats, w_wino=wino_u(o.w, case["k"]).to("cuda") if wino else None)
    torch.cuda.synchronize()
    ref, rstats = reference(o)
    tol = 4e-5 if wino else 2e-5
    check(dv.out, ref, tol, "conv out")
    if o.ld_out != o.Cout:
        assert (dv.outbuf[..., o.Cout:] == SENTINEL).all(), "conv wrote outside its channel slice"
    if stats is not None:
        check(stats[..., 0], rstats[..., 0], tol, "stats sum")
        check(stats[..., 1], rstats[..., 1], tol, "stats sumsq")
        # the fused finalisation equals the stand-alone kernel on the same table, and the reference formula
        sc_f, sh_f = res
        sc_k, sh_k = ops.stats_finalize(stats, o.count)
        assert torch.equal(sc_f, sc_k) and torch.equal(sh_f, sh_k), "fused InstanceNorm finalisation differs from g6d_stats_finalize"
        rsc, rsh = ref_ops.stats_finalize(rstats, o.count)
        check(sc_f, rsc.double(), 1e-4, "finalised scale"); check(sh_f, rsh.double(), 1e-4, "finalised shift")
