"""Reduced-precision matrix-core mode (G6dConv.math_mode / ops.math_mode: bf16 or fp16 operands, fp32 accumulation) — the
opt-in speed mode of BASELINE configs[2] ("bf16") and [4] ("fp16 MFMA convs").  It is graded separately from the fp32 path:
per kernel against the float64 reference with the operand-rounding bound of the type, per stage by arg-max equality with the
reference's own outputs plus the achieved logit error (recorded in the parity log, profiles/r02_parity.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gen6d_amd import synth
from parity_log import record
from test_networks_gpu import _net

pytestmark = pytest.mark.gpu

TOL = {"bf16": 2e-2, "fp16": 3e-3}        # relative to the output range: ~ 2^-8 / 2^-11 operand rounding, random signs


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


CASES = [
    dict(N=1, D=8, H=8, W=8, Cin=128, Cout=64, k=(3, 3, 3), s=1, p=(1, 1, 1)),                 # conv_igemm split-K or patch
    dict(N=1, D=16, H=16, W=16, Cin=64, Cout=64, k=(3, 3, 3), s=1, p=(1, 1, 1), aff=True),     # conv_patch 3-D
    dict(N=40, D=1, H=16, W=16, Cin=512, Cout=64, k=(1, 3, 3), s=1, p=(0, 1, 1), mul=True),    # conv_patch 2-D with product prologue
    dict(N=1, D=8, H=8, W=8, Cin=64, Cout=256, k=(3, 3, 3), s=2, p=(1, 1, 1)),                 # strided, generic kernel
    dict(N=1, D=1, H=1, W=320, Cin=516, Cout=512, k=(1, 1, 1), s=1, p=(0, 0, 0)),              # 1x1 tail GEMM, ragged Cin
]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_conv_lowp(mode, case):
    from gen6d_amd import ops
    c = case
    g = torch.Generator().manual_seed(7 + c["Cin"])
    kd, kh, kw = c["k"]
    x = _rand(g, c["N"], c["D"], c["H"], c["W"], c["Cin"])
    w = _rand(g, c["Cout"], kd * kh * kw, c["Cin"], scale=(1.0 / (kd * kh * kw * c["Cin"])) ** 0.5 * 3)
    b = _rand(g, c["Cout"], scale=0.2)
    mul = _rand(g, c["H"], c["W"], c["Cin"]) if c.get("mul") else None
    sc = (_rand(g, 1, c["Cin"]) * 0.5 + 1.0) if (c.get("aff") or c.get("mul")) else None
    sh = _rand(g, 1, c["Cin"], scale=0.3) if sc is not None else None
    st = (c["s"],) * 3
    Do, Ho, Wo = [(i + 2 * pp - kk) // c["s"] + 1 for i, kk, pp in zip((c["D"], c["H"], c["W"]), c["k"], c["p"])]
    out = torch.empty((c["N"], Do, Ho, Wo, c["Cout"]), device="cuda")
    cu = lambda t: t.cuda() if t is not None else None
    with ops.math_mode(mode):
        ops.conv(cu(x), cu(w), cu(b), out, ksize=c["k"], stride=st, pad=c["p"], mul=cu(mul), in_scale=cu(sc), in_shift=cu(sh),
                 in_relu=bool(c.get("aff")))
    xin = x.double()
    if mul is not None:
        xin = xin * mul.double()
    if sc is not None:
        xin = xin * sc.double().view(1, 1, 1, 1, -1) + sh.double().view(1, 1, 1, 1, -1)
        if c.get("aff"):
            xin = F.relu(xin)
    w5 = w.double().reshape(c["Cout"], kd, kh, kw, c["Cin"]).permute(0, 4, 1, 2, 3)
    ref = F.conv3d(xin.permute(0, 4, 1, 2, 3), w5, b.double(), stride=st, padding=c["p"]).permute(0, 2, 3, 4, 1)
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    record("test_conv_lowp", f"{mode} N={c['N']} {c['D']}x{c['H']}x{c['W']}x{c['Cin']}->{c['Cout']} k={c['k']}", err, TOL[mode], note="relative to range")
    assert err <= TOL[mode], err
    assert ops.MATH_MODE == 0                          # the context manager restores the default


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_corr2d_patch_lowp(mode):
    from gen6d_amd import ops
    g = torch.Generator().manual_seed(3)
    H, W, Cin, Cout, k = 30, 40, 512, 32, 15
    x = F.relu(_rand(g, 1, 1, H, W, Cin))
    w = F.relu(_rand(g, Cout, k * k, Cin))
    out = torch.empty((1, 1, H, W, Cout), device="cuda")
    with ops.math_mode(mode):
        ops.corr2d_patch(x.cuda(), w.cuda(), out, k)
    w4 = w.double().reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double()[0].permute(0, 3, 1, 2), w4, padding=k // 2)[0].permute(1, 2, 0)
    err = (out.cpu().double()[0, 0] - ref).abs().max().item() / ref.abs().max().item()
    record("test_corr2d_patch_lowp", f"{mode} 30x40x512 -> 32, 15x15", err, TOL[mode], note="relative to range")
    assert err <= TOL[mode], err


CORR16_CASES = [
    # segment sizes (N, H, W), Cin, Cout, k
    ([(1, 30, 40)], 512, 32, 15),                                      # one map, split over the units
    ([(2, 22, 29), (2, 15, 20), (1, 11, 15), (3, 8, 10)], 64, 32, 15),  # pyramid with batches, ragged tiles, short reduction (2 chunks)
    ([(8, 44, 58), (8, 30, 40)], 128, 20, 7),                          # batch of 8, fewer than 32 references, 7x7 level
    ([(1, 9, 33)], 32, 32, 3),                                         # one chunk, 3x3, a second column tile of one column
]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("sizes,Cin,Cout,k", CORR16_CASES)
def test_corr2d_patch16_multi(mode, sizes, Cin, Cout, k):
    """The 16-bit correlation kernel (corr16_patch_kernel via ops.corr2d_patch_multi in the reduced-precision mode: host-rounded
    unit-major filters, all kw weight tiles of a unit staged at once) against (a) the restatement of its arithmetic — inputs and
    filters rounded to the operand type, exact products, wide accumulation: tight — and (b) the float64 correlation of the
    unrounded operands with the rounding bound of the type."""
    from gen6d_amd import ops
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    g = torch.Generator().manual_seed(900 + Cin + k)
    w = _rand(g, Cout, k * k, Cin, scale=(1.0 / (k * k * Cin)) ** 0.5 * 3)
    xs_cpu = [F.relu(_rand(g, n, 1, h, ww, Cin)) for n, h, ww in sizes]
    xs = ops.alloc_like_segments([tuple(x.shape) for x in xs_cpu], torch.device("cuda"))
    outs = ops.alloc_like_segments([(n, 1, h, ww, Cout) for n, h, ww in sizes], torch.device("cuda"))
    for d_, x in zip(xs, xs_cpu):
        d_.copy_(x)
    wd = w.cuda()
    w4 = w.double().reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)
    w4r = w.to(dt).double().reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)
    for rep in range(2):                                   # twice: split counters re-armed
        for o in outs:
            o.fill_(float("nan"))
        with ops.math_mode(mode):
            ops.corr2d_patch_multi(xs, wd, outs, k)
            assert wd._g6d_c16[ops.MATH_MODE].dtype == dt     # the 16-bit filters were built and handed over
        for x, o in zip(xs_cpu, outs):
            xin = x[:, 0].permute(0, 3, 1, 2)
            ref = F.conv2d(xin.double(), w4, padding=k // 2).permute(0, 2, 3, 1)
            own = F.conv2d(xin.to(dt).double(), w4r, padding=k // 2).permute(0, 2, 3, 1)
            got = o.cpu().double()[:, 0]
            rng = ref.abs().max().item()
            e_own, e_ref = (got - own).abs().max().item() / rng, (got - ref).abs().max().item() / rng
            assert e_own <= 2e-5 and e_ref <= TOL[mode], (e_own, e_ref)
    record("test_corr2d_patch16_multi", f"{mode} {sizes} x{Cin} -> {Cout}, {k}x{k}", e_ref, TOL[mode], note="relative to range")


@pytest.mark.parametrize("mode,keep,hi", [("fp16", None, 0.25), ("fp16", (), 1.0), ("bf16", None, 4.0), ("bf16", (), 8.0)],
                         ids=["fp16-default-scheme", "fp16-nothing-kept", "bf16-default-keep-list", "bf16-nothing-kept"])
def test_selector_headline_lowp(golden, mode, keep, hi):
    """64 references x 5 rotations in the reduced-precision modes against the reference's own logits — the four synthetic queries of
    bench.py (tests/golden/pipeline_rows.npz), whose smallest top-2 margin is 0.038.  The bounds are TIED TO THE MARGIN as on the bench
    line (lo / hi in units of it).  The product's scheme — fp16 with the cfg default keep-list (query trunk and
    attention / predictor tail on fp32 operands, the InstanceNorm stacks on fp16); "bf16mix" on the bench line is this selector inside a
    bf16 pipeline — must keep every logit within a QUARTER of the margin: the arg-max is then equal by construction.  The other three
    document why: fp16 with nothing kept and bf16 (with or without the keep-list: every InstanceNorm-stack layer alone moves the logits by
    0.2-0.8 of the margin in bf16) are held to their type's rounding class only — UPPER bounds (a lower bound turns a better
    result into a failure); that they exceed the quarter bar on this box is recorded in the parity log, not asserted
    (profiles/r05_lowp_selector_sensitivity.md)."""
    g = golden("pipeline_rows")
    gl = g["logits"]
    top2 = np.sort(gl, 1)[:, -2:]
    margin = float((top2[:, 1] - top2[:, 0]).min())
    case = synth.selector_case(64, 5)
    cfg = {"math_mode": mode}
    if keep is not None:
        cfg["lowp_keep_fp32"] = keep
    net = _net("selector", **cfg)
    crops = synth.imgs_to_tensor(synth.synth_images(4, 128, 128, seed=200)).cuda()
    with torch.no_grad():
        net.extract_ref_feats(case["ref_imgs"].cuda(), case["ref_poses"].cuda(), case["object_center"].cuda(), case["object_vert"].cuda())
        got = net.compute_view_point_feats(crops)[0].cpu().numpy()
    err = float(np.abs(got - gl).max())
    record("test_selector_headline_lowp", f"{mode} keep={'default' if keep is None else keep} 64x5 logits of 4 queries vs reference golden "
           f"(smallest top-2 margin {margin:.4f})", err, hi * margin,
           note="" if hi <= 0.25 else f"informational: {err / margin:.2f} of the margin (the product scheme's bar is 0.25)")
    assert err <= hi * margin, (err / margin, hi)
    if hi <= 0.25:
        assert np.array_equal(got.argmax(1), gl.argmax(1)), (err, margin)


ALL_ROWS_SCHEMES = {   # name -> (context mode, selector cfg math_mode, refiner cfg math_mode, must hold the all-rows bar)
    "fp16ref32": ("fp16", None, "fp32", True),     # detector + selector fp16, refiner fp32: the scheme that holds every bar
    "fp16": ("fp16", None, None, False),           # BASELINE configs[4]: logits / position / scale hold, the synthetic refiner's pose heads do not
    "bf16": ("bf16", None, None, False),           # BASELINE configs[2] as it reads
}


@pytest.mark.parametrize("scheme", list(ALL_ROWS_SCHEMES))
def test_pipeline_all_rows_lowp(golden, scheme):
    """The ALL-ROWS bar of the reduced-precision modes (gen6d_amd/bars.py): every column of the [26]-wide result rows
    — detection position, scale, viewpoint index, angle and the 21 pose-head outputs of the three refinement steps — plus the selector
    logits, on the four bench queries AND on sixteen held-out queries nothing was tuned on (tests/golden/pipeline_rows_heldout.npz, outputs of
    the reference's own modules), against the reference's rows and against the fp32 path's.  `fp16ref32` must hold every bar.  `fp16` must
    hold the logit, viewpoint, position and scale bars on all 20 queries; its pose heads are recorded and bounded at 5e-2 only: every part of
    the synthetic refiner alone moves them by 0.6-1.6e-2 in fp16 (profiles/r06_lowp_refiner_sensitivity.md), the bar is 5e-3.  `bf16` is
    recorded with its type's bounds (it does not hold the logit bar; arg-max equality is not asserted)."""
    from gen6d_amd import bars, ops
    from gen6d_amd.pipeline import TensorPipeline
    mode, sel_mode, ref_mode, must_hold = ALL_ROWS_SCHEMES[scheme]
    dev = torch.device("cuda", 0)
    pipe = TensorPipeline(dev)
    pipe.build()
    sets = {}
    for tag, n, fs, cs, fn in (("bench4", 4, 100, 200, "pipeline_rows"), ("heldout16", 16, 300, 400, "pipeline_rows_heldout")):
        g = golden(fn)
        sets[tag] = (synth.imgs_to_tensor(synth.synth_images(n, 480, 640, seed=fs)).to(dev),
                     synth.imgs_to_tensor(synth.synth_images(n, 128, 128, seed=cs)).to(dev),
                     torch.from_numpy(np.asarray(g["rows"])).float(), torch.from_numpy(np.asarray(g["logits"])).float())
    with torch.no_grad():
        r32 = {t: pipe.query(v[0], v[1]).cpu() for t, v in sets.items()}
        l32 = {t: pipe.selector.compute_view_point_feats(v[1])[0].cpu() for t, v in sets.items()}
        pipe.selector.cfg["math_mode"], pipe.refiner.cfg["math_mode"] = sel_mode, ref_mode
        with ops.math_mode(mode):
            got = {t: (pipe.query(v[0], v[1]).cpu(), pipe.selector.compute_view_point_feats(v[1])[0].cpu()) for t, v in sets.items()}
    for t, v in sets.items():
        e32 = bars.row_errors(r32[t], v[2])
        assert e32["ref_idx_equal"] and e32["max_rel"] <= bars.FP32_REL and float((l32[t] - v[3]).abs().max()) <= bars.FP32_REL, (t, e32)
        b = bars.lowp_all_rows(got[t][0], v[2], r32[t], got[t][1], v[3])
        worst = max(b["vs_reference"]["pose_heads_rel"], b["vs_fp32_path"]["pose_heads_rel"])
        record("test_pipeline_all_rows_lowp", f"{scheme} {t}: pose heads rel (worst of vs reference / vs fp32 path)", worst, bars.LOWP_REL,
               note=f"ok_rows={b['ok_rows']} ok_logits={b['ok_logits']} position {b['vs_reference']['position_px']:.3f} px, scale(log2) "
                    f"{b['vs_reference']['scale_log2_rel']:.2e}, logits {b['logits']['worst_err_over_own_margin']:.3f} of own margin")
        if must_hold:
            assert b["ok"], (scheme, t, b)
        elif scheme == "fp16":
            assert b["ok_logits"] and b["vs_reference"]["ref_idx_equal"], (t, b["logits"])
            assert b["vs_reference"]["position_px"] <= bars.LOWP_POS_PX and b["vs_reference"]["scale_log2_rel"] <= bars.LOWP_REL, (t, b["vs_reference"])
            assert worst <= 5e-2, (t, worst)
        else:
            assert b["vs_reference"]["position_px"] <= 2.0 and worst <= 0.5, (t, b["vs_reference"])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_detector_headline_lowp(golden, mode):
    g = golden("det_head")
    net = _net("detector", math_mode=mode)
    case = synth.detector_case(32, 480, 640)
    with torch.no_grad():
        out = net({"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}})
    err = np.abs(out["scores"].cpu().numpy() - g["scores"]).max() / max(np.abs(g["scores"]).max(), 1.0)
    record("test_detector_headline_lowp", f"{mode} 480x640x32 scores vs reference golden", err, 5e-2, note="relative to range")
    assert np.array_equal(out["que_select_id"].cpu().numpy(), g["que_select_id"])
    assert err <= 5e-2


WINO16_CASES = [
    # segment sizes (N, H, W), Cin, Cout, relu, full, pool
    ([(1, 44, 58), (1, 30, 40), (1, 22, 30), (1, 16, 20)], 512, 512, False, True, True),     # detector pyramid, 1/16 level
    ([(2, 22, 30), (3, 16, 20)], 64, 128, True, False, True),                                # pooled output only, batches
    ([(2, 9, 7), (1, 8, 8), (3, 5, 13)], 128, 64, True, True, False),                        # ragged sizes
    ([(4, 64, 64)], 64, 128, True, False, True),                                             # selector / refiner first Winograd layer
    ([(7, 8, 8)], 512, 512, False, True, False),                                             # small maps: chunk split
    ([(8, 44, 58), (8, 30, 40), (5, 22, 30), (8, 16, 20)], 256, 256, True, True, True),      # batch-8 pyramid: un-split grid (two-wave kernel), masked quarters
    ([(24, 32, 32)], 128, 256, True, True, False),                                           # un-split, full output only
    ([(12, 16, 16)], 32, 64, True, True, True),                                              # two chunks: the request pipeline's shortest case
    ([(3, 16, 24)], 16, 64, False, True, False),                                             # one chunk
]


@pytest.mark.parametrize("kernel", ["two-waves", "one-wave"])       # knob wino16_2w: un-split launches on wino16b_conv3x3_kernel or not
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("sizes,Cin,Cout,relu,full,pool", WINO16_CASES)
def test_wino16_conv3x3_multi(mode, sizes, Cin, Cout, relu, full, pool, kernel, knob):
    knob("wino16_2w", 1 if kernel == "two-waves" else 0)
    """The trunk's 16-bit Winograd kernel (wino16_conv3x3_kernel: v_mfma_f32_32x32x16_{bf16,f16}, host-rounded filters) against
    (a) the restatement of its own arithmetic (tests/ref_ops.py: fp32 input transform rounded to the operand type, exact products,
    wide accumulation) — tight, and (b) the float64 convolution with the operand-rounding bound of the type."""
    import ref_ops
    from gen6d_amd import ops
    from gen6d_amd.network.backbone import winograd_filters16
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    g = torch.Generator().manual_seed(300 + Cin + Cout)
    w = _rand(g, Cout, Cin, 3, 3, scale=(2.0 / (9 * Cin)) ** 0.5 * 2)
    b = _rand(g, Cout, scale=0.2)
    U16 = winograd_filters16(w, dt)
    xs_cpu = [F.relu(_rand(g, n, h, ww, Cin)) for n, h, ww in sizes]
    xs = ops.alloc_like_segments([tuple(x.shape) for x in xs_cpu], torch.device("cuda"))
    for d_, x in zip(xs, xs_cpu):
        d_.copy_(x)
    for rep in range(2):                                   # twice: split counters re-armed
        ys, yps = ops.wino16_conv3x3_multi(xs, U16.cuda(), b.cuda(), relu=relu, full=full, pool=pool)
        rys, ryps = ref_ops.wino16_conv3x3_multi([x.double() for x in xs_cpu], U16, b, relu=relu, full=full, pool=pool)
        for i, x in enumerate(xs_cpu):
            ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)
            if relu:
                ref = F.relu(ref)
            refp = F.max_pool2d(ref, 2, 2).permute(0, 2, 3, 1)
            ref = ref.permute(0, 2, 3, 1)
            rng = ref.abs().max().item()
            if full:
                e_own = (ys[i].cpu().double() - rys[i].double()).abs().max().item() / rng
                e_ref = (ys[i].cpu().double() - ref).abs().max().item() / rng
                assert e_own <= 3e-4 and e_ref <= TOL[mode], (i, e_own, e_ref)
            if pool:
                e_own = (yps[i].cpu().double() - ryps[i].double()).abs().max().item() / rng
                e_ref = (yps[i].cpu().double() - refp).abs().max().item() / rng
                assert e_own <= 3e-4 and e_ref <= TOL[mode], (i, e_own, e_ref)
    record("test_wino16_conv3x3_multi", f"{mode} {sizes} {Cin}->{Cout}", e_ref, TOL[mode], note="relative to range")


# conv-family layers on the 16-bit Winograd kernel (G6dConv.weight_wino16): every operand prologue of the fp32 kernel, the depth fold,
# statistics + finalisation, query-batch addressing (image-group tables, shared input images, per-group multiplier maps)
WINO16_CONV_CASES = [
    dict(N=6, D=1, H=16, W=16, Cin=128, Cout=64),                                                # MODE 0, 2-D
    dict(N=5, D=1, H=13, W=18, Cin=64, Cout=128, aff=1, single=True, relu=True, stats=5),        # MODE 1 + statistics, ragged extents
    dict(N=12, D=1, H=16, W=16, Cin=128, Cout=64, aff=3, relu=True, stats=3),                    # MODE 2: a table per 3 images
    dict(N=12, D=1, H=16, W=16, Cin=256, Cout=64, aff=6, mul=6, in_mod=6, stats=6),              # MODE 3: query batch of 2 over 6 shared images
    dict(N=2, D=8, H=8, W=8, Cin=64, Cout=64, k3=True),                                          # 3x3x3, MODE 0
    dict(N=2, D=6, H=10, W=12, Cin=128, Cout=64, k3=True, aff=1, relu=True, stats=1),            # 3x3x3, table per volume, statistics
    dict(N=1, D=8, H=8, W=8, Cin=64, Cout=128, k3=True, aff=1, single=True, relu=True, stats=1),  # 3x3x3, one table
]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("case", WINO16_CONV_CASES)
def test_conv_wino16_family(mode, case, knob):
    import ctypes as C
    import ref_ops
    from gen6d_amd import ops
    from gen6d_amd.network.backbone import winograd_filters_taps
    knob("wino_min_work", 0)
    c = case
    g = torch.Generator().manual_seed(11 + c["Cin"] + c["N"])
    kd = 3 if c.get("k3") else 1
    N, D, H, W, Cin, Cout = c["N"], c["D"], c["H"], c["W"], c["Cin"], c["Cout"]
    in_mod, mul_g, per_n = c.get("in_mod", 0), c.get("mul", 0), c.get("aff", 0)
    x = _rand(g, in_mod or N, D, H, W, Cin)
    w = _rand(g, Cout, kd * 9, Cin, scale=(1.0 / (kd * 9 * Cin)) ** 0.5 * 3)
    b = _rand(g, Cout, scale=0.2)
    mul = _rand(g, N // mul_g, H, W, Cin) if mul_g else None
    G = (N + per_n - 1) // per_n if per_n else 0
    one = bool(c.get("single"))                                         # the single-table prologue (MODE 1)
    sc = (_rand(g, 1 if one else G, Cin) * 0.5 + 1.0) if per_n else None
    sh = _rand(g, 1 if one else G, Cin, scale=0.3) if per_n else None
    out = torch.empty((N, D, H, W, Cout), device="cuda")
    sg = c.get("stats", 0)
    stats = torch.zeros((N // sg, Cout, 2), dtype=torch.float64, device="cuda") if sg else None
    kw = dict(ksize=(kd, 3, 3), pad=(kd // 2, 1, 1), in_relu=bool(c.get("relu")), per_n=0 if one else per_n, in_mod=in_mod, mul_group=mul_g,
              rows_per_group=sg * D * H * W if sg else 0)
    cu = lambda t: t.cuda() if t is not None else None
    u = winograd_filters_taps(w, kd).cuda()
    with ops.math_mode(mode):
        fin = ops.conv(cu(x), cu(w), cu(b), out, mul=cu(mul), in_scale=cu(sc), in_shift=cu(sh), stats=stats, w_wino=u,
                       finalize=sg * D * H * W if sg else None, **kw)
        assert mode and u._g6d_u16                                    # the 16-bit filters were built and handed over
    ref = torch.empty((N, D, H, W, Cout), dtype=torch.float64)
    rstats = torch.zeros((N // sg, Cout, 2), dtype=torch.float64) if sg else None
    dbl = lambda t: t.double() if t is not None else None
    rfin = ref_ops.conv(dbl(x), dbl(w), dbl(b), ref, mul=dbl(mul), in_scale=dbl(sc), in_shift=dbl(sh), stats=rstats,
                        finalize=sg * D * H * W if sg else None, **kw)
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    record("test_conv_wino16_family", f"{mode} N={N} {D}x{H}x{W}x{Cin}->{Cout} kd={kd} aff={per_n} mul={mul_g} mod={in_mod} stats={sg}", err, TOL[mode],
           note="relative to range")
    assert err <= TOL[mode], err
    if sg:
        # statistics are sums over the kernel's own outputs: compare with the sums of what it wrote (fp64, tight), and the finalised
        # affine with the reference's loosely (it carries the operand rounding)
        o = out.cpu().double().reshape(N // sg, -1, Cout)
        np.testing.assert_allclose(stats[:, :, 0].cpu().numpy(), o.sum(1).numpy(), rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(stats[:, :, 1].cpu().numpy(), (o * o).sum(1).numpy(), rtol=1e-6, atol=1e-4)
        assert (fin[0].cpu().double() - rfin[0]).abs().max().item() <= 20 * TOL[mode] * rfin[0].abs().max().item()
