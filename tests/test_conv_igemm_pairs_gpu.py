"""The implicit-GEMM kernel's own fp16 hi / lo pair mode (conv_igemm_kernel<., MM = 3>, G6dConv.math_mode 3, ops.conv(pairs=...)): the
loader splits both fp32 operands after the prologue, three v_mfma_f32_32x32x16_f16 per product.  Reference: the float64 convolution of
the fp32 operands with the prologue applied in float64.  Bars: the pair kernels' own — 2e-6 of the output range (test_conv16_gpu), sums
2e-6 (test_conv16w_depth_gpu: |sum error| / count / range, squares / range^2).  Every output sits in a wider buffer whose guard values
before and after must survive.  Shapes: the smallest that still reach every path — M no multiple of the block tile, even and odd edges
under stride 2, one and two K steps per tap, a partial channel tile, split-K off / automatic / forced, both affine prologues, the
position-major row order, the 64x64 and 128x64 tiles."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BAR = 2e-6
GUARD = 12345.0
PADF = 256


def _rand(g, *shape, scale=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


class Out:
    """A [N,Do,Ho,Wo,Cout] fp32 view inside a wider buffer of guard values."""

    def __init__(self, N, Do, Ho, Wo, Cout):
        self.n = N * Do * Ho * Wo * Cout
        self.buf = torch.full((self.n + 2 * PADF,), GUARD, dtype=torch.float32, device="cuda")
        self.map = self.buf[PADF:PADF + self.n].view(N, Do, Ho, Wo, Cout)

    def untouched(self):
        return bool((self.buf[:PADF] == GUARD).all()) and bool((self.buf[PADF + self.n:] == GUARD).all())


def _reference(x, w, b, k, stride, pad, aff=None, per_n=0, relu=False):
    """float64: prologue (affine per image group + ReLU), zero padding, convolution.  x [N,D,H,W,Cin], w [Cout,taps,Cin] -> [N,Do,Ho,Wo,Cout]"""
    xd = x.double()
    if aff is not None:
        sc, sh = aff
        if per_n:
            idx = torch.arange(x.shape[0]) // per_n
            xd = xd * sc.double()[idx][:, None, None, None, :] + sh.double()[idx][:, None, None, None, :]
        else:
            xd = xd * sc.double().view(1, 1, 1, 1, -1) + sh.double().view(1, 1, 1, 1, -1)
        if relu:
            xd = xd.clamp(min=0)
    w5 = w.double().reshape(w.shape[0], k[0], k[1], k[2], w.shape[2]).permute(0, 4, 1, 2, 3)
    y = F.conv3d(xd.permute(0, 4, 1, 2, 3), w5, b.double() if b is not None else None, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 4, 1).contiguous(), xd


def _run(x, w, b, k, stride, pad, table, slot, aff=None, per_n=0, relu=False, stats_groups=0, rows_per_group=0, split_k=0, finalize=None):
    from gen6d_amd import ops
    N, D, H, W, _ = x.shape
    Do, Ho, Wo = [(i + 2 * p - kk) // s + 1 for i, p, kk, s in zip((D, H, W), pad, k, stride)]
    out = Out(N, Do, Ho, Wo, w.shape[0])
    st = torch.zeros((stats_groups, w.shape[0], 2), dtype=torch.float64, device="cuda") if stats_groups else None
    sc, sh = (aff[0].cuda(), aff[1].cuda()) if aff is not None else (None, None)
    r = ops.conv(x.cuda(), w.cuda().contiguous(), b.cuda() if b is not None else None, out.map, ksize=k, stride=stride, pad=pad, in_scale=sc,
                 in_shift=sh, in_relu=relu, per_n=per_n, stats=st, rows_per_group=rows_per_group, split_k=split_k, finalize=finalize,
                 pairs=(table, table.slot(slot)))
    torch.cuda.synchronize()
    return out, st, r


def _table():
    from gen6d_amd import ops
    return ops.RangeTable(torch.device("cuda", 0))


def _err(out, ref):
    return float((out.map.cpu().double() - ref).abs().max()) / float(ref.abs().max())


S2 = [(8, 32, 64), (7, 64, 128), (7, 32, 72), (8, 64, 72)]


@pytest.mark.parametrize("size,cin,cout", S2, ids=[f"{s}cube-{a}to{b}" for s, a, b in S2])
def test_stride2_3d(size, cin, cout):
    """3x3x3, stride 2, pad 1 on 3 volumes (M = 3 * 4^3 = 192: one and a half 128-row tiles), even and odd edge, one and two K steps per
    tap, Cout 72 = one 64-channel tile and a partial one.  Two statistics groups would not divide 3 volumes: one group per volume."""
    g = torch.Generator().manual_seed(size * 1000 + cin + cout)
    x = _rand(g, 3, size, size, size, cin) * (1.0 + torch.arange(3).view(3, 1, 1, 1, 1))
    w = _rand(g, cout, 27, cin, scale=(1.0 / (27 * cin)) ** 0.5 * 3)
    b = _rand(g, cout, scale=0.2)
    ref, _ = _reference(x, w, b, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    t = _table()
    rows = ref.shape[1] * ref.shape[2] * ref.shape[3]
    out, st, _ = _run(x, w, b, (3, 3, 3), (2, 2, 2), (1, 1, 1), t, "a", stats_groups=3, rows_per_group=rows)
    e = _err(out, ref)
    rng = float(ref.abs().max())
    r3 = ref.reshape(3, rows, cout)
    e1 = float((st.cpu()[:, :, 0] - r3.sum(1)).abs().max()) / rows / rng
    e2 = float((st.cpu()[:, :, 1] - (r3 * r3).sum(1)).abs().max()) / rows / rng ** 2
    print(f"error / range {e:.3e}, sums {e1:.3e}, squares {e2:.3e} (bars {BAR:.0e})")
    assert e <= BAR, e
    assert e1 <= BAR and e2 <= BAR, (e1, e2)
    assert out.untouched(), "wrote outside the map"
    assert t.read()["a"] == float(x.abs().max()), "the record is the largest |operand|"


def test_split_k_agree():
    """3x3x3, stride 1 on 4^3, 64 -> 64, 3 volumes: split_k 1, automatic and forced 3 each hold the bar (so they agree within it)."""
    g = torch.Generator().manual_seed(7)
    x = _rand(g, 3, 4, 4, 4, 64)
    w = _rand(g, 64, 27, 64, scale=(1.0 / (27 * 64)) ** 0.5 * 3)
    b = _rand(g, 64, scale=0.2)
    ref, _ = _reference(x, w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    t = _table()
    outs = []
    for sk in (1, 0, 3):
        out, _, _ = _run(x, w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1), t, "a", split_k=sk)
        e = _err(out, ref)
        print(f"split_k {sk}: error / range {e:.3e}")
        assert e <= BAR, (sk, e)
        assert out.untouched()
        outs.append(out.map.cpu().double())
    rng = float(ref.abs().max())
    assert float((outs[0] - outs[1]).abs().max()) / rng <= BAR and float((outs[0] - outs[2]).abs().max()) / rng <= BAR


@pytest.mark.parametrize("per_n", [2, 0], ids=["table-per-group", "one-table"])
def test_affine_relu_prologue(per_n):
    """MODE 2 (a table per image group: 4 volumes, 2 per table) and MODE 1: affine with a NONZERO shift and ReLU in the loader; the taps in
    the padding contribute exactly zero (the reference pads after the prologue), 7^3 under stride 2."""
    g = torch.Generator().manual_seed(11 + per_n)
    x = _rand(g, 4, 7, 7, 7, 32)
    G = 2 if per_n else 1
    sc, sh = _rand(g, G, 32) + 1.5, _rand(g, G, 32) + 0.75
    w = _rand(g, 64, 27, 32, scale=(1.0 / (27 * 32)) ** 0.5 * 3)
    aff = (sc, sh) if per_n else (sc[0], sh[0])
    ref, xd = _reference(x, w, None, (3, 3, 3), (2, 2, 2), (1, 1, 1), aff=aff, per_n=per_n, relu=True)
    t = _table()
    out, _, _ = _run(x, w, None, (3, 3, 3), (2, 2, 2), (1, 1, 1), t, "a", aff=aff, per_n=per_n, relu=True)
    e = _err(out, ref)
    print(f"error / range {e:.3e}")
    assert e <= BAR, e
    assert out.untouched()
    # the record holds the operand AFTER the prologue (fp32 arithmetic of the loader: within an ulp or two of the float64 value)
    assert abs(t.read()["a"] - float(xd.abs().max())) <= 4e-7 * float(xd.abs().max())


def test_1x1_wide_reduction_stats_finalize():
    """1x1 with Cin 768 (24 K steps), 2 images of 4x4 = 32 rows (the 64x64 tile), Cout 64, statistics in two groups and the fused finalize."""
    g = torch.Generator().manual_seed(3)
    x = _rand(g, 2, 1, 4, 4, 768) * torch.tensor([1.0, 3.0]).view(2, 1, 1, 1, 1)
    w = _rand(g, 64, 1, 768, scale=(1.0 / 768) ** 0.5 * 3)
    b = _rand(g, 64, scale=0.2)
    ref, _ = _reference(x, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    t = _table()
    out, st, (fsc, fsh) = _run(x, w, b, (1, 1, 1), (1, 1, 1), (0, 0, 0), t, "a", stats_groups=2, rows_per_group=16, finalize=16)
    e = _err(out, ref)
    rng = float(ref.abs().max())
    r3 = ref.reshape(2, 16, 64)
    st = st.cpu()
    e1 = float((st[:, :, 0] - r3.sum(1)).abs().max()) / 16 / rng
    e2 = float((st[:, :, 1] - (r3 * r3).sum(1)).abs().max()) / 16 / rng ** 2
    print(f"error / range {e:.3e}, sums {e1:.3e}, squares {e2:.3e}")
    assert e <= BAR and e1 <= BAR and e2 <= BAR, (e, e1, e2)
    assert out.untouched()
    # the fused finalize is the fp32 rounding of the affine of the device's own fp64 sums
    mean = st[:, :, 0] / 16
    rs = 1.0 / torch.sqrt((st[:, :, 1] / 16 - mean * mean).clamp(min=0) + 1e-5)
    assert torch.allclose(fsc.cpu().double(), rs, rtol=2e-7, atol=0) and torch.allclose(fsh.cpu().double(), -mean * rs, rtol=2e-7, atol=1e-12)


@pytest.mark.parametrize("pm", [1, 0], ids=["position-major", "row-order"])
def test_position_major_tiles(pm, knob):
    """512 images of 4x4, 3x3 stride 1 with an affine prologue, split_k = 1: the shape meets every condition of the library's
    position-major rule (igemm_position_major in conv_igemm.hip: 2-D, stride 1, "same" padding, map <= 8x8, an affine prologue under knob
    conv_pm 1, un-split, N >= 4 tiles of 128 images — a forced split_k skips the tile policy, so the tile stays 128x64), so knob 1 runs the
    pair mode in position-major order and knob 0 in row order; both hold the bar.  g6d_conv_route (the launcher's own decision code)
    says which order the launch takes."""
    from gen6d_amd import ops
    knob("conv_pm", pm)
    g = torch.Generator().manual_seed(5)
    x = _rand(g, 512, 1, 4, 4, 32)
    sc, sh = _rand(g, 32) + 1.5, _rand(g, 32) * 0.5
    w = _rand(g, 64, 9, 32, scale=(1.0 / (9 * 32)) ** 0.5 * 3)
    ref, _ = _reference(x, w, None, (1, 3, 3), (1, 1, 1), (0, 1, 1), aff=(sc, sh), relu=True)
    ops.ROUTE = []
    try:
        out, _, _ = _run(x, w, None, (1, 3, 3), (1, 1, 1), (0, 1, 1), _table(), "a", aff=(sc, sh), relu=True, split_k=1)
        route, = ops.ROUTE
    finally:
        ops.ROUTE = None
    assert (route.family, route.bm, route.bn, route.splits) == (5, 128, 64, 1)
    assert route.position_major == pm, "the launch did not take the row order this case is about"
    e = _err(out, ref)
    print(f"conv_pm {pm}: error / range {e:.3e}")
    assert e <= BAR, e
    assert out.untouched()


def test_small_filters_hold_the_bar():
    """Filters scaled by 1e-3: unscaled, their lo parts would be fp16 subnormals; with the filter exponent (ops.pair_filter_exponent, the
    rule of ops.conv16_pack, carried in the descriptor) the bar holds.  (Checked once while developing: with the exponent forced to 0
    this case fails the bar.)"""
    from gen6d_amd import ops
    g = torch.Generator().manual_seed(13)
    x = _rand(g, 3, 7, 7, 7, 32)
    w = _rand(g, 64, 27, 32, scale=(1.0 / (27 * 32)) ** 0.5 * 3) * 1e-3
    assert ops.pair_filter_exponent(w) == 14
    ref, _ = _reference(x, w, None, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    out, _, _ = _run(x, w, None, (3, 3, 3), (2, 2, 2), (1, 1, 1), _table(), "a")
    e = _err(out, ref)
    print(f"error / range {e:.3e}")
    assert e <= BAR, e


def test_activation_exponent():
    """An activation exponent of 3 (the loader splits v * 2^-3 and folds 2^3 into the accumulator scale) gives the result of exponent 0
    within the bar, and the record still holds the UNSCALED maximum."""
    g = torch.Generator().manual_seed(17)
    x = _rand(g, 3, 8, 8, 8, 32)
    w = _rand(g, 64, 27, 32, scale=(1.0 / (27 * 32)) ** 0.5 * 3)
    b = _rand(g, 64, scale=0.2)
    ref, _ = _reference(x, w, b, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    t = _table()
    o0, _, _ = _run(x, w, b, (3, 3, 3), (2, 2, 2), (1, 1, 1), t, "a")
    t.set_exponents({"a": 3})
    t.clear()
    o3, _, _ = _run(x, w, b, (3, 3, 3), (2, 2, 2), (1, 1, 1), t, "a")
    rng = float(ref.abs().max())
    d = float((o3.map.cpu().double() - o0.map.cpu().double()).abs().max()) / rng
    print(f"exponent 3 against exponent 0 / range {d:.3e}; against float64 {_err(o3, ref):.3e}")
    assert d <= BAR and _err(o3, ref) <= BAR
    assert t.read()["a"] == float(x.abs().max())


def _desc(x, w, out, **kw):
    from gen6d_amd import lib, ops
    ws = ops.workspace(x.device)
    N, D, H, W, Cin = x.shape
    d = lib.G6dConv(in_=x.data_ptr(), weight=w.data_ptr(), out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel() * 4,
                    N=N, Di=D, Hi=H, Wi=W, Cin=Cin, ld_in=Cin, Do=D, Ho=H, Wo=W, Cout=w.shape[0], ld_out=w.shape[0], kd=1, kh=1, kw=1, sd=1, sh=1,
                    sw=1, math_mode=3)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_range_record_and_no_record():
    """An operand of 1e5 (outside the fp16 window at exponent 0) shows up in the record; with no G6dRange16 nothing is written."""
    from gen6d_amd import lib, ops
    g = torch.Generator().manual_seed(19)
    x = _rand(g, 2, 1, 4, 4, 64)
    x[1, 0, 2, 3, 17] = -1e5
    w = _rand(g, 64, 1, 64, scale=0.1)
    t = _table()
    _run(x, w, None, (1, 1, 1), (1, 1, 1), (0, 0, 0), t, "a")
    assert t.read()["a"] == 1e5
    assert ops.pair_out_of_window(t.read()["a"], 0)
    t.clear()
    xc, wc = x.cuda(), w.cuda()
    xc[1, 0, 2, 3, 17] = 0.5
    out = Out(2, 1, 4, 4, 64)
    d = _desc(xc, wc, out.map)
    lib.check(lib.load().g6d_conv_igemm_ex(C.byref(d), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "g6d_conv_igemm_ex")
    torch.cuda.synchronize()
    assert int(t.rec.abs().max()) == 0, "a launch without a range wrote a record"
    ref, _ = _reference(xc.cpu(), w, None, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    assert _err(out, ref) <= BAR and out.untouched()
    assert lib.load().g6d_conv_plan(C.byref(d)) == 5


def test_error_paths():
    """G6D_EINVAL with a message: math_mode 3 with weight_wino16, with a channel count the 16-bit K step does not take, with Cout <= 32,
    and a range on another math mode."""
    from gen6d_amd import lib
    L = lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros((1, 1, 4, 4, 64), device="cuda")
    w = torch.zeros((64, 1, 64), device="cuda")
    out = torch.zeros((1, 1, 4, 4, 64), device="cuda")
    t = _table()
    cases = [(_desc(x, w, out, weight_wino16=w.data_ptr()), "weight_wino16"),
             (_desc(x[..., :36].contiguous(), w[..., :36].contiguous(), out), "Cin % 8"),
             (_desc(x, w[:32].contiguous(), out[..., :32].contiguous()), "Cout > 32")]
    for d, word in cases:
        assert L.g6d_conv_igemm_ex(C.byref(d), None, stream) == -1
        assert word in L.g6d_last_error().decode(), L.g6d_last_error().decode()
    d = _desc(x, w, out, math_mode=0)
    assert L.g6d_conv_igemm_ex(C.byref(d), C.byref(t.arg(-1, 0)), stream) == -1 and "math_mode 3" in L.g6d_last_error().decode()
    torch.cuda.synchronize()
