"""The fp16 hi / lo pair kernels (math_mode 3 / 4 / 5) on operands whose CHANNEL SCALES DIFFER: channel c of the activations times
top 2^-a[c], input channel c of the filters times 2^a[c] / top (tests/pair_format.py), so every product is that of the family's uniform
cases while the small channels sink to the lo plane's subnormal grid — the regime "error relative to the output range" on i.i.d. operands
never sees.  Every consumer launch is compared twice:

  (a) against pair_format.emulate, the kernels' arithmetic without rounding: the family's bar, 2e-6 of the output range (+ 2^-21 for a pair
      output).  Only fp32 accumulation separates the two; a kernel that loses, flushes or misplaces small-channel lo values fails here.
  (b) against the float64 convolution of the fp32 operands, elementwise: pair_format.bound + the bar; where the restatement itself lies
      within 2e-6 of the range (computed before the launch), also the family's plain bar.  The three figures go to the parity log.

Patterns "mixed" / "slice" / "outlier", spreads A = 4 and 12 binades, maps at the bottom of the keep window and at 1, all stored at
e = 0; one case per kernel stored high in the window (e = -12).  Then: the producers unmasked (every element within the format's delta of
the fp32 entry point's value), a chain of two pair layers, the fp32 kernels as controls on the same operands, and the detector under a
per-channel reparameterisation that leaves its function unchanged."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pair_format as pf
from gen6d_amd import synth
from parity_log import record
from test_split16_range_cpu import reparam_channels

pytestmark = pytest.mark.gpu

BAR = 2e-6                                   # test_conv16_gpu / test_conv_igemm_pairs_gpu
PAIR_ULP = 2.0 ** -21                        # added where the output is a pair map
TOPS = {"bottom": pf.TOP_BOTTOM, "1": 1.0}
SPREAD = [(p, A, t, 0) for p in pf.PATTERNS for A in (4, 12) for t in ("bottom", "1")] + [("mixed", 12, "1", -12)]
IDS = [f"{p}-A{A}-{t}" + ("-high" if e else "") for p, A, t, e in SPREAD]
spread = pytest.mark.parametrize("pattern,A,top,e", SPREAD, ids=IDS)


DEV = "cuda"


def _tag(pattern, A, top, e):
    return IDS[SPREAD.index((pattern, A, top, e))]


def _ops():
    from gen6d_amd import lib, ops
    lib.load()
    return ops


class Ref:
    """One (shape, pattern, A, top): the operands, the float64 convolution of them, and per exponent the restatement and its bound — each
    computed once and shared by every kernel and knob of the test."""

    def __init__(self, lead, Cin, Cout, k, pattern, A, top, stride=None, pad=None, bias=True):
        g = torch.Generator().manual_seed(1000 * len(lead) + 10 * Cin + Cout + A)
        k3 = (1, k, k) if isinstance(k, int) else k
        self.a = pf.exponents(pattern, Cin, A)
        self.x, self.w = pf.spread_operands(g, lead, Cin, Cout, k3[0] * k3[1] * k3[2], self.a, top=TOPS[top], relu=True)
        self.b = (torch.rand(Cout, generator=g) * 2 - 1) * 0.2 if bias else None
        self.geom = dict(k=k, stride=stride, pad=pad)
        self.ref = pf.conv64(self.x, self.w, bias=self.b, **self.geom)
        self._emu, self._bnd = {}, {}
        assert float(self.x.abs().max()) == float(np.float32(TOPS[top] * 2.0 ** -int(self.a.min())))

    def emu(self, e):
        if e not in self._emu:
            self._emu[e] = pf.emulate(self.x, self.w, e, bias=self.b, **self.geom)
        return self._emu[e]

    def bnd(self, e):
        if e not in self._bnd:
            self._bnd[e] = pf.bound(self.x, self.w, e, **self.geom)
        return self._bnd[e]

    def pair_input(self, e):
        """The map as a PairMap of exponent e: split(x 2^-e)."""
        ops = _ops()
        t = ops.RangeTable(torch.device(DEV))
        s = t.slot("x")
        t.set_exponents({"x": e})
        return ops.PairMap(pf.pairs_tensor(self.x, e).to(DEV), t, s)


def _pool(t):
    sh = t.shape
    return F.max_pool2d(t.reshape(-1, *sh[-3:]).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(*sh[:-3], sh[-3] // 2, sh[-2] // 2, sh[-1])


def _value(t):
    """An output as float64 on the CPU: fp32 as it is, a pair map [..., 2, C] as hi + lo."""
    t = t.detach().cpu()
    return t[..., 0, :].double() + t[..., 1, :].double() if t.dtype == torch.float16 else t.double()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _compare(test, what, got, R, e, relu=False, pool=False, pair_out=False):
    """Comparisons (a) and (b) of one output.  ReLU and max-pool are 1-Lipschitz: the bound of a pooled output is the largest bound of
    its window."""
    ref, emu, bnd = R.ref, R.emu(e), R.bnd(e)
    if relu:
        ref, emu = ref.clamp_min(0), emu.clamp_min(0)
    rng = float(ref.abs().max())
    if pool:
        ref, emu, bnd = _pool(ref), _pool(emu), _pool(bnd)
    got = _value(got).reshape(ref.shape)
    tol = BAR + (PAIR_ULP if pair_out else 0.0)
    d = (got - ref).abs()
    fa, fb, fr = float((got - emu).abs().max()) / rng, float(d.max()) / rng, float((emu - ref).abs().max()) / rng
    slack = float((d / (bnd + tol * rng)).max())
    print(f"{what}: kernel - restatement {fa:.2e}, kernel - float64 {fb:.2e}, restatement - float64 {fr:.2e} of range "
          f"(bar {tol:.2e}); worst |kernel - float64| / (bound + bar) {slack:.3f}")
    record(test, f"{what}: kernel - restatement / range", fa, tol)
    record(test, f"{what}: kernel - float64 / range", fb, tol if fr <= BAR else 0.0,
           note="elementwise bound asserted" + ("" if fr <= BAR else "; no bar on the maximum (tol 0): the format itself is beyond it"))
    record(test, f"{what}: restatement - float64 / range", fr, BAR, note="the format alone; recorded")
    assert bool(torch.isfinite(got).all()), f"{what}: an output element was never written or is not finite"
    assert fa <= tol, (what, "(a) kernel against the restatement", fa, tol)
    assert slack <= 1.0, (what, "(b) kernel against float64, elementwise", slack)
    if fr <= BAR:
        assert fb <= tol, (what, "(b) the plain bar, held where the restatement holds it", fb, tol)


# ---- consumers: conv16_direct_multi -------------------------------------------------------------------------------------------------------
def _conv16(R, e, filt, lead, relu, full, pool, kd=1):
    """One launch through ops; the full output lies in a NaN-filled tensor.  full / pool: None, "f32" or "t16"."""
    ops = _ops()
    ty = {None: None, "f32": torch.float32, "t16": "t16"}
    out = None
    if full is not None:
        out = [_nan((*lead, 2, filt.Cout), torch.float16) if full == "t16" else _nan((*lead, filt.Cout))]
    fulls, pools = ops.conv16_direct_multi([R.pair_input(e)], filt, R.b.to(DEV), relu=relu, full=ty[full], pool=ty[pool], kd=kd, out_full=out)
    torch.cuda.synchronize()
    return fulls[0], pools[0]


@spread
def test_conv16_2d_halo_and_per_tap(pattern, A, top, e, knob):
    """[(2, 16, 24)], 64 -> 128 on the halo-patch kernel and (knob conv16_halo 0) on the per-tap kernels: fp32 and pair full outputs,
    pooled pair and fp32 outputs."""
    ops = _ops()
    lead = (2, 16, 24)
    R = Ref(lead, 64, 128, 3, pattern, A, top)
    filt = ops.conv16_pack(R.w.to(DEV), 3, 1)
    for halo in (1, 0):
        knob("conv16_halo", halo)
        assert ops.conv16_direct_plan(*lead, 64, 128, 3) == halo, "the case no longer reaches the kernel it was written for"
        name = "halo-patch" if halo else "per-tap"
        f, p = _conv16(R, e, filt, lead, True, "f32", "t16")
        _compare("test_conv16_2d", f"{name} {_tag(pattern, A, top, e)} full fp32", f, R, e, relu=True)
        _compare("test_conv16_2d", f"{name} {_tag(pattern, A, top, e)} pool pairs", p, R, e, relu=True, pool=True, pair_out=True)
        f, p = _conv16(R, e, filt, lead, True, "t16", "f32")
        _compare("test_conv16_2d", f"{name} {_tag(pattern, A, top, e)} full pairs", f, R, e, relu=True, pair_out=True)
        _compare("test_conv16_2d", f"{name} {_tag(pattern, A, top, e)} pool fp32", p, R, e, relu=True, pool=True)


@spread
def test_conv16_two_tile_form(pattern, A, top, e, knob):
    """[(6, 8, 8)], 64 -> 64: the halo-patch kernel's two-tile blocks (three banded tiles: an odd count)."""
    ops = _ops()
    knob("conv16_halo", 1)
    lead = (6, 8, 8)
    R = Ref(lead, 64, 64, 3, pattern, A, top)
    assert ops.conv16_direct_plan(*lead, 64, 64, 3) == 1
    f, _ = _conv16(R, e, ops.conv16_pack(R.w.to(DEV), 3, 1), lead, False, "f32", None)
    _compare("test_conv16_two_tile_form", f"two-tile {_tag(pattern, A, top, e)} full fp32", f, R, e)


@spread
def test_conv16_per_tap_3d(pattern, A, top, e):
    """[(1, 8, 8, 8)], 64 -> 128, kd = 3 on the per-tap kernel (27-tap fragment-major filters)."""
    ops = _ops()
    lead = (1, 8, 8, 8)
    R = Ref(lead, 64, 128, (3, 3, 3), pattern, A, top)
    filt = ops.conv16_pack(R.w.to(DEV), 3, 1)
    f, _ = _conv16(R, e, filt, lead, False, "f32", None, kd=3)
    _compare("test_conv16_per_tap_3d", f"per-tap kd=3 {_tag(pattern, A, top, e)} full fp32", f, R, e)
    f, _ = _conv16(R, e, filt, lead, True, "t16", None, kd=3)
    _compare("test_conv16_per_tap_3d", f"per-tap kd=3 {_tag(pattern, A, top, e)} full pairs", f, R, e, relu=True, pair_out=True)


@spread
def test_conv16_depth_folded(pattern, A, top, e, knob):
    """The first D = 3 case of test_conv16w_depth_gpu: 2 volumes of 3 x 16 x 16, 32 -> 64, filter layout 2 (the depth taps folded into the
    reduction: three 32-channel slices per in-plane tap).  A 32-channel map IS one slice, so "slice" puts the whole map 2^-A down: hi
    partly and lo wholly on the subnormal grid."""
    ops = _ops()
    knob("conv16_halo", 1)
    lead = (2, 3, 16, 16)
    R = Ref(lead, 32, 64, (3, 3, 3), pattern, A, top)
    assert ops.conv16_direct_plan(2, 16, 16, 32, 64, 3, D=3) == 1, "the folded layer must take the halo-patch kernel"
    filt = ops.conv16_pack(R.w.to(DEV), 3, layout=2)
    f, _ = _conv16(R, e, filt, lead, False, "f32", None, kd=3)
    _compare("test_conv16_depth_folded", f"depth-folded {_tag(pattern, A, top, e)} full fp32", f, R, e)
    f, _ = _conv16(R, e, filt, lead, False, "t16", None, kd=3)
    _compare("test_conv16_depth_folded", f"depth-folded {_tag(pattern, A, top, e)} full pairs", f, R, e, pair_out=True)


# ---- consumers: corr16_multi --------------------------------------------------------------------------------------------------------------
# (g6d_corr16_multi takes k = 15 and k = 7 only — the detector's 3 x 3 level runs on corr2d_patch — so the ragged 9 x 33 map with 32
# channels runs at k = 7)
CORR = [((1, 20, 28), 64, 15), ((1, 20, 28), 64, 7), ((1, 9, 33), 32, 7)]


@spread
@pytest.mark.parametrize("lead,Cin,k", CORR, ids=[f"{l[1]}x{l[2]}x{c}-k{k}" for l, c, k in CORR])
def test_corr16(lead, Cin, k, pattern, A, top, e):
    ops = _ops()
    R = Ref(lead, Cin, 32, k, pattern, A, top, bias=False)
    out = _nan((lead[0], 1, lead[1], lead[2], 32))
    ops.corr16_multi([R.pair_input(e)], ops.corr16_pack(R.w.to(DEV), 3), [out])
    torch.cuda.synchronize()
    _compare("test_corr16", f"corr16 k={k} {lead[1]}x{lead[2]}x{Cin} {_tag(pattern, A, top, e)}", out[:, 0], R, e)


def test_corr16_has_no_3x3_form():
    """The 3 x 3 level is not a corr16 shape: the launcher refuses it before any launch.  Once it takes k = 3, the case belongs in CORR."""
    ops = _ops()
    R = Ref((1, 9, 33), 32, 32, 3, "mixed", 4, "1", bias=False)
    with pytest.raises(RuntimeError, match="k in"):
        ops.corr16_multi([R.pair_input(0)], ops.corr16_pack(R.w.to(DEV), 3), [_nan((1, 1, 9, 33, 32))])


# ---- consumers: ops.conv(pairs=(table, slot, variant)) ------------------------------------------------------------------------------------
IGEMM = [dict(id="3x3x3-s2", lead=(3, 8, 8, 8), Cin=32, Cout=64, k=(3, 3, 3), stride=(2, 2, 2), pad=(1, 1, 1)),
         dict(id="1x1", lead=(1, 1, 1, 64), Cin=96, Cout=72, k=(1, 1, 1), stride=(1, 1, 1), pad=(0, 0, 0))]


def _igemm(R, c, e, variant, w=None, **prologue):
    """ops.conv in the pair mode `variant` ("5p": a PairMap input some producer wrote) with the activations stored at exponent e; w: other
    filters than R.w."""
    ops = _ops()
    t = ops.RangeTable(torch.device(DEV))
    s = t.slot("a")
    t.set_exponents({"a": e})
    out = _nan(R.ref.shape)
    if variant == "5p":
        xin, variant = ops.PairMap(pf.pairs_tensor(R.x, e).to(DEV), t, s), 5
    else:
        xin = R.x.to(DEV)
    w = (R.w if w is None else w).to(DEV).contiguous()
    ops.conv(xin, w, R.b.to(DEV), out, ksize=c["k"], stride=c["stride"], pad=c["pad"], pairs=(t, s, variant), **prologue)
    torch.cuda.synchronize()
    return out, t


@spread
@pytest.mark.parametrize("c", IGEMM, ids=[c["id"] for c in IGEMM])
def test_conv_igemm_pair_variants(c, pattern, A, top, e):
    R = Ref(c["lead"], c["Cin"], c["Cout"], c["k"], pattern, A, top, stride=c["stride"], pad=c["pad"])
    for variant in (3, 4, 5) + (("5p",) if e else ()):
        out, t = _igemm(R, c, e, variant)
        _compare("test_conv_igemm_pair_variants", f"igemm {c['id']} variant {variant} {_tag(pattern, A, top, e)}", out, R, e)
        if variant != "5p":
            assert t.read()["a"] == float(R.x.abs().max()), "the record is the largest |operand|"


@pytest.mark.parametrize("variant", [3, 5])
def test_conv_igemm_prologue_is_immune(variant):
    """in_scale = 2^a[c] on activations 2^-a[c] down, uniform filters: the prologue runs BEFORE the split, so the layer sees uniform
    channels and holds the plain 2e-6 bar at A = 12 — what protects the InstanceNorm stacks, whose affine lives in the prologue."""
    c = IGEMM[0]
    R = Ref(c["lead"], c["Cin"], c["Cout"], c["k"], "mixed", 12, "1", stride=c["stride"], pad=c["pad"])
    gain = 2.0 ** R.a.double()
    w_uniform = (R.w.double() / gain).float()                      # exact: the products are those of R.ref
    assert torch.equal(w_uniform.double() * gain, R.w.double())
    out, t = _igemm(R, c, 0, variant, w=w_uniform, in_scale=gain.float().to(DEV), in_shift=torch.zeros(c["Cin"], device=DEV))
    rng = float(R.ref.abs().max())
    err = float((_value(out) - R.ref).abs().max()) / rng
    print(f"prologue immunity, variant {variant}: kernel - float64 {err:.2e} of range (bar {BAR:.0e}); at e = 0 without the prologue the "
          f"restatement is at {float((R.emu(0) - R.ref).abs().max()) / rng:.2e}")
    record("test_conv_igemm_prologue_is_immune", f"igemm variant {variant}, in_scale 2^a[c], A = 12: kernel - float64 / range", err, BAR)
    assert err <= BAR, err
    assert t.read()["a"] == 1.0, "the record holds the operand after the prologue"


# ---- producers, unmasked ------------------------------------------------------------------------------------------------------------------
def _table(e, *names):
    ops = _ops()
    t = ops.RangeTable(torch.device(DEV))
    slots = [t.slot(n) for n in names]
    t.set_exponents({n: e for n in names})
    t.clear()
    return (t, *slots)


def _check_producer(what, p, v, e, t=0.0):
    """EVERY element: |(hi + lo) 2^e - v| <= delta(v 2^-e) 2^e + t, v the fp32 entry point's values and t the producer's own fp32
    evaluation error (2^-22 x the magnitudes of the terms it adds; 0 where it splits a result the fp32 entry point gives bit for bit)."""
    data = p.data if hasattr(p, "table") else p
    vd = v.detach().cpu().double()
    got = _value(data).reshape(vd.shape) * 2.0 ** e
    assert float(vd.abs().max()) * 2.0 ** -e < 65504.0, "the case must fit fp16 at this exponent"
    lim = pf.delta(vd * 2.0 ** -e) * 2.0 ** e + (t.detach().cpu().double().reshape(vd.shape) if torch.is_tensor(t) else t)
    err = (got - vd).abs()
    worst = float((err / lim).max())
    small = vd.abs() < vd.abs().max() / 16
    print(f"{what} e={e}: worst error / bound {worst:.3f} over all {vd.numel()} elements ({int(small.sum())} of them below max / 16, "
          f"which the masked check skips)")
    record("test_producers_unmasked", f"{what} e={e}: worst |pairs - fp32 value| / (delta + t), every element", worst, 1.0)
    assert bool(torch.isfinite(got).all()), what
    assert bool(small.any()), f"{what}: the case holds no small-channel element"
    assert worst <= 1.0, (what, e, worst)


def _u(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


EXPS = pytest.mark.parametrize("e", [0, -12])


@EXPS
def test_producer_product_split16(e):
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    D, P, Cc, qn = 11, 40, 64, 2
    gain = pf.mixed_gains(Cc, 12)
    ref, que = _u(g, D, P, Cc), _u(g, qn, P, Cc)
    scale, shift = (0.5 + torch.rand((qn, Cc), generator=g)) * gain, _u(g, qn, Cc, scale=0.3) * gain
    prod = (ref[None].double() * que[:, None].double()) * scale[:, None, None].double()
    v = (prod + shift[:, None, None].double()).reshape(qn * D, P, Cc)
    t = 2.0 ** -22 * (prod.abs() + shift[:, None, None].double().abs()).reshape(qn * D, P, Cc)
    tb, s = _table(e, "x")
    p = ops.product_split16(ref.to(DEV), que.to(DEV), scale.to(DEV), shift.to(DEV), 3, rng=(tb, s))
    torch.cuda.synchronize()
    _check_producer("product_split16", p, v, e, t)


@EXPS
@pytest.mark.parametrize("pool", [False, True], ids=["full", "pool"])
def test_producer_affine_split16(e, pool):
    ops = _ops()
    g = torch.Generator().manual_seed(8)
    N, H, W, Cc = 3, 10, 12, 64
    gain = pf.mixed_gains(Cc, 12)
    x = _u(g, N, 1, H, W, Cc).to(DEV)
    scale, shift = ((0.5 + torch.rand((N, Cc), generator=g)) * gain).to(DEV), (_u(g, N, Cc, scale=0.3) * gain).to(DEV)
    v = torch.empty((N, 1, H // 2, W // 2, Cc) if pool else (N, 1, H, W, Cc), device=DEV)
    ops.affine_act_pool(x, v, scale, shift, per_n=True, relu=True, pool=1 if pool else 0)
    mag = x.abs().double() * scale.double()[:, None, None, None] + shift.abs().double()[:, None, None, None]
    t = 2.0 ** -22 * (_pool(mag[:, 0].cpu()) if pool else mag[:, 0].cpu())
    tb, s = _table(e, "x")
    p = ops.affine_split16(x, scale, shift, 1, True, pool, 3, rng=(tb, s))
    torch.cuda.synchronize()
    _check_producer(f"affine_split16 pool={int(pool)}", p, v[:, 0], e, t)


@EXPS
def test_producer_affine_split16_to_and_upsample(e):
    """The two slice producers into channels [64, 128) and [128, 192) of one pair map of 192 channels: the other slice keeps its NaNs."""
    ops = _ops()
    g = torch.Generator().manual_seed(9)
    N, Cc = 3, 64
    gain = pf.mixed_gains(Cc, 12)
    tb, s = _table(e, "cat")
    cat = ops.new_map16(N, 8, 8, 192, 3, torch.device(DEV), rng=(tb, s))
    cat.data.fill_(float("nan"))
    for i, (hw, f) in enumerate(((8, 1), (4, 2))):
        x = _u(g, N, 1, hw, hw, Cc, scale=2.0).to(DEV)
        scale, shift = ((0.5 + torch.rand((N, Cc), generator=g)) * gain).to(DEV), (_u(g, N, Cc, scale=0.3) * gain).to(DEV)
        v, mag = torch.empty((N, 1, 8, 8, Cc), device=DEV), torch.empty((N, 1, 8, 8, Cc), device=DEV)
        c_off = 64 * (i + 1)
        if f == 1:
            ops.affine_act_pool(x, v, scale, shift, per_n=True)
            ops.affine_act_pool(x.abs(), mag, scale, shift.abs(), per_n=True)
            ops.affine_split16_to(x, scale, shift, 1, False, 3, cat, c_off)
        else:
            ops.upsample_bilinear(x, v, f, scale, shift, per_n=True)
            ops.upsample_bilinear(x.abs(), mag, f, scale, shift.abs(), per_n=True)      # (positive weights: the sum of the terms' magnitudes)
            ops.upsample_bilinear_split16(x, cat, c_off, f, scale, shift, 1, 3)
        torch.cuda.synchronize()
        _check_producer("affine_split16_to" if f == 1 else "upsample_bilinear_split16", cat.data[..., c_off:c_off + Cc], v[:, 0], e,
                        2.0 ** -22 * mag[:, 0].double())
    assert bool(torch.isnan(cat.data[..., :64]).all()), "a slice producer wrote outside its channels"


@EXPS
def test_producer_l2norm_split16(e):
    ops = _ops()
    g = torch.Generator().manual_seed(10)
    Cc = 256
    x = (_u(g, 2, 3, 5, Cc) * pf.mixed_gains(Cc, 12)).to(DEV)
    x[0, 1, 2] = 0.0                                              # a zero pixel: the eps clamp
    v = ops.l2norm_rows(x.clone())
    tb, s = _table(e, "x")
    p = ops.l2norm_split16(x, 3, rng=(tb, s))
    torch.cuda.synchronize()
    _check_producer("l2norm_split16", p, v, e, 2.0 ** -22 * v.abs().double())    # (one multiplication by the row's 1 / norm)


@EXPS
def test_producer_vgg_conv1(e):
    ops = _ops()
    g = torch.Generator().manual_seed(6)
    gain = pf.mixed_gains(64, 12)
    x = torch.rand((1, 3, 64, 96), generator=g).to(DEV)
    w = (_u(g, 64, 3, 3, 3, scale=0.3) * gain[:, None, None, None]).to(DEV)
    b = (_u(g, 64, scale=0.1) * gain).to(DEV)
    v = ops.vgg_conv1_pool_nhwc(x, w, b)                           # the same kernel with an fp32 result: bit for bit (test_conv16_gpu)
    tb, s = _table(e, "x")
    p = ops.vgg_conv1_pool_nhwc16(x, w, b, mode=3, rng=(tb, s))
    torch.cuda.synchronize()
    _check_producer("vgg_conv1_pool_nhwc16", p, v, e)
    assert tb.read()["x"] == float(v.abs().max())


@EXPS
def test_producer_conv16_epilogue(e):
    """The pair epilogue of conv16_direct_multi (full and pooled) against the fp32 outputs of the same launch shape."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    gain = pf.mixed_gains(128, 12)
    x = pf.pairs_tensor(_u(g, 2, 16, 24, 64)).to(DEV)
    filt = ops.conv16_pack((_u(g, 128, 9, 64, scale=(3.0 / 576) ** 0.5) * gain[:, None, None]).to(DEV), 3)
    b = (_u(g, 128, scale=0.2) * gain).to(DEV)
    full, pool = ops.conv16_direct_multi([x], filt, b, relu=True, full=torch.float32, pool=torch.float32)
    tb, s = _table(e, "x")
    f16, p16 = ops.conv16_direct_multi([x], filt, b, relu=True, full="t16", pool="t16", rng=(tb, s))
    torch.cuda.synchronize()
    _check_producer("conv16 epilogue full", f16[0], full[0], e)
    _check_producer("conv16 epilogue pool", p16[0], pool[0], e)
    assert tb.read()["x"] == float(full[0].abs().max())


@EXPS
def test_producer_refiner_volume(e):
    """The small case of test_refiner_volume_pairs_gpu with per-channel gains on the feature maps.  t: the mean adds rfn sampled values
    (2^-22 of their magnitudes' mean); the deviation adds rfn differences s_r - mean (2^-22 x 2 rfn x that mean bounds their magnitudes)."""
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    B, rfn, fh, fw, Cc, sn, h_in, w_in = 2, 2, 6, 5, 12, 5, 24, 20
    feats = (_u(g, B, rfn + 1, fh, fw, Cc) * pf.mixed_gains(Cc, 12)).to(DEV)
    K = torch.tensor([[30.0, 0, w_in / 2], [0, 30.0, h_in / 2], [0, 0, 1]])
    ang = torch.tensor(0.3)
    R = torch.tensor([[torch.cos(ang), 0, torch.sin(ang)], [0, 1, 0], [-torch.sin(ang), 0, torch.cos(ang)]])
    pose = lambda tx, tz: torch.cat([R, torch.tensor([[tx], [0.1], [tz]])], 1)
    ref_Ks = K.expand(B, rfn, 3, 3).contiguous().to(DEV)
    ref_poses = torch.stack([torch.stack([pose(0.2 * (r + q), 2.5 + 0.5 * r) for r in range(rfn)]) for q in range(B)]).contiguous().to(DEV)
    K_in = K.expand(B, 3, 3).contiguous().to(DEV)
    pose_in = torch.stack([pose(-0.4 * q, 2.0) for q in range(B)]).contiguous().to(DEV)
    lin = torch.linspace(-1, 1, sn).to(DEV)
    vox = sn ** 3
    outs = []
    for f in (feats, feats.abs()):
        mean32, std32 = torch.empty((B, vox, 2 * Cc), device=DEV), torch.empty((B, vox, Cc), device=DEV)
        ops.refiner_volume_kp(f, ref_Ks, ref_poses, K_in, pose_in, lin, h_in, w_in, mean32, std32)
        outs.append((mean32, std32))
    (mean32, std32), (mag, _) = outs
    tb, sm, ss = _table(e, "mean", "std")
    pm, ps = ops.refiner_volume_kp_pairs(feats, ref_Ks, ref_poses, K_in, pose_in, lin, h_in, w_in, rng_mean=(tb, sm), rng_std=(tb, ss))
    torch.cuda.synchronize()
    _check_producer("refiner_volume mean_in", pm.data.view(B, vox, 2, 2 * Cc), mean32, e, 2.0 ** -22 * mag.double())
    _check_producer("refiner_volume std", ps.data.view(B, vox, 2, Cc), std32, e, 2.0 ** -22 * 2 * rfn * mag[..., :Cc].double())
    rec = tb.read()
    assert rec["mean"] == float(mean32.abs().max()) and rec["std"] == float(std32.abs().max())


# ---- a chain of two layers in pairs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("high", [False, True], ids=["e0", "high"])
def test_chain_of_two_pair_layers(high, knob):
    """[(2, 16, 24)], 64 -> 128 -> 128: layer 1's output channel c is 2^-a[c] down (filters and bias), layer 2's input channel c makes up
    for it.  The intermediate map is a PairMap written by the kernel under its own slot."""
    ops = _ops()
    knob("conv16_halo", 1)
    g = torch.Generator().manual_seed(21)
    a = pf.exponents("mixed", 128, 12)
    x, w1 = pf.spread_operands(g, (2, 16, 24), 64, 128, 9, torch.zeros(64), relu=True)
    w1 = (w1.double() * 2.0 ** -a.double()[:, None, None]).float()
    b1 = ((torch.rand(128, generator=g) * 2 - 1) * 0.2 * 2.0 ** -a.double()).float()
    w2 = ((torch.rand((128, 9, 128), generator=g) * 2 - 1).double() * (3.0 / (9 * 128)) ** 0.5 * 2.0 ** a.double()).float()
    b2 = (torch.rand(128, generator=g) * 2 - 1) * 0.2
    f1, f2 = ops.conv16_pack(w1.to(DEV), 3), ops.conv16_pack(w2.to(DEV), 3)
    x16 = pf.pairs_tensor(x).to(DEV)
    mid32, _ = ops.conv16_direct_multi([x16], f1, b1.to(DEV), relu=True, full=torch.float32)
    amax = float(mid32[0].abs().max())
    assert ops.pair_exponent(amax) == 0, "the guard sees nothing: the intermediate map's maximum lies in the keep window"
    e = pf.high_exponent(amax) if high else 0
    tb, s = _table(e, "mid")
    mid, _ = ops.conv16_direct_multi([x16], f1, b1.to(DEV), relu=True, full="t16", rng=(tb, s))
    out = [_nan((2, 16, 24, 128))]
    ops.conv16_direct_multi(mid, f2, b2.to(DEV), relu=False, full=torch.float32, out_full=out)
    torch.cuda.synchronize()
    assert tb.read()["mid"] == amax, "the recorded maximum is the fp32 intermediate's, bit for bit"
    # layer 1 against its restatement: the bar of the range, and — its products scale with the output channel — of every channel's range
    m32, m64 = mid32[0].cpu().double(), pf.conv64(x, w1, bias=b1).clamp_min(0)
    d1 = (m32 - pf.emulate(x, w1, 0, bias=b1).clamp_min(0)).abs()
    per_channel = float((d1.reshape(-1, 128).amax(0) / m64.reshape(-1, 128).amax(0)).max())
    print(f"chain e={e}: layer 1 kernel - restatement {float(d1.max()) / float(m64.max()):.2e} of range, {per_channel:.2e} of the channel's range at worst")
    assert per_channel <= BAR, ("layer 1, per channel", per_channel)
    # the intermediate map read back: the split of the fp32 intermediate at e, bit for bit
    stored = mid[0].data.cpu()
    assert torch.equal(stored.view(torch.int16), pf.pairs_tensor(mid32[0].cpu(), e).view(torch.int16)), "the stored pairs are not split(v 2^-e)"
    # the chained restatement: layer 2 without rounding on the planes layer 1 stored.  (Not on a float64 layer 1: where the lo plane is on
    # the subnormal grid the split of two intermediates an ulp apart differs by a whole grid step, which is the format's loss, not the
    # kernel's.)
    emu = pf.emulate_pairs(stored[..., 0, :].double(), stored[..., 1, :].double(), w2, e, bias=b2)
    ref = pf.conv64(pf.conv64(x, w1, bias=b1).clamp_min(0), w2, bias=b2)
    rng = float(ref.abs().max())
    got = _value(out[0])
    fa, fb, fr = float((got - emu).abs().max()) / rng, float((got - ref).abs().max()) / rng, float((emu - ref).abs().max()) / rng
    print(f"chain e={e}: kernel - restatement {fa:.2e}, kernel - float64 {fb:.2e}, restatement - float64 {fr:.2e} of range")
    for what, v, tol in (("kernel - restatement", fa, BAR), ("kernel - float64", fb, BAR if high else 0.0), ("restatement - float64", fr, BAR)):
        record("test_chain_of_two_pair_layers", f"chain 64 -> 128 -> 128, mixed A = 12, e = {e}: {what} / range", v, tol)
    assert bool(torch.isfinite(got).all())
    assert fa <= BAR, ("(a) against the chained restatement", fa)
    # (b): layer 1 keeps the bar per channel (its products scale with the channel), the bound of layer 2 on its fp32 input does the rest
    lim = pf.bound(mid32[0].cpu(), w2, e) + pf.conv64((m32 - m64).abs(), w2.abs()) + BAR * rng
    assert bool(((got - ref).abs() <= lim).all())
    if high:
        assert fb <= BAR, ("stored high in the window the plain bar holds against float64", fb)


# ---- controls: the fp32 kernels on the same operands --------------------------------------------------------------------------------------
def test_controls_fp32_kernels_are_scale_invariant():
    """The Winograd kernels, the implicit-GEMM kernel without pairs and corr2d_patch on the A = 12 "mixed" operands hold their own bars
    (test_kernels_gpu: 3e-5 / 2e-5 / 2e-5, test_wino43_gpu: 1e-5): the inputs are not ill-conditioned; fp32 arithmetic is scale-invariant
    per channel."""
    ops = _ops()
    from gen6d_amd.network.backbone import winograd43_filters, winograd_filters
    R = Ref((2, 16, 24), 64, 128, 3, "mixed", 12, "1")
    ref = R.ref.clamp_min(0)
    rng = float(ref.abs().max())
    w4 = R.w.reshape(128, 3, 3, 64).permute(0, 3, 1, 2).contiguous()
    xs = ops.alloc_like_segments([tuple(R.x.shape)], torch.device(DEV))
    xs[0].copy_(R.x)
    figures = {}
    ys, _ = ops.wino_conv3x3_multi(xs, winograd_filters(w4).to(DEV), R.b.to(DEV), relu=True, full=True, pool=False)
    figures["wino_conv3x3_multi"] = (float((_value(ys[0]) - ref).abs().max()) / rng, 3e-5)
    ys, _ = ops.wino43_conv3x3_multi(xs, winograd43_filters(w4).to(DEV), R.b.to(DEV), relu=True, full=True, pool=False)
    figures["wino43_conv3x3_multi"] = (float((_value(ys[0]) - ref).abs().max()) / rng, 1e-5)
    out = _nan((2, 1, 16, 24, 128))
    ops.conv(xs[0].view(2, 1, 16, 24, 64), R.w.to(DEV).contiguous(), R.b.to(DEV), out, ksize=(1, 3, 3), pad=(0, 1, 1), out_act=1)
    figures["conv (no pairs)"] = (float((_value(out[:, 0]) - ref).abs().max()) / rng, 2e-5)
    Rc = Ref((1, 20, 28), 64, 32, 15, "mixed", 12, "1", bias=False)
    outc = _nan((1, 1, 20, 28, 32))
    ops.corr2d_patch(Rc.x.to(DEV).view(1, 1, 20, 28, 64), Rc.w.to(DEV).contiguous(), outc, 15)
    torch.cuda.synchronize()
    figures["corr2d_patch k=15"] = (float((_value(outc[:, 0]) - Rc.ref).abs().max()) / float(Rc.ref.abs().max()), 2e-5)
    print(f"the pair restatement of the same operands at e = 0: 3 x 3 {float((R.emu(0) - R.ref).abs().max()) / float(R.ref.abs().max()):.2e}, "
          f"k = 15 {float((Rc.emu(0) - Rc.ref).abs().max()) / float(Rc.ref.abs().max()):.2e} of range")
    for name, (err, bar) in figures.items():
        print(f"control {name}: error / range {err:.2e} (bar {bar:.0e})")
        record("test_controls", f"{name}, mixed A = 12: error / range", err, bar)
    for name, (err, bar) in figures.items():
        assert err <= bar, (name, err, bar)


# ---- the detector under a per-channel reparameterisation ----------------------------------------------------------------------------------
MAPS = ("scores", "select_pr_offset", "select_pr_scale")


def _gains(A, lift=(1.0, 1.0)):
    return {2: pf.mixed_gains(256, A, lift[0]), 4: pf.mixed_gains(512, A, lift[1])}


def _detector(gains=None, **cfg):
    from test_networks_gpu import _net
    net = _net("detector", **cfg)
    if gains is not None:
        net.load_state_dict(reparam_channels(synth.synth_state_dict("detector"), gains))
    return net


def _detect(net, g):
    case = synth.detector_case(int(g["rfn"]), int(g["hq"]), int(g["wq"]))
    data = {"ref_imgs_info": {"imgs": case["ref_imgs"].to(DEV)}, "que_imgs_info": {"imgs": case["que_imgs"].to(DEV)}}
    with torch.no_grad():
        return net.range_guarded(lambda: net(data))


def test_detector_fp32_cores_is_invariant(golden):
    """fp32_cores, A = 12: the golden bars hold, and the maps are those of the original weights within 1e-6 of their range (the CPU
    oracle test's tolerance).  Power-of-two gains commute with every fp32 rounding: whether the outputs are in fact identical is recorded."""
    from test_networks_gpu import _check_detector
    g = golden("det_small")
    net = _detector(_gains(12), fp32_cores=True)
    _check_detector(g, net, "det_small")
    out, base = _detect(net, g), _detect(_detector(fp32_cores=True), g)
    same = True
    for k in MAPS:
        d = float((out[k].double() - base[k].double()).abs().max()) / float(base[k].abs().max())
        same = same and torch.equal(out[k], base[k])
        record("test_detector_fp32_cores_is_invariant", f"det_small/{k}: reparameterised - original, fp32_cores / range", d, 1e-6)
        assert d <= 1e-6, (k, d)
    print(f"fp32_cores, mixed gains A = 12 on trunk layers 2 and 4: outputs bit-identical to the original weights': {same}")
    record("test_detector_fp32_cores_is_invariant", "det_small: outputs bit-identical (1 = yes)", float(same), 1.0, note="recorded")
    assert torch.equal(out["que_select_id"], base["que_select_id"])
    assert net.range_fallbacks == 0


def test_detector_default_routes_mild_spread(golden):
    """Default routes, A = 4.  Precondition, read from range_report(): the reparameterised maps peak at >= 2 with exponent 0 (the gain
    vectors carry the power of two that lifts them there).  The floor 2^-25 then sits at most 2^-25 / (2 x 2^-4) = 2^-22 below the
    smallest channel's peak — the format's own relative precision — so the golden bars must hold."""
    from test_networks_gpu import _check_detector
    g = golden("det_small")
    probe = _detector(_gains(4))
    _detect(probe, g)
    rep = probe.range_report()
    lift = tuple(2.0 ** max(0, math.ceil(math.log2(2.0 / rep[n]["A"]))) for n in ("trunk2", "trunk4"))
    net = _detector(_gains(4, lift))
    _check_detector(g, net, "det_small")
    assert net.range_check() is False and net.range_fallbacks == 0
    rep = net.range_report()
    print(f"default routes, A = 4, lifts {lift}: {rep}")
    for n in ("trunk2", "trunk4"):
        assert 2.0 <= rep[n]["A"] < 2.0 ** 14 and rep[n]["e"] == 0, (n, rep[n])


@pytest.mark.parametrize("A", [8, 12])
def test_detector_default_routes_wide_spread(golden, A):
    """Default routes, A = 8 and 12: finite outputs and the golden's detection cell; the three errors and the guard's fallback count are
    RECORDED, not bounded — the guard records one maximum per map and stays silent (the blind spot this file documents)."""
    g = golden("det_small")
    net = _detector(_gains(A))
    out = _detect(net, g)
    for k in MAPS:
        assert bool(torch.isfinite(out[k]).all()), k
        err = float(np.abs(out[k].cpu().double().numpy() - g[k]).max()) / max(float(np.abs(g[k]).max()), 1.0)
        print(f"default routes, A = {A}: det_small/{k} error vs golden {err:.2e} of range")
        record("test_detector_default_routes_wide_spread", f"det_small/{k}, mixed gains A = {A}, default routes vs golden / range", err, 0.0,
               note="recorded, not bounded (tol 0)")
    rep = net.range_report()
    print(f"default routes, A = {A}: range_fallbacks {net.range_fallbacks}, trunk2 {rep.get('trunk2')}, trunk4 {rep.get('trunk4')}")
    record("test_detector_default_routes_wide_spread", f"det_small, mixed gains A = {A}: range_fallbacks", float(net.range_fallbacks), 0.0,
           note="recorded: 0 is the blind spot")
    assert np.array_equal(out["que_select_id"].cpu().numpy(), g["que_select_id"])
