"""The hand-over passes of the refiner's feature net to the pair kernel, each against the fp32 kernel whose arithmetic it repeats, on the
same input: g6d_l2norm_split16 (g6d_l2norm_rows), g6d_affine_split16_to (g6d_affine_act_pool) and g6d_upsample_bilinear_split16
(g6d_upsample_bilinear), the last two into a channel slice of wider pair rows.  hi + lo, scaled back by the slot's exponent (set to a
non-zero value here), must lie within 2^-21 of the map's range of the fp32 result — the pair resolution the pair outputs are allowed
everywhere — and the recorded maximum must be the fp32 result's, bit for bit.  Every output lies in a NaN-filled buffer with guard
elements around it and guard channels at both ends of every row: neighbouring slices, guards and the other plane's gaps keep their NaNs.
One fp16 (math_mode 2) instance of each: a single plane, half an fp16 ulp of the range."""
import ctypes as C

import pytest
import torch

from parity_log import record

pytestmark = pytest.mark.gpu

GUARD_CH, GUARD_EL = 8, 4096
EXP = -2                                     # the slot's exponent: the maps here peak below 1, stored as v * 4


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


class Rows16:
    """[pixels] rows of an fp16 map of `planes` x `width` channels in a NaN-filled buffer: GUARD_CH guard channels at both ends of a row,
    GUARD_EL guard elements around the map."""

    def __init__(self, pixels, width, planes):
        self.width, self.planes, self.pixels = width, planes, pixels
        self.ld = planes * width + 2 * GUARD_CH
        self.n = pixels * self.ld
        self.buf = torch.full((self.n + 2 * GUARD_EL,), float("nan"), dtype=torch.float16, device="cuda")
        self.first = self.buf[GUARD_EL + GUARD_CH:]                      # channel 0 of pixel 0

    def read(self, c_off, Cc):
        """(value = sum of the planes of the slice as float64 [pixels, Cc], everything else still NaN?)"""
        b = self.buf.cpu()
        rows = b[GUARD_EL:GUARD_EL + self.n].view(self.pixels, self.ld)
        body = rows[:, GUARD_CH:GUARD_CH + self.planes * self.width].reshape(self.pixels, self.planes, self.width)
        val = body[:, :, c_off:c_off + Cc].double().sum(1)
        rest = body.clone()
        rest[:, :, c_off:c_off + Cc] = float("nan")
        clean = bool(torch.isnan(b[:GUARD_EL]).all() and torch.isnan(b[GUARD_EL + self.n:]).all() and torch.isnan(rows[:, :GUARD_CH]).all()
                     and torch.isnan(rows[:, -GUARD_CH:]).all() and torch.isnan(rest).all())
        return val, clean


def _range(mode):
    from gen6d_amd import ops
    if mode != 3:
        return None, None
    t = ops.RangeTable(torch.device("cuda"))
    t.set_exponents({"map": EXP})
    t.clear()
    return t, C.byref(t.arg(-1, t.slot("map")))


def _check(what, rows, c_off, Cc, want, table, mode):
    """want: the fp32 kernel's result [pixels, Cc]."""
    torch.cuda.synchronize()
    val, clean = rows.read(c_off, Cc)
    want = want.cpu()
    rng = float(want.abs().max())
    e = float((val * (2.0 ** EXP if mode == 3 else 1.0) - want.double()).abs().max()) / rng
    bar = 2.0 ** -21 if mode == 3 else 2.0 ** -11
    print(f"{what}: error / range {e:.3e} (bar {bar:.3e})")
    record("test_pair_handover", f"{what} (error / bar)", e / bar, 1.0, note="vs the fp32 kernel of the same arithmetic")
    assert e <= bar, (what, e)                                  # (NaN — an element never written — fails here too)
    assert clean, f"{what}: wrote outside its slice"
    if mode == 3:
        got = table.read()["map"]
        assert got == rng, (what, "recorded maximum", got, rng)


@pytest.mark.parametrize("Cc,mode", [(256, 3), (512, 3), (256, 2)])
def test_l2norm_split16(Cc, mode):
    from gen6d_amd import lib, ops
    g = torch.Generator().manual_seed(3 + Cc)
    x = _rand(g, 2, 3, 5, Cc).cuda()
    x[0, 1, 2] = 0.0                                            # a zero pixel: the eps clamp
    want = ops.l2norm_rows(x.clone()).view(30, Cc)
    planes = 2 if mode == 3 else 1
    out = torch.full((30 * planes * Cc + 2 * GUARD_EL,), float("nan"), dtype=torch.float16, device="cuda")
    table, ra = _range(mode)
    lib.check(lib.load().g6d_l2norm_split16(C.c_void_p(x.data_ptr()), Cc, 30, Cc, C.c_void_p(out[GUARD_EL:].data_ptr()), mode, ra, ops._stream()),
              "g6d_l2norm_split16")
    torch.cuda.synchronize()
    b = out.cpu()
    assert bool(torch.isnan(b[:GUARD_EL]).all() and torch.isnan(b[-GUARD_EL:]).all()), "wrote outside the map"
    val = b[GUARD_EL:-GUARD_EL].view(30, planes, Cc).double().sum(1)
    rng = float(want.abs().max())
    e = float((val * (2.0 ** EXP if mode == 3 else 1.0) - want.cpu().double()).abs().max()) / rng
    bar = 2.0 ** -21 if mode == 3 else 2.0 ** -11
    print(f"l2norm_split16 C={Cc} mode {mode}: error / range {e:.3e} (bar {bar:.3e})")
    record("test_pair_handover", f"l2norm_split16 2x3x5 x{Cc} mode {mode} (error / bar)", e / bar, 1.0, note="vs g6d_l2norm_rows")
    assert e <= bar
    if mode == 3:
        assert table.read()["map"] == rng
        # the wrapper: same bits, a PairMap of the slot
        t2 = ops.RangeTable(torch.device("cuda"))
        t2.set_exponents({"m": EXP})
        pm = ops.l2norm_split16(x, 3, rng=(t2, t2.slot("m")))
        assert isinstance(pm, ops.PairMap) and tuple(pm.shape) == (2, 3, 5, 2, Cc)
        assert torch.equal(pm.data.cpu().view(-1), b[GUARD_EL:-GUARD_EL])


@pytest.mark.parametrize("c_off,mode", [(0, 3), (64, 3), (128, 3), (64, 2)])
def test_affine_slice(c_off, mode):
    from gen6d_amd import lib, ops
    N, H, W, Cc, Ct = 3, 4, 4, 64, 192
    g = torch.Generator().manual_seed(17 + c_off)
    x = _rand(g, N, 1, H, W, Cc, scale=2.0).cuda()
    sc, sh = (_rand(g, N, Cc) * 0.2 + 0.3).cuda(), _rand(g, N, Cc, scale=0.2).cuda()
    want = torch.empty_like(x)
    ops.affine_act_pool(x, want, sc, sh, per_n=True)
    planes = 2 if mode == 3 else 1
    rows = Rows16(N * H * W, Ct, planes)
    table, ra = _range(mode)
    lib.check(lib.load().g6d_affine_split16_to(C.c_void_p(x.data_ptr()), Cc, C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), 1, 0, 0, N, H, W, Cc,
                                               C.c_void_p(rows.first.data_ptr()), rows.ld, Ct, c_off, mode, ra, ops._stream()), "g6d_affine_split16_to")
    _check(f"affine slice @{c_off} mode {mode}", rows, c_off, Cc, want.view(-1, Cc), table, mode)


@pytest.mark.parametrize("factor,c_off,mode", [(2, 64, 3), (4, 128, 3), (2, 0, 2)])
def test_upsample_slice(factor, c_off, mode):
    from gen6d_amd import lib, ops
    N, Cc, Ct = 3, 64, 192
    H = W = 8 // factor
    g = torch.Generator().manual_seed(29 + factor)
    x = _rand(g, N, 1, H, W, Cc, scale=2.0).cuda()
    sc, sh = (_rand(g, N, Cc) * 0.2 + 0.3).cuda(), _rand(g, N, Cc, scale=0.2).cuda()
    want = torch.empty((N, 1, 8, 8, Cc), dtype=torch.float32, device="cuda")
    ops.upsample_bilinear(x, want, factor, sc, sh, per_n=True)
    planes = 2 if mode == 3 else 1
    rows = Rows16(N * 64, Ct, planes)
    table, ra = _range(mode)
    lib.check(lib.load().g6d_upsample_bilinear_split16(C.c_void_p(x.data_ptr()), Cc, C.c_void_p(sc.data_ptr()), C.c_void_p(sh.data_ptr()), 1, N, H, W, Cc,
                                                       factor, C.c_void_p(rows.first.data_ptr()), rows.ld, Ct, c_off, mode, ra, ops._stream()),
              "g6d_upsample_bilinear_split16")
    _check(f"upsample x{factor} slice @{c_off} mode {mode}", rows, c_off, Cc, want.view(-1, Cc), table, mode)


def test_slices_share_one_pair_map():
    """The wrappers: three producers fill one PairMap [N,8,8,2,192] with one slot; the record is the maximum over the three."""
    from gen6d_amd import ops
    N, Cc = 3, 64
    g = torch.Generator().manual_seed(41)
    t = ops.RangeTable(torch.device("cuda"))
    t.set_exponents({"cat": EXP})
    t.clear()
    cat = ops.new_map16(N, 8, 8, 192, 3, torch.device("cuda"), rng=(t, t.slot("cat")))
    cat.data.fill_(float("nan"))
    wants = []
    for i, (hw, f) in enumerate(((8, 1), (4, 2), (2, 4))):
        x = _rand(g, N, 1, hw, hw, Cc, scale=1.0 + i).cuda()
        sc, sh = (_rand(g, N, Cc) * 0.2 + 0.3).cuda(), _rand(g, N, Cc, scale=0.2).cuda()
        want = torch.empty((N, 1, 8, 8, Cc), dtype=torch.float32, device="cuda")
        if f == 1:
            ops.affine_act_pool(x, want, sc, sh, per_n=True)
            assert ops.affine_split16_to(x, sc, sh, 1, False, 3, cat, 64 * i) is cat
        else:
            ops.upsample_bilinear(x, want, f, sc, sh, per_n=True)
            assert ops.upsample_bilinear_split16(x, cat, 64 * i, f, sc, sh, 1, 3) is cat
        wants.append(want[:, 0])
    want = torch.cat(wants, -1).cpu()
    got = cat.data.cpu().double().sum(-2) * 2.0 ** EXP
    rng = float(want.abs().max())
    assert float((got - want.double()).abs().max()) / rng <= 2.0 ** -21
    assert t.read()["cat"] == rng
    with pytest.raises(ValueError):
        ops.affine_split16_to(torch.zeros((N, 1, 8, 8, Cc), device="cuda"), None, None, 0, False, 3, cat, 160)     # past the row's channels
