"""The halo-patch pair kernel with the depth taps of a 3x3x3 layer folded into its reduction (conv16w_kernel<3, ., 1, 3>, filter layout 2)
against the float64 conv3d of the fp32 operands, at the smallest shapes that can still go wrong: two volumes (the plane after the last
plane of volume 0 is plane 0 of volume 1: it must read as padding), D = 1 / 2 / 3 (padding only; no middle plane; first, middle and last
plane), planes of 16 x 16 (two tiles per plane), 16 x 24 (three tiles per plane: the two-tile blocks of Cout = 64 straddle planes) and
18 x 20 (tiles that hang over the right and the bottom edge), one and two channel slices per depth tap, both block shapes (Cout = 64 and
128), fp32 output with per-volume sums and pair output without.  Bars, those of test_conv16w_edges_gpu: output 2e-6 of the output range
(+ 2^-21 for a pair output), sums 2e-6.  Also: agreement with the existing per-tap kd = 3 path (conv16r_kernel on 27-tap filters) within
the sum of the two paths' bars, guard bands around every output untouched, and two launches agreeing bit for bit."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from parity_log import record

pytestmark = pytest.mark.gpu

BAR = 2e-6
GUARD_CH, GUARD_EL = 8, 4096


def _split(x):
    hi = x.to(torch.float16)
    return torch.stack([hi, (x - hi.float()).to(torch.float16)], -2).contiguous()


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


class Guarded:
    """An output map of `pixels` rows of `width` elements inside a NaN-filled buffer: rows of width + 2 GUARD_CH, GUARD_EL elements around."""

    def __init__(self, pixels, width, dtype):
        self.ld = width + 2 * GUARD_CH
        self.n = pixels * self.ld
        self.buf = torch.full((self.n + 2 * GUARD_EL,), float("nan"), dtype=dtype, device="cuda")
        self.rows = self.buf[GUARD_EL:GUARD_EL + self.n].view(pixels, self.ld)
        self.map = self.rows[:, GUARD_CH:GUARD_CH + width]

    def untouched(self):
        b = self.buf.cpu()
        r = b[GUARD_EL:GUARD_EL + self.n].view(self.rows.shape)
        return bool(torch.isnan(b[:GUARD_EL]).all() and torch.isnan(b[GUARD_EL + self.n:]).all() and torch.isnan(r[:, :GUARD_CH]).all()
                    and torch.isnan(r[:, -GUARD_CH:]).all())


def _launch(x16, filt, bias, kind, stats, rpg):
    """g6d_conv16_direct_multi_ex, kd = 3, on a guarded output.  kind: "f32" or "t16" (pairs)."""
    from gen6d_amd import lib, ops
    N, D, H, W = x16.shape[:4]
    Cout, Cin = filt.Cout, filt.Cin
    out = Guarded(N * D * H * W, Cout * (2 if kind == "t16" else 1), torch.float16 if kind == "t16" else torch.float32)
    seg = (lib.G6dConv16Seg * 1)(lib.G6dConv16Seg(in_=x16.data_ptr(), out_full=out.map.data_ptr(), out_pool=None, N=N, D=D, H=H, W=W, ld_in=2 * Cin,
                                                  ld_full=out.ld, ld_pool=0))
    lib.check(lib.load().g6d_conv16_direct_multi_ex(seg, 1, Cin, C.c_void_p(filt.data.data_ptr()), int(filt.layout), float(filt.acc_scale),
                                                    C.c_void_p(bias.data_ptr()), Cout, 3, 0, 3 if kind == "t16" else 2, 0, 3,
                                                    C.c_void_p(stats.data_ptr()) if stats is not None else C.c_void_p(0), int(rpg), None,
                                                    ops._stream()), "g6d_conv16_direct_multi_ex")
    torch.cuda.synchronize()
    return out


CASES = [dict(D=D, plane=pl, Cin=ci, Cout=co) for pl in ((16, 16), (16, 24)) for D in (1, 2, 3) for ci in (32, 64) for co in (64, 128)] + \
        [dict(D=D, plane=(18, 20), Cin=32, Cout=co) for D in (1, 2, 3) for co in (64, 128)]


@pytest.mark.parametrize("case", CASES, ids=[f"D{c['D']}-{c['plane'][0]}x{c['plane'][1]}-{c['Cin']}to{c['Cout']}" for c in CASES])
def test_conv16w_depth(case, knob):
    from gen6d_amd import ops
    knob("conv16_halo", 1)
    D, (H, W), Cin, Cout = case["D"], case["plane"], case["Cin"], case["Cout"]
    N = 2
    assert ops.conv16_direct_plan(N, H, W, Cin, Cout, 3, stats_rows=D * H * W, D=D) == 1, "the folded layer must take the halo-patch kernel"
    g = torch.Generator().manual_seed(1000 * D + 10 * H + W + Cin + Cout)
    w = _rand(g, Cout, 27, Cin, scale=(1.0 / (27 * Cin)) ** 0.5 * 3)
    b = _rand(g, Cout, scale=0.2)
    x = _rand(g, N, D, H, W, Cin)
    x = x * (1.0 + torch.arange(N).view(N, 1, 1, 1, 1))          # every volume its own scale: a plane read from the neighbour shows
    w5 = w.double().reshape(Cout, 3, 3, 3, Cin).permute(0, 4, 1, 2, 3)
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w5, b.double(), padding=1).permute(0, 2, 3, 4, 1).reshape(N, D * H * W, Cout)
    rng = float(ref.abs().max())
    filt = ops.conv16_pack(w.cuda(), 3, layout=2)
    assert filt.layout == 2 and filt.taps == 27
    x16, bias = _split(x).cuda(), b.cuda()

    # fp32 output with per-volume sums
    stats = torch.zeros((N, Cout, 2), dtype=torch.float64, device="cuda")
    out = _launch(x16, filt, bias, "f32", stats, D * H * W)
    got = out.map.cpu().double().reshape(N, D * H * W, Cout)
    e = float((got - ref).abs().max()) / rng
    n = D * H * W
    st = stats.cpu()
    e1 = float((st[:, :, 0] - ref.sum(1)).abs().max()) / n / rng
    e2 = float((st[:, :, 1] - (ref * ref).sum(1)).abs().max()) / n / rng ** 2
    print(f"fp32 output error / range {e:.3e}, sums {e1:.3e}, squares {e2:.3e} (bars {BAR:.0e})")
    assert e <= BAR, ("fp32 output", e)                            # (NaN — an output pixel never written — fails here too)
    assert e1 <= BAR and e2 <= BAR, ("sums", e1, e2)
    assert out.untouched(), "the fp32 output wrote outside its map"

    # two launches agree bit for bit (the sums are fp64 atomics in any order: the map only)
    again = _launch(x16, filt, bias, "f32", None, 0)
    assert torch.equal(again.map, out.map), "two launches differ"
    assert again.untouched()

    # pair output, no sums
    pr = _launch(x16, filt, bias, "t16", None, 0)
    m = pr.map.cpu()
    ep = float(((m[:, :Cout].double() + m[:, Cout:].double()).reshape(N, n, Cout) - ref).abs().max()) / rng
    print(f"pair output error / range {ep:.3e} (bar {BAR + 2.0 ** -21:.3e})")
    assert ep <= BAR + 2.0 ** -21, ("pair output", ep)
    assert pr.untouched(), "the pair output wrote outside its map"

    # the existing per-tap kd = 3 path on the 27-tap filters (Cout % 128 == 0: 64 filters are padded with zeros): both lie within BAR of
    # the float64 result, so they agree within 2 BAR
    wp = torch.cat([w, torch.zeros_like(w)], 0) if Cout == 64 else w
    tap, _ = ops.conv16_direct_multi([x16], ops.conv16_pack(wp.cuda(), 3, layout=1), torch.cat([b, torch.zeros_like(b)]).cuda() if Cout == 64 else bias,
                                     relu=False, full=torch.float32, kd=3)
    et = float((tap[0].cpu().double().reshape(N, n, -1)[..., :Cout] - got).abs().max()) / rng
    print(f"folded against per-tap / range {et:.3e} (bar {2 * BAR:.0e})")
    assert et <= 2 * BAR, ("per-tap path", et)
    record("test_conv16w_depth", f"depth-folded pairs {N}x{D}x{H}x{W}x{Cin} -> {Cout} (error / bar)", max(e, e1, e2, ep / (1 + 2.0 ** -21 / BAR)) / BAR, 1.0,
           note="vs fp64 conv3d of the fp32 operands, bar 2e-6 of range")
