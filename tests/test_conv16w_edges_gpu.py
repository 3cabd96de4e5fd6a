"""The halo-patch kernel (conv16w_kernel) at the edges of its tiling: interior tiles beside all four edges and corners in one launch,
bottom / right overhang with pooling, banded tiles whose last tile is not filled, the two-tile form (Cout = 64) with an odd tile count,
a pyramid whose segments differ in tile width, statistics on whole and on cut tiles — pairs against the float64 convolution of the fp32
operands (bar 2e-6 of the output range, + 2^-21 for pair outputs), one fp16 and one bf16 case through the same prologue and epilogue
(float64 convolution of the rounded operands, bar 2e-5 + half an ulp of a 16-bit output).  Every output lies inside a NaN-filled buffer
with guard rows before and after it and guard channels on both sides of every pixel: nothing may be written outside the output."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from parity_log import record

pytestmark = pytest.mark.gpu

T16 = {1: torch.bfloat16, 2: torch.float16, 3: torch.float16}
ULP = {1: 2.0 ** -8, 2: 2.0 ** -11, 3: 2.0 ** -21}
GUARD_CH, GUARD_EL = 8, 4096                 # guard channels on each side of a pixel's row, guard elements before / after the map


def _split(x):
    hi = x.to(torch.float16)
    return torch.stack([hi, (x - hi.float()).to(torch.float16)], -2).contiguous()


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _halo_tw(N, H, W):
    """The tile width c16g::halo_tiling picks (least overhang, ties to the wider tile)."""
    best, res = 1e30, None
    for tw in (32, 16, 8, 4):
        th, tx = 128 // tw, -(-W // tw)
        if H >= th:
            nt, segh, bands = N * tx * -(-H // th), th, 1
        elif th % H == 0:
            nt, segh, bands = tx * -(-(N * H) // th), H, th // H
        else:
            continue
        if bands * (segh + 2) * (tw + 2) > 288:
            continue
        waste = nt * 128 / (N * H * W)
        if waste < best - 1e-9:
            best, res = waste, (tw, nt)
    return res


class Guarded:
    """An output map [N, H, W, width] of `dtype` inside a NaN-filled buffer: rows of width + 2 GUARD_CH elements, GUARD_EL elements around."""

    def __init__(self, N, H, W, width, dtype):
        self.ld = width + 2 * GUARD_CH
        self.n = N * H * W * self.ld
        self.buf = torch.full((self.n + 2 * GUARD_EL,), float("nan"), dtype=dtype, device="cuda")
        self.rows = self.buf[GUARD_EL:GUARD_EL + self.n].view(N, H, W, self.ld)
        self.map = self.rows[..., GUARD_CH:GUARD_CH + width]

    def untouched(self):
        b = self.buf.cpu()
        r = b[GUARD_EL:GUARD_EL + self.n].view(self.rows.shape)
        return bool(torch.isnan(b[:GUARD_EL]).all() and torch.isnan(b[GUARD_EL + self.n:]).all() and torch.isnan(r[..., :GUARD_CH]).all()
                    and torch.isnan(r[..., -GUARD_CH:]).all())


def _launch(xs, filt, bias, relu, full, pool, stats, rpg):
    """g6d_conv16_direct_multi_ex on caller-made (guarded) outputs.  full / pool: None, "t16" or "f32" -> lists of Guarded."""
    from gen6d_amd import lib, ops
    mode, Cout, Cin = filt.mode, filt.Cout, filt.Cin
    pair = mode == 3
    code = {None: 0, "t16": 3 if pair else 1, "f32": 2}
    segs = (lib.G6dConv16Seg * len(xs))()
    fulls, pools = [], []
    for i, x in enumerate(xs):
        N, H, W = x.shape[:3]

        def make(kind, h, w):
            if kind is None:
                return None
            return Guarded(N, h, w, Cout * (2 if pair and kind == "t16" else 1), T16[mode] if kind == "t16" else torch.float32)
        f, q = make(full, H, W), make(pool, H // 2, W // 2)
        fulls.append(f); pools.append(q)
        segs[i] = lib.G6dConv16Seg(in_=x.data_ptr(), out_full=f.map.data_ptr() if f else None, out_pool=q.map.data_ptr() if q else None, N=N, D=1, H=H,
                                   W=W, ld_in=(2 if pair else 1) * Cin, ld_full=f.ld if f else 0, ld_pool=q.ld if q else 0)
    lib.check(lib.load().g6d_conv16_direct_multi_ex(segs, len(xs), Cin, C.c_void_p(filt.data.data_ptr()), int(filt.layout), float(filt.acc_scale),
                                                    C.c_void_p(bias.data_ptr()), Cout, 1, int(relu), code[full], code[pool], int(mode),
                                                    C.c_void_p(stats.data_ptr()) if stats is not None else C.c_void_p(0), int(rpg), None,
                                                    ops._stream()), "g6d_conv16_direct_multi_ex")
    torch.cuda.synchronize()
    return fulls, pools


CASES = [
    # segs (N, H, W); tw: the tile widths the tiling must choose; mode 3 = pairs, 2 = fp16, 1 = bf16; gi: images per statistics group
    # 5 x 5 tiles of 8 x 16: nine interior tiles, every edge and corner; one slice; pair output with statistics
    dict(id="interior+edges-1slice-stats", segs=[(1, 40, 80)], tw=[16], Cin=32, Cout=128, full="t16", pool=None, gi=1),
    # the same tiling with a ragged right edge (72 = 4.5 tiles), two slices, fp32 output
    dict(id="interior+edges-ragged-f32", segs=[(1, 40, 72)], tw=[16], Cin=64, Cout=128, full="f32", pool=None),
    # 4 x 32 tiles hanging over the bottom (24 > 22) and the right (32 > 30), pooled pair output beside the full fp32 map
    dict(id="overhang-pool", segs=[(2, 22, 30)], tw=[32], Cin=64, Cout=128, full="f32", pool="t16"),
    # banded tiles, two-tile form (Cout = 64), three tiles = an odd count: the last tile half filled (5 images, 2 per tile) ...
    dict(id="banded8-odd-partial", segs=[(5, 8, 8)], tw=[8], Cin=64, Cout=64, full="f32", pool=None, relu=False),
    # ... and with statistics (the launcher wants a tile inside ONE group: groups of 2 images = one tile)
    dict(id="banded8-odd-stats", segs=[(6, 8, 8)], tw=[8], Cin=64, Cout=64, full="f32", pool=None, relu=False, gi=2),
    # 4 x 4 maps, eight per tile: 17 images leave seven bands of the third tile empty; 24 images = three tiles with statistics
    dict(id="banded4-partial", segs=[(17, 4, 4)], tw=[4], Cin=64, Cout=64, full="f32", pool=None, relu=False),
    dict(id="banded4-odd-stats", segs=[(24, 4, 4)], tw=[4], Cin=64, Cout=64, full="f32", pool=None, relu=False, gi=8),
    # a pyramid of four segments with tile widths 32 / 16 / 8 / 4 (the last one banded), pooled pair output only
    dict(id="pyramid-4widths-pool", segs=[(2, 44, 58), (2, 24, 16), (2, 16, 8), (3, 8, 4)], tw=[32, 16, 8, 4], Cin=64, Cout=128, full=None, pool="t16"),
    # the 16-bit modes through the same prologue and epilogue: pooled 16-bit output and statistics
    dict(id="fp16-pool-stats", mode=2, segs=[(2, 24, 30)], tw=[32], Cin=64, Cout=128, full=None, pool="t16", gi=1),
    dict(id="bf16-pool-full-stats", mode=1, segs=[(3, 16, 24)], tw=[8], Cin=64, Cout=256, full="t16", pool="t16", gi=1),
]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_conv16w_edges(case, knob):
    from gen6d_amd import ops
    knob("conv16_halo", 1)
    c = case
    mode, Cin, Cout, relu = c.get("mode", 3), c["Cin"], c["Cout"], c.get("relu", True)
    pair = mode == 3
    assert [_halo_tw(*s)[0] for s in c["segs"]] == c["tw"], "the case no longer has the tiling it was written for"
    if Cout == 64:
        assert sum(_halo_tw(*s)[1] for s in c["segs"]) % 2 == 1, "an odd tile count is what the two-tile case is about"
    g = torch.Generator().manual_seed(11 + Cin + 5 * len(c["segs"]) + c["segs"][0][0])
    w = _rand(g, Cout, 9, Cin, scale=(1.0 / (9 * Cin)) ** 0.5 * 3)
    b = _rand(g, Cout, scale=0.2)
    xs = [_rand(g, *s, Cin) for s in c["segs"]]
    if not pair:                                               # the 16-bit modes: the reference convolves the rounded operands
        w, xs = w.to(T16[mode]).float(), [x.to(T16[mode]).float() for x in xs]
    stats, rpg = None, 0
    if c.get("gi"):
        N0, H0, W0 = c["segs"][0]
        stats = torch.zeros((N0 // c["gi"], Cout, 2), dtype=torch.float64, device="cuda")
        rpg = c["gi"] * H0 * W0
    filt = ops.conv16_pack(w.cuda(), mode, 1)
    xin = [(_split(x) if pair else x.to(T16[mode])).cuda() for x in xs]
    fulls, pools = _launch(xin, filt, b.cuda(), relu, c["full"], c["pool"], stats, rpg)
    base = 2e-6 if pair else 2e-5
    worst = 0.0
    w4 = w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)

    def value(gd, kind):
        m = gd.map.cpu()
        if pair and kind == "t16":
            return m[..., :Cout].double() + m[..., Cout:].double()
        return m.double()
    for i, x in enumerate(xs):
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4, b.double(), padding=1).permute(0, 2, 3, 1)
        if relu:
            ref = F.relu(ref)
        rng = float(ref.abs().max())
        if stats is not None and i == 0:                     # (of the outputs: after the ReLU)
            G = stats.shape[0]
            n = ref.numel() / (G * Cout)
            got = stats.cpu()
            e1 = float((got[:, :, 0] - ref.reshape(G, -1, Cout).sum(1)).abs().max()) / n / rng
            e2 = float((got[:, :, 1] - (ref * ref).reshape(G, -1, Cout).sum(1)).abs().max()) / n / rng ** 2
            print(f"{c['id']}: statistics error / range {e1:.3e} (bar {base:.0e}), squares {e2:.3e} (bar {2 * base:.0e})")
            assert e1 <= base, ("statistics: sum", e1)
            assert e2 <= 2 * base, ("statistics: sum of squares", e2)
        for kind, gd, want in (("full", fulls[i], ref), ("pool", pools[i], None)):
            if gd is None:
                continue
            if want is None:
                want = F.max_pool2d(ref.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
            otype = c[kind]
            tol = base + (ULP[mode] if otype == "t16" else 0.0)
            e = float((value(gd, otype) - want).abs().max()) / rng
            print(f"{c['id']}: segment {i} {kind} error / range {e:.3e} (bar {tol:.3e})")
            worst = max(worst, e / tol)
            assert e <= tol, (i, kind, e, tol)                  # (NaN — an output pixel never written — fails here too)
            assert gd.untouched(), f"segment {i}: the {kind} output wrote outside its map"
    record("test_conv16w_edges", f"halo edges {c['id']} {c['segs']} x{Cin} -> {Cout} (error / bar)", worst, 1.0,
           note="vs fp64 conv of the fp32 operands, bar 2e-6 of range" if pair else "vs fp64 conv of the rounded operands, bar 2e-5 of range")
