"""The halo-patch kernel's fp16 hi / lo pair path (conv16w_kernel<3, WM>, v_mfma_f32_16x16x32_f16 fragments) against the float64
convolution of the fp32 operands, bar 2e-6 of the output range: every tile width of the halo tiling (32 / 16 / 8 / 4), banded tiles of
several small images, multi-segment launches, Cin 32 .. 512, Cout 64 (two pixel tiles per block) .. 512, full / pooled / fp32 / strided
outputs and statistics, and channels whose gains spread over 1e-3 .. 1e3."""
import pytest
import torch
import torch.nn.functional as F

from parity_log import record

pytestmark = pytest.mark.gpu


def _split(x):
    hi = x.to(torch.float16)
    return torch.stack([hi, (x - hi.float()).to(torch.float16)], -2).contiguous()


def _join(p):
    return p[..., 0, :].double() + p[..., 1, :].double()


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


CASES = [
    # segments (N, H, W); Cin; Cout; full; pool; optional: stats, gains, strided fp32 output
    dict(segs=[(2, 20, 64)], Cin=32, Cout=128, full="t16", pool=torch.float32),                        # tile width 32
    dict(segs=[(1, 24, 48)], Cin=64, Cout=256, full=torch.float32, pool="t16"),                       # 16
    dict(segs=[(2, 16, 24)], Cin=512, Cout=512, full="t16", pool=None),                               # 8
    dict(segs=[(2, 32, 12)], Cin=64, Cout=128, full=torch.float32, pool=None, stats=True),            # 4, statistics per image
    dict(segs=[(5, 8, 8)], Cin=64, Cout=64, full=torch.float32, pool="t16"),                          # 8x8: 2 images per tile, Cout = 64
    dict(segs=[(9, 4, 4)], Cin=32, Cout=128, full="t16", pool="t16"),                                 # 4x4: 8 images per tile
    dict(segs=[(4, 2, 64), (3, 4, 16)], Cin=64, Cout=128, full=torch.float32, pool=None),              # banded tiles of widths 32 and 16
    dict(segs=[(2, 44, 58), (2, 22, 30), (2, 11, 15), (2, 6, 8)], Cin=64, Cout=128, full="t16", pool=None),   # a pyramid in one launch
    dict(segs=[(2, 12, 20), (3, 8, 8)], Cin=64, Cout=64, full=torch.float32, pool=None, strided=True),  # Cout = 64, fp32 channel slice
    dict(segs=[(2, 18, 36)], Cin=128, Cout=256, full=torch.float32, pool=torch.float32, gains=True),  # gains 1e-3 .. 1e3
]


@pytest.mark.parametrize("case", CASES, ids=[f"case{i}" for i in range(len(CASES))])
def test_conv16w_pairs(case, knob):
    from gen6d_amd import ops
    knob("conv16_halo", 1)
    c = case
    Cin, Cout = c["Cin"], c["Cout"]
    g = torch.Generator().manual_seed(7 + Cin + 3 * len(c["segs"]))
    w = _rand(g, Cout, 9, Cin, scale=(1.0 / (9 * Cin)) ** 0.5 * 3)
    b = _rand(g, Cout, scale=0.2)
    xs = [_rand(g, *s, Cin) for s in c["segs"]]
    if c.get("gains"):
        gin = 10.0 ** (torch.rand(Cin, generator=g) * 6 - 3)
        gout = 10.0 ** (torch.rand(Cout, generator=g) * 6 - 3)
        xs = [x * gin for x in xs]
        w = w * gout[:, None, None]
        b = b * gout
    stats = None
    if c.get("stats"):
        stats = torch.zeros((c["segs"][0][0], Cout, 2), dtype=torch.float64, device="cuda")
    out_full, wide = None, []
    if c.get("strided"):
        for (N, H, W) in c["segs"]:
            buf = torch.full((N, H, W, Cout + 32), float("nan"), device="cuda")
            wide.append(buf)
        out_full = [t[..., 16:16 + Cout] for t in wide]
    filt = ops.conv16_pack(w.cuda(), 3, 1)
    fulls, pools = ops.conv16_direct_multi([_split(x).cuda() for x in xs], filt, b.cuda(), relu=True, full=c["full"], pool=c["pool"],
                                           stats=stats, rows_per_group=c["segs"][0][1] * c["segs"][0][2] if stats is not None else 0,
                                           out_full=out_full)
    torch.cuda.synchronize()
    worst = 0.0
    w4 = w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    for i, x in enumerate(xs):
        ref = F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w4, b.double(), padding=1).permute(0, 2, 3, 1))
        if stats is not None and i == 0:                     # (of the outputs: after the ReLU)
            n = ref[0].numel() / Cout
            got = stats.cpu()
            assert (got[:, :, 0] - ref.reshape(ref.shape[0], -1, Cout).sum(1)).abs().max() / n <= 2e-6 * ref.abs().max()
            assert (got[:, :, 1] - (ref * ref).reshape(ref.shape[0], -1, Cout).sum(1)).abs().max() / n <= 4e-6 * ref.abs().max() ** 2
        rng = float(ref.abs().max())
        outs = []
        if fulls[i] is not None:
            f = fulls[i].cpu()
            outs.append(("full", _join(f) if f.dtype == torch.float16 else f.double(), ref, f.dtype == torch.float16))
        if pools[i] is not None:
            q = pools[i].cpu()
            outs.append(("pool", _join(q) if q.dtype == torch.float16 else q.double(), F.max_pool2d(ref.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1),
                         q.dtype == torch.float16))
        for kind, got, want, is_pair in outs:
            tol = 2e-6 + (2.0 ** -21 if is_pair else 0.0)
            e = float((got - want).abs().max()) / rng
            worst = max(worst, e / tol)
            assert e <= tol, (i, kind, e, tol)
        if wide:
            rest = torch.cat([wide[i][..., :16], wide[i][..., 16 + Cout:]], -1)
            assert bool(torch.isnan(rest).all()), "a strided output wrote outside its channel slice"
    record("test_conv16w_pairs", f"pairs halo {c['segs']} x{Cin} -> {Cout} (error / bar)", worst, 1.0,
           note="16x16x32 pair fragments vs fp64 conv of the fp32 operands, bar 2e-6 of range")
