"""The pre-split variants of the implicit-GEMM kernel's pair mode (G6dConv.math_mode 4 / 5, ops.conv(pairs=(table, slot, variant))), host side:
(1) ops.pair_filter_pack reproduces the device split rule bit for bit — against ops._split_hi_lo and against a plain float32 restatement
    of pair16.h (hi = rn16(u), lo = rn16(u - hi), u = w * 2^w_exp) — with filters small enough that lo parts go subnormal and a forced
    non-zero exponent, in the layout include/gen6d_hip.h states: [Cout][taps][Cin / 32][hi 32 | lo 32];
(2) a Python restatement of the loader's offset formula (conv_igemm.hip: per-row constant offset + uniform tap / chunk offset, 16 bytes per
    thread, LDS address row * 144 + 16 lseg) addresses every (row, tap, chunk, plane, segment) of both packed layouts exactly once, a
    channel slice of a wider pair map included;
(3) over the recording fake library: variant 4 passes math_mode 4 with the cached pack as `weight`; variant 5 issues the affine_split16
    pass (planes as images, per_n * D planes per table, the layer's own slot as slot_out) and then a math_mode 5 launch without prologue
    that reads that slot as slot_in, booked under the layer's `aff` label."""
import numpy as np
import pytest
import torch

from gen6d_amd import lib, ops
from test_multi_launch_cpu import fake  # noqa: F401  (the fixture)


def _rule32(w, e):
    """pair16.h restated in float32 arithmetic: the scaling is exact, u - hi is exact in fp32."""
    u = (w * np.float32(2.0 ** e)).astype(np.float32)
    hi = u.astype(np.float16)
    lo = (u - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


@pytest.mark.parametrize("scale,force", [(1.0, None), (1e-3, None), (1e-2, 0), (0.5, 7)], ids=["unit", "small", "subnormal-lo", "forced-exp7"])
def test_pack_reproduces_the_split_rule(scale, force):
    g = torch.Generator().manual_seed(5)
    w = ((torch.rand((48, 27, 64), generator=g) - 0.5) * scale).contiguous()
    if force is not None:
        w.__dict__["_g6d_w_exp"] = force
    e = ops.pair_filter_prepare(w)
    assert e == (force if force is not None else ops.pair_filter_exponent(w))
    pk = ops.pair_filter_pack(w)
    assert pk.dtype == torch.float16 and tuple(pk.shape) == (48, 27, 2, 2, 32) and pk.is_contiguous()
    assert ops.pair_filter_pack(w) is pk, "cached on the weight"
    hi = pk[:, :, :, 0, :].reshape(48, 27, 64)
    lo = pk[:, :, :, 1, :].reshape(48, 27, 64)
    h32, l32 = _rule32(w.numpy(), e)
    assert np.array_equal(hi.numpy().view(np.uint16), h32.view(np.uint16))
    assert np.array_equal(lo.numpy().view(np.uint16), l32.view(np.uint16))
    if force is None:
        h, l, inv = ops._split_hi_lo(w)
        assert inv == 2.0 ** -e
        assert torch.equal(h.view(torch.int16), hi.view(torch.int16)) and torch.equal(l.view(torch.int16), lo.view(torch.int16))
    if force == 0:       # exponent 0 forced on tiny filters: the case has fp16-subnormal lo parts (below 2^-14), kept by the pack
        sub = (lo.abs() > 0) & (lo.abs() < 2.0 ** -14)
        assert bool(sub.any())


def test_filter_loader_offsets_cover_the_pack_once():
    """rows (co), taps, chunks, thread segments: byte offset = the fp32 loader's (co T Cin + 4 lseg) 4 + (tap Cin + 32 cc) 4; the 16 bytes go
    to LDS bytes [16 lseg, 16 lseg + 16) of the row: plane lseg >> 2, channels 8 (lseg & 3) .. + 7 of the chunk."""
    Cout, T, Cin = 5, 3, 64
    w = torch.arange(Cout * T * Cin, dtype=torch.float32).view(Cout, T, Cin) / 8.0
    w.__dict__["_g6d_w_exp"] = 0
    pk = ops.pair_filter_pack(w)
    flat = pk.reshape(-1)
    seen = np.zeros(flat.numel() // 8, dtype=np.int64)
    for co in range(Cout):
        for tap in range(T):
            for cc in range(Cin // 32):
                for lseg in range(8):
                    off = ((co * T * Cin + 4 * lseg) << 2) + ((tap * Cin + cc * 32) << 2)
                    assert off % 16 == 0
                    seen[off // 16] += 1
                    got = flat[off // 2: off // 2 + 8]
                    want = pk[co, tap, cc, lseg >> 2, 8 * (lseg & 3): 8 * (lseg & 3) + 8]
                    assert torch.equal(got, want)
    assert (seen == 1).all()
    assert flat.numel() * 2 == Cout * T * Cin * 4, "the pack fills the bytes of the fp32 filters: w_bytes holds"


@pytest.mark.parametrize("Ct,c_off", [(64, 0), (96, 32)], ids=["dense", "slice-of-96"])
def test_activation_loader_offsets_cover_the_pair_map_once(Ct, c_off):
    """The math_mode 5 loader: row offset ((pixel ld_in + 8 (lseg & 3)) << 1) + (lseg >> 2) ld_in bytes, uniform offset (tap pixels ld_in +
    32 cc) << 1, on a map [pixels][2][Ct] of 16-bit elements with ld_in = 2 Ct and `in` pointing at channel c_off of the hi plane."""
    P, Cin = 7, 64
    ld_in = 2 * Ct
    m = torch.arange(P * 2 * Ct, dtype=torch.int32).view(P, 2, Ct)
    flat = m.reshape(-1)
    base = c_off                       # element offset of `in`
    seen = np.zeros(flat.numel(), dtype=np.int64)
    for row in range(P - 2):           # output rows of a 1-D stride-1 window of 3 taps without padding
        for tap in range(3):
            for cc in range(Cin // 32):
                for lseg in range(8):
                    voff = ((row * ld_in + 8 * (lseg & 3)) << 1) + (lseg >> 2) * ld_in
                    soff = (tap * ld_in + cc * 32) << 1
                    assert (voff + soff) % 16 == 0
                    e0 = base + (voff + soff) // 2
                    want = m[row + tap, lseg >> 2, c_off + 32 * cc + 8 * (lseg & 3): c_off + 32 * cc + 8 * (lseg & 3) + 8]
                    assert torch.equal(flat[e0:e0 + 8], want)
                    if tap == 0:
                        seen[e0:e0 + 8] += 1
    cover = np.zeros((P, 2, Ct), dtype=np.int64)
    cover[:P - 2, :, c_off:c_off + Cin] = 1      # tap 0 of every row: each element of the slice once, nothing outside it
    assert np.array_equal(seen.reshape(P, 2, Ct), cover)


def _volume():
    g = torch.Generator().manual_seed(2)
    x = torch.rand((4, 3, 5, 5, 32), generator=g)
    w = torch.rand((64, 27, 32), generator=g) - 0.5
    out = torch.empty((4, 3, 5, 5, 64))
    sc, sh = torch.rand((2, 32), generator=g), torch.rand((2, 32), generator=g)
    return x, w, out, sc, sh


def test_variant_4_passes_the_pack(fake):  # noqa: F811
    x, w, out, sc, sh = _volume()
    table = ops.RangeTable(torch.device("cpu"))
    ops.conv(x, w, None, out, ksize=(3, 3, 3), pad=(1, 1, 1), in_scale=sc, in_shift=sh, in_relu=True, per_n=2, pairs=(table, table.slot("a"), 4))
    (name, (dref, rref, _)), = fake.calls
    d, r = dref._obj, rref._obj
    assert name == "g6d_conv_igemm_ex" and d.math_mode == 4 and d.weight == ops.pair_filter_pack(w).data_ptr() != w.data_ptr()
    assert d.in_scale == sc.data_ptr() and d.in_affine_per_n == 2 and d.w_exp == ops.pair_filter_exponent(w)
    assert (r.slot_in, r.slot_out) == (-1, 0)
    with pytest.raises(ValueError, match="Cin % 32"):
        ops.conv(x[..., :16], w[..., :16].contiguous(), None, out, ksize=(3, 3, 3), pad=(1, 1, 1), pairs=(table, 0, 4))


def test_variant_5_issues_the_pass_then_copies(fake, monkeypatch):  # noqa: F811
    x, w, out, sc, sh = _volume()
    table = ops.RangeTable(torch.device("cpu"))
    table.slot("other")
    fake.plan = 5
    monkeypatch.setattr(ops, "PROFILE", [])
    monkeypatch.setattr(ops, "PROFILE_HBM", {})
    ops.conv(x, w, None, out, ksize=(3, 3, 3), pad=(1, 1, 1), in_scale=sc, in_shift=sh, in_relu=True, per_n=2, pairs=(table, table.slot("a"), 5))
    (n0, a0), (n1, (dref, rref, _)) = fake.calls
    assert n0 == "g6d_affine_split16_ex" and n1 == "g6d_conv_igemm_ex"
    # (in, ld_in, scale, shift, per_n, relu, pool, N, H, W, C, out, mode, range, stream): planes as images, 2 volumes x 3 planes per table
    assert a0[1] == 32 and a0[4:11] == (6, 1, 0, 12, 5, 5, 32) and a0[12] == 3
    assert (a0[13]._obj.slot_in, a0[13]._obj.slot_out) == (-1, 1)
    d, r = dref._obj, rref._obj
    assert d.math_mode == 5 and d.in_scale is None and d.in_shift is None and d.in_relu == 0 and d.in_affine_per_n == 0
    assert d.ld_in == 64 and d.Cin == 32 and d.weight == ops.pair_filter_pack(w).data_ptr()
    assert (r.slot_in, r.slot_out) == (1, -1)
    (fl, _, _, label, _, _), = ops.PROFILE
    assert label.startswith("conv16x3 igemm conv N=4 in=3x5x5x32") and label.endswith(" aff")
    assert list(ops.PROFILE_HBM) == ["affine_split16"]
    assert lib.G6dRange16 is type(r)
