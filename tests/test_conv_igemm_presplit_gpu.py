"""The pre-split variants of the implicit-GEMM kernel's fp16 hi / lo pair mode, through ops.conv(pairs=(table, slot, variant)):
variant 4 (G6dConv.math_mode 4: filters pre-split by ops.pair_filter_pack) and variant 5 (math_mode 5: the activations pre-split as well,
by the affine_split16 pass ops.conv issues, or a PairMap some producer wrote).

Bit equality with variant 3 (the loader that splits both operands): same operands, same MFMA order, same split-K order — variant 4 on
every case, variant 5 on the cases without a prologue (there the pass is the bare split under the same exponent).  The fp64 sums are
compared bit for bit where their order is fixed — a tile inside one statistics group, at most one tile per (group, channel tile), case
`tables` — and against float64 elsewhere (case `s2`: a tile spans groups, every value is its own fp64 atomic, whose order no launch fixes).
Float64 convolution of the fp32 operands with the prologue applied in float64, at the pair kernels' bar (2e-6 of the output range; sums:
the same bar, as in test_conv_igemm_pairs_gpu), every case and variant, variant 5 behind a per-group affine + ReLU with non-zero
shifts included (padding contributes zero, not the shift).

Shapes.  The issue names "1x1, Cin 32, Cout 32, 70 rows: one chunk, partial 64x64 tile"; the pair modes have no 32-channel tile and reject
Cout <= 32 (test_conv_igemm_pairs_gpu.test_error_paths pins that for mode 3, and the new modes share its tiles), and 70 rows take the
128x64 tile.  So that case is split in three: Cout 32 is asserted to be REJECTED in modes 4 / 5 (test_error_paths), `1x1-70rows` (Cout 40:
one chunk, one partial 128x64 tile) and `1x1-40rows` (M <= 64: the partial 64x64 tile)."""
import ctypes as C

import pytest
import torch

from test_conv_igemm_pairs_gpu import BAR, Out, _desc, _rand, _reference, _table

pytestmark = pytest.mark.gpu
K1, K3 = (1, 1, 1), (3, 3, 3)
S1, S2, P0, P1 = (1, 1, 1), (2, 2, 2), (0, 0, 0), (1, 1, 1)


def _case(name):
    """name -> dict(x, w, b, k, stride, pad, and optionally aff, per_n, relu, groups, rows, finalize)."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def wgt(co, taps, ci):
        return _rand(g, co, taps, ci, scale=(1.0 / (taps * ci)) ** 0.5 * 3)
    if name in ("1x1-70rows", "1x1-40rows"):
        rows = 70 if name == "1x1-70rows" else 40
        return dict(x=_rand(g, 1, 1, rows // 10, 10, 32), w=wgt(40, 1, 32), b=_rand(g, 40, scale=0.2), k=K1, stride=S1, pad=P0)
    if name == "s2":            # 3 volumes of 6^3 -> 3^3 (81 rows: odd, rows beyond the tile), Cout 96 (columns beyond Cout), stride masks, sums
        x = _rand(g, 3, 6, 6, 6, 64) * (1.0 + torch.arange(3).view(3, 1, 1, 1, 1))
        return dict(x=x, w=wgt(96, 27, 64), b=_rand(g, 96, scale=0.2), k=K3, stride=S2, pad=P1, groups=3, rows=27)
    if name == "s1":            # 5 volumes of 4^3 (320 rows), Cin 64 -> 128: 128x128 with a forced split_k, 128x64 with the automatic one
        return dict(x=_rand(g, 5, 4, 4, 4, 64), w=wgt(128, 27, 64), b=_rand(g, 128, scale=0.2), k=K3, stride=S1, pad=P1)
    if name == "tables":        # 4 volumes of 4x4x8 (128 rows each = one 128x64 tile per statistics group), a table per 2 volumes, ReLU, finalize
        return dict(x=_rand(g, 4, 4, 4, 8, 32), w=wgt(64, 27, 32), b=None, k=K3, stride=S1, pad=P1, aff=(_rand(g, 2, 32) + 1.5, _rand(g, 2, 32) + 0.75),
                    per_n=2, relu=True, groups=4, rows=128, finalize=128)
    raise KeyError(name)


_REF = {}


def _ref(name):
    """The float64 reference of a case, computed once and shared."""
    if name not in _REF:
        c = _case(name)
        _REF[name] = (c, *_reference(c["x"], c["w"], c["b"], c["k"], c["stride"], c["pad"], aff=c.get("aff"), per_n=c.get("per_n", 0),
                                     relu=c.get("relu", False)))
    return _REF[name]


def _run(c, variant, table, slot="a", split_k=0, x=None, w=None):
    """ops.conv of case c on `variant` -> (Out, stats or None, fused finalize or None)."""
    from gen6d_amd import ops
    xs = c["x"] if x is None else x
    N, D, H, W = xs.shape[:4]
    Do, Ho, Wo = [(i + 2 * p - kk) // s + 1 for i, p, kk, s in zip((D, H, W), c["pad"], c["k"], c["stride"])]
    w = c["w"].cuda().contiguous() if w is None else w
    out = Out(N, Do, Ho, Wo, w.shape[0])
    st = torch.zeros((c["groups"], w.shape[0], 2), dtype=torch.float64, device="cuda") if c.get("groups") else None
    aff = c.get("aff")
    sc, sh = (aff[0].cuda(), aff[1].cuda()) if aff is not None else (None, None)
    r = ops.conv(xs if isinstance(xs, ops.PairMap) else xs.cuda(), w, c["b"].cuda() if c["b"] is not None else None, out.map, ksize=c["k"],
                 stride=c["stride"], pad=c["pad"], in_scale=sc, in_shift=sh, in_relu=c.get("relu", False), per_n=c.get("per_n", 0), stats=st,
                 rows_per_group=c.get("rows", 0), split_k=split_k, finalize=c.get("finalize"), pairs=(table, table.slot(slot), variant))
    torch.cuda.synchronize()
    return out, st, (r if c.get("finalize") else None)


def _check64(name, out, st, what):
    c, ref, _ = _ref(name)
    rng = float(ref.abs().max())
    e = float((out.map.cpu().double() - ref).abs().max()) / rng
    print(f"{name} {what}: error / range {e:.3e} (bar {BAR:.0e})")
    assert e <= BAR, (what, e)
    assert out.untouched(), "wrote outside the map"
    if st is not None:
        rows, co = c["rows"], ref.shape[-1]
        r3 = ref.reshape(c["groups"], rows, co)
        e1 = float((st.cpu()[:, :, 0] - r3.sum(1)).abs().max()) / rows / rng
        e2 = float((st.cpu()[:, :, 1] - (r3 * r3).sum(1)).abs().max()) / rows / rng ** 2
        print(f"{name} {what}: sums {e1:.3e}, squares {e2:.3e}")
        assert e1 <= BAR and e2 <= BAR, (what, e1, e2)


CASES = [("1x1-70rows", 0), ("1x1-40rows", 0), ("s2", 0), ("s1", 1), ("s1", 0), ("s1", 3), ("tables", 0)]


@pytest.mark.parametrize("name,split_k", CASES, ids=[f"{n}-split{k}" for n, k in CASES])
def test_bits_of_variant_3_and_float64(name, split_k):
    c, _, _ = _ref(name)
    t = _table()
    o3, s3, f3 = _run(c, 3, t, split_k=split_k)
    _check64(name, o3, s3, "variant 3")
    for v in (4, 5):
        o, s, f = _run(c, v, t, split_k=split_k)
        _check64(name, o, s, f"variant {v}")
        if v == 4 or c.get("aff") is None:
            assert torch.equal(o.map, o3.map), f"variant {v} differs from variant 3 in bits"
            if name == "tables":          # one tile per (group, channel tile): the fp64 sums have a fixed order
                assert torch.equal(s, s3), f"variant {v}: the fp64 sums differ from variant 3 in bits"
                assert torch.equal(f[0], f3[0]) and torch.equal(f[1], f3[1])
    assert t.read()["a"] > 0


def test_pair_map_slice_of_a_wider_map():
    """ld_in > 2 Cin: the operand is channels [32, 96) of a 96-channel pair map (affine_split16_to wrote the slice; the rest holds a guard
    pattern that must not be read): bits of variant 3 on the fp32 operand, and the launch itself writes no record."""
    from gen6d_amd import ops
    c, _, _ = _ref("s2")
    t = _table()
    o3, _, _ = _run(dict(c, groups=0, rows=0), 3, t)
    N, D, H, W, Cin = c["x"].shape
    wide = ops.new_map16(N * D, H, W, 96, 3, torch.device("cuda", 0), rng=(t, t.slot("p")))
    wide.data.fill_(1000.0)
    ops.affine_split16_to(c["x"].cuda().view(N * D, 1, H, W, Cin), None, None, 0, False, 3, wide, c_off=32)
    torch.cuda.synchronize()
    assert t.read()["p"] == float(c["x"].abs().max()), "the producer's record is the unscaled maximum"
    t.clear()
    xs = wide.view(N, D, H, W, 2, 96)[..., 32:96]
    o5, _, _ = _run(dict(c, groups=0, rows=0), 5, t, x=xs)
    assert torch.equal(o5.map, o3.map) and o5.untouched()
    assert int(t.rec.abs().max()) == 0, "a math_mode 5 launch wrote a record"


@pytest.mark.parametrize("variant", [4, 5])
@pytest.mark.parametrize("e", [3, -5])
def test_slot_exponents(variant, e):
    """Exponents +3 / -5 in the layer's slot: the result of exponent 0 within the bar, and the record — the loader's (4) or the pass's (5) —
    still holds the UNSCALED maximum."""
    c, ref, _ = _ref("s2")
    c = dict(c, groups=0, rows=0)
    t = _table()
    o0, _, _ = _run(c, variant, t)
    t.set_exponents({"a": e})
    t.clear()
    oe, _, _ = _run(c, variant, t)
    rng = float(ref.abs().max())
    d = float((oe.map.cpu().double() - o0.map.cpu().double()).abs().max()) / rng
    ee = float((oe.map.cpu().double() - ref).abs().max()) / rng
    print(f"variant {variant}, exponent {e}: against exponent 0 {d:.3e}, against float64 {ee:.3e} of the range (bar {BAR:.0e})")
    assert d <= BAR and ee <= BAR
    assert t.read()["a"] == float(c["x"].abs().max())


@pytest.mark.parametrize("variant", [4, 5])
def test_forced_filter_exponent(variant):
    """A forced w_exp (5 instead of the rule's) goes into the pack and the descriptor together: within the bar of the run on the rule's."""
    from gen6d_amd import ops
    c, ref, _ = _ref("1x1-70rows")
    t = _table()
    o0, _, _ = _run(c, variant, t)
    w = c["w"].cuda().contiguous()
    assert ops.pair_filter_exponent(w) != 5
    w.__dict__["_g6d_w_exp"] = 5
    o5, _, _ = _run(c, variant, t, w=w)
    rng = float(ref.abs().max())
    d = float((o5.map.cpu().double() - o0.map.cpu().double()).abs().max()) / rng
    print(f"variant {variant}, w_exp 5 against the rule's: {d:.3e} of the range")
    assert d <= BAR and float((o5.map.cpu().double() - ref).abs().max()) / rng <= BAR


def test_error_paths():
    """G6D_EINVAL with a message that names the condition, and nothing written: Cin % 32 != 0 in modes 4 / 5, a prologue or a multiplier in
    mode 5, a too-short and a misaligned ld_in in mode 5, and Cout <= 32 (no 32-channel tile) in both."""
    from gen6d_amd import lib
    L = lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros((1, 1, 4, 4, 64), device="cuda")
    x16 = torch.zeros((1, 1, 4, 4, 2, 64), dtype=torch.float16, device="cuda")
    w = torch.zeros((64, 1, 64), device="cuda")
    tab = torch.ones(64, device="cuda")
    out = Out(1, 1, 4, 4, 64)
    d40 = dict(Cin=40, ld_in=40)
    cases = [(_desc(x, w, out.map, math_mode=4, **d40), "Cin % 32"),
             (_desc(x, w, out.map, math_mode=5, Cin=40, ld_in=80), "Cin % 32"),
             (_desc(x16[..., 0, :], w, out.map, math_mode=5, ld_in=128, in_scale=tab.data_ptr(), in_shift=tab.data_ptr()), "no prologue"),
             (_desc(x16[..., 0, :], w, out.map, math_mode=5, ld_in=128, mul=x.data_ptr()), "no multiplier"),
             (_desc(x16[..., 0, :], w, out.map, math_mode=5, ld_in=112), "ld_in"),
             (_desc(x16[..., 0, :], w, out.map, math_mode=5, ld_in=136), "ld_in"),
             (_desc(x, w, out.map, math_mode=4, Cout=32, ld_out=32), "Cout > 32"),
             (_desc(x16[..., 0, :], w, out.map, math_mode=5, ld_in=128, Cout=32, ld_out=32), "Cout > 32")]
    for d, word in cases:
        assert L.g6d_conv_igemm_ex(C.byref(d), None, stream) == -1
        assert word in L.g6d_last_error().decode(), (word, L.g6d_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out.buf == 12345.0).all()), "a rejected launch wrote"
    # the accepted twin of the mode-5 descriptors above (so the rejections are about the named condition, not the test's descriptor)
    d = _desc(x16[..., 0, :], w, out.map, math_mode=5, ld_in=128)
    assert L.g6d_conv_igemm_ex(C.byref(d), None, stream) == 0
    torch.cuda.synchronize()
    assert bool((out.map == 0).all()) and out.untouched()
    assert L.g6d_conv_plan(C.byref(d)) == 5
