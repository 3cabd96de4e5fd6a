"""The 16-bit sweep on a real MI355X: every case of tests/conv16_sweep.py through g6d_conv16_direct_multi_ex / g6d_corr16_multi_ex, one
test per cell (what the host code chooses: kernel, arithmetic, tiling shape of the first segment, block form — conv16_sweep's docstring).
Outputs are caller-made, NaN-filled and guarded (the Guarded idea of tests/test_conv16w_edges_gpu.py: guard channels on both sides of
every pixel row, guard elements around the map; the statistics table lies between two guard groups).

Per case:
  route    before the launch g6d_conv16_direct_route (the launcher's own decision code), on the launch's own segment table, files the
           case in its cell; corr16 cases are filed by corr16g::pick_tile through tests/corr16_geom_shim.cpp;
  parity   every output against the float64 convolution (16-bit modes: of the rounded operands) at the bars of the tests these kernels
           already answer to, in those tests' metrics (conv16_sweep.BARS quotes test and figure): pairs 2e-6 of the output range + 2^-21
           for a pair output, sums 2e-6 and squares 4e-6 per pixel of a group; 16-bit 2e-5 + half an ulp of a 16-bit output, 2e-5 /
           4e-5; corr16 2e-6 / 2e-5.  A NaN left in an output — a pixel never written — fails parity;
  guard    every guard element keeps its NaN, the statistics guard groups keep their fill;
  repeat   a second launch on the same operands into fresh buffers gives the same bits, guards included (statistics pass through fp64
           atomics and are excluded, as in tests/test_conv_sweep_gpu.py).
Each cell records its worst error over its bar (parity_log)."""
import ctypes as C

import pytest
import torch

import conv16_case as CC
import conv16_sweep as S
import parity_log

pytestmark = pytest.mark.gpu

GUARD_CH, GUARD_EL, GUARD_FILL = 8, 4096, 12345.0


@pytest.fixture(scope="module")
def ops():
    from gen6d_amd import lib, ops as _ops
    lib.load()
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    return CC.build_shims(str(tmp_path_factory.mktemp("c16sweep")))


class Guarded:
    """An output map of `pixels` rows of `width` elements inside a NaN-filled buffer: `left` + width + GUARD_CH elements per row (the map is
    a channel slice of wider rows), GUARD_EL elements before and after."""

    def __init__(self, pixels, width, dtype, left=GUARD_CH):
        self.ld = left + width + GUARD_CH
        self.n = pixels * self.ld
        self.buf = torch.full((self.n + 2 * GUARD_EL,), float("nan"), dtype=dtype, device="cuda")
        self.rows = self.buf[GUARD_EL:GUARD_EL + self.n].view(pixels, self.ld)
        self.map = self.rows[:, left:left + width]
        self.left, self.width = left, width

    def untouched(self):
        b = self.buf.cpu()
        r = b[GUARD_EL:GUARD_EL + self.n].view(self.rows.shape)
        return bool(torch.isnan(b[:GUARD_EL]).all() and torch.isnan(b[GUARD_EL + self.n:]).all() and torch.isnan(r[:, :self.left]).all()
                    and torch.isnan(r[:, self.left + self.width:]).all())

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.element_size() == 2 else torch.int32)


def _launch(ops, case, o, filt, bias, shims):
    """One launch of the case on fresh guarded outputs -> (fulls, pools, statistics table with its two guard groups)."""
    from gen6d_amd import lib
    l = lib.load()
    c = case
    pair = o.pair
    Cout, Cin = c["Cout"], c["Cin"]
    segs = (lib.G6dConv16Seg * len(c["segs"]))()
    fulls, pools = [], []
    for i, (N, D, H, W) in enumerate(c["segs"]):
        def make(kind, px, left=GUARD_CH):
            if kind is None:
                return None
            return Guarded(px, Cout * (2 if pair and kind == "t16" else 1), CC.T16[o.mode] if kind == "t16" else torch.float32, left)
        # (wide: the fp32 full map is a channel slice that starts 64 channels into wider rows)
        f = make(c["full"], N * D * H * W, GUARD_CH + (64 if c["wide"] else 0))
        q = make(c["pool"], N * (H // 2) * (W // 2))
        fulls.append(f); pools.append(q)
        segs[i] = lib.G6dConv16Seg(in_=o.dev[i].data_ptr(), out_full=f.map.data_ptr() if f else None, out_pool=q.map.data_ptr() if q else None, N=N, D=D, H=H, W=W,
                                   ld_in=(2 if pair else 1) * Cin, ld_full=f.ld if f else 0, ld_pool=q.ld if q else 0)
    G = S.stat_groups(c)
    table = None
    if G:
        table = torch.zeros((G + 2, Cout, 2), dtype=torch.float64, device="cuda")
        table[0] = GUARD_FILL
        table[-1] = GUARD_FILL
    stats_ptr = C.c_void_p(table[1:].data_ptr()) if G else C.c_void_p(0)
    if o.corr:
        k = c["kd"]
        full_grid = (C.c_int * (40 * 40 * 5))()
        shims["corr"].g_pick_grid(k, 40, 40, full_grid)
        _, _, H0, W0 = c["segs"][0]
        tl2 = full_grid[((H0 - 1) * 40 + (W0 - 1)) * 5]
        assert tl2 >= 0 and S.c_cell("pairs" if pair else "b16", k, 1 << tl2) == c["cell"], f"{c['id']}: pick_tile files it under tile width {1 << tl2}"
        lib.check(l.g6d_corr16_multi_ex(segs, len(c["segs"]), Cin, C.c_void_p(filt.data.data_ptr()), float(filt.acc_scale), 32, k, int(o.mode), None,
                                        ops._stream()), "g6d_corr16_multi_ex")
    else:
        args = (segs, len(c["segs"]), Cin, C.c_void_p(filt.data.data_ptr()), int(filt.layout), Cout, c["kd"], S.type_code(c, c["full"]),
                S.type_code(c, c["pool"]), int(o.mode), stats_ptr, int(c["rpg"]))
        r = lib.G6dConv16Route()
        lib.check(l.g6d_conv16_direct_route(*args, C.byref(r)), "g6d_conv16_direct_route")
        assert S.classify(c, r) == c["cell"], f"{c['id']}: routed to {S.classify(c, r)} (kernel {r.kernel}, wm {r.wm}, half {r.half_tile}, folded {r.folded})"
        assert r.kernel == (2 if c["stats"] == "passes" else (0 if c["fam"] == "T" else 1)), (c["id"], r.kernel)
        lib.check(l.g6d_conv16_direct_multi_ex(segs, len(c["segs"]), Cin, C.c_void_p(filt.data.data_ptr()), int(filt.layout), float(filt.acc_scale),
                                               C.c_void_p(bias.data_ptr()), Cout, c["kd"], int(c["relu"]), S.type_code(c, c["full"]), S.type_code(c, c["pool"]),
                                               int(o.mode), stats_ptr, int(c["rpg"]), None, ops._stream()), "g6d_conv16_direct_multi_ex")
    torch.cuda.synchronize()
    return fulls, pools, table


def _run_case(ops, case, knob, shims):
    """-> worst error / bar of the case."""
    for name, value in case["knobs"].items():
        knob(name, value)
    o = CC.operands(case)
    o.dev = [x.cuda() for x in o.x16]
    if o.corr:
        filt, bias = ops.corr16_pack(o.w.cuda(), o.mode), None
    else:
        filt, bias = ops.conv16_pack(o.w.cuda(), o.mode, case["layout"]), o.b.cuda()
        assert filt.layout == case["layout"] and filt.Cout == case["Cout"]
    runs = [_launch(ops, case, o, filt, bias, shims) for _ in range(2)]
    fulls, pools, table = runs[0]
    for gd, again in zip(fulls + pools, runs[1][0] + runs[1][1]):
        if gd is not None:
            assert gd.untouched() and again.untouched(), f"{case['id']}: wrote outside an output map"
            assert torch.equal(gd.bits(), again.bits()), f"{case['id']}: the second launch changed bits of an output"
    stats = None
    if table is not None:
        got = table.cpu()
        assert bool((got[0] == GUARD_FILL).all() and (got[-1] == GUARD_FILL).all()), f"{case['id']}: statistics were added outside the table's groups"
        stats = got[1:-1]
    ref = CC.reference(o)
    worst, bad = CC.grade(case, ref, [None if f is None else f.map for f in fulls], [None if q is None else q.map for q in pools], stats)
    assert not bad, "\n".join(bad)
    return worst


@pytest.mark.parametrize("cid", list(S.CELLS), ids=list(S.CELLS))
def test_cell(ops, cid, knob, shims):
    from gen6d_amd import lib
    worst = 0.0
    for case in S.CELLS[cid]["cases"]:
        before = {name: lib.get_knob(name) for name in case["knobs"]}
        worst = max(worst, _run_case(ops, case, knob, shims))
        for name, value in before.items():          # the next case starts from the policy this one found
            knob(name, value)
    src = CC.bars_of(S.CELLS[cid]["cases"][0])["src"]
    print(f"{cid}: {len(S.CELLS[cid]['cases'])} cases, worst error / bar {worst:.3f} ({src})")
    parity_log.record(f"test_conv16_sweep_gpu::test_cell[{cid}]", "worst error / bar", worst, 1.0, note=src)
