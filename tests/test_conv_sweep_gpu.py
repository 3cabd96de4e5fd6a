"""The descriptor sweep on a real MI355X: every case of tests/conv_sweep.py through gen6d_amd.ops.conv against tests/ref_ops.conv in
float64, one test per cell (a route of g6d_conv_igemm: family, tile, loader prologue, split class, row order — conv_sweep's docstring).

Per case:
  route    before the launch g6d_conv_route (the launcher's own decision code) files the descriptor in the case's cell — a clamped cell
           reports split_source 3 under the small workspace the test hands out — and after it the ops.PROFILE label names the family;
  parity   map, statistics and finalised affine within the bar of the existing test of that family (conv_sweep.BARS quotes test and
           figure: 2e-5 implicit GEMM / LDS patch / narrow, 4e-5 F(2x2,3x3), 1e-5 and 2e-5 F(4x4,3x3), 2e-6 pairs in that test's
           metrics), the sentinel columns of the output rows keep their bits;
  repeat   a second launch on the same operands and the same workspace gives the same map bits (statistics pass through fp64 atomics
           and are excluded, as in tests/test_guarded_memory_gpu.py; no split launch adds its partials with atomics), and after EACH
           launch the tile counters at the head of the workspace and the finalisation counter are zero: the header's "every call
           leaves them zero".
Each cell records its worst error over its bar (parity_log)."""
import pytest
import torch

import conv_case
import conv_sweep as S
import parity_log
import ref_ops

pytestmark = pytest.mark.gpu

COUNTER_INTS = S.COUNTER_BYTES // 4


@pytest.fixture(scope="module")
def ops():
    from gen6d_amd import lib, ops as _ops
    lib.load()
    assert torch.cuda.is_available()
    return _ops


def _label_family(label):
    return 3 if label.startswith("wino3x3 F43 ") else 2 if label.startswith("wino3x3 ") else 5 if label.startswith("conv16x3 igemm ") else 0


def _pair_stat_errs(stats, rstats, rows, rng):
    s, r = stats.detach().cpu(), rstats
    return float((s[..., 0] - r[..., 0]).abs().max()) / rows / rng, float((s[..., 1] - r[..., 1]).abs().max()) / rows / rng ** 2


def _run_case(ops, case, knob, monkeypatch):
    """-> worst error / bar of the case."""
    from gen6d_amd.network.backbone import winograd43_filters_taps
    cell = S.CELLS[case["cell"]]
    fam = cell["family"]
    bar = S.BARS[fam]
    for name, value in case.get("knobs", {}).items():
        knob(name, value)
    o = conv_case.operands(case)
    dv = conv_case.device_operands(o)
    extra = {}
    if case.get("wino"):
        extra["w_wino"] = conv_case.wino_u(o.w, case["k"]).cuda()
    if case.get("wino43"):
        extra["w_wino43"] = winograd43_filters_taps(o.w, case["k"][0]).cuda()
    if case.get("pairs"):
        table = ops.RangeTable(torch.device("cuda", 0))
        extra["pairs"] = (table, table.slot("a"), case["pairs"])
    if "ws_bytes" in case:       # a zeroed workspace with room for fewer splits than the automatic rule wants
        small = torch.zeros(case["ws_bytes"] // 4, dtype=torch.float32, device="cuda")
        monkeypatch.setattr(ops, "workspace", lambda device: small)
    ws = ops.workspace(dv.x.device)
    counters = []
    new_counter = ops.new_counter
    monkeypatch.setattr(ops, "new_counter", lambda device: counters.append(new_counter(device)) or counters[-1])
    fin = bool(case.get("fin"))
    maps, results = [], []
    for launch in range(2):
        stats = torch.zeros((o.G, o.Cout, 2), dtype=torch.float64, device="cuda") if o.stats else None
        ops.ROUTE, ops.PROFILE, ops.PROFILE_HBM = [], [], {}
        try:
            res = conv_case.launch(ops, o, dv, stats, finalize=fin, **extra)
            torch.cuda.synchronize()
            route, = ops.ROUTE
            labels, hbm = [p[3] for p in ops.PROFILE], dict(ops.PROFILE_HBM)
        finally:
            ops.ROUTE = ops.PROFILE = ops.PROFILE_HBM = None
        assert S.cell_matches(case, route), f"{case['id']}: routed to {S.classify(route)} (family {route.family}, mode {route.mode}, splits {route.splits})"
        if cell.get("split") == "clamped":
            assert route.split_source == 3 and route.splits <= case["ws_fit"], (case["id"], route.splits, route.split_source)
        if fam == 4:
            assert not labels and "conv_narrow" in hbm, case["id"]
        else:
            assert len(labels) == 1 and _label_family(labels[0]) == (0 if fam == 1 else fam), (case["id"], labels)
        assert not bool(ws[:COUNTER_INTS].view(torch.int32).any()), f"{case['id']}: launch {launch} left tile counters set"
        assert all(not bool(t.any()) for t in counters), f"{case['id']}: launch {launch} left the finalisation counter set"
        maps.append(dv.outbuf.clone())
        results.append((stats, res))
    assert torch.equal(maps[0], maps[1]), f"{case['id']}: the second launch changed bits of the map"
    stats, res = results[0]
    ref, rstats = conv_case.reference(o)
    worst = conv_case.rel_err(dv.out, ref) / bar["map"]
    assert worst <= 1.0, f"{case['id']}: map error {worst * bar['map']:.3e} > {bar['map']}"
    if o.ld_out != o.Cout:
        assert bool((dv.outbuf[..., o.Cout:] == conv_case.SENTINEL).all()), f"{case['id']}: wrote outside its channel slice"
    if stats is not None:
        if fam == 5:
            e1, e2 = _pair_stat_errs(stats, rstats, o.count, float(ref.abs().max()))
        else:
            e1, e2 = conv_case.rel_err(stats[..., 0], rstats[..., 0]), conv_case.rel_err(stats[..., 1], rstats[..., 1])
        assert max(e1, e2) <= bar["stats"], f"{case['id']}: statistics error {e1:.3e}, {e2:.3e} > {bar['stats']}"
        worst = max(worst, e1 / bar["stats"], e2 / bar["stats"])
        if fin:
            sc_f, sh_f = res
            sc_k, sh_k = ops.stats_finalize(stats, o.count)
            assert torch.equal(sc_f, sc_k) and torch.equal(sh_f, sh_k), f"{case['id']}: fused finalisation differs from g6d_stats_finalize"
            if bar["fin"]:
                rsc, rsh = ref_ops.stats_finalize(rstats, o.count)
                e3, e4 = conv_case.rel_err(sc_f, rsc.double()), conv_case.rel_err(sh_f, rsh.double())
                assert max(e3, e4) <= bar["fin"], f"{case['id']}: finalised affine error {e3:.3e}, {e4:.3e} > {bar['fin']}"
                worst = max(worst, e3 / bar["fin"], e4 / bar["fin"])
    return worst


@pytest.mark.parametrize("cid", list(S.CELLS), ids=list(S.CELLS))
def test_cell(ops, cid, knob, monkeypatch):
    from gen6d_amd import lib
    worst = 0.0
    for case in S.CELLS[cid]["cases"]:
        before = {name: lib.get_knob(name) for name in case.get("knobs", {})}
        with monkeypatch.context() as m:
            worst = max(worst, _run_case(ops, case, knob, m))
        for name, value in before.items():          # the next case starts from the policy this one found
            knob(name, value)
    fam = S.CELLS[cid]["family"]
    print(f"{cid}: {len(S.CELLS[cid]['cases'])} cases, worst error / bar {worst:.3f} ({S.BARS[fam]['src']})")
    parity_log.record(f"test_conv_sweep_gpu::test_cell[{cid}]", "worst error / bar", worst, 1.0, note=S.BARS[fam]["src"])


def test_in_relu_alone_is_refused(ops):
    """in_relu without the affine used to be dropped by every kernel family: ops.conv raises, the library answers G6D_EINVAL."""
    import ctypes as C
    from gen6d_amd import lib
    x = torch.zeros((1, 1, 4, 4, 8), device="cuda")
    w = torch.zeros((40, 9, 8), device="cuda")
    out = torch.zeros((1, 1, 4, 4, 40), device="cuda")
    with pytest.raises(ValueError, match="in_relu"):
        ops.conv(x, w, None, out, ksize=(1, 3, 3), pad=(0, 1, 1), in_relu=True)
    d = lib.G6dConv(in_=x.data_ptr(), weight=w.data_ptr(), out=out.data_ptr(), N=1, Di=1, Hi=4, Wi=4, Cin=8, ld_in=8, Do=1, Ho=4, Wo=4, Cout=40,
                    ld_out=40, kd=1, kh=3, kw=3, sd=1, sh=1, sw=1, pd=0, ph=1, pw=1, in_relu=1)
    assert lib.load().g6d_conv_igemm(C.byref(d), None) == -1
    assert b"in_relu requires in_scale" in lib.load().g6d_last_error()
