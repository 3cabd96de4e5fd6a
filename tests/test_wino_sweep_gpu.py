"""The Winograd sweep (tests/wino_sweep.py) on a real MI355X: one test per cell — one outcome of the host's choice of block form, split of
the chunk list, kernel instantiation and F(4x4,3x3) block-id decode — runs the cell's cases under their knobs, twice each, through
gen6d_amd.lib with explicit row lengths and an explicit workspace pointer and byte count (tests/wino_case.py).

  reference   float64 on the CPU: F.conv2d + bias (+ ReLU) (+ F.max_pool2d(2, 2)); the correlations: ref_ops.corr2d_patch
  bars        wino_sweep.BARS, each borrowed from the hand-written test of its entry point and not retuned; metric max |error| /
              max |reference| per segment and output kind.  The 16-bit cells are graded twice: against float64 (TOL[mode]) and against the
              ref_ops restatement of the kernel's arithmetic (3e-4)
  route       immediately before each launch g6d_wino_multi_route (the launchers' own code), on the live pointers, files the launch in the
              cell under test
  re-arming   the second launch returns bit-identical maps and the workspace's counter region reads zero afterwards
  slack       outputs are prefilled with a sentinel: channels beyond Cout of a row and the gaps between segments keep it; no map holds
              NaN, although every input float outside the segments' Cin-channel slices is NaN; an output kind the case does not ask for is
              passed as NULL

On a miss the message names the worst element's segment, coordinates and position modulo 8 (F(4x4,3x3): modulo the 4x4 tile)."""
import ctypes as C

import pytest
import torch

import wino_case as WC
import wino_sweep as S
from gen6d_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ws():
    lib.load()
    assert torch.cuda.is_available()
    return torch.zeros(S.AMPLE // 4, dtype=torch.float32, device="cuda")      # zero once: every launch leaves the counters at zero


def _run(case, cid, ws):
    dev = torch.device("cuda")
    o = WC.operands(case)
    ref = WC.reference(case, o)
    live = WC.Live(case, o, dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fails, outs = [], []
    with WC.knobs(case):
        for rep in range(2):
            live.prefill()
            rc, r, ra = WC.routes(case, live.table, live.U.data_ptr(), ws.data_ptr())
            assert rc == 0 and S.classify_case(case, r, ra) == cid, f"{case['id']}: the live launch routes to {S.classify_case(case, r, ra) if rc == 0 else rc}"
            lib.check(WC.launch(case, live.table, live.U.data_ptr(), live.bias.data_ptr() if live.bias is not None else 0, ws.data_ptr(), stream), case["entry"])
            torch.cuda.synchronize()
            outs.append(live.maps())
            fails += [f"launch {rep}: {m}" for m in live.slack_errors()]
            if bool(ws[:S.COUNTER_BYTES // 4].view(torch.int32).any()):
                fails.append(f"{case['id']} launch {rep}: a tile counter of the workspace was left set")
                ws[:S.COUNTER_BYTES // 4].zero_()
    for i, (a, b) in enumerate(zip(*outs)):
        for kind, x, y in (("full", a[0], b[0]), ("pool", a[1], b[1])):
            if x is not None and not torch.equal(x, y):
                fails.append(f"{case['id']} {kind} segment {i}: the second launch differs from the first; {WC.where(y, x, 8)}")
    fam = case["fam"]
    if fam == "W16":
        worst, f1 = WC.grade(case, ref, outs[0], S.TOL16[case["mode"]])
        w2, f2 = WC.grade(case, WC.restatement16(case, o), outs[0], S.BARS[fam]["restated"])
        return max(worst, w2), fails + f1 + ["against the restated arithmetic: " + m for m in f2]
    worst, f1 = WC.grade(case, ref, outs[0], S.BARS[fam]["bar"])
    return worst, fails + f1


@pytest.mark.parametrize("cid", list(S.CELLS))
def test_cell(cid, ws):
    worst, worst_id, fails = 0.0, None, []
    for case in S.CELLS[cid]["cases"]:
        ratio, f = _run(case, cid, ws)
        fails += f
        if ratio >= worst:
            worst, worst_id = ratio, case["id"]
    print(f"cell {cid}: worst error / bar {worst:.3f} ({worst_id})")
    assert not fails, f"{len(fails)} findings in cell {cid}:\n" + "\n".join(fails[:12])
