"""The descriptor sweep (tests/conv_sweep.py) checked on a host WITHOUT a GPU: every sampled descriptor, built as gen6d_amd.ops.conv builds
it on fake operand addresses (tests/launch_contract.py), is ACCEPTED by g6d_conv_igemm(_ex) — it reaches the launch and fails there with
G6D_ELAUNCH — and g6d_conv_route files it in the cell the sampler filed it under; every cell holds its cases, every excluded cell is
unreachable, every listed value of the free dimensions occurs, and torch's own fp32 convolution of every case of families 0, 1 and 4
stays within half of the family's bar (so a bar is never missed, or met, because of the case instead of the kernel).

The calls that launch carry FAKE device pointers: skipped where a GPU is visible, as tests/test_launch_contract_cpu.py."""
import ctypes as C

import pytest
import torch

import conv_case
import conv_sweep as S
import launch_contract as LC
from gen6d_amd import lib

ELAUNCH = -3
WORKSPACE_BYTES = 96 << 20          # gen6d_amd.ops.WORKSPACE_BYTES
NAMES = ("in", "mul", "in_scale", "in_shift", "weight", "bias", "out", "stats", "workspace", "weight_wino", "weight_wino43", "fin_scale",
         "fin_shift", "fin_counter")
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="issues calls on fake device pointers: only where no GPU is visible")


def _ptr(name):
    return LC.dev(LC.SEG_PTRS + NAMES.index(name))


def _desc(case):
    return S.descriptor(case, lib.G6dConv, _ptr, WORKSPACE_BYTES)


class _knobs:
    def __init__(self, case):
        self.case = case

    def __enter__(self):
        for k, v in self.case.get("knobs", {}).items():
            lib.set_knob(k, v)

    def __exit__(self, *exc):
        lib.reset_knobs()
        return False


def _route(case):
    """-> (rc, lib.G6dConvRoute, g6d_conv_plan's answer) under the case's knobs."""
    l = lib.load()
    d = _desc(case)
    r = lib.G6dConvRoute()
    with _knobs(case):
        rc = l.g6d_conv_route(C.byref(d), C.byref(r))
        plan = l.g6d_conv_plan(C.byref(d))
    return rc, r, plan


def _show(case, rc, r):
    return (f"{case.get('id')}: rc {rc} ({lib.load().g6d_last_error().decode()!r}) family {r.family} tile {r.bm}x{r.bn} mode {r.mode} splits {r.splits} "
            f"source {r.split_source} pm {r.position_major}; case { {k: v for k, v in case.items() if k not in ('id', 'cell')} }")


def test_counts_and_ids():
    ids = [c["id"] for c in S.CASES]
    assert len(set(ids)) == len(ids)
    thin = {cid: len(cell["cases"]) for cid, cell in S.CELLS.items() if len(cell["cases"]) < 4}
    assert not thin, f"cells with fewer than 4 cases: {thin}"
    assert len(S.CASES) >= 250
    assert not set(S.CELLS) & {e["id"] for e in S.EXCLUDED}
    per_family = {f: sum(S.CELLS[c["cell"]]["family"] == f for c in S.CASES) for f in range(6)}
    print(f"conv sweep: {len(S.CASES)} cases in {len(S.CELLS)} cells ({len(S.EXCLUDED)} excluded); per family {per_family}")


def test_every_case_lands_in_its_cell_and_plan_agrees():
    wrong = []
    for case in S.CASES:
        rc, r, plan = _route(case)
        if rc != 0 or not S.cell_matches(case, r) or plan != r.family:
            wrong.append(_show(case, rc, r) + f" plan {plan}")
    assert not wrong, f"{len(wrong)} of {len(S.CASES)} cases off their cell:\n" + "\n".join(wrong[:12])


def test_sizes_stay_small():
    """M * K * Cout <= 2^26 (position-major cells and the unsplit 128x128 cell may pass it) and K within the borrowed bar's test."""
    for case in S.CASES:
        cell = S.CELLS[case["cell"]]
        fam = cell["family"]
        free = fam in (0, 5) and (cell["pm"] or case.get("knobs", {}).get("conv_pm") == 0 or (cell["bm"], cell["bn"], cell["split"]) == (128, 128, "none"))
        assert free or S.work_of(case) <= S.MAX_WORK, case["id"]
        assert S.work_of(case) <= 8 * S.MAX_WORK, case["id"]
        assert case["k"][0] * case["k"][1] * case["k"][2] * case["Cin"] <= S.MAX_K[fam], case["id"]


@no_gpu
def test_every_case_is_accepted_by_the_launcher():
    l = lib.load()
    refused = []
    for case in S.CASES:
        d = _desc(case)
        with _knobs(case):
            if case.get("pairs"):
                rng = lib.G6dRange16(exps=None, rec=None, slot_in=-1, slot_out=-1)
                rc = l.g6d_conv_igemm_ex(C.byref(d), C.cast(C.pointer(rng), C.c_void_p), None)
            else:
                rc = l.g6d_conv_igemm(C.byref(d), None)
        if rc != ELAUNCH:
            refused.append(f"{case['id']}: rc {rc} {l.g6d_last_error().decode()!r}")
    assert not refused, f"{len(refused)} refused (a sampler bug, not a skip):\n" + "\n".join(refused[:12])


def test_excluded_cells_are_unreachable():
    """A descriptor built for an excluded cell routes to another cell or is refused."""
    for ex in S.EXCLUDED:
        case = S.probe_of(ex)
        rc, r, _ = _route(case)
        if rc != 0:
            continue
        fam = ex["family"]
        if fam in (0, 5):
            got = (r.family, r.bm, r.bn, r.mode, r.position_major)
            want = (fam, ex["bm"], ex["bn"], ex["mode"], ex["pm"])
            split = "clamped" if r.split_source == 3 else ("none" if r.splits == 1 else ("forced" if r.split_source == 1 else "auto"))
            assert got != want or split != ex["split"], f"excluded cell {ex['id']} was reached: {_show(case, rc, r)}"
        else:
            assert r.family != fam, f"excluded cell {ex['id']} was reached: {_show(case, rc, r)}"
            near = S.probe_neighbour(ex)                  # ... and only the excluded property turned it away: its neighbour runs there
            nrc, nr, _ = _route(near)
            assert nrc == 0 and nr.family == fam, f"the neighbour of the probe for {ex['id']} is not on family {fam}: {_show(near, nrc, nr)}"
        assert ex["file"] and ex["condition"]


def test_in_relu_alone_is_refused():
    """The one hole the sweep's domain had: in_relu without the affine was dropped by every kernel.  Now G6D_EINVAL, in the launcher and
    in the route report (and a ValueError in ops.conv: tests/test_conv_sweep_gpu.py)."""
    case = dict(N=2, D=1, H=7, W=7, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), Cin=8, Cout=40)
    d = _desc(case)
    d.in_relu = 1
    r = lib.G6dConvRoute()
    assert lib.load().g6d_conv_route(C.byref(d), C.byref(r)) == -1
    assert b"in_relu requires in_scale" in lib.load().g6d_last_error()


def test_forced_split_beyond_the_counters_is_refused_not_clamped():
    """More tiles than tile counters: an automatic split never gets here (it needs < 256 blocks), a forced one is G6D_ENOSPC."""
    case = dict(N=4100, D=1, H=8, W=16, k=(1, 1, 1), s=(1, 1, 1), p=(0, 0, 0), Cin=64, Cout=8, split=2)
    rc, r, _ = _route(case)
    assert rc == -2


def test_forced_split_counts_are_rounded_as_launch_mm_rounds_them():
    """A forced split_k = s cuts the `total` K steps into ranges of ips = ceil(total / s) steps; ranges past the last step hold no work
    and the grid drops them: ceil(total / ips) splits (igemm_round_splits).  Every forced case reports exactly that count, and the draw
    holds cases where it is smaller than split_k."""
    rounded = []
    for case in S.CASES:
        cell = S.CELLS[case["cell"]]
        if cell["family"] not in (0, 5) or cell["split"] != "forced":
            continue
        total, s = S.total_of(case), case["split"]
        ips = -(-total // min(s, total))
        want = -(-total // ips)
        rc, r, _ = _route(case)
        assert rc == 0 and r.splits == want and r.split_source == 1, (case["id"], total, s, want, r.splits)
        if want < s:
            rounded.append((case["id"], total, s, want))
    print(f"forced splits rounded down: {rounded}")
    assert len(rounded) >= 2, rounded
    # the arithmetic itself, on a fixed descriptor: 15 K steps (1x5x3 taps, one channel chunk) forced to 7 -> ranges of 3 -> 5 blocks
    fixed = dict(N=2, D=1, H=9, W=9, k=(1, 5, 3), s=(1, 1, 1), p=(0, 2, 1), Cin=32, Cout=40, split=7)
    rc, r, _ = _route(fixed)
    assert (rc, r.splits, r.split_source) == (0, 5, 1)


def _seen(pred):
    return {f for c in S.CASES if pred(c) for f in [S.CELLS[c["cell"]]["family"]]}


def test_free_dimensions_occur():
    fams_all = {0, 1, 2, 3, 4, 5}
    igemm = {0, 5}
    same = lambda c, a: c["p"][a] == c["k"][a] // 2
    need = {
        "kd=1": (lambda c: c["k"][0] == 1, fams_all), "kd=3": (lambda c: c["k"][0] == 3, {0, 1, 2, 3, 5}),
        "kh!=kw": (lambda c: c["k"][1] != c["k"][2], igemm),
        "stride 2": (lambda c: 2 in c["s"], igemm), "stride 1": (lambda c: set(c["s"]) == {1}, fams_all),
        "no padding": (lambda c: c["k"][1] > 1 and c["p"][1] == 0, igemm), "same padding": (lambda c: c["k"][1] > 1 and same(c, 1), fams_all),
        "padding > same": (lambda c: c["p"][1] > c["k"][1] // 2 or c["p"][2] > c["k"][2] // 2, igemm),
        "odd sizes": (lambda c: c["H"] % 2 == 1 and c["W"] % 2 == 1, fams_all),
        "ld_in > Cin at an offset": (lambda c: c.get("ld_in", c["Cin"]) >= c["Cin"] + 64, fams_all),
        "ld_out > Cout": (lambda c: c.get("ld_out", c["Cout"]) > c["Cout"], fams_all),
        "no bias": (lambda c: c.get("no_bias"), fams_all), "bias": (lambda c: not c.get("no_bias"), fams_all),
        "act 0": (lambda c: c.get("act", 0) == 0, fams_all), "act 1": (lambda c: c.get("act") == 1, fams_all), "act 2": (lambda c: c.get("act") == 2, {0, 1, 4, 5}),
        "ragged per_n": (lambda c: c.get("per_n") and c["N"] % c["per_n"], {0, 1, 2, 3, 5}),
        "in_mod": (lambda c: c.get("in_mod"), {0, 2}), "mul_group": (lambda c: c.get("mul_group"), {0, 2}),
        "stats none": (lambda c: S.stats_kind(c) == "none", fams_all), "stats one group": (lambda c: S.stats_kind(c) == "one", {0, 1, 2, 3, 5}),
        "stats aligned": (lambda c: S.stats_kind(c) == "aligned", {0, 1, 5}), "stats straddle": (lambda c: S.stats_kind(c) == "straddle", {0, 1, 2, 3, 5}),
        "finalise on": (lambda c: c.get("stats") and c.get("fin"), {0, 1, 2, 3, 5}), "finalise off": (lambda c: c.get("stats") and not c.get("fin"), {0, 1, 2, 3, 5}),
        "relu with the affine": (lambda c: c.get("relu") and c.get("aff"), {0, 1, 2, 3, 5}),
    }
    for v in S.CIN_TAIL:
        need[f"Cin={v}"] = ((lambda c, v=v: c["Cin"] == v), {0, 1})
    need["Cin with a tail chunk"] = (lambda c: c["Cin"] % 32, fams_all)
    for v in S.COUT_PARTIAL:
        need[f"Cout={v}"] = ((lambda c, v=v: c["Cout"] == v), {0} | ({1} if v <= 40 else set()) | ({5} if v > 32 else set()) | ({4} if v <= 3 else set()))
    for v in (3, 4, 5):
        need[f"pairs variant {v}"] = ((lambda c, v=v: c.get("pairs") == v), {5})
    missing = {name: sorted(fams - _seen(pred)) for name, (pred, fams) in need.items() if fams - _seen(pred)}
    assert not missing, f"free-dimension values that never occur (value: families): {missing}"
    assert not [c["id"] for c in S.CASES if c.get("relu") and not c.get("aff")], "relu is drawn only with the affine"
    for c in S.CASES:                                       # the documented domain
        assert not c.get("rpg") or (c["rpg"] % (S.rows_of(c) // c["N"]) == 0 and S.rows_of(c) % c["rpg"] == 0), c["id"]
        assert not c.get("mul") or c.get("aff"), c["id"]


FP32_RATIO = {}


@pytest.mark.parametrize("fam", [0, 1, 2, 3, 4, 5])
def test_reference_precision(fam):
    """torch's CPU fp32 conv3d of every case against the float64 reference, under the suite's metric: within half of the family's bar
    (families 0, 1 and 4, whose kernels are direct fp32 convolutions; measured worst ratios: profiles/r34_conv_sweep.md).  Every
    family: the reference map has a range — a case whose outputs all read padding only is constant, and the relative metric and the
    finalised affine (1 / sqrt(0 + eps)) mean nothing on it."""
    bar = S.BARS[fam]
    worst, worst_id = 0.0, None
    for case in S.CASES:
        if S.CELLS[case["cell"]]["family"] != fam:
            continue
        o = conv_case.operands(case)
        ref, rstats = conv_case.reference(o)
        assert float(ref.abs().max()) > 1e-3, case["id"]
        if fam in (2, 3, 5):
            continue
        got, gstats = conv_case.reference(o, torch.float32)
        ratio = conv_case.rel_err(got, ref) / bar["map"]
        if rstats is not None:
            ratio = max(ratio, conv_case.rel_err(gstats[..., 0], rstats[..., 0]) / bar["stats"], conv_case.rel_err(gstats[..., 1], rstats[..., 1]) / bar["stats"])
        if ratio > worst:
            worst, worst_id = ratio, case["id"]
    print(f"family {fam}: worst CPU fp32 error / bar {worst:.3f} ({worst_id})")
    assert worst <= 0.5, (worst, worst_id)
