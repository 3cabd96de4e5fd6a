"""The Winograd sweep (tests/wino_sweep.py) checked on a host WITHOUT a GPU.  Every sampled launch, built on fake operand addresses
(tests/launch_contract.py), is ACCEPTED by its entry point — it reaches the launch and fails there with G6D_ELAUNCH — and
g6d_wino_multi_route (the launchers' own validation, segment table, plan and kernel choice) files it in the cell the sampler filed it under,
under the case's knobs.  The route's numbers equal wplan::f2_plan / f4_plan through tests/wino_plan_shim.cpp, every cell holds its cases,
every excluded cell's probe is refused or routes elsewhere, and every listed value of the free dimensions occurs.

Conditioning, in the suite's metric (max |error| / max |reference| per segment and output kind): every float64 reference map has a range;
for the fp32 families torch's own fp32 convolution (the correlations: the fp32 direct correlation) stays within HALF of the cell's bar
against float64, for the 16-bit cells the ref_ops restatement of the kernel's arithmetic within half of TOL[mode] — so no case meets or
misses a bar because of its own conditioning.  A case that fails this is replaced by the next draw (wino_sweep.REPLACED), never dropped.

The calls that launch carry FAKE device pointers: skipped where a GPU is visible, as tests/test_launch_contract_cpu.py."""
import ctypes as C

import pytest
import torch

import launch_contract as LC
import wino_case as WC
import wino_sweep as S
from gen6d_amd import lib
from test_wino_plan_cpu import real_f2, real_f4, wp  # noqa: F401  (wp: the fixture that builds tests/wino_plan_shim.cpp)

ELAUNCH = -3
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="issues calls on fake device pointers: only where no GPU is visible")
IN, FULL, POOL, U, BIAS, WS = (LC.dev(k) for k in (100, 300, 500, 20, 22, 700))


def _routes(case):
    with WC.knobs(case):
        return WC.routes(case, WC.table(case, IN, FULL, POOL), U, WS)


def _show(case, rc, r):
    return (f"{case.get('id')}: rc {rc} ({lib.load().g6d_last_error().decode()!r}) family {r.family} kd {r.kd} wide {r.wide} nq {r.nq} nwn {r.nwn} blocks {r.blocks} "
            f"grid2 {r.grid2} nchunks {r.nchunks} splits {r.splits} x {r.chunks_per_split} map {r.map_mode} lds {r.lds_bytes}; case "
            f"{ {k: v for k, v in case.items() if k not in ('id', 'cell')} }")


def test_counts_and_ids():
    ids = [c["id"] for c in S.CASES]
    assert len(set(ids)) == len(ids)
    thin = {cid: len(cell["cases"]) for cid, cell in S.CELLS.items() if len(cell["cases"]) < 4}
    assert not thin, f"cells with fewer than 4 cases: {thin}"
    assert not set(S.CELLS) & {e["id"] for e in S.EXCLUDED}
    # 2 block forms x 5 split classes; 2 widths x 5; 2 arithmetics x (two waves: none, clamped, no-ws + one wave: 5); 4 decodes x 5; 2 kd x 2 nt x 5
    per = {f: sum(cell["fam"] == f for cell in S.CELLS.values()) for f in S.ENTRY}
    assert per == {"F2": 10, "F2C": 10, "W16": 16, "F4": 20, "F4C": 20}, per
    print(f"wino sweep: {len(S.CASES)} cases in {len(S.CELLS)} cells ({len(S.EXCLUDED)} excluded); cells per family {per}; replaced draws {S.REPLACED}")


def test_sizes_stay_small():
    for c in S.CASES:
        assert S.work_of(c) <= S.MAX_WORK and c["Cin"] <= 512, c["id"]
        assert 1 <= len(c["segs"]) <= 4, c["id"]
        assert c["ws"] is None or S.COUNTER_BYTES < c["ws"] <= S.AMPLE, c["id"]


def test_every_case_lands_in_its_cell():
    wrong = []
    for case in S.CASES:
        rc, r, ra = _routes(case)
        got = S.classify_case(case, r, ra) if rc == 0 else None
        fam = {"F2": (0,), "F2C": (0,), "W16": (1, 2), "F4": (3,), "F4C": (3,)}[case["fam"]]
        if got != case["cell"] or r.family not in fam or r.kd != S.kd_of(case) or r.entry != lib.WINO_ROUTE_ENTRIES[case["entry"]]:
            wrong.append(_show(case, rc, r) + f" -> {got}")
        elif case["fam"] == "W16" and r.family != (2 if "-2w-" in case["cell"] else 1):
            wrong.append(_show(case, rc, r) + " -> the other 16-bit kernel")
    assert not wrong, f"{len(wrong)} of {len(S.CASES)} cases off their cell:\n" + "\n".join(wrong[:12])


def _knob(case, name, default):
    return case["knobs"].get(name, default)


def test_route_numbers_are_wino_plan_h(wp):  # noqa: F811
    """The report equals wplan::f2_plan / f4_plan on the same segments, knobs and workspace bytes, through the shim; the LDS bytes are the
    header's for the instantiation the report names; segments past nseg are zero."""
    for case in S.CASES:
        rc, r, _ = _routes(case)
        assert rc == 0, case["id"]
        in_offs = S.layout(case)[0]
        segs = [(N, H, W, off - min(in_offs), S.ld_in_of(case)) for (N, H, W), off in zip(case["segs"], in_offs)]
        if case["fam"] in S.F4_FAMS:
            p = real_f4(wp, segs, 0, S.kd_of(case), case["Cin"], case["Cout"], case["ws"], int(_knob(case, "w43_split_max", 32)), _knob(case, "w43_split_gain", 0.85),
                        _knob(case, "w43_chunk_us", 2.8))
            assert (r.nq, r.nwn, r.wide) == (8, p["nt"], 0), case["id"]
            lds = max(wp.wp_lds(3, 0, p["nt"], 0, case["Cin"]), 4 * 4096 * 4)
        else:
            p = real_f2(wp, segs, 0, 1, case["mode"], 0, S.kd_of(case), case["Cin"], case["Cout"], case["ws"], int(_knob(case, "wino_wide", 1)),
                        int(_knob(case, "wino_split_max", 32)), _knob(case, "wino_split_gain", 0.85), _knob(case, "wino_split_fix", 2.0), _knob(case, "wino_split_per", 0.6))
            assert (r.nq, r.nwn, r.wide) == (p["nq"], p["nwn"], p["wide"]), case["id"]
            lds = {0: wp.wp_lds(0, 0, p["nwn"], 1 if p["wide"] else 2, case["Cin"]), 1: wp.wp_lds(1, 0, 0, 0, case["Cin"]), 2: wp.wp_lds(2, 0, 0, 0, 0)}[r.family]
            assert r.map_mode == 0, case["id"]
        assert not isinstance(p, str), (case["id"], p)
        assert (r.blocks, r.grid2, r.nchunks, r.splits, r.chunks_per_split) == (p["blocks"], p["grid2"], p["nchunks"], p["splits"], p["cps"]), (case["id"], p)
        assert r.lds_bytes == lds <= 160 * 1024, case["id"]
        for k in range(4):
            want = tuple(p["geo"][k][:3]) if k < len(segs) else (0, 0, 0)
            assert (r.seg[k].qstart, r.seg[k].QH, r.seg[k].QW) == want, (case["id"], k)
        assert r.splits * r.chunks_per_split >= r.nchunks > (r.splits - 1) * r.chunks_per_split, case["id"]


@no_gpu
def test_every_case_is_accepted_by_the_launcher():
    refused = []
    for case in S.CASES:
        with WC.knobs(case):
            rc = WC.launch(case, WC.table(case, IN, FULL, POOL), U, BIAS, WS, None)
        if rc != ELAUNCH:
            refused.append(f"{case['id']}: rc {rc} {lib.load().g6d_last_error().decode()!r}")
    assert not refused, f"{len(refused)} refused (a sampler bug, not a skip):\n" + "\n".join(refused[:12])


def test_excluded_cells_are_unreachable():
    """A launch built for an excluded cell is refused — by the route report AND (where no GPU is visible) by the launch — or routes to
    another cell."""
    for ex in S.EXCLUDED:
        assert ex["file"] and ex["condition"]
        case = dict(ex["probe"], id="probe of " + ex["id"])
        rc, r, ra = _routes(case)
        if rc != 0:
            assert rc == -1 and lib.load().g6d_last_error(), ex["id"]
            if not torch.cuda.is_available():
                with WC.knobs(case):
                    assert WC.launch(case, WC.table(case, IN, FULL, POOL), U, BIAS, WS, None) == -1, ex["id"]
            continue
        got = S.classify_case(case, r, ra)
        assert got != ex["id"] and not ex["id"].startswith(got + "-"), f"excluded cell {ex['id']} was reached: {_show(case, rc, r)}"
        if ex["id"].endswith("3chunks"):
            assert r.nchunks == 3 and r.splits == 1, _show(case, rc, r)
        if ex["id"].endswith("-wide"):
            assert r.wide == 0 and r.nq == 4, _show(case, rc, r)
        if "-2w-" in ex["id"]:
            assert r.family == 1 and r.splits > 1, _show(case, rc, r)


def test_unsplit_route_past_the_counter_limit():
    """A launch with more blocks x channel slices than the workspace has tile counters (G6D_WS_COUNTERS = 4096) is never split, whatever
    the knobs say.  That needs about a million output pixels: shown from the report alone, on fake addresses, and not run on the GPU."""
    for fam, cout, px in (("F2", 128, 1024), ("F4", 128, 1536), ("W16", 128, 1024)):
        case = S._probe(fam, segs=[(1, px, 1024)], Cin=64, Cout=cout, knobs={"wino_wide": 0, "wino_split_max": 8, "wino_split_gain": 1.0, "wino_split_fix": 0.0,
                                                                             "wino_split_per": 0.0, "w43_split_max": 8, "w43_split_gain": 1.0})
        rc, r, _ = _routes(case)
        assert rc == 0 and r.grid2 > 4096 and r.splits == 1 and r.chunks_per_split == r.nchunks, _show(case, rc, r)
        small = dict(case, segs=[(1, 16, 16)])
        rc, r, _ = _routes(small)
        assert rc == 0 and r.grid2 <= 4096 and r.splits > 1, _show(small, rc, r)


def _q(case):
    return [S.quarters(s) for s in case["segs"]]


def _starts(case):
    q, out = 0, []
    for s in case["segs"]:
        out.append(q)
        q += S.quarters(s)
    return out, q


def _gx(case):
    return -(-_starts(case)[1] // S.nq_of(case))


def test_free_dimensions_occur():
    ALL, TRUNK, CORR = ("F2", "F2C", "W16", "F4", "F4C"), ("F2", "W16", "F4"), ("F2C", "F4C")
    need = {
        "full only": (lambda c: c["full"] and not c["pool"], ALL), "pool only": (lambda c: c["pool"] and not c["full"], TRUNK), "both outputs": (lambda c: c["full"] and c["pool"], TRUNK),
        "relu": (lambda c: c["relu"], TRUNK), "no relu": (lambda c: not c["relu"], TRUNK), "NULL bias": (lambda c: not c["bias"], TRUNK), "a bias": (lambda c: c["bias"], TRUNK),
        "1 segment": (lambda c: len(c["segs"]) == 1, ALL), "2 segments": (lambda c: len(c["segs"]) == 2, ALL), "3 segments": (lambda c: len(c["segs"]) == 3, ALL),
        "4 segments": (lambda c: len(c["segs"]) == 4, ALL), "N > 1 in a segment": (lambda c: any(s[0] > 1 for s in c["segs"]), ALL),
        "a block that straddles a segment boundary": (lambda c: any(q % S.nq_of(c) for q in _starts(c)[0][1:]), ALL),
        "a last block that is not full": (lambda c: _starts(c)[1] % S.nq_of(c) != 0, ALL),
        "an odd quarter count under the wide form": (lambda c: S.nq_of(c) == 2 and _starts(c)[1] % 2 == 1, ("F2",)),
        "maps of at most 8x8, several images per block": (lambda c: any(s[0] > 1 and s[1] <= 8 and s[2] <= 8 for s in c["segs"]), ALL),
        "H or W not a multiple of 8": (lambda c: any(s[1] % 8 or s[2] % 8 for s in c["segs"]), ALL),
        "H or W odd with a pooled output": (lambda c: c["pool"] and any(s[1] % 2 or s[2] % 2 for s in c["segs"]), TRUNK),
        "H = 1 or W = 1 with the full output only": (lambda c: not c["pool"] and any(1 in s[1:] for s in c["segs"]), ALL),
        "H = 2 or W = 2 with the pool": (lambda c: c["pool"] and any(2 in s[1:] for s in c["segs"]), TRUNK),
        "an input slice that starts past channel 0": (lambda c: c["c_off"] > 0, ALL), "slack after the input slice": (lambda c: c["in_tail"] > 0, ALL),
        "ld_full > Cout": (lambda c: c["full"] and c["ldf"] > 0, ALL), "ld_pool > Cout": (lambda c: c["pool"] and c["ldp"] > 0, TRUNK),
        "segment 0 not at the lowest address": (lambda c: c["rev"] and len(c["segs"]) > 1, ALL),
        "the one-map entry g6d_wino_conv3x3": (lambda c: c["single"], ("F2",)),
        "w43_map 1 with a short last group": (lambda c: c["knobs"].get("w43_map") == 1 and c["Cout"] > 64 and _gx(c) % 8 != 0, S.F4_FAMS),
        "w43_map 1 with a full group before the short one": (lambda c: c["knobs"].get("w43_map") == 1 and c["Cout"] > 64 and _gx(c) > 8 and _gx(c) % 8 != 0, S.F4_FAMS),
        "w43_map 2": (lambda c: c["knobs"].get("w43_map", 2) == 2, S.F4_FAMS), "w43_map 0": (lambda c: c["knobs"].get("w43_map") == 0, S.F4_FAMS),
        "7x7 filters zero-extended to 9x9": (lambda c: c["k7"], ("F4C",)), "9x9 filters": (lambda c: c["kb"] == 3 and not c["k7"], ("F4C",)),
        "the one-wave kernel by its split, knob wino16_2w at its default": (lambda c: "-1w-" in c["cell"] and "wino16_2w" not in c["knobs"], ("W16",)),
        "the two-waves kernel on the shape of a split one-wave case": (lambda c: "twin" in c, ("W16",)),
    }
    missing = {name: [f for f in fams if not any(pred(c) for c in S.CASES if c["fam"] == f)] for name, (pred, fams) in need.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, f"free-dimension values that never occur (value: families): {missing}"
    # kd 25 and 9: the even and tail cells between them hold split boundaries inside the sub-filter blocks of one channel chunk
    for form in sorted({cell["form"] for cell in S.CELLS.values() if cell["fam"] in CORR}):
        fam = "F2C" if form.startswith("nwn") else "F4C"
        inside = [c["id"] for sp in ("even", "tail") for c in S.CELLS[S.cell_id(fam, form, sp)]["cases"] if S.model(c)["cps"] % S.kd_of(c)]
        assert len(inside) >= 2, (form, inside)
    for c in S.CASES:                                          # the documented domain
        assert c["full"] or c["pool"], c["id"]
        assert not c["pool"] or all(h >= 2 and w >= 2 for _, h, w in c["segs"]), c["id"]
        assert c["c_off"] % 4 == 0 and S.ld_in_of(c) % 4 == 0, c["id"]
        if c.get("twin"):
            t = next(x for x in S.CASES if x["id"] == c["twin"])
            assert (t["segs"], t["Cin"], t["Cout"], t["mode"]) == (c["segs"], c["Cin"], c["Cout"], c["mode"]) and S.model(t)["splits"] > 1


@pytest.mark.parametrize("fam", list(S.ENTRY))
def test_conditioning(fam):
    worst, worst_id, bad = 0.0, None, []
    for case in S.CASES:
        if case["fam"] != fam:
            continue
        o = WC.operands(case)
        ref = WC.reference(case, o)
        if not min(WC.ranges(ref)) > 1e-3:
            bad.append(f"{case['id']}: a reference map without a range {WC.ranges(ref)}")
            continue
        if fam == "W16":
            ratio, fails = WC.grade(case, ref, WC.restatement16(case, o), 0.5 * S.TOL16[case["mode"]])
        else:
            ratio, fails = WC.grade(case, ref, WC.fp32_comparator(case, o), 0.5 * S.BARS[fam]["bar"])
        bad += fails
        if ratio > worst:
            worst, worst_id = ratio, case["id"]
    print(f"family {fam}: worst CPU comparator error / (bar / 2) {worst:.3f} ({worst_id})")
    assert not bad, f"{len(bad)} checks past half of the bar (replace the draw: wino_sweep.REPLACED):\n" + "\n".join(bad[:12])
