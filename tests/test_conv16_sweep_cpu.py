"""The 16-bit sweep (tests/conv16_sweep.py) checked on a host WITHOUT a GPU.  Every sampled launch, built on fake operand addresses
(tests/launch_contract.py), is ACCEPTED by g6d_conv16_direct_multi_ex / g6d_corr16_multi_ex — it reaches the launch and fails there with
G6D_ELAUNCH — and g6d_conv16_direct_route (the launcher's own decision code) files it in the cell the sampler filed it under, under the
case's knobs; corr16 cases are filed by corr16g::pick_tile through tests/corr16_geom_shim.cpp.  The route's per-segment tiling equals
c16g::halo_tiling / pick_tw through tests/conv16w_geom_shim.cpp, its kernel code equals g6d_conv16_direct_plan's answer, every cell holds
its cases, every excluded cell's probe is refused or routes elsewhere, and every listed value of the free dimensions occurs.

Conditioning: for every case the CPU restatement of the kernel's arithmetic (tests/ref_ops.py conv16_direct_multi / corr16_multi on the
rounded or split operands) is graded against the float64 convolution in the suite's metric and stays within HALF of the arithmetic bar
of its cell — 1e-6 (pairs) / 1e-5 (16-bit) of range, sums likewise — so no case meets or misses a bar because of its own conditioning.
The half ulp a 16-bit OUTPUT adds to a bar is not halved: an exact result rounded once to bf16 is already up to 2^-8 of range away (a
value just above a power of two that is also the map's maximum), which is the whole allowance; no choice of case could halve it.

The calls that launch carry FAKE device pointers: skipped where a GPU is visible, as tests/test_launch_contract_cpu.py."""
import ctypes as C

import pytest
import torch

import conv16_case as CC
import conv16_sweep as S
import launch_contract as LC
from gen6d_amd import lib

ELAUNCH = -3
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="issues calls on fake device pointers: only where no GPU is visible")


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    return CC.build_shims(str(tmp_path_factory.mktemp("c16sweep")))


class _knobs:
    def __init__(self, case):
        self.case = case

    def __enter__(self):
        for k, v in self.case.get("knobs", {}).items():
            lib.set_knob(k, v)

    def __exit__(self, *exc):
        lib.reset_knobs()
        return False


def _segs(case):
    """The segment table of a case on fake addresses, dense rows (pairs: both planes)."""
    pair = case["mode"] == 3
    t = (lib.G6dConv16Seg * len(case["segs"]))()
    for i, (N, D, H, W) in enumerate(case["segs"]):
        code_f, code_p = S.type_code(case, case["full"]), S.type_code(case, case["pool"])
        t[i] = lib.G6dConv16Seg(in_=LC.dev(LC.SEG_PTRS + 3 * i), out_full=LC.dev(LC.SEG_PTRS + 3 * i + 1) if code_f else None,
                                out_pool=LC.dev(LC.SEG_PTRS + 3 * i + 2) if code_p else None, N=N, D=D, H=H, W=W, ld_in=(2 if pair else 1) * case["Cin"],
                                ld_full=(2 if code_f == 3 else 1) * case["Cout"] + (64 if case["wide"] else 0) if code_f else 0,
                                ld_pool=(2 if code_p == 3 else 1) * case["Cout"] if code_p else 0)
    return t


def _plan_args(case, t):
    return (t, len(case["segs"]), case["Cin"], C.c_void_p(LC.dev(20)), case["layout"], case["Cout"], case["kd"], S.type_code(case, case["full"]),
            S.type_code(case, case["pool"]), case["mode"], C.c_void_p(LC.dev(21)) if case["stats"] else None, case["rpg"])


def _route(case):
    """-> (rc, lib.G6dConv16Route, g6d_conv16_direct_plan's answer) under the case's knobs."""
    l = lib.load()
    t = _segs(case)
    r = lib.G6dConv16Route()
    with _knobs(case):
        rc = l.g6d_conv16_direct_route(*_plan_args(case, t), C.byref(r))
        plan = l.g6d_conv16_direct_plan(*_plan_args(case, t))
    return rc, r, plan


def _show(case, rc, r):
    s = r.seg[0]
    return (f"{case.get('id')}: rc {rc} ({lib.load().g6d_last_error().decode()!r}) kernel {r.kernel} layout {r.w_layout} mode {r.math_mode} kd {r.kd} wm {r.wm} "
            f"half {r.half_tile} folded {r.folded} seg0 tw {1 << s.tw_log2} bands {s.bands} segh {1 << s.segh_log2} tpi {s.tpi}; case "
            f"{ {k: v for k, v in case.items() if k not in ('id', 'cell')} }")


CONV = [c for c in S.CASES if c["fam"] != "C"]
CORR = [c for c in S.CASES if c["fam"] == "C"]


def test_counts_and_ids():
    ids = [c["id"] for c in S.CASES]
    assert len(set(ids)) == len(ids)
    thin = {cid: len(cell["cases"]) for cid, cell in S.CELLS.items() if len(cell["cases"]) < 4}
    assert not thin, f"cells with fewer than 4 cases: {thin}"
    assert not set(S.CELLS) & {e["id"] for e in S.EXCLUDED}
    # the cell table the issue describes: 2 x 16 x 3 halo cells less the 16 that pairs cannot reach, 4 x 2 folded, 3 x 5 x 2 per-tap,
    # 2 x (4 + 2) correlation
    per = {f: sum(cell["fam"] == f for cell in S.CELLS.values()) for f in "HFTC"}
    assert per == {"H": 80, "F": 8, "T": 30, "C": 12}, per
    print(f"conv16 sweep: {len(S.CASES)} cases in {len(S.CELLS)} cells ({len(S.EXCLUDED)} excluded); cells per family {per}; "
          f"cases per family { {f: sum(c['fam'] == f for c in S.CASES) for f in 'HFTC'} }")


def test_sizes_stay_small():
    for c in S.CASES:
        assert S.work_of(c) <= S.MAX_WORK, c["id"]
        taps = c["kd"] ** 2 if c["fam"] == "C" else 9 * c["kd"]
        assert taps * c["Cin"] <= S.MAX_K["corr" if c["fam"] == "C" else ("3d" if c["kd"] == 3 else "2d")], c["id"]
        assert 1 <= len(c["segs"]) <= 4, c["id"]


def test_every_case_lands_in_its_cell_and_plan_agrees():
    wrong = []
    for case in CONV:
        rc, r, plan = _route(case)
        if rc != 0 or S.classify(case, r) != case["cell"] or plan != r.kernel:
            wrong.append(_show(case, rc, r) + f" plan {plan} -> {S.classify(case, r) if rc == 0 else None}")
            continue
        want_kernel = 2 if case["stats"] == "passes" else (0 if case["fam"] == "T" else 1)
        if r.kernel != want_kernel or (r.w_layout, r.math_mode, r.kd) != (case["layout"], case["mode"], case["kd"]):
            wrong.append(_show(case, rc, r) + f" kernel {want_kernel} expected")
    assert not wrong, f"{len(wrong)} of {len(CONV)} cases off their cell:\n" + "\n".join(wrong[:12])


def test_route_tiling_is_the_geometry_headers(shims):
    """Per segment the report equals c16g::halo_tiling (folded: of the N D planes, in-image) / pick_tw through the shim; tile0 runs on,
    and the launch's counts are the sums and the grid formula of the two launches."""
    geo = shims["conv"]
    tl = C.create_string_buffer(geo.g_sizeof_tiling())
    out8 = (C.c_int * 8)()
    for case in CONV:
        rc, r, _ = _route(case)
        assert rc == 0, case["id"]
        tile0 = 0
        for i, (N, D, H, W) in enumerate(case["segs"]):
            s = r.seg[i]
            assert s.tile0 == tile0, (case["id"], i)
            if r.kernel:
                folded = case["layout"] == 2
                assert geo.g_halo_tiling(N * D if folded else N, H, W, int(case["mode"] == 3), int(folded), tl, out8) == 1, (case["id"], i)
                assert (s.tw_log2, s.tiles_x, s.tpi, s.segh_log2, s.bands) == tuple(out8[:5]), (case["id"], i, tuple(out8))
                tile0 += out8[7]
            else:
                tw = geo.g_pick_tw(W)
                assert (1 << s.tw_log2, s.tiles_x, s.tpi, s.segh_log2, s.bands) == (tw, -(-W // tw), 0, 0, 0), (case["id"], i)
                tile0 += s.tiles_x * -(-(N * D * H) // (128 // tw))
        for i in range(len(case["segs"]), 4):
            s = r.seg[i]
            assert (s.tile0, s.tw_log2, s.tiles_x, s.tpi, s.segh_log2, s.bands) == (0,) * 6, (case["id"], i)
        assert r.tiles == tile0, case["id"]
        cw = 32 if (r.half_tile or r.math_mode == 3) else 64
        assert r.nN == (case["Cout"] // (cw * (4 // r.wm)) if r.kernel else case["Cout"] // 128), case["id"]
        assert r.blocks == (-(-r.tiles // r.wm) + 7) // 8 * 8 * r.nN, case["id"]
        assert r.half_tile == int(case["Cout"] == 64) and r.folded == int(case["layout"] == 2), case["id"]


def test_corr_cases_are_filed_by_pick_tile(shims):
    geo = shims["corr"]
    for case in CORR:
        k = case["kd"]
        grid = (C.c_int * (40 * 40 * 5))()
        geo.g_pick_grid(k, 40, 40, grid)
        tws = []
        for N, D, H, W in case["segs"]:
            o = ((H - 1) * 40 + (W - 1)) * 5
            assert grid[o] >= 0, case["id"]
            tws.append(1 << grid[o])
        assert S.c_cell("pairs" if case["mode"] == 3 else "b16", k, tws[0]) == case["cell"], (case["id"], tws)
        case_tws = [S.corr_tile_model(H, W, k) for _, _, H, W in case["segs"]]
        assert tws == case_tws, case["id"]


def _issue(case):
    l = lib.load()
    t = _segs(case)
    with _knobs(case):
        if case["fam"] == "C":
            return l.g6d_corr16_multi_ex(t, len(case["segs"]), case["Cin"], C.c_void_p(LC.dev(20)), 1.0, 32, case["kd"], case["mode"], None, None)
        return l.g6d_conv16_direct_multi_ex(t, len(case["segs"]), case["Cin"], C.c_void_p(LC.dev(20)), case["layout"], 1.0, C.c_void_p(LC.dev(22)), case["Cout"],
                                            case["kd"], case["relu"], S.type_code(case, case["full"]), S.type_code(case, case["pool"]), case["mode"],
                                            C.c_void_p(LC.dev(21)) if case["stats"] else None, case["rpg"], None, None)


@no_gpu
def test_every_case_is_accepted_by_the_launcher():
    refused = []
    for case in S.CASES:
        rc = _issue(case)
        if rc != ELAUNCH:
            refused.append(f"{case['id']}: rc {rc} {lib.load().g6d_last_error().decode()!r}")
    assert not refused, f"{len(refused)} refused (a sampler bug, not a skip):\n" + "\n".join(refused[:12])


def test_excluded_cells_are_unreachable(shims):
    """A launch built for an excluded cell is refused or routes to another cell."""
    for ex in S.EXCLUDED:
        assert ex["file"] and ex["condition"]
        case = dict(ex["probe"], id="probe of " + ex["id"])
        if case["fam"] == "C":
            _, _, H, W = case["segs"][0]
            grid = (C.c_int * (40 * 40 * 5))()
            shims["corr"].g_pick_grid(case["kd"], 40, 40, grid)
            tl2 = grid[((H - 1) * 40 + (W - 1)) * 5]
            got = None if tl2 < 0 else S.c_cell("pairs" if case["mode"] == 3 else "b16", case["kd"], 1 << tl2)
            assert got != ex["id"], f"excluded cell {ex['id']} was reached"
            continue
        rc, r, _ = _route(case)
        if rc != 0:
            continue
        got = S.classify(case, r)
        assert got != ex["id"] and not ex["id"].startswith(got + "-"), f"excluded cell {ex['id']} was reached: {_show(case, rc, r)}"
        # a banded shape past the patch limit: no segment of the route has it
        if ex["id"].split("-")[2:3] and ex["id"].split("-")[2].startswith("b") and r.kernel:
            tw, bands, segh = S._band_of(ex["id"].split("-")[2])
            assert (1 << r.seg[0].tw_log2, r.seg[0].bands, 1 << r.seg[0].segh_log2) != (tw, bands, segh), ex["id"]


def _seen(pred, fam):
    return any(pred(c) for c in S.CASES if c["fam"] == fam)


def test_free_dimensions_occur():
    tw_of = lambda c: S.halo_model(c["segs"][0][0], c["segs"][0][2], c["segs"][0][3])
    need = {
        "bf16": (lambda c: c["mode"] == 1, "HTC"), "fp16": (lambda c: c["mode"] == 2, "HTC"), "pairs": (lambda c: c["mode"] == 3, "HFTC"),
        "1 segment": (lambda c: len(c["segs"]) == 1, "HFTC"), "2 segments": (lambda c: len(c["segs"]) == 2, "HFTC"),
        "3 segments": (lambda c: len(c["segs"]) == 3, "HTC"), "4 segments": (lambda c: len(c["segs"]) == 4, "HT"),
        "Cin=32": (lambda c: c["Cin"] == 32, "HFTC"), "Cin=96": (lambda c: c["Cin"] == 96, "HFTC"), "Cin=64": (lambda c: c["Cin"] == 64, "HFTC"),
        "Cin=128": (lambda c: c["Cin"] == 128, "HT"),
        "Cout=64": (lambda c: c["Cout"] == 64, "HF"), "Cout=128": (lambda c: c["Cout"] == 128, "HFT"), "Cout=256": (lambda c: c["Cout"] == 256, "HFT"),
        "Cout=384": (lambda c: c["Cout"] == 384, "HFT"),
        "relu": (lambda c: c["relu"], "HFT"), "no relu": (lambda c: not c["relu"], "HFT"),
        "full 16-bit": (lambda c: c["full"] == "t16", "HFT"), "full fp32": (lambda c: c["full"] == "f32", "HFT"), "no full map": (lambda c: c["full"] is None, "HFT"),
        "pool 16-bit": (lambda c: c["pool"] == "t16", "HT"), "pool fp32": (lambda c: c["pool"] == "f32", "HT"), "no pool": (lambda c: c["pool"] is None, "HFT"),
        "statistics only": (lambda c: c["full"] is None and c["pool"] is None, "HFT"),
        "fp32 slice of wider rows": (lambda c: c["wide"], "HFT"),
        "no statistics": (lambda c: c["stats"] is None, "HFT"), "one group": (lambda c: c["stats"] == "one", "HFT"),
        "groups of images": (lambda c: c["stats"] == "images", "H"), "groups of tiles": (lambda c: c["stats"] == "tiles", "H"),
        "groups of passes": (lambda c: c["stats"] == "passes", "H"), "groups of tile rows": (lambda c: c["stats"] == "rows", "T"),
        "groups of volumes": (lambda c: c["stats"] == "volumes", "F"),
        "statistics with relu": (lambda c: c["stats"] and c["relu"], "HFT"),
        "W a multiple of the tile": (lambda c: c["segs"][0][3] % tw_of(c)[0] == 0, "H"), "W one over": (lambda c: c["segs"][0][3] % tw_of(c)[0] == 1, "H"),
        "W one short": (lambda c: c["segs"][0][3] % tw_of(c)[0] == tw_of(c)[0] - 1, "H"),
        "H one over the tile height": (lambda c: tw_of(c)[1] == 1 and c["segs"][0][2] % (128 // tw_of(c)[0]) == 1, "H"),
        "H one short": (lambda c: tw_of(c)[1] == 1 and c["segs"][0][2] % (128 // tw_of(c)[0]) == 128 // tw_of(c)[0] - 1, "H"),
        "H a multiple": (lambda c: tw_of(c)[1] == 1 and c["segs"][0][2] % (128 // tw_of(c)[0]) == 0, "H"),
        "last banded tile part-filled": (lambda c: tw_of(c)[1] > 1 and c["segs"][0][0] % tw_of(c)[1], "H"),
        "odd tile count under two tiles per block": (lambda c: c["Cout"] != 256 and (c["mode"] != 3 or c["Cout"] == 64) and
                                                     sum(S.halo_model(n, h, w)[5] for n, _, h, w in c["segs"]) % 2 == 1, "H"),
        "a seam inside a two-tile block": (lambda c: c["Cout"] == 64 and len(c["segs"]) > 1 and tw_of(c)[5] % 2 == 1, "H"),
        "D=1": (lambda c: c["segs"][0][1] == 1, "F"), "D=2": (lambda c: c["segs"][0][1] == 2, "F"), "D=3": (lambda c: c["segs"][0][1] == 3, "F"),
        "D=5": (lambda c: c["segs"][0][1] == 5, "F"),
        "knob conv16_halo = 0": (lambda c: c["knobs"].get("conv16_halo") == 0, "T"),
        "default knob, H = 1": (lambda c: not c["knobs"] and c["layout"] == 1 and c["kd"] == 1 and c["segs"][0][2] == 1, "T"),
        "default knob, H = 3": (lambda c: not c["knobs"] and c["layout"] == 1 and c["kd"] == 1 and c["segs"][0][2] == 3, "T"),
        "one slice": (lambda c: c["mode"] != 3 and c["Cin"] == 32, "C"), "three or more slices": (lambda c: c["Cin"] // (16 if c["mode"] == 3 else 32) >= 3, "C"),
        "a map lower or narrower than the filter radius": (lambda c: min(c["segs"][0][2:]) < c["kd"] // 2, "C"), "N > 1": (lambda c: c["segs"][0][0] > 1, "HFTC"),
        "segments of different widths": (lambda c: len({S.corr_tile_model(h, w, c["kd"]) for _, _, h, w in c["segs"]}) > 1, "C"),
    }
    missing = {name: [f for f in fams if not _seen(pred, f)] for name, (pred, fams) in need.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, f"free-dimension values that never occur (value: families): {missing}"
    for cid, cell in S.CELLS.items():                         # inside a 16-bit cell bf16 and fp16 both occur
        if cell.get("arith") == "b16" or cell.get("loader") in ("lds16", "frag16"):
            assert {c["mode"] for c in cell["cases"]} == {1, 2}, cid
        if cell["fam"] == "H" and cell["shape"][0] == "b":     # every banded cell: statistics groups of whole tiles and of whole passes
            assert {"tiles", "passes"} <= {c["stats"] for c in cell["cases"]}, cid
    for c in S.CASES:                                          # the documented domain
        assert c["pool"] is None or all(h % 2 == 0 and w % 2 == 0 for _, _, h, w in c["segs"]), c["id"]
        assert c["full"] or c["pool"] or c["stats"], c["id"]
        assert not c["rpg"] or len(c["segs"]) == 1, c["id"]


RATIO = {}


@pytest.mark.parametrize("fam", ["H", "F", "T", "C"])
def test_conditioning(fam):
    """The CPU restatement against the float64 convolution: within half of the arithmetic bar (the module docstring), and every
    reference map has a range."""
    worst, worst_id, bad = 0.0, None, []
    for case in S.CASES:
        if case["fam"] != fam:
            continue
        o = CC.operands(case)
        ref = CC.reference(o)
        assert min(ref.rngs) > 1e-3, case["id"]
        fulls, pools, stats = CC.restatement(o)
        _, fails = CC.grade(case, ref, fulls, pools, stats, arith=0.5)
        bad += fails
        ratio, _ = CC.grade(case, ref, fulls, pools, stats)
        if ratio > worst:
            worst, worst_id = ratio, case["id"]
    print(f"family {fam}: worst CPU restatement error / bar {worst:.3f} ({worst_id})")
    assert not bad, f"{len(bad)} checks past half of the arithmetic bar:\n" + "\n".join(bad[:12])
