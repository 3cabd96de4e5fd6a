"""A deterministic sampler of launches of the Winograd multi-map entry points — g6d_wino_conv3x3 / g6d_wino_conv3x3_multi,
g6d_wino16_conv3x3_multi, g6d_wino43_conv3x3_multi, g6d_corr2d_wino_multi, g6d_corr2d_wino43_multi — filed by what the HOST code chooses
for them (g6d_wino_multi_route: block form, split of the chunk list, kernel instantiation, F(4x4,3x3) block-id decode).

Pure Python, fixed seeds, no GPU and no library call: CASES, CELLS and EXCLUDED are built at import, so the pytest ids are stable.  The
plan is restated here (tests/test_wino_plan_cpu.py parent_f2 / parent_f4, the Python statement that module already checks against
wino_plan.h) only to FIND shapes; tests/test_wino_sweep_cpu.py proves on the host that every case lands in its cell by the launchers' own
code, and tests/test_wino_sweep_gpu.py runs every cell.

Families and their cells (a cell = one outcome of the host's choice):
  F2    g6d_wino_conv3x3_multi (one segment, `single`: g6d_wino_conv3x3)   block form {wide 2 x 128, square 4 x 64} x split class
  F2C   g6d_corr2d_wino_multi, kd 25                                         nwn {1 (Cout % 64 != 0), 2} x split class
  W16   g6d_wino16_conv3x3_multi                                             {bf16, fp16} x {2w (un-split only), 1w} x split class
  F4    g6d_wino43_conv3x3_multi                                             effective map_mode {0k by knob, 0g by gy == 1, 1, 2} x split class
  F4C   g6d_corr2d_wino43_multi                                              kd {25, 9} x nt {2, 4} x split class
Split classes: none (the model chose 1 with room), even (splits >= 2, chunks_per_split * splits == nchunks), tail (the last split is
shorter), clamped (the workspace bytes handed over end the search below what ample room gives), no-ws (NULL workspace, one split).

A CASE: dict(fam, cell, id, entry, single, mode (0 fp32, 1 bf16, 2 fp16), kb (kblocks, 0 for the trunk), k7 (kd 9: the 7x7 filters
zero-extended), segs [(N, H, W)], Cin, Cout, relu, bias, full, pool, c_off / in_tail (channels of slack before / after the Cin-channel slice
of an input row), ldf / ldp (channels of slack after Cout in a full / pooled row), rev (segments laid out in reverse: segment 0 at the
HIGHEST address), ws (None = NULL workspace, else the bytes handed to the launch), knobs, seed).

Sizes: the smallest that reach the cell; every case at most 2^27 multiply-adds; Cin <= 512."""
import random

import test_wino_plan_cpu as P

MAX_WORK = 1 << 27
PER_CELL = 4
COUNTER_BYTES = P.COUNTER_BYTES
AMPLE = COUNTER_BYTES + (64 << 20)          # "room available": more than any case's splits x partial images
SPLITS = ("none", "even", "tail", "clamped", "no-ws")
TOL16 = {1: 2e-2, 2: 3e-3}                  # tests/test_lowp_gpu.py TOL (bf16, fp16)
# The bars (max |error| / max |reference| per segment and output kind), with the test each is borrowed from
BARS = {
    "F2": dict(bar=3e-5, src="tests/test_kernels_gpu.py::test_wino_conv3x3_multi (3e-5)"),
    "F2C": dict(bar=4e-5, src="tests/test_kernels_gpu.py::test_corr2d_wino_multi (4e-5)"),
    "F4": dict(bar=1e-5, src="tests/test_wino43_gpu.py::test_wino43_conv3x3_multi (1e-5)"),
    "F4C": dict(bar=2e-5, src="tests/test_wino43_gpu.py::test_corr2d_wino43_multi, ..._7x7_on_9x9_blocks (2e-5)"),
    "W16": dict(bar=TOL16, restated=3e-4, src="tests/test_lowp_gpu.py::test_wino16_conv3x3_multi (TOL[mode] against float64: 2e-2 bf16 / 3e-3 fp16; 3e-4 against "
                                            "the ref_ops restatement of the kernel's arithmetic)"),
}
ENTRY = {"F2": "g6d_wino_conv3x3_multi", "F2C": "g6d_corr2d_wino_multi", "W16": "g6d_wino16_conv3x3_multi", "F4": "g6d_wino43_conv3x3_multi",
         "F4C": "g6d_corr2d_wino43_multi"}
F4_FAMS = ("F4", "F4C")
CORR_FAMS = ("F2C", "F4C")

CELLS = {}          # id -> dict(fam, ..., split, cases=[...])
EXCLUDED = []       # dict(id, file, condition, probe = a case built for the cell: refused or routed elsewhere)
CASES = []


# ------------------------------------------------------------------------------------------------------------------ the plan, restated
def kd_of(case):
    return case["kb"] ** 2 if case["kb"] else 1


def taps_of(case):
    return (7 * 7 if case.get("k7") else 9 * case["kb"] ** 2) if case["kb"] else 9


def pixels(case):
    return sum(N * H * W for N, H, W in case["segs"])


def work_of(case):
    return pixels(case) * taps_of(case) * case["Cin"] * case["Cout"]


def ld_in_of(case):
    return case["c_off"] + case["Cin"] + case["in_tail"]


def layout(case):
    """Where the segments lie in the three buffers (floats from each buffer's start) -> (in_offs, full_offs, pool_offs, totals).  Every
    start is 16-byte aligned; `rev` lays the segments out in reverse, so that segment 0 has the highest address of each kind; an input
    row's slice starts c_off channels into the row."""
    n = len(case["segs"])
    order = list(range(n))[::-1] if case["rev"] else list(range(n))
    offs = [[0] * n for _ in range(3)]
    tot = [0, 0, 0]
    lds = (ld_in_of(case), case["Cout"] + case["ldf"], case["Cout"] + case["ldp"])
    for k in order:
        N, H, W = case["segs"][k]
        px = (N * H * W, N * H * W, N * (H // 2) * (W // 2))
        for kind in range(3):
            offs[kind][k] = tot[kind]
            tot[kind] += (px[kind] * lds[kind] + 3) // 4 * 4
    return offs[0], offs[1], offs[2], tot


def model(case, ws="case"):
    """parent_f2 / parent_f4 of the case under its knobs -> the plan dict (None: refused).  ws: bytes, None, or the case's own."""
    ws = case["ws"] if ws == "case" else ws
    kn = case["knobs"]
    in_offs = layout(case)[0]
    base = min(in_offs)
    segs = [(N, H, W, off - base + 0, ld_in_of(case)) for (N, H, W), off in zip(case["segs"], in_offs)]
    if case["fam"] in F4_FAMS:
        p = P.parent_f4(segs, 0, kd_of(case), case["Cin"], case["Cout"], ws, int(kn.get("w43_split_max", P.F4_KNOBS["split_max"])),
                        kn.get("w43_split_gain", P.F4_KNOBS["gain"]), kn.get("w43_chunk_us", P.F4_KNOBS["chunk_us"]))
    else:
        p = P.parent_f2(segs, 0, 1, case["mode"], 0, kd_of(case), case["Cin"], case["Cout"], ws, int(kn.get("wino_wide", P.F2_KNOBS["wide"])),
                        int(kn.get("wino_split_max", P.F2_KNOBS["split_max"])), kn.get("wino_split_gain", P.F2_KNOBS["gain"]),
                        kn.get("wino_split_fix", P.F2_KNOBS["fix"]), kn.get("wino_split_per", P.F2_KNOBS["per"]))
    return None if isinstance(p, str) else p


def split_class(splits, cps, nchunks, splits_ample, no_ws):
    if no_ws:
        return "no-ws"
    if splits < splits_ample:
        return "clamped"
    if splits == 1:
        return "none"
    return "even" if cps * splits == nchunks else "tail"


def model_class(case):
    p, pa = model(case), model(case, AMPLE)
    return split_class(p["splits"], p["cps"], p["nchunks"], pa["splits"], case["ws"] is None)


def nq_of(case):
    if case["fam"] in F4_FAMS:
        return 8
    return 2 if case["fam"] == "F2" and case["knobs"].get("wino_wide") == 2 and case["Cout"] % 128 == 0 else 4


def quarters(seg):
    N, H, W = seg
    return N * ((H + 7) // 8) * ((W + 7) // 8)


# ------------------------------------------------------------------------------------------------------------------ free dimensions
class Deal:
    """Round-robin dealer of the listed values of one free dimension, so that every value occurs whatever the random draws do."""

    def __init__(self, values, seed):
        self.values, self.i = list(values), 0
        random.Random(seed).shuffle(self.values)

    def next(self, ok=lambda v: True):
        for _ in range(len(self.values)):
            v = self.values[self.i % len(self.values)]
            self.i += 1
            if ok(v):
                return v
        raise ValueError("no admissible value")


KINDS = ("small", "ragged", "oddpool", "thin", "two", "plain", "small", "ragged")


def _dealers(seed):
    return dict(out=Deal(("full", "pool", "both"), seed + 1), relu=Deal((1, 0), seed + 2), bias=Deal((1, 1, 0), seed + 3), nseg=Deal((1, 2, 3, 4, 2), seed + 4),
                kind=Deal(KINDS, seed + 5), slack=Deal(((0, 0), (4, 4), (8, 0), (16, 8), (0, 0)), seed + 6), ldf=Deal((0, 32, 0, 4), seed + 7),
                ldp=Deal((0, 0, 16, 8), seed + 8), rev=Deal((0, 1, 1), seed + 9), map=Deal((2, 1, 0), seed + 10), single=Deal((1, 0), seed + 11),
                k7=Deal((1, 0), seed + 12))


def _first(r, kind):
    """The first segment of a case: (N, H, W) of the dealt kind."""
    if kind == "small":                   # maps of at most 8x8: one quarter per image, several images per block
        return (r.choice((2, 3, 5, 6, 7)), r.choice((3, 4, 5, 7, 8)), r.choice((3, 5, 6, 8)))
    if kind == "ragged":                  # H or W not a multiple of 8
        return (r.choice((1, 2, 3)), r.choice((9, 11, 12, 14, 17)), r.choice((10, 13, 15, 18, 20)))
    if kind == "oddpool":                 # odd H or W under a pooled output
        return (r.choice((1, 2)), r.choice((5, 9, 11, 15)), r.choice((7, 9, 12, 13)))
    if kind == "thin":                    # one row or one column: the full output only
        return (r.choice((1, 2, 3)),) + r.choice(((1, 13), (11, 1), (1, 8), (1, 1), (17, 1)))
    if kind == "two":                     # two rows or two columns under the pool
        return (r.choice((1, 2, 3)),) + r.choice(((2, 12), (10, 2), (2, 2), (2, 9), (16, 2)))
    return (r.choice((1, 2)), r.choice((8, 16)), r.choice((8, 16, 24)))


def _geometry(r, kind, nseg, out, crowd):
    """segs of a case: the first of the dealt kind, the others small and ragged; a pooled output needs H, W >= 2 everywhere.  crowd: many
    one-quarter images, so that more than eight blocks of eight quarters form."""
    segs = [_first(r, kind)]
    if crowd:
        segs = [(r.choice((67, 70, 75)), r.choice((2, 3)), r.choice((2, 3)))]
    lo = 2 if out != "full" else 1
    while len(segs) < nseg:
        segs.append((r.choice((1, 2, 3)), r.choice((lo, 3, 5, 6, 8, 9, 10)), r.choice((lo, 4, 7, 8, 11))))
    return segs


def _knob_variants(fam, r):
    if fam in F4_FAMS:
        v = [{}] + [{"w43_split_max": s, "w43_split_gain": 1.0} for s in range(2, 9)] + [{"w43_split_gain": 0.05}, {"w43_split_max": 1}, {"w43_chunk_us": 0.01},
                                                                                          {"w43_chunk_us": 40.0}]
    else:
        v = [{}] + [{"wino_split_max": s, "wino_split_gain": 1.0, "wino_split_fix": 0.0, "wino_split_per": 0.0} for s in range(2, 9)] + \
            [{"wino_split_gain": 0.05}, {"wino_split_max": 1}, {"wino_split_fix": 500.0}, {"wino_split_per": 200.0}]
    r.shuffle(v)
    return v


CINS = {"F2": (32, 40, 48, 56, 64, 72, 96, 128), "F4": (32, 40, 48, 56, 64, 72, 96, 128), "W16": (64, 80, 96, 112, 128, 160), "F2C": (8, 16, 24, 32, 40),
        "F4C": (8, 16, 24, 32, 40, 64)}


def _draw(cell, r, deal, idx):
    """One case of the cell: deal the free dimensions, then search channels x knobs x workspace for the cell's split class."""
    fam, want = cell["fam"], cell["split"]
    corr = fam in CORR_FAMS
    for _ in range(400):
        kind = deal["kind"].next()
        out = "full" if corr else deal["out"].next()
        if kind == "thin":
            out = "full"
        elif kind in ("two", "oddpool") and not corr:
            out = deal["out"].next(lambda o: o != "full")
        nseg = deal["nseg"].next()
        crowd = fam in F4_FAMS and idx == 0 and (cell.get("map") == "1" or corr)
        segs = _geometry(r, kind, nseg, out, crowd)
        c_off, in_tail = deal["slack"].next()
        base = dict(fam=fam, entry=ENTRY[fam], single=False, mode=cell.get("mode", 0), kb=cell.get("kb", 0), k7=False, segs=segs, relu=0 if corr else deal["relu"].next(),
                    bias=0 if corr else deal["bias"].next(), full=out != "pool", pool=out != "full", c_off=c_off, in_tail=in_tail, ldf=deal["ldf"].next(),
                    ldp=0 if corr else deal["ldp"].next(), rev=bool(deal["rev"].next()) and nseg > 1, ws=AMPLE, knobs={})
        if fam == "F2" and nseg == 1 and deal["single"].next():
            base["single"], base["entry"] = True, "g6d_wino_conv3x3"
        if base["kb"] == 3:
            base["k7"] = bool(deal["k7"].next())
        fixed = dict(cell["knobs"])
        if fam == "F4C":
            fixed["w43_map"] = deal["map"].next()
        if fam == "W16" and cell["waves"] == "1w" and (want in ("none", "no-ws") or idx % 2):
            fixed["wino16_2w"] = 0                      # (a split launch runs the one-wave kernel under either value of the knob)
        cands = []
        for Cin in CINS[fam]:
            if len(cands) >= 6:                             # (ascending Cin: the smallest sizes that reach the cell)
                break
            for Cout in cell["couts"]:
                for kn in _knob_variants(fam, r):
                    c = dict(base, Cin=Cin, Cout=Cout, knobs=dict(fixed, **kn))
                    if work_of(c) > MAX_WORK:
                        continue
                    pa = model(c, AMPLE)
                    if pa is None:
                        continue
                    if want == "no-ws":
                        if pa["splits"] < 2:              # a NULL workspace that takes a split away
                            continue
                        c["ws"] = None
                    elif want == "clamped":
                        if pa["splits"] < 2:
                            continue
                        k = r.randrange(1, pa["splits"])
                        if fam == "W16" and cell["waves"] == "2w":
                            k = 0                           # room for less than one partial image: the two-waves kernel's only clamped launch
                        c["ws"] = COUNTER_BYTES + int(k * pa["tile_bytes"]) + (r.choice((0, 4, 1000)) if k else r.choice((1, 4096)))
                    p = model(c)
                    if split_class(p["splits"], p["cps"], p["nchunks"], pa["splits"], c["ws"] is None) != want:
                        continue
                    if fam == "W16" and cell["waves"] == "2w" and p["splits"] != 1:
                        continue
                    if fam == "W16" and cell["waves"] == "1w" and p["splits"] == 1:
                        c["knobs"]["wino16_2w"] = 0         # an un-split launch runs the one-wave kernel only by the knob
                    kd = kd_of(c)
                    if kd > 1 and want in ("even", "tail") and idx < 2 and p["cps"] % kd == 0:
                        continue                            # a split boundary inside the sub-filter blocks of one channel chunk
                    cands.append(c)
        if cands:
            cands.sort(key=work_of)
            return r.choice(cands[:8])
    raise RuntimeError(f"no case found for {cell}")


# ------------------------------------------------------------------------------------------------------------------ the cell table
def cell_id(fam, form, split):
    return f"{fam}-{form}-{split}"


WINO = "gen6d_amd/csrc/wino_conv.hip"
W16F = "gen6d_amd/csrc/wino16_conv.hip wino16_pick"
W43 = "gen6d_amd/csrc/wino43_conv.hip"
PLAN = "gen6d_amd/csrc/wino_plan.h"


def _probe(fam, **over):
    c = dict(fam=fam, entry=ENTRY[fam], single=False, mode={"W16": 2}.get(fam, 0), kb=5 if fam in CORR_FAMS else 0, k7=False, segs=[(2, 9, 13)],
             Cin=64, Cout=64 if fam != "F2" else 128, relu=0, bias=0, full=True, pool=False, c_off=0, in_tail=0, ldf=0, ldp=0, rev=False, ws=AMPLE, knobs={})
    c.update(over)
    return c


def _declare():
    for sp in SPLITS:
        CELLS[cell_id("F2", "wide", sp)] = dict(fam="F2", form="wide", split=sp, knobs={"wino_wide": 2}, couts=(128, 256), cases=[])
        CELLS[cell_id("F2", "square", sp)] = dict(fam="F2", form="square", split=sp, knobs={"wino_wide": 0}, couts=(64, 128, 192), cases=[])
    for sp in SPLITS:
        CELLS[cell_id("F2C", "nwn1", sp)] = dict(fam="F2C", form="nwn1", split=sp, kb=5, knobs={}, couts=(32, 96), cases=[])
        CELLS[cell_id("F2C", "nwn2", sp)] = dict(fam="F2C", form="nwn2", split=sp, kb=5, knobs={}, couts=(64, 128), cases=[])
    for mode, name in ((1, "bf16"), (2, "fp16")):
        for waves in ("2w", "1w"):
            for sp in SPLITS:
                if waves == "2w" and sp in ("even", "tail"):
                    EXCLUDED.append(dict(id=cell_id("W16", f"{name}-2w", sp), file=W16F, condition="two_waves = trunk && knob wino16_2w != 0 && a.splits == 1: a split launch "
                                         "runs the one-wave kernel", probe=_probe("W16", mode=mode, Cin=128, knobs={"wino16_2w": 1, "wino_split_max": 2, "wino_split_gain": 1.0,
                                                                                                                     "wino_split_fix": 0.0, "wino_split_per": 0.0})))
                    continue
                CELLS[cell_id("W16", f"{name}-{waves}", sp)] = dict(fam="W16", form=f"{name}-{waves}", split=sp, mode=mode, waves=waves, knobs={}, couts=(64, 128), cases=[])
    for m in ("0k", "0g", "1", "2"):
        for sp in SPLITS:
            CELLS[cell_id("F4", f"map{m}", sp)] = dict(fam="F4", form=f"map{m}", split=sp, map=m, knobs={"w43_map": {"0k": 0, "0g": 1 + len(sp) % 2, "1": 1, "2": 2}[m]},
                                                        couts=(64,) if m == "0g" else (128, 192), cases=[])
    for kb in (5, 3):
        for nt in (2, 4):
            for sp in SPLITS:
                CELLS[cell_id("F4C", f"kd{kb * kb}-nt{nt}", sp)] = dict(fam="F4C", form=f"kd{kb * kb}-nt{nt}", split=sp, kb=kb, knobs={},
                                                                         couts=(32, 96) if nt == 2 else (64, 128), cases=[])
    forced = {"wino_split_max": 4, "wino_split_gain": 1.0, "wino_split_fix": 0.0, "wino_split_per": 0.0}
    EXCLUDED.extend([
        dict(id="W16-wide", file=PLAN + " f2_shape", condition="wide = wide_on && !mm && ...: the 16-bit kernels have 64-channel blocks only",
             probe=_probe("W16", Cout=128, knobs={"wino_wide": 2})),
        dict(id="F2C-wide", file=PLAN + " f2_shape", condition="wide = ... && kd == 1 && ...: the correlation runs square blocks", probe=_probe("F2C", Cout=128, Cin=16, knobs={"wino_wide": 2})),
        dict(id="F2-nwn1", file=WINO + " wino_multi_args", condition="(Cout & 63): the trunk entry takes multiples of 64 channels, so 32-channel blocks never form",
             probe=_probe("F2", Cout=96)),
        dict(id="F4-nt2", file=W43 + " w43_multi_args, w43_prepare", condition="(Cout & 63) at the entry; kd != 25 && kd != 9 && nt != 4 in the launcher", probe=_probe("F4", Cout=96)),
        dict(id="F2C-kd9", file=WINO + " wino_corr_args", condition="kblocks != 5: the F(2x2,3x3) correlation has the 25-block kernel only", probe=_probe("F2C", kb=3, Cin=16)),
        dict(id="F4C-kd49", file=W43 + " w43_corr_args", condition="kblocks != 5 && kblocks != 3", probe=_probe("F4C", kb=7, Cin=8)),
        dict(id="F2-square-even-3chunks", file=PLAN + " split_search", condition="nchunks >= 4: three chunks are never split", probe=_probe("F2", Cin=24, Cout=64, knobs=forced)),
        dict(id="F4-map2-even-3chunks", file=PLAN + " split_search", condition="nchunks >= 4: three chunks are never split",
             probe=_probe("F4", Cin=24, Cout=128, knobs={"w43_split_max": 4, "w43_split_gain": 1.0})),
        dict(id="W16-fp16-1w-even-3chunks", file=PLAN + " split_search", condition="nchunks >= 4 (chunks of 16 channels): Cin = 48 is never split",
             probe=_probe("W16", Cin=48, knobs=dict(forced, wino16_2w=0))),
    ])


def _file(cid, c, n):
    c["cell"] = cid
    c["id"] = f"{cid}#{len(CELLS[cid]['cases'])}"
    c["seed"] = 1000 * n + len(CELLS[cid]["cases"])
    CELLS[cid]["cases"].append(c)
    CASES.append(c)


# Draws that tests/test_wino_sweep_cpu.py's conditioning checks turned down: (cell id, index) -> how many further draws were taken.  A
# replaced case is drawn again from the same stream, never dropped.
REPLACED = {}


def _enumerate():
    for n, (cid, cell) in enumerate(list(CELLS.items())):
        r = random.Random(3600 + n)
        deal = _dealers(13 * n)
        for idx in range(PER_CELL):
            c = _draw(cell, r, deal, idx)
            for _ in range(REPLACED.get((cid, idx), 0)):
                c = _draw(cell, r, deal, idx)
            _file(cid, c, n)
    # the two-waves 16-bit kernel beside a split launch of the one-wave kernel on the SAME shape: the last two un-split two-waves cases of an
    # arithmetic are its first even and tail cases with the split switched off
    for name in ("bf16", "fp16"):
        for k, sp in ((2, "even"), (3, "tail")):
            src = CELLS[cell_id("W16", f"{name}-1w", sp)]["cases"][0]
            dst = CELLS[cell_id("W16", f"{name}-2w", "none")]["cases"][k]
            keep = {f: dst[f] for f in ("cell", "id", "seed")}
            dst.clear()
            dst.update(src, knobs={"wino_split_max": 1}, twin=src["id"], **keep)


_declare()
_enumerate()


# ------------------------------------------------------------------------------------------------------------------ filing
def classify(route, route_ample, no_ws):
    """The cell id of a g6d_wino_multi_route report (lib.G6dWinoRoute) beside the report of the same launch with ample workspace."""
    sp = split_class(route.splits, route.chunks_per_split, route.nchunks, route_ample.splits, no_ws)
    e = route.entry
    if e in (0, 1):
        return cell_id("F2", "wide" if route.wide else ("square" if route.nwn == 2 else f"nwn{route.nwn}"), sp)
    if e == 4:
        return cell_id("F2C", ("wide" if route.wide else f"nwn{route.nwn}") if route.kd == 25 else f"kd{route.kd}", sp)
    if e == 2:
        return cell_id("W16", "wide" if route.wide else "?-" + {1: "1w", 2: "2w"}.get(route.family, "fp32"), sp)
    gy = route.grid2 // route.blocks
    if e == 3:
        return cell_id("F4", f"nt{route.nwn}" if route.nwn != 4 else "map" + ("0g" if gy == 1 else "0k" if route.map_mode == 0 else str(route.map_mode)), sp)
    return cell_id("F4C", f"kd{route.kd}-nt{route.nwn}", sp)


def classify_case(case, route, route_ample):
    cid = classify(route, route_ample, case["ws"] is None)
    return cid.replace("?", {1: "bf16", 2: "fp16"}.get(case["mode"], "fp32"))
