"""A deterministic sampler of valid G6dConv descriptors, filed by the route g6d_conv_igemm takes with them (g6d_conv_route).

Pure Python, fixed seeds, no GPU and no library call: CASES and CELLS are built at import, so the pytest ids are stable.
tests/test_conv_sweep_cpu.py proves on the host that every case is accepted and lands in the cell it is filed under (and that the
excluded cells are unreachable); tests/test_conv_sweep_gpu.py runs every cell against the float64 reference.

A CELL is a route: (family, tile, prologue mode, split class, row order) for the implicit GEMM (families 0 and 5), (family, prologue
mode, 2-D / 3x3x3, split / unsplit) for the kernels that take a descriptor over (1 LDS patch, 2 F(2x2,3x3), 3 F(4x4,3x3), 4 narrow).
Split classes: "none" (one block per tile, not clamped), "auto" (the launcher's rule), "forced" (split_k > 1), "clamped" (the rule's
count cut down by a small workspace: case["ws_fit"] = the counts that fit).  A CASE is a dict in the vocabulary of CONV_CASES
(tests/conv_case.py) plus: cell, knobs {name: value}, and the markers wino / wino43 (hand the transformed filters over), pairs (the
loader variant 3 / 4 / 5), ws_fit, fin (fused finalisation, with stats), no_bias.

Inside a cell the free dimensions are drawn at random or dealt round-robin (so that every listed value occurs): kd, kh != kw, strides,
padding none / same / larger, odd D H W, Cin with a tail chunk, partial tiles in M and Cout, channel-slice views on both sides, bias,
activation, ragged affine groups, in_mod / mul_group, statistics none / one group / whole images aligned with the tiles / straddling
them, finalisation.  Sizes: the smallest that reach the cell, M * K * Cout <= 2^26 multiply-adds (position-major cells and the unsplit
128x128 cell may pass it: they need >= 4 tiles of images / >= 256 blocks by definition).

The domain is the documented contract (include/gen6d_hip.h): rows_per_group 0 or whole images that divide N; mul and relu only with the
affine; pairs with Cin % 8 == 0 (variant 3) / % 32 (4, 5), Cout > 32, no mul, variant 5 without prologue in the descriptor (ops.conv runs
the affine as a hand-over pass)."""
import itertools
import random

MAX_WORK = 1 << 26
COUNTER_BYTES = 16384
TILES = ((128, 128), (128, 64), (128, 32), (64, 64))
MODES = {0: "none", 1: "affine", 2: "affine-per-group", 3: "mul+affine", 4: "mul+affine-per-group"}
SPLITS = ("none", "auto", "forced", "clamped")

# The bar each family borrows, quoted with its test (the metric is that test's: max |error| / max |reference| for maps, statistics and
# the finalised affine; the pair tests grade sums as |error| / count / range and squares / range^2):
BARS = {
    0: dict(map=2e-5, stats=2e-5, fin=1e-4, src="tests/test_kernels_gpu.py::test_conv_igemm (conv_case.run_conv_case)"),
    1: dict(map=2e-5, stats=2e-5, fin=1e-4, src="tests/test_kernels_gpu.py::test_conv_igemm (conv_case.run_conv_case: the LDS-patch shapes)"),
    2: dict(map=4e-5, stats=4e-5, fin=1e-4, src="tests/test_kernels_gpu.py::test_conv_on_winograd_kernel (conv_case.run_conv_case, wino)"),
    3: dict(map=1e-5, stats=2e-5, fin=1e-4, src="tests/test_wino43_gpu.py::test_conv_on_wino43_kernel"),
    4: dict(map=2e-5, stats=2e-5, fin=1e-4, src="tests/test_kernels_gpu.py::test_conv_narrow (conv_case.run_conv_case)"),
    5: dict(map=2e-6, stats=2e-6, fin=None, src="tests/test_conv_igemm_pairs_gpu.py BAR (test_stride2_3d's metrics)"),
}
# largest K = taps * Cin of the test whose bar is borrowed: the sweep stays below it
MAX_K = {0: 15 * 15 * 512, 1: 27 * 100, 2: 27 * 256, 3: 27 * 128, 4: 9 * 256, 5: 27 * 64}

CIN_TAIL = (4, 20, 36, 100)
COUT_PARTIAL = (1, 3, 33, 40, 72, 200)


def tile_name(bm, bn):
    return f"{bm}x{bn}"


# ------------------------------------------------------------------------------------------------------------------ the cell table
CELLS = {}          # id -> dict(family, ..., cases=[...])
EXCLUDED = []       # dict(id, family, ..., file, condition, probe = a case built for the cell that must route elsewhere or be refused)


def igemm_cell_id(fam, bm, bn, mode, split, pm):
    return f"f{fam}-{tile_name(bm, bn)}-m{mode}-{split}-{'pm' if pm else 'row'}"


def other_cell_id(fam, mode, dim, split):
    return f"f{fam}-m{mode}-{dim}-{'split' if split else 'unsplit'}"


def _declare():
    for fam in (0, 5):
        for (bm, bn), mode in itertools.product(TILES, (0, 1, 2, 3, 4)):
            why = None
            if fam == 5 and mode >= 3:
                why = ("gen6d_amd/csrc/conv_igemm.hip conv_route", "math_mode 3 - 5 take no multiplier: d.mul is refused")
            elif fam == 5 and bn == 32:
                why = ("gen6d_amd/csrc/conv_igemm.hip conv_route", "math_mode 3 - 5 need Cout > 32, and bn = 32 only for Cout <= 32")
            elif (bm, bn) == (128, 128) and mode >= 2:
                why = ("gen6d_amd/csrc/conv_igemm.hip conv_route", "bn == 128 && (d.mul || (d.in_scale && d.in_affine_per_n)) narrows the tile to 128x64")
            for split in SPLITS:
                cid = igemm_cell_id(fam, bm, bn, mode, split, 0)
                if why:
                    EXCLUDED.append(dict(id=cid, family=fam, bm=bm, bn=bn, mode=mode, split=split, pm=0, file=why[0], condition=why[1]))
                else:
                    CELLS[cid] = dict(family=fam, bm=bm, bn=bn, mode=mode, split=split, pm=0, cases=[])
            cid = igemm_cell_id(fam, bm, bn, mode, "none", 1)
            if why:
                EXCLUDED.append(dict(id=cid, family=fam, bm=bm, bn=bn, mode=mode, split="none", pm=1, file=why[0], condition=why[1]))
            else:
                CELLS[cid] = dict(family=fam, bm=bm, bn=bn, mode=mode, split="none", pm=1, cases=[])
            for split in ("auto", "forced"):
                EXCLUDED.append(dict(id=igemm_cell_id(fam, bm, bn, mode, split, 1), family=fam, bm=bm, bn=bn, mode=mode, split=split, pm=1,
                                     file="gen6d_amd/csrc/conv_igemm.hip igemm_position_major", condition="splits == 1: a split launch keeps the row order"))
    # families 1 - 3: prologue mode x {2-D, 3x3x3} x {split, unsplit}; family 4: one route
    for fam, modes in ((1, (0, 1, 3)), (2, (0, 1, 2, 3)), (3, (0, 1, 2))):
        for mode, dim, split in itertools.product(modes, ("2d", "3d"), (0, 1)):
            cid = other_cell_id(fam, mode, dim, split)
            if mode == 3 and dim == "3d":
                f = {1: ("gen6d_amd/csrc/conv_patch.hip g6d_conv_patch_eligible", "d.mul && !k2"),
                     2: ("gen6d_amd/csrc/wino_conv.hip g6d_wino_eligible", "d.mul && (!k2 || !d.in_scale)")}[fam]
                EXCLUDED.append(dict(id=cid, family=fam, mode=mode, dim=dim, split=split, file=f[0], condition=f[1]))
            else:
                CELLS[cid] = dict(family=fam, mode=mode, dim=dim, split=split, cases=[])
    for split in (0, 1):      # the cells of the issue's own examples
        EXCLUDED.append(dict(id=other_cell_id(3, 3, "2d", split), family=3, mode=3, dim="2d", split=split,
                             file="gen6d_amd/csrc/wino43_conv.hip g6d_wino43_eligible", condition="d.mul: F(4x4,3x3) has no multiplier prologue"))
        EXCLUDED.append(dict(id=f"f1-in_mod-2d-{'split' if split else 'unsplit'}", family=1, mode=3, dim="2d", split=split, in_mod=True,
                             file="gen6d_amd/csrc/conv_patch.hip g6d_conv_patch_eligible", condition="d.in_image_mod > 0 || d.mul_group_images > 0"))
    CELLS["f4-m0-2d-unsplit"] = dict(family=4, mode=0, dim="2d", split=0, cases=[])
    for why, extra in (("!d.mul && !d.in_scale && !d.stats: the kernel has neither prologue nor statistics", dict(aff=True)),
                       ("kd == 1 && Di == 1: 2-D layers only", dict(dim="3d"))):
        EXCLUDED.append(dict(id=f"f4-{'m1-2d' if 'aff' in extra else 'm0-3d'}-unsplit", family=4, mode=1 if "aff" in extra else 0,
                             dim=extra.get("dim", "2d"), split=0, file="gen6d_amd/csrc/conv_igemm.hip conv_narrow_eligible", condition=why))


_declare()


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


def out_extent(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def rows_of(c):
    return c["N"] * out_extent(c["D"], c["k"][0], c["s"][0], c["p"][0]) * out_extent(c["H"], c["k"][1], c["s"][1], c["p"][1]) * \
        out_extent(c["W"], c["k"][2], c["s"][2], c["p"][2])


def work_of(c):
    return rows_of(c) * c["k"][0] * c["k"][1] * c["k"][2] * c["Cin"] * c["Cout"]


def total_of(c):
    return c["k"][0] * c["k"][1] * c["k"][2] * ((c["Cin"] + 31) // 32)


def _geometry(r, kd3, want_rows, stride_ok=True, taps_max=None):
    """Draw kernel, strides, padding and odd map sizes, then the image count that puts the output rows into want_rows = (lo, hi)."""
    for _ in range(4000):
        kd = 3 if kd3 else 1
        kh, kw = r.choice((1, 3, 5, 7)), r.choice((1, 3, 5, 7))
        if taps_max and kd * kh * kw > max(taps_max, kd):
            continue
        k = (kd, kh, kw)
        s = tuple(r.choice((1, 2)) if stride_ok else 1 for _ in range(3))
        if not kd3:
            s = (1,) + s[1:]
        padc = [r.choice(("none", "same", "larger")) for _ in range(3)]
        p = tuple({"none": 0, "same": kk // 2, "larger": kk // 2 + 1}[pc] for kk, pc in zip(k, padc))
        if not kd3:
            p = (0,) + p[1:]
        D = r.choice((3, 5, 7)) if kd3 else 1
        H, W = r.choice((1, 3, 5, 7, 9, 11, 13, 15)), r.choice((1, 3, 5, 7, 9, 11, 13, 15))
        ext = [out_extent(i, kk, ss, pp) for i, kk, ss, pp in zip((D, H, W), k, s, p)]
        if min(ext) < 1:
            continue
        # an axis on which EVERY output position reads padding only makes the whole output bias-only: a constant map has no range for
        # the relative metric and no variance for the finalised affine (1 / sqrt(0 + eps) amplifies a statistics error 1000-fold)
        if any(all(not (0 <= o * ss - pp + t < i) for o in range(e) for t in range(kk)) for i, kk, ss, pp, e in zip((D, H, W), k, s, p, ext)):
            continue
        per = ext[0] * ext[1] * ext[2]
        lo, hi = want_rows
        n_lo, n_hi = (lo + per - 1) // per, hi // per
        if n_lo > n_hi or n_hi < 1:
            continue
        N = r.randint(max(n_lo, 1), min(n_hi, max(n_lo, 1) + 6))
        return dict(N=N, D=D, H=H, W=W, k=k, s=s, p=p)
    raise RuntimeError("no geometry")


def _prologue(c, mode, r, deal):
    """The operands of loader mode 0 - 4 (as igemm_mode): affine, its groups (ragged where the draw says so), multiplier and query batching."""
    N = c["N"]
    if mode >= 1:
        c["aff"] = True
        c["relu"] = deal["relu"].next()
    if mode in (2, 4):
        if mode == 4 and N >= 4 and N % 2 == 0 and deal["qbatch"].next():
            k = N // 2                                     # a query batch: 2 queries of k images share k inputs, own multiplier, own table
            c.update(per_n=k, in_mod=k, mul_group=k)
        else:
            c["per_n"] = deal["per_n"].next(lambda v: v <= max(N, 1))      # 1 = a table per image; 2 / 3: a ragged last group when N % k
    if mode >= 3:
        c["mul"] = True
        if mode == 3 and N >= 2 and deal["qbatch"].next():
            c["mul_group"] = deal["per_n"].next(lambda v: v <= N)
    return c


def _epilogue(c, r, deal, bm):
    """Bias, activation, channel-slice views, statistics and finalisation."""
    if not deal["bias"].next():
        c["no_bias"] = True
    c["act"] = deal["act"].next()
    ld = deal["ld"].next()
    if ld in ("in", "both"):
        c["ld_in"] = c["Cin"] + 64 + 4 * r.randint(0, 3)      # the view starts at channel 64 of a wider row (conv_case.operands)
    if ld in ("out", "both"):
        c["ld_out"] = c["Cout"] + r.choice((1, 3, 8))
    rows = rows_of(c)
    per = rows // c["N"]
    kind = deal["stats"].next()
    if kind != "none":
        c["stats"] = True
        c["fin"] = bool(deal["fin"].next())
        if kind != "one":
            # whole images per group, the group count dividing N; "aligned" asks for groups made of whole tiles where a divisor allows
            # it, "straddle" for group boundaries inside tiles
            divs = [g for g in range(1, c["N"] + 1) if c["N"] % g == 0]
            al = [g for g in divs if (g * per) % bm == 0]
            st = [g for g in divs if (g * per) % bm != 0 and g < c["N"]] or [g for g in divs if (g * per) % bm != 0]
            pick = al if (kind == "aligned" and al) else (st or divs)
            c["rpg"] = r.choice(pick) * per
    return c


def stats_kind(c, bm=128):
    if not c.get("stats"):
        return "none"
    if not c.get("rpg"):
        return "one"
    return "aligned" if c["rpg"] % bm == 0 else "straddle"


def _dealers(seed):
    return dict(relu=Deal((0, 1), seed + 1), per_n=Deal((1, 2, 3, 2), seed + 2), qbatch=Deal((0, 1, 0), seed + 3), bias=Deal((1, 1, 0), seed + 4),
                act=Deal((0, 1, 2), seed + 5), ld=Deal(("none", "in", "out", "both"), seed + 6),
                stats=Deal(("none", "one", "aligned", "straddle", "straddle"), seed + 7), fin=Deal((1, 0), seed + 8),
                cin=Deal(CIN_TAIL + (8, 64), seed + 9), kd3=Deal((0, 1, 0), seed + 10))


# ------------------------------------------------------------------------------------------------------------------ implicit GEMM
PER_CELL = 4
_COUT = {(128, 128): (72, 200, 136), (128, 64): (33, 40, 64), (128, 32): (1, 3, 8, 20, 32), (64, 64): (33, 40, 72, 200)}


def _igemm_case(fam, bm, bn, mode, split, r, deal, idx):
    """One row-order case of an implicit-GEMM cell.  The tile is reached as conv_route reaches it: Cout picks the channel width, the
    row count M and the split class pick the branch of the tile policy (a forced split_k skips the policy)."""
    pairs = fam == 5
    forced_none = split == "none" and idx % 2 == 0       # "none" comes about two ways: split_k = 1, or a reduction too short to split
    skip_policy = split == "forced" or forced_none
    couts = list(_COUT[(bm, bn)])
    if (bm, bn) == (128, 64) and (mode >= 2) and (skip_policy or idx % 2):
        couts = [72, 200]                                # the narrowed 128x128
    if pairs:
        couts = [v for v in couts if v > 32]
    cout = couts[(idx + r.randint(0, 1)) % len(couts)] if (bm, bn) != (128, 64) or couts[0] != 72 else couts[idx % 2]
    wide = cout > 64
    # rows
    if bm == 64:
        rows = (1, 64) if (skip_policy or idx % 2 == 0) else (2048, 2300)      # M <= 64; or the policy's mid-size branch
        if pairs and rows[0] == 2048:
            rows = (1, 64)
    elif (bm, bn) == (128, 128):
        rows = (65, 900) if skip_policy else (1025, 2047)                    # the policy leaves 128x128 only between its two M rules
    elif (bm, bn) == (128, 64):
        if skip_policy:
            rows = (65, 900)
        elif wide and mode >= 2:
            rows = (65, 2047)
        elif wide:
            rows = (65, 1024)                                               # M <= 1024 && bn == 128 narrows
        else:
            rows = (65, 2047)
    else:
        rows = (1, 1500)
    natural_none = split == "none" and not forced_none
    need_total = {"auto": 8, "clamped": 16, "forced": 4, "none": 1}[split]
    for attempt in range(600):
        if attempt == 200:
            cout = min(couts)                             # (a wide Cout can leave no reduction long enough inside the work limit)
        kd3 = bool(deal["kd3"].next())
        g = _geometry(r, kd3, rows, taps_max=1 if natural_none and r.random() < 0.5 else None)
        cin = deal["cin"].next(lambda v: (not pairs) or v % 8 == 0) if not pairs else r.choice((8, 32, 64, 40, 96))
        c = dict(g, Cin=cin, Cout=cout)
        if pairs:
            var = (3, 4, 5)[idx % 3] if mode == 0 else (3, 4)[idx % 2]
            if var >= 4:
                c["Cin"] = r.choice((32, 64))
            c["pairs"] = var
        T = c["k"][0] * c["k"][1] * c["k"][2]
        if natural_none and total_of(c) >= 8:
            continue
        if not natural_none and total_of(c) < need_total:
            continue
        if work_of(c) > MAX_WORK or T * c["Cin"] > MAX_K[fam]:
            continue
        break
    else:
        raise RuntimeError(f"no case for {igemm_cell_id(fam, bm, bn, mode, split, 0)}")
    _prologue(c, mode, r, deal)
    _epilogue(c, r, deal, bm)
    if pairs:      # (modes 0 - 2 draw no multiplier; a channel-slice input view stays: variants 3 / 4 load it, 5 hands it to its pass)
        if c["pairs"] == 5:
            for key in ("aff", "relu", "per_n"):
                c.pop(key, None)
    M = rows_of(c)
    blocks = -(-M // bm) * -(-cout // bn)
    if split == "forced":
        c["split"] = r.choice([v for v in (2, 3, 5, 7) if v <= total_of(c) // 2] or [2])
    elif forced_none:
        c["split"] = 1
    elif split == "clamped":
        c["ws_fit"] = (1, 2, 2, 3)[idx % 4] if total_of(c) // 4 > 3 else (1, 2)[idx % 2]
        c["ws_bytes"] = COUNTER_BYTES + blocks * bm * bn * 4 * c["ws_fit"] + (bm * bn * 2 if c["ws_fit"] > 1 else 0)
        if c["ws_fit"] == 1:
            c["ws_bytes"] = COUNTER_BYTES + blocks * bm * bn * 4 + 64      # room for ONE partial set: the launch falls back to no split
    knobs = {}
    k, s, p = c["k"], c["s"], c["p"]
    if not pairs and k[1:] == (3, 3) and s == (1, 1, 1) and p[1:] == (1, 1):
        knobs["conv_patch"] = 0
        if cout <= 4:
            knobs["conv_narrow"] = 0
    c["knobs"] = knobs
    return c


_PM_MAPS = ((1, 3, (1, 1, 3)), (3, 1, (1, 3, 1)), (3, 3, (1, 3, 3)), (1, 5, (1, 1, 5)), (3, 3, (1, 3, 1)), (5, 3, (1, 1, 3)), (2, 2, (1, 3, 3)), (1, 2, (1, 1, 3)))


def _pm_case(fam, bm, bn, mode, r, deal, idx):
    """A shape igemm_position_major admits on this tile: 2-D, stride 1, "same" padding, a map of 2..64 positions, >= 4 tiles of images,
    un-split.  128-row tiles are taken with split_k = 1 (which skips the tile policy); the 64x64 tile only comes out of the policy, so
    its reduction is kept too short to split (fewer than 8 K steps)."""
    pairs = fam == 5
    maps = [m for m in _PM_MAPS if bm != 64 or m[2][1] * m[2][2] <= 5]      # (the 64x64 tile: a reduction too short to split)
    H, W, k = maps[(idx + r.randint(0, 7)) % len(maps)]
    couts = [v for v in _COUT[(bm, bn)] if not pairs or v > 32]
    if (bm, bn) == (128, 64) and mode >= 2 and idx % 2:
        couts = [72, 200]
    cout = couts[idx % len(couts)]
    if bm == 64:
        N = max(4 * bm, -(-2048 // (H * W))) + r.randint(0, 9)
        if pairs:
            cin = (32, 64, 32, 8)[idx % 4]
            if k[1] * k[2] * ((cin + 31) // 32) >= 8:
                cin = 32
        else:
            cin = deal["cin"].next(lambda v: k[1] * k[2] * ((v + 31) // 32) < 8)
    else:
        N = 4 * bm + r.choice((0, 1, 3, 7, 64, 129))
        cin = r.choice((32, 64, 8)) if pairs else deal["cin"].next(lambda v: v <= 64)
    c = dict(N=N, D=1, H=H, W=W, k=k, s=(1, 1, 1), p=(0, k[1] // 2, k[2] // 2), Cin=cin, Cout=cout)
    if pairs:
        var = (3, 4, 5)[idx % 3] if mode == 0 else (3, 4)[idx % 2]
        if var >= 4:
            c["Cin"] = 32
        c["pairs"] = var
    _prologue(c, mode, r, deal)
    _epilogue(c, r, deal, bm)
    if pairs:
        if c["pairs"] == 5:
            for key in ("aff", "relu", "per_n"):
                c.pop(key, None)
    if bm != 64:
        c["split"] = 1
    c["knobs"] = {"conv_pm": 2, "conv_patch": 0}
    if cout <= 4:
        c["knobs"]["conv_narrow"] = 0
    return c


# ------------------------------------------------------------------------------------------------------------------ families 1 - 4
def _other_case(fam, mode, dim, split, r, deal, idx):
    """A 3x3 / 3x3x3 stride-1 "same" layer for the LDS-patch, Winograd and narrow kernels.  Whether their own launcher splits is its
    cost model's decision: short reductions (and the *_split_max knobs at 1) stay whole, small grids with long reductions split."""
    d3 = dim == "3d"
    k, s, p = ((3, 3, 3), (1, 1, 1), (1, 1, 1)) if d3 else ((1, 3, 3), (1, 1, 1), (0, 1, 1))
    knobs = {}
    if fam == 1:
        # >= 128 well-filled 128-row tiles run unsplit; 100..127 tiles with >= 4 channel chunks split (g6d_conv_patch_eligible)
        if split:
            cin, cout = (100, 128, 256, 100)[idx % 4], (1, 3, 2, 1)[idx % 4] if not d3 else 1
            tiles = {100: 104, 128: 100, 256: 52}[cin] + idx
            if d3:
                cin, tiles = 100, 100 + 2 * idx            # (K = 2700, the largest of the patch shapes in CONV_CASES)
        else:
            # (16384 rows at the least: K * Cout stays below 4096 to keep the work limit)
            cin, cout = ((4, 33), (4, 40), (20, 8), (36, 8))[idx % 4]
            if d3:
                cin, cout = ((4, 33), (8, 8), (4, 20), (20, 5))[idx % 4]
            tiles = 128 + idx
        if d3 and not split and idx == 3:
            c = dict(N=8, D=8, H=15, W=15, k=k, s=s, p=p, Cin=cin, Cout=cout)                 # odd maps: 4 tiles of 8x8 hold 225 of 256 rows
        elif d3:
            c = dict(N=1 + (idx % 2), D=2 * (tiles // (1 + idx % 2) // 4 + 1), H=16, W=16, k=k, s=s, p=p, Cin=cin, Cout=cout)
            if split:
                c.update(N=1, D=2 * (tiles // 2), H=8, W=16)
        elif not split and idx == 2:
            c = dict(N=65, D=1, H=15, W=15, k=k, s=s, p=p, Cin=cin, Cout=cout)                # odd maps: 2 tiles of 8x16 hold 225 of 256 rows
        elif idx % 2:
            c = dict(N=2 * tiles, D=1, H=8, W=8, k=k, s=s, p=p, Cin=cin, Cout=cout)           # two images per tile
        else:
            c = dict(N=tiles, D=1, H=8, W=16, k=k, s=s, p=p, Cin=cin, Cout=cout)
        if cout <= 4:
            knobs["conv_narrow"] = 0
    elif fam in (2, 3):
        q = 64 if fam == 3 else 32
        if split:
            cin, cout = (64, 128, 96, 64)[idx % 4], (q, 2 * q, q, q)[idx % 4]
            if d3:
                cin, cout = (32, 64, 32, 64)[idx % 4], q
            c = dict(N=1 if d3 else 1 + idx % 2, D=3 if d3 else 1, H=(8, 9, 11, 8)[idx % 4], W=(8, 11, 9, 13)[idx % 4], k=k, s=s, p=p, Cin=cin, Cout=cout)
        else:
            cin, cout = (8, 16, 8, 24)[idx % 4], (q, q, 2 * q, q)[idx % 4]
            c = dict(N=(1, 2, 1, 2)[idx % 4] if d3 else (3, 5, 2, 7)[idx % 4], D=(3, 5)[idx % 2] if d3 else 1, H=(9, 8, 13, 11)[idx % 4], W=(8, 15, 9, 11)[idx % 4], k=k, s=s, p=p, Cin=cin, Cout=cout)
            knobs["wino_split_max" if fam == 2 else "w43_split_max"] = 1
        knobs["wino_min_work"] = 0
        knobs["conv_patch"] = 0
        c["wino43" if fam == 3 else "wino"] = True
    else:
        c = dict(N=(3, 2, 1, 5)[idx % 4], D=1, H=(9, 5, 15, 7)[idx % 4], W=(13, 7, 21, 9)[idx % 4], k=k, s=s, p=p, Cin=(192, 64, 100, 20)[idx % 4],
                 Cout=(4, 1, 3, 2)[idx % 4])
    _prologue(c, mode, r, deal)
    if fam == 1:                                           # g6d_conv_patch_eligible: no in_image_mod, no mul_group_images
        c.pop("in_mod", None); c.pop("mul_group", None)
    if fam == 2 and mode == 3 and idx % 2:
        # a query batch on the F(2x2,3x3) kernel (g6d_wino_eligible admits it on 2-D layers): 2 queries of k images share k inputs,
        # each with its own multiplier map, affine table and, where statistics are drawn, groups of whole images
        kq = 2 + idx // 2
        c.update(N=2 * kq, per_n=kq, in_mod=kq, mul_group=kq)
    if fam == 1 and mode == 1:
        c["per_n"] = (3, 2, 0, 1)[idx % 4]                 # the kernel's one affine mode reads one table or one per group (3: ragged)
    if fam == 1 and not d3 and idx % 2 and c.get("per_n", 0) % 2:
        c["per_n"] = 2                                     # the two images of a tile share their table (pick_kind)
    _epilogue(c, r, deal, 128)
    if fam == 1 and c["H"] == 15:
        c.update(stats=True, fin=bool(idx % 2 or d3), rpg=rows_of(c) // c["N"])      # groups of one 225-row image straddle the tiles
    if fam == 4:
        for key in ("stats", "fin", "rpg"):
            c.pop(key, None)
    if fam in (2, 3) and c.get("act") == 2:
        c["act"] = idx % 2                                 # no LeakyReLU on the Winograd kernels (their *_eligible)
    if fam == 1 and not d3 and idx % 2 and c.get("rpg") and (c["rpg"] // 64) % 2:
        c["rpg"] = 2 * 64 if c["N"] % 2 == 0 else 0        # groups of an even image count for the two-image tile
    c["knobs"] = knobs
    return c


# ------------------------------------------------------------------------------------------------------------------ enumeration
CASES = []


def _file(cid, c):
    c["cell"] = cid
    c["id"] = f"{cid}#{len(CELLS[cid]['cases'])}"
    CELLS[cid]["cases"].append(c)
    CASES.append(c)


def _enumerate():
    for n, (cid, cell) in enumerate(list(CELLS.items())):
        r = random.Random(1000 + n)
        deal = _dealers(7 * n)
        fam = cell["family"]
        for idx in range(PER_CELL):
            if fam in (0, 5) and cell["pm"]:
                c = _pm_case(fam, cell["bm"], cell["bn"], cell["mode"], r, deal, idx)
                _file(cid, c)
                row = dict(c, knobs=dict(c["knobs"], conv_pm=0))       # the same shape in row order: files under the un-split row cell
                _file(igemm_cell_id(fam, cell["bm"], cell["bn"], cell["mode"], "none", 0), row)
            elif fam in (0, 5):
                _file(cid, _igemm_case(fam, cell["bm"], cell["bn"], cell["mode"], cell["split"], r, deal, idx))
            else:
                _file(cid, _other_case(fam, cell["mode"], cell["dim"], cell["split"], r, deal, idx))


_enumerate()


def probe_of(ex):
    """A case built FOR an excluded cell: the CPU test shows that it routes elsewhere or is refused."""
    fam = ex["family"]
    if fam in (0, 5):
        bm, bn = ex["bm"], ex["bn"]
        cout = {128: 72, 64: 40, 32: 8}[bn]
        if ex["pm"]:
            c = dict(N=4 * bm + 8, D=1, H=3, W=3, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), Cin=256, Cout=cout, knobs={"conv_pm": 2, "conv_patch": 0})
            if ex["split"] == "forced":
                c["split"] = 3
        else:
            c = dict(N=1, D=1, H=(7 if bm == 64 else 15), W=(7 if bm == 64 else 15), k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), Cin=64, Cout=cout,
                     knobs={"conv_patch": 0}, split={"none": 1, "forced": 2}.get(ex["split"], 0))
        if ex["mode"] >= 1:
            c["aff"] = True
        if ex["mode"] in (2, 4):
            c["per_n"] = 1
        if ex["mode"] >= 3:
            c["mul"] = True
        if fam == 5:
            c["pairs"] = 3
        return c
    # families 1 - 4: an ACCEPTED case of the same family (the CPU test shows that this neighbour does run on the family) with the one
    # excluded property added, so nothing else can be what turns the probe away
    d3 = ex["dim"] == "3d"
    if fam == 4:
        c = dict(CELLS["f4-m0-2d-unsplit"]["cases"][0])
        if d3:
            c.update(D=3, k=(3, 3, 3), p=(1, 1, 1))
        else:
            c["aff"] = True
        return c
    base = other_cell_id(fam, 1, ex["dim"], ex["split"])                  # the affine cell next to the excluded multiplier cell
    if ex.get("in_mod"):
        base = other_cell_id(1, 3, "2d", ex["split"])                     # the patch kernel's multiplier cell, plus a query batch
    c = dict(CELLS[base]["cases"][0])
    c["mul"] = True
    if ex.get("in_mod"):
        kq = c["N"] // 2
        c.update(N=2 * kq, in_mod=kq, per_n=kq, mul_group=kq)
        c.pop("rpg", None)
    return c


def probe_neighbour(ex):
    """The accepted case a family 1 - 4 probe was made from (None for the implicit-GEMM probes)."""
    fam = ex["family"]
    if fam in (0, 5):
        return None
    if fam == 4:
        return CELLS["f4-m0-2d-unsplit"]["cases"][0]
    return CELLS[other_cell_id(1, 3, "2d", ex["split"]) if ex.get("in_mod") else other_cell_id(fam, 1, ex["dim"], ex["split"])]["cases"][0]


# ------------------------------------------------------------------------------------------------------------------ descriptors
def classify(route):
    """The cell id of a route report (lib.G6dConvRoute)."""
    fam = route.family
    if fam in (0, 5):
        split = "clamped" if route.split_source == 3 else ("none" if route.splits == 1 else ("forced" if route.split_source == 1 else "auto"))
        return igemm_cell_id(fam, route.bm, route.bn, route.mode, split, route.position_major)
    return other_cell_id(fam, route.mode, None, route.splits > 1)


def cell_matches(case, route):
    want = CELLS[case["cell"]]
    if want["family"] != route.family:
        return False
    if route.family in (0, 5):      # (the loader variant of a pair case is the descriptor's math_mode, reported back)
        return classify(route) == case["cell"] and route.math_mode == case.get("pairs", 0)
    return route.mode == want["mode"] and (route.splits > 1) == bool(want["split"]) and (case["k"][0] == 3) == (want["dim"] == "3d")


def descriptor(case, G6dConv, ptr, workspace_bytes):
    """The G6dConv of a case exactly as gen6d_amd.ops.conv fills it, on the operand addresses ptr(name) (fake ones on the host)."""
    c = case
    D, H, W, k, s, p = c["D"], c["H"], c["W"], c["k"], c["s"], c["p"]
    Do, Ho, Wo = [out_extent(i, kk, ss, pp) for i, kk, ss, pp in zip((D, H, W), k, s, p)]
    var = c.get("pairs")
    aff = bool(c.get("aff")) and var != 5
    ld_in = c.get("ld_in", c["Cin"]) if var != 5 else 2 * c["Cin"]
    d = G6dConv(in_=ptr("in"), mul=ptr("mul") if c.get("mul") else None, in_scale=ptr("in_scale") if aff else None,
                in_shift=ptr("in_shift") if aff else None, weight=ptr("weight"), bias=None if c.get("no_bias") else ptr("bias"), out=ptr("out"),
                stats=ptr("stats") if c.get("stats") else None, workspace=ptr("workspace"), workspace_bytes=c.get("ws_bytes", workspace_bytes),
                N=c["N"], Di=D, Hi=H, Wi=W, Cin=c["Cin"], ld_in=ld_in, Do=Do, Ho=Ho, Wo=Wo, Cout=c["Cout"], ld_out=c.get("ld_out", c["Cout"]),
                kd=k[0], kh=k[1], kw=k[2], sd=s[0], sh=s[1], sw=s[2], pd=p[0], ph=p[1], pw=p[2],
                in_relu=int(bool(c.get("relu")) and aff), in_affine_per_n=int(c.get("per_n", 0)) if aff else 0, out_act=c.get("act", 0),
                stat_rows_per_group=c.get("rpg", 0), split_k=c.get("split", 0), math_mode=var or 0, w_exp=3 if var else 0,
                weight_wino=ptr("weight_wino") if (c.get("wino") and not var) else None, in_image_mod=c.get("in_mod", 0),
                mul_group_images=c.get("mul_group", 0), weight_wino43=ptr("weight_wino43") if (c.get("wino43") and not var) else None)
    if c.get("stats") and c.get("fin"):
        d.fin_scale, d.fin_shift, d.fin_counter = ptr("fin_scale"), ptr("fin_shift"), ptr("fin_counter")
        d.fin_count, d.fin_eps, d.fin_groups = float(c.get("rpg") or rows_of(c)), 1e-5, (rows_of(c) // c["rpg"] if c.get("rpg") else 1)
    return d
