"""A deterministic sampler of launches of the 16-bit direct convolution (g6d_conv16_direct_multi_ex) and of the detector correlation
(g6d_corr16_multi_ex), filed by what the HOST code chooses for them: g6d_conv16_direct_route for the convolution, corr16g::pick_tile
(tests/corr16_geom_shim.cpp) for the correlation.

Pure Python, fixed seeds, no GPU and no library call: CASES, CELLS and EXCLUDED are built at import, so the pytest ids are stable.  The
tiling choosers are restated here (halo_model, pick_tw_model, corr_tile_model) only to FIND shapes; tests/test_conv16_sweep_cpu.py proves
on the host that every case lands in its cell by the launcher's own code, and tests/test_conv16_sweep_gpu.py runs every cell.

Families and their cells:
  H  halo-patch kernel, w_layout 1, kd 1:  arithmetic (pairs / b16 = bf16 and fp16 in turn) x tiling shape of the FIRST segment x block form.
     Tiling shapes: in-image at tile width 32 / 16 / 8 / 4, each with an interior tile ("in32i") or with edge tiles only ("in32e"), and the
     eight banded shapes "b<tw>x<bands>x<band height>".  Block forms: wm1 (one pixel tile x 256 / 128 channels), wm2 (two tiles x 128
     channels: 16-bit modes with Cout % 256 != 0), half (Cout = 64: two tiles x two 32-channel groups).
  F  depth-folded 3x3x3 layers (w_layout 2, pairs): in-image tile width x block form (wm1 / half); D in {1, 2, 3, 5} is dealt.
  T  per-tap kernels: loader (lds16 = 16-bit with LDS filters, w_layout 0; frag16 / fragp = 16-bit / pairs with fragment-major filters) x
     pick_tw 64 .. 4 x kd.  Reached under knob conv16_halo = 0 or, with the knob at its default, on maps without a halo tiling (H = 1, 3).
  C  corr16: arithmetic x k x tile width.

A CASE: dict(fam, cell, id, mode 1 bf16 / 2 fp16 / 3 pairs, layout, kd (C: k), segs [(N, D, H, W)], Cin, Cout, relu, full / pool in
{None, "t16", "f32"}, wide (the fp32 full output is a channel slice of rows 64 channels wider), stats in {None, "one", "images", "tiles",
"passes", "rows", "volumes"}, rpg (pixels per statistics group, 0 = one group), knobs, seed).  Pair exponents: slot 0 throughout.

Sizes: the smallest that reach the cell; every case at most 2^27 multiply-adds; taps x Cin within the largest the borrowed bars' tests run
(MAX_K)."""
import random

MAX_WORK = 1 << 27
PER_CELL = 4
ARITH = ("pairs", "b16")
# The bars, with the test each is borrowed from (metric: max |error| / max |reference| of the segment; a 16-bit output adds half an ulp of
# its format; statistics: |sum error| / pixels per group / range and |squares error| / pixels per group / range^2)
BARS = {
    "pairs": dict(map=2e-6, ulp=2.0 ** -21, stat1=2e-6, stat2=4e-6,
                  src="tests/test_conv16w_edges_gpu.py::test_conv16w_edges, tests/test_conv16_gpu.py::test_conv16_direct_multi (pairs: 2e-6 + 2^-21, sums 2e-6 / 4e-6)"),
    "b16": dict(map=2e-5, ulp={1: 2.0 ** -8, 2: 2.0 ** -11}, stat1=2e-5, stat2=4e-5,
                src="tests/test_conv16_gpu.py::test_conv16_direct_multi, tests/test_conv16w_edges_gpu.py::test_conv16w_edges (16-bit: 2e-5 + half an ulp, sums 2e-5 / 4e-5)"),
    "corr-pairs": dict(map=2e-6, src="tests/test_conv16_gpu.py::test_corr16_multi (pairs: 2e-6)"),
    "corr-b16": dict(map=2e-5, src="tests/test_conv16_gpu.py::test_corr16_multi (16-bit: 2e-5)"),
}
MAX_K = {"2d": 9 * 512, "3d": 27 * 128, "corr": 225 * 512}      # taps x Cin of test_conv16_direct_multi (case2, case9) and test_corr16_multi

CELLS = {}          # id -> dict(fam, ..., cases=[...])
EXCLUDED = []       # dict(id, file, condition, probe = a case built for the cell: refused or routed elsewhere)
CASES = []


# ------------------------------------------------------------------------------------------------------------------ chooser models
def halo_model(N, H, W, in_image=False):
    """c16g::halo_tiling restated: (tw, bands, segh, tpi, tiles_x, tiles) or None."""
    best, res = 1e30, None
    for tw in (32, 16, 8, 4):
        th, tx = 128 // tw, -(-W // tw)
        if H >= th:
            tpi = tx * -(-H // th)
            nt, segh, bands = N * tpi, th, 1
        else:
            if th % H or in_image:
                continue
            tpi, nt, segh, bands = 0, tx * -(-(N * H) // th), H, th // H
        if bands * (segh + 2) * (tw + 2) > 288:
            continue
        waste = nt * 128 / (N * H * W)
        if waste < best - 1e-9:
            best, res = waste, (tw, bands, segh, tpi, tx, nt)
    return res


def pick_tw_model(W):
    best, bw = 8, 1e9
    for tw in (64, 32, 16, 8, 4):
        waste = (-(-W // tw) * tw) / W
        if waste < bw - 1e-9:
            bw, best = waste, tw
    return best


def corr_tile_model(H, W, K):
    best, btw = 1e30, 0
    for tw in (32, 16, 8, 4):
        th = 128 // tw
        if (th + K - 1) * (tw + K - 1) > 42 * 1024 // 64:
            continue
        waste = (-(-W // tw) * tw) * (-(-H // th) * th) / (W * H)
        if waste < best - 1e-9:
            best, btw = waste, tw
    return btw


def has_interior(tw, H, W):
    """An in-image tiling holds a tile whose whole halo lies inside the image (c16g::tile_of: y0 >= 1, y0 + TH < H, x0 >= 1, x0 + TW < W)."""
    return H > 2 * (128 // tw) and W > 2 * tw


def shape_name(tw, bands, segh, H, W):
    if bands == 1:
        return f"in{tw}{'i' if has_interior(tw, H, W) else 'e'}"
    return f"b{tw}x{bands}x{segh}"


IN_SHAPES = [f"in{tw}{k}" for tw in (32, 16, 8, 4) for k in "ie"]
BAND_SHAPES = ["b32x2x2", "b16x2x4", "b16x4x2", "b8x2x8", "b8x4x4", "b4x2x16", "b4x4x8", "b4x8x4"]
SHAPES = IN_SHAPES + BAND_SHAPES
# banded shapes th % H == 0 would allow but whose patch bands * (segh + 2) * (tw + 2) passes 288 pixels (NI_MAX pieces)
BAND_TOO_BIG = [(32, 4, 1), (16, 8, 1), (8, 16, 1), (4, 32, 1), (8, 8, 2), (4, 16, 2)]


def _band_of(shape):
    tw, bands, segh = (int(v) for v in shape[1:].split("x"))
    return tw, bands, segh


def shape_tw(shape):
    return _band_of(shape)[0] if shape[0] == "b" else int(shape[2:-1])


def _tables():
    halo, folded, tap, corr = {s: [] for s in SHAPES}, {tw: [] for tw in (32, 16, 8, 4)}, {tw: [] for tw in (64, 32, 16, 8, 4)}, {}
    for H in range(1, 97):
        for W in range(1, 97):
            nmax = min(24 if H * W <= 64 else 9, 1400 // (H * W))
            for N in range(1, nmax + 1):
                m = halo_model(N, H, W)
                if m:
                    halo[shape_name(m[0], m[1], m[2], H, W)].append((N, H, W))
            if H * W <= 700:
                m = halo_model(1, H, W, True)
                if m:
                    folded[m[0]].append((H, W))
    for W in range(1, 131):
        tap[pick_tw_model(W)].append(W)
    for K in (7, 15):
        for H in range(1, 41):
            for W in range(1, 41):
                corr.setdefault((K, corr_tile_model(H, W, K)), []).append((H, W))
    return halo, folded, tap, corr


HALO_TAB, FOLD_TAB, TAP_TAB, CORR_TAB = _tables()


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


OUTS = (("t16", None), ("f32", None), (None, "t16"), ("t16", "t16"), ("f32", "t16"), ("t16", "f32"), (None, "f32"), ("f32", "f32"), (None, None))


def _dealers(seed):
    return dict(m16=Deal((1, 2), seed + 1), wcls=Deal((0, 1, 2, 3), seed + 2), hcls=Deal((0, 1, 2, 3), seed + 3), nseg=Deal((1, 2, 1, 3, 4), seed + 4),
                cin=Deal((32, 64, 96, 128), seed + 5), cout=Deal((128, 256, 384), seed + 6), relu=Deal((1, 0), seed + 7), out=Deal(OUTS, seed + 8),
                st_in=Deal(("none", "none", "one", "images"), seed + 9), st_band=Deal(("none", "one", "tiles", "passes"), seed + 10),
                st_tap=Deal(("none", "none", "one", "rows"), seed + 11), st_fold=Deal(("none", "one", "volumes", "none"), seed + 12),
                part=Deal((1, 0), seed + 13), odd=Deal((1, 0), seed + 14), wide=Deal((1, 0), seed + 15), D=Deal((1, 2, 3, 5), seed + 16),
                ccin=Deal((32, 96, 64), seed + 17), low=Deal((1, 0, 0), seed + 18), cn=Deal((1, 2, 3), seed + 19))


def _cls(v, m, cls):
    """v falls in class cls against the tile extent m: 0 a multiple, 1 one over, 2 one short, 3 another even remainder."""
    rem = v % m
    return (rem == 0, rem == 1, rem == m - 1, rem % 2 == 0 and rem not in (0,))[cls]


def _pick(r, cands, wants, size=lambda g: g):
    """Among cands, those that meet the most of the soft wants (earlier wants weigh more), then the smallest few; one at random."""
    if not cands:
        raise RuntimeError("no candidate")
    def score(g):
        return sum((1 << (len(wants) - i)) for i, wnt in enumerate(wants) if wnt(g))
    top = max(score(g) for g in cands)
    best = sorted((g for g in cands if score(g) == top), key=size)
    return r.choice(best[:5])


def pixels(case):
    return sum(N * D * H * W for N, D, H, W in case["segs"])


def work_of(case):
    taps = case["kd"] ** 2 if case["fam"] == "C" else 9 * case["kd"]
    return pixels(case) * taps * case["Cin"] * case["Cout"]


def _channels(case, r, deal, form, pairs, taps):
    """Cin and Cout the block form allows, inside the work limit and the borrowed bars' reduction length."""
    px = pixels(case)
    couts = {"half": (64,), "wm2": (128, 384), "wm1": (128, 256, 384) if pairs else (256,), "tap": (128, 256, 384)}[form]
    kmax = MAX_K["3d" if taps == 27 else "2d"]
    def cin_ok(v, co):
        return (pairs or v % 64 == 0) and taps * v <= kmax and px * taps * v * co <= MAX_WORK
    for _ in range(len(couts)):
        co = couts[0] if len(couts) == 1 else deal["cout"].next(lambda v: v in couts)
        try:
            case["Cin"], case["Cout"] = deal["cin"].next(lambda v: cin_ok(v, co)), co
            return True
        except ValueError:
            continue
    co = min(couts)
    for v in ((32, 64) if pairs else (64,)):
        if cin_ok(v, co):
            case["Cin"], case["Cout"] = v, co
            return True
    return False


def _outputs(case, deal, even, allow_pool=True):
    stats = case["stats"] is not None
    full, pool = deal["out"].next(lambda o: (o[1] is None or (even and allow_pool)) and (stats or o != (None, None)))
    case["full"], case["pool"] = full, pool
    case["wide"] = bool(full == "f32" and deal["wide"].next())


# ------------------------------------------------------------------------------------------------------------------ H: halo-patch, 2-D
def _small_of(shape, even):
    return [g for g in HALO_TAB[shape] if g[0] * g[1] * g[2] <= 260 and (not even or (g[1] % 2 == 0 and g[2] % 2 == 0))]


def _h_case(arith, shape, form, r, deal, idx):
    pairs = arith == "pairs"
    mode = 3 if pairs else deal["m16"].next()
    tw = shape_tw(shape)
    th = 128 // tw
    banded = shape[0] == "b"
    stats = (deal["st_band"] if banded else deal["st_in"]).next()
    grouped = stats not in ("none", "one")
    nseg = 1 if grouped else deal["nseg"].next()
    wcls, hcls, part, odd = deal["wcls"].next(), deal["hcls"].next(), deal["part"].next(), deal["odd"].next()
    want_pool = idx % 2 == 1
    wants = []
    if want_pool:
        wants.append(lambda g: g[1] % 2 == 0 and g[2] % 2 == 0)
    wants.append(lambda g: _cls(g[2], tw, wcls))
    if banded:
        bands = _band_of(shape)[1]
        if stats == "tiles":
            wants.append(lambda g: g[0] > bands)
        wants.append(lambda g: (g[0] % bands != 0) == bool(part))
    else:
        wants.append(lambda g: _cls(g[1], th, hcls))
        if stats == "images":
            wants.append(lambda g: g[0] >= 2)
    if form != "wm1" and nseg == 1:
        wants.append(lambda g: (halo_model(*g)[5] % 2 == 1) == bool(odd))
    cap = MAX_WORK // (9 * (32 if pairs else 64) * {"half": 64, "wm2": 128, "wm1": 128 if pairs else 256}[form])      # the first segment alone fits
    N, H, W = _pick(r, [g for g in HALO_TAB[shape] if g[0] * g[1] * g[2] <= cap], wants, size=lambda g: g[0] * g[1] * g[2])
    segs = [(N, 1, H, W)]
    even = H % 2 == 0 and W % 2 == 0
    others = [s for s in SHAPES if s != shape and _small_of(s, even)]
    r.shuffle(others)
    for s in others[:nseg - 1]:
        n2, h2, w2 = r.choice(_small_of(s, even))
        segs.append((n2, 1, h2, w2))
    case = dict(fam="H", mode=mode, layout=1, kd=1, segs=segs, relu=deal["relu"].next(), stats=None if stats == "none" else stats, rpg=0, knobs={})
    while not _channels(case, r, deal, form, pairs, 9):
        assert len(case["segs"]) > 1                        # (the first segment fits by construction)
        case["segs"].pop()
    if stats == "images":
        gi = r.choice([g for g in range(1, N + 1) if N % g == 0 and (g < N or N == 1)])
        case["rpg"] = gi * H * W
    elif stats == "tiles":
        case["rpg"] = _band_of(shape)[1] * H * W            # one tile of whole images per group
    elif stats == "passes":
        case["rpg"] = _band_of(shape)[1] // 2 * H * W       # one 64-pixel epilogue pass x W / tw per group: half a tile
    _outputs(case, deal, all(s[2] % 2 == 0 and s[3] % 2 == 0 for s in case["segs"]))
    return case


# ------------------------------------------------------------------------------------------------------------------ F: depth-folded
def _f_case(tw, form, r, deal, idx):
    th = 128 // tw
    D = deal["D"].next()
    stats = deal["st_fold"].next()
    wcls, hcls = deal["wcls"].next(), deal["hcls"].next()
    cap = 1100 // D
    H, W = _pick(r, [g for g in FOLD_TAB[tw] if g[0] * g[1] <= cap], [lambda g: _cls(g[1], tw, wcls), lambda g: _cls(g[0], th, hcls)], size=lambda g: g[0] * g[1])
    N = 2 if (D * H * W <= 400 and idx % 2 == 0) or stats == "volumes" and D * H * W <= 550 else 1
    segs = [(N, D, H, W)]
    if stats != "volumes" and idx % 2 == 1:
        tw2 = r.choice([t for t in (32, 16, 8, 4) if t != tw])
        small = [g for g in FOLD_TAB[tw2] if g[0] * g[1] * D <= 300]
        if small:
            segs.append((1, D) + r.choice(sorted(small, key=lambda g: g[0] * g[1])[:6]))
    case = dict(fam="F", mode=3, layout=2, kd=3, segs=segs, relu=deal["relu"].next(), stats=None if stats == "none" else stats, rpg=0, knobs={})
    while not _channels(case, r, deal, form, True, 27):
        assert len(case["segs"]) > 1
        case["segs"].pop()
    if stats == "volumes":
        case["rpg"] = D * H * W
    _outputs(case, deal, False, allow_pool=False)
    return case


# ------------------------------------------------------------------------------------------------------------------ T: per-tap kernels
def _t_case(loader, tw, kd, r, deal, idx):
    pairs = loader == "fragp"
    mode = 3 if pairs else deal["m16"].next()
    th = 128 // tw
    # the way to the per-tap route: w_layout 0 and kd = 3 never qualify for the halo-patch kernel; fragment-major 2-D layers get there
    # under knob conv16_halo = 0 (even cases) or, at the knob's default, on maps without a halo tiling: H = 1 or 3 (odd cases)
    two_ways = loader != "lds16" and kd == 1
    no_halo = two_ways and idx % 2 == 1
    stats = deal["st_tap"].next()
    nseg = 1 if stats == "rows" else deal["nseg"].next()
    wcls = deal["wcls"].next()
    want_pool = kd == 1 and not no_halo and idx % 4 == 2
    W = _pick(r, [w for w in TAP_TAB[tw] if w <= (130 if tw == 64 else 72)], [lambda w: (w % 2 == 0) == want_pool, lambda w: _cls(w, tw, wcls)])
    D = r.choice((1, 2, 3)) if kd == 3 else 1
    if no_halo:
        H = (1, 3)[(idx // 2) % 2]
    elif want_pool:
        H = r.choice((2, 4, 6))
    else:
        H = r.choice((1, 2, 3, 5, 6, 8)) if kd == 1 else r.choice((1, 2, 3, 4))
    cap = 1200 if kd == 1 else 420
    N = max(1, min(r.choice((1, 2, 3)), cap // (D * H * W)))
    if stats == "rows" and N * D * H < 2 * th:               # two groups of one tile row at the least
        N = -(-2 * th // (D * H))
    segs = [(N, D, H, W)]
    for _ in range(nseg - 1):
        tw2 = r.choice([t for t in (64, 32, 16, 8, 4) if t != tw])
        w2 = r.choice([w for w in TAP_TAB[tw2] if w <= 40 and (not want_pool or w % 2 == 0)] or [tw2])
        segs.append((1, D, H if want_pool else r.choice((1, 2, 3)), w2))
    case = dict(fam="T", mode=mode, layout=0 if loader == "lds16" else 1, kd=kd, segs=segs, relu=deal["relu"].next(), stats=None if stats == "none" else stats,
                rpg=0, knobs={"conv16_halo": 0} if two_ways and not no_halo else {})
    while not _channels(case, r, deal, "tap", pairs, 9 * kd):
        if len(case["segs"]) > 1:
            case["segs"].pop()
        else:
            n, d, h, w = case["segs"][0]
            case["segs"][0] = (max(1, n - 1), d, h, w) if n > 1 else (1, max(1, d - 1), h, w)
    if stats == "rows":
        n, d, h, w = case["segs"][0]
        m = r.choice([v for v in (1, 2) if v * th < n * d * h] or [1])
        case["rpg"] = m * th * w
    _outputs(case, deal, all(s[2] % 2 == 0 and s[3] % 2 == 0 for s in case["segs"]), allow_pool=kd == 1)
    return case


# ------------------------------------------------------------------------------------------------------------------ C: corr16
def _c_case(arith, k, tw, r, deal, idx):
    pairs = arith == "pairs"
    mode = 3 if pairs else deal["m16"].next()
    low = deal["low"].next()
    cin = deal["ccin"].next()
    N = deal["cn"].next()
    cap = MAX_WORK // (k * k * cin * 32)
    cands = [g for g in CORR_TAB[(k, tw)] if N * g[0] * g[1] <= cap]
    if not cands:
        N = 1
        cands = [g for g in CORR_TAB[(k, tw)] if g[0] * g[1] <= cap]
    H, W = _pick(r, cands, [lambda g: (min(g) < k // 2) == bool(low), lambda g: g[0] % (128 // tw) != 0 or g[1] % tw != 0], size=lambda g: -g[0] * g[1] if not low else g[0] * g[1])
    segs = [(N, 1, H, W)]
    case = dict(fam="C", mode=mode, layout=1, kd=k, segs=segs, Cin=cin, Cout=32, relu=0, stats=None, rpg=0, full="f32", pool=None, wide=False, knobs={})
    other = [t for t in (32, 16, 8, 4) if t != tw and (k, t) in CORR_TAB]
    for tw2 in r.sample(other, min(len(other), (0, 1, 0, 2)[idx % 4])):
        h2, w2 = r.choice(sorted(CORR_TAB[(k, tw2)], key=lambda g: g[0] * g[1])[:40])
        if work_of(dict(case, segs=segs + [(N, 1, h2, w2)])) <= MAX_WORK:
            segs.append((N, 1, h2, w2))
    return case


# ------------------------------------------------------------------------------------------------------------------ the cell table
def h_cell(arith, shape, form):
    return f"H-{arith}-{shape}-{form}"


def f_cell(tw, form):
    return f"F-tw{tw}-{form}"


def t_cell(loader, tw, kd):
    return f"T-{loader}-tw{tw}-kd{kd}"


def c_cell(arith, k, tw):
    return f"C-{arith}-k{k}-tw{tw}"


C16 = "gen6d_amd/csrc/conv16_direct.hip c16_direct"


def _declare():
    for arith in ARITH:
        for shape in SHAPES:
            for form in ("wm1", "wm2", "half"):
                if arith == "pairs" and form == "wm2":
                    N, H, W = HALO_TAB[shape][0]
                    EXCLUDED.append(dict(id=h_cell(arith, shape, form), file=C16, condition="wm = Cout % (4 * cw) == 0 ? 1 : 2 with cw = 32 for pairs and Cout % 128 == 0 "
                                         "unless half_tile: pairs run two tiles per block only as the Cout = 64 half tile",
                                         probe=dict(fam="H", mode=3, layout=1, kd=1, segs=[(N, 1, H, W)], Cin=32, Cout=192, relu=0, full="f32", pool=None, wide=False,
                                                    stats=None, rpg=0, knobs={})))
                else:
                    CELLS[h_cell(arith, shape, form)] = dict(fam="H", arith=arith, shape=shape, form=form, cases=[])
        for tw, bands, segh in BAND_TOO_BIG:
            EXCLUDED.append(dict(id=h_cell(arith, f"b{tw}x{bands}x{segh}", "wm1"), file="gen6d_amd/csrc/conv16w_geom.h halo_tiling",
                                 condition="bands * (segh + 2) * (tw + 2) > 288: the patch passes NI_MAX pieces",
                                 probe=dict(fam="H", mode=3 if arith == "pairs" else 2, layout=1, kd=1, segs=[(bands, 1, segh, tw)], Cin=64, Cout=128 if arith == "pairs" else 256,
                                            relu=0, full="f32", pool=None, wide=False, stats=None, rpg=0, knobs={})))
    for tw in (32, 16, 8, 4):
        H, W = FOLD_TAB[tw][0]
        for form in ("wm1", "half"):
            CELLS[f_cell(tw, form)] = dict(fam="F", tw=tw, form=form, cases=[])
        base = dict(fam="F", mode=3, layout=2, kd=3, segs=[(1, 2, H, W)], Cin=32, Cout=128, relu=0, full="f32", pool=None, wide=False, stats=None, rpg=0, knobs={})
        EXCLUDED.append(dict(id=f_cell(tw, "wm2"), file=C16, condition="folded runs pairs only, and pairs take two tiles per block only at Cout = 64", probe=dict(base, Cout=192)))
        EXCLUDED.append(dict(id=f"F-b16-tw{tw}", file=C16, condition="folded && math_mode != 3", probe=dict(base, mode=2, Cin=64)))
    EXCLUDED.append(dict(id="F-banded", file="gen6d_amd/csrc/conv16w.hip c16w_admit", condition="folded: halo_tiling(..., in_image = true) admits no tile of several planes",
                         probe=dict(fam="F", mode=3, layout=2, kd=3, segs=[(2, 2, 4, 16)], Cin=32, Cout=128, relu=0, full="f32", pool=None, wide=False, stats=None, rpg=0, knobs={})))
    EXCLUDED.append(dict(id="F-pool", file=C16, condition="pool_type && kd != 1",
                         probe=dict(fam="F", mode=3, layout=2, kd=3, segs=[(1, 2, 16, 16)], Cin=32, Cout=128, relu=0, full="f32", pool="f32", wide=False, stats=None, rpg=0, knobs={})))
    for loader in ("lds16", "frag16", "fragp", "ldsp"):
        for tw in (64, 32, 16, 8, 4):
            for kd in (1, 3):
                W = TAP_TAB[tw][-1 if tw == 64 else 0]
                if loader == "ldsp":
                    EXCLUDED.append(dict(id=t_cell(loader, tw, kd), file=C16, condition="math_mode == 3 && w_layout == 0: pairs read fragment-major filters only",
                                         probe=dict(fam="T", mode=3, layout=0, kd=kd, segs=[(1, 1, 3, W)], Cin=32, Cout=128, relu=0, full="f32", pool=None, wide=False, stats=None,
                                                    rpg=0, knobs={})))
                    continue
                CELLS[t_cell(loader, tw, kd)] = dict(fam="T", loader=loader, tw=tw, kd=kd, cases=[])
                mode = 3 if loader == "fragp" else 2
                base = dict(fam="T", mode=mode, layout=0 if loader == "lds16" else 1, kd=kd, segs=[(1, 1 if kd == 1 else 2, 3, W)], Cin=64, Cout=128, relu=0, full="f32", pool=None,
                            wide=False, stats=None, rpg=0, knobs={"conv16_halo": 0})
                EXCLUDED.append(dict(id=t_cell(loader, tw, kd) + "-half", file=C16, condition="Cout % 128 && !half_tile; half_tile runs on the halo-patch kernel only",
                                     probe=dict(base, Cout=64)))
                if kd == 3:
                    EXCLUDED.append(dict(id=t_cell(loader, tw, kd) + "-pool", file=C16, condition="pool_type && kd != 1",
                                         probe=dict(base, segs=[(1, 2, 2, 2 * ((W + 1) // 2))], pool="f32")))
    for arith in ARITH:
        for k in (7, 15):
            for tw in (32, 16, 8, 4):
                if (k, tw) in CORR_TAB:
                    CELLS[c_cell(arith, k, tw)] = dict(fam="C", arith=arith, k=k, tw=tw, cases=[])
                else:
                    H, W = CORR_TAB[(7, tw)][0]
                    EXCLUDED.append(dict(id=c_cell(arith, k, tw), file="gen6d_amd/csrc/corr16_geom.h pick_tile",
                                         condition="(th + K - 1) * (tw + K - 1) > STAGE / 64: the patch does not fit a stage",
                                         probe=dict(fam="C", mode=3 if arith == "pairs" else 2, layout=1, kd=k, segs=[(1, 1, H, W)], Cin=32, Cout=32, relu=0, full="f32", pool=None,
                                                    wide=False, stats=None, rpg=0, knobs={})))


def _file(cid, c, n):
    c["cell"] = cid
    c["id"] = f"{cid}#{len(CELLS[cid]['cases'])}"
    c["seed"] = 1000 * n + len(CELLS[cid]["cases"])
    CELLS[cid]["cases"].append(c)
    CASES.append(c)


def _enumerate():
    for n, (cid, cell) in enumerate(list(CELLS.items())):
        r = random.Random(3500 + n)
        deal = _dealers(11 * n)
        for idx in range(PER_CELL):
            if cell["fam"] == "H":
                c = _h_case(cell["arith"], cell["shape"], cell["form"], r, deal, idx)
            elif cell["fam"] == "F":
                c = _f_case(cell["tw"], cell["form"], r, deal, idx)
            elif cell["fam"] == "T":
                c = _t_case(cell["loader"], cell["tw"], cell["kd"], r, deal, idx)
            else:
                c = _c_case(cell["arith"], cell["k"], cell["tw"], r, deal, idx)
            _file(cid, c, n)


_declare()
_enumerate()


# ------------------------------------------------------------------------------------------------------------------ filing
def type_code(case, kind):
    return {None: 0, "t16": 3 if case["mode"] == 3 else 1, "f32": 2}[kind]


def classify(case, route):
    """The cell id of a conv16 route report (lib.G6dConv16Route) for `case` (its first segment's map size decides interior / edge)."""
    s0 = route.seg[0]
    if route.kernel == 0:
        loader = "lds16" if route.w_layout == 0 else ("fragp" if route.math_mode == 3 else "frag16")
        if route.math_mode == 3 and route.w_layout == 0:
            loader = "ldsp"
        return t_cell(loader, 1 << s0.tw_log2, route.kd)
    form = "half" if route.half_tile else f"wm{route.wm}"
    tw = 1 << s0.tw_log2
    if route.folded:
        return f_cell(tw, form) if s0.bands == 1 else "F-banded"
    _, _, H, W = case["segs"][0]
    return h_cell("pairs" if route.math_mode == 3 else "b16", shape_name(tw, s0.bands, 1 << s0.segh_log2, H, W), form)


def stat_groups(case):
    """Rows of the statistics table the case's launch adds to."""
    if not case["stats"]:
        return 0
    if not case["rpg"]:
        return 1
    return max(-(-(N * D * H * W) // case["rpg"]) for N, D, H, W in case["segs"])
