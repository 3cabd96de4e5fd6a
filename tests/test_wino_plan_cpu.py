"""The host plan of the Winograd launches (gen6d_amd/csrc/wino_plan.h: quarter list, F(2x2) block shape, limits, split over gridDim.z,
LDS sizes), built for the host (tests/wino_plan_shim.cpp) and compared with the arithmetic the two launchers (wino_run of wino_conv.hip,
w43_run of wino43_conv.hip) spelled out before the header existed, restated below in the same floating-point expression order: the
choice must be that one, not one close to it.  A seeded sample over map sizes, batch, channels, kd, math mode, prologue mode and the
wino_wide knob in which every value of every axis appears, plus the edge cases of the split search, the error cases in their order, and
the invariants the kernels rely on.  No GPU needed."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTER_BYTES = 16384                      # G6D_WORKSPACE_COUNTER_BYTES (include/gen6d_hip.h)
COUNTERS = COUNTER_BYTES // 4
WS_DEFAULT = 96 << 20                      # the workspace gen6d_amd/ops.py hands every launch
F2_KNOBS = dict(wide=1, split_max=32, gain=0.85, fix=2.0, per=0.6)      # defaults of gen6d_amd/csrc/common.hip
F4_KNOBS = dict(split_max=32, gain=0.85, chunk_us=2.8)
LL = C.POINTER(C.c_longlong)
I32 = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def wp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wplan") / "wino_plan.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "wino_plan_shim.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.wp_f2_plan.argtypes = [I32, C.c_int, C.c_longlong] + [C.c_int] * 6 + [C.c_size_t, C.c_size_t] + [C.c_int] * 3 + [C.c_double] * 3 + [LL, LL]
    lib.wp_f2_plan.restype = C.c_char_p
    lib.wp_f4_plan.argtypes = [I32] + [C.c_int] * 6 + [C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double, LL, LL]
    lib.wp_f4_plan.restype = C.c_char_p
    lib.wp_split.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_size_t, C.c_int] + [C.c_double] * 7 + [C.c_int, I32]
    lib.wp_f4_limits.argtypes = [C.c_longlong, C.c_longlong] + [C.c_int] * 4
    lib.wp_f4_limits.restype = C.c_char_p
    lib.wp_w16_limits.argtypes = [C.c_int] * 3
    lib.wp_w16_limits.restype = C.c_char_p
    lib.wp_lds.argtypes = [C.c_int] * 5
    lib.wp_lds.restype = C.c_size_t
    lib.wp_segments.argtypes = [I32, C.c_int, I32]
    return lib


# ---- the parent's arithmetic.  A segment is (N, H, W, in_off, ld_in); ws = workspace bytes, None = no workspace
def parent_quarters(segs, cap):
    quarters, in_extent, out_elems, geo = 0, 0, 0.0, []
    for N, H, W, in_off, ld_in in segs:
        n_in = min(N, cap) if cap > 0 else N
        in_extent = max(in_extent, in_off + n_in * H * W * ld_in)
        QH, QW = (H + 7) // 8, (W + 7) // 8
        geo.append((quarters, QH, QW, n_in))
        quarters += N * QH * QW
        out_elems += float(N) * H * W
    return quarters, in_extent, out_elems, geo


def parent_split(nchunks, grid2, slots, room, tile_bytes, out_bytes, chunk_us, block_us, fix, per, gain, split_max, counters=COUNTERS):
    splits = 1
    if room > 0 and grid2 <= counters and split_max > 1 and nchunks >= 4:
        best = 1e30
        sp = 1
        while sp <= split_max and sp <= nchunks // 2:
            if float(sp) * tile_bytes > float(room):
                break
            cps_ = (nchunks + sp - 1) // sp
            real = (nchunks + cps_ - 1) // cps_
            if real == sp:
                rounds = float((grid2 * sp + slots - 1) // slots)
                t = rounds * (cps_ * chunk_us + block_us)
                if sp > 1:
                    t += fix + per * sp + (2 * sp + 1) * out_bytes / 2.5e6
                if t < best * gain:
                    best, splits = t, sp
            sp += 1
    cps = (nchunks + splits - 1) // splits
    return (nchunks + cps - 1) // cps, cps


def _room(ws):
    return ws - COUNTER_BYTES if ws is not None and ws > COUNTER_BYTES else 0


def parent_f2(segs, img_mod, D, mm, mode, kd, Cin, Cout, ws, wide, split_max, gain, fix, per):
    """wino_run up to the launch: the error string, or the plan."""
    quarters, in_extent, out_elems, geo = parent_quarters(segs, img_mod * D if img_mod > 0 else 0)
    wide_on, wide_all = wide != 0, wide == 2
    is_wide = wide_on and not mm and mode == 0 and kd == 1 and (Cout & 127) == 0 and (wide_all or in_extent >= 6 * 16 * Cin * Cout)
    nq = 2 if is_wide else 4
    blocks = (quarters + nq - 1) // nq
    if blocks > 0x3fffffff:
        return "wino_conv3x3: grid too large"
    if in_extent * 4 >= 1 << 31:
        return "wino_conv3x3: input tensor exceeds 2^31 bytes"
    nwn = 4 if is_wide else (1 if Cout & 63 else 2)
    nchunks = kd * (Cin // 16) if mm else kd * (Cin // 8)
    grid2 = blocks * (Cout // (32 * nwn))
    slots = 256 * (2 if nwn == 1 else 1)
    tile_bytes = float(grid2) * (256 if is_wide else 128 * nwn) * 64 * 4
    out_bytes = out_elems * Cout * 4
    splits, cps = parent_split(nchunks, grid2, slots, _room(ws), tile_bytes, out_bytes, 1.2 if mm else 2.7, 4.0, fix, per, gain, split_max)
    return dict(quarters=quarters, in_bytes=in_extent * 4, blocks=blocks, grid2=grid2, nchunks=nchunks, splits=splits, cps=cps, wide=int(is_wide), nq=nq,
                nwn=nwn, geo=geo, tile_bytes=tile_bytes)


def parent_f4_limits(quarters, in_extent, kd, Cin, Cout, mode):
    if (quarters + 7) // 8 > 0x3fffffff:
        return "wino43: grid too large"
    if in_extent * 4 >= 1 << 31:
        return "wino43: input tensor exceeds 2^31 bytes"
    if kd * (Cin // 8) * 36 * Cout * 32 >= 1 << 31:
        return "wino43: filter bank exceeds 2^31 bytes"
    nt = 2 if Cout & 63 else 4
    if mode != 0 and (2 * 8 if mode >= 2 else 2) * Cin * 4 + (2 * (28 * 64 * 4) + 2 * 18 * 16 * nt * 8) * 4 > 160 * 1024 - 512:
        return "wino43: affine tables do not fit LDS"
    return None


def parent_f4(segs, mode, kd, Cin, Cout, ws, split_max, gain, chunk_us):
    """w43_run up to the launch."""
    quarters, in_extent, out_elems, geo = parent_quarters(segs, 0)
    blocks = (quarters + 7) // 8
    nt = 2 if Cout & 63 else 4
    why = parent_f4_limits(quarters, in_extent, kd, Cin, Cout, mode)
    if why:
        return why
    nchunks = kd * (Cin // 8)
    grid2 = blocks * (Cout // (16 * nt))
    tile_bytes = float(grid2) * 256 * nt * 32 * 4
    out_bytes = out_elems * Cout * 4
    splits, cps = parent_split(nchunks, grid2, 256, _room(ws), tile_bytes, out_bytes, chunk_us if nt == 4 else 0.55 * chunk_us, 6.0, 2.0, 0.6, gain,
                               split_max)
    return dict(quarters=quarters, in_bytes=in_extent * 4, blocks=blocks, grid2=grid2, nchunks=nchunks, splits=splits, cps=cps, nt=nt, geo=geo,
                tile_bytes=tile_bytes)


# ---- the header, through the shim
def _rows(segs):
    flat = [v for s in segs for v in s]
    return (C.c_int * len(flat))(*flat)


def real_f2(wp, segs, img_mod, D, mm, mode, kd, Cin, Cout, ws, wide, split_max, gain, fix, per):
    out, geo = (C.c_longlong * 10)(), (C.c_longlong * 16)()
    err = wp.wp_f2_plan(_rows(segs), len(segs), img_mod * D if img_mod > 0 else 0, mm, mode, kd, Cin, Cout, int(ws is not None), ws or 0, COUNTER_BYTES,
                        COUNTERS, wide, split_max, gain, fix, per, out, geo)
    if err:
        return err.decode()
    quarters, in_extent, blocks, grid2, nchunks, splits, cps, is_wide, nq, nwn = list(out)
    return dict(quarters=quarters, in_bytes=in_extent * 4, blocks=blocks, grid2=grid2, nchunks=nchunks, splits=splits, cps=cps, wide=is_wide, nq=nq, nwn=nwn,
                geo=[tuple(geo[4 * k:4 * k + 4]) for k in range(len(segs))])


def real_f4(wp, segs, mode, kd, Cin, Cout, ws, split_max, gain, chunk_us):
    out, geo = (C.c_longlong * 8)(), (C.c_longlong * 16)()
    err = wp.wp_f4_plan(_rows(segs), len(segs), mode, kd, Cin, Cout, int(ws is not None), ws or 0, COUNTER_BYTES, COUNTERS, split_max, gain, chunk_us,
                        out, geo)
    if err:
        return err.decode()
    quarters, in_extent, blocks, grid2, nchunks, splits, cps, nt = list(out)
    return dict(quarters=quarters, in_bytes=in_extent * 4, blocks=blocks, grid2=grid2, nchunks=nchunks, splits=splits, cps=cps, nt=nt,
                geo=[tuple(geo[4 * k:4 * k + 4]) for k in range(len(segs))])


def _check_invariants(plan, room, tile_bytes):
    """What the kernels rely on, whatever the model chose."""
    s, cps, n = plan["splits"], plan["cps"], plan["nchunks"]
    assert s * cps >= n > (s - 1) * cps, plan
    if s > 1:
        assert s * tile_bytes <= room and plan["grid2"] <= COUNTERS, plan
    starts = [g[0] for g in plan["geo"]]
    assert all(b > a for a, b in zip(starts, starts[1:])) and starts[0] == 0, plan
    return 1


def _same(want, got, room):
    if isinstance(want, str):
        assert got == want
        return 0
    tile_bytes = want.pop("tile_bytes")
    assert got == want
    return _check_invariants(got, room, tile_bytes)


def _stack(sizes, N, ld_in):
    """Segments of N maps each laid out one behind the other in one buffer."""
    segs, off = [], 0
    for H, W in sizes:
        segs.append((N, H, W, off, ld_in))
        off += N * H * W * ld_in
    return segs


SIZES = (1, 2, 6, 7, 8, 9, 15, 16, 17, 32, 60, 120)
NS = (1, 3, 7, 56, 448)
CINS = (8, 16, 64, 128, 256, 512)
COUTS = (32, 64, 96, 128, 512)
WSS = (None, COUNTER_BYTES, COUNTER_BYTES + 1, 1 << 20, WS_DEFAULT)
# the detector's pyramid as the benchmark runs it (480 x 640 queries at the four detection scales, after conv1 + pool and after every
# further pool of the trunk), 16 queries per launch: (Cin, Cout) of the trunk layers at that level, the pyramid's four sizes
PYRAMID = [((64, 128), [(352, 464), (240, 320), (176, 240), (128, 160)]), ((128, 256), [(176, 232), (120, 160), (88, 120), (64, 80)]),
           ((256, 256), [(176, 232), (120, 160), (88, 120), (64, 80)]), ((256, 512), [(88, 116), (60, 80), (44, 60), (32, 40)]),
           ((512, 512), [(88, 116), (60, 80), (44, 60), (32, 40)]), ((512, 512), [(44, 58), (30, 40), (22, 30), (16, 20)])]


def _sample(seed, n):
    """n seeded launches; the first ones walk every axis value once (the others drawn), the rest are drawn on all axes — the last 300 among
    the launches that may take the wide F(2x2) block (fp32 trunk layers with Cout % 128 == 0), which a uniform draw rarely meets."""
    rng = random.Random(seed)
    axes = dict(H=SIZES, W=SIZES, N=NS, Cin=CINS, Cout=COUTS, kd=(1, 3, 9, 25), mm=(0, 1, 2), mode=(0, 1, 2, 3), wide=(0, 1, 2), nseg=(1, 2, 3, 4), ws=WSS)
    cases = []
    for name, values in axes.items():
        for v in values:
            c = {k: rng.choice(vs) for k, vs in axes.items()}
            c[name] = v
            cases.append(c)
    while len(cases) < n:
        cases.append({k: rng.choice(vs) for k, vs in axes.items()})
    for c in cases[n - 300:]:
        c.update(mm=0, mode=0, kd=1, Cout=rng.choice((128, 512)))
    for c in cases:
        if c["mm"] and c["Cin"] < 16:
            c["Cin"] = 16                                      # (the 16-bit entries need Cin % 16 == 0; mm = 0 keeps Cin = 8 in the sample)
        ld_in = c["Cin"] + rng.choice((0, 0, 4, 64))
        sizes = [(c["H"], c["W"])] + [(rng.choice(SIZES), rng.choice(SIZES)) for _ in range(c["nseg"] - 1)]
        c["segs"] = _stack(sizes, c["N"], ld_in)
        c["img_mod"], c["D"] = rng.choice(((0, 1), (0, 1), (2, 1), (5, 3), (1000, 1)))
    return cases


def test_f2_plan_is_the_parents(wp):
    seen = {k: set() for k in ("H", "W", "N", "Cin", "Cout", "kd", "mm", "mode", "wide", "nseg", "ws")}
    n_ok = n_split = n_wide = 0
    for c in _sample(11, 3000):
        args = (c["segs"], c["img_mod"], c["D"], c["mm"], c["mode"], c["kd"], c["Cin"], c["Cout"], c["ws"], c["wide"], F2_KNOBS["split_max"],
                F2_KNOBS["gain"], F2_KNOBS["fix"], F2_KNOBS["per"])
        want, got = parent_f2(*args), real_f2(wp, *args)
        n_ok += _same(want, got, _room(c["ws"]))
        for k in seen:
            seen[k].add(c[k])
        if not isinstance(got, str):
            n_split += got["splits"] > 1
            n_wide += got["wide"]
    assert seen["H"] == set(SIZES) and seen["W"] == set(SIZES) and seen["N"] == set(NS) and seen["Cin"] == set(CINS) and seen["Cout"] == set(COUTS)
    assert seen["kd"] == {1, 3, 9, 25} and seen["mm"] == {0, 1, 2} and seen["mode"] == {0, 1, 2, 3} and seen["wide"] == {0, 1, 2} and seen["nseg"] == {1, 2, 3, 4}
    assert n_ok > 2900 and n_split > 300 and n_wide > 100, (n_ok, n_split, n_wide)      # (the rest: inputs beyond 2^31 bytes, refused in both)


def test_f4_plan_is_the_parents(wp):
    n_ok = n_split = 0
    for c in _sample(12, 3000):
        args = (c["segs"], min(c["mode"], 2), c["kd"], c["Cin"], c["Cout"], c["ws"], F4_KNOBS["split_max"], F4_KNOBS["gain"], F4_KNOBS["chunk_us"])
        want, got = parent_f4(*args), real_f4(wp, *args)
        n_ok += _same(want, got, _room(c["ws"]))
        n_split += (not isinstance(got, str)) and got["splits"] > 1
    assert n_ok > 2700 and n_split > 300, (n_ok, n_split)      # (the rest: inputs or filter banks beyond 2^31 bytes, mode 2 tables of 512 channels — refused in both)


@pytest.mark.parametrize("knobs", [dict(), dict(split_max=1), dict(split_max=2), dict(gain=1.0), dict(fix=0.0, per=0.0), dict(wide=0), dict(wide=2)],
                         ids=["defaults", "split_max1", "split_max2", "gain1", "free-handoff", "never-wide", "always-wide"])
def test_pyramid_and_crops(wp, knobs):
    """The launches of the benchmark: the detector's four-scale pyramid at 16 queries (trunk layers and the 15x15 / 7x7 correlations on the
    last level), the crops' trunks at 56 / 448 maps, the 32^3 volume layers — with the default workspace and under the model's knobs."""
    k2 = dict(F2_KNOBS, **knobs)
    k4 = dict(F4_KNOBS, **{k: v for k, v in knobs.items() if k in F4_KNOBS})
    launches = [(_stack(sizes, 16, cin), 1, cin, cout, 0) for (cin, cout), sizes in PYRAMID]
    launches += [(_stack(PYRAMID[-1][1], 16, 512), kd, 512, 32, 0) for kd in (25, 9)]
    launches += [(_stack([(s, s)], n, cin), 1, cin, cout, mode) for n in (56, 448) for s, cin, cout in ((64, 64, 128), (32, 128, 256), (16, 256, 512), (8, 512, 512))
                 for mode in (0, 1)]
    launches += [(_stack([(32, 32)], 7 * 32, 64), 3, 64, 64, mode) for mode in (0, 1, 2)]
    n = 0
    for segs, kd, Cin, Cout, mode in launches:
        for mm in (0, 1, 2):
            if kd in (9, 25) and mm:
                continue
            a2 = (segs, 0, 1, mm, mode, kd, Cin, Cout, WS_DEFAULT, k2["wide"], k2["split_max"], k2["gain"], k2["fix"], k2["per"])
            n += _same(parent_f2(*a2), real_f2(wp, *a2), _room(WS_DEFAULT))
        a4 = (segs, mode, kd, Cin, Cout, WS_DEFAULT, k4["split_max"], k4["gain"], k4["chunk_us"])
        n += _same(parent_f4(*a4), real_f4(wp, *a4), _room(WS_DEFAULT))
    assert n > 80
    if knobs.get("split_max") == 1:                            # nothing splits
        assert real_f2(wp, _stack([(8, 8)], 7, 512), 0, 1, 0, 0, 1, 512, 512, WS_DEFAULT, 1, 1, 0.85, 2.0, 0.6)["splits"] == 1


def _split(wp, *a):
    out = (C.c_int * 2)()
    wp.wp_split(*a, out)
    return tuple(out)


def test_split_search_edges(wp):
    """The search on its own: workspace absent / counters only / one tile short of a second split, grids around the counter count and
    around the model's round boundary, chunk lists of 3 and 4 (the search starts at 4), split_max 1."""
    cost = dict(f2=(2.7, 4.0, 2.0, 0.6, 0.85), f2_16=(1.2, 4.0, 2.0, 0.6, 0.85), f4=(2.8, 6.0, 2.0, 0.6, 0.85), f4_nt2=(0.55 * 2.8, 6.0, 2.0, 0.6, 0.85))
    n = n_split = 0
    for (chunk, block, fix, per, gain) in cost.values():
        for grid2 in (1, 7, 64, 255, 256, 257, 511, 512, 513, COUNTERS - 1, COUNTERS, COUNTERS + 1):
            tile = float(grid2) * 256 * 64 * 4
            for nchunks in (1, 2, 3, 4, 5, 8, 9, 63, 64, 75, 200, 1600):
                for room in (0, 1, int(tile), int(2 * tile) - 1, int(2 * tile), int(3 * tile) - 1, int(33 * tile), WS_DEFAULT - COUNTER_BYTES):
                    for split_max in (1, 2, 32):
                        for slots in (256, 512):
                            for out_bytes in (0.0, 4.0 * grid2 * 64 * 64, 4e8):
                                want = parent_split(nchunks, grid2, slots, room, tile, out_bytes, chunk, block, fix, per, gain, split_max)
                                got = _split(wp, nchunks, grid2, slots, room, COUNTERS, tile, out_bytes, chunk, block, fix, per, gain, split_max)
                                assert got == want, (nchunks, grid2, slots, room, split_max, out_bytes)
                                s, cps = got
                                assert s * cps >= nchunks > (s - 1) * cps
                                if s > 1:
                                    assert s * tile <= room and grid2 <= COUNTERS and nchunks >= 4 and split_max > 1
                                if room < 2 * tile or grid2 > COUNTERS or nchunks < 4 or split_max == 1:
                                    assert s == 1
                                n += 1
                                n_split += s > 1
    assert n > 20000 and n_split > 2000, (n, n_split)
    # a small grid with a long chunk list does split once the second tile fits, and not one byte earlier
    tile = 8.0 * 256 * 64 * 4
    assert _split(wp, 64, 8, 256, int(2 * tile) - 1, COUNTERS, tile, 0.0, 2.7, 4.0, 2.0, 0.6, 0.85, 32) == (1, 64)
    assert _split(wp, 64, 8, 256, int(2 * tile), COUNTERS, tile, 0.0, 2.7, 4.0, 2.0, 0.6, 0.85, 32)[0] == 2


def test_plan_edges_through_the_launch_shapes(wp):
    """The same edges reached through whole launches: 8x8 maps (one quarter each) put the block count under the caller's control."""
    n = 0
    for blocks in (255, 256, 257, COUNTERS - 1, COUNTERS, COUNTERS + 1):
        for ws in (None, COUNTER_BYTES, WS_DEFAULT, COUNTER_BYTES + 2 * blocks * 256 * 64 * 4 - 1, COUNTER_BYTES + 2 * blocks * 256 * 64 * 4):
            for Cin in (24, 32, 128):                                  # 3 and 4 chunks of 8, a longer list (the inputs stay below 2 GB)
                a2 = (_stack([(8, 8)], 4 * blocks, Cin), 0, 1, 0, 0, 1, Cin, 64, ws, 1, 32, 0.85, 2.0, 0.6)
                want, got = parent_f2(*a2), real_f2(wp, *a2)
                assert got["blocks"] == blocks and got["grid2"] == blocks
                n += _same(want, got, _room(ws))
                a4 = (_stack([(8, 8)], 8 * blocks, Cin), 0, 1, Cin, 64, ws, 32, 0.85, 2.8)
                want, got = parent_f4(*a4), real_f4(wp, *a4)
                assert got["blocks"] == blocks and got["grid2"] == blocks
                n += _same(want, got, _room(ws))
    assert n == 6 * 5 * 3 * 2
    # img_mod: a query batch that shares 5 x 3 input slices reads only those
    got = real_f2(wp, [(448, 16, 16, 0, 64)], 5, 3, 0, 3, 1, 64, 64, WS_DEFAULT, 1, 32, 0.85, 2.0, 0.6)
    assert got["geo"][0][3] == 15 and got["in_bytes"] == 15 * 16 * 16 * 64 * 4 and got["quarters"] == 448 * 4


def test_errors_in_the_parents_order(wp):
    # grid too large comes before the input extent: 2^33 quarters of 1x1 maps exceed both
    segs = [((1 << 31) - 1, 1, 1, 0, 8)] * 4
    for mm in (0, 1):
        a2 = (segs, 0, 1, mm, 0, 1, 16, 64, WS_DEFAULT, 1, 32, 0.85, 2.0, 0.6)
        assert real_f2(wp, *a2) == parent_f2(*a2) == "wino_conv3x3: grid too large"
    a4 = (segs, 0, 1, 16, 64, WS_DEFAULT, 32, 0.85, 2.8)
    assert real_f4(wp, *a4) == parent_f4(*a4) == "wino43: grid too large"
    # input over 2^31 bytes: an extent of 2^29 floats is refused, one vector of four floats less passes
    for in_off, want2, want4 in (((1 << 29) - (1 << 19), "wino_conv3x3: input tensor exceeds 2^31 bytes", "wino43: input tensor exceeds 2^31 bytes"),
                                 ((1 << 29) - (1 << 19) - 4, None, None)):
        segs = [(7, 8, 8, 0, 512), (1, 32, 32, in_off, 512)]
        a2 = (segs, 0, 1, 0, 0, 1, 512, 64, WS_DEFAULT, 1, 32, 0.85, 2.0, 0.6)
        got, want = real_f2(wp, *a2), parent_f2(*a2)
        assert (got if isinstance(got, str) else None) == want2 and (want if isinstance(want, str) else None) == want2
        a4 = (segs, 0, 1, 512, 64, WS_DEFAULT, 32, 0.85, 2.8)
        got, want = real_f4(wp, *a4), parent_f4(*a4)
        assert (got if isinstance(got, str) else None) == want4 and (want if isinstance(want, str) else None) == want4
    # F(4x4) limits one by one, in order: every earlier cause hides the later ones
    cases = [((1 << 34, 1 << 29, 25, 1 << 20, 512, 2), "wino43: grid too large"), ((8, 1 << 29, 25, 1 << 20, 512, 2), "wino43: input tensor exceeds 2^31 bytes"),
             ((8, 1 << 20, 25, 1 << 20, 512, 2), "wino43: filter bank exceeds 2^31 bytes"), ((8, 1 << 20, 1, 4096, 64, 2), "wino43: affine tables do not fit LDS"),
             ((8, 1 << 20, 25, 512, 1152, 0), None), ((8, 1 << 20, 25, 512, 1216, 0), "wino43: filter bank exceeds 2^31 bytes")]
    for args, want in cases:
        got = wp.wp_f4_limits(*args)
        assert (got.decode() if got else None) == want == parent_f4_limits(*args), args
    for mode in (1, 2):                                               # the table limit, channel by channel around it
        for Cin in range(8, 4097, 8):
            got = wp.wp_f4_limits(8, 1 << 20, 1, Cin, 64, mode)
            assert (got.decode() if got else None) == parent_f4_limits(8, 1 << 20, 1, Cin, 64, mode)
    # the 16-bit kernels: channel width first, then the tables of the block's four quarters beside the two stages
    def parent_w16(nwn, mode, Cin):
        if nwn != 2:
            return "wino16: Cout % 64 == 0 expected"
        stage16 = 2 * (4 * 101 * 8) + 16 * 64 * 8 + 4 * 256
        lds16 = (2 * stage16 + (0 if mode == 0 else (8 if mode >= 2 else 2) * Cin)) * 4
        return "wino16: affine tables do not fit LDS" if lds16 > 160 * 1024 else None
    n_refused = 0
    for Cout in (32, 64, 96, 128, 512):
        nwn = 1 if Cout & 63 else 2                                   # (the 16-bit launches are never wide)
        for mode in (0, 1, 2, 3):
            for Cin in list(range(16, 1025, 16)) + [1024, 1040, 1200, 1216, 4800, 4816]:
                got = wp.wp_w16_limits(Cout, mode, Cin)
                assert (got.decode() if got else None) == parent_w16(nwn, mode, Cin), (Cout, mode, Cin)
                n_refused += got is not None and nwn == 2
    assert n_refused == 3 * 2 * 3 + 3                                # modes 2 / 3 from 1216 channels on, mode 1 at 4816
    for mode in (2, 3):
        assert wp.wp_w16_limits(64, mode, 1024) is None and wp.wp_w16_limits(64, mode, 1040) is None     # g6d_wino_eligible's cap fits


def test_lds_sizes(wp):
    """Every launched instantiation's dynamic LDS against the sum its launcher spelled out."""
    for Cin in (8, 16, 64, 256, 1024):
        for mode in (0, 1, 2, 3):
            for nwn, nwm in ((1, 2), (2, 2), (4, 1)):
                want = (2 * (2 * nwm * 101 * 8 + 16 * 32 * nwn * 8 + 4 * (64 * nwm * nwn)) + (0 if mode == 0 else (4 * nwm if mode >= 2 else 2) * Cin + Cin)) * 4
                assert wp.wp_lds(0, mode, nwn, nwm, Cin) == want
            assert wp.wp_lds(1, mode, 0, 0, Cin) == (2 * (2 * 3232 + 16 * 64 * 8 + 4 * 256) + (0 if mode == 0 else (8 if mode >= 2 else 2) * Cin)) * 4
            for nt in (2, 4):
                assert wp.wp_lds(3, min(mode, 2), nt, 0, Cin) == (2 * (28 * 64 * 4) + 2 * (18 * 16 * nt * 8) + (0 if mode == 0 else (16 if mode >= 2 else 2) * Cin)) * 4
    assert wp.wp_lds(2, 0, 0, 0, 0) == (2 * 3232 + 4 * 16 * 64 * 8 + 256) * 4 == 157952
    assert wp.wp_lds(1, 0, 0, 0, 0) == 125440 and wp.wp_lds(0, 0, 2, 2, 0) == 99584 and wp.wp_lds(3, 0, 4, 0, 0) == 131072


def test_table_copy(wp):
    rows = [(16, 352, 464, 64, 128, 128, 0, 0, 0), (16, 240, 320, 64, 128, 128, 167247872, 334495744, 83623936), (3, 7, 9, 72, 200, 136, 5, 6, 7),
            (1, 2, 2, 8, 64, 64, 11, 12, 13)]
    for nseg in (1, 2, 3, 4):
        flat = [v for r in rows[:nseg] for v in r]
        out = (C.c_int * 48)()
        assert wp.wp_segments((C.c_int * len(flat))(*flat), nseg, out) == nseg
        for k, (N, H, W, ld_in, ld_full, ld_pool, in_off, full_off, pool_off) in enumerate(rows[:nseg]):
            assert tuple(out[12 * k:12 * k + 12]) == (0, N, H, W, 0, 0, in_off, full_off, pool_off, ld_in, ld_full, ld_pool)


def test_plan_under_sanitizers(tmp_path):
    """The plan is host code the launchers run on caller-supplied sizes: a stand-alone program (no Python in the process) walks it over the
    same axes and over extreme shapes, built with the address and undefined-behaviour sanitizers, and checks the invariants."""
    exe = str(tmp_path / "wplan_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "wino_plan_sanitize.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 broken" in r.stdout, r.stdout[-2000:]
