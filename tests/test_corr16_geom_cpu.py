"""corr16_kernel's integer geometry (gen6d_amd/csrc/corr16_geom.h: tile choice, tile index -> tile, (piece, lane) -> patch pixel / validity /
logical slot, tile pixel and tap -> fragment address, the waves' tap walk and the running filter pointer), built for the host
(tests/corr16_geom_shim.cpp) and compared with the plain formulas, written out here with // and %.  Exhaustive over K = 7 / 15, every tile
width whose patch fits a stage, both arithmetics, every piece, lane, tile pixel, tap, lane half and fragment.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_conv16w_shape_cpu import GROUPS      # the 16-lane groups of a ds_read_b128

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = C.POINTER(C.c_int)
BM, NW, STAGE, PIECE, NPL, TAP_BYTES, RING = 128, 11, 42 * 1024, 1024, 42, 2048, 3
WIDTHS = {7: (32, 16, 8, 4), 15: (16, 8)}      # the widths whose (128 / tw + K - 1) x (tw + K - 1) patch fits STAGE / 64 = 672 rows


def swizzle(tw):
    """(swa, swd) of a tile width: the fill puts logical slot s ^ (((pcol >> swa) + prow * swd) & 3) into physical slot s."""
    return (2 if tw == 32 else 1 if tw == 16 else 0), (1 if tw <= 8 else 0)


def layouts():
    for K, widths in WIDTHS.items():
        for tw in widths:
            yield K, tw, (tw.bit_length() - 1, K) + swizzle(tw)


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("corr16g") / "corr16_geom.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "corr16_geom_shim.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.g_pick_grid.argtypes = [C.c_int] * 3 + [I32]
    lib.g_patch.argtypes = [C.c_int] * 4 + [I32]
    lib.g_origins.argtypes = [C.c_int] * 7 + [I32]
    lib.g_pieces.argtypes = [C.c_int] * 10 + [I32]
    lib.g_taps.argtypes = [C.c_int] * 5 + [I32]
    lib.g_walk.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_long), I32, I32, I32]
    return lib


def _patch(geo, g):
    o = (C.c_int * 3)()
    geo.g_patch(*g, o)
    return tuple(o)                           # PW, P, NI


def _pieces(geo, g, y0, x0, H, W, pairs, Cin):
    out = np.zeros((NPL, 64, 8), np.int32)
    geo.g_pieces(*g, y0, x0, H, W, int(pairs), Cin, out.ctypes.data_as(I32))
    return out


def _check_pieces(geo, K, tw, g, y0, x0, H, W, pairs, Cin):
    """Every (piece, lane) of one tile against the plain formulas; returns (in_patch, requested, y, x)."""
    th, R, (swa, swd) = BM // tw, K // 2, swizzle(tw)
    PW, P = tw + K - 1, (th + K - 1) * (tw + K - 1)
    NI = -(-P // 16)
    assert _patch(geo, g) == (PW, P, NI) and NI <= NPL and P * 64 <= STAGE
    k = np.arange(NPL)[:, None]
    lane = np.arange(64)[None, :]
    q = k * 16 + lane // 4
    prow, pcol = q // PW, q % PW
    y, x = y0 - R + prow, x0 - R + pcol
    L = (lane % 4) ^ (((pcol >> swa) + prow * swd) % 4)
    in_patch = (k < NI) & (q < P)
    inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    within = (L // 2) * Cin * 2 + (L % 2) * 16 if pairs else 16 * L
    out = _pieces(geo, g, y0, x0, H, W, pairs, Cin)
    for i, want in enumerate((prow, pcol, y, x, L, in_patch, inside, within)):
        assert np.array_equal(out[..., i], want + 0 * q), (K, tw, i)
    return in_patch, in_patch & inside, y, x


def test_constants(geo):
    o = (C.c_int * 8)()
    geo.g_consts(o)
    assert tuple(o) == (BM, NW, STAGE, PIECE, NPL, TAP_BYTES, RING, 2 * STAGE)
    assert 4 * BM * 33 * 4 <= 2 * STAGE                        # the final reduction's four partial tiles
    for K in (7, 15):                                          # WIDTHS is the fit rule
        assert WIDTHS[K] == tuple(tw for tw in (32, 16, 8, 4) if (BM // tw + K - 1) * (tw + K - 1) <= STAGE // 64)
    assert all(not (swizzle(tw)[1] and swizzle(tw)[0]) for tw in (32, 16, 8, 4))      # swd = 1 => swa = 0: the reader's precondition


@pytest.mark.parametrize("pairs", [False, True], ids=["16bit", "pairs"])
def test_loader_coverage(geo, pairs):
    """(a) Every patch pixel is requested by exactly one (piece, lane quad), whose four lanes carry the four logical slots; pieces from NI on
    request nothing."""
    for K, tw, g in layouts():
        in_patch, req, _, _ = _check_pieces(geo, K, tw, g, 500, 500, 1000, 1000, pairs, 96)
        assert np.array_equal(req, in_patch)                   # a tile deep inside the map: the whole patch is requested
        PW, P, NI = _patch(geo, g)
        out = _pieces(geo, g, 500, 500, 1000, 1000, pairs, 96)
        pix = out[..., 0] * PW + out[..., 1]
        quads = pix[in_patch].reshape(-1, 4)
        assert (quads == quads[:, :1]).all() and np.array_equal(np.sort(quads[:, 0]), np.arange(P))
        assert (np.sort(out[..., 4][in_patch].reshape(-1, 4), axis=1) == np.arange(4)).all()
        assert in_patch[:NI].any(1).all() and not in_patch[NI:].any()
        if pairs:                                              # plane L >> 1 (Cin 16-bit values), channel half L & 1
            assert set(out[..., 7][in_patch].tolist()) == {0, 16, 192, 208}


def _tap_addresses(geo, K, tw, g, stage):
    out = np.zeros((K, K, 2, BM), np.int32)
    geo.g_taps(*g, stage, out.ctypes.data_as(I32))
    return out


def test_fragment_slots(geo):
    """(b) For every tile pixel, tap, lane half and fragment the address read lies in patch pixel (py + ky, px + kx) of the stage and holds
    logical slot half ^ 2 * fragment under the loader's swizzle."""
    for K, tw, g in layouts():
        (swa, swd), PW = swizzle(tw), tw + K - 1
        r = np.arange(BM)[None, None, None, :]
        ky = np.arange(K)[:, None, None, None]
        kx = np.arange(K)[None, :, None, None]
        half = np.arange(2)[None, None, :, None]
        prow, pcol = r // tw + ky, r % tw + kx
        for stage in (0, 1):
            a0 = _tap_addresses(geo, K, tw, g, stage)
            for frag in (0, 1):
                a = (a0 ^ (32 * frag)) - stage * STAGE
                assert (a % 16 == 0).all() and np.array_equal(a // 64, prow * PW + pcol + 0 * half), (K, tw, stage, frag)
                phys = a % 64 // 16
                assert np.array_equal(phys ^ (((pcol >> swa) + prow * swd) % 4), (half ^ (2 * frag)) + 0 * a), (K, tw, stage, frag)


def test_bank_conflicts(geo):
    """(c) Every 16-lane group of a ds_read_b128 (lane l: tile pixel 32 mt + (l & 31), half l >> 5) covers 16 distinct 16-byte bank slots."""
    lanes = np.array(GROUPS)                                   # [4][16]
    for K, tw, g in layouts():
        a0 = _tap_addresses(geo, K, tw, g, 1)
        for mt in range(4):
            for frag in (0, 1):
                a = a0[:, :, lanes >> 5, 32 * mt + (lanes & 31)] ^ (32 * frag)        # [K][K][4][16]
                slots = np.sort(a // 16 % 16, axis=-1)
                assert (slots == np.arange(16)).all(), (K, tw, mt, frag)


@pytest.mark.parametrize("nslice", [1, 2, 3, 7])
def test_tap_dealing(geo, nslice):
    """(d) The waves' tap sequences partition range(K^2) in every slice, the filter pointer stands at (slice K^2 + tap) * 2048 before each
    load, and the steps are padded to a multiple of three (their loads re-read the base)."""
    for K in (7, 15):
        T = K * K
        seen = []
        for wv in range(NW):
            off = (C.c_long * (nslice * T + 8))()
            tap = (C.c_int * (nslice * T))()
            ntaps, ntw = C.c_int(), C.c_int()
            nl = geo.g_walk(K, wv, nslice, off, tap, C.byref(ntaps), C.byref(ntw))
            mine = list(range(wv, T, NW))
            assert ntw.value == len(mine) and ntaps.value == nslice * len(mine)
            assert list(tap[:ntaps.value]) == mine * nslice
            steps = -(-ntaps.value // RING) * RING
            assert nl == 2 + steps
            want = [(c * T + t) * TAP_BYTES for c in range(nslice) for t in mine]
            assert list(off[:nl]) == want + [-1] * (nl - len(want))
            seen += mine
        assert sorted(seen) == list(range(T))


def pick_plain(H, W, K):
    """The launcher's search restated: widths 32 .. 4 whose patch fits, least overhang, ties to the wider tile."""
    best, btw = 1e30, 0
    for tw in (32, 16, 8, 4):
        th = BM // tw
        if (th + K - 1) * (tw + K - 1) > STAGE // 64:
            continue
        waste = float(-(-W // tw) * tw) * (-(-H // th) * th) / (float(W) * H)
        if waste < best - 1e-9:
            best, btw = waste, tw
    return btw


def test_pick_tile(geo):
    """(e) pick_tile equals the restatement for H, W in 1 .. 199 and always finds a tile."""
    for K in (7, 15):
        out = np.zeros((199, 199, 5), np.int32)
        geo.g_pick_grid(K, 199, 199, out.ctypes.data_as(I32))
        used = set()
        for H in range(1, 200):
            for W in range(1, 200):
                tw = pick_plain(H, W, K)
                assert tw in WIDTHS[K]
                tx = -(-W // tw)
                assert tuple(out[H - 1, W - 1]) == (tw.bit_length() - 1, tx, tx * -(-H // (BM // tw))) + swizzle(tw), (K, H, W)
                used.add(tw)
        assert used == set(WIDTHS[K])


RAGGED = [(3, 31), (7, 15), (15, 7), (31, 3), (9, 13), (22, 30), (1, 1), (33, 17), (5, 70)]


@pytest.mark.parametrize("K", [7, 15])
def test_ragged_tiles(geo, K):
    """(e) Tile index -> (image, row, column) by plain division, and on every tile of ragged maps a request is made for exactly the patch pixels
    that lie in the map: none outside it, none of them missed."""
    for H, W in RAGGED:
        tw = pick_plain(H, W, K)
        th, g = BM // tw, (tw.bit_length() - 1, K) + swizzle(tw)
        tiles_x, tiles_y = -(-W // tw), -(-H // th)
        tpi, N = tiles_x * tiles_y, 3
        org = np.zeros((N * tpi, 3), np.int32)
        geo.g_origins(*g, tiles_x, tpi, N * tpi, org.ctypes.data_as(I32))
        t = np.arange(N * tpi)
        assert np.array_equal(org, np.stack([t // tpi, t % tpi // tiles_x * th, t % tpi % tiles_x * tw], 1))
        for _, y0, x0 in org[:tpi]:
            _, req, y, x = _check_pieces(geo, K, tw, g, int(y0), int(x0), H, W, True, 96)
            assert ((y[req] >= 0) & (y[req] < H) & (x[req] >= 0) & (x[req] < W)).all()
            quad = req[:, ::4]                                     # (one lane of each quad: the four share their pixel)
            got = set(zip(y[:, ::4][quad].tolist(), x[:, ::4][quad].tolist()))
            R = K // 2
            want = {(yy, xx) for yy in range(max(0, y0 - R), min(H, y0 + th + R)) for xx in range(max(0, x0 - R), min(W, x0 + tw + R))}
            assert got == want, (K, H, W, y0, x0)


def test_kernel_uses_the_header():
    """(f) corr16.hip holds no second copy of the swizzle, the fit rule, the tile search or the tap dealing: it calls the header."""
    src = open(os.path.join(ROOT, "gen6d_amd", "csrc", "corr16.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.split("\n"))
    assert '#include "corr16_geom.h"' in code
    for pattern in (r">>\s*\(?\s*\w*\.?swa", r"\*\s*\w*\.?swd", r"STAGE\s*/\s*64", r"waste", r"/\s*\w*\.?PW\b", r"\+\s*NW\s*-\s*1\s*\)\s*/", r"\^\s*sw\b", r"\bwv\s*/\s*K\b"):
        assert not re.search(pattern, code), pattern
    for call in ("pick_tile", "patch_of", "tile_origin", "piece_of", "in_map", "slot_bytes", "frag_base", "tap_addr", "wave_taps", "first_tap", "next_tap",
                 "filter_advance"):
        assert re.search(r"\bcg::%s\(" % call, code), call
