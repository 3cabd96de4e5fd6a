"""The halo-patch kernel's integer geometry (gen6d_amd/csrc/conv16w_geom.h: tile index -> tile, (piece, lane) -> patch pixel / validity /
32-bit offset, tile pixel -> fragment base, all without run-time division), built for the host (tests/conv16w_geom_shim.cpp) and compared
with the plain-division formulas the kernel used before, written out here with // and %.  Exhaustive over the tile widths 4 / 8 / 16 / 32,
bands of 1 .. 32 rows and maps at least a tile high, every piece index a wave can hold and every lane, and every tile index of the
headline launches (5120 maps of 16x16 for Cout = 64, the pyramid of 16 queries).  The launcher's own choice of tile width, bands and slot
swizzle (c16g::halo_tiling in the same header) is called through the shim and compared with the Python model below.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BM, NPIECE = 128, 20                       # pixels per tile; piece indices wv + 4 j, wv < 4, j < 5
I32 = C.POINTER(C.c_int)
U32 = C.POINTER(C.c_uint)


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("c16g") / "conv16w_geom.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "conv16w_geom_shim.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.g_tiling.argtypes = [C.c_int] * 7 + [C.c_long, C.c_void_p]
    lib.g_tiles.argtypes = [C.c_void_p] + [C.c_int] * 4 + [I32]
    lib.g_pieces.argtypes = [C.c_void_p] + [C.c_int] * 6 + [I32]
    lib.g_frag.argtypes = [C.c_void_p, I32]
    lib.g_patch_pixels.argtypes = [C.c_void_p]
    lib.g_halo_tiling.argtypes = [C.c_int] * 5 + [C.c_void_p, I32]
    lib.g_div31.argtypes = [U32, U32, C.c_int, U32, I32]
    lib.g_div16.argtypes = [U32, U32, C.c_int, U32]
    return lib


class Tiling:
    """One segment (N maps of H x W) tiled with tiles of width tw, as c16g::halo_tiling lays it out; fits: that width is admissible
    (in_image: only with tiles inside one image)."""

    def __init__(self, N, H, W, tw, pairs=True, in_image=False):
        th = BM // tw
        self.N, self.H, self.W, self.tw, self.th = N, H, W, tw, th
        self.tiles_x = -(-W // tw)
        if H >= th:
            self.tpi = self.tiles_x * -(-H // th)
            self.ntiles, self.segh, self.bands = N * self.tpi, th, 1
        else:
            self.tpi = 0
            self.ntiles, self.segh, self.bands = self.tiles_x * -(-(N * H) // th), H, th // H
        self.fits = (H >= th or (th % H == 0 and not in_image)) and self.bands * (self.segh + 2) * (tw + 2) <= 288
        if pairs:
            self.swa, self.swd = (1 if tw >= 16 else 0), 0
        else:
            self.swa, self.swd = (2 if tw == 32 else (1 if tw == 16 else 0)), (1 if tw <= 8 else 0)
        self.PW, self.bandr = tw + 2, self.segh + 2
        self.P = self.bands * self.bandr * self.PW
        self.rows = N * H

    def make(self, geo):
        buf = C.create_string_buffer(geo.g_sizeof_tiling())
        ok = geo.g_tiling(self.tw.bit_length() - 1, self.tiles_x, self.tpi, self.segh.bit_length() - 1, self.bands, self.swa, self.swd, self.ntiles, buf)
        assert geo.g_patch_pixels(buf) == self.P
        return buf, bool(ok)

    def ref_tiles(self, t):
        """Plain-division tile geometry for an array of tile indices -> g0, x0, y0, ylim."""
        if self.tpi > 0:
            n, r = t // self.tpi, t % self.tpi
            ty, tx = r // self.tiles_x, r % self.tiles_x
            y0 = ty * self.th
            return n * self.H + y0, tx * self.tw, y0, np.minimum(self.th, self.H - y0)
        ty, tx = t // self.tiles_x, t % self.tiles_x
        return ty * self.th, tx * self.tw, 0 * t, 0 * t + self.th


def halo_tiling(N, H, W, pairs=True, in_image=False):
    """The independent model of c16g::halo_tiling's choice: the width with the least overhang, ties to the wider tile."""
    best, res = 1e30, None
    for tw in (32, 16, 8, 4):
        t = Tiling(N, H, W, tw, pairs, in_image)
        if not t.fits:
            continue
        waste = t.ntiles * BM / (N * H * W)
        if waste < best - 1e-9:
            best, res = waste, t
    return res


def _check_tiles(geo, tl, buf):
    out = np.zeros((tl.ntiles, 5), np.int32)
    geo.g_tiles(buf, tl.H, tl.W, 0, tl.ntiles, out.ctypes.data_as(I32))
    t = np.arange(tl.ntiles, dtype=np.int64)
    g0, x0, y0, ylim = tl.ref_tiles(t)
    for k, want in enumerate((g0, x0, y0, ylim)):
        assert np.array_equal(out[:, k], want), (tl.N, tl.H, tl.W, tl.tw, k)
    return out


def _check_pieces(geo, tl, buf, tiles, ld_in, which):
    """Every (piece, lane) of the tiles `which` against the plain formulas; returns the number of interior tiles seen."""
    ii = np.arange(NPIECE, dtype=np.int64)[:, None]
    lane = np.arange(64, dtype=np.int64)[None, :]
    q = ii * 16 + (lane >> 2)
    prow, pcol = q // tl.PW, q % tl.PW
    band = prow // tl.bandr
    lr = prow - band * tl.bandr - 1
    slot = (lane & 3) ^ (((pcol >> tl.swa) + prow * tl.swd) & 3)
    in_patch = q < tl.P
    out = np.zeros((NPIECE, 64, 8), np.int32)
    n_int = 0
    for t in which:
        g0, x0, y0, _, interior = (int(v) for v in tiles[t])
        geo.g_pieces(buf, tl.H, tl.W, tl.rows, ld_in, int(t), NPIECE, out.ctypes.data_as(I32))
        g, x, yimg = g0 + band * tl.segh + lr, x0 + pcol - 1, y0 + lr
        ok = in_patch & (yimg >= 0) & (yimg < tl.H) & (g < tl.rows) & (x >= 0) & (x < tl.W)
        off = ((g * tl.W + x) * ld_in) * 2 + slot * 16
        for k, want in enumerate((prow, pcol, band, lr, slot, in_patch, ok)):
            assert np.array_equal(out[..., k], want + 0 * q), (tl.H, tl.W, tl.tw, t, k)
        # the 32-bit offset: the old 64-bit value truncated; exact (and inside the 2 GB a launch may address) wherever it is requested
        assert np.array_equal(out[..., 7].astype(np.int64) & 0xFFFFFFFF, off & 0xFFFFFFFF), (tl.H, tl.W, tl.tw, t)
        assert np.array_equal(out[..., 7][ok], off[ok]) and (off[ok] >= 0).all() and (off[ok] < 2 ** 31).all()
        if interior:                                           # interior => every lane of every piece that lies in the patch is valid
            n_int += 1
            assert np.array_equal(ok, in_patch), (tl.H, tl.W, tl.tw, t)
        # (what the kernel relies on: a piece below ni = ceil(P / 16) has a lane in the patch, pieces from ni on have none)
        ni = (tl.P + 15) >> 4
        assert in_patch[:ni].any(1).all() and not in_patch[ni:].any()
    return n_int


def _check_frag(geo, tl, buf):
    out = np.zeros((BM, 2), np.int32)
    geo.g_frag(buf, out.ctypes.data_as(I32))
    r = np.arange(BM)
    py, px = r // tl.tw, r % tl.tw
    b, ly = py // tl.segh, py % tl.segh
    assert np.array_equal(out[:, 1], b * tl.bandr + ly)
    assert np.array_equal(out[:, 0], (b * tl.bandr + ly) * tl.PW + px)


def test_layouts_exhaustive(geo):
    """Every tile width x (banded forms of 1 .. 32 rows, maps of one tile row and more, ragged and exact widths): all tiles, pieces, lanes."""
    n_tilings = n_interior = 0
    for pairs in (True, False):
        for tw in (4, 8, 16, 32):
            th = BM // tw
            heights = [h for h in (1, 2, 4, 8, 16, 32) if h < th] + [th, th + 1, 2 * th + 3, 3 * th, 4 * th - 1]
            for H in heights:
                for W in (tw, tw + 1, 3 * tw - 1, 3 * tw, 3 * tw + 2):
                    for N in (1, 5):
                        tl = Tiling(N, H, W, tw, pairs)
                        if not tl.fits:
                            continue
                        buf, ok = tl.make(geo)
                        assert ok
                        tiles = _check_tiles(geo, tl, buf)
                        n_interior += _check_pieces(geo, tl, buf, tiles, 2 * 64 if pairs else 64, range(tl.ntiles))
                        _check_frag(geo, tl, buf)
                        n_tilings += 1
    assert n_tilings > 300 and n_interior > 50
    # the interior rule itself: a map of 3 x 3 whole tiles has exactly one interior tile per image, ragged or not
    for tw in (4, 8, 16, 32):
        th = BM // tw
        tl = Tiling(2, 3 * th, 3 * tw, tw)
        tiles = _check_tiles(geo, tl, tl.make(geo)[0])
        assert tiles[:, 4].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0] * 2
        tl = Tiling(1, 3 * th - 1, 3 * tw - 1, tw)                   # the centre tile's halo still ends inside the map
        assert _check_tiles(geo, tl, tl.make(geo)[0])[:, 4].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
        tl = Tiling(1, 2 * th + 1, 2 * tw + 1, tw)                   # second tile row / column: halo row 2 TH, the last one
        assert _check_tiles(geo, tl, tl.make(geo)[0])[4, 4] == 1
        tl = Tiling(1, 2 * th, 2 * tw, tw)
        assert not _check_tiles(geo, tl, tl.make(geo)[0])[:, 4].any()


def _real_choice(geo, N, H, W, pairs, in_image):
    """c16g::halo_tiling itself (the function the launcher calls): None, or its tiling as a dict and the buffer it filled."""
    buf = C.create_string_buffer(geo.g_sizeof_tiling())
    out = np.zeros(8, np.int32)
    if not geo.g_halo_tiling(N, H, W, int(pairs), int(in_image), buf, out.ctypes.data_as(I32)):
        return None, buf
    keys = ("tw_log2", "tiles_x", "tpi", "segh_log2", "bands", "swa", "swd", "tiles")
    return dict(zip(keys, out.tolist())), buf


def _assert_choice_matches_model(geo, N, H, W, pairs, in_image):
    got, buf = _real_choice(geo, N, H, W, pairs, in_image)
    want = halo_tiling(N, H, W, pairs, in_image)
    # fits: the real function finds a tiling exactly where the model has a width that fits
    assert (got is not None) == (want is not None), (N, H, W, pairs, in_image)
    if want is None:
        return 0
    assert got == dict(tw_log2=want.tw.bit_length() - 1, tiles_x=want.tiles_x, tpi=want.tpi, segh_log2=want.segh.bit_length() - 1, bands=want.bands,
                       swa=want.swa, swd=want.swd, tiles=want.ntiles), (N, H, W, pairs, in_image)
    assert 1 << got["segh_log2"] == want.segh and geo.g_patch_pixels(buf) == want.P
    if in_image:
        assert got["tpi"] > 0 and got["bands"] == 1
    return 1


def test_real_chooser_matches_model(geo):
    """The launcher's tiling choice (c16g::halo_tiling, through the shim) against the Python model above, over the shape set of
    test_layouts_exhaustive and the headline shapes: width, bands, rows per band, tiles, swizzle, fits — pair and 16-bit mode, with and
    without in_image."""
    shapes = set(HEADLINE)
    for tw in (4, 8, 16, 32):
        th = BM // tw
        heights = [h for h in (1, 2, 4, 8, 16, 32) if h < th] + [th, th + 1, 2 * th + 3, 3 * th, 4 * th - 1]
        shapes |= {(N, H, W) for H in heights for W in (tw, tw + 1, 3 * tw - 1, 3 * tw, 3 * tw + 2) for N in (1, 5)}
    shapes |= {(3, H, 8) for H in (3, 5, 6, 7, 12)}            # heights that divide no tile: banded forms must not be chosen
    n = {}
    for pairs in (True, False):
        for in_image in (False, True):
            n[pairs, in_image] = sum(_assert_choice_matches_model(geo, N, H, W, pairs, in_image) for N, H, W in sorted(shapes))
    assert min(n.values()) > 250 and n[True, False] > n[True, True], n   # (in_image turns the banded tilings away)


def test_choosers_under_sanitizers(tmp_path):
    """The choosers are host code the launcher runs on caller-supplied sizes: a stand-alone program (no Python in the process) walks them
    over small shapes exhaustively and over the extremes a launch admits, built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "geom_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "conv16w_geom_sanitize.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 broken" in r.stdout, r.stdout[-2000:]


HEADLINE = [
    # the selector's level-0 stack at 16 queries (5120 hypothesis maps; Cout = 64 takes the two-tile form) and its lower levels
    (5120, 16, 16), (5120, 8, 8), (5120, 4, 4),
    # the detector's pyramid of 16 queries of 480 x 640 at 1/2 .. 1/64 resolution
    (16, 352, 464), (16, 240, 320), (16, 176, 240), (16, 128, 160), (16, 88, 116), (16, 44, 58), (16, 22, 30), (16, 11, 15), (16, 8, 10),
    # the refiner's crops
    (112, 128, 128), (112, 64, 64), (112, 32, 32), (112, 16, 16), (112, 8, 8),
]


@pytest.mark.parametrize("shape", HEADLINE, ids=["x".join(map(str, s)) for s in HEADLINE])
def test_headline_tile_indices(geo, shape):
    """Every tile index of the headline launches decomposes as with plain division (the reciprocals are exact over the whole range), in both
    arithmetics' tilings; pieces and lanes of the first, last and a spread of tiles."""
    for pairs in (True, False):
        tl = halo_tiling(*shape, pairs=pairs)
        if tl is None:
            continue
        buf, ok = tl.make(geo)
        assert ok, "a reciprocal is not exact over the launch's tile indices"
        tiles = _check_tiles(geo, tl, buf)
        ld_in = 2 * 64 if pairs else 64
        assert tl.rows * tl.W * ld_in * 2 < 2 ** 31
        which = sorted(set(np.linspace(0, tl.ntiles - 1, 40).astype(int).tolist() + list(range(min(tl.ntiles, 20)))))
        _check_pieces(geo, tl, buf, tiles, ld_in, which)


def test_reciprocal_helpers(geo):
    rng = np.random.default_rng(5)
    # div31: wherever recip31_ok holds the quotient is exact, and it holds at least whenever n d <= 2^31
    d = np.concatenate([np.arange(1, 4097), rng.integers(1, 2 ** 20, 20000), 2 ** np.arange(0, 31), [2 ** 31 - 1, 46341, 65535, 65537]]).astype(np.int64)
    parts_n, parts_d = [], []
    for scale in (2 ** 31 - 1, 2 ** 24, 2 ** 16):
        parts_n.append(rng.integers(0, scale, len(d))); parts_d.append(d)
    for k in (-1, 0, 1):                                        # multiples of d and their neighbours, up to the n d <= 2^31 bound
        m = np.minimum(2 ** 31 // d, rng.integers(1, 2 ** 20, len(d)))
        parts_n.append(np.clip(m * d + k, 0, 2 ** 31 - 1)); parts_d.append(d)
        parts_n.append(np.clip((2 ** 31 // (d * d)) * d + k, 0, 2 ** 31 - 1)); parts_d.append(d)
    n = np.concatenate(parts_n).astype(np.uint32)
    dd = np.concatenate(parts_d).astype(np.uint32)
    q = np.zeros(len(n), np.uint32)
    ok = np.zeros(len(n), np.int32)
    geo.g_div31(n.ctypes.data_as(U32), dd.ctypes.data_as(U32), len(n), q.ctypes.data_as(U32), ok.ctypes.data_as(I32))
    n64, d64 = n.astype(np.int64), dd.astype(np.int64)
    assert np.array_equal(q[ok == 1].astype(np.int64), (n64 // d64)[ok == 1])
    small = n64 * d64 <= 2 ** 31
    assert small.sum() > 50000 and (ok[small] == 1).all()
    # div16: exhaustive over its whole domain (patch pixels and rows below 512, patch widths / band heights 2 .. 64)
    nn, d2 = np.meshgrid(np.arange(512, dtype=np.uint32), np.arange(2, 65, dtype=np.uint32))
    nn, d2 = np.ascontiguousarray(nn.ravel()), np.ascontiguousarray(d2.ravel())
    q2 = np.zeros(len(nn), np.uint32)
    geo.g_div16(nn.ctypes.data_as(U32), d2.ctypes.data_as(U32), len(nn), q2.ctypes.data_as(U32))
    assert np.array_equal(q2, nn // d2)
