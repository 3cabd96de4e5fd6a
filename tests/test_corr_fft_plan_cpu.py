"""The integer plan of the frequency-domain correlation (gen6d_amd/csrc/corr_fft_plan.h), built for the host (tests/corr_fft_plan_shim.cpp)
and compared with plain formulas: every output pixel of every map up to 120 x 120 in exactly one tile's valid corner, window origins, bin
count, buffer sizes and the query chunk against the 2^31-byte limit; the float64 numpy restatement of the whole route
(tests/corr_fft_ref.py) against float64 conv2d; the header once under the address and undefined-behaviour sanitizers in a stand-alone
program.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import corr_fft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "corr_fft_plan_shim.cpp")
I32 = C.POINTER(C.c_int)
K = 15


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cfft") / "corr_fft_plan.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.p_plan.argtypes = [C.c_int] * 3 + [I32] * 4
    lib.p_tiles.argtypes = [C.c_int] * 3 + [I32] * 4
    lib.p_chunk.argtypes = [C.c_int] * 4
    for f in (lib.p_spectrum_bytes, lib.p_product_bytes, lib.p_filter_bytes):
        f.restype = C.c_longlong
    lib.p_spectrum_bytes.argtypes = [C.c_int, C.c_longlong, C.c_int]
    lib.p_product_bytes.argtypes = [C.c_int, C.c_longlong, C.c_int]
    lib.p_filter_bytes.argtypes = [C.c_int] * 3
    return lib


def _arr(v):
    return np.ascontiguousarray(v, np.int32).ctypes.data_as(I32)


def _plan(lib, T, segs):
    N, H, W = (np.array(v, np.int32) for v in zip(*segs))
    head = np.zeros(5 + 4 * len(segs), np.int32)
    assert lib.p_plan(T, K, len(segs), _arr(N), _arr(H), _arr(W), head.ctypes.data_as(I32)) == 1
    tiles = np.zeros((head[4], 6), np.int32)
    assert lib.p_tiles(T, K, len(segs), _arr(N), _arr(H), _arr(W), tiles.ctypes.data_as(I32)) == 1
    return head, tiles


@pytest.mark.parametrize("T", [32, 64])
def test_every_pixel_in_one_valid_corner(plan, T):
    """Every map up to 120 x 120, two images each: the corners (n, y0 .. y0 + V, x0 .. x0 + V) cut at the map's edge partition the pixels
    exactly when the tiles are all different, start at multiples of V inside the map and number N * ceil(H / V) * ceil(W / V) — pixel
    (y, x) then lies in the corner that starts at (y // V * V, x // V * V) and in no other.  A spread of sizes is also counted pixel by pixel."""
    V = T - K + 1
    counted = {(h, w) for h in (1, 5, V - 1, V, V + 1, 2 * V, 2 * V + 1, 57, 120) for w in (1, V - 1, V, V + 1, 2 * V, 37, 40, 120)}
    for H in range(1, 121):
        for W in range(1, 121):
            head, tiles = _plan(plan, T, [(2, H, W)])
            tx, ty = -(-W // V), -(-H // V)
            assert tuple(head[:5]) == (T, K, V, T * (T // 2 + 1), 2 * tx * ty) and tuple(head[5:9]) == (tx, ty, tx * ty, 0)
            s, n, y0, x0, wy, wx = tiles.T
            assert (s == 0).all() and ((n == 0) | (n == 1)).all() and (y0 % V == 0).all() and (x0 % V == 0).all()
            assert (y0 >= 0).all() and (y0 < H).all() and (x0 >= 0).all() and (x0 < W).all()
            assert (wy == y0 - K // 2).all() and (wx == x0 - K // 2).all()
            assert len(np.unique((n * 128 + y0) * 128 + x0)) == 2 * tx * ty == len(tiles)
            if (H, W) in counted:
                hit = np.zeros((2, H, W), np.int32)
                for _, n_, y_, x_, _, _ in tiles:
                    hit[n_, y_:y_ + V, x_:x_ + V] += 1
                assert (hit == 1).all(), (T, H, W)


def test_segments_and_tile_order(plan):
    """The detector's four maps in one launch: segment, image, row, column order; tile0 = tiles before the segment."""
    segs = [(3, 88, 116), (3, 60, 80), (3, 44, 60), (3, 32, 40)]
    head, tiles = _plan(plan, 32, segs)
    want, tile0 = [], []
    for s, (N, H, W) in enumerate(segs):
        tile0.append(len(want))
        want += [(s, n, y0, x0, y0 - 7, x0 - 7) for n in range(N) for y0, x0 in R.tile_list(H, W, 32, K)]
    assert [tuple(t) for t in tiles] == want
    assert [head[8 + 4 * s] for s in range(4)] == tile0
    assert [head[7 + 4 * s] for s in range(4)] == [35, 20, 12, 6] and head[4] == 3 * 73      # the issue's tile counts


def test_refusals(plan):
    out = np.zeros(32, np.int32)
    for T, k, segs in ((48, 15, [(1, 8, 8)]), (32, 14, [(1, 8, 8)]), (32, 33, [(1, 8, 8)]), (32, 15, [(0, 8, 8)]), (32, 15, [(1, 0, 8)]),
                       (32, 15, [(1, 8, 8)] * 5), (32, 15, [(1 << 20, 120, 120)])):
        N, H, W = (np.array(v, np.int32) for v in zip(*segs))
        lib_rc = plan.p_plan(T, k, len(segs), _arr(N), _arr(H), _arr(W), out.ctypes.data_as(I32))
        assert lib_rc == 0, (T, k, segs)


def test_sizes_and_chunks(plan):
    for T in (32, 64):
        bins = T * (T // 2 + 1)
        for tiles, Cin in ((1, 32), (73, 512), (1168, 512), (70000, 512)):
            assert plan.p_spectrum_bytes(T, tiles, Cin) == bins * tiles * 2 * Cin * 4
            assert plan.p_product_bytes(T, tiles, 32) == bins * tiles * 64 * 4
        assert plan.p_filter_bytes(T, 512, 32) == bins * 1024 * 64 * 4
        for tpq, Cin in ((73, 512), (73, 64), (1, 32), (600, 512), (5000, 512)):
            for want in (1, 2, 4, 8, 16, 64):
                q = plan.p_chunk(T, tpq, Cin, want)
                assert 0 <= q <= want
                assert q == 0 or bins * q * tpq * 2 * Cin * 4 < 2 ** 31
                assert q == want or bins * (q + 1) * tpq * 2 * Cin * 4 >= 2 ** 31      # the largest that fits
    assert plan.p_chunk(32, 73, 512, 16) == 13 and plan.p_chunk(32, 73, 512, 8) == 8 and plan.p_chunk(32, 5000, 512, 4) == 0


@pytest.mark.parametrize("H,W", [(18, 18), (19, 37), (5, 40), (18, 36)])
def test_restatement_equals_conv2d(H, W):
    """One tile exactly, partial tiles on both axes, a map smaller than V, an exact tiling: float64, 1e-12 of the output range."""
    rng = np.random.default_rng(H * 100 + W)
    C_, Rn = 6, 3
    x = np.maximum(rng.standard_normal((H, W, C_)), 0)
    w = rng.standard_normal((Rn, K, K, C_))
    got = R.corr_fft(x, w, 32, np.float64)
    want = torch.nn.functional.conv2d(torch.from_numpy(x).permute(2, 0, 1)[None], torch.from_numpy(w).permute(0, 3, 1, 2), padding=K // 2)
    want = want[0].permute(1, 2, 0).numpy()
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_restatement_keeps_float32():
    rng = np.random.default_rng(1)
    x = np.maximum(rng.standard_normal((19, 20, 4)), 0).astype(np.float32)
    w = rng.standard_normal((2, K, K, 4)).astype(np.float32)
    got = R.corr_fft(x, w, 32, np.float32)
    assert got.dtype == np.float32
    ref = R.corr_fft(x, w, 32, np.float64)
    assert 0 < np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()


def test_header_under_sanitizers(tmp_path):
    """The header in a stand-alone program (its own main walks every map up to 40 x 40 and the detector's pyramid) under
    -fsanitize=address,undefined."""
    exe = str(tmp_path / "corr_fft_plan_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DCFFT_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SHIM, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "corr_fft_plan ok" in r.stdout, r.stdout + r.stderr
