"""The product kernel's share of gen6d_amd/csrc/corr_fft_plan.h (corrfft_gemm_kernel: block shape, grid order, the LDS stage image its
direct-to-LDS requests build, the ring of stages), built for the host (tests/corr_fft_gemm_plan_shim.cpp) and checked against plain
formulas for M = 1 .. 600 rows and Cin = 32 .. 512 in steps of 32; the same walk once in a stand-alone program under the address and
undefined-behaviour sanitizers (tests/corr_fft_gemm_plan_sanitize.cpp).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "corr_fft_gemm_plan_shim.cpp")
I32 = C.POINTER(C.c_int)
BINS = 32 * 17
LDS_LIMIT = 160 * 1024
MS = range(1, 601)
CINS = range(32, 513, 32)


@pytest.fixture(scope="module")
def gp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cfftg") / "corr_fft_gemm_plan.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.g_shape.argtypes = [C.c_int, I32]
    lib.g_cover.argtypes = [C.c_int, C.c_int, I32, I32]
    lib.g_ring.argtypes = [C.c_int, C.c_int, I32]
    lib.g_conflicts.argtypes = [I32]
    return lib


def _shape(gp, M):
    out = np.zeros(10, np.int32)
    gp.g_shape(M, out.ctypes.data_as(I32))
    return dict(zip(("waves", "stages", "cap", "mblocks", "stage", "lds", "loads", "bpw", "rows", "idle_loads"), (int(v) for v in out)))


def test_block_shape_and_sizes(gp):
    """Waves of 64 rows; two waves up to 128 rows (three such blocks fit a CU), four waves beyond (two fit), a ring of two stages each;
    a stage = 128 bytes per row + 8 KB of B'; blocks per bin = ceil(M / rows a block can hold), the rows spread evenly over them in whole
    waves; everything under the 160 KB of a CU."""
    for M in MS:
        s = _shape(gp, M)
        assert s["waves"] == (2 if M <= 128 else 4) and s["cap"] == 64 * s["waves"] and s["stages"] == 2
        assert s["mblocks"] == -(-M // s["cap"]) and (s["mblocks"] == 1 if M <= 256 else s["mblocks"] >= 2)
        assert s["rows"] == 64 * -(-M // (64 * s["mblocks"])) <= s["cap"] and (s["mblocks"] - 1) * s["rows"] < M <= s["mblocks"] * s["rows"]
        assert s["stage"] == s["cap"] * 128 + 32 * 64 * 4 and s["lds"] == s["stages"] * s["stage"] <= LDS_LIMIT
        assert s["loads"] == 8 + 8 // s["waves"] and s["idle_loads"] == 8 // s["waves"] and s["bpw"] * s["waves"] == 8
        assert s["loads"] * (s["stages"] - 1) < 64                              # the counted wait fits vmcnt's six bits
    assert _shape(gp, 128)["lds"] * 3 <= LDS_LIMIT and _shape(gp, 129)["lds"] * 2 <= LDS_LIMIT
    assert [_shape(gp, M)["rows"] for M in (73, 146, 292, 584)] == [128, 192, 192, 256]


def test_rows_covered_exactly_once(gp):
    """Every (bin, row) belongs to exactly one (block, wave, lane row) of the grid of bins * mblocks blocks; every request names a row
    of the bin (a wave with rows asks for 64: those from M on as row M - 1; a wave without rows asks for none); the blocks of a bin follow
    each other among the blocks of one XCD label."""
    for M in MS:
        s = _shape(gp, M)
        hit, clamp = np.zeros((BINS, M), np.int32), np.zeros((BINS, M), np.int32)
        assert gp.g_cover(M, BINS, hit.ctypes.data_as(I32), clamp.ctypes.data_as(I32)) == 0, M
        assert (hit == 1).all(), M
        per_bin = -(-M // 64) * 64 * 8                                           # 8 requests of 16 bytes per row and stage, whole waves
        assert (clamp.sum(1) == per_bin).all() and (clamp[:, :M - 1] == 8).all() and (clamp[:, M - 1] == per_bin - 8 * (M - 1)).all(), M


@pytest.mark.parametrize("waves", [2, 4])
def test_stage_image(gp, waves):
    """The requests of a stage land lane-linear and tile it exactly once; each X row arrives as one whole 128-byte line from 8 consecutive
    lanes, and every 16-byte k-segment lies where the fragment read (same swizzle) looks for it; B' keeps its own order behind the X images."""
    assert gp.g_stage_image(waves) == 0


def test_fragment_reads_are_conflict_free(gp):
    """The eight 16-byte reads of X (lane groups of ds_read_b128, 64 banks) and the 32 four-byte reads of B' (half waves, 32 banks) of a
    stage cost no extra LDS cycle, and both operands take the same 16 k per lane."""
    out = np.full(2, -1, np.int32)
    assert gp.g_conflicts(out.ctypes.data_as(I32)) == 0
    assert out.tolist() == [0, 0]


@pytest.mark.parametrize("waves", [2, 4])
def test_ring_schedule(gp, waves):
    """Over every step count of Cin = 32 .. 512: a step is read only after the counted wait retired its requests, a request never lands in
    a stage that is being read or still unread, prologue and drain included; stages - 1 steps are in flight at the most."""
    stages = 2
    for Cin in CINS:
        steps = gp.g_steps(Cin)
        assert steps == 2 * Cin // 32
        peak = C.c_int(-1)
        assert gp.g_ring(waves, steps, C.byref(peak)) == 0, Cin
        assert peak.value == min(stages - 1, steps), Cin


def test_plan_under_sanitizers(tmp_path):
    """The same walk in a stand-alone program (its own main, no Python in the process) under -fsanitize=address,undefined."""
    exe = str(tmp_path / "cfft_gemm_plan_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "corr_fft_gemm_plan_sanitize.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 broken" in r.stdout, r.stdout[-2000:]
