"""The halo-patch kernel's instruction shapes and LDS swizzle, checked without a GPU.
(1) conv16w_kernel<3, *> (fp16 hi / lo pairs) runs on v_mfma_f32_16x16x32_f16 only; the 16-bit modes (MM = 1 / 2) stay on the 32x32x16 forms.
(2) A model of the ds_read_b128 lane groups: the pair kernel's slot swizzle is conflict-free for every tile width and banded layout of
c16g::halo_tiling and every tap shift, and the address the kernel reads (one swizzle term per tap column, shared by its eight m-tiles)
finds the logical slot the patch fill put there."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# ds_read_b128: four groups of 16 lanes, one LDS cycle each when their 16 addresses fall in 16 distinct 16-byte bank slots
GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS += [[l + 32 for l in g] for g in GROUPS]


def _pair_swizzle(tw):
    """(swa, swd) of c16g::halo_tiling for the pair kernel."""
    return (1 if tw >= 16 else 0), 0


def _layouts():
    """(tile width, rows per band, bands) of every halo tiling (bands of segh + 2 patch rows, at most 288 patch rows)."""
    for tw in (4, 8, 16, 32):
        th = 128 // tw
        for segh in (1, 2, 4, 8, 16, 32):
            if segh <= th and th % segh == 0 and (th // segh) * (segh + 2) * (tw + 2) <= 288:
                yield tw, segh


def test_pair_swizzle_conflict_free_and_consistent():
    n = 0
    for tw, segh in _layouts():
        swa, swd = _pair_swizzle(tw)
        pw = tw + 2

        def fill_sw(prow, pcol):                    # the patch fill: physical slot s of (prow, pcol) holds logical slot s ^ fill_sw
            return ((pcol >> swa) + prow * swd) & 3
        assert swd == 0 and swa <= 2, "the pair kernel's shared per-tap swizzle term needs swd = 0 and swa <= 2"
        for mt in range(8):
            for ky, kx in itertools.product(range(3), range(3)):
                for g in GROUPS:
                    slots = set()
                    for l in g:
                        p = 16 * mt + (l & 15)
                        py, px = p // tw, p % tw
                        b, ly = py // segh, py % segh
                        prow, pcol = b * (segh + 2) + ly + ky, px + kx
                        logical = l >> 4
                        # the kernel's read: xs[kx] = (logical ^ ((((l & 15) & (tw - 1)) + kx) >> swa) & 3) << 4, the same for all m-tiles
                        phys = logical ^ (((((l & 15) & (tw - 1)) + kx) >> swa) & 3)
                        assert phys ^ fill_sw(prow, pcol) == logical, (tw, segh, mt, ky, kx, l)
                        slots.add((4 * (prow * pw + pcol) + phys) % 16)
                    assert len(slots) == 16, f"bank conflict: TW {tw}, rows per band {segh}, m-tile {mt}, tap ({ky}, {kx})"
                    n += 1
    assert n == 12 * 8 * 9 * 4


def test_halo_tiling_pair_swizzle_matches_model(tmp_path):
    """The values the model checks are the ones the launcher's chooser (c16g::halo_tiling, called through tests/conv16w_geom_shim.cpp)
    assigns in pair mode, for every tile width and banded layout of the model."""
    so = str(tmp_path / "conv16w_geom.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "conv16w_geom_shim.cpp"), "-o", so], check=True)
    geo = C.CDLL(so)
    geo.g_halo_tiling.argtypes = [C.c_int] * 5 + [C.c_void_p, C.POINTER(C.c_int)]
    buf = C.create_string_buffer(geo.g_sizeof_tiling())
    seen = set()
    for tw, segh in _layouts():
        # maps exactly one tile wide and segh high, whole tiles of them: the chooser takes width tw (no overhang, ties to the wider tile)
        out = (C.c_int * 8)()
        assert geo.g_halo_tiling(2 * (128 // tw // segh), segh, tw, 1, 0, buf, out) == 1
        tw_log2, segh_log2, swa, swd = out[0], out[3], out[5], out[6]
        assert (1 << tw_log2, 1 << segh_log2) == (tw, segh)
        assert (swa, swd) == _pair_swizzle(tw), (tw, segh)
        assert swd == 0 and swa <= 2
        seen.add(tw)
    assert seen == {4, 8, 16, 32}
    shutil.rmtree(tmp_path, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_conv16w_mfma_shapes(tmp_path):
    out = tmp_path / "conv16.s"
    src = os.path.join(ROOT, "gen6d_amd", "csrc", "conv16w.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                        "-o", str(out), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    bodies = dict(re.findall(r"^(_ZN\S*conv16w_kernelILi(\d)E\S*):", text, re.M))
    seen = set()
    for m in re.finditer(r"^(_ZN\S*conv16w_kernelILi(\d)E\S*):(.*?)s_endpgm", text, re.S | re.M):
        name, mm, body = m.group(1), int(m.group(2)), m.group(3)
        seen.add(mm)
        n16 = len(re.findall(r"v_mfma_f32_16x16x32_(?:f16|bf16)", body))
        n32 = len(re.findall(r"v_mfma_f32_32x32x16_(?:f16|bf16)", body))
        if mm == 3:
            assert n16 > 0 and n32 == 0, f"{name}: {n16} 16x16x32 / {n32} 32x32x16 MFMAs"
        else:
            assert n32 > 0 and n16 == 0, f"{name}: {n16} 16x16x32 / {n32} 32x32x16 MFMAs"
    assert seen == {1, 2, 3}, bodies
    shutil.rmtree(tmp_path, ignore_errors=True)
