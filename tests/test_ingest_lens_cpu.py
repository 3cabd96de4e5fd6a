"""Lens undistortion in the ingest (gen6d_amd.ingest.Lens, g6d_frame_ingest_mesh) on the CPU.  `np_frame_ingest_mesh` restates the integer
per-pixel rule of the mesh path (include/gen6d_hip.h) in numpy with the signature of ops.frame_ingest_mesh (on a CPU
device the tables' pointers are host addresses), `np_mesh` restates the host's mesh construction and step choice.  Checks the model
formulas against hand-computed values, the mesh against the float64 model, an analytic picture through a lens, the formats, the border
rule, mixed launches, the tracker on lens frames, the errors, the descriptor's layout and the kernel's resources."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_ingest_cpu import YUV, cpu_ingest, ingest_cpu, np_frame_ingest, np_ingest, nv12_of, patched, pitched, rgb_to, scene  # noqa: F401

BARREL = ("brown", (-0.35, 0.12, 0.001, -0.0005, -0.02))
PINCUSHION = ("brown", (0.25, 0.05, 0, 0, 0))
FISHEYE = ("fisheye", (0.05, -0.01, 0.003, -0.001))


def camera(ws, hs, f):
    return np.array([[f, 0, ws / 2 - 0.5], [0, f, hs / 2 - 0.5], [0, 0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_model(model, c, x, y):
    """The lens models as the issue writes them out (OpenCV's conventions), float64."""
    r2 = x * x + y * y
    if model == "fisheye":
        r = np.sqrt(r2)
        th = np.arctan(r)
        thd = th * (1 + c[0] * th ** 2 + c[1] * th ** 4 + c[2] * th ** 6 + c[3] * th ** 8)
        s = np.ones_like(r)
        s[r > 0] = thd[r > 0] / r[r > 0]
        return s * x, s * y
    k1, k2, p1, p2, k3, k4, k5, k6 = (list(c) + [0.0] * 8)[:8]
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def np_source(model, c, K, new_K, ws, hs, rot, out_w, out_h, X, Y):
    """Canvas pixel (X, Y) -> source coordinate (float64): quarter turn undone, scaling undone, new_K^-1, the model, K."""
    wt, ht = (out_h, out_w) if rot in (90, 270) else (out_w, out_h)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    x, y = {0: (X, Y), 90: (Y, ht - 1 - X), 180: (wt - 1 - X, ht - 1 - Y), 270: (wt - 1 - Y, X)}[rot]
    u, v = (x + 0.5) * ws / wt - 0.5, (y + 0.5) * hs / ht - 0.5
    n = np.linalg.inv(new_K) @ np.stack([u.ravel(), v.ravel(), np.ones(u.size)])
    xd, yd = np_model(model, c, n[0] / n[2], n[1] / n[2])
    d = K @ np.stack([xd, yd, np.ones(xd.size)])
    return (d[0] / d[2]).reshape(u.shape), (d[1] / d[2]).reshape(u.shape)


def np_mesh_miss(model, c, K, new_K, ws, hs, rot, out_w, out_h, g):
    """(float64 nodes [ny,nx,2] of step g, the largest per-axis distance in source pixels between their bilinear interpolation and the
    model over every cell's centre and four edge midpoints)."""
    at = lambda X, Y: np.stack(np_source(model, c, K, new_K, ws, hs, rot, out_w, out_h, X, Y), -1)
    nx, ny = -(-out_w // g) + 1, -(-out_h // g) + 1
    m = at(*np.meshgrid(np.arange(nx) * g, np.arange(ny) * g))
    r, col = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")          # every cell
    m00, m01, m10, m11 = m[r, col], m[r, col + 1], m[r + 1, col], m[r + 1, col + 1]
    miss = 0.0
    for (dx, dy), v in (((0.5, 0.5), (m00 + m01 + m10 + m11) / 4), ((0.5, 0), (m00 + m01) / 2), ((0.5, 1), (m10 + m11) / 2),
                        ((0, 0.5), (m00 + m10) / 2), ((1, 0.5), (m01 + m11) / 2)):
        miss = max(miss, np.abs(at((col + dx) * g, (r + dy) * g) - v).max())
    return m, miss


def np_mesh(model, c, K, new_K, ws, hs, rot, out_w, out_h, tol):
    """-> (int32 nodes, step_log2, {step: miss}): the largest step of 16, 8, 4, 2 whose miss is within tol * max(ws/wt, hs/ht)."""
    wt, ht = (out_h, out_w) if rot in (90, 270) else (out_w, out_h)
    seen = {}
    for g in (16, 8, 4, 2):
        m, seen[g] = np_mesh_miss(model, c, K, new_K, ws, hs, rot, out_w, out_h, g)
        if seen[g] <= tol * max(ws / wt, hs / ht):
            return np.clip(np.rint(m * 65536), -2 ** 30, 2 ** 30).astype(np.int32), int(math.log2(g)), seen
    return None, None, seen


def np_mesh_coords(nodes, lg, out_w, out_h):
    """The per-pixel rule, first half: int32 nodes [ny,nx,2] -> (fx, fy) int64 [out_h,out_w] in 1/2048 source pixels, exact integers."""
    g, s = 1 << lg, 2 * lg + 5
    Y, X = np.meshgrid(np.arange(out_h), np.arange(out_w), indexing="ij")
    i, j, cx, cy = X % g, Y % g, X // g, Y // g
    m = nodes.astype(np.int64)
    out = []
    for a in (0, 1):
        S = (g - i) * (g - j) * m[cy, cx, a] + i * (g - j) * m[cy, cx + 1, a] + (g - i) * j * m[cy + 1, cx, a] + i * j * m[cy + 1, cx + 1, a]
        out.append((S + (1 << (s - 1))) >> s)
    return out


def np_mesh_picture(p0, p1, pitch0, pitch1, ws, hs, fmt, matrix, out_w, out_h, H, W, nodes, lg):
    """Flat uint8 planes + mesh -> the [H,W,3] canvas: border test, clamp, four taps converted to RGB, 11-bit blend."""
    fx, fy = np_mesh_coords(nodes, lg, out_w, out_h)
    inside = (fx >= -1024) & (fx <= (ws - 1) * 2048 + 1024) & (fy >= -1024) & (fy <= (hs - 1) * 2048 + 1024)
    fx, fy = np.clip(fx, 0, (ws - 1) * 2048), np.clip(fy, 0, (hs - 1) * 2048)
    x0, a, y0, b = fx >> 11, fx & 2047, fy >> 11, fy & 2047
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    p0 = np.asarray(p0).astype(np.int64)

    def rgb(xi, yi):
        if fmt == 4:
            uv = np.asarray(p1).astype(np.int64)
            CY, CVR, CUG, CVG, CUB = YUV[matrix]
            c = np.maximum(p0[yi * pitch0 + xi] - 16, 0)
            d = uv[(yi >> 1) * pitch1 + (xi >> 1) * 2] - 128
            e = uv[(yi >> 1) * pitch1 + (xi >> 1) * 2 + 1] - 128
            ch = [(CY * c + CVR * e + 2 ** 19) >> 20, (CY * c - CUG * d - CVG * e + 2 ** 19) >> 20, (CY * c + CUB * d + 2 ** 19) >> 20]
            return np.clip(np.stack(ch, -1), 0, 255)
        bpp, ro = (4 if fmt >= 2 else 3), (2 if fmt in (1, 3) else 0)
        o = yi * pitch0 + xi * bpp
        return np.stack([p0[o + ro], p0[o + 1], p0[o + 2 - ro]], -1)
    a, b = a[..., None], b[..., None]
    s = ((2048 - a) * (2048 - b) * rgb(x0, y0) + a * (2048 - b) * rgb(x1, y0) + (2048 - a) * b * rgb(x0, y1) + a * b * rgb(x1, y1) + 2 ** 21)
    canvas = np.zeros((H, W, 3), np.uint8)
    canvas[:out_h, :out_w] = np.where(inside[..., None], s >> 22, 0).astype(np.uint8)
    return canvas


def np_frame_ingest_mesh(table, meshes, n, out, K_out):
    """ops.frame_ingest_mesh on host memory: entries without nodes through np_frame_ingest, the others through the mesh rule."""
    fsize, msize = C.sizeof(lib.G6dFrame), C.sizeof(lib.G6dMesh)
    ents = (lib.G6dFrame * n).from_buffer_copy(table.numpy()[:n * fsize].tobytes())
    mesh = (lib.G6dMesh * n).from_buffer_copy(meshes.numpy()[:n * msize].tobytes())
    B, H, W = out.shape[:3]
    view = lambda ptr, nb: np.ctypeslib.as_array((C.c_uint8 * nb).from_address(ptr))
    for k, (e, m) in enumerate(zip(ents, mesh)):
        if not m.nodes:
            np_frame_ingest(table[k * fsize:], 1, out, K_out)
            continue
        if not 0 <= e.slot < B:
            continue
        nv12 = e.format == 4
        bpp = 1 if nv12 else (4 if e.format >= 2 else 3)
        p0 = view(e.plane0, (e.height - 1) * e.pitch0 + e.width * bpp)
        p1 = view(e.plane1, (e.height // 2 - 1) * e.pitch1 + e.width) if nv12 else None
        assert 1 <= m.step_log2 <= 4 and m.nx >= -(-e.out_w >> m.step_log2) + 1 and m.ny >= -(-e.out_h >> m.step_log2) + 1
        nodes = np.ctypeslib.as_array((C.c_int32 * (m.ny * m.nx * 2)).from_address(m.nodes)).reshape(m.ny, m.nx, 2)
        out.numpy()[e.slot] = np_mesh_picture(p0, p1, e.pitch0, e.pitch1, e.width, e.height, e.format, e.matrix, e.out_w, e.out_h, H, W,
                                              nodes, m.step_log2)
        K_out.numpy()[e.slot] = np.asarray(list(e.K), np.float32).reshape(3, 3)
    return out


_restated = {}     # np_mesh results of this session (the same camera comes in several formats)


def np_ingest_lens(frame, H, W):
    """One ingest.Frame with a lens -> [H,W,3] canvas through `plan`, np_mesh (the restated mesh) and np_mesh_picture."""
    out_h, out_w, _ = I.plan(frame, (H, W))
    L = frame.lens
    new_K = frame.K if L.new_K is None else np.asarray(L.new_K).reshape(3, 3)
    key = (L.model, L.coeffs, frame.K.tobytes(), new_K.tobytes(), frame.width, frame.height, frame.rotate, out_w, out_h, L.tol)
    if key not in _restated:
        _restated[key] = np_mesh(L.model, L.coeffs, frame.K, new_K, frame.width, frame.height, frame.rotate, out_w, out_h, L.tol)[:2]
    nodes, lg = _restated[key]
    host = lambda p: None if p is None else (p.cpu().numpy() if torch.is_tensor(p) else p)
    return np_mesh_picture(host(frame.plane0), host(frame.plane1), frame.pitch, frame.uv_pitch, frame.width, frame.height,
                           I.FORMATS[frame.fmt], I.MATRICES[frame.matrix], out_w, out_h, H, W, nodes, lg)


@pytest.fixture
def cpu_lens(monkeypatch, cpu_ingest):
    monkeypatch.setattr(ops, "frame_ingest_mesh", np_frame_ingest_mesh)
    I._meshes.clear()


def run_table(frame, nodes, lg, H, W, out_w, out_h):
    """np_frame_ingest_mesh on one host frame with a hand-made mesh."""
    t, m = lib.G6dFrame(), lib.G6dMesh()
    t.plane0, t.pitch0, t.width, t.height, t.format, t.out_w, t.out_h = frame.plane0.ctypes.data, frame.pitch, frame.width, frame.height, I.FORMATS[frame.fmt], out_w, out_h
    nodes = np.ascontiguousarray(nodes, np.int32)
    m.nodes, m.ny, m.nx, m.step_log2 = nodes.ctypes.data, nodes.shape[0], nodes.shape[1], lg
    out, K = torch.zeros((1, H, W, 3), dtype=torch.uint8), torch.zeros((1, 3, 3))
    as_t = lambda s: torch.from_numpy(np.frombuffer(bytes(s), np.uint8).copy())
    return np_frame_ingest_mesh(as_t(t), as_t(m), 1, out, K).numpy()[0]


# ---------------------------------------------------------------------------------------------------------------- 1: the models
def test_model_formulas_against_hand_computed_values():
    """brown at r2 = 0.25 with BARREL: rad = 1 - 0.0875 + 0.0075 - 0.0003125 = 0.9196875;
      (0.5, 0):     xd = 0.45984375 + p2 (0.25 + 0.5) = 0.45946875,                 yd = p1 0.25 = 0.00025
      (0, 0.5):     xd = p2 0.25 = -0.000125,                                       yd = 0.45984375 + p1 0.75 = 0.46059375
      (0.3, -0.4):  xd = 0.27590625 - 0.00024 - 0.0005 (0.25 + 0.18) = 0.27545125,  yd = -0.367875 + 0.001 0.57 + 0.00012 = -0.367185
    the rational form (k1 = 0.1, k4 = 0.2) at (1, 0): rad = 1.1 / 1.2; four coefficients (0.1, 0.2, 0.01, 0.02) at (1, 1): r2 = 2,
    rad = 1 + 0.2 + 0.8 = 2, xd = 2 + 2 0.01 + 0.02 (2 + 2) = 2.1, yd = 2 + 0.01 (2 + 2) + 2 0.02 = 2.08.
    fisheye FISHEYE at r = 1: t = pi/4 = 0.785398163, t2 = 0.616850275, t4 = 0.380504262, t6 = 0.234714159, t8 = 0.144783493,
      td = t (1 + 0.030842514 - 0.003805043 + 0.000704142 - 0.000144783) = 0.785398163 * 1.02759683 = 0.80707266; at r = sqrt 3 (t = pi/3):
      td = 1.09465178, td / r = 0.63199750; at r = 0.5: t = 0.46364761, td = 0.46842967, td / r = 0.93685935."""
    L = I.Lens(*BARREL)
    for (x, y), want in (((0.5, 0.0), (0.45946875, 0.00025)), ((0.0, 0.5), (-0.000125, 0.46059375)), ((0.3, -0.4), (0.27545125, -0.367185))):
        np.testing.assert_allclose(L.distort(x, y), want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(np_model("brown", BARREL[1], np.float64(x), np.float64(y)), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(I.Lens("brown", (0.1, 0, 0, 0, 0, 0.2, 0, 0)).distort(1.0, 0.0), (1.1 / 1.2, 0.0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(I.Lens("brown", (0.1, 0.2, 0.01, 0.02)).distort(1.0, 1.0), (2.0 + 0.02 + 0.08, 2.0 + 0.04 + 0.04), rtol=0, atol=1e-14)
    F = I.Lens(*FISHEYE)
    for (x, y), s in (((1.0, 0.0), 0.80707266), ((0.6, -0.8), 0.80707266), ((0.0, math.sqrt(3)), 0.63199750), ((0.3, 0.4), 0.93685935)):
        np.testing.assert_allclose(F.distort(x, y), (s * x, s * y), rtol=0, atol=2e-8)
        np.testing.assert_allclose(np_model("fisheye", FISHEYE[1], np.array([x]), np.array([y])), [[s * x], [s * y]], rtol=0, atol=2e-8)
    assert tuple(np.asarray(v).item() for v in F.distort(0.0, 0.0)) == (0.0, 0.0)                    # factor 1 at r = 0: no 0 / 0
    near = F.distort(np.array([0.0, 1e-9]), np.array([0.0, 0.0]))
    np.testing.assert_allclose(near[0], [0.0, 1e-9], rtol=1e-12, atol=0)
    assert L == I.Lens(*BARREL) and hash(L) == hash(I.Lens(*BARREL)) and L != F and L != I.Lens(BARREL[0], BARREL[1], tol=1 / 8)
    with pytest.raises(AttributeError):
        L.tol = 1.0


# ---------------------------------------------------------------------------------------------------------------- 2: the mesh
MESH_CASES = [((240, 320), (120, 160), 0, 200.0), ((488, 652), (163, 122), 90, 400.0)]


@pytest.mark.parametrize("lens", [BARREL, PINCUSHION, FISHEYE], ids=["barrel", "pincushion", "fisheye"])
@pytest.mark.parametrize("src_hw,canvas,rot,f", MESH_CASES, ids=["320x240", "652x488-rot90"])
def test_mesh_stays_within_tol_of_the_model(lens, src_hw, canvas, rot, f):
    """At every pixel the integer interpolation of the mesh stays within tol * max(ws/wt, hs/ht) source pixels (tol = 1/16 canvas pixel)
    of the float64 model, plus the quantisation of the nodes (2^-16) and of the result (half of 1/2048 = 2^-12); the step is the largest
    whose centre / edge-midpoint check passes; ingest.Lens.mesh gives the restated nodes bit for bit.
    Measured (step, largest distance over all pixels in source pixels; bound 0.1253 at 2:1 and 0.2503 at 4:1; the next coarser step's
    miss at the checked points):
      320x240 -> 160x120, f 200:          barrel 4, 0.0459 (step 8: 0.182); pincushion 4, 0.0988 (0.378); fisheye 4, 0.0345 (0.137)
      652x488 -> 122x163 rot 90, f 400:   barrel 4, 0.0915 (step 8: 0.366); pincushion 4, 0.2072 (0.880); fisheye 4, 0.0688 (0.274)"""
    (hs, ws), (H, W) = src_hw, canvas
    K = camera(ws, hs, f)
    fr = I.Frame(np.zeros((hs, ws, 3), np.uint8), rotate=rot, K=K, lens=I.Lens(*lens))
    out_h, out_w, _ = I.plan(fr, (H, W))
    wt, ht = (out_h, out_w) if rot else (out_w, out_h)
    scale = max(ws / wt, hs / ht)
    nodes, lg, seen = np_mesh(lens[0], lens[1], K, K, ws, hs, rot, out_w, out_h, 1 / 16)
    got, got_lg = fr.lens.mesh(K, ws, hs, rot, out_w, out_h)
    assert got_lg == lg and got.dtype == np.int32 and got.shape == (-(-out_h >> lg) + 1, -(-out_w >> lg) + 1, 2)
    np.testing.assert_array_equal(got, nodes)
    fx, fy = np_mesh_coords(nodes, lg, out_w, out_h)
    Y, X = np.meshgrid(np.arange(out_h), np.arange(out_w), indexing="ij")
    u, v = np_source(lens[0], lens[1], K, K, ws, hs, rot, out_w, out_h, X, Y)
    dist = max(np.abs(fx / 2048 - u).max(), np.abs(fy / 2048 - v).max())
    print(f"{lens[0]} {ws}x{hs} -> {out_w}x{out_h} rotate {rot}: step {1 << lg}, largest distance {dist:.4f} source pixels, "
          f"bound {scale / 16 + 2.0 ** -16 + 2.0 ** -12:.4f}; misses by step {seen}")
    assert dist <= scale / 16 + 2.0 ** -16 + 2.0 ** -12
    assert seen[1 << lg] <= scale / 16 and all(miss > scale / 16 for g, miss in seen.items() if g > 1 << lg)
    assert 1 << lg < 16                                                   # these lenses are strong: the coarsest step never suffices here


# ---------------------------------------------------------------------------------------------------------------- 3: an analytic picture
def wave(u, v):
    return 127.5 + 60 * np.sin(2 * np.pi * u / 37) + 50 * np.cos(2 * np.pi * v / 29)


@pytest.mark.parametrize("lens", [BARREL, PINCUSHION, FISHEYE], ids=["barrel", "pincushion", "fisheye"])
@pytest.mark.parametrize("src_hw,canvas,rot,f", MESH_CASES, ids=["320x240", "652x488-rot90"])
def test_analytic_picture_through_a_lens(cpu_lens, lens, src_hw, canvas, rot, f):
    """Source g(u, v) = 127.5 + 60 sin(2 pi u / 37) + 50 cos(2 pi v / 29) in all channels, sampled at pixel centres.  A pixel of the
    ingested picture lies within
        max|grad g| (tol max(ws/wt, hs/ht) + 1/2048) + (|g_uu| + |g_vv|) / 8 + 0.75
    of g(distort(pinhole pixel)): |grad g| <= sqrt((60 2pi/37)^2 + (50 2pi/29)^2) = sqrt(10.189^2 + 10.833^2) = 14.872 per source pixel
    times the mesh's distance to the model and the 1/2048 grid of the weights; a bilinear blend over a unit cell misses a smooth function
    by at most (max|g_uu| + max|g_vv|) / 8 = (60 (2pi/37)^2 + 50 (2pi/29)^2) / 8 = (1.730 + 2.347) / 8 = 0.510; 0.25 for the 11-bit
    weights (2 * 255 / 2048) and 0.5 for the final rounding.  At 2:1 that is 14.872 * 0.12549 + 0.510 + 0.75 = 3.126, at 4:1 4.985.
    Pixels the model puts more than half a pixel + the mesh tolerance outside the source are exactly 0, pixels as far inside are not
    border pixels (the band between is either).  Measured: at most 1.76 (2:1, the pincushion lens) and 2.67 (4:1)."""
    (hs, ws), (H, W) = src_hw, canvas
    K = camera(ws, hs, f)
    v, u = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
    src = np.repeat(np.rint(wave(u, v)).astype(np.uint8)[..., None], 3, -1)
    fr = I.Frame(src, rotate=rot, K=K, lens=I.Lens(*lens))
    out_h, out_w, _ = I.plan(fr, (H, W))
    got, _ = ingest_cpu([fr], H, W)
    np.testing.assert_array_equal(got[0], np_ingest_lens(fr, H, W))
    Y, X = np.meshgrid(np.arange(out_h), np.arange(out_w), indexing="ij")
    ud, vd = np_source(lens[0], lens[1], K, K, ws, hs, rot, out_w, out_h, X, Y)
    scale = max(ws / (out_h if rot else out_w), hs / (out_w if rot else out_h))
    tol = scale / 16
    bound = math.hypot(60 * 2 * math.pi / 37, 50 * 2 * math.pi / 29) * (tol + 1 / 2048) + (60 * (2 * math.pi / 37) ** 2 + 50 * (2 * math.pi / 29) ** 2) / 8 + 0.75
    assert (got[0] == got[0][..., :1]).all()
    pic = got[0, :out_h, :out_w, 0].astype(np.float64)
    margin = 0.5 + tol + 2.0 ** -10
    inside = (ud >= margin - 0.5) & (ud <= ws - 0.5 - margin) & (vd >= margin - 0.5) & (vd <= hs - 0.5 - margin)   # all four taps are real pixels
    outside = (ud < -margin) | (ud > ws - 1 + margin) | (vd < -margin) | (vd > hs - 1 + margin)
    err = np.abs(pic - wave(ud, vd))[inside].max()
    print(f"{lens[0]} {ws}x{hs} -> {out_w}x{out_h}: {inside.mean():.1%} inside, {outside.mean():.1%} outside, largest distance {err:.3f}, bound {bound:.3f}")
    assert inside.mean() > 0.3 and err <= bound
    assert (pic[outside] == 0).all() and (pic[inside] > 0).all()
    assert (lens == PINCUSHION) == bool(outside.mean() > 0.02)            # only the pincushion lens looks past the source here
    assert not got[0, out_h:].any() and not got[0, :, out_w:].any()


# ---------------------------------------------------------------------------------------------------------------- 4: zero coefficients
@pytest.mark.parametrize("src_hw,canvas,rot", [((186, 246), (96, 120), 0), ((120, 160), (120, 160), 0), ((186, 246), (120, 96), 270)])
def test_zero_coefficients_stay_within_one_grey_level_of_the_plain_path(cpu_lens, src_hw, canvas, rot):
    """A lens that does nothing (new_K = K, coefficients 0) differs from the plain rule only through the nodes' rounding to 2^-16 pixels,
    which can move a coordinate across one 1/2048 step per axis: 2 * 255 / 2048 = 0.25 before rounding, so at most 1 grey level."""
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, src_hw + (3,)).astype(np.uint8)
    K = camera(src_hw[1], src_hw[0], 210.0)
    plain, Kp = ingest_cpu([I.Frame(img, rotate=rot, K=K)], *canvas)
    for n in (4, 5, 8):
        lens, Kl = ingest_cpu([I.Frame(img, rotate=rot, K=K, lens=I.Lens("brown", [0.0] * n, new_K=K))], *canvas)
        d = np.abs(plain.astype(int) - lens.astype(int))
        print(f"{src_hw} -> {canvas} rotate {rot}: {100 * (d > 0).mean():.2f}% of the values differ, by at most {d.max()}")
        assert d.max() <= 1
        np.testing.assert_array_equal(Kl, Kp)


# ---------------------------------------------------------------------------------------------------------------- 5: formats, border, mixed
def lens_frame(rng, h, w, fmt, lens, rot=0, extra=0, matrix="bt601", f=None, tol=1 / 16, lo=0, mv=lambda a: a):
    """A random picture (values lo..255) of the format with a lens (model, coeffs) or None, focal length f (default: 0.62 of the longer side), `extra`
    bytes of row padding (255s); `mv` moves the planes (to a device)."""
    K = camera(w, h, 0.62 * max(w, h) if f is None else f)
    L = None if lens is None else I.Lens(lens[0], lens[1], tol=tol)
    if fmt == "nv12":
        buf = np.full((h * 3 // 2, w + extra), 255, np.uint8)
        buf[:, :w] = rng.randint(lo, 256, (h * 3 // 2, w))
        return I.Frame(mv(buf), fmt, width=w, rotate=rot, K=K, matrix=matrix, lens=L)
    src = rgb_to(rng.randint(lo, 256, (h, w, 3)).astype(np.uint8), fmt, rng)
    return I.Frame(mv(pitched(src, extra)) if extra else mv(src), fmt, width=w, rotate=rot, K=K, lens=L)


def test_every_format_gives_the_picture_of_its_rgb_pixels(cpu_lens):
    rng = np.random.RandomState(5)
    h, w, H, W = 186, 246, 96, 120
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    K = camera(w, h, 150.0)
    for lens in (BARREL, FISHEYE):
        L = I.Lens(*lens)
        ref, Kr = ingest_cpu([I.Frame(img, K=K, lens=L)], H, W)
        assert ref.any()
        for fmt in ("bgr24", "rgba32", "bgra32"):
            got, Kg = ingest_cpu([I.Frame(pitched(rgb_to(img, fmt, rng), 11), fmt, width=w, K=K, lens=L)], H, W)
            np.testing.assert_array_equal(got, ref, err_msg=fmt)
            np.testing.assert_array_equal(Kg, Kr)
        # NV12: every tap is converted before the blend, so the picture is that of the converted pixels
        Yp, U, V = rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h // 2, w // 2)), rng.randint(0, 256, (h // 2, w // 2))
        for matrix in ("bt601", "bt709"):
            CY, CVR, CUG, CVG, CUB = YUV[I.MATRICES[matrix]]
            c = np.maximum(Yp.astype(np.int64) - 16, 0)
            d, e = np.repeat(np.repeat(U, 2, 0), 2, 1) - 128, np.repeat(np.repeat(V, 2, 0), 2, 1) - 128
            rgb = np.clip(np.stack([(CY * c + CVR * e + 2 ** 19) >> 20, (CY * c - CUG * d - CVG * e + 2 ** 19) >> 20,
                                    (CY * c + CUB * d + 2 ** 19) >> 20], -1), 0, 255).astype(np.uint8)
            want, _ = ingest_cpu([I.Frame(rgb, K=K, lens=L)], H, W)
            got, _ = ingest_cpu([I.Frame(nv12_of(Yp, U, V, pitch=w + 10), "nv12", width=w, K=K, lens=L, matrix=matrix)], H, W)
            np.testing.assert_array_equal(got, want, err_msg=matrix)


def test_constant_border_at_both_edges():
    """At a node pixel of a step-2 mesh f = (4 m + 64) >> 7 = (m + 16) >> 5: m = -32768 gives f = -1024 (still the edge pixel, clamped),
    m = -32800 gives -1025 (black); at the far edge of a 5-pixel axis, 4 * 2048 + 1024 = 9216: m = 294912 gives 9216, m = 294944 gives 9217."""
    src = np.arange(1, 5 * 5 * 3 + 1, dtype=np.uint8).reshape(5, 5, 3)
    fr = I.Frame(src)
    centre = 2 * 65536

    def one(mx, my):
        nodes = np.empty((2, 2, 2), np.int32)
        nodes[..., 0], nodes[..., 1] = mx, my
        return run_table(fr, nodes, 1, 4, 4, 1, 1)
    for lo, hi, ax in ((-32768, -32800, 0), (294912, 294944, -1)):
        np.testing.assert_array_equal(one(lo, centre)[0, 0], src[2, ax])
        np.testing.assert_array_equal(one(centre, lo)[0, 0], src[ax, 2])
        assert not one(hi, centre).any() and not one(centre, hi).any()
    full = one(centre + 32768, centre)                                      # half a pixel to the right: the mean of two pixels, rounded up
    np.testing.assert_array_equal(full[0, 0], (src[2, 2].astype(int) + src[2, 3] + 1) // 2)
    assert not full[1:].any() and not full[:, 1:].any()                     # the canvas beyond the 1 x 1 picture is black


def test_plain_and_lens_frames_share_one_launch(cpu_lens, monkeypatch):
    rng = np.random.RandomState(6)
    H, W, B = 96, 120, 9
    kinds = [("rgb24", None), ("nv12", BARREL), ("bgra32", FISHEYE), ("nv12", None), ("bgr24", PINCUSHION), ("rgba32", None), ("rgb24", BARREL)]
    frames = [lens_frame(rng, 2 * rng.randint(40, 120), 2 * rng.randint(40, 120), fmt, lens, rot=90 * (i % 4), extra=7 * (i % 2),
                         matrix=("bt601", "bt709")[i % 2]) for i, (fmt, lens) in enumerate(kinds)]
    slots = [8, 0, 3, 4, 1, 6, 5]
    calls = []
    monkeypatch.setattr(ops, "frame_ingest_mesh", lambda *a: (calls.append("mesh"), np_frame_ingest_mesh(*a))[1])
    monkeypatch.setattr(ops, "frame_ingest", lambda *a: (calls.append("plain"), np_frame_ingest(*a))[1])
    got, Ks = ingest_cpu(frames, H, W, B=B, slots=slots, fill=77)
    assert calls == ["mesh"]
    for f, s in zip(frames, slots):
        np.testing.assert_array_equal(got[s], (np_ingest_lens if f.lens else np_ingest)(f, H, W), err_msg=f"slot {s}")
        np.testing.assert_array_equal(Ks[s], I.plan(f, (H, W))[2].astype(np.float32))
    for s in (2, 7):
        assert (got[s] == 77).all() and (Ks[s] == -7.0).all()
    # without a lens in the call it is the existing entry point; a camera's mesh is built once
    ingest_cpu([f for f in frames if not f.lens], H, W)
    assert calls == ["mesh", "plain"]
    n = len(I._meshes)

    def rebuilt(self, *a):
        raise AssertionError("a cached mesh was built again")
    monkeypatch.setattr(I.Lens, "mesh", rebuilt)
    again, _ = ingest_cpu(frames, H, W, B=B, slots=slots, fill=77)
    np.testing.assert_array_equal(again, got)
    assert len(I._meshes) == n == 4


def test_mesh_cache_is_bounded(cpu_lens, monkeypatch):
    monkeypatch.setattr(I, "MESH_CACHE", 3)
    img = np.zeros((24, 32, 3), np.uint8)
    for k in range(5):
        ingest_cpu([I.Frame(img, K=camera(32, 24, 40.0 + k), lens=I.Lens("brown", (0.01, 0, 0, 0)))], 24, 32)
    assert len(I._meshes) == 3
    assert [np.frombuffer(key[2])[0] for key in I._meshes] == [42.0, 43.0, 44.0]    # least recently used first


def test_new_K_sets_the_pictures_intrinsics(cpu_lens):
    """plan: K' = pixel_map @ new_K; with a new_K of a shorter focal length the picture shows a wider field, so more of it is border."""
    rng = np.random.RandomState(8)
    img = rng.randint(1, 256, (120, 160, 3)).astype(np.uint8)
    K = camera(160, 120, 140.0)
    wide = camera(160, 120, 100.0)
    fr = I.Frame(img, rotate=180, K=K, lens=I.Lens(*PINCUSHION, new_K=wide))
    out_h, out_w, Kp = I.plan(fr, (60, 80))
    np.testing.assert_array_equal(Kp, I.pixel_map(fr, 60, 80) @ wide)
    got, Kt = ingest_cpu([fr], 60, 80)
    np.testing.assert_array_equal(Kt[0], Kp.astype(np.float32))
    np.testing.assert_array_equal(got[0], np_ingest_lens(fr, 60, 80))
    same, _ = ingest_cpu([I.Frame(img, rotate=180, K=K, lens=I.Lens(*PINCUSHION))], 60, 80)
    assert (got[0] == 0).all(-1).mean() > 0.4 > 0.2 > (same[0] == 0).all(-1).mean()


# ---------------------------------------------------------------------------------------------------------------- 6: tracker
@pytest.fixture
def patched_lens(monkeypatch, patched):
    monkeypatch.setattr(ops, "frame_ingest_mesh", np_frame_ingest_mesh)
    I._meshes.clear()
    return patched


def test_tracker_on_lens_frames_is_bit_identical_to_the_undistorted_pictures(scene, patched_lens):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    L = [I.Lens("brown", (-0.12, 0.03, 0.001, -0.0005, 0.0)), I.Lens("fisheye", (0.02, -0.005, 0.0, 0.0))]
    seqs = [[frames[0], frames[1]], [frames[3]]]
    cams = [(Ks[0], L[0]), (Ks[3], L[1])]
    native = [[I.Frame(f, K=K, lens=lens) for f in q] for q, (K, lens) in zip(seqs, cams)]
    flat = [[I.Frame(np_ingest_lens(f, h, w) if f.lens else f.plane0.reshape(h, w, 3), K=f.K) for f in q] for q in native]
    assert any((a.plane0 != b.plane0).any() for a, b in zip(native[0], flat[0]))
    want = T.track_streams(est, flat, batch=2, lanes=1, graphs=False, frame_size=(h, w))
    got = T.track_streams(est, native, batch=2, lanes=1, graphs=False, frame_size=(h, w))
    for (p, s), (gp, gs) in zip(want, got):
        np.testing.assert_array_equal(gp, p)
        np.testing.assert_array_equal(gs, s)
    imgs, Kh = T._ingest_to_host(native[1], (h, w), "cpu")                     # the fallback path of track_streams
    np.testing.assert_array_equal(imgs[0], np_ingest_lens(native[1][0], h, w))
    np.testing.assert_array_equal(Kh[0], np.asarray(Ks[3], np.float64).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- 7: errors
def test_errors():
    z = np.zeros((24, 32, 3), np.uint8)
    K = camera(32, 24, 30.0)
    with pytest.raises(ValueError, match="K"):
        I.Frame(z, lens=I.Lens(*BARREL))
    with pytest.raises(ValueError, match="Lens"):
        I.Frame(z, K=K, lens=BARREL)
    for model, n in (("brown", 3), ("brown", 6), ("brown", 9), ("fisheye", 5), ("fisheye", 3)):
        with pytest.raises(ValueError, match="coefficients"):
            I.Lens(model, [0.0] * n)
    with pytest.raises(ValueError, match="model"):
        I.Lens("division", [0.1])
    with pytest.raises(ValueError, match="tol"):
        I.Lens("brown", [0.0] * 4, tol=0)
    bad = I.Lens("brown", (-0.35, 0.12, 0, 0), tol=1e-6)                          # step 2 cannot reach a millionth of a pixel
    with pytest.raises(ValueError, match="brown.*step 2"):
        bad.mesh(K, 32, 24, 0, 32, 24)
    out, Ko = torch.zeros((1, 24, 32, 3), dtype=torch.uint8), torch.zeros((1, 3, 3))
    with pytest.raises(ValueError, match="step 2"):
        I.ingest_frames([I.Frame(z, K=K, lens=bad)], out, Ko)
    assert not any(k[1] == bad for k in I._meshes)
    with pytest.raises(RuntimeError, match="GPU"):                               # no CPU fallback behind the entry point
        I.ingest_frames([I.Frame(z, K=K, lens=I.Lens("brown", (0.01, 0, 0, 0)))], out, Ko)


# ---------------------------------------------------------------------------------------------------------------- 8: ABI
def test_mesh_descriptor_layout_and_null_tables():
    l = lib.load()
    M = lib.G6dMesh
    assert C.sizeof(M) == l.g6d_sizeof_mesh_desc() == 24
    assert [getattr(M, n).offset for n, _ in M._fields_] == [0, 8, 12, 16, 20]
    assert C.sizeof(lib.G6dFrame) == l.g6d_sizeof_frame_desc() == 96 and l.g6d_abi_version() == 12
    buf = (C.c_uint8 * 96)()
    a = C.addressof(buf)
    assert l.g6d_frame_ingest_mesh(None, a, 1, a, 1, 8, 8, a, None) == -1         # G6D_EINVAL before any HIP call
    assert l.g6d_frame_ingest_mesh(a, None, 1, a, 1, 8, 8, a, None) == -1
    assert l.g6d_frame_ingest_mesh(a, a, -1, a, 1, 8, 8, a, None) == -1
    assert l.g6d_frame_ingest_mesh(a, a, 1, a, 1, 8, 0, a, None) == -1
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_ingest_mesh(torch.zeros(96, dtype=torch.uint8), torch.zeros(24, dtype=torch.uint8), 1, torch.zeros((1, 8, 8, 3), dtype=torch.uint8),
                              torch.zeros((1, 3, 3)))


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_lens_kernel_has_no_scratch(tmp_path):
    """The 64-bit mesh interpolation and the px[] staging stay in registers (compiler metadata; cross-compiles without a GPU)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "ingest.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", "ingest.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    (name, body), = re.findall(r"\.name:\s+(\S*frame_ingest_lens_kernel\S*)\n(.*?)\.wavefront_size", out.read_text(), re.S)
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1)) <= 64, name      # 8 waves per SIMD, as the plain kernel
