"""gen6d_amd.ingest on the CPU.  `np_frame_ingest` restates the integer specification of g6d_frame_ingest (include/gen6d_hip.h, DESIGN.md
§4.17) in numpy, with the signature of ops.frame_ingest: on a CPU device the table's pointers are host addresses, so it reads the planes
the way the kernel does.  Checks the sampling rule against a float64 bilinear, the formats, NV12 conversion, pitch, rotation, `plan`, the
descriptor's layout, and the tracker with `frame_size` on the patched ops (tests/ref_ops.py + this function)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import eval as EV
from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_track_streams_cpu import np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)

YUV = {0: (1220542, 1673527, 409993, 852492, 2116026), 1: (1220542, 1880097, 223347, 558891, 2214593)}


def _axis(t, tgt, src):
    f = np.clip((2 * t.astype(np.int64) + 1) * src * 1024 // tgt - 1024, 0, (src - 1) * 2048)
    i0 = f >> 11
    return i0, np.minimum(i0 + 1, src - 1), f & 2047


def np_ingest_picture(p0, p1, pitch0, pitch1, ws, hs, fmt, rot, matrix, out_w, out_h, H, W):
    """Flat uint8 planes -> the [H,W,3] canvas, by the rules of the header: canvas pixel -> unrotated pixel -> four taps, each converted to
    RGB, blended with 11-bit weights."""
    wt, ht = (out_h, out_w) if rot in (90, 270) else (out_w, out_h)
    Y, X = np.meshgrid(np.arange(out_h), np.arange(out_w), indexing="ij")
    x, y = {0: (X, Y), 90: (Y, ht - 1 - X), 180: (wt - 1 - X, ht - 1 - Y), 270: (wt - 1 - Y, X)}[rot]
    x0, x1, a = _axis(x, wt, ws)
    y0, y1, b = _axis(y, ht, hs)
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
    assert s.max() < 2 ** 32                       # the kernel's 32-bit blend sum
    canvas = np.zeros((H, W, 3), np.uint8)
    canvas[:out_h, :out_w] = (s >> 22).astype(np.uint8)
    return canvas


def np_ingest(frame, H, W):
    """One ingest.Frame (host or device planes) -> [H,W,3] canvas through `plan` and np_ingest_picture."""
    out_h, out_w, _ = I.plan(frame, (H, W))
    host = lambda p: None if p is None else (p.cpu().numpy() if torch.is_tensor(p) else p)
    return np_ingest_picture(host(frame.plane0), host(frame.plane1), frame.pitch, frame.uv_pitch, frame.width, frame.height,
                             I.FORMATS[frame.fmt], frame.rotate, I.MATRICES[frame.matrix], out_w, out_h, H, W)


def np_frame_ingest(table, n, out, K_out):
    """ops.frame_ingest on host memory."""
    size = C.sizeof(lib.G6dFrame)
    ents = (lib.G6dFrame * n).from_buffer_copy(table.numpy()[:n * size].tobytes())
    B, H, W = out.shape[:3]
    view = lambda ptr, nb: np.ctypeslib.as_array((C.c_uint8 * nb).from_address(ptr))
    for e in ents:
        if not 0 <= e.slot < B:
            continue
        nv12 = e.format == 4
        bpp = 1 if nv12 else (4 if e.format >= 2 else 3)
        p0 = view(e.plane0, (e.height - 1) * e.pitch0 + e.width * bpp)
        p1 = view(e.plane1, (e.height // 2 - 1) * e.pitch1 + e.width) if nv12 else None
        out.numpy()[e.slot] = np_ingest_picture(p0, p1, e.pitch0, e.pitch1, e.width, e.height, e.format, e.rotate, e.matrix, e.out_w,
                                                e.out_h, H, W)
        K_out.numpy()[e.slot] = np.asarray(list(e.K), np.float32).reshape(3, 3)
    return out


def ingest_cpu(frames, H, W, B=None, slots=None, fill=0):
    B = len(frames) if B is None else B
    out = torch.full((B, H, W, 3), fill, dtype=torch.uint8)
    K = torch.full((B, 3, 3), -7.0)
    I.ingest_frames(frames, out, K, slots=slots)
    return out.numpy(), K.numpy()


@pytest.fixture
def cpu_ingest(monkeypatch):
    monkeypatch.setattr(ops, "frame_ingest", np_frame_ingest)


def rgb_to(img, fmt, rng=None):
    """[h,w,3] RGB -> the packed format's array (alpha random)."""
    if fmt == "rgb24":
        return img.copy()
    if fmt == "bgr24":
        return img[..., ::-1].copy()
    alpha = (rng or np.random.RandomState(0)).randint(0, 256, img.shape[:2] + (1,)).astype(np.uint8)
    return np.concatenate([img if fmt == "rgba32" else img[..., ::-1], alpha], -1)


def pitched(arr, extra, fill=255):
    """[h,w,c] or [h,bytes] -> a view with `extra` bytes of row padding filled with `fill`."""
    h = arr.shape[0]
    row = arr.reshape(h, -1)
    buf = np.full((h, row.shape[1] + extra), fill, np.uint8)
    buf[:, :row.shape[1]] = row
    return buf


def float_bilinear(img, ht, wt):
    """float64 bilinear with half-pixel centres and edge clamp (cv2.INTER_LINEAR's geometry), unrounded."""
    hs, ws = img.shape[:2]
    fx = np.clip((np.arange(wt) + 0.5) * ws / wt - 0.5, 0, ws - 1)
    fy = np.clip((np.arange(ht) + 0.5) * hs / ht - 0.5, 0, hs - 1)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    a, b = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    im = img.astype(np.float64)
    return ((1 - a) * (1 - b) * im[y0][:, x0] + a * (1 - b) * im[y0][:, x1] + (1 - a) * b * im[y1][:, x0] + a * b * im[y1][:, x1])


# ---------------------------------------------------------------------------------------------------------------- 1: identity, formats, pitch
def test_identity_formats_and_pitch(cpu_ingest):
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    ref, K = ingest_cpu([I.Frame(img)], 37, 53)
    np.testing.assert_array_equal(ref[0], img)
    np.testing.assert_array_equal(K[0], EV.pseudo_K(37, 53))
    for fmt in ("bgr24", "rgba32", "bgra32"):
        src = rgb_to(img, fmt, rng)
        got, _ = ingest_cpu([I.Frame(src, fmt)], 37, 53)
        np.testing.assert_array_equal(got[0], img, err_msg=fmt)
        buf = pitched(src, 13)                                       # row padding of 255s, as a [h, pitch] buffer and as a sliced view
        got, _ = ingest_cpu([I.Frame(buf, fmt, width=53)], 37, 53)
        np.testing.assert_array_equal(got[0], img, err_msg=fmt + " pitched")
        got, _ = ingest_cpu([I.Frame(torch.from_numpy(buf), fmt, width=53, height=37)], 37, 53)
        np.testing.assert_array_equal(got[0], img, err_msg=fmt + " pitched tensor")
    wide = np.full((37, 60, 3), 255, np.uint8)
    wide[:, :53] = img
    f = I.Frame(wide[:, :53])
    assert f.pitch == 180 and f.width == 53
    np.testing.assert_array_equal(ingest_cpu([f], 37, 53)[0][0], img)
    # scaled down from a pitched source: the padding still never shows (the picture stays below 255 everywhere)
    dark = (img // 2)
    got, _ = ingest_cpu([I.Frame(pitched(dark, 9), width=53)], 20, 28)
    assert got[0].max() <= 127
    # a canvas larger than the picture: the remainder is written as 0 over whatever was there
    out, _ = ingest_cpu([I.Frame(img)], 37, 70, fill=9)
    np.testing.assert_array_equal(out[0, :, :53], img)
    assert not out[0, :, 53:].any()


# ---------------------------------------------------------------------------------------------------------------- 2: the sampling rule
@pytest.mark.parametrize("src_hw,canvas", [((960, 1280), (480, 640)), ((1297, 1733), (480, 640)), ((480, 640), (480, 640)),
                                           ((185, 246), (480, 640)), ((487, 651), (480, 640)), ((120, 160), (480, 640)),
                                           ((1080, 1920), (540, 960))])
def test_within_one_grey_level_of_float_bilinear(cpu_ingest, src_hw, canvas):
    """Ratios 0.5, 0.37, 1.0, 2.6, odd sizes.  The bound of 1 grey level is derived: 11-bit weights move a value by less than
    2 * 255 / 2048 = 0.25, the rounding of the result by at most 0.5 (and the float reference's own rounding by 0.5 for the rounded form)."""
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, src_hw + (3,)).astype(np.uint8)
    f = I.Frame(img)
    out_h, out_w, _ = I.plan(f, canvas)
    got, _ = ingest_cpu([f], *canvas)
    ref = float_bilinear(img, out_h, out_w)
    pic = got[0, :out_h, :out_w].astype(np.float64)
    d_raw, d_rnd = np.abs(pic - ref).max(), np.abs(pic - np.rint(ref)).max()
    print(f"{src_hw} -> {out_h}x{out_w}: max distance to the float64 bilinear {d_raw:.3f}, to its rounding {d_rnd:.0f}")
    assert d_raw <= 1.0 and d_rnd <= 1.0
    assert not got[0, out_h:].any() and not got[0, :, out_w:].any()
    if src_hw == canvas:
        np.testing.assert_array_equal(got[0], img)


# ---------------------------------------------------------------------------------------------------------------- 3: NV12
def nv12_of(Y, U, V, pitch=None):
    """Y [h,w], U / V [h/2,w/2] -> one [h*3/2, pitch] buffer."""
    h, w = Y.shape
    pitch = w if pitch is None else pitch
    buf = np.full((h * 3 // 2, pitch), 255, np.uint8)
    buf[:h, :w] = Y
    buf[h:, 0:w:2] = U
    buf[h:, 1:w:2] = V
    return buf


def yuv_formula(Y, U, V, matrix):
    CY, CVR, CUG, CVG, CUB = YUV[matrix]
    c, d, e = max(Y - 16, 0), U - 128, V - 128
    sat = lambda v: min(max(v, 0), 255)
    return (sat((CY * c + CVR * e + 2 ** 19) >> 20), sat((CY * c - CUG * d - CVG * e + 2 ** 19) >> 20), sat((CY * c + CUB * d + 2 ** 19) >> 20))


BT601 = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (81, 90, 240): (254, 0, 0), (145, 54, 34): (0, 255, 1),
         (41, 240, 110): (0, 0, 255), (255, 0, 255): (255, 225, 20), (0, 255, 0): (0, 54, 255)}
# the same colours through the BT.709 constants of the header, by hand from the formula (e.g. (81, 90, 240): c = 65, d = -38, e = 112:
# R = (79335230 + 210570864 + 524288) >> 20 = 276, saturated)
BT709 = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (81, 90, 240): (255, 24, 0), (145, 54, 34): (0, 216, 0),
         (41, 240, 110): (0, 15, 255), (255, 0, 255): (255, 238, 8), (0, 255, 0): (0, 41, 255), (63, 102, 240): (255, 1, 0),
         (173, 42, 26): (0, 255, 1), (32, 240, 118): (1, 0, 255)}


def test_nv12_uniform_colours_and_nearest_chroma(cpu_ingest):
    for matrix, table in (("bt601", BT601), ("bt709", BT709)):
        for (Y, U, V), rgb in table.items():
            assert yuv_formula(Y, U, V, I.MATRICES[matrix]) == rgb, (matrix, Y, U, V)
            buf = nv12_of(np.full((8, 12), Y, np.uint8), np.full((4, 6), U, np.uint8), np.full((4, 6), V, np.uint8), pitch=16)
            for canvas in ((8, 12), (4, 6), (16, 24)):
                got, _ = ingest_cpu([I.Frame(buf, "nv12", width=12, matrix=matrix)], *canvas)
                assert (got[0] == np.asarray(rgb, np.uint8)).all(), (matrix, Y, U, V, canvas)
    # a different colour in every 2x2 block, same size: each pixel takes the chroma of its block and its own luma
    rng = np.random.RandomState(3)
    Y, U, V = rng.randint(0, 256, (10, 14)), rng.randint(0, 256, (5, 7)), rng.randint(0, 256, (5, 7))
    Yp, UVp = Y.astype(np.uint8), np.stack([U, V], -1).astype(np.uint8)
    for matrix in ("bt601", "bt709"):
        want = np.asarray([[yuv_formula(int(Y[y, x]), int(U[y // 2, x // 2]), int(V[y // 2, x // 2]), I.MATRICES[matrix]) for x in range(14)]
                           for y in range(10)], np.uint8)
        one, _ = ingest_cpu([I.Frame(nv12_of(Yp, U, V), "nv12", matrix=matrix)], 10, 14)
        np.testing.assert_array_equal(one[0], want)
        two, _ = ingest_cpu([I.Frame(Yp, "nv12", uv=UVp, matrix=matrix)], 10, 14)       # separate planes, [h/2, w/2, 2] chroma
        np.testing.assert_array_equal(two[0], want)
        dev, _ = ingest_cpu([I.Frame(torch.from_numpy(Yp), "nv12", uv=torch.from_numpy(pitched(UVp, 6)), width=14, matrix=matrix)], 10, 14)
        np.testing.assert_array_equal(dev[0], want)


# ---------------------------------------------------------------------------------------------------------------- 4: rotation
@pytest.mark.parametrize("fmt", ["rgb24", "bgra32", "nv12"])
def test_rotation_is_rot90_of_the_scaled_picture(cpu_ingest, fmt):
    rng = np.random.RandomState(4)
    h, w = 46, 62
    if fmt == "nv12":
        src = rng.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)
    else:
        src = rgb_to(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), fmt, rng)
    plain, _ = ingest_cpu([I.Frame(src, fmt)], 23, 31)                  # the scaled picture, unrotated (ratio 0.5)
    for rot, k in ((90, -1), (180, -2), (270, -3)):
        H, W = (31, 23) if rot != 180 else (23, 31)
        got, _ = ingest_cpu([I.Frame(src, fmt, rotate=rot)], H, W + 3, fill=9)       # the height decides the scale: 3 columns remain
        np.testing.assert_array_equal(got[0, :, :W], np.rot90(plain[0], k), err_msg=f"{fmt} rotate {rot}")
        assert not got[0, :, W:].any()


# ---------------------------------------------------------------------------------------------------------------- 5: plan, K
def test_plan_maps_intrinsics_with_the_pixel_map(cpu_ingest):
    rng = np.random.RandomState(5)
    assert I.canvas_for(960, 1080, 1920) == (540, 960) and I.canvas_for(960, 1080, 1920, rotate=90) == (960, 540)
    assert I.canvas_for(640, 1080, 1920) == (360, 640)
    for rot in (0, 90, 180, 270):
        for (hs, ws), canvas in (((1080, 1920), (540, 960)), ((487, 651), (480, 640)), ((300, 200), (96, 128)), ((3, 2000), (64, 64))):
            K = np.array([[rng.uniform(500, 1500), rng.uniform(-2, 2), rng.uniform(0, ws)], [0, rng.uniform(500, 1500), rng.uniform(0, hs)],
                          [0, 0, 1]])
            f = I.Frame(np.zeros((hs, ws, 3), np.uint8), rotate=rot, K=K)
            out_h, out_w, K2 = I.plan(f, canvas)
            hr, wr = (ws, hs) if rot in (90, 270) else (hs, ws)
            assert out_h <= canvas[0] and out_w <= canvas[1] and (out_h == canvas[0] or out_w == canvas[1])
            assert (out_h, out_w) == ((canvas[0], max(1, canvas[0] * wr // hr)) if canvas[0] * wr <= canvas[1] * hr else
                                      (max(1, canvas[1] * hr // wr), canvas[1]))
            wt, ht = (out_h, out_w) if rot in (90, 270) else (out_w, out_h)
            pts = rng.uniform(-1, 1, (50, 3)) + [0, 0, 4]
            uvw = pts @ K.T
            u, v = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
            x, y = (u + 0.5) * wt / ws - 0.5, (v + 0.5) * ht / hs - 0.5            # the scaled picture
            X, Y = {0: (x, y), 90: (ht - 1 - y, x), 180: (wt - 1 - x, ht - 1 - y), 270: (y, wt - 1 - x)}[rot]
            q = pts @ K2.T
            np.testing.assert_allclose(q[:, 0] / q[:, 2], X, rtol=0, atol=1e-9)
            np.testing.assert_allclose(q[:, 1] / q[:, 2], Y, rtol=0, atol=1e-9)
            _, Kt = ingest_cpu([f], *canvas)
            np.testing.assert_array_equal(Kt[0], K2.astype(np.float32))           # rounded once
            g = I.Frame(np.zeros((hs, ws, 3), np.uint8), rotate=rot)
            oh, ow, Kp = I.plan(g, canvas)
            assert (oh, ow) == (out_h, out_w)
            np.testing.assert_array_equal(Kp.astype(np.float32), EV.pseudo_K(out_h, out_w))
    # the corner pixel centres of the source land on the corner pixel centres' images: consistency of the map with the rotation of test 4
    f = I.Frame(np.zeros((40, 60, 3), np.uint8), rotate=90, K=np.eye(3))
    A = I.pixel_map(f, 60, 40)
    np.testing.assert_allclose(A @ [0, 0, 1], [39, 0, 1], atol=1e-12)            # top-left -> top-right
    np.testing.assert_allclose(A @ [59, 0, 1], [39, 59, 1], atol=1e-12)          # top-right -> bottom-right


# ---------------------------------------------------------------------------------------------------------------- 6: tracker
@pytest.fixture
def patched(monkeypatch, cpu_ingest):
    ref_ops.patch_ops(monkeypatch)
    monkeypatch.setattr(ops, "track_gather", np_track_gather)
    monkeypatch.setattr(ops, "track_commit", np_track_commit)
    calls = []
    monkeypatch.setattr(ops, "frame_ingest", lambda table, n, out, K_out: (calls.append((n, tuple(out.shape))), np_frame_ingest(table, n, out, K_out))[1])
    return calls


def test_tracker_with_canvas_sized_frames_is_bit_identical(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    seqs = [[frames[0], frames[1], frames[2]], [frames[2], frames[3]], [frames[3], frames[1], frames[0]]]
    plain = T.track_streams(est, seqs, [Ks[0], None, Ks[3]], batch=2, lanes=2, graphs=False)
    assert not patched
    native = [[I.Frame(f, K=Ks[0]) for f in seqs[0]], seqs[1], [I.Frame(torch.from_numpy(f), K=Ks[3]) for f in seqs[2]]]
    got = T.track_streams(est, native, batch=2, lanes=2, graphs=False, frame_size=(h, w))
    for (p, s), (gp, gs) in zip(plain, got):
        np.testing.assert_array_equal(gp, p)
        np.testing.assert_array_equal(gs, s)
    # tick 0: one init batch per group (2 and 1 first frames); ticks 1 and 2: one ingest per lane with work, into the lane's 2 slots
    assert patched == [(2, (2, h, w, 3)), (1, (1, h, w, 3)), (2, (2, h, w, 3)), (1, (2, h, w, 3)), (1, (2, h, w, 3)), (1, (2, h, w, 3))]


def test_tracker_mixed_formats_subsets_and_reset(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    rng = np.random.RandomState(6)
    big = lambda f: np.repeat(np.repeat(f, 2, 0), 2, 1)                              # a 2x larger source of the same picture

    def native(i, kind):
        f = frames[i]
        if kind == "bgra2x":
            return I.Frame(pitched(rgb_to(big(f), "bgra32", rng), 20), "bgra32", width=2 * w)
        if kind == "nv12":
            g = f.astype(np.int64)
            Y = ((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16
            return I.Frame(nv12_of(Y.astype(np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)), "nv12")
        if kind == "rot":
            return I.Frame(np.ascontiguousarray(np.rot90(f, 1)), rotate=90)          # stored turned left, turned back on ingest
        return f

    tr = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False, frame_size=(h, w))
    chain = est.device_chain()
    it = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    push = [(0, native(0, "bgra2x")), (1, native(1, "nv12")), (3, native(2, "rot"))]
    tr.push([s for s, _ in push], [f for _, f in push])
    r0 = tr.result()
    assert set(r0) == {0, 1, 3} and len(patched) == 2
    np.testing.assert_array_equal(np_ingest(native(2, "rot"), h, w), frames[2])       # the turned-back picture is the frame itself
    # a subset push: stream 1's tracked frame is one chain step on the numpy-ingested image with the pseudo K of the picture
    del patched[:]
    f1 = native(3, "bgra2x")
    tr.push([1], [f1])
    r1 = tr.result([1])
    assert patched == [(1, (2, h, w, 3))]
    img = np_ingest(f1, h, w)
    np.testing.assert_array_equal(tr._lanes[0].img[1].numpy(), img)
    one = chain.query(it(img), it(EV.pseudo_K(h, w)), pose_init=it(r0[1][0]), refine_iter=1)["pose"].numpy()
    np.testing.assert_allclose(r1[1][0], one, atol=2e-4)
    np.testing.assert_array_equal(tr.result([0])[0][0], r0[0][0])
    tr.reset([3])
    tr.push([0, 3], [native(1, "nv12"), frames[3]])
    r2 = tr.result()
    full = chain.query(it(frames[3]), it(EV.pseudo_K(h, w)))["pose"].numpy()
    np.testing.assert_allclose(r2[3][0], full, atol=2e-4)
    assert int(tr.hist_count[3]) == 1 and int(tr.hist_count[0]) == 2


def test_fallback_path_reads_ingested_frames_back(cpu_ingest):
    """track_streams' range-guard fallback (host_track) takes plain arrays: each frame through the ingest, read back."""
    rng = np.random.RandomState(7)
    K = np.array([[800.0, 0, 60], [0, 800.0, 40], [0, 0, 1]])
    fr = [I.Frame(rgb_to(rng.randint(0, 256, (80, 120, 3)).astype(np.uint8), "bgra32", rng), "bgra32", K=K),
          rng.randint(0, 256, (40, 60, 3)).astype(np.uint8)]
    imgs, Ks = T._ingest_to_host(fr, (40, 60), "cpu")
    np.testing.assert_array_equal(imgs[0], np_ingest(fr[0], 40, 60))
    np.testing.assert_array_equal(imgs[1], fr[1])
    np.testing.assert_array_equal(Ks[0], I.plan(fr[0], (40, 60))[2].astype(np.float32))
    np.testing.assert_array_equal(Ks[1], EV.pseudo_K(40, 60))


def test_errors(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    z = np.zeros
    with pytest.raises(ValueError, match="even"):
        I.Frame(z((15, 11), np.uint8), "nv12", width=11, height=10)
    with pytest.raises(ValueError, match="even"):
        I.Frame(z((7, 12), np.uint8), "nv12", uv=z((3, 12), np.uint8))
    with pytest.raises(ValueError, match="pitch"):
        I.Frame(z((10, 20), np.uint8), "rgb24", width=7)
    with pytest.raises(ValueError, match="pitch"):
        I.Frame(z(1000, np.uint8), "bgra32", width=8, height=8, pitch=31)
    with pytest.raises(ValueError, match="format"):
        I.Frame(z((4, 4, 3), np.uint8), "yuyv")
    with pytest.raises(ValueError, match="rotate"):
        I.Frame(z((4, 4, 3), np.uint8), rotate=45)
    with pytest.raises(ValueError, match="outside"):
        I.Frame(z((2, 8193, 3), np.uint8))
    with pytest.raises(ValueError, match="outside"):
        I.Frame(z(0, np.uint8), width=0, height=4)
    with pytest.raises(ValueError, match="holds"):
        I.Frame(z(100, np.uint8), width=8, height=8)
    with pytest.raises(ValueError, match="uint8"):
        I.Frame(z((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        I.Frame(z((4, 4, 3), np.uint8), "rgba32")
    with pytest.raises(ValueError, match="matrix"):
        I.Frame(z((6, 4), np.uint8), "nv12", matrix="bt2020")
    out, K = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 3, 3))
    with pytest.raises(ValueError, match="slot"):
        I.ingest_frames([I.Frame(z((4, 4, 3), np.uint8))] * 2, out, K, slots=[1, 1])
    with pytest.raises(ValueError, match="slot"):
        I.ingest_frames([I.Frame(z((4, 4, 3), np.uint8))], out, K, slots=[2])
    tr = T.StreamTracker(est, 4, batch=2, graphs=False, frame_size=(h, w))
    with pytest.raises(ValueError, match="Frame.K"):
        tr.push([0], [frames[0]], [Ks[0]])
    with pytest.raises(ValueError, match="Frame.K"):
        T.track_streams(est, [[frames[0]]], [Ks[0]], graphs=False, frame_size=(h, w))
    with pytest.raises(ValueError):
        tr.push([0], [frames[0].astype(np.float32)])
    with pytest.raises(ValueError):
        T.StreamTracker(est, 4, batch=2, graphs=False, frame_size=(0, 5))
    old = T.StreamTracker(est, 4, batch=2, graphs=False)                       # without frame_size: today's message for another shape
    old.push([1], [frames[0]])
    with pytest.raises(ValueError, match="differs from the tracker's"):
        old.push([2], [np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(ValueError):
        old.push([2], [I.Frame(frames[0])])


# ---------------------------------------------------------------------------------------------------------------- 7: ABI
def test_descriptor_layout_and_null_table():
    l = lib.load()
    F = lib.G6dFrame
    assert C.sizeof(F) == l.g6d_sizeof_frame_desc() == 96
    assert [getattr(F, n).offset for n, _ in F._fields_] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56]
    assert l.g6d_frame_ingest(None, 1, None, 1, 8, 8, None, None) == -1            # G6D_EINVAL before any HIP call
    buf = (C.c_uint8 * 96)()
    assert l.g6d_frame_ingest(C.addressof(buf), -1, C.addressof(buf), 1, 8, 8, C.addressof(buf), None) == -1
    assert l.g6d_frame_ingest(C.addressof(buf), 1, C.addressof(buf), 1, 0, 8, C.addressof(buf), None) == -1
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_ingest(torch.zeros(96, dtype=torch.uint8), 1, torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 3, 3)))


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_has_no_scratch(tmp_path):
    """The px[] staging of a thread's 12 output bytes must stay in registers (compiler metadata; cross-compiles without a GPU)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "ingest.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", "ingest.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    (name, body), = re.findall(r"\.name:\s+(\S*frame_ingest_kernel\S*)\n(.*?)\.wavefront_size", out.read_text(), re.S)
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1)) <= 64, name      # 8 waves per SIMD
