"""g6d_frame_crop's rule (include/gen6d_hip.h) restated in numpy, and the host logic around it.
1: the restatement against an independent oracle: the project's reference warp run on the source picture converted to RGB per pixel, under
   the crop homography composed with the inverse of `ingest.pixel_map`, which the ingest and emit tests pin; every format and rotation.
2: a same-size source gives the canvas crop.  3: slots without a source are the reference warp of their canvas.
4: the tracker with crops="source" on patched ops: errors, same-size frames against the canvas mode, the lens fallback, and which slots
   of which launches carry a source record."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_ingest_cpu import YUV, np_frame_ingest, np_ingest, np_ingest_picture, nv12_of, pitched, rgb_to
from test_ingest_lens_cpu import np_frame_ingest_mesh
from test_track_streams_cpu import np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)


def _host(p):
    return None if p is None else np.asarray(p.cpu().numpy() if torch.is_tensor(p) else p)


def records_of_frames(frames, H, W):
    """ingest.Frame objects with host (or device) planes -> what the rule reads of their G6dFrame records, planned for an H x W canvas."""
    out = []
    for f in frames:
        out_h, out_w, _ = I.plan(f, (H, W))
        out.append(types.SimpleNamespace(p0=_host(f.plane0), p1=_host(f.plane1), pitch0=f.pitch, pitch1=f.uv_pitch, width=f.width,
                                         height=f.height, format=I.FORMATS[f.fmt], rotate=f.rotate, matrix=I.MATRICES[f.matrix],
                                         out_w=out_w, out_h=out_h))
    return out


def records_of_table(table):
    """A frame table in HOST memory (torch uint8) -> the same, read the way test_ingest_cpu.np_frame_ingest reads it."""
    size = C.sizeof(lib.G6dFrame)
    n = table.numel() // size
    view = lambda ptr, nb: np.ctypeslib.as_array((C.c_uint8 * nb).from_address(ptr))
    out = []
    for e in (lib.G6dFrame * n).from_buffer_copy(table.numpy()[:n * size].tobytes()):
        if not e.plane0:                               # a record nobody filled (the tracker's static table before its first tick)
            out.append(None)
            continue
        nv12 = e.format == 4
        bpp = 1 if nv12 else (4 if e.format >= 2 else 3)
        out.append(types.SimpleNamespace(p0=view(e.plane0, (e.height - 1) * e.pitch0 + e.width * bpp),
                                         p1=view(e.plane1, (e.height // 2 - 1) * e.pitch1 + e.width) if nv12 else None, pitch0=e.pitch0,
                                         pitch1=e.pitch1, width=e.width, height=e.height, format=e.format, rotate=e.rotate,
                                         matrix=e.matrix, out_w=e.out_w, out_h=e.out_h))
    return out


def _tap_rgb(e, xi, yi):
    """The ingest's tap rule at integer source positions -> int64 [..., 3]."""
    p0 = e.p0.astype(np.int64)
    if e.format == 4:
        uv = e.p1.astype(np.int64)
        CY, CVR, CUG, CVG, CUB = YUV[e.matrix]
        c = np.maximum(p0[yi * e.pitch0 + xi] - 16, 0)
        d = uv[(yi >> 1) * e.pitch1 + (xi >> 1) * 2] - 128
        v = uv[(yi >> 1) * e.pitch1 + (xi >> 1) * 2 + 1] - 128
        ch = [(CY * c + CVR * v + 2 ** 19) >> 20, (CY * c - CUG * d - CVG * v + 2 ** 19) >> 20, (CY * c + CUB * d + 2 ** 19) >> 20]
        return np.clip(np.stack(ch, -1), 0, 255)
    bpp, ro = (4 if e.format >= 2 else 3), (2 if e.format in (1, 3) else 0)
    o = yi * e.pitch0 + xi * bpp
    return np.stack([p0[o + ro], p0[o + 1], p0[o + 2 - ro]], -1)


def np_crop(records, rec, imgs, hinv, dh, dw, dtype=np.float32):
    """The header's rule, every operation in `dtype` -> [B,3,dh,dw] of that dtype.  records: records_of_frames / records_of_table; imgs
    uint8 [B,H,W,3] and hinv float32 [B,9] as numpy arrays."""
    ft = np.dtype(dtype).type
    B, H, W = imgs.shape[:3]
    y, x = np.meshgrid(np.arange(dh).astype(ft), np.arange(dw).astype(ft), indexing="ij")
    out = np.zeros((B, 3, dh, dw), ft)
    for b in range(B):
        h = np.asarray(hinv[b], np.float32).reshape(9).astype(ft)
        X, Y, Wd = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]
        with np.errstate(divide="ignore", invalid="ignore"):
            iw = np.where(Wd != 0, ft(1) / Wd, ft(0))
            cx, cy = X * iw, Y * iw                                                        # 1
        r = int(rec[b])
        if r < 0:                                      # no source: g6d_warp_batch's rule on the slot's canvas
            sw, sh, fx, fy = W, H, cx, cy
            flat = imgs[b].reshape(-1).astype(np.int64)
            tap = lambda xi, yi: np.stack([flat[(yi * W + xi) * 3 + c] for c in range(3)], -1)
        else:
            e = records[r]
            sw, sh = e.width, e.height
            wt, ht = (e.out_h, e.out_w) if e.rotate in (90, 270) else (e.out_w, e.out_h)
            px, py = {0: (cx, cy), 90: (cy, ft(ht - 1) - cx), 180: (ft(wt - 1) - cx, ft(ht - 1) - cy), 270: (ft(wt - 1) - cy, cx)}[e.rotate]   # 2
            with np.errstate(divide="ignore", invalid="ignore"):
                ax, ay = ft(sw) / ft(wt), ft(sh) / ft(ht)
                # 3: one fused multiply-add per axis.  A product of two float32 values is exact in float64, so the float32 rule is
                # evaluated there and rounded to float32 once more (float64 itself has nothing wider to fuse in: plain operations)
                fma = lambda p, a, b: (p.astype(np.float64) * np.float64(a) + np.float64(b)).astype(ft)
                fx, fy = fma(px, ax, ft(0.5) * ax - ft(0.5)), fma(py, ay, ft(0.5) * ay - ft(0.5))
            tap = lambda xi, yi, e=e: _tap_rgb(e, xi, yi)
        fx, fy = np.fmin(np.fmax(fx, ft(-4)), ft(sw + 4)), np.fmin(np.fmax(fy, ft(-4)), ft(sh + 4))   # 4 (a NaN becomes -4, as fmaxf makes it)
        x0f, y0f = np.floor(fx), np.floor(fy)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        a, bb = fx - x0f, fy - y0f
        vx0, vx1, vy0, vy1 = (x0 >= 0) & (x0 < sw), (x0 + 1 >= 0) & (x0 + 1 < sw), (y0 >= 0) & (y0 < sh), (y0 + 1 >= 0) & (y0 + 1 < sh)
        xc0, xc1, yc0, yc1 = np.clip(x0, 0, sw - 1), np.clip(x0 + 1, 0, sw - 1), np.clip(y0, 0, sh - 1), np.clip(y0 + 1, 0, sh - 1)
        one = ft(1)
        w00, w01 = np.where(vx0 & vy0, (one - a) * (one - bb), 0), np.where(vx1 & vy0, a * (one - bb), 0)
        w10, w11 = np.where(vx0 & vy1, (one - a) * bb, 0), np.where(vx1 & vy1, a * bb, 0)
        v = (w00[..., None] * tap(xc0, yc0).astype(ft) + w01[..., None] * tap(xc1, yc0).astype(ft) + w10[..., None] * tap(xc0, yc1).astype(ft) +
             w11[..., None] * tap(xc1, yc1).astype(ft))                                    # 5, 6
        assert v.dtype == ft
        out[b] = (np.clip(np.rint(v), 0, 255) / ft(255)).transpose(2, 0, 1)
    return out


def np_frame_crop(table, rec, imgs, hinv, dh, dw, out=None, dtype=np.float32):
    """ops.frame_crop on host memory."""
    r = torch.from_numpy(np_crop(records_of_table(table), rec.numpy(), imgs.numpy(), hinv.reshape(-1, 9).numpy(), dh, dw, dtype).astype(np.float32))
    if out is not None:
        out.copy_(r)
        return out
    return r


def warp_rule(got, want, what):
    """test_glue_edges_gpu._warp_rule on grey levels: at most 1 level, fewer than 1 % of the values off by more than 1/2."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    print(f"{what}: max {d.max():.3f} levels, {100 * (d > 0.5).mean():.3f} % off by more than 1/2")
    assert d.max() <= 1.001 and (d > 0.5).mean() < 0.01, what


def homographies(rng, n, zoom=(0.6, 1.4), shift=(-10, 30)):
    """test_glue_edges_gpu._homographies: crop -> canvas maps, float32 [n,9]; the crop magnifies the canvas `zoom` times."""
    hinv = []
    for _ in range(n):
        a, s = rng.uniform(-0.6, 0.6), rng.uniform(*zoom)
        M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(*shift)], [s * np.sin(a), s * np.cos(a), rng.uniform(*shift)],
                      [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])
        hinv.append(np.linalg.inv(M).reshape(9))
    return np.asarray(hinv, np.float32)


def source_frame(rng, h, w, fmt, rotate=0, extra=0, matrix="bt601", split=False, mv=lambda a: a):
    """A noise picture of the format as a Frame with `extra` bytes of row padding; nv12 as one buffer or (split) as two planes."""
    if fmt == "nv12":
        buf = np.full((h * 3 // 2, w + extra), 255, np.uint8)
        buf[:, :w] = rng.randint(0, 256, (h * 3 // 2, w))
        if split:
            return I.Frame(mv(np.ascontiguousarray(buf[:h])), fmt, width=w, uv=mv(np.ascontiguousarray(buf[h:])), rotate=rotate, matrix=matrix)
        return I.Frame(mv(buf), fmt, width=w, rotate=rotate, matrix=matrix)
    src = rgb_to(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), fmt, rng)
    return I.Frame(mv(pitched(src, extra)), fmt, width=w, rotate=rotate) if extra else I.Frame(mv(src), fmt, rotate=rotate)


def source_rgb(frame):
    """The source picture converted to RGB per pixel by the ingest's tap rule: the same-size, unturned ingest."""
    e = records_of_frames([frame], frame.height, frame.width)[0]
    return np_ingest_picture(e.p0, e.p1, e.pitch0, e.pitch1, e.width, e.height, e.format, 0, e.matrix, e.width, e.height, e.height, e.width)


def oracle(frame, H, W, hinv, dh, dw):
    """The reference warp in float64 on the source's RGB picture under inv(pixel_map) @ hinv -> [n,3,dh,dw] grey levels."""
    out_h, out_w, _ = I.plan(frame, (H, W))
    A = np.linalg.inv(I.pixel_map(frame, out_h, out_w))
    full = np.stack([A @ np.asarray(h, np.float64).reshape(3, 3) for h in hinv]).reshape(-1, 9)
    rgb = torch.from_numpy(source_rgb(frame))
    return ref_ops.warp_batch(None, rgb, None, torch.from_numpy(full), dh, dw, dtype=torch.float64).numpy() * 255


# ---------------------------------------------------------------------------------------------------------------- 1: independent oracle
@pytest.mark.parametrize("rot", [0, 90, 180, 270])
@pytest.mark.parametrize("fmt", ["rgb24", "bgr24", "rgba32", "bgra32", "nv12"])
def test_rule_matches_the_reference_warp_of_the_source(fmt, rot):
    rng = np.random.RandomState(10 + rot)
    hs, ws = (26, 38) if fmt == "nv12" else (23, 37)
    dh, dw = 20, 28
    for div in (2.0, 3.7):                             # the canvas is 2x to 3.7x smaller than the source
        hr, wr = (ws, hs) if rot in (90, 270) else (hs, ws)
        H, W = -int(-hr // div), -int(-wr // div)
        f = source_frame(rng, hs, ws, fmt, rot, extra=5, matrix=("bt601", "bt709")[rot == 180], split=rot == 270)
        out_h, out_w, _ = I.plan(f, (H, W))
        assert 1.9 < max(hr, wr) / max(out_h, out_w) < 3.9
        hinv = homographies(rng, 3, zoom=(1.5, 4.0), shift=(-2, 6))
        imgs = np.zeros((3, H, W, 3), np.uint8)        # not read: every slot has a source
        got = np_crop(records_of_frames([f], H, W), [0, 0, 0], imgs, hinv, dh, dw, np.float64) * 255
        want = oracle(f, H, W, hinv, dh, dw)
        outside = (want == 0).all(1).mean()
        assert 0.02 < outside < 0.9, outside           # part of every crop set looks past the source's edge
        warp_rule(got, want, f"{fmt} rotate {rot} 1/{div}")


# ---------------------------------------------------------------------------------------------------------------- 2: same-size sources
@pytest.mark.parametrize("rot", [0, 90])
@pytest.mark.parametrize("fmt", ["rgb24", "nv12"])
def test_same_size_source_gives_the_canvas_crop(fmt, rot):
    rng = np.random.RandomState(20 + rot)
    hs, ws = 26, 38
    H, W = (ws, hs) if rot == 90 else (hs, ws)
    f = source_frame(rng, hs, ws, fmt, rot, extra=3)
    canvas = np_ingest(f, H, W)
    hinv = homographies(rng, 4, zoom=(1.5, 4.0), shift=(-3, 12))
    imgs = np.zeros((4, H, W, 3), np.uint8)
    got = np_crop(records_of_frames([f], H, W), [0] * 4, imgs, hinv, 20, 28, np.float64) * 255
    want = ref_ops.warp_batch(None, torch.from_numpy(canvas), None, torch.from_numpy(hinv), 20, 28, dtype=torch.float64).numpy() * 255
    assert (want > 0).mean() > 0.3
    warp_rule(got, want, f"same size {fmt} rotate {rot}")
    if rot == 0:                                       # unturned, the float32 coordinates are the canvas path's own: fx = px * 1 + 0
        np.testing.assert_array_equal(np_crop(records_of_frames([f], H, W), [0] * 4, imgs, hinv, 20, 28),
                                      np_crop([], [-1] * 4, np.stack([canvas] * 4), hinv, 20, 28))


# ---------------------------------------------------------------------------------------------------------------- 3: slots without a source
def test_slots_without_a_source_are_the_reference_warp_of_their_canvas():
    rng = np.random.RandomState(30)
    H, W, dh, dw = 32, 48, 20, 28
    imgs = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    f = source_frame(rng, 26, 38, "nv12")
    hinv = homographies(rng, 3)
    got = np_crop(records_of_frames([f], H, W), [-1, 0, -1], imgs, hinv, dh, dw, np.float64)
    want = ref_ops.warp_batch(torch.from_numpy(imgs), None, torch.arange(3, dtype=torch.int32), torch.from_numpy(hinv), dh, dw,
                              dtype=torch.float64).numpy()
    # float64 on both sides: the two evaluations differ in the last bits of v, which no uint8 rounding of these inputs sees
    np.testing.assert_array_equal(got[[0, 2]], want[[0, 2]])
    assert (got[1] != want[1]).mean() > 0.2            # ... while the slot with a record shows its source


# ---------------------------------------------------------------------------------------------------------------- 4: tracker
@pytest.fixture
def patched(monkeypatch):
    """Every op on its host reference; returns the list of (rec, dh) of the frame_crop calls."""
    ref_ops.patch_ops(monkeypatch)
    monkeypatch.setattr(ops, "track_gather", np_track_gather)
    monkeypatch.setattr(ops, "track_commit", np_track_commit)
    monkeypatch.setattr(ops, "frame_ingest", np_frame_ingest)
    monkeypatch.setattr(ops, "frame_ingest_mesh", np_frame_ingest_mesh)
    calls = []

    def crop(table, rec, imgs, hinv, dh, dw, out=None):
        calls.append((rec.numpy().copy(), dh))
        return np_frame_crop(table, rec, imgs, hinv, dh, dw, out)
    monkeypatch.setattr(ops, "frame_crop", crop)
    return calls


def native2x(frame, kind):
    """test_ingest_gpu._native: a scene frame [h,w,3] -> a 2x larger camera-style Frame of the same picture, built on the host."""
    big = np.repeat(np.repeat(frame, 2, 0), 2, 1)
    w = big.shape[1]
    if kind == "bgra":
        return I.Frame(pitched(rgb_to(big, "bgra32"), 24), "bgra32", width=w)
    g = frame.astype(np.int64)                          # BT.601 limited range, one chroma sample per original pixel = per 2x2 block
    Y = ((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16
    U = ((-38 * g[..., 0] - 74 * g[..., 1] + 112 * g[..., 2] + 128) >> 8) + 128
    V = ((112 * g[..., 0] - 94 * g[..., 1] - 18 * g[..., 2] + 128) >> 8) + 128
    Yb = np.repeat(np.repeat(Y, 2, 0), 2, 1)
    return I.Frame(nv12_of(Yb.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8), pitch=w + 32), "nv12", width=w)


def test_tracker_option_errors(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    with pytest.raises(ValueError, match="frame_size"):
        T.StreamTracker(est, 2, batch=2, graphs=False, crops="source")
    with pytest.raises(ValueError, match="crops"):
        T.StreamTracker(est, 2, batch=2, graphs=False, frame_size=(h, w), crops="native")
    with pytest.raises(ValueError, match="crops"):
        T.track_streams(est, [[frames[0]]], batch=2, graphs=False, frame_size=(h, w), crops=None)
    assert not patched


def test_tracker_same_size_frames_match_canvas_mode(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    seqs = [[frames[0], frames[1], frames[2]], [frames[2], frames[3]], [frames[3], frames[1], frames[0]]]
    native = [[I.Frame(f, K=Ks[0]) for f in seqs[0]], seqs[1], [I.Frame(torch.from_numpy(f), K=Ks[3]) for f in seqs[2]]]
    canvas = T.track_streams(est, native, batch=2, lanes=2, graphs=False, frame_size=(h, w))
    assert not patched                                 # the default mode launches what it launched
    source = T.track_streams(est, native, batch=2, lanes=2, graphs=False, frame_size=(h, w), crops="source")
    assert patched
    for (p, s), (gp, gs) in zip(canvas, source):
        np.testing.assert_allclose(gp, p, atol=3e-4)
        np.testing.assert_allclose(gs, s, atol=3e-4)


def test_tracker_serves_a_lens_frame_from_the_canvas(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    lens = I.Lens("brown", (0.05, -0.01, 0.0, 0.0))
    K = np.asarray(Ks[0], np.float64)
    tr = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, frame_size=(h, w), crops="source")
    for t in range(2):
        tr.push([0, 1], [I.Frame(frames[t], K=K, lens=lens), I.Frame(frames[t + 1], K=K)])
    r = tr.result()
    assert all(np.isfinite(r[s][0]).all() for s in (0, 1))
    assert len(patched) == 1 + est.cfg["refine_iter"] + 1      # selector crop + the first frames' steps, then one tracked step
    for rec, _ in patched:
        np.testing.assert_array_equal(rec, [-1, 1])    # record 1 is stream 1's frame; the lens frame keeps its canvas crop
    # the lens stream's tracked pose is the step on its (undistorted) canvas, as in canvas mode
    ref = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, frame_size=(h, w))
    for t in range(2):
        ref.push([0, 1], [I.Frame(frames[t], K=K, lens=lens), I.Frame(frames[t + 1], K=K)])
    np.testing.assert_allclose(r[0][0], ref.result()[0][0], atol=3e-4)


def test_tracker_launches_one_crop_per_step_with_the_pushed_slots(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    steps, size, rs = est.cfg["refine_iter"], est.device_chain().size, est.device_chain().refine_size
    tr = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False, frame_size=(h, w), crops="source", track_iter=2)
    tr.push([0, 1, 2], [native2x(frames[0], "nv12"), native2x(frames[1], "bgra"), native2x(frames[2], "nv12")])
    # first frames: per init chunk (streams 0 and 1; stream 2) the selector crop and one crop per refinement step, every slot with a record
    want = [([0, 1], size)] + [([0, 1], rs)] * steps + [([0], size)] + [([0], rs)] * steps
    assert [(list(r), d) for r, d in patched] == want
    del patched[:]
    tr.push([1, 2], [native2x(frames[2], "bgra"), native2x(frames[3], "bgra")])
    # tracked frames: track_iter crops per lane; a slot nobody pushed has no record (stream 1 is slot 1 of lane 0, stream 2 slot 0 of lane 1)
    assert [(list(r), d) for r, d in patched] == [([-1, 0], rs)] * 2 + [([0, -1], rs)] * 2
    r = tr.result()
    assert set(r) == {0, 1, 2} and all(np.isfinite(r[s][0]).all() for s in r)
    # stream 1's tracked frame is two eager steps of query_batch from its first pose, with the same source
    first = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False, frame_size=(h, w), crops="source")
    first.push([0, 1], [native2x(frames[0], "nv12"), native2x(frames[1], "bgra")])
    p0 = first.result()[1][0]
    img, K = torch.empty((1, h, w, 3), dtype=torch.uint8), torch.empty((1, 3, 3))
    staged = I.ingest_frames_keep([native2x(frames[2], "bgra")], img, K)[1]
    one = est.device_chain().query_batch_source(img, K, I.SourceTable.of(staged), pose_init=torch.from_numpy(p0)[None], refine_iter=2)
    np.testing.assert_allclose(r[1][0], one["pose"][0].numpy(), atol=3e-4)


def test_track_streams_recomputes_a_left_window_with_eager_source_ticks(scene, patched, monkeypatch):
    """The range guard's recompute path in "source" mode: the same ticks once more, eager, with the refiner's pair routes off."""
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    native = [[native2x(frames[0], "nv12"), native2x(frames[1], "bgra")]]
    want = T.track_streams(est, native, batch=2, lanes=1, graphs=False, frame_size=(h, w), crops="source")
    del patched[:]
    built, left = [], [True]
    init = T.StreamTracker.__init__

    def recorded(self, *a, **k):
        built.append((k.get("graphs"), k.get("crops"), bool(getattr(est.refiner, "_pairs_off", False))))
        init(self, *a, **k)
    monkeypatch.setattr(T.StreamTracker, "__init__", recorded)
    monkeypatch.setattr(est.refiner, "range_check", lambda: left.pop() if left else False)      # the window is left once
    got = T.track_streams(est, native, batch=2, lanes=1, graphs=False, frame_size=(h, w), crops="source")
    assert built == [(False, "source", False), (False, "source", True)]
    assert len(patched) == 2 * (1 + est.cfg["refine_iter"] + 1)        # both runs cut every crop from the source
    assert not getattr(est.refiner, "_pairs_off", False)
    for (p, s), (gp, gs) in zip(want, got):
        np.testing.assert_allclose(gp, p, atol=3e-4)
        np.testing.assert_allclose(gs, s, atol=3e-4)
    with pytest.raises(ValueError, match="record 1"):
        I.SourceTable._upload(np.array([0, 1, -1], np.int32), 1, torch.device("cpu"))


# ---------------------------------------------------------------------------------------------------------------- 5: ABI, compiler metadata
def test_launcher_rejects_null_and_empty_arguments():
    l = lib.load()
    buf = (C.c_uint8 * 96)()
    p = C.addressof(buf)
    for args in ((None, p, p, 1, 8, 8, p, p, 4, 4), (p, None, p, 1, 8, 8, p, p, 4, 4), (p, p, None, 1, 8, 8, p, p, 4, 4),
                 (p, p, p, 1, 8, 8, None, p, 4, 4), (p, p, p, 1, 8, 8, p, None, 4, 4), (p, p, p, 0, 8, 8, p, p, 4, 4),
                 (p, p, p, 1, 0, 8, p, p, 4, 4), (p, p, p, 1, 8, 8, p, p, 0, 4), (p, p, p, 1, 8, 8, p, p, 4, 0)):
        assert l.g6d_frame_crop(*args, None) == -1, args                           # G6D_EINVAL before any HIP call
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_crop(torch.zeros(96, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 8, 8, 3), dtype=torch.uint8),
                       torch.zeros((1, 9)), 4, 4)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_has_no_scratch(tmp_path):
    """The twelve tap values of a pixel stay in registers (compiler metadata; cross-compiles without a GPU)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "frame_crop.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", "frame_crop.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    (name, body), = re.findall(r"\.name:\s+(\S*frame_crop_kernel\S*)\n(.*?)\.wavefront_size", out.read_text(), re.S)
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1)) == 0, name
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1)) <= 64, name      # 8 waves per SIMD
