"""Source-view sinks (emit.Sink(view="source")) on the CPU.  `np_emit_source` restates the integer specification of g6d_frame_emit_source
(include/gen6d_hip.h) in numpy, written from the header's text; `np_frame_emit_source` gives it the signature of
ops.frame_emit_source (on a CPU device both tables hold host addresses, so it reads and writes the planes the way the kernel does).
Checks the restatement against the two existing ones (the ingest's and the canvas emit's), the NV12 pass-through, `ingest.source_K`, the
eager tracker with mixed canvas and source sinks on the patched ops, the argument errors, the layouts, and that the kernel has no scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import emit as E
from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_emit_cpu import BOX, assert_sink, np_annotate, np_corners, np_emit, np_frame_emit, np_nv12, np_packed, np_track_corners, sink_content
from test_emit_cpu import visible_object_pts
from test_ingest_cpu import np_frame_ingest, np_ingest, nv12_of
from test_track_streams_cpu import np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)

# round(k * 2^20) of the limited-range inverse matrices, as listed in the header: (CY, CVR, CUG, CVG, CUB) per matrix
INV = {0: (1220542, 1673527, 409993, 852492, 2116026), 1: (1220542, 1880097, 223347, 558891, 2214593)}
FMT_NAMES = ("rgb24", "bgr24", "rgba32", "bgra32", "nv12")


def _rows(p, n, pitch, nb):
    return np.stack([np.asarray(p[r * pitch:r * pitch + nb]) for r in range(n)])


def source_planes(p0, p1, pitch0, pitch1, w, h, fmt, matrix):
    """Flat planes of a frame -> (RGB [h,w,3] at the integer source pixels, raw Y [h,w] or None, raw UV [h/2,w] or None)."""
    if fmt == 4:
        Y, UV = _rows(p0, h, pitch0, w), _rows(p1, h // 2, pitch1, w)
        CY, CVR, CUG, CVG, CUB = INV[matrix]
        c = np.maximum(Y.astype(np.int64) - 16, 0)
        d = np.repeat(np.repeat(UV[:, 0::2].astype(np.int64) - 128, 2, 0), 2, 1)
        e = np.repeat(np.repeat(UV[:, 1::2].astype(np.int64) - 128, 2, 0), 2, 1)
        ch = [(CY * c + CVR * e + 2 ** 19) >> 20, (CY * c - CUG * d - CVG * e + 2 ** 19) >> 20, (CY * c + CUB * d + 2 ** 19) >> 20]
        return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8), Y, UV
    bpp = 4 if fmt >= 2 else 3
    px = _rows(p0, h, pitch0, w * bpp).reshape(h, w, bpp)[..., :3]
    return np.ascontiguousarray(px[..., ::-1] if fmt in (1, 3) else px), None, None


def emit_source_rule(rgb, Y, UV, same_matrix, q, width, height, fmt, matrix, thickness, dot_radius, line, dot):
    """The rules of the header on one source picture -> packed [h,w,c], or (Y, UV) for an nv12 sink."""
    h, w = rgb.shape[:2]
    ann = np_annotate(rgb, q, w, h, width, height, thickness, dot_radius, line, dot)
    if fmt != 4:
        return np_packed(ann, fmt)
    Yf, UVf = np_nv12(ann, matrix)
    if Y is None or not same_matrix:
        return Yf, UVf
    # the pass-through: which pixels a primitive covers, from the same drawing rules on a blank picture
    cov = np_annotate(np.zeros_like(rgb), q, w, h, width, height, thickness, dot_radius, (1, 1, 1), (1, 1, 1)).any(-1)
    Yr, UVr = np.full((height, width), 16, np.uint8), np.full((height // 2, width), 128, np.uint8)
    hh, ww = min(h, height), min(w, width)
    Yr[:hh, :ww], UVr[:hh // 2, :ww] = Y[:hh, :ww], UV[:hh // 2, :ww]
    block = cov[0::2, 0::2] | cov[0::2, 1::2] | cov[1::2, 0::2] | cov[1::2, 1::2]
    return np.where(cov, Yf, Yr), np.where(np.repeat(block, 2, 1), UVf, UVr)


def _colour(v):
    return ((v >> 16) & 255, (v >> 8) & 255, v & 255)


def np_emit_source(frame, q, sink):
    """One source-view emit.Sink's expected content from an ingest.Frame and integer corners in SOURCE pixels (None: no box)."""
    host = lambda p: None if p is None else (p.cpu().numpy() if torch.is_tensor(p) else p)
    sm, km = I.MATRICES[frame.matrix], I.MATRICES[sink.matrix]
    rgb, Y, UV = source_planes(host(frame.plane0), host(frame.plane1), frame.pitch, frame.uv_pitch, frame.width, frame.height,
                               I.FORMATS[frame.fmt], sm)
    return emit_source_rule(rgb, Y, UV, sm == km, q if sink.box else None, sink.width, sink.height, I.FORMATS[sink.fmt], km, sink.thickness,
                            sink.dot_radius, _colour(sink.line_rgb), _colour(sink.dot_rgb))


def np_frame_emit_source(table, n, frames, nf, pts, valid, max_w, max_h):
    """ops.frame_emit_source on host memory."""
    sinks = (lib.G6dSink * n).from_buffer_copy(table.numpy()[:n * C.sizeof(lib.G6dSink)].tobytes())
    recs = (lib.G6dFrame * nf).from_buffer_copy(frames.numpy()[:nf * C.sizeof(lib.G6dFrame)].tobytes())
    sets, B = pts.shape[:2]
    view = lambda ptr, nb: np.ctypeslib.as_array((C.c_uint8 * nb).from_address(ptr))
    for e in sinks:
        if not 0 <= e.slot < nf:
            continue
        f = recs[e.slot]
        nv12 = f.format == 4
        bpp = 1 if nv12 else (4 if f.format >= 2 else 3)
        p0 = view(f.plane0, (f.height - 1) * f.pitch0 + f.width * bpp)
        p1 = view(f.plane1, (f.height // 2 - 1) * f.pitch1 + f.width) if nv12 else None
        rgb, Y, UV = source_planes(p0, p1, f.pitch0, f.pitch1, f.width, f.height, f.format, f.matrix)
        draw = e.box in (0, 1) and e.box < sets and 0 <= f.slot < B and int(valid[e.box, f.slot])
        q = pts[e.box, f.slot].numpy() if draw else None
        out = emit_source_rule(rgb, Y, UV, f.matrix == e.matrix, q, e.width, e.height, e.format, e.matrix, e.thickness, e.dot_radius,
                               _colour(e.line_rgb), _colour(e.dot_rgb))
        if e.format == 4:
            d0, d1 = view(e.plane0, (e.height - 1) * e.pitch0 + e.width), view(e.plane1, (e.height // 2 - 1) * e.pitch1 + e.width)
            for r in range(e.height):
                d0[r * e.pitch0:r * e.pitch0 + e.width] = out[0][r]
            for r in range(e.height // 2):
                d1[r * e.pitch1:r * e.pitch1 + e.width] = out[1][r]
        else:
            flat = out.reshape(e.height, -1)
            d0 = view(e.plane0, (e.height - 1) * e.pitch0 + flat.shape[1])
            for r in range(e.height):
                d0[r * e.pitch0:r * e.pitch0 + flat.shape[1]] = flat[r]


@pytest.fixture
def cpu_source(monkeypatch):
    monkeypatch.setattr(ops, "frame_ingest", np_frame_ingest)
    monkeypatch.setattr(ops, "frame_emit", np_frame_emit)
    monkeypatch.setattr(ops, "track_corners", np_track_corners)
    monkeypatch.setattr(ops, "frame_emit_source", np_frame_emit_source)


def emit_sources(frames, pts, valid, sinks, sources=None, slots=None, B=None, device="cpu"):
    """Frames -> a small canvas batch on `device` (ingest_frames_keep), then the sinks through emit_source_frames.  pts [B,8,2] / [2,B,8,2]."""
    B = len(frames) if B is None else B
    out = torch.zeros((B, 8, 8, 3), dtype=torch.uint8, device=device)
    K = torch.zeros((B, 3, 3), dtype=torch.float32, device=device)
    got, staged = I.ingest_frames_keep(frames, out, K, slots=slots)
    assert got is out and staged.n == len(frames) and staged.batch == B
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
    E.emit_source_frames(staged, d(pts), d(valid), sinks, sources=sources)
    return staged


def make_frame(rng, fmt, w, h, matrix="bt601", extra=0, offset=0, where="host", **kw):
    """A random frame of the format: `extra` bytes of row padding, the plane `offset` bytes into its buffer; a numpy array ("host") or a
    device tensor ("cuda")."""
    rows, bpp = (h * 3 // 2, 1) if fmt == "nv12" else (h, I.BPP[fmt])
    pitch = w * bpp + extra
    buf = rng.randint(0, 256, offset + rows * pitch).astype(np.uint8)
    data = buf[offset:] if where == "host" else torch.from_numpy(buf).to(where)[offset:]
    return I.Frame(data, fmt, width=w, height=h, pitch=pitch, matrix=matrix, **kw)


def blank_sink(fmt, w, h, matrix="bt601", device="cpu", **kw):
    rows = h * 3 // 2 if fmt == "nv12" else h
    return E.Sink(torch.full((rows, w * I.BPP[fmt] + 5), 7, dtype=torch.uint8, device=device), fmt, width=w, height=h, matrix=matrix,
                  view="source", **kw)


SRC_BOX = BOX * 2 - [20, 20]                                            # edges that leave a 70 x 46 picture


# ---------------------------------------------------------------------------------------------------------------- a: the two restatements
def test_restatement_agrees_with_ingest_and_canvas_emit():
    """Every (source format, sink format, matrix) pair that is not a pass-through: the source view of a frame is the canvas view of the
    same frame ingested into a same-size canvas at rotation 0."""
    rng = np.random.RandomState(0)
    pairs = 0
    for sfmt in FMT_NAMES:
        for sm in (("bt601", "bt709") if sfmt == "nv12" else ("bt601",)):
            w, h = (72, 46) if sfmt == "nv12" else (70, 46)
            frame = make_frame(rng, sfmt, w, h, sm, extra=7, offset=1)
            canvas = np_ingest(frame, h, w)
            for kfmt in FMT_NAMES:
                for km in (("bt601", "bt709") if kfmt == "nv12" else ("bt601",)):
                    if sfmt == kfmt == "nv12" and sm == km:
                        continue
                    for dw, dh in ((0, 0), (8, 8), (-10, -10)):
                        sink = blank_sink(kfmt, w + dw, h + dh, km, pose="raw")
                        for q in (SRC_BOX, None):
                            want = np_emit(canvas, q, sink)
                            got = np_emit_source(frame, q, sink)
                            for a, b in (zip(got, want) if kfmt == "nv12" else ((got, want),)):
                                np.testing.assert_array_equal(a, b, err_msg=f"{sfmt}/{sm} -> {kfmt}/{km} {dw:+d}")
                    pairs += 1
    assert pairs == 6 * 6 - 2


# ---------------------------------------------------------------------------------------------------------------- b: pass-through
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_nv12_pass_through(cpu_source, matrix):
    rng = np.random.RandomState(1)
    w, h = 72, 46
    frame = make_frame(rng, "nv12", w, h, matrix, extra=3, offset=1)
    Y, UV = _rows(frame.plane0, h, frame.pitch, w), _rows(frame.plane1, h // 2, frame.uv_pitch, w)
    other = "bt709" if matrix == "bt601" else "bt601"
    plain, boxed, big, small, cross = (blank_sink("nv12", w, h, matrix, box=False), blank_sink("nv12", w, h, matrix),
                                       blank_sink("nv12", w + 8, h + 8, matrix), blank_sink("nv12", w - 10, h - 10, matrix),
                                       blank_sink("nv12", w, h, other))
    emit_sources([frame], SRC_BOX[None], [1], [plain, boxed, big, small, cross], sources=[0] * 5)
    # without a box: a byte copy of the picture
    gy, guv = sink_content(plain)
    np.testing.assert_array_equal(gy, Y)
    np.testing.assert_array_equal(guv, UV)
    # with the box: uncovered pixels and untouched blocks are the source's bytes, the touched ones the forward formulas
    rgb = source_planes(frame.plane0, frame.plane1, frame.pitch, frame.uv_pitch, w, h, 4, I.MATRICES[matrix])[0]
    ann = np_annotate(rgb, SRC_BOX, w, h, w, h)
    cov = np_annotate(np.zeros_like(rgb), SRC_BOX, w, h, w, h, line=(1, 1, 1), dot=(1, 1, 1)).any(-1)
    assert 200 < cov.sum() < cov.size // 2
    block = np.repeat(cov[0::2, 0::2] | cov[0::2, 1::2] | cov[1::2, 0::2] | cov[1::2, 1::2], 2, 1)
    Yf, UVf = np_nv12(ann, I.MATRICES[matrix])
    gy, guv = sink_content(boxed)
    np.testing.assert_array_equal(gy[~cov], Y[~cov])
    np.testing.assert_array_equal(guv[~block], UV[~block])
    np.testing.assert_array_equal(gy[cov], Yf[cov])
    np.testing.assert_array_equal(guv[block], UVf[block])
    assert (gy[cov] != Y[cov]).any() and (guv[block] != UV[block]).any()
    # a larger sink pads with what black converts to, a smaller one crops; both keep the source's bytes where nothing is drawn
    gy, guv = sink_content(big)
    assert (gy[h:] == 16).all() and (gy[:, w:] == 16).all() and (guv[h // 2:] == 128).all() and (guv[:, w:] == 128).all()
    np.testing.assert_array_equal(gy[:h, :w][~cov], Y[~cov])
    gy, guv = sink_content(small)
    np.testing.assert_array_equal(gy[~cov[:h - 10, :w - 10]], Y[:h - 10, :w - 10][~cov[:h - 10, :w - 10]])
    for s in (boxed, big, small):
        assert_sink(s, np_emit_source(frame, SRC_BOX, s))
    # the other matrix: the full conversion, no byte is passed through
    want = np_nv12(ann, I.MATRICES[other])
    assert_sink(cross, want)
    assert (want[0] != Y).any()


# ---------------------------------------------------------------------------------------------------------------- c: source_K
def test_source_K():
    rng = np.random.RandomState(2)
    K = np.array([[1234.5, 0.25, 951.0], [0, 1230.25, 533.5], [0, 0, 1]])
    f = I.Frame(np.zeros((1080, 1920, 3), np.uint8), rotate=90, K=K)
    assert I.source_K(f, (960, 540)).tobytes() == K.tobytes()
    box = rng.uniform(-0.4, 0.4, (8, 3)) + [0, 0, 3.0]
    for rot in (0, 90, 180, 270):
        for (hs, ws), canvas in (((1080, 1920), (540, 960)), ((720, 960), (480, 480))):
            canvas = canvas[::-1] if rot in (90, 270) else canvas
            f = I.Frame(np.zeros((hs, ws, 3), np.uint8), rotate=rot)
            out_h, out_w, Kc = I.plan(f, canvas)
            A, Ks = I.pixel_map(f, out_h, out_w), I.source_K(f, canvas)
            assert Ks.dtype == np.float64
            np.testing.assert_allclose(A @ Ks, Kc, rtol=1e-9, atol=1e-9 * np.abs(Kc).max())
            # the box's corners through the source's K, then the pixel map, land where the canvas K puts them
            a = box @ Ks.T
            a = (np.concatenate([a[:, :2] / a[:, 2:], np.ones((8, 1))], 1)) @ A.T
            b = box @ Kc.T
            np.testing.assert_allclose(a[:, :2], b[:, :2] / b[:, 2:], rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="lens"):
        I.source_K(I.Frame(np.zeros((8, 8, 3), np.uint8), K=np.eye(3), lens=I.Lens("brown", (0.1, 0, 0, 0))), (8, 8))


# ---------------------------------------------------------------------------------------------------------------- d: tracker
@pytest.fixture
def patched(monkeypatch, cpu_source):
    ref_ops.patch_ops(monkeypatch)
    monkeypatch.setattr(ops, "track_gather", np_track_gather)
    monkeypatch.setattr(ops, "track_commit", np_track_commit)
    calls = []
    for name in ("frame_ingest", "frame_emit", "track_corners", "frame_emit_source"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    return calls


def camera_frame(img, size=(240, 320), rotate=0, K=None, where="host"):
    """An [h,w,3] picture -> an NV12 ingest.Frame of `size` (nearest-neighbour scaled), stored turned back by `rotate` so that the
    ingest's quarter turn shows it upright again."""
    h, w = size
    big = img[(np.arange(h) * img.shape[0]) // h][:, (np.arange(w) * img.shape[1]) // w]
    big = np.ascontiguousarray(np.rot90(big, rotate // 90))
    Y, UV = np_nv12(big, 0)
    buf = nv12_of(Y, UV[:, 0::2], UV[:, 1::2])
    return I.Frame(buf if where == "host" else torch.from_numpy(buf).to(where), "nv12", rotate=rotate, K=K)


def own_K(K, scale=2.5):
    """Intrinsics of a picture -> those of its `scale` times larger source (half-pixel centres)."""
    return np.array([[scale, 0, 0.5 * scale - 0.5], [0, scale, 0.5 * scale - 0.5], [0, 0, 1]]) @ np.asarray(K, np.float64)


def expect_sink(tr, sink, frame, stream, canvas_hw):
    """A tracker sink's expected content under the committed pose of `stream`: the source view under source_K, the canvas view under
    the planned K', both rounded to float32 once."""
    table = tr.pose_table if sink.pose == "raw" else tr.smooth_table
    pose = table[stream].cpu().numpy()
    if sink.view == "source":
        q, ok, _ = np_corners(tr.box_np, pose, I.source_K(frame, canvas_hw).astype(np.float32))
        return np_emit_source(frame, q if ok else None, sink), ok
    out_h, out_w, K = I.plan(frame, canvas_hw)
    q, ok, _ = np_corners(tr.box_np, pose, K.astype(np.float32))
    return np_emit(np_ingest(frame, *canvas_hw), q if ok else None, sink, (out_h, out_w)), ok


def test_tracker_mixes_canvas_and_source_sinks(scene, patched):
    est, frames, Ks = scene
    hw = (120, 160)
    src = lambda t: [camera_frame(frames[t % 4]), camera_frame(frames[(t + 1) % 4], rotate=90),
                     camera_frame(frames[(t + 2) % 4], K=own_K(Ks[(t + 2) % 4]))]
    probe = T.StreamTracker(est, 1, batch=1, lanes=1, graphs=False, frame_size=hw)
    probe.push([0], [src(0)[0]])
    pts = visible_object_pts(probe.result()[0][0], I.plan(src(0)[0], hw)[2], *hw)
    tr = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False, frame_size=hw, object_pts=pts)
    z = lambda *s: torch.full(s, 7, dtype=torch.uint8)
    drawn = 0
    for t in range(2):                                                                        # an init push, then a tracked tick
        fr = src(t)
        assert fr[1].width == 240 and fr[1].height == 320 and I.plan(fr[1], hw)[:2] == hw
        sinks = [[E.Sink(z(360, 320), "nv12", view="source"), E.Sink(z(180, 160), "nv12"), E.Sink(z(240, 320, 3), "rgb24", view="source", pose="raw")],
                 E.Sink(z(480 + 12, 240 + 8), "nv12", width=240 + 8, view="source", matrix="bt709"),
                 [E.Sink(z(120, 160, 4), "bgra32", pose="raw"), E.Sink(z(345, 310), "nv12", view="source", thickness=5, dot_radius=6)]]
        del patched[:]
        tr.push([0, 1, 2], fr, sinks=sinks)
        # streams 0, 1 share a lane (2 source + 1 canvas sink), stream 2 has one sink of each view on the other
        assert patched.count("frame_emit_source") == 2 and patched.count("frame_emit") == 2
        assert patched.count("frame_ingest") == 2 and patched.count("track_corners") == 2 + 1 + 1 + 1
        tr.result()
        for s, ent in zip((0, 1, 2), sinks):
            for k in ([ent] if isinstance(ent, E.Sink) else ent):
                want, ok = expect_sink(tr, k, fr[s], s, hw)
                drawn += int(ok and k.view == "source")
                assert_sink(k, want, f"push {t} stream {s} {k.view} {k.fmt} {k.pose}")
    assert drawn >= 4
    # a push without source-view sinks keeps no frame table and launches nothing new
    del patched[:]
    tr.push([0, 1], src(2)[:2], sinks=[E.Sink(z(180, 160), "nv12"), None])
    assert "frame_emit_source" not in patched and patched.count("track_corners") == 1


# ---------------------------------------------------------------------------------------------------------------- e: errors
def test_errors(scene, patched):
    est, frames, Ks = scene
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    with pytest.raises(ValueError, match="view"):
        E.Sink(z(8, 8, 3), "rgb24", view="camera")
    assert E.Sink(z(8, 8, 3), "rgb24").view == "canvas"
    src = E.Sink(z(96, 128, 3), "rgb24", view="source")
    tr = T.StreamTracker(est, 2, batch=2, graphs=False)
    with pytest.raises(ValueError, match="frame_size"):
        tr.push([0], [frames[0]], sinks=[src])
    tr = T.StreamTracker(est, 2, batch=2, graphs=False, frame_size=(96, 128))
    lens = I.Frame(frames[0], K=Ks[0], lens=I.Lens("brown", (0.05, 0.0, 0.0, 0.0)))
    with pytest.raises(ValueError, match="lens.*out of scope"):
        tr.push([0, 1], [frames[1], lens], sinks=[src, [E.Sink(z(96, 128, 3), "rgb24"), src]])
    assert patched == [] and not tr._frames[0] and tr._sinks == {}
    # the stand-alone entry: canvas sinks, lens frames, frame indices, the table's type
    out, K = z(1, 8, 8, 3), torch.zeros((1, 3, 3))
    _, staged = I.ingest_frames_keep([I.Frame(frames[0])], out, K)
    pts, valid = torch.zeros((1, 8, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="source"):
        E.emit_source_frames(staged, pts, valid, [E.Sink(z(8, 8, 3), "rgb24")])
    with pytest.raises(ValueError, match="canvas"):
        E.emit_frames(out, pts, valid, [src])
    with pytest.raises(ValueError, match="frame index"):
        E.emit_source_frames(staged, pts, valid, [src], sources=[1])
    with pytest.raises(ValueError, match="ingest_frames_keep"):
        E.emit_source_frames(out, pts, valid, [src])
    with pytest.raises(ValueError, match="pts"):
        E.emit_source_frames(staged, torch.zeros((2, 8, 2), dtype=torch.int32), valid, [src])
    assert I.ingest_frames([I.Frame(frames[0])], out, K) is out                     # without keep: what it always returned
    assert patched.count("frame_emit_source") == 0


# ---------------------------------------------------------------------------------------------------------------- f: layout
def test_layout_and_null_tables():
    l = lib.load()
    assert C.sizeof(lib.G6dSink) == l.g6d_sizeof_sink_desc() == 72
    assert C.sizeof(lib.G6dFrame) == l.g6d_sizeof_frame_desc() == 96
    assert l.g6d_abi_version() == 12
    buf = (C.c_uint8 * 96)()
    a = C.addressof(buf)
    assert l.g6d_frame_emit_source(None, 1, a, 1, a, a, 1, 1, 8, 8, None) == -1       # G6D_EINVAL before any HIP call
    assert b"frame_emit_source" in l.g6d_last_error()
    assert l.g6d_frame_emit_source(a, 1, None, 1, a, a, 1, 1, 8, 8, None) == -1
    assert l.g6d_frame_emit_source(a, -1, a, 1, a, a, 1, 1, 8, 8, None) == -1
    assert l.g6d_frame_emit_source(a, 1, a, 0, a, a, 1, 1, 8, 8, None) == -1
    assert l.g6d_frame_emit_source(a, 1, a, 1, None, a, 1, 1, 8, 8, None) == -1
    assert l.g6d_frame_emit_source(a, 1, a, 1, a, a, 3, 1, 8, 8, None) == -1
    assert l.g6d_frame_emit_source(a, 1, a, 1, a, a, 1, 1, 0, 8, None) == -1
    assert l.g6d_frame_emit_source(a, 1, a, 1, a, a, 1, 1, 8, 8193, None) == -1
    assert l.g6d_frame_emit_source(a, 0, a, 1, a, a, 1, 1, 8, 8, None) == 0           # nothing to do: no launch
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_emit_source(z(72, dtype=torch.uint8), 1, z(96, dtype=torch.uint8), 1, z((1, 1, 8, 2), dtype=torch.int32),
                              z((1, 1), dtype=torch.int32), 8, 8)


# ---------------------------------------------------------------------------------------------------------------- g: no scratch
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_has_no_scratch(tmp_path):
    """A thread's 8 pixels and its raw NV12 words stay in registers: no scratch and no spills.  Compiler metadata; cross-compiles
    without a GPU."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "emit_source.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", "emit_source.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    # shift-then-clamp pairs fused into this instruction came out with a garbage B byte on the device (csrc/emit_source.hip, sat8s20)
    assert "v_ashr_pk_u8_i32" not in text
    blocks = text.split("\n  - .agpr_count")                                # one metadata block per kernel
    body, = [b for b in blocks[1:] if re.search(r"\.name:\s+\S*frame_emit_source_kernel", b)]
    field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", body).group(1))
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
