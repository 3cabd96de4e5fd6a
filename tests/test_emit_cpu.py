"""gen6d_amd.emit on the CPU.  `np_emit` restates the integer specification of g6d_frame_emit (include/gen6d_hip.h) in
numpy, written from the header's text; `np_frame_emit` gives it the signature of ops.frame_emit (on a CPU device the table's pointers are
host addresses, so it writes the planes the way the kernel does) and `np_track_corners` that of ops.track_corners.  Checks the colour
formulas, the edge rule against float64 geometry, the NV12 round trip through the ingest's restatement, the descriptor's layout, the
eager tracker with sinks on the patched ops, the argument errors, and that the kernel has no scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import emit as E
from gen6d_amd import geometry as G
from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_ingest_cpu import np_frame_ingest, np_ingest, nv12_of
from test_track_streams_cpu import np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)

EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
# round(k * 2^20) of the limited-range forward matrices, as listed in the header: (Y row, Cb row, Cr row) per matrix
FWD = {0: ((269262, 528618, 102662), (-155423, -305128, 460551), (460551, -385654, -74897)),
       1: ((191455, 644067, 65019), (-105533, -355018, 460551), (460551, -418321, -42230))}
KRB = {0: (0.299, 0.114), 1: (0.2126, 0.0722)}
QMIN, QMAX = -8192, 16383


def edge_cover(xs, ys, a, b, thickness):
    """The header's edge rule on int64 grids xs, ys -> bool."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    d = b - a
    px, py = xs.astype(np.int64) - a[0], ys.astype(np.int64) - a[1]
    L, pp = int(d @ d), px * px + py * py
    if L == 0:
        return 4 * pp <= thickness * thickness
    s = px * d[0] + py * d[1]
    t = np.clip(s, 0, L)
    return L * pp - 2 * t * s + t * t <= (thickness * thickness * L) // 4


def np_annotate(canvas, q, pic_w, pic_h, width, height, thickness=2, dot_radius=2, line=(0, 0, 255), dot=(255, 0, 0)):
    """canvas [H,W,3] -> the sink's annotated RGB [height,width,3]; q: int corners [8,2], or None for no box."""
    H, W = canvas.shape[:2]
    pw, ph = max(min(pic_w, W), 0), max(min(pic_h, H), 0)
    pic = canvas[:ph, :pw].copy()
    if q is not None and ((np.asarray(q) < QMIN) | (np.asarray(q) > QMAX)).any():
        q = None
    if q is not None and pw and ph:
        ys, xs = np.meshgrid(np.arange(ph), np.arange(pw), indexing="ij")
        if dot_radius >= 0:
            for j in range(8):
                pic[(xs - int(q[j][0])) ** 2 + (ys - int(q[j][1])) ** 2 <= dot_radius * dot_radius] = dot
        if thickness > 0:
            for a, b in EDGES:
                pic[edge_cover(xs, ys, q[a], q[b], thickness)] = line
    out = np.zeros((height, width, 3), np.uint8)
    h, w = min(ph, height), min(pw, width)
    out[:h, :w] = pic[:h, :w]
    return out


def np_nv12(rgb, matrix):
    """Annotated sink RGB [h,w,3] (even h, w) -> (Y [h,w], UV [h/2,w]) uint8 by the header's forward formulas."""
    cy, cb, cr = FWD[matrix]
    p = rgb.astype(np.int64)
    Y = np.clip((cy[0] * p[..., 0] + cy[1] * p[..., 1] + cy[2] * p[..., 2] + 2 ** 19 + 16 * 2 ** 20) >> 20, 0, 255)
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    Cb = np.clip((cb[0] * s[..., 0] + cb[1] * s[..., 1] + cb[2] * s[..., 2] + 2 ** 21 + 128 * 2 ** 22) >> 22, 0, 255)
    Cr = np.clip((cr[0] * s[..., 0] + cr[1] * s[..., 1] + cr[2] * s[..., 2] + 2 ** 21 + 128 * 2 ** 22) >> 22, 0, 255)
    return Y.astype(np.uint8), np.stack([Cb, Cr], -1).reshape(rgb.shape[0] // 2, rgb.shape[1]).astype(np.uint8)


def np_packed(rgb, fmt):
    """Annotated sink RGB -> [h,w,3 or 4] in the packed format's channel order, alpha 255."""
    c = rgb[..., ::-1] if fmt in (1, 3) else rgb
    return c.copy() if fmt < 2 else np.concatenate([c, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], -1)


def np_emit(canvas, q, sink, pic_hw=None):
    """One emit.Sink's expected content from a canvas and integer corners (None: no box) -> packed [h,w,c], or (Y, UV) for nv12."""
    ph, pw = canvas.shape[:2] if pic_hw is None else pic_hw
    rgb = np_annotate(canvas, q if sink.box else None, pw, ph, sink.width, sink.height, sink.thickness, sink.dot_radius,
                      ((sink.line_rgb >> 16) & 255, (sink.line_rgb >> 8) & 255, sink.line_rgb & 255),
                      ((sink.dot_rgb >> 16) & 255, (sink.dot_rgb >> 8) & 255, sink.dot_rgb & 255))
    fmt = I.FORMATS[sink.fmt]
    return np_nv12(rgb, I.MATRICES[sink.matrix]) if fmt == 4 else np_packed(rgb, fmt)


def sink_content(sink):
    """What a Sink's memory holds now, in np_emit's form (the row padding is not part of it)."""
    rows = lambda p, n, pitch, nb: np.stack([p[r * pitch:r * pitch + nb] for r in range(n)])
    p0 = sink.plane0.cpu().numpy()
    if sink.fmt == "nv12":
        return rows(p0, sink.height, sink.pitch, sink.width), rows(sink.plane1.cpu().numpy(), sink.height // 2, sink.uv_pitch, sink.width)
    bpp = I.BPP[sink.fmt]
    return rows(p0, sink.height, sink.pitch, sink.width * bpp).reshape(sink.height, sink.width, bpp)


def assert_sink(sink, want, msg=""):
    got = sink_content(sink)
    if sink.fmt == "nv12":
        np.testing.assert_array_equal(got[0], want[0], err_msg=msg + " (Y)")
        np.testing.assert_array_equal(got[1], want[1], err_msg=msg + " (UV)")
    else:
        np.testing.assert_array_equal(got, want, err_msg=msg)


def np_frame_emit(table, n, imgs, pts, valid):
    """ops.frame_emit on host memory."""
    size = C.sizeof(lib.G6dSink)
    ents = (lib.G6dSink * n).from_buffer_copy(table.numpy()[:n * size].tobytes())
    B = imgs.shape[0]
    view = lambda ptr, nb: np.ctypeslib.as_array((C.c_uint8 * nb).from_address(ptr))
    for e in ents:
        if not 0 <= e.slot < B:
            continue
        q = pts[e.box, e.slot].numpy() if e.box in (0, 1) and int(valid[e.box, e.slot]) else None
        rgb = np_annotate(imgs[e.slot].numpy(), q, e.pic_w, e.pic_h, e.width, e.height, e.thickness, e.dot_radius,
                          ((e.line_rgb >> 16) & 255, (e.line_rgb >> 8) & 255, e.line_rgb & 255),
                          ((e.dot_rgb >> 16) & 255, (e.dot_rgb >> 8) & 255, e.dot_rgb & 255))
        if e.format == 4:
            Y, UV = np_nv12(rgb, e.matrix)
            p0, p1 = view(e.plane0, (e.height - 1) * e.pitch0 + e.width), view(e.plane1, (e.height // 2 - 1) * e.pitch1 + e.width)
            for r in range(e.height):
                p0[r * e.pitch0:r * e.pitch0 + e.width] = Y[r]
            for r in range(e.height // 2):
                p1[r * e.pitch1:r * e.pitch1 + e.width] = UV[r]
        else:
            out = np_packed(rgb, e.format).reshape(e.height, -1)
            p0 = view(e.plane0, (e.height - 1) * e.pitch0 + out.shape[1])
            for r in range(e.height):
                p0[r * e.pitch0:r * e.pitch0 + out.shape[1]] = out[r]


def np_corners(box, pose, K):
    """float64 projection of the box [8,3] -> (int corners [8,2], valid, the unrounded float coordinates)."""
    uv, d = G.project_points(np.asarray(box, np.float64), np.asarray(pose, np.float64).reshape(3, 4), np.asarray(K, np.float64).reshape(3, 3))
    with np.errstate(invalid="ignore"):
        r = np.floor(uv + 0.5)
        ok = bool((d > 0).all() and (r >= QMIN).all() and (r <= QMAX).all())
    return (r.astype(np.int32) if ok else np.zeros((8, 2), np.int32)), int(ok), uv


def np_track_corners(table, K, slot_stream, box, pts=None, valid=None):
    """ops.track_corners on host memory."""
    B = slot_stream.shape[0]
    pts = torch.zeros((B, 8, 2), dtype=torch.int32) if pts is None else pts
    valid = torch.zeros((B,), dtype=torch.int32) if valid is None else valid
    Ks = K.reshape(B, 3, 3).numpy()
    for b, s in enumerate(slot_stream.tolist()):
        q, ok = (np.zeros((8, 2), np.int32), 0) if s < 0 else np_corners(box.numpy(), table[s].numpy(), Ks[b])[:2]
        pts[b] = torch.from_numpy(q)
        valid[b] = ok
    return pts, valid


@pytest.fixture
def cpu_emit(monkeypatch):
    monkeypatch.setattr(ops, "frame_emit", np_frame_emit)
    monkeypatch.setattr(ops, "track_corners", np_track_corners)


def emit_cpu(canvas, q, sink, pic_hw=None, fill=None):
    """One canvas [H,W,3] and corners -> the sink filled through emit_frames on the CPU."""
    imgs = torch.from_numpy(np.ascontiguousarray(canvas))[None]
    pts = torch.zeros((1, 8, 2), dtype=torch.int32) if q is None else torch.from_numpy(np.asarray(q, np.int32).reshape(1, 8, 2))
    valid = torch.tensor([0 if q is None else 1], dtype=torch.int32)
    E.emit_frames(imgs, pts, valid, [sink], pic_sizes=None if pic_hw is None else [pic_hw])
    return sink


BOX = np.array([[10, 8], [10, 40], [50, 44], [52, 6], [20, 14], [20, 34], [44, 36], [45, 12]], np.int32)


# ---------------------------------------------------------------------------------------------------------------- a: colour formulas
def float_ycbcr(rgb, matrix):
    Kr, Kb = KRB[matrix]
    Kg = 1 - Kr - Kb
    R, G_, B = (float(v) for v in rgb)
    return (16 + 219 / 255 * (Kr * R + Kg * G_ + Kb * B),
            128 + 224 / 255 * (-Kr / (2 * (1 - Kb)) * R - Kg / (2 * (1 - Kb)) * G_ + 0.5 * B),
            128 + 224 / 255 * (0.5 * R - Kg / (2 * (1 - Kr)) * G_ - Kb / (2 * (1 - Kr)) * B))


# (Y, Cb, Cr) of the primaries by hand from the float formulas, rounded: e.g. BT.601 red: Y = 16 + 219 * 0.299 = 81.48 -> 81,
# Cb = 128 - 224 * 0.299 / 1.772 = 90.20 -> 90, Cr = 128 + 112 = 240
HAND = {0: {(0, 0, 0): (16, 128, 128), (255, 255, 255): (235, 128, 128), (255, 0, 0): (81, 90, 240), (0, 255, 0): (145, 54, 34),
            (0, 0, 255): (41, 240, 110)},
        1: {(0, 0, 0): (16, 128, 128), (255, 255, 255): (235, 128, 128), (255, 0, 0): (63, 102, 240), (0, 255, 0): (173, 42, 26),
            (0, 0, 255): (32, 240, 118)}}


def test_uniform_colours_match_the_float_formulas(cpu_emit):
    """The integer form is within 1 level of the float form, derived: each of the three constants is off by at most 2^-21 of its scale, so
    the weighted sum moves by at most 3 * 255 * 2^-21 < 0.0004 levels (the chroma sums: 3 * 1020 * 2^-21 / 4, the same), and the one
    rounding adds at most 0.5; the measured distance is printed."""
    for m, name in ((0, "bt601"), (1, "bt709")):
        for k, row in zip("Y Cb Cr".split(), FWD[m]):
            Kr, Kb = KRB[m]
            Kg = 1 - Kr - Kb
            f = {"Y": [219 / 255 * v for v in (Kr, Kg, Kb)], "Cb": [224 / 255 * v for v in (-Kr / (2 * (1 - Kb)), -Kg / (2 * (1 - Kb)), 0.5)],
                 "Cr": [224 / 255 * v for v in (0.5, -Kg / (2 * (1 - Kr)), -Kb / (2 * (1 - Kr)))]}[k]
            assert list(row) == [round(v * 2 ** 20) for v in f], (name, k)
        rng = np.random.RandomState(m)
        colours = list(HAND[m]) + [tuple(int(v) for v in rng.randint(0, 256, 3)) for _ in range(200)]
        worst = 0.0
        for rgb in colours:
            sink = emit_cpu(np.full((6, 8, 3), rgb, np.uint8), None, E.Sink(torch.zeros((9, 8), dtype=torch.uint8), "nv12", matrix=name))
            Y, UV = sink_content(sink)
            assert (Y == Y[0, 0]).all() and (UV[:, 0::2] == UV[0, 0]).all() and (UV[:, 1::2] == UV[0, 1]).all()
            got, want = (int(Y[0, 0]), int(UV[0, 0]), int(UV[0, 1])), float_ycbcr(rgb, m)
            if rgb in HAND[m]:
                assert got == HAND[m][rgb], (name, rgb)
            worst = max(worst, max(abs(g - w) for g, w in zip(got, want)))
        print(f"{name}: integer form within {worst:.4f} levels of the float form")
        assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- b: the edge rule
def test_edge_rule_is_centre_within_half_thickness():
    """Random integer segments, odd thickness: with integer endpoints the squared distance times L is an integer and (thickness/2)^2 * L is
    an integer plus a quarter L, so a pixel centre lies on the boundary only when L is a multiple of 4 and E hits it exactly; pixels whose
    float64 distance is within 1e-9 of the boundary are skipped, at most 0.1 % of the covered ones."""
    rng = np.random.RandomState(0)
    ys, xs = np.meshgrid(np.arange(96), np.arange(128), indexing="ij")
    covered = skipped = 0
    for k in range(300):
        th = (1, 3, 5, 7)[k % 4]
        a, b = rng.randint(-40, 170, 2), rng.randint(-40, 140, 2)
        if k % 50 == 0:
            b = a.copy()                                                       # the degenerate edge
        got = edge_cover(xs, ys, a, b, th)
        d = (b - a).astype(np.float64)
        p = np.stack([xs - a[0], ys - a[1]], -1).astype(np.float64)
        L = d @ d
        u = np.clip((p @ d) / L, 0, 1) if L > 0 else np.zeros(xs.shape)
        dist = np.linalg.norm(p - u[..., None] * d, axis=-1)
        near = np.abs(dist - th / 2) <= 1e-9
        np.testing.assert_array_equal(got[~near], (dist <= th / 2)[~near], err_msg=f"segment {a} - {b}, thickness {th}")
        covered += int(got.sum())
        skipped += int(near.sum())
    print(f"{covered} covered pixels, {skipped} skipped at the boundary")
    assert covered > 20000 and skipped <= covered // 1000
    # an even thickness on an axis-aligned edge: centres at exactly thickness / 2 are inside (<=), as for cv2's 2-pixel lines
    got = edge_cover(xs, ys, (10, 20), (30, 20), 2)
    assert got[19:22, 10:31].all() and not got[18].any() and not got[22].any() and got[20, 9] and not got[20, 8]


# ---------------------------------------------------------------------------------------------------------------- c: round trip
MEASURED_ROUND_TRIP = {"bt601": 2, "bt709": 2}


def test_nv12_round_trip_through_the_ingest(cpu_emit):
    """A picture of flat 2x2-aligned blocks: emit -> NV12 -> np_ingest at equal size.  Measured here with the two restatements: the
    maximum channel error is 2 for BT.601 and 2 for BT.709 (limited range keeps 219 / 224 of 255 levels, each direction rounds once); the
    asserted bar is that value plus 1.  The kernel is held bit-exact to the restatement on the GPU."""
    rng = np.random.RandomState(1)
    blocks = rng.randint(0, 256, (24, 32, 3)).astype(np.uint8)
    blocks[0, :6] = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)]
    pic = np.repeat(np.repeat(blocks, 2, 0), 2, 1)
    for name, measured in (("bt601", MEASURED_ROUND_TRIP["bt601"]), ("bt709", MEASURED_ROUND_TRIP["bt709"])):
        sink = emit_cpu(pic, None, E.Sink(torch.zeros((72, 64), dtype=torch.uint8), "nv12", matrix=name))
        Y, UV = sink_content(sink)
        back = np_ingest(I.Frame(nv12_of(Y, UV[:, 0::2], UV[:, 1::2]), "nv12", matrix=name), 48, 64)
        err = int(np.abs(back.astype(int) - pic.astype(int)).max())
        print(f"{name}: round-trip max channel error {err}")
        assert err <= measured + 1


# ---------------------------------------------------------------------------------------------------------------- d: descriptor layout
def test_descriptor_layout_and_null_table():
    l = lib.load()
    S = lib.G6dSink
    assert C.sizeof(S) == l.g6d_sizeof_sink_desc() == 72
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68]
    buf = (C.c_uint8 * 72)()
    a = C.addressof(buf)
    assert l.g6d_frame_emit(None, 1, a, 1, 8, 8, a, a, None) == -1                 # G6D_EINVAL before any HIP call
    assert l.g6d_frame_emit(a, -1, a, 1, 8, 8, a, a, None) == -1
    assert l.g6d_frame_emit(a, 1, a, 1, 0, 8, a, a, None) == -1
    assert l.g6d_frame_emit(a, 1, a, 1, 8, 8, None, a, None) == -1
    assert l.g6d_track_corners(None, a, a, a, a, a, 1, None) == -1
    assert l.g6d_track_corners(a, a, a, a, a, a, 0, None) == -1
    assert l.g6d_abi_version() == 12
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_emit(z(72, dtype=torch.uint8), 1, z((1, 8, 8, 3), dtype=torch.uint8), z((1, 1, 8, 2), dtype=torch.int32), z((1, 1), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.track_corners(z((2, 12)), z((1, 9)), z(1, dtype=torch.int32), z((8, 3)))


# ---------------------------------------------------------------------------------------------------------------- formats, padding, crop
def test_formats_padding_crop_and_priority(cpu_emit):
    rng = np.random.RandomState(2)
    canvas = rng.randint(0, 256, (48, 64, 3)).astype(np.uint8)
    z = lambda *s: torch.full(s, 7, dtype=torch.uint8)
    # the picture occupies 45 x 61 of the canvas; sinks larger (black padding), equal and smaller (crop), pitched, every format
    wide = z(30, 200)
    cases = [E.Sink(z(48, 64, 3), "rgb24"), E.Sink(z(45, 61, 3), "bgr24"), E.Sink(wide, "rgba32", width=40), E.Sink(z(52, 70, 4), "bgra32"),
             E.Sink(z(69, 80), "nv12", width=62, matrix="bt709"), E.Sink(z(20, 30), "nv12", uv=z(10, 40), width=30, pose="raw"),
             E.Sink(z(48, 64, 3), "rgb24", box=False), E.Sink(z(48, 64, 3), "rgb24", thickness=5, dot_radius=4, line_color=(1, 2, 3), dot_color=(9, 8, 7))]
    for s in cases:
        emit_cpu(canvas, BOX, s, pic_hw=(45, 61))
        assert_sink(s, np_emit(canvas, BOX, s, (45, 61)), f"{s.fmt} {s.width}x{s.height}")
    rgb = sink_content(cases[0])
    assert (rgb[45:] == 0).all() and (rgb[:, 61:] == 0).all()
    assert tuple(rgb[8, 10]) == (0, 0, 255) and tuple(rgb[6, 52]) == (0, 0, 255)              # a corner pixel lies on its edges: blue over red
    assert tuple(rgb[8, 8]) == (255, 0, 0)                                                     # two pixels left of corner 0: disc only
    np.testing.assert_array_equal(sink_content(cases[6])[:45, :61], canvas[:45, :61])         # box=False: the plain picture
    assert (wide[:, 160:] == 7).all() and not (wide[:, :160] == 7).all()                     # a device sink's row padding is not written
    # an invalid box and a corner outside the exact range draw nothing
    s = emit_cpu(canvas, None, E.Sink(z(48, 64, 3), "rgb24"))
    np.testing.assert_array_equal(sink_content(s), canvas)
    far = BOX.copy()
    far[3] = (20000, 5)
    s = emit_cpu(canvas, far, E.Sink(z(48, 64, 3), "rgb24"))
    np.testing.assert_array_equal(sink_content(s), canvas)


# ---------------------------------------------------------------------------------------------------------------- e: tracker
@pytest.fixture
def patched(monkeypatch, cpu_emit):
    ref_ops.patch_ops(monkeypatch)
    monkeypatch.setattr(ops, "track_gather", np_track_gather)
    monkeypatch.setattr(ops, "track_commit", np_track_commit)
    monkeypatch.setattr(ops, "frame_ingest", np_frame_ingest)
    calls = []
    monkeypatch.setattr(ops, "frame_emit", lambda table, n, imgs, pts, valid: (calls.append((n, tuple(imgs.shape))), np_frame_emit(table, n, imgs, pts, valid))[1])
    return calls


def visible_object_pts(pose, K, h, w, depth=1.0, half=0.15):
    """Object points whose box lies in front of a camera with this pose, around the image centre (the synthetic weights' poses do not
    look at the database's own object, whose box then has corners behind the camera: valid = 0)."""
    pose, K = np.asarray(pose, np.float64).reshape(3, 4), np.asarray(K, np.float64).reshape(3, 3)
    c = depth * np.linalg.solve(K, [w / 2, h / 2, 1.0])
    cube = c + half * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    return (cube - pose[:, 3]) @ pose[:, :3]


def _expect(tr, sink, canvas, stream, K, pic_hw=None):
    table = tr.pose_table if sink.pose == "raw" else tr.smooth_table
    q, ok, _ = np_corners(tr.box_np, table[stream].numpy(), K)
    return np_emit(canvas, q if ok else None, sink, pic_hw), q


def test_tracker_fills_sinks_of_pushed_streams(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    z = lambda *s: torch.full(s, 7, dtype=torch.uint8)
    probe = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False)
    probe.push([0], [frames[0]], [Ks[0]])
    tr = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False, object_pts=visible_object_pts(probe.result()[0][0], Ks[0], h, w))
    mk = lambda: [E.Sink(z(h, w, 3), "rgb24", pose="raw", line_color=(0, 255, 0)), E.Sink(z(h * 3 // 2, w), "nv12")]
    # first frames: emitted from the init path, one launch per init chunk (streams 0, 1 share group 0; stream 3 sits in group 1)
    first = {0: mk(), 1: mk()[1], 3: None}
    tr.push([0, 1, 3], [frames[0], frames[1], frames[2]], [Ks[0], Ks[1], Ks[2]], sinks=[first[0], first[1], first[3]])
    assert patched == [(3, (2, h, w, 3))]
    tr.result()
    for k in first[0]:
        assert_sink(k, _expect(tr, k, frames[0], 0, Ks[0])[0], f"first frame, {k.pose}")
    assert_sink(first[1], _expect(tr, first[1], frames[1], 1, Ks[1])[0])
    # tracked frames: stream 0 gets both pictures, stream 3 a cropped and a padded one; stream 1 is not pushed and its sink stays
    del patched[:]
    keep = sink_content(first[1])
    second = {0: mk(), 3: [E.Sink(z(40, 50, 4), "bgra32"), E.Sink(z(h + 10, w + 12, 3), "bgr24", pose="raw")]}
    untouched = z(h, w, 3)
    tr.push([0, 3], [frames[2], frames[3]], [Ks[2], Ks[3]], sinks=[second[0], second[3]])
    assert patched == [(2, (2, h, w, 3)), (2, (2, h, w, 3))]                          # one emit launch per lane and tick
    tr.result()
    qs = {}
    for s, f, K in ((0, frames[2], Ks[2]), (3, frames[3], Ks[3])):
        for k in second[s]:
            want, qs[s, k.pose] = _expect(tr, k, f, s, K)
            assert_sink(k, want, f"stream {s}, {k.pose}")
    assert (qs[0, "raw"] != qs[0, "smooth"]).any()                                     # the two pictures of a frame carry two boxes
    raw_rgb = sink_content(second[0][0])
    assert (raw_rgb == (0, 255, 0)).all(-1).any() and not (frames[2] == (0, 255, 0)).all(-1).any()
    big = sink_content(second[3][1])
    assert (big[h:] == 0).all() and (big[:, w:] == 0).all()
    np.testing.assert_array_equal(sink_content(first[1])[0], keep[0])
    assert (untouched == 7).all()
    # a reset stream's first frame is emitted from the init path again, with a fresh history: raw and smoothed corners agree
    del patched[:]
    tr.reset([3])
    third = mk()
    tr.push([3], [frames[1]], [Ks[1]], sinks=[third])
    assert patched == [(2, (1, h, w, 3))]
    tr.result()
    for k in third:
        assert_sink(k, _expect(tr, k, frames[1], 3, Ks[1])[0], f"after reset, {k.pose}")
    # without sinks nothing is emitted
    del patched[:]
    tr.push([0, 3], [frames[0], frames[0]], [Ks[0], Ks[0]])
    tr.push([0], [frames[0]], [Ks[0]], sinks=[None])
    assert patched == []


def test_tracker_with_frame_size_emits_the_planned_picture(scene, patched):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    tr = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, frame_size=(h, w))
    tall = np.ascontiguousarray(np.repeat(np.repeat(frames[0][:, :w // 2], 2, 0), 2, 1))       # 2h x w source: planned h x w/2 picture
    src = [I.Frame(tall), I.Frame(frames[1])]
    for _ in range(2):                                                                        # an init push, then a tracked tick
        sinks = [E.Sink(torch.zeros((h, w, 3), dtype=torch.uint8), "rgb24"), E.Sink(torch.zeros((h * 3 // 2, w), dtype=torch.uint8), "nv12")]
        tr.push([0, 1], src, sinks=sinks)
        tr.result()
        K = [I.plan(f, (h, w))[2].astype(np.float32) for f in src]
        assert I.plan(src[0], (h, w))[:2] == (h, w // 2)
        assert_sink(sinks[0], _expect(tr, sinks[0], np_ingest(src[0], h, w), 0, K[0], (h, w // 2))[0])
        assert_sink(sinks[1], _expect(tr, sinks[1], np_ingest(src[1], h, w), 1, K[1])[0])
        assert (sink_content(sinks[0])[:, w // 2:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- f: errors
def test_errors(scene, patched):
    est, frames, Ks = scene
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    pageable = E.Sink(z(8, 8, 3), "rgb24")
    assert pageable.placement("cpu") == "device"
    with pytest.raises(ValueError, match="pinned"):
        pageable.placement(torch.device("cuda", 0))                     # a host destination of a GPU tracker must be pinned
    with pytest.raises(ValueError, match="lives on"):
        pageable.placement(torch.device("meta"))                        # a sink on another device
    with pytest.raises(ValueError, match="lives on"):
        E.emit_frames(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="meta"), torch.zeros((1, 8, 2), dtype=torch.int32, device="meta"),
                      torch.zeros(1, dtype=torch.int32, device="meta"), [pageable])
    with pytest.raises(ValueError, match="even"):
        E.Sink(z(15, 11), "nv12", width=11, height=10)
    with pytest.raises(ValueError, match="even"):
        E.Sink(z(7, 12), "nv12", uv=z(3, 12))
    with pytest.raises(ValueError, match="pitch"):
        E.Sink(z(10, 20), "rgb24", width=7)
    with pytest.raises(ValueError, match="pitch"):
        E.Sink(z(1000), "bgra32", width=8, height=8, pitch=31)
    with pytest.raises(ValueError, match="holds"):
        E.Sink(z(100), "rgb24", width=8, height=8)
    with pytest.raises(ValueError, match="outside"):
        E.Sink(z(2, 8193, 3), "rgb24")
    with pytest.raises(ValueError, match="torch tensor"):
        E.Sink(np.zeros((8, 8, 3), np.uint8), "rgb24")
    with pytest.raises(ValueError, match="layout"):
        E.Sink(z(8, 16, 3)[:, ::2], "rgb24")                            # no pitch describes it: a copy would be written, not the tensor
    with pytest.raises(ValueError, match="pose"):
        E.Sink(z(8, 8, 3), "rgb24", pose="filtered")
    with pytest.raises(ValueError, match="thickness"):
        E.Sink(z(8, 8, 3), "rgb24", thickness=300)
    with pytest.raises(ValueError, match="line_color"):
        E.Sink(z(8, 8, 3), "rgb24", line_color=(0, 0, 256))
    imgs, pts, valid = z(2, 8, 8, 3), torch.zeros((2, 8, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="slot"):
        E.emit_frames(imgs, pts, valid, [pageable], slots=[2])
    with pytest.raises(ValueError, match="picture size"):
        E.emit_frames(imgs, pts, valid, [pageable], pic_sizes=[(9, 8)])
    with pytest.raises(ValueError, match="pts"):
        E.emit_frames(imgs, pts[:1], valid, [pageable])
    tr = T.StreamTracker(est, 4, batch=2, graphs=False)
    with pytest.raises(ValueError, match="sinks"):
        tr.push([0, 1], [frames[0], frames[1]], sinks=[pageable])      # a length mismatch
    with pytest.raises(ValueError, match="sinks"):
        tr.push([0], [frames[0]], sinks=[[pageable, "x"]])
    assert not tr._frames[0] and patched == []


# ---------------------------------------------------------------------------------------------------------------- g: no scratch
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_has_no_scratch(tmp_path):
    """A thread's 8 pixels stay in registers: no scratch and no spills.  Compiler metadata; cross-compiles without a GPU."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "emit.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", "emit.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = out.read_text().split("\n  - .agpr_count")                     # one metadata block per kernel
    for kernel in ("frame_emit_kernel", "track_corners_kernel"):
        body, = [b for b in blocks[1:] if re.search(r"\.name:\s+\S*" + kernel, b)]
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", body).group(1))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0, kernel
