"""The pixel formats after NV12 (yuyv422, uyvy422, i420, yv12, p010, gray8) and the full-range matrices on the CPU.
The tap rules and the forward rules of include/gen6d_hip.h are restated in numpy here, written from the header's text: `frame_yuv` reads
a frame's samples, `yuv_to_rgb` is the tap rule, `forward_yuv` the forward rule, `pass_through` the source view's pass-through rule.
Everything downstream of a tap is unchanged by the header, so the ops are patched as tests/test_ingest_cpu.py and
tests/test_emit_source_cpu.py patch them: a frame of a new format is converted to RGB per pixel by the tap rule and handed to the
existing restatements (which know formats <= 4 only and stay as they are) as an rgb24 record; a sink of a new format takes the existing
annotation and the forward rule here.  Checks: equivalences that tie the new paths to the NV12 path without this restatement, the
integer rules against float64, the pass-through, validation, the layouts, an eager tracker over all eleven formats, compiler metadata."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import emit as E
from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_emit_cpu import BOX, FWD, KRB, np_annotate, np_frame_emit, np_nv12, np_track_corners, visible_object_pts
from test_emit_source_cpu import SRC_BOX, _colour, _rows, np_frame_emit_source
from test_frame_crop_cpu import homographies, np_crop, np_frame_crop, records_of_table
from test_ingest_cpu import np_frame_ingest, nv12_of, pitched
from test_ingest_lens_cpu import np_frame_ingest_mesh
from test_track_streams_cpu import np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)

NEW = ("yuyv422", "uyvy422", "i420", "yv12", "p010", "gray8")
YUV8 = ("nv12", "yuyv422", "uyvy422", "i420", "yv12")                       # the formats a sink can have beside packed RGB
ALL = tuple(I.FORMATS)
# (CY, Y offset, CVR, CUG, CVG, CUB) per matrix value, as listed in the header
INV_X = {0: (1220542, 16, 1673527, 409993, 852492, 2116026), 1: (1220542, 16, 1880097, 223347, 558891, 2214593),
         2: (1 << 20, 0, 1470104, 360853, 748826, 1858077), 3: (1 << 20, 0, 1651297, 196424, 490864, 1945738)}
# ((CY, CB, CR), Y offset) per matrix value
FWD_X = {0: (FWD[0], 16), 1: (FWD[1], 16),
         2: (((313524, 615514, 119538), (-176932, -347356, 524288), (524288, -439026, -85262)), 0),
         3: (((222927, 749942, 75707), (-120138, -404150, 524288), (524288, -476214, -48074)), 0)}
# the float matrices the constants are rounded from: (inverse (kvr, kug, kvg, kub), (Kr, Kb))
FLOAT = {2: ((1.402, 0.344136, 0.714136, 1.772), KRB[0]), 3: ((1.5748, 0.187324, 0.468124, 1.8556), KRB[1])}


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _i32(*values):
    """The sums the header leaves in 32-bit stay below 2^31 in magnitude."""
    for v in values:
        assert np.abs(np.asarray(v)).max() < 2 ** 31


def yuv_to_rgb(Y, U, V, matrix, bits=8):
    """The tap rule: samples (int64, chroma already at the luma grid) -> RGB int64 [..., 3].  8 bit: 32-bit sums, >> 20; 10 bit (P010):
    the same constants on c, d, e in 10-bit units, >> 22, 64-bit sums."""
    CY, yoff, CVR, CUG, CVG, CUB = INV_X[matrix]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    mid, sh = (128, 20) if bits == 8 else (512, 22)
    c, d, e = np.maximum(Y - (yoff if bits == 8 else 4 * yoff), 0), U - mid, V - mid
    rnd = 1 << (sh - 1)
    kr, kg, kb = CVR * e + rnd, -CUG * d - CVG * e + rnd, CUB * d + rnd
    if bits == 8:
        _i32(CY * c, kr, kg, kb, CY * c + kr, CY * c + kg, CY * c + kb)
    return np.clip(np.stack([(CY * c + kr) >> sh, (CY * c + kg) >> sh, (CY * c + kb) >> sh], -1), 0, 255)


def frame_yuv(p0, p1, pitch0, pitch1, w, h, fmt):
    """Flat planes of a YUV frame -> (Y [h,w], U, V [h or h/2, w/2]) as the memory holds them (P010: word >> 6)."""
    if fmt == 4:
        UV = _rows(p1, h // 2, pitch1, w)
        return _rows(p0, h, pitch0, w), UV[:, 0::2], UV[:, 1::2]
    if fmt in (5, 6):
        r = _rows(p0, h, pitch0, 2 * w)
        return (r[:, 0::2], r[:, 1::4], r[:, 3::4]) if fmt == 5 else (r[:, 1::2], r[:, 0::4], r[:, 2::4])
    if fmt in (7, 8):
        c = _rows(p1, h, pitch1, w // 2)              # the second chroma plane starts at plane1 + pitch1 * (h / 2)
        first, second = c[:h // 2], c[h // 2:]
        return (_rows(p0, h, pitch0, w),) + ((first, second) if fmt == 7 else (second, first))
    assert fmt == 9
    words = lambda rows: np.ascontiguousarray(rows).view("<u2") >> 6
    UV = words(_rows(p1, h // 2, pitch1, 2 * w))
    return words(_rows(p0, h, pitch0, 2 * w)), UV[:, 0::2], UV[:, 1::2]


def frame_rgb(p0, p1, pitch0, pitch1, w, h, fmt, matrix):
    """A frame of a format after NV12 (or NV12 under any matrix) -> RGB uint8 [h,w,3] at its integer pixels, chroma point-sampled."""
    if fmt == 10:
        return np.repeat(_rows(p0, h, pitch0, w)[..., None], 3, -1).astype(np.uint8)
    Y, U, V = frame_yuv(p0, p1, pitch0, pitch1, w, h, fmt)
    up = lambda c: np.repeat(c if c.shape[0] == h else np.repeat(c, 2, 0), 2, 1)
    return yuv_to_rgb(Y, up(U), up(V), matrix, 10 if fmt == 9 else 8).astype(np.uint8)


def forward_yuv(rgb, matrix, c422):
    """Annotated sink RGB [h,w,3] -> (Y [h,w], U, V [h or h/2, w/2]) uint8 by the forward rule: Y per pixel, chroma once per block from
    the channel sums (2 x 1 for 4:2:2, 2 x 2 for 4:2:0)."""
    (cy, cb, cr), yoff = FWD_X[matrix]
    p = rgb.astype(np.int64)
    ys = cy[0] * p[..., 0] + cy[1] * p[..., 1] + cy[2] * p[..., 2] + 2 ** 19 + yoff * 2 ** 20
    s = p[:, 0::2] + p[:, 1::2]
    sh = 21
    if not c422:
        s, sh = s[0::2] + s[1::2], 22
    us, vs = (c[0] * s[..., 0] + c[1] * s[..., 1] + c[2] * s[..., 2] + 2 ** (sh - 1) + 128 * 2 ** sh for c in (cb, cr))
    _i32(ys, us, vs)
    return tuple(np.clip(v >> k, 0, 255).astype(np.uint8) for v, k in ((ys, 20), (us, sh), (vs, sh)))


def pass_through(rgb, raw, q, width, height, matrix, c422, style, yblack):
    """The header's pass-through on one source picture (rgb: its converted pixels, raw: its (Y, U, V)) -> the sink's (Y, U, V)."""
    h, w = rgb.shape[:2]
    ann = np_annotate(rgb, q, w, h, width, height, *style)
    cov = np_annotate(np.zeros_like(rgb), q, w, h, width, height, style[0], style[1], (1, 1, 1), (1, 1, 1)).any(-1)
    Yf, Uf, Vf = forward_yuv(ann, matrix, c422)
    cs = 1 if c422 else 2
    Yr = np.full((height, width), yblack, np.uint8)
    Ur, Vr = (np.full((height // cs, width // 2), 128, np.uint8) for _ in range(2))
    hh, ww = min(h, height), min(w, width)
    Yr[:hh, :ww], Ur[:hh // cs, :ww // 2], Vr[:hh // cs, :ww // 2] = raw[0][:hh, :ww], raw[1][:hh // cs, :ww // 2], raw[2][:hh // cs, :ww // 2]
    block = cov[:, 0::2] | cov[:, 1::2]
    if not c422:
        block = block[0::2] | block[1::2]
    return np.where(cov, Yf, Yr), np.where(block, Uf, Ur), np.where(block, Vf, Vr)


# ---------------------------------------------------------------------------------------------------------------- tables and memory
_view = lambda ptr, nb: np.ctypeslib.as_array((C.c_uint8 * nb).from_address(ptr))
_ext = lambda fmt, matrix: fmt > 4 or (fmt == 4 and matrix > 1)


def frame_planes(e):
    """A G6dFrame record in host memory -> its two flat planes."""
    bpp = 2 if e.format in (5, 6, 9) else 1
    p0 = _view(e.plane0, (e.height - 1) * e.pitch0 + e.width * bpp)
    nb = {4: (e.height // 2 - 1) * e.pitch1 + e.width, 9: (e.height // 2 - 1) * e.pitch1 + 2 * e.width,
          7: (e.height - 1) * e.pitch1 + e.width // 2, 8: (e.height - 1) * e.pitch1 + e.width // 2}.get(e.format)
    return p0, (_view(e.plane1, nb) if nb else None)


def rgb_table(table, n):
    """A frame table in host memory -> (the same table with every record of a new format replaced by an rgb24 record of its converted
    picture, the arrays those records point into)."""
    size = C.sizeof(lib.G6dFrame)
    ents = (lib.G6dFrame * n).from_buffer_copy(table.numpy()[:n * size].tobytes())
    keep = []
    for e in ents:
        if e.plane0 and _ext(e.format, e.matrix):
            rgb = np.ascontiguousarray(frame_rgb(*frame_planes(e), e.pitch0, e.pitch1, e.width, e.height, e.format, e.matrix))
            keep.append(rgb)
            e.plane0, e.plane1, e.pitch0, e.pitch1, e.format, e.matrix = rgb.ctypes.data, None, 3 * e.width, 0, 0, 0
    return torch.from_numpy(np.frombuffer(ents, np.uint8, n * size).copy()), keep


def x_frame_ingest(table, n, out, K_out):
    t, keep = rgb_table(table, n)
    return np_frame_ingest(t, n, out, K_out)


def x_frame_ingest_mesh(table, meshes, n, out, K_out):
    t, keep = rgb_table(table, n)
    return np_frame_ingest_mesh(t, meshes, n, out, K_out)


def x_frame_crop(table, rec, imgs, hinv, dh, dw, out=None):
    t, keep = rgb_table(table, table.numel() // C.sizeof(lib.G6dFrame))
    return np_frame_crop(t, rec, imgs, hinv, dh, dw, out)


def write_yuv(e, Y, U, V):
    """(Y, U, V) of forward_yuv / pass_through -> a G6dSink record's memory in its layout."""
    h, w = Y.shape
    if e.format in (5, 6):
        row = np.zeros((h, 2 * w), np.uint8)
        if e.format == 5:
            row[:, 0::2], row[:, 1::4], row[:, 3::4] = Y, U, V
        else:
            row[:, 1::2], row[:, 0::4], row[:, 2::4] = Y, U, V
        planes = [(e.plane0, e.pitch0, row)]
    elif e.format == 4:
        planes = [(e.plane0, e.pitch0, Y), (e.plane1, e.pitch1, np.stack([U, V], -1).reshape(h // 2, w))]
    else:
        planes = [(e.plane0, e.pitch0, Y), (e.plane1, e.pitch1, np.concatenate([U, V] if e.format == 7 else [V, U]))]
    for ptr, pitch, rows in planes:
        d = _view(ptr, (rows.shape[0] - 1) * pitch + rows.shape[1])
        for r in range(rows.shape[0]):
            d[r * pitch:r * pitch + rows.shape[1]] = rows[r]


def _style(e):
    return e.thickness, e.dot_radius, _colour(e.line_rgb), _colour(e.dot_rgb)


def x_frame_emit(table, n, imgs, pts, valid):
    """ops.frame_emit on host memory: sinks of the new formats and matrices here, the others through tests/test_emit_cpu.py."""
    size = C.sizeof(lib.G6dSink)
    ents = (lib.G6dSink * n).from_buffer_copy(table.numpy()[:n * size].tobytes())
    for i, e in enumerate(ents):
        if not _ext(e.format, e.matrix):
            np_frame_emit(table[i * size:], 1, imgs, pts, valid)
        elif 0 <= e.slot < imgs.shape[0]:
            q = pts[e.box, e.slot].numpy() if e.box in (0, 1) and int(valid[e.box, e.slot]) else None
            rgb = np_annotate(imgs[e.slot].numpy(), q, e.pic_w, e.pic_h, e.width, e.height, *_style(e))
            write_yuv(e, *forward_yuv(rgb, e.matrix, e.format in (5, 6)))


def x_frame_emit_source(table, n, frames, nf, pts, valid, max_w, max_h):
    """ops.frame_emit_source on host memory: pairs with a new format or matrix on either side here, the others through
    tests/test_emit_source_cpu.py."""
    size, fsize = C.sizeof(lib.G6dSink), C.sizeof(lib.G6dFrame)
    ents = (lib.G6dSink * n).from_buffer_copy(table.numpy()[:n * size].tobytes())
    recs = (lib.G6dFrame * nf).from_buffer_copy(frames.numpy()[:nf * fsize].tobytes())
    rgb_frames, keep = rgb_table(frames, nf)
    sets, B = pts.shape[:2]
    for i, e in enumerate(ents):
        if not 0 <= e.slot < nf:
            continue
        f = recs[e.slot]
        fx, kx = _ext(f.format, f.matrix), _ext(e.format, e.matrix)
        if not kx:                                     # an existing sink: the existing rule on the converted picture (never a pass-through)
            np_frame_emit_source(table[i * size:], 1, rgb_frames if fx else frames, nf, pts, valid, max_w, max_h)
            continue
        draw = e.box in (0, 1) and e.box < sets and 0 <= f.slot < B and int(valid[e.box, f.slot])
        q = pts[e.box, f.slot].numpy() if draw else None
        if fx:
            rgb = frame_rgb(*frame_planes(f), f.pitch0, f.pitch1, f.width, f.height, f.format, f.matrix)
        else:                                          # a frame of the five first formats: its picture by the existing restatement
            from test_emit_source_cpu import source_planes
            bpp = 1 if f.format == 4 else (4 if f.format >= 2 else 3)
            p0 = _view(f.plane0, (f.height - 1) * f.pitch0 + f.width * bpp)
            p1 = _view(f.plane1, (f.height // 2 - 1) * f.pitch1 + f.width) if f.format == 4 else None
            rgb = source_planes(p0, p1, f.pitch0, f.pitch1, f.width, f.height, f.format, f.matrix)[0]
        c422 = e.format in (5, 6)
        if f.format == e.format and f.matrix == e.matrix:                      # (a sink's format is one of the five 8-bit YUV layouts)
            raw = frame_yuv(*frame_planes(f), f.pitch0, f.pitch1, f.width, f.height, f.format)
            out = pass_through(rgb, raw, q, e.width, e.height, e.matrix, c422, _style(e), FWD_X[e.matrix][1])
        else:
            out = forward_yuv(np_annotate(rgb, q, f.width, f.height, e.width, e.height, *_style(e)), e.matrix, c422)
        write_yuv(e, *out)


@pytest.fixture
def cpu_ops(monkeypatch):
    monkeypatch.setattr(ops, "frame_ingest", x_frame_ingest)
    monkeypatch.setattr(ops, "frame_ingest_mesh", x_frame_ingest_mesh)
    monkeypatch.setattr(ops, "frame_crop", x_frame_crop)
    monkeypatch.setattr(ops, "frame_emit", x_frame_emit)
    monkeypatch.setattr(ops, "frame_emit_source", x_frame_emit_source)
    monkeypatch.setattr(ops, "track_corners", np_track_corners)


# ---------------------------------------------------------------------------------------------------------------- building frames and sinks
def build_frame(fmt, Y, U, V, extra=0, offset=0, mv=lambda a: a, low=None, split=False, **kw):
    """Samples -> an ingest.Frame of the format: Y [h,w] uint8, U / V [h/2,w/2] (4:2:2: [h,w/2]); `extra` bytes of row padding (255s),
    the planes `offset` bytes into their buffer; p010 stores v8 << 8 | low (low: the six bits under the sample, and the rest).
    split: two-plane formats as `data` + `uv`.  mv moves a host array to where the frame should live."""
    h, w = Y.shape
    if fmt in ("yuyv422", "uyvy422"):
        row = np.zeros((h, 2 * w), np.uint8)
        if fmt == "yuyv422":
            row[:, 0::2], row[:, 1::4], row[:, 3::4] = Y, U, V
        else:
            row[:, 1::2], row[:, 0::4], row[:, 2::4] = Y, U, V
        bufs = [row]
    elif fmt == "gray8":
        bufs = [Y]
    elif fmt == "nv12":
        bufs = [Y, np.stack([U, V], -1).reshape(h // 2, w)]
    elif fmt in ("i420", "yv12"):
        bufs = [Y, np.concatenate([U, V] if fmt == "i420" else [V, U])]
    else:
        w16 = lambda a: ((a.astype(np.uint16) << 8) | (0 if low is None else low[:a.shape[0], :a.shape[1]])).astype("<u2").view(np.uint8)
        bufs = [w16(Y), w16(np.stack([U, V], -1).reshape(h // 2, w))]
    planar = fmt in I.PLANAR
    if len(bufs) == 2 and not split:                   # one buffer: the luma pitch rules; planar chroma rows are half a luma row
        p = bufs[0].shape[1] + (extra & ~1 if planar or fmt == "p010" else extra)
        one = np.full(offset + p * h * 3 // 2, 255, np.uint8)
        body = one[offset:]
        body[:p * h].reshape(h, p)[:, :bufs[0].shape[1]] = bufs[0]
        cp = p // 2 if planar else p
        body[p * h:].reshape(-1, cp)[:, :bufs[1].shape[1]] = bufs[1]
        return I.Frame(mv(one)[offset:], fmt, width=w, height=h, pitch=p, **kw)
    flat = []
    for b in bufs:
        e = extra & ~1 if fmt == "p010" else extra
        buf = np.full(offset + b.shape[0] * (b.shape[1] + e), 255, np.uint8)
        buf[offset:].reshape(b.shape[0], -1)[:, :b.shape[1]] = b
        flat.append((mv(buf)[offset:], b.shape[1] + e))
    if len(flat) == 2:
        return I.Frame(flat[0][0], fmt, width=w, height=h, pitch=flat[0][1], uv=flat[1][0], uv_pitch=flat[1][1], **kw)
    return I.Frame(flat[0][0], fmt, width=w, height=h, pitch=flat[0][1], **kw)


def random_samples(rng, h, w, c422=False):
    return (rng.randint(0, 256, (h, w)).astype(np.uint8),) + tuple(rng.randint(0, 256, (h if c422 else h // 2, w // 2)).astype(np.uint8) for _ in range(2))


def random_frame(rng, fmt, h, w, **kw):
    """A noise frame of any of the eleven formats (p010 with every bit of its words random)."""
    if fmt in ("rgb24", "bgr24", "rgba32", "bgra32"):
        kw.pop("matrix", None)
        extra, offset, mv = kw.pop("extra", 0), kw.pop("offset", 0), kw.pop("mv", lambda a: a)
        kw.pop("split", None)
        bpp = I.BPP[fmt]
        buf = rng.randint(0, 256, offset + h * (w * bpp + extra)).astype(np.uint8)
        return I.Frame(mv(buf)[offset:], fmt, width=w, height=h, pitch=w * bpp + extra, **kw)
    Y, U, V = random_samples(rng, h, w, fmt in I.PACKED_422)
    low = rng.randint(0, 256, (h, w)).astype(np.uint16) if fmt == "p010" else None
    return build_frame(fmt, Y, U, V, low=low, **kw)


def host_record(frame, H, W):
    """An ingest.Frame with host planes -> what the restatements read of its record, planned for an H x W canvas; a frame of a new format
    as the rgb24 record of its converted picture."""
    host = lambda p: None if p is None else np.asarray(p.cpu().numpy() if torch.is_tensor(p) else p)
    out_h, out_w, _ = I.plan(frame, (H, W))
    fmt, m = I.FORMATS[frame.fmt], I.MATRICES[frame.matrix]
    p0, p1, pitch0, pitch1 = host(frame.plane0), host(frame.plane1), frame.pitch, frame.uv_pitch
    if _ext(fmt, m):
        p0, p1 = frame_rgb(p0, p1, pitch0, pitch1, frame.width, frame.height, fmt, m).reshape(-1), None
        pitch0, pitch1, fmt, m = 3 * frame.width, 0, 0, 0
    return types.SimpleNamespace(p0=p0, p1=p1, pitch0=pitch0, pitch1=pitch1, width=frame.width, height=frame.height, format=fmt,
                                 rotate=frame.rotate, matrix=m, out_w=out_w, out_h=out_h)


def x_ingest(frame, H, W):
    """One ingest.Frame of any format -> the [H,W,3] canvas the header asks for."""
    from test_ingest_cpu import np_ingest_picture
    e = host_record(frame, H, W)
    return np_ingest_picture(e.p0, e.p1, e.pitch0, e.pitch1, e.width, e.height, e.format, e.rotate, e.matrix, e.out_w, e.out_h, H, W)


def blank_sink(fmt, w, h, matrix="bt601", extra=5, offset=0, device="cpu", fill=7, **kw):
    """A sink of `fmt` in one buffer filled with `fill`: `extra` bytes of row padding (planar: even), its first byte `offset` bytes in."""
    bpp = I.BPP[fmt]
    two = fmt in I.SEMI_PLANAR or fmt in I.PLANAR
    p = w * bpp + (extra & ~1 if fmt in I.PLANAR else extra)
    buf = torch.full((offset + p * (h * 3 // 2 if two else h),), fill, dtype=torch.uint8, device=device)
    s = E.Sink(buf[offset:], fmt, width=w, height=h, pitch=p, matrix=matrix, **kw)
    s.buffer, s.offset, s.fill = buf, offset, fill
    return s


def assert_padding_untouched(s):
    """The bytes before a blank_sink's first byte and the padding of its plane0 rows still hold the fill."""
    b = s.buffer.cpu().numpy()
    row = s.width * I.BPP[s.fmt]
    assert (b[:s.offset] == s.fill).all(), s.fmt
    if s.pitch > row:
        assert (b[s.offset:s.offset + s.height * s.pitch].reshape(s.height, s.pitch)[:, row:] == s.fill).all(), s.fmt


def sink_yuv(s):
    """A YUV sink's content as (Y, U, V), whatever its layout."""
    p1 = None if s.plane1 is None else s.plane1.cpu().numpy()
    return frame_yuv(s.plane0.cpu().numpy(), p1, s.pitch, s.uv_pitch, s.width, s.height, I.FORMATS[s.fmt])


def assert_yuv(got, want, msg=""):
    for g, w, name in zip(got, want, "YUV"):
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} ({name})")


def expect_canvas_sink(canvas, q, sink, pic_hw=None):
    ph, pw = canvas.shape[:2] if pic_hw is None else pic_hw
    rgb = np_annotate(canvas, q if sink.box else None, pw, ph, sink.width, sink.height, sink.thickness, sink.dot_radius,
                      _colour(sink.line_rgb), _colour(sink.dot_rgb))
    return forward_yuv(rgb, I.MATRICES[sink.matrix], sink.fmt in I.PACKED_422)


def expect_source_sink(frame, q, sink):
    """A source-view YUV sink's expected (Y, U, V) from a frame with HOST planes."""
    host = lambda p: None if p is None else np.asarray(p.cpu().numpy() if torch.is_tensor(p) else p)
    fmt, m, km = I.FORMATS[frame.fmt], I.MATRICES[frame.matrix], I.MATRICES[sink.matrix]
    args = (host(frame.plane0), host(frame.plane1), frame.pitch, frame.uv_pitch, frame.width, frame.height, fmt)
    if _ext(fmt, m):
        rgb = frame_rgb(*args, m)
    else:
        from test_emit_source_cpu import source_planes
        rgb = source_planes(*args, m)[0]
    style = (sink.thickness, sink.dot_radius, _colour(sink.line_rgb), _colour(sink.dot_rgb))
    q = q if sink.box else None
    c422 = sink.fmt in I.PACKED_422
    if frame.fmt == sink.fmt and m == km:
        return pass_through(rgb, frame_yuv(*args), q, sink.width, sink.height, km, c422, style, FWD_X[km][1])
    return forward_yuv(np_annotate(rgb, q, frame.width, frame.height, sink.width, sink.height, *style), km, c422)


def ingest_cpu(frames, H, W, B=None, slots=None, fill=0):
    B = len(frames) if B is None else B
    out = torch.full((B, H, W, 3), fill, dtype=torch.uint8)
    K = torch.full((B, 3, 3), -7.0)
    I.ingest_frames(frames, out, K, slots=slots)
    return out.numpy()


def emit_cpu(canvas, q, sinks):
    imgs = torch.from_numpy(np.ascontiguousarray(canvas))[None]
    pts = torch.zeros((1, 8, 2), dtype=torch.int32) if q is None else torch.from_numpy(np.asarray(q, np.int32).reshape(1, 8, 2))
    E.emit_frames(imgs, pts, torch.tensor([0 if q is None else 1], dtype=torch.int32), sinks, slots=[0] * len(sinks))


def emit_source_cpu(frames, q, sinks, sources, device="cpu"):
    B = len(frames)
    out = torch.zeros((B, 8, 8, 3), dtype=torch.uint8, device=device)
    staged = I.ingest_frames_keep(frames, out, torch.zeros((B, 3, 3), device=device))[1]
    pts = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(q, np.int32), (B, 8, 2)))).to(device)
    E.emit_source_frames(staged, pts, torch.ones(B, dtype=torch.int32, device=device), sinks, sources=sources)


# ---------------------------------------------------------------------------------------------------------------- 1: equivalences
def same_samples(rng, h, w):
    """The same picture in four families: 4:2:0 samples as nv12 / i420 / yv12 / p010, their 4:2:2 doubling as yuyv422 / uyvy422."""
    Y, U, V = random_samples(rng, h, w)
    low = rng.randint(0, 64, (h, w)).astype(np.uint16)                          # random bits under the 10-bit sample's two zero bits
    return Y, U, V, low


@pytest.mark.parametrize("matrix", list(I.MATRICES))
def test_equivalent_frames_give_identical_canvases(cpu_ops, matrix):
    """Ingest, mesh ingest and crop of frames built from the same samples: i420 = yv12 = p010 (v8 << 8) = nv12, yuyv422 = uyvy422 = the
    nv12 frame of the row-doubled chroma... (here: 4:2:2 chroma repeated down a block), gray8 = rgb24 of three equal channels.  For the
    limited-range matrices the nv12 side runs the EXISTING restatement, untouched by this file's."""
    rng = np.random.RandomState(1)
    h, w, H, W = 46, 62, 30, 40
    Y, U, V, low = same_samples(rng, h, w)
    K = np.array([[60.0, 0, 30.5], [0, 60.0, 22.5], [0, 0, 1]])
    lens = I.Lens("brown", (-0.2, 0.05, 0.001, -0.0005))
    for kw in (dict(), dict(rotate=90), dict(K=K, lens=lens)):
        mk = lambda fmt, **k: build_frame(fmt, Y, U, V, extra=6, matrix=matrix, low=low, **k, **kw)
        frames = [mk("nv12"), mk("i420"), mk("yv12", split=True), mk("p010"), mk("i420", split=True, offset=1)]
        U2, V2 = np.repeat(U, 2, 0), np.repeat(V, 2, 0)
        frames += [build_frame(f, Y, U2, V2, extra=3, offset=o, matrix=matrix, **kw) for f, o in (("yuyv422", 0), ("uyvy422", 1))]
        grey = [build_frame("gray8", Y, None, None, extra=3, **kw), I.Frame(np.repeat(Y[..., None], 3, -1), "rgb24", **kw)]
        Hc, Wc = (W, H) if kw.get("rotate") else (H, W)
        got = ingest_cpu(frames + grey, Hc, Wc)
        assert got[0].any() and (got[0] != got[7]).any()
        for i in range(1, 7):                          # (a 4:2:2 frame whose chroma rows repeat in pairs holds the 4:2:0 picture)
            np.testing.assert_array_equal(got[i], got[0], err_msg=f"{matrix} {kw.keys()} {frames[i].fmt}")
        np.testing.assert_array_equal(got[7], got[8], err_msg="gray8")
        if "lens" in kw:
            continue                                   # (a lens frame has no source record: its crop is its canvas's)
        out = torch.zeros((9, Hc, Wc, 3), dtype=torch.uint8)
        staged = I.ingest_frames_keep(frames + grey, out, torch.zeros((9, 3, 3)))[1]
        hinv = torch.from_numpy(np.repeat(homographies(rng, 1, zoom=(1.5, 4.0), shift=(-3, 8)), 9, 0))
        crops = ops.frame_crop(staged.table, torch.arange(9, dtype=torch.int32), out, hinv, 20, 28).numpy()
        assert crops[0].any()
        for i in range(1, 7):
            np.testing.assert_array_equal(crops[i], crops[0], err_msg=f"crop {matrix} {frames[i].fmt}")
        np.testing.assert_array_equal(crops[7], crops[8], err_msg="crop gray8")


@pytest.mark.parametrize("matrix", list(I.MATRICES))
def test_equivalent_sinks_hold_the_same_samples(cpu_ops, matrix):
    """Canvas and source view: an i420 / yv12 sink's planes are the de-interleaved planes of the nv12 sink of the same call (for the
    limited-range matrices the nv12 sink is filled by the EXISTING restatement); a yuyv422 and a uyvy422 sink hold the same samples."""
    rng = np.random.RandomState(2)
    w, h = 70, 46
    canvas = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    frame = I.Frame(canvas.copy())
    for view, (dw, dh) in (("canvas", (0, 0)), ("canvas", (8, 8)), ("source", (0, 0)), ("source", (-10, -10))):
        sinks = [blank_sink(f, w + dw, h + dh, matrix, extra=4 + i, offset=i % 2, view=view, pose="raw") for i, f in enumerate(YUV8)]
        if view == "canvas":
            emit_cpu(canvas, BOX, sinks)
        else:
            emit_source_cpu([frame], SRC_BOX, sinks, [0] * 5)
        nv12, yuyv, uyvy, i420, yv12 = (sink_yuv(s) for s in sinks)
        assert nv12[0].std() > 10
        if matrix in ("bt601", "bt709"):               # the existing restatement's own form of the same sink
            s = sinks[0]
            want = np_nv12(np_annotate(canvas, BOX if view == "canvas" else SRC_BOX, w, h, s.width, s.height), I.MATRICES[matrix])
            assert_yuv(nv12, (want[0], want[1][:, 0::2], want[1][:, 1::2]), "nv12 against test_emit_cpu")
        assert_yuv(i420, nv12, f"{view} i420")
        assert_yuv(yv12, nv12, f"{view} yv12")
        assert_yuv(uyvy, yuyv, f"{view} uyvy422")
        np.testing.assert_array_equal(yuyv[0], nv12[0])                         # Y is per pixel in every layout
        for s in sinks:                                # the row padding and the bytes before the sink are not written
            assert_padding_untouched(s)
            assert_yuv(sink_yuv(s), (expect_canvas_sink(canvas, BOX, s) if view == "canvas" else expect_source_sink(frame, SRC_BOX, s)), s.fmt)


# ---------------------------------------------------------------------------------------------------------------- 2: integer against float
def _grid(step, top, must):
    return np.unique(np.concatenate([np.arange(0, top + 1, step), must]))


@pytest.mark.parametrize("matrix", [2, 3])
def test_full_range_tap_is_within_one_level_of_float64(matrix):
    """Every (Y, U, V) on a grid of step 5 with the range's landmarks.  Bound 1: the constants are off by at most 2^-21 (times |d|, |e| <=
    128: under 1e-4 levels), the shift's rounding and the float's rounding move a value by at most 1/2 each."""
    g = _grid(5, 255, [0, 16, 128, 235, 240, 255])
    Y, U, V = np.meshgrid(g, g, g, indexing="ij")
    got = yuv_to_rgb(Y, U, V, matrix)
    kvr, kug, kvg, kub = FLOAT[matrix][0]
    d, e = U - 128.0, V - 128.0
    want = np.clip(np.rint(np.stack([Y + kvr * e, Y - kug * d - kvg * e, Y + kub * d], -1)), 0, 255)
    diff = np.abs(got - want)
    print(f"matrix {matrix}: max {diff.max():.0f} level, {100 * (diff > 0).mean():.3f} % of the values differ")
    assert diff.max() <= 1
    assert (got[:, g == 128, g == 128][:, 0] == g[:, None]).all()              # grey stays grey, exactly


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
def test_p010_tap_is_within_one_level_of_float64(matrix):
    """10-bit samples on a grid of step 20 (every 8-bit step of 5) with the landmarks, both ranges.  The float value is the matrix on
    the 10-bit samples scaled to 8 bits (a quarter); the same bound (|d|, |e| <= 128 after the scaling).  And the multiples of 4 give the 8-bit tap bit for bit."""
    g = _grid(20, 1023, [0, 64, 512, 940, 960, 1023])
    Y, U, V = np.meshgrid(g, g, g, indexing="ij")
    got = yuv_to_rgb(Y, U, V, matrix, bits=10)
    CY, yoff, CVR, CUG, CVG, CUB = INV_X[matrix]
    c, d, e = np.maximum(Y - 4.0 * yoff, 0) / 4, (U - 512.0) / 4, (V - 512.0) / 4
    # full range: the matrix the header names; limited range: the NV12 constants, whose stated matrix is their own value k / 2^20
    k = [1.0] + list(FLOAT[matrix][0]) if matrix >= 2 else [v / 2.0 ** 20 for v in (CY, CVR, CUG, CVG, CUB)]
    want = np.clip(np.rint(np.stack([k[0] * c + k[1] * e, k[0] * c - k[2] * d - k[3] * e, k[0] * c + k[4] * d], -1)), 0, 255)
    assert np.abs(got - want).max() <= 1
    g8 = np.arange(0, 256, 5)
    Y, U, V = np.meshgrid(g8, g8, g8, indexing="ij")
    np.testing.assert_array_equal(yuv_to_rgb(4 * Y, 4 * U, 4 * V, matrix, bits=10), yuv_to_rgb(Y, U, V, matrix))
    # the bound the header states: the limited-range sums leave 32 bits
    assert 1220542 * 959 + 2214593 * 511 + 2 ** 21 > 2 ** 31


@pytest.mark.parametrize("matrix", [2, 3])
def test_full_range_forward_is_within_one_level_of_float64(matrix):
    """Every (R, G, B) on a grid of step 5 as a uniform 2 x 2 picture, 4:2:0 and 4:2:2: Y = Kr R + Kg G + Kb B, Cb = (B - Y) / (2 (1 -
    Kb)) + 128, Cr likewise, rounded; the same bound.  The Y rows sum to 2^20 and black is (0, 128, 128)."""
    g = _grid(5, 255, [0, 16, 128, 235, 240, 255])
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 1, 3)
    pic = np.repeat(np.repeat(rgb, 2, 0), 2, 1).astype(np.uint8)               # rows 2 i, 2 i + 1: colour i
    kr, kb = FLOAT[matrix][1]
    p = rgb[:, 0].astype(np.float64)
    Yf = kr * p[:, 0] + (1 - kr - kb) * p[:, 1] + kb * p[:, 2]
    want = [np.clip(np.rint(v), 0, 255) for v in (Yf, (p[:, 2] - Yf) / (2 * (1 - kb)) + 128, (p[:, 0] - Yf) / (2 * (1 - kr)) + 128)]
    for c422 in (False, True):
        Y, U, V = forward_yuv(pic, matrix, c422)
        for got, w, name in ((Y[0::2, 0], want[0], "Y"), (U[0::(2 if c422 else 1), 0], want[1], "Cb"), (V[0::(2 if c422 else 1), 0], want[2], "Cr")):
            assert np.abs(got.astype(np.float64) - w).max() <= 1, (matrix, c422, name)
    (cy, cb, cr), yoff = FWD_X[matrix]
    assert sum(cy) == 2 ** 20 and sum(cb) == 0 and sum(cr) == 0 and yoff == 0
    assert [int(v[0, 0]) for v in forward_yuv(np.zeros((2, 2, 3), np.uint8), matrix, False)] == [0, 128, 128]
    assert [int(v[0, 0]) for v in forward_yuv(np.full((2, 2, 3), 255, np.uint8), matrix, True)] == [255, 128, 128]


def test_limited_range_is_unchanged():
    """Matrix values 0 / 1 on the new layouts are the NV12 formula with its constants: this file's tap rule against test_ingest_cpu's."""
    from test_ingest_cpu import yuv_formula
    rng = np.random.RandomState(3)
    for m in (0, 1):
        for y, u, v in rng.randint(0, 256, (200, 3)):
            assert tuple(yuv_to_rgb(y, u, v, m)) == yuv_formula(int(y), int(u), int(v), m)


# ---------------------------------------------------------------------------------------------------------------- 3: pass-through
@pytest.mark.parametrize("fmt", YUV8)
def test_pass_through(cpu_ops, fmt):
    rng = np.random.RandomState(4)
    w, h = 72, 46 if fmt not in I.PACKED_422 else 45                           # (4:2:2: any height)
    c422 = fmt in I.PACKED_422
    for matrix, other in (("bt601-full", "bt709-full"), ("bt709", "bt709-full")) + ((("bt601", "bt709"),) if fmt != "nv12" else ()):
        frame = random_frame(rng, fmt, h, w, matrix=matrix, extra=3, offset=1)  # odd pitches, an unaligned base
        raw = frame_yuv(frame.plane0, frame.plane1, frame.pitch, frame.uv_pitch, w, h, I.FORMATS[fmt])
        mk = lambda dw=0, dh=0, m=matrix, **kw: blank_sink(fmt, w + dw, h + dh, m, extra=7, offset=3, view="source", **kw)
        plain, boxed, big, small, cross = mk(box=False), mk(), mk(8, 8), mk(-10, -10), mk(m=other)
        emit_source_cpu([frame], SRC_BOX, [plain, boxed, big, small, cross], [0] * 5)
        assert_yuv(sink_yuv(plain), raw, f"{fmt} {matrix}: a byte copy without a box")
        m = I.MATRICES[matrix]
        rgb = frame_rgb(frame.plane0, frame.plane1, frame.pitch, frame.uv_pitch, w, h, I.FORMATS[fmt], m)
        cov = np_annotate(np.zeros_like(rgb), SRC_BOX, w, h, w, h, line=(1, 1, 1), dot=(1, 1, 1)).any(-1)
        assert 200 < cov.sum() < cov.size // 2
        block = cov[:, 0::2] | cov[:, 1::2]
        block = block if c422 else block[0::2] | block[1::2]
        Yf, Uf, Vf = forward_yuv(np_annotate(rgb, SRC_BOX, w, h, w, h), m, c422)
        gy, gu, gv = sink_yuv(boxed)
        np.testing.assert_array_equal(gy[~cov], raw[0][~cov])                   # uncovered Y bytes and untouched blocks: the source's
        np.testing.assert_array_equal(gu[~block], raw[1][~block])
        np.testing.assert_array_equal(gv[~block], raw[2][~block])
        np.testing.assert_array_equal(gy[cov], Yf[cov])                         # touched ones: the forward formula
        np.testing.assert_array_equal(gu[block], Uf[block])
        np.testing.assert_array_equal(gv[block], Vf[block])
        assert (gy[cov] != raw[0][cov]).any() and (gu[block] != raw[1][block]).any()
        yb = FWD_X[m][1]
        gy, gu, gv = sink_yuv(big)                      # a larger sink pads with what black converts to in the sink's range
        assert (gy[h:] == yb).all() and (gy[:, w:] == yb).all() and (gu[:, w // 2:] == 128).all() and (gv[-4:] == 128).all()
        for s in (boxed, big, small):
            assert_yuv(sink_yuv(s), expect_source_sink(frame, SRC_BOX, s), f"{fmt} {matrix} {s.width}x{s.height}")
        # a matrix mismatch goes through RGB: the full conversion, no byte is passed through
        want = forward_yuv(np_annotate(rgb, SRC_BOX, w, h, w, h), I.MATRICES[other], c422)
        assert_yuv(sink_yuv(cross), want, f"{fmt} {matrix} -> {other}")
        assert (want[0] != raw[0]).any()


def test_other_pairs_go_through_rgb(cpu_ops):
    """yuyv422 <-> uyvy422, i420 <-> nv12, p010 / gray8 into anything: the converted picture through the forward rule; and a new frame
    into the five first sink formats is the existing rule on the converted picture."""
    rng = np.random.RandomState(5)
    w, h = 72, 46
    for sfmt, kfmt in (("yuyv422", "uyvy422"), ("uyvy422", "yuyv422"), ("i420", "nv12"), ("nv12", "i420"), ("p010", "yv12"), ("gray8", "yuyv422"),
                       ("bgra32", "i420"), ("p010", "nv12")):
        frame = random_frame(rng, sfmt, h, w, matrix="bt709", extra=2, offset=1)
        sink = blank_sink(kfmt, w, h, "bt709", view="source")
        emit_source_cpu([frame], SRC_BOX, [sink], [0])
        rgb = x_ingest(frame, h, w)                     # a same-size, unturned ingest: the picture converted per pixel
        want = forward_yuv(np_annotate(rgb, SRC_BOX, w, h, w, h), 1, kfmt in I.PACKED_422)
        assert_yuv(sink_yuv(sink), want, f"{sfmt} -> {kfmt}")
    frame = random_frame(rng, "yuyv422", h, w, matrix="bt601-full")
    sink = E.Sink(torch.zeros((h, w, 3), dtype=torch.uint8), "bgr24", view="source")
    emit_source_cpu([frame], SRC_BOX, [sink], [0])
    np.testing.assert_array_equal(sink.plane0.numpy().reshape(h, w, 3)[..., ::-1], np_annotate(x_ingest(frame, h, w), SRC_BOX, w, h, w, h))


# ---------------------------------------------------------------------------------------------------------------- 4: validation, layout
def test_frame_validation():
    z = lambda *s, dt=np.uint8: np.zeros(s, dt)
    for fmt in NEW:
        assert fmt in I.FORMATS and fmt in I.BPP
    assert [I.BPP[f] for f in NEW] == [2, 2, 1, 1, 2, 1] and [I.FORMATS[f] for f in NEW] == [5, 6, 7, 8, 9, 10]
    assert I.MATRICES == {"bt601": 0, "bt709": 1, "bt601-full": 2, "bt709-full": 3}
    # geometries
    f = I.Frame(z(9, 8, 2), "yuyv422")
    assert (f.width, f.height, f.pitch, f.plane1) == (8, 9, 16, None)
    f = I.Frame(z(9, 20), "uyvy422", width=8)
    assert (f.width, f.height, f.pitch) == (8, 9, 20)
    f = I.Frame(z(12, 10), "i420", width=8)
    assert (f.width, f.height, f.pitch, f.uv_pitch, f.plane1.shape[0]) == (8, 8, 10, 5, 7 * 5 + 4)
    f = I.Frame(z(8, 8), "yv12", uv=z(8, 6))
    assert (f.height, f.uv_pitch, f.plane1.shape[0]) == (8, 6, 7 * 6 + 4)
    f = I.Frame(z(12, 8, dt=np.uint16), "p010")
    assert (f.width, f.height, f.pitch, f.uv_pitch, f.plane0.dtype) == (8, 8, 16, 16, np.uint8)
    f = I.Frame(torch.zeros(12 * 20, dtype=torch.uint8), "p010", width=8, height=8, pitch=20)
    assert (f.pitch, f.uv_pitch) == (20, 20)
    f = I.Frame(z(8, 8, dt=np.uint16), "p010", uv=z(4, 4, 2, dt=np.uint16))
    assert (f.uv_pitch, f.plane1.shape[0]) == (16, 64)
    f = I.Frame(z(7, 9), "gray8", width=5)
    assert (f.width, f.height, f.pitch) == (5, 7, 9)
    # errors
    for bad, match in ((lambda: I.Frame(z(8, 7, 2), "yuyv422"), "even width"),
                       (lambda: I.Frame(z(8, 14), "uyvy422", width=7), "even width"),
                       (lambda: I.Frame(z(9, 6), "i420", width=5), "even"),
                       (lambda: I.Frame(z(7, 8), "yv12", uv=z(7, 4)), "even"),
                       (lambda: I.Frame(z(9, 6, dt=np.uint16), "p010", width=5), "even"),
                       (lambda: I.Frame(z(12 * 19), "p010", width=8, height=8, pitch=19), "even"),
                       (lambda: I.Frame(z(12, 9), "i420", width=8), "even pitch"),
                       (lambda: I.Frame(z(10, 8), "i420"), "H\\*3/2"),
                       (lambda: I.Frame(z(8, 10), "yuyv422", width=6), "pitch"),
                       (lambda: I.Frame(z(12, 7), "yv12", width=8), "pitch"),
                       (lambda: I.Frame(z(8, 8), "i420", uv=z(8, 3)), "pitch"),
                       (lambda: I.Frame(z(8, 8), "gray8", width=9), "pitch"),
                       (lambda: I.Frame(z(100), "p010", width=8, height=8), "holds"),
                       (lambda: I.Frame(z(8, 8, 3), "yuyv422"), "cannot be"),
                       (lambda: I.Frame(z(12, 8, 1), "i420"), "cannot be"),
                       (lambda: I.Frame(z(8, 8), "i420", uv=z(4, 4, 2)), "does not belong"),
                       (lambda: I.Frame(z(8, 8), "yv12", uv=z(4, 4)), "does not belong"),
                       (lambda: I.Frame(z(8, 8, 2), "yuyv422", uv=z(4, 8)), "uv"),
                       (lambda: I.Frame(z(8, 8), "gray8", uv=z(4, 8)), "uv"),
                       (lambda: I.Frame(z(8, 8), "i420", uv=torch.zeros((8, 4), dtype=torch.uint8)), "same kind"),
                       (lambda: I.Frame(z(8, 8, 2, dt=np.uint16), "yuyv422"), "uint8"),
                       (lambda: I.Frame(z(8, 8, 2), "yuyv"), "format"),
                       (lambda: I.Frame(z(8, 8, 2), "yuyv422", matrix="bt2020"), "matrix")):
        with pytest.raises(ValueError, match=match):
            bad()


def test_sink_validation_and_layout():
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    for fmt in ("p010", "gray8"):
        with pytest.raises(ValueError, match="cannot be written"):
            E.Sink(z(12, 16), fmt, width=8, height=8)
    for fmt in YUV8:
        for matrix in I.MATRICES:
            s = blank_sink(fmt, 8, 8, matrix)
            assert (s.fmt, s.matrix) == (fmt, matrix)
    with pytest.raises(ValueError, match="even width"):
        E.Sink(z(8, 7, 2), "yuyv422")
    with pytest.raises(ValueError, match="matrix"):
        E.Sink(z(12, 8), "i420", matrix="bt2020")
    # the spans a host sink travels in cover the second chroma plane
    s = E.Sink(z(12, 10), "yv12", width=8)
    (field, view), = s._spans()
    assert field == "both" and view.numel() == 8 * 10 + 7 * 5 + 4 and s.plane1.numel() == 7 * 5 + 4
    s = E.Sink(z(8, 8), "i420", uv=z(8, 4))
    assert [(f, v.numel()) for f, v in s._spans()] == [("plane0", 64), ("plane1", 32)]
    l = lib.load()
    assert C.sizeof(lib.G6dFrame) == l.g6d_sizeof_frame_desc() == 96
    assert C.sizeof(lib.G6dSink) == l.g6d_sizeof_sink_desc() == 72
    assert l.g6d_abi_version() == 12
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gen6d_hip.h")).read()
    for name, value in (("YUYV422", 5), ("UYVY422", 6), ("I420", 7), ("YV12", 8), ("P010", 9), ("GRAY8", 10)):
        assert re.search(rf"G6D_FMT_{name} = {value}\b", header), name
        assert I.FORMATS[name.lower()] == value


# ---------------------------------------------------------------------------------------------------------------- 5: tracker
def camera_frame(img, fmt, matrix, size=(240, 320), K=None):
    """An [h,w,3] picture -> an ingest.Frame of `size` in any format (nearest-neighbour scaled; YUV through the forward rule)."""
    h, w = size
    big = np.ascontiguousarray(img[(np.arange(h) * img.shape[0]) // h][:, (np.arange(w) * img.shape[1]) // w])
    if fmt in ("rgb24", "bgr24", "rgba32", "bgra32"):
        from test_ingest_cpu import rgb_to
        return I.Frame(rgb_to(big, fmt), fmt, K=K)
    Y, U, V = forward_yuv(big, I.MATRICES[matrix], fmt in I.PACKED_422)
    return build_frame(fmt, Y, U, V, extra=2, matrix=matrix, K=K)


def test_tracker_takes_all_eleven_formats_in_one_tick(scene, cpu_ops, monkeypatch):
    """One eager tracker, one lane, eleven streams, a frame of each format per tick with crops="source", one canvas sink and one source
    sink: one ingest, one emit and one emit_source launch per lane and tick, and a frame_crop launch in place of every query warp."""
    est, frames, Ks = scene
    ref_ops.patch_ops(monkeypatch)
    monkeypatch.setattr(ops, "track_gather", np_track_gather)
    monkeypatch.setattr(ops, "track_commit", np_track_commit)
    calls = []
    for name in ("frame_ingest", "frame_ingest_mesh", "frame_crop", "frame_emit", "frame_emit_source"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _name=name, **k: (calls.append(_name), _fn(*a, **k))[1])
    hw = (120, 160)
    matrices = list(I.MATRICES)
    src = lambda t: [camera_frame(frames[(t + i) % 4], fmt, matrices[i % 4]) for i, fmt in enumerate(ALL)]
    tr = T.StreamTracker(est, 11, batch=11, lanes=1, graphs=False, frame_size=hw, crops="source", track_iter=2)
    z = lambda *s: torch.full(s, 7, dtype=torch.uint8)
    for t in range(2):                                 # an init push, then a tracked tick
        fr = src(t)
        assert fr[6].fmt == "uyvy422" and fr[6].matrix == "bt601-full"
        canvas_sink = E.Sink(z(180, 160), "i420", matrix="bt601-full")
        source_sink = E.Sink(z(240, 640), "uyvy422", view="source", matrix="bt601-full")        # stream 6's own format and matrix: a pass-through
        sinks = [None] * 11
        sinks[2], sinks[6] = canvas_sink, source_sink
        del calls[:]
        tr.push(list(range(11)), fr, sinks=sinks)
        # first frames are ingested and estimated in chunks of INIT_CHUNK streams (sinks 2 and 6 lie in the first); a tracked tick is
        # one launch of each kind per lane, with a crop launch where canvas mode has its query warp (the refiner's other warps stay)
        chunks = 1 if t else -(-11 // T.INIT_CHUNK)
        assert calls.count("frame_ingest") == chunks and calls.count("frame_ingest_mesh") == 0
        assert calls.count("frame_emit") == 1 and calls.count("frame_emit_source") == 1
        assert calls.count("frame_crop") == (2 if t else chunks * (1 + est.cfg["refine_iter"]))
        r = tr.result()
        assert set(r) == set(range(11)) and all(np.isfinite(r[s][0]).all() for s in r)
        for s in range(11 if t else 0):                # tracked frames sit in the lane's static slots
            np.testing.assert_array_equal(tr._lanes[0].img[s].numpy(), x_ingest(fr[s], *hw), err_msg=f"tick {t} stream {s} {fr[s].fmt}")
        assert sink_yuv(canvas_sink)[0].std() > 5 and sink_yuv(source_sink)[0].std() > 5
        raw = frame_yuv(fr[6].plane0, None, fr[6].pitch, 0, 320, 240, 6)
        assert (sink_yuv(source_sink)[0] == raw[0]).mean() > 0.9               # the camera's own bytes outside the box


# ---------------------------------------------------------------------------------------------------------------- 6: compiler metadata
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,kernels", [("ingest.hip", ("frame_ingest_kernel", "frame_ingest_lens_kernel")), ("frame_crop.hip", ("frame_crop_kernel",)),
                                         ("emit.hip", ("frame_emit_kernel",)), ("emit_source.hip", ("frame_emit_source_kernel",))])
def test_kernels_have_no_scratch(tmp_path, src, kernels):
    """With the new formats' paths in them, the five kernels keep a thread's taps and pixels in registers: no scratch, no spilled
    vector registers.  Compiler metadata; cross-compiles without a GPU."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / (src + ".s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = out.read_text().split("\n  - .agpr_count")                         # one metadata block per kernel
    for k in kernels:
        body, = [b for b in blocks[1:] if re.search(r"\.name:\s+\S*" + k + r"E", b)]
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", body).group(1))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0, k
