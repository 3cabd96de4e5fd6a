"""Device-side annotated frame output (reference predict.py:60-72 + utils/draw_utils.py draw_bbox_3d): the working-resolution images of a
batch with the object's projected 3-D box drawn on them (red corner discs, twelve blue edges on top), written in the format an encoder
or a display takes, in ONE launch of g6d_frame_emit (csrc/emit.hip) for any number of destinations.  The output side of gen6d_amd.ingest.

A `Sink` describes one destination the way `ingest.Frame` describes a source: packed rgb24 / bgr24 / rgba32 / bgra32, NV12, planar i420 /
yv12 (a software encoder's input) or packed 4:2:2 yuyv422 / uyvy422 (a capture-card style display path), limited or full range, any
size up to 8192 and any row pitch, in device memory or in pinned host memory.  The picture sits at the sink's top-left corner at working resolution:
a larger sink (an encoder's aligned surface, an odd picture under NV12) is padded with black, a smaller one crops; nothing is scaled or
rotated.  `project_corners` turns poses into integer pixel corners on the device (g6d_track_corners), `emit_frames` fills the sinks.
The drawing and the colour conversion are the exact integer rules of include/gen6d_hip.h, not cv2's.

A sink with view="source" shows the camera's own frame instead of the canvas: the `ingest.Frame` as it was delivered (full resolution,
not turned) with the box drawn in its pixel grid, in ONE launch of g6d_frame_emit_source (csrc/emit_source.hip) that reads the frame
table an ingest launch left on the device (`ingest_frames_keep`, `emit_source_frames`).  A frame into a sink of
the same format among nv12 / i420 / yv12 / yuyv422 / uyvy422 and the same matrix passes through: bytes the box does not cover are the
camera's bytes; every other pair goes through RGB.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import ingest as I
from . import lib as _lib
from . import ops

POSES = {"raw": 0, "smooth": 1}
VIEWS = ("canvas", "source")
MAX_STYLE = 255                     # thickness and dot radius the 64-bit edge rule is bounded for (include/gen6d_hip.h)


def _rgb(color, what):
    c = [int(v) for v in color]
    if len(c) != 3 or any(not 0 <= v <= 255 for v in c):
        raise ValueError(f"Sink: {what} must be three values in 0..255 (R, G, B)")
    return (c[0] << 16) | (c[1] << 8) | c[2]


class Sink:
    """One destination.  data: a uint8 torch tensor, on the device or in PINNED host memory, [H,W,C] (C = 3 / 4 as the format says; sizes and
    the pitch are taken from it), [rows, row bytes] or a flat buffer (give width / height / pitch).  NV12: either one [H*3/2, pitch]
    buffer (Y rows, then H/2 rows of interleaved UV) or `data` = Y plane and `uv` = UV plane; even width and height.  i420 / yv12 and
    yuyv422 / uyvy422: the layouts of `ingest.Frame` (planar: one buffer of contiguous planes, or `uv` = the two chroma planes
    stacked; 4:2:2: even width, any height).  p010 and gray8 cannot be written.
    pose: which pose's box is drawn, "smooth" or "raw" (predict.py writes both pictures of a frame).  matrix (YUV formats): "bt601" /
    "bt709" (limited range) or "bt601-full" / "bt709-full" (full range: black is Y = 0).  Style: thickness, dot_radius, line_color / dot_color (R, G, B), box=False for the plain picture; the defaults are
    draw_bbox_3d's.  A HOST sink's planes travel in one copy each, from the first row's first byte to the last row's last: the row padding
    in between is overwritten with zeros.  Host sinks therefore cannot share rows of one surface (two halves of a picture, a
    sub-rectangle of a larger image); device sinks, which the kernel writes pixel by pixel, can.
    view: "canvas" (the working-resolution picture) or "source": the stream's own camera frame of this push, the `ingest.Frame` as the
    camera delivered it (not scaled, not turned), with the box drawn in the source's pixel grid.  The sink has the source's size, or is
    larger (padded black) or smaller (cropped from the top-left), as a canvas sink relates to its picture.  thickness and dot_radius
    are in SINK pixels and are not scaled with the resolution: on a 4K frame the defaults (2, 2) are thin, so choose them for the
    size you display.  A source-view sink needs a tracker with `frame_size` (or `emit_source_frames`) and a frame without a lens."""

    def __init__(self, data, fmt="nv12", width=None, height=None, pitch=None, uv=None, uv_pitch=None, matrix="bt601", pose="smooth",
                 thickness=2, dot_radius=2, line_color=(0, 0, 255), dot_color=(255, 0, 0), box=True, view="canvas"):
        if not torch.is_tensor(data) or (uv is not None and not torch.is_tensor(uv)):
            raise ValueError("Sink: a destination is a torch tensor (device memory or pinned host memory)")
        if view not in VIEWS:
            raise ValueError(f"Sink: view must be 'canvas' or 'source', not {view!r}")
        if pose not in POSES:
            raise ValueError(f"Sink: pose must be 'smooth' or 'raw', not {pose!r}")
        if not 0 <= int(thickness) <= MAX_STYLE or not 0 <= int(dot_radius) <= MAX_STYLE:
            raise ValueError(f"Sink: thickness and dot_radius must lie in 0..{MAX_STYLE}")
        if fmt in I.READ_ONLY:
            raise ValueError(f"Sink: a {fmt} picture cannot be written (p010 and gray8 are formats of a source Frame only); the written "
                             f"formats are {sorted(f for f in I.FORMATS if f not in I.READ_ONLY)}")
        try:                                   # the plane, pitch and extent rules of a source picture are those of a destination
            f = I.Frame(data, fmt, width=width, height=height, pitch=pitch, uv=uv, uv_pitch=uv_pitch, matrix=matrix)
        except ValueError as e:
            raise ValueError("Sink: " + str(e).removeprefix("Frame: ")) from None
        for plane, src in ((f.plane0, data), (f.plane1, data if uv is None else uv)):
            if plane is not None and plane.untyped_storage().data_ptr() != src.untyped_storage().data_ptr():
                raise ValueError("Sink: the tensor's layout cannot be written through a row pitch (unit-stride rows expected)")
        self.fmt, self.width, self.height, self.pitch, self.uv_pitch, self.matrix = f.fmt, f.width, f.height, f.pitch, f.uv_pitch, f.matrix
        self.plane0, self.plane1 = f.plane0, f.plane1
        self.pose, self.box, self.view = pose, bool(box), view
        self.thickness, self.dot_radius = int(thickness), int(dot_radius)
        self.line_rgb, self.dot_rgb = _rgb(line_color, "line_color"), _rgb(dot_color, "dot_color")

    @property
    def device(self):
        return self.plane0.device

    def placement(self, device):
        """'device' when the sink lives on `device` (the kernel writes it directly), 'host' when it is pinned host memory and `device` a
        GPU (rendered into device staging, then copied).  Pageable host memory and other devices raise ValueError."""
        device = torch.device(device)
        planes = [p for p in (self.plane0, self.plane1) if p is not None]
        if all(p.device.type == device.type and (p.device.index in (None, device.index) or device.index is None) for p in planes):
            return "device"
        if device.type == "cuda" and all(p.device.type == "cpu" for p in planes):
            if not all(p.is_pinned() for p in planes):
                raise ValueError("Sink: a host destination must be pinned memory (tensor.pin_memory()); pageable memory cannot be "
                                 "written without stalling the stream")
            return "host"
        raise ValueError(f"Sink: the destination lives on {self.device}, the images on {device}")

    def _spans(self):
        """The sink's memory as [(first plane field, flat uint8 view)]: one span when both planes share a buffer, else one per plane."""
        if self.plane1 is None:
            return [("plane0", self.plane0)]
        a, b = self.plane0, self.plane1
        if a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr():
            lo = min(a.storage_offset(), b.storage_offset())
            hi = max(a.storage_offset() + a.numel(), b.storage_offset() + b.numel())
            return [("both", torch.as_strided(a, (hi - lo,), (1,), lo))]
        return [("plane0", a), ("plane1", b)]


def project_corners(table, K, slot_stream, box, pts=None, valid=None):
    """Per slot b, the box [8,3] under row slot_stream[b] of a pose table [S,12] and K[b] -> (pts int32 [B,8,2], valid int32 [B]); a thin
    wrapper over ops.track_corners (g6d_track_corners).  For poses of `predict_many`, pass them as the table with slot_stream = arange."""
    return ops.track_corners(table, K, slot_stream, box, pts, valid)


def _fill(what, sinks, dev, slots, sizes, sets, stream, launch):
    """The part every emit launch shares: the descriptor table of `sinks` (sink i: slot slots[i], picture sizes[i]) is built and
    uploaded through pinned memory, host sinks get device staging (zeroed), `launch(table, n)` runs on `stream` (the current stream if
    None) and the staging is copied out, one non-blocking copy per buffer."""
    n = len(sinks)
    cuda = dev.type == "cuda"
    size = C.sizeof(_lib.G6dSink)
    table = (_lib.G6dSink * max(n, 1))()
    staged, total = [], 0                      # host sinks: (sink index, span field, host view, offset in the staging allocation)
    for i, s in enumerate(sinks):
        if not isinstance(s, Sink):
            raise ValueError(f"{what}: Sink objects expected")
        where = s.placement(dev)
        e = table[i]
        e.pitch0, e.pitch1, e.width, e.height = s.pitch, s.uv_pitch, s.width, s.height
        e.format, e.matrix, e.slot = I.FORMATS[s.fmt], I.MATRICES[s.matrix], slots[i]
        e.pic_h, e.pic_w = sizes[i]
        e.thickness, e.dot_radius, e.line_rgb, e.dot_rgb = s.thickness, s.dot_radius, s.line_rgb, s.dot_rgb
        e.box = (POSES[s.pose] if sets == 2 else 0) if s.box else -1
        if where == "device":
            e.plane0 = s.plane0.data_ptr()
            e.plane1 = 0 if s.plane1 is None else s.plane1.data_ptr()
        else:
            for field, view in s._spans():
                staged.append((i, field, view, total))
                total += (view.numel() + 255) & ~255
    if n == 0:
        return
    with (torch.cuda.stream(stream) if (cuda and stream is not None) else contextlib.nullcontext()):
        if cuda:
            cur = torch.cuda.current_stream(dev)
            for s in sinks:
                if s.plane0.device.type == "cuda":
                    s.plane0.record_stream(cur)
                    if s.plane1 is not None:
                        s.plane1.record_stream(cur)
            stage = torch.zeros(total, dtype=torch.uint8, device=dev) if total else None      # zeros: what a host sink's row padding receives
            for i, field, view, off in staged:
                s, base = sinks[i], stage.data_ptr() + off
                if field == "both":
                    lo = min(s.plane0.storage_offset(), s.plane1.storage_offset())
                    table[i].plane0, table[i].plane1 = base + s.plane0.storage_offset() - lo, base + s.plane1.storage_offset() - lo
                else:
                    setattr(table[i], field, base)
            host = torch.empty(n * size, dtype=torch.uint8, pin_memory=True)
            host.numpy()[:] = np.frombuffer(table, np.uint8, n * size)
            buf = torch.empty(n * size, dtype=torch.uint8, device=dev)
            buf.copy_(host, non_blocking=True)
        else:
            buf = torch.from_numpy(np.frombuffer(table, np.uint8, n * size).copy())
        launch(buf, n)
        for i, field, view, off in staged:
            view.copy_(stage[off:off + view.numel()], non_blocking=True)


def _corner_sets(what, pts, valid, B):
    if pts.dim() == 3:
        pts, valid = pts[None], valid[None]
    if pts.dim() != 4 or pts.shape[0] not in (1, 2) or tuple(pts.shape[1:]) != (B, 8, 2) or tuple(valid.shape) != (pts.shape[0], B):
        raise ValueError(f"{what}: pts int32 [B,8,2] / [2,B,8,2] and valid int32 [B] / [2,B] expected")
    return pts, valid


def emit_frames(imgs, pts, valid, sinks, slots=None, pic_sizes=None, stream=None):
    """Fill `sinks` from imgs uint8 [B,H,W,3]: sink i shows image slots[i] (i by default; sinks may share a slot) with the box of that
    slot's corners drawn on it.  pts int32 [B,8,2] with valid [B] (every sink draws these), or [2,B,8,2] with [2,B] = (raw, smoothed)
    corners, chosen by Sink.pose.  pic_sizes[i] = (h, w) of the picture inside the canvas (the whole image by default).  One pinned upload
    of the descriptor table and one launch on `stream` (the current stream if None); host sinks are rendered into one device staging
    allocation (zeroed: a pitched host sink's row padding receives zeros) and copied out with one non-blocking copy per buffer; device
    sinks are recorded on the stream.  Does not synchronise."""
    sinks = list(sinks)
    n = len(sinks)
    if imgs.dim() != 4 or imgs.shape[3] != 3 or imgs.dtype != torch.uint8:
        raise ValueError("emit_frames: imgs must be a uint8 [B,H,W,3] tensor")
    B, H, W = imgs.shape[:3]
    slots = list(range(n)) if slots is None else [int(s) for s in slots]
    if len(slots) != n or any(not 0 <= s < B for s in slots):
        raise ValueError(f"emit_frames: one slot in [0, {B}) per sink expected")
    sizes = [(H, W)] * n if pic_sizes is None else [(int(h), int(w)) for h, w in pic_sizes]
    if len(sizes) != n or any(not (0 <= h <= H and 0 <= w <= W) for h, w in sizes):
        raise ValueError(f"emit_frames: one picture size (h, w) within {H} x {W} per sink expected")
    pts, valid = _corner_sets("emit_frames", pts, valid, B)
    if any(isinstance(s, Sink) and s.view != "canvas" for s in sinks):
        raise ValueError("emit_frames: a source-view sink shows the camera's frame, not the canvas (emit_source_frames fills it)")
    _fill("emit_frames", sinks, imgs.device, slots, sizes, pts.shape[0], stream, lambda table, n: ops.frame_emit(table, n, imgs, pts, valid))


def emit_source_frames(staged, pts, valid, sinks, sources=None, stream=None):
    """Fill source-view `sinks` from the frames of an `ingest_frames_keep` call: sink i shows frame sources[i] of that call (i by
    default; sinks may share a frame) as the camera delivered it, with the box drawn in its own pixel grid.  pts int32 [B,8,2] with
    valid [B], or [2,B,8,2] with [2,B] = (raw, smoothed), are indexed by the frame's canvas slot and come from `project_corners` under a
    table of `ingest.source_K` rows (B: the canvas count of the ingest call).  One pinned upload of the sink table and one launch of
    g6d_frame_emit_source on `stream` (the current stream if None; launch it on the ingest's stream, or order the two yourself); host
    (pinned) sinks go through device staging as in `emit_frames`.  Frames with a lens are refused.  Does not synchronise."""
    sinks = list(sinks)
    n = len(sinks)
    if not isinstance(staged, I.Staged):
        raise ValueError("emit_source_frames: staged is what ingest.ingest_frames_keep returns beside out")
    sources = list(range(n)) if sources is None else [int(s) for s in sources]
    if len(sources) != n or any(not 0 <= s < staged.n for s in sources):
        raise ValueError(f"emit_source_frames: one frame index in [0, {staged.n}) per sink expected")
    pts, valid = _corner_sets("emit_source_frames", pts, valid, staged.batch)
    if any(not isinstance(s, Sink) or s.view != "source" for s in sinks):
        raise ValueError("emit_source_frames: Sink(view='source') objects expected (emit_frames fills canvas sinks)")
    for i in set(sources):
        if staged.frames[i].lens is not None:
            raise ValueError(f"emit_source_frames: frame {i} has a lens: its source picture is distorted (a straight box edge is a curve "
                             "in it); the source view of lens frames is out of scope, use a canvas sink")
    if n == 0:
        return
    dev = staged.device
    max_w, max_h = max(s.width for s in sinks), max(s.height for s in sinks)

    def launch(table, n):
        if dev.type == "cuda":
            staged.table.record_stream(torch.cuda.current_stream(dev))
        ops.frame_emit_source(table, n, staged.table, staged.n, pts, valid, max_w, max_h)
    _fill("emit_source_frames", sinks, dev, sources, [(0, 0)] * n, pts.shape[0], stream, launch)
