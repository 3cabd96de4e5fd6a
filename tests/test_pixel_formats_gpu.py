"""The pixel formats after NV12 and the full-range matrices on the MI355X, bit for bit against the numpy restatement of
tests/test_pixel_formats_cpu.py: the ingest (plain and mesh, mixed launches), g6d_frame_crop, both emit kernels into the four new sink
formats, the pass-through, and the tracker on equivalent frames.  Shapes sit at the kernels' edges: ingest tiles are 128 x 8, emit tiles
128 x 16, crop tiles 64 x 4, with 4 pixels per thread."""
import numpy as np
import pytest
import torch

from gen6d_amd import emit as E
from gen6d_amd import ingest as I
from gen6d_amd import ops
from gen6d_amd import tracking as T
from test_emit_cpu import np_nv12
from test_frame_crop_cpu import homographies, np_crop, warp_rule
from test_ingest_cpu import nv12_of
from test_pixel_formats_cpu import (ALL, NEW, YUV8, assert_padding_untouched, assert_yuv, build_frame, expect_canvas_sink, expect_source_sink,
                                    forward_yuv, frame_yuv, host_record, ingest_cpu, random_frame, sink_yuv, x_frame_ingest,
                                    x_frame_ingest_mesh, x_ingest)
from test_track_streams_gpu import _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

_cuda = lambda a: torch.from_numpy(a).cuda()
MOVE = {"host": lambda a: a, "device": _cuda, "pinned": lambda a: torch.from_numpy(a).pin_memory()}
MATRIX_NAMES = list(I.MATRICES)


def run(frames, H, W, B=None, slots=None, fill=0):
    B = len(frames) if B is None else B
    out = torch.full((B, H, W, 3), fill, dtype=torch.uint8, device="cuda")
    K = torch.full((B, 3, 3), -7.0, device="cuda")
    I.ingest_frames(frames, out, K, slots=slots)
    return out.cpu().numpy(), K.cpu().numpy()


def draw_frame(rng, fmt, rot=0, size=None, mv=None):
    """A noise frame as tests/test_ingest_gpu.py draws them: 2 randint(60, 140) per side (gray8: odd sizes, 4:2:2: an odd height), row
    padding of 7 or 14 bytes, planes on the host, on the device or pinned."""
    h, w = size or (2 * rng.randint(60, 140), 2 * rng.randint(60, 140))
    if size is None and fmt == "gray8":
        h, w = h + 1, w + 1
    if size is None and fmt in I.PACKED_422:
        h += 1
    where = MOVE[("host", "device", "pinned")[rng.randint(0, 3)]]
    return random_frame(rng, fmt, h, w, rotate=rot, extra=7 * int(rng.randint(1, 3)), mv=mv or where, split=bool(rng.randint(0, 2)),
                        matrix=MATRIX_NAMES[rng.randint(0, 4)])


# ---------------------------------------------------------------------------------------------------------------- ingest
@pytest.mark.parametrize("canvas", [(96, 128), (50, 67)])                   # dword stores, byte stores
def test_ingest_every_new_format_and_rotation(canvas):
    rng = np.random.RandomState(0)
    frames = [draw_frame(rng, fmt, rot) for fmt in NEW + ("nv12",) for rot in (0, 90, 180, 270)]
    for f in frames[-4:]:
        f.matrix = ("bt601-full", "bt709-full")[f.rotate in (90, 270)]      # nv12 under the new matrices
    seen = {(f.fmt in NEW or None, f.matrix) for f in frames}
    assert {(True, m) for m in MATRIX_NAMES} <= seen
    got, _ = run(frames, *canvas)
    for i, f in enumerate(frames):
        np.testing.assert_array_equal(got[i], x_ingest(f, *canvas), err_msg=f"{canvas} {f.fmt} {f.matrix} rotate {f.rotate} {f.width}x{f.height}")


def test_ingest_two_to_one_and_same_size():
    """At exactly 2:1 all four taps of a pixel share one chroma sample (4:2:0) or one pair per row (4:2:2); a same-size frame costs one tap."""
    rng = np.random.RandomState(1)
    H, W = 96, 128
    frames = [draw_frame(rng, fmt, size=s) for fmt in NEW + ("nv12",) for s in ((2 * H, 2 * W), (H, W))]
    for f in frames[-2:]:
        f.matrix = "bt709-full"
    got, _ = run(frames, H, W)
    for i, f in enumerate(frames):
        np.testing.assert_array_equal(got[i], x_ingest(f, H, W), err_msg=f"{f.fmt} {f.matrix} {f.width}x{f.height}")


def _on_host(frames, H, W, monkeypatch):
    """The canvases the restatement makes of host frames, through the same Python path on patched ops."""
    with monkeypatch.context() as m:
        m.setattr(ops, "frame_ingest", x_frame_ingest)
        m.setattr(ops, "frame_ingest_mesh", x_frame_ingest_mesh)
        return ingest_cpu(frames, H, W)


def test_mesh_ingest_one_lens_frame_per_new_format(monkeypatch):
    """One launch of g6d_frame_ingest_mesh: a lens frame and a plain frame of every new format."""
    H, W = 96, 128
    lens = I.Lens("brown", (-0.25, 0.08, 0.001, -0.0005))
    twins = []
    for mv in ("host", "device"):                      # the same frames twice: host planes for the restatement, device planes for the kernel
        rng = np.random.RandomState(2)
        frames = []
        for fmt in NEW:
            h, w = 2 * rng.randint(60, 140), 2 * rng.randint(60, 140)
            K = np.array([[0.9 * w, 0, w / 2 - 0.5], [0, 0.9 * w, h / 2 - 0.5], [0, 0, 1]])
            m = MATRIX_NAMES[rng.randint(0, 4)]
            frames += [random_frame(rng, fmt, h, w, extra=6, matrix=m, K=K, lens=lens, mv=MOVE[mv]),
                       random_frame(rng, fmt, h, w, extra=6, matrix=m, rotate=180, mv=MOVE[mv])]
        twins.append(frames)
    want = _on_host(twins[0], H, W, monkeypatch)
    got, _ = run(twins[1], H, W)
    for i, f in enumerate(twins[1]):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"{f.fmt} {f.matrix} {'lens' if f.lens else 'plain'}")
        if f.lens is None:
            np.testing.assert_array_equal(want[i], x_ingest(twins[0][i], H, W))


def test_32_mixed_frames_of_all_eleven_formats_into_scattered_slots():
    rng = np.random.RandomState(3)
    H, W, B = 96, 128, 40
    frames = [draw_frame(rng, ALL[i % 11], 90 * int(rng.randint(0, 4)), size=(2 * rng.randint(20, 160), 2 * rng.randint(20, 160))) for i in range(32)]
    assert {f.fmt for f in frames} == set(ALL)
    slots = [int(s) for s in rng.permutation(B)[:32]]
    got, Ks = run(frames, H, W, B=B, slots=slots, fill=77)
    for f, s in zip(frames, slots):
        np.testing.assert_array_equal(got[s], x_ingest(f, H, W), err_msg=f"slot {s}: {f.fmt} {f.matrix} {f.width}x{f.height} rotate {f.rotate}")
        np.testing.assert_array_equal(Ks[s], np.asarray(I.plan(f, (H, W))[2], np.float64).astype(np.float32))
    for s in set(range(B)) - set(slots):
        assert (got[s] == 77).all() and (Ks[s] == -7.0).all(), f"slot {s} was touched"


# ---------------------------------------------------------------------------------------------------------------- frame_crop
@pytest.mark.parametrize("dh,dw", [(128, 128), (70, 50)])
@pytest.mark.parametrize("rot", [0, 90])
def test_frame_crop_every_new_format(rot, dh, dw):
    """As tests/test_frame_crop_gpu.py compares: the kernel against the float64 restatement under the project's warp rule."""
    rng = np.random.RandomState(10 + rot)
    H, W = (129, 97) if rot == 90 else (97, 129)
    frames = [draw_frame(rng, fmt, rot, mv=_cuda) for fmt in NEW] + [draw_frame(rng, "nv12", rot, mv=_cuda)]
    frames[-1].matrix = "bt601-full"
    B = len(frames)
    imgs = _cuda(rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8))
    staged = I.ingest_frames_keep(frames, imgs, torch.empty((B, 3, 3), device="cuda"))[1]
    hinv = homographies(rng, B, zoom=(1.5, 5.0), shift=(-10, 30))
    rec = list(range(B))
    recs, host = [host_record(f, H, W) for f in frames], imgs.cpu().numpy()
    want = np_crop(recs, rec, host, hinv, dh, dw, np.float64) * 255
    assert 0.02 < (want == 0).all(1).mean() < 0.9
    got = ops.frame_crop(staged.table, _cuda(np.asarray(rec, np.int32)), imgs, _cuda(hinv), dh, dw)
    for b, f in enumerate(frames):
        warp_rule(got[b].cpu().numpy().astype(np.float64) * 255, want[b], f"{f.fmt} {f.matrix} rotate {rot} {dh}x{dw}")


# ---------------------------------------------------------------------------------------------------------------- emit
def make_sink(fmt, w, h, matrix, **kw):
    """A device sink with odd pitches whose planes start 1 byte into their buffers (planar and nv12: two buffers), filled with 7."""
    bpp = I.BPP[fmt]
    z = lambda n: torch.full((1 + n,), 7, dtype=torch.uint8, device="cuda")
    p = w * bpp + 5                                     # (w is even: an odd pitch)
    if fmt in I.PACKED_422:
        buf = z(p * h)
        s = E.Sink(buf[1:], fmt, width=w, height=h, pitch=p, matrix=matrix, **kw)
        s.buffer, s.offset, s.fill = buf, 1, 7
        return s
    crow, crows = (w, h // 2) if fmt == "nv12" else (w // 2, h)
    buf, cbuf = z(p * h), z((crow + 3) * crows)
    s = E.Sink(buf[1:], fmt, width=w, height=h, pitch=p, uv=cbuf[1:], uv_pitch=crow + 3, matrix=matrix, **kw)
    s.buffer, s.offset, s.fill = buf, 1, 7
    return s


SINK_SIZES = [("yuyv422", 130, 18), ("uyvy422", 130, 17), ("i420", 130, 18), ("yv12", 130, 18), ("yuyv422", 256, 32), ("uyvy422", 256, 32),
              ("i420", 256, 32), ("yv12", 256, 32), ("yuyv422", 130, 17), ("nv12", 130, 18)]


def _box(w, h):
    return np.array([[w // 8, h // 4], [w // 8, h - 3], [w - 20, h - 2], [w - 16, 2], [w // 4, h // 3], [w // 4, h - 6], [w - 40, h - 5],
                     [w - 38, 4]], np.int32)


@pytest.mark.parametrize("rng_range", ["limited", "full"])
def test_canvas_emit_into_the_new_sink_formats(rng_range):
    """Sinks that cross a tile edge with a remainder of 2 (130 x 18, 256 x 32; 4:2:2 also at an odd height), larger and smaller than the
    picture, with and without a box."""
    rng = np.random.RandomState(20)
    B, H, W = 2, 40, 280
    canvas = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    matrices = ("bt601", "bt709") if rng_range == "limited" else ("bt601-full", "bt709-full")
    sinks, slots, pics = [], [], []
    for i, (fmt, w, h) in enumerate(SINK_SIZES):
        for pic, box in (((h + 6, w + 10), True), ((h - 5, w - 21), True), ((h, w), False)):
            sinks.append(make_sink(fmt, w, h, matrices[i % 2], box=box, pose="raw"))
            slots.append(i % 2)
            pics.append(pic)
    q = np.stack([_box(130, 18), _box(256, 32)])
    E.emit_frames(_cuda(canvas), _cuda(q), torch.ones(B, dtype=torch.int32, device="cuda"), sinks, slots=slots, pic_sizes=pics)
    torch.cuda.synchronize()
    for s, b, pic in zip(sinks, slots, pics):
        assert_yuv(sink_yuv(s), expect_canvas_sink(canvas[b], q[b], s, pic), f"{s.fmt} {s.matrix} {s.width}x{s.height} picture {pic} box {s.box}")
        assert_padding_untouched(s)


@pytest.mark.parametrize("rng_range", ["limited", "full"])
def test_source_emit_into_the_new_sink_formats(rng_range):
    """Every new sink format from frames of its own format and matrix (the pass-through with a box), of its own format under another
    matrix, and of other formats (through RGB); sinks larger and smaller than the frame."""
    rng = np.random.RandomState(21)
    matrices = ("bt601", "bt709") if rng_range == "limited" else ("bt601-full", "bt709-full")
    frames, sinks, sources = [], [], []
    for i, (fmt, w, h) in enumerate(SINK_SIZES):
        m = matrices[i % 2]
        other = MATRIX_NAMES[(I.MATRICES[m] + 1 + i % 3) % 4]
        hh = h + (h % 2 if fmt not in I.PACKED_422 else 0)
        for sfmt, sm, (dw, dh) in ((fmt, m, (0, 0)), (fmt, m, (12, 6)), (fmt, m, (-22, -6)), (fmt, other, (0, 0)), ("bgr24", m, (0, 0)),
                                   ("p010", other, (-22, -6)), ("gray8", m, (12, 6)), (("nv12", "i420", "uyvy422")[i % 3], m, (0, 0))):
            fh, fw = hh + dh + (0 if sfmt in I.PACKED_422 + ("gray8", "bgr24") else (hh + dh) % 2), w + dw
            frames.append(random_frame(rng, sfmt, fh, fw, matrix=sm, extra=3, offset=1, mv=_cuda))
            sinks.append(make_sink(fmt, w, h, m, view="source", box=len(frames) % 4 != 0))
            sources.append(len(frames) - 1)
    B = len(frames)
    out = torch.zeros((B, 8, 8, 3), dtype=torch.uint8, device="cuda")
    staged = I.ingest_frames_keep(frames, out, torch.zeros((B, 3, 3), device="cuda"))[1]
    q = np.stack([_box(s.width, s.height) for s in sinks])
    E.emit_source_frames(staged, _cuda(q), torch.ones(B, dtype=torch.int32, device="cuda"), sinks, sources=sources)
    torch.cuda.synchronize()
    passes = 0
    for s, f, qq in zip(sinks, frames, q):
        passes += f.fmt == s.fmt and f.matrix == s.matrix and s.box
        assert_yuv(sink_yuv(s), expect_source_sink(f, qq, s), f"{f.fmt} {f.matrix} {f.width}x{f.height} -> {s.fmt} {s.matrix} {s.width}x{s.height} box {s.box}")
        assert_padding_untouched(s)
    assert passes >= 15


def test_new_frames_into_the_first_five_sink_formats():
    """The read half alone: frames of the new formats into rgb24 / bgra32 / nv12 sinks equal the canvas emit of their same-size ingest."""
    rng = np.random.RandomState(22)
    w, h = 130, 18
    frames = [random_frame(rng, fmt, h, w, matrix=MATRIX_NAMES[i % 4], extra=3, offset=1, mv=_cuda) for i, fmt in enumerate(NEW + ("nv12",))]
    frames[-1].matrix = "bt709-full"
    B = len(frames)
    canvas = torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda")
    staged = I.ingest_frames_keep(frames, canvas, torch.zeros((B, 3, 3), device="cuda"))[1]
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    q = _cuda(np.stack([_box(w, h)] * B))
    valid = torch.ones(B, dtype=torch.int32, device="cuda")
    for fmt, shape in (("rgb24", (h, w, 3)), ("bgra32", (h, w, 4)), ("nv12", (h * 3 // 2, w))):
        a, b = [E.Sink(z(*shape), fmt, view="source") for _ in range(B)], [E.Sink(z(*shape), fmt) for _ in range(B)]
        E.emit_source_frames(staged, q, valid, a)
        E.emit_frames(canvas, q, valid, b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x.plane0, y.plane0) and (x.plane1 is None or torch.equal(x.plane1, y.plane1)), f"{frames[i].fmt} -> {fmt}"
            np.testing.assert_array_equal(canvas[i].cpu().numpy(), x_ingest(frames[i], h, w))


def test_pass_through_is_a_byte_copy_on_the_device():
    """The five formats, without a box: the sink's samples are the frame's, with odd pitches and unaligned bases on both sides."""
    rng = np.random.RandomState(23)
    frames, sinks = [], []
    for i, fmt in enumerate(YUV8):
        for w, h in ((130, 18), (256, 32)):
            m = MATRIX_NAMES[(i + w) % 4 if fmt != "nv12" else 2 + i % 2]
            hh = h + 1 if fmt in I.PACKED_422 else h
            frames.append(random_frame(rng, fmt, hh, w, matrix=m, extra=3, offset=1 + i, split=fmt not in I.PACKED_422, mv=_cuda))
            sinks.append(make_sink(fmt, w, hh, m, view="source", box=False))
    B = len(frames)
    staged = I.ingest_frames_keep(frames, torch.zeros((B, 8, 8, 3), dtype=torch.uint8, device="cuda"), torch.zeros((B, 3, 3), device="cuda"))[1]
    E.emit_source_frames(staged, torch.zeros((B, 8, 2), dtype=torch.int32, device="cuda"), torch.ones(B, dtype=torch.int32, device="cuda"), sinks)
    torch.cuda.synchronize()
    for f, s in zip(frames, sinks):
        p1 = None if f.plane1 is None else f.plane1.cpu().numpy()
        raw = frame_yuv(f.plane0.cpu().numpy(), p1, f.pitch, f.uv_pitch, f.width, f.height, I.FORMATS[f.fmt])
        assert_yuv(sink_yuv(s), raw, f"{f.fmt} {f.matrix} {f.width}x{f.height}")
        assert_padding_untouched(s)


# ---------------------------------------------------------------------------------------------------------------- tracker
def _camera(frame, fmt):
    """A scene frame [h,w,3] -> a 2x larger camera frame of the same BT.601 samples in `fmt`: one chroma sample per original pixel, i.e.
    per 2 x 2 block (4:2:2: the same sample in both rows of the block)."""
    Y, UV = np_nv12(np.repeat(np.repeat(frame, 2, 0), 2, 1), 0)
    U, V = UV[:, 0::2], UV[:, 1::2]
    if fmt in I.PACKED_422:
        U, V = np.repeat(U, 2, 0), np.repeat(V, 2, 0)
    return build_frame(fmt, Y, U, V, extra=4)


@pytest.mark.parametrize("a,b", [("i420", "nv12"), ("yuyv422", "uyvy422")])
def test_tracker_equivalent_frames_give_equal_poses(scene, a, b):
    """graphs=True, crops="source": streams fed frames of one format give torch.equal poses to the same streams fed the other format of
    the same samples (the canvases and the crops are bit-equal, so everything after them is)."""
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    assert (H, W) == (96, 128)
    seqs = _seqs(frames, 4, 3)
    res = []
    for fmt in (a, b):
        native = [[_camera(f, fmt) for f in q] for q in seqs]
        res.append(T.track_streams(est, native, batch=2, lanes=2, graphs=True, frame_size=(H, W), crops="source"))
    for (pa, sa), (pb, sb) in zip(*res):
        assert np.isfinite(pa).all() and len(pa) >= 2
        assert torch.equal(torch.as_tensor(pa), torch.as_tensor(pb)) and torch.equal(torch.as_tensor(sa), torch.as_tensor(sb))
    img = {}
    for fmt in (a, b):                                 # ... and the canvases are: one ingest of the first stream's last frame
        img[fmt] = run([_camera(seqs[0][-1], fmt)], H, W)[0]
    np.testing.assert_array_equal(img[a], img[b])
