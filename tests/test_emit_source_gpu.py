"""g6d_frame_emit_source on the MI355X against the numpy restatement of its specification (tests/test_emit_source_cpu.py), bit for bit:
every source format into every sink format with both matrices on each side, pitched and byte-offset planes, sinks larger and smaller
than the source, tile edges and the corner range's ends, 32 sinks from 16 frames in one launch with host and device sinks mixed, a
full-HD NV12 pass-through, and the tracker with canvas and source sinks mixed, with graphs and eager ticks."""
import numpy as np
import pytest
import torch

from gen6d_amd import emit as E
from gen6d_amd import ingest as I
from gen6d_amd import ops
from gen6d_amd import tracking as T
from test_emit_cpu import BOX, assert_sink, sink_content, visible_object_pts
from test_emit_gpu import make_sink
from test_emit_source_cpu import FMT_NAMES, SRC_BOX, camera_frame, emit_sources, make_frame, np_emit_source, own_K
from test_track_streams_gpu import scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

KINDS = [(f, "bt601") for f in FMT_NAMES] + [("nv12", "bt709")]           # (format, matrix) of a source or a sink


def source_sink(rng, fmt, w, h, **kw):
    return make_sink(rng, fmt, w, h, view="source", **kw)


def test_every_source_format_into_every_sink_format():
    rng = np.random.RandomState(0)
    frames = [make_frame(rng, fmt, *((72, 46) if fmt == "nv12" else (70, 46)), matrix=m, extra=(0 if fmt == "nv12" else 5),
                         offset=(0 if fmt == "nv12" else 1), where=("host", "cuda")[i % 2]) for i, (fmt, m) in enumerate(KINDS)]
    frames.append(make_frame(rng, "nv12", 72, 46, extra=3, offset=1, where="cuda"))             # NV12 on the byte paths too
    sinks, sources = [], []
    for fi, f in enumerate(frames):
        for ki, (fmt, m) in enumerate(KINDS):
            for v, (dw, dh) in enumerate(((0, 0), (8, 8), (-10, -10))):
                sinks.append(source_sink(rng, fmt, f.width + dw, f.height + dh, matrix=m, extra=(0, 13, 3)[v], offset=(0, 5, 2)[(v + ki) % 3],
                                         pose=("raw", "smooth")[(fi + ki + v) % 2], box=(fi + ki + v) % 7 != 0))
                sources.append(fi)
    pts = np.stack([np.tile(SRC_BOX, (len(frames), 1, 1)), np.tile(SRC_BOX[::-1] + [3, -2], (len(frames), 1, 1))])
    emit_sources(frames, pts, np.ones((2, len(frames)), np.int32), sinks, sources=sources, device="cuda")
    torch.cuda.synchronize()
    for s, fi in zip(sinks, sources):
        f = frames[fi]
        assert_sink(s, np_emit_source(f, pts[E.POSES[s.pose], fi], s), f"{f.fmt}/{f.matrix} -> {s.fmt}/{s.matrix} {s.width}x{s.height} box {s.box}")


def test_tile_edges_and_the_corner_range():
    rng = np.random.RandomState(1)
    frames = [make_frame(rng, "nv12", 130, 18, where="cuda"), make_frame(rng, "rgb24", 130, 18, where="host"),
              make_frame(rng, "nv12", 8192, 16, matrix="bt709", where="cuda"), make_frame(rng, "bgra32", 8192, 16, where="cuda")]
    far = np.array([[-8192, -8192], [16383, -8192], [16383, 16383], [-8192, 16383], [-8192, 3], [16383, 5], [16383, 12], [-8192, 9]], np.int32)
    near = BOX * [3, 1] // [1, 3] + [-20, 2]                             # crosses x = 128 and y = 16
    pts = np.stack([near, near, far, far])
    sinks, sources = [], []
    for fi, f in enumerate(frames):
        for fmt, m in (("nv12", f.matrix), ("nv12", "bt601" if f.matrix == "bt709" else "bt709"), ("rgb24", "bt601")):
            sinks.append(source_sink(rng, fmt, f.width, f.height, matrix=m, thickness=3))
            sources.append(fi)
    emit_sources(frames, pts, np.ones(4, np.int32), sinks, sources=sources, device="cuda")
    torch.cuda.synchronize()
    for s, fi in zip(sinks, sources):
        assert_sink(s, np_emit_source(frames[fi], pts[fi], s), f"frame {fi} {frames[fi].fmt} -> {s.fmt}/{s.matrix}")
    # beyond the range nothing is drawn: the pass-through is the byte copy
    out = far.copy()
    out[2] = (16384, 16383)
    s = source_sink(rng, "nv12", 8192, 16, matrix="bt709")
    emit_sources(frames[2:3], out[None], [1], [s], device="cuda")
    torch.cuda.synchronize()
    assert_sink(s, np_emit_source(frames[2], None, s))
    f = frames[2]
    np.testing.assert_array_equal(sink_content(s)[0], f.plane0.cpu().numpy()[:16 * 8192].reshape(16, 8192))


def test_32_sinks_from_16_frames_in_one_launch():
    rng = np.random.RandomState(2)
    B, nf = 40, 16
    frames = []
    for i in range(nf):
        fmt = FMT_NAMES[rng.randint(0, 5)]
        w, h = int(rng.randint(20, 201)) & ~1, int(rng.randint(20, 121)) & ~1
        frames.append(make_frame(rng, fmt, w, h, matrix=("bt601", "bt709")[rng.randint(0, 2)], extra=int(rng.randint(0, 2)) * 7,
                                 offset=int(rng.randint(0, 2)), where=("host", "cuda")[rng.randint(0, 2)]))
    slots = [int(s) for s in rng.permutation(B)[:nf]]
    pts, valid = np.zeros((2, B, 8, 2), np.int32), np.zeros((2, B), np.int32)
    for i, f in enumerate(frames):
        for k in range(2):
            pts[k, slots[i]] = np.stack([rng.randint(-20, f.width + 20, 8), rng.randint(-20, f.height + 20, 8)], -1)
            valid[k, slots[i]] = 0 if i in (3, 11) else 1
    sinks, sources = [], []
    for i, f in enumerate(frames):
        for pose in ("raw", "smooth"):
            fmt = FMT_NAMES[rng.randint(0, 5)]
            dw, dh = (int(rng.randint(-4, 5)) * 2 for _ in range(2))
            sinks.append(source_sink(rng, fmt, f.width + dw, f.height + dh, matrix=("bt601", "bt709")[rng.randint(0, 2)], pose=pose,
                                     extra=int(rng.randint(0, 2)) * 11, where=("device", "pinned")[rng.randint(0, 2)]))
            sources.append(i)
    # sink 5 names a frame index outside [0, nf): it is skipped.  emit_source_frames refuses such an index, so the launch goes through
    # the module's shared table builder with the same arguments emit_source_frames passes
    sinks[5] = source_sink(rng, "rgb24", 64, 32)
    sources[5] = nf
    out = torch.zeros((B, 8, 8, 3), dtype=torch.uint8, device="cuda")
    _, staged = I.ingest_frames_keep(frames, out, torch.zeros((B, 3, 3), device="cuda"), slots=slots)
    d = lambda a: torch.from_numpy(a).cuda()
    dp, dv = d(pts), d(valid)
    launches = []
    E._fill("test", sinks, out.device, sources, [(0, 0)] * 32, 2, None,
            lambda table, n: (launches.append(n), ops.frame_emit_source(table, n, staged.table, nf, dp, dv, 208, 128)))
    torch.cuda.synchronize()
    assert launches == [32]
    for j, (s, i) in enumerate(zip(sinks, sources)):
        if j == 5:
            assert (sink_content(s) == 7).all()
            continue
        k = E.POSES[s.pose]
        q = pts[k, slots[i]] if valid[k, slots[i]] else None
        assert_sink(s, np_emit_source(frames[i], q, s), f"sink {j} frame {i} {frames[i].fmt} -> {s.fmt} {s.pose}")


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_full_hd_nv12(matrix):
    """One 1080 x 1920 NV12 frame (BT.601) into an NV12 sink of the same matrix (the pass-through) and of the other one (the conversion)."""
    rng = np.random.RandomState(3)
    frame = make_frame(rng, "nv12", 1920, 1080, where="cuda")
    q = BOX * 18 + [400, 60]                                             # x 580 .. 1336, y 168 .. 852: dozens of tiles
    sink = source_sink(rng, "nv12", 1920, 1080, matrix=matrix, extra=64)
    emit_sources([frame], q[None], [1], [sink], device="cuda")
    torch.cuda.synchronize()
    assert_sink(sink, np_emit_source(frame, q, sink), matrix)


@pytest.fixture(scope="module")
def object_pts(scene):
    """Object points whose box is in view under the first stream's first pose, computed once for the module."""
    db, est, frames, Ks = scene
    f = camera_frame(frames[0])
    probe = T.StreamTracker(est, 1, batch=1, graphs=False, frame_size=(120, 160))
    probe.push([0], [f])
    return visible_object_pts(probe.result()[0][0], I.plan(f, (120, 160))[2], 120, 160)


@pytest.mark.parametrize("graphs", [True, False])
def test_tracker_mixes_canvas_and_source_sinks(scene, object_pts, graphs):
    db, est, frames, Ks = scene
    hw, S = (120, 160), 4
    make = lambda: T.StreamTracker(est, S, batch=2, lanes=2, graphs=graphs, frame_size=hw, object_pts=object_pts)
    plain, tr = make(), make()
    z = lambda *s: torch.full(s, 7, dtype=torch.uint8, device="cuda")
    src = lambda t: [camera_frame(frames[t % len(frames)], where="cuda"), camera_frame(frames[(t + 1) % len(frames)], rotate=90),
                     camera_frame(frames[(t + 2) % len(frames)], K=own_K(Ks[(t + 2) % len(frames)]), where="cuda"), camera_frame(frames[(t + 3) % len(frames)])]
    canvas_sinks = lambda: [E.Sink(z(180, 160), "nv12", pose="raw"), E.Sink(z(120, 160, 3), "rgb24"), E.Sink(z(180, 160), "nv12"),
                            E.Sink(z(120, 160, 4), "bgra32")]
    drawn = 0
    for t in range(3):                                                   # an init push, then two ticks
        fr = src(t)
        alone, mixed = canvas_sinks(), canvas_sinks()
        plain.push(range(S), fr, sinks=alone)
        source = [[E.Sink(z(360, 320), "nv12", view="source"), E.Sink(z(240, 320, 3), "rgb24", view="source", pose="raw")],
                  [E.Sink(z(480 + 12, 248), "nv12", view="source", matrix="bt709")],
                  [E.Sink(z(345, 310), "nv12", view="source", thickness=5, dot_radius=6)],
                  [E.Sink(torch.full((360, 320), 7, dtype=torch.uint8).pin_memory(), "nv12", view="source", pose="raw")]]
        tr.push(range(S), fr, sinks=[[c] + s for c, s in zip(mixed, source)])
        tr.wait_emitted()
        rp, rs = plain.result(), tr.result()
        corners = {}
        Kd = torch.from_numpy(np.stack([I.source_K(f, hw).astype(np.float32) for f in fr])).cuda()
        for name, table in (("raw", tr.pose_table), ("smooth", tr.smooth_table)):
            q, ok = E.project_corners(table, Kd, torch.arange(S, dtype=torch.int32, device="cuda"), tr.box)
            corners[name] = (q.cpu().numpy(), ok.cpu().numpy())
        for s in range(S):
            np.testing.assert_array_equal(rs[s][0], rp[s][0])            # source sinks change no pose
            assert_sink(mixed[s], sink_content(alone[s]), f"canvas sink of stream {s}, push {t}")
            for k in source[s]:
                q, ok = corners[k.pose]
                drawn += int(ok[s])
                assert_sink(k, np_emit_source(fr[s], q[s] if ok[s] else None, k), f"push {t} stream {s} {k.fmt} {k.pose}")
    assert drawn >= 6
