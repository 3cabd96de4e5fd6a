"""g6d_frame_ingest_mesh on the MI355X against the numpy restatement of its integer specification (tests/test_ingest_lens_cpu.py), bit for
bit: every format x rotation x lens model, pitched sources in host and device memory, every mesh step, a canvas with byte-store rows, a
lens that leaves a black border, one launch of plain and lens frames into scattered slots; the tracker on lens frames (graphs and eager
ticks) and that its push does not synchronise."""
import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import tracking as T
from test_ingest_cpu import np_ingest, nv12_of
from test_ingest_gpu import FORMATS, expect_K, run
from test_ingest_lens_cpu import BARREL, FISHEYE, PINCUSHION, camera, lens_frame, np_ingest_lens
from test_track_streams_gpu import _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

MOVES = (lambda a: a, lambda a: torch.from_numpy(a).cuda(), lambda a: torch.from_numpy(a).pin_memory())     # host, device, pinned host


def check(frames, got, Ks, H, W, slots=None):
    for i, f in enumerate(frames):
        s = i if slots is None else slots[i]
        want = (np_ingest_lens if f.lens else np_ingest)(f, H, W)
        np.testing.assert_array_equal(got[s], want, err_msg=f"slot {s}: {f.fmt} {f.width}x{f.height} rotate {f.rotate} {f.lens}")
        np.testing.assert_array_equal(Ks[s], expect_K(f, H, W))


@pytest.mark.parametrize("src_hw,canvas", [((186, 246), (96, 120)), ((120, 160), (120, 160))], ids=["246x186-to-120x96", "160x120-same"])
def test_every_format_rotation_and_model_matches_numpy(src_hw, canvas):
    rng = np.random.RandomState(0)
    (h, w), (H, W) = src_hw, canvas
    frames = [lens_frame(rng, h, w, fmt, lens, rot=rot, extra=(0, 7, 14)[(k + rot // 90) % 3], matrix=("bt601", "bt709")[rot == 180],
                         mv=MOVES[(k + rot // 90) % 3])
              for lens in (BARREL, FISHEYE) for k, fmt in enumerate(FORMATS) for rot in (0, 90, 180, 270)]
    got, Ks = run(frames, H, W)
    check(frames, got, Ks, H, W)
    assert all(g.any() for g in got)


def test_every_mesh_step():
    """tol 1/64, 1/16, 1/4 and 1 canvas pixel make the steps 2, 4, 8 and 16 for these lenses."""
    rng = np.random.RandomState(1)
    h, w, H, W = 186, 246, 96, 120
    frames = [lens_frame(rng, h, w, fmt, lens, rot=rot, extra=5, tol=tol, mv=MOVES[1])
              for tol in (1 / 64, 1 / 16, 1 / 4, 1.0) for lens, fmt, rot in ((BARREL, "nv12", 0), (FISHEYE, "bgr24", 270))]
    steps = [f.lens.mesh(f.K, f.width, f.height, f.rotate, *I.plan(f, (H, W))[1::-1])[1] for f in frames]
    assert steps == [1, 1, 2, 2, 3, 3, 4, 4]
    got, Ks = run(frames, H, W)
    check(frames, got, Ks, H, W)


def test_canvas_with_byte_store_rows():
    rng = np.random.RandomState(2)
    H, W = 97, 123                                       # W % 4 != 0: the tail of every row and the unaligned rows go out as bytes
    frames = [lens_frame(rng, 2 * rng.randint(50, 130), 2 * rng.randint(50, 130), fmt, lens, rot=rot, extra=3, mv=MOVES[k % 3])
              for k, (fmt, lens, rot) in enumerate((("rgb24", BARREL, 0), ("nv12", FISHEYE, 90), ("bgra32", FISHEYE, 180), ("nv12", BARREL, 270),
                                                    ("bgr24", None, 0)))]
    got, Ks = run(frames, H, W, B=6, slots=[5, 1, 0, 3, 2], fill=9)
    check(frames, got, Ks, H, W, slots=[5, 1, 0, 3, 2])
    assert (got[4] == 9).all()


def test_constant_border():
    """brown (0.25, 0.05) at f = 0.52 ws pushes the corners past the source: at least a fifth of the picture is the black border."""
    rng = np.random.RandomState(3)
    h, w, H, W = 186, 246, 96, 128
    frames = [lens_frame(rng, h, w, fmt, PINCUSHION, rot=rot, f=0.52 * w, lo=17, mv=MOVES[k])      # (no source pixel is black itself)
              for k, (fmt, rot) in enumerate((("nv12", 0), ("rgba32", 90)))]
    got, Ks = run(frames, H, W)
    check(frames, got, Ks, H, W)
    for f, g in zip(frames, got):
        out_h, out_w, _ = I.plan(f, (H, W))
        black = (g[:out_h, :out_w] == 0).all(-1).mean()
        assert 0.2 <= black < 0.8, black


def test_16_mixed_frames_into_scattered_slots():
    rng = np.random.RandomState(4)
    H, W, B = 96, 128, 24
    lenses = (None, BARREL, FISHEYE, None, PINCUSHION)
    frames = [lens_frame(rng, 2 * rng.randint(30, 150), 2 * rng.randint(30, 150), FORMATS[k % 5], lenses[(k // 5 + k) % 5], rot=90 * int(rng.randint(0, 4)),
                         extra=int(rng.randint(0, 2)) * 11, matrix=("bt601", "bt709")[k % 2], mv=MOVES[k % 3]) for k in range(16)]
    assert {(f.fmt, f.lens is None) for f in frames} >= {(fmt, plain) for fmt in FORMATS for plain in (True, False)}
    slots = [int(s) for s in rng.permutation(B)[:16]]
    got, Ks = run(frames, H, W, B=B, slots=slots, fill=77)
    check(frames, got, Ks, H, W, slots=slots)
    for s in set(range(B)) - set(slots):
        assert (got[s] == 77).all() and (Ks[s] == -7.0).all(), f"slot {s} was touched"
    plain = [k for k, f in enumerate(frames) if f.lens is None]
    ref, Kr = run([frames[k] for k in plain], H, W)      # without a lens in the call: g6d_frame_ingest
    for i, k in enumerate(plain):
        np.testing.assert_array_equal(got[slots[k]], ref[i])
        np.testing.assert_array_equal(Ks[slots[k]], Kr[i])


# ---------------------------------------------------------------------------------------------------------------- tracker
LENS = I.Lens("brown", (-0.12, 0.03, 0.001, -0.0005, 0.0))
UP = np.array([[2.0, 0, 0.5], [0, 2.0, 0.5], [0, 0, 1]])          # the scene's pixel coordinates -> those of the 2x larger source


def _camera_frame(frame, K, device=False):
    """A scene frame [h,w,3] -> the 2x larger pitched NV12 frame of a camera with LENS (BT.601 limited range, one chroma sample per
    scene pixel)."""
    g = frame.astype(np.int64)
    Y = ((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16
    U = ((-38 * g[..., 0] - 74 * g[..., 1] + 112 * g[..., 2] + 128) >> 8) + 128
    V = ((112 * g[..., 0] - 94 * g[..., 1] - 18 * g[..., 2] + 128) >> 8) + 128
    w = 2 * frame.shape[1]
    buf = nv12_of(np.repeat(np.repeat(Y, 2, 0), 2, 1).astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8), pitch=w + 32)
    return I.Frame(torch.from_numpy(buf).cuda() if device else buf, "nv12", width=w, K=UP @ np.asarray(K, np.float64), lens=LENS)


def _undistorted(f, H, W):
    """The restatement's canvas of a lens frame as a plain canvas-sized frame with the intrinsics the ingest plans for it."""
    return I.Frame(np_ingest_lens(f, H, W), K=I.plan(f, (H, W))[2])


@pytest.mark.parametrize("graphs", [True, False])
def test_tracker_on_lens_frames(scene, graphs):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    S, batch = 4, 2
    seqs = _seqs(frames, S, 3)
    cams = [[_camera_frame(f, Ks[s], device=(s + t) % 2 == 1) for t, f in enumerate(q)] for s, q in enumerate(seqs)]
    flat = [[_undistorted(f, H, W) for f in q] for q in cams]
    assert (flat[0][0].plane0.reshape(H, W, 3) != seqs[0][0]).mean() > 0.2           # the lens moves the picture
    got = T.track_streams(est, cams, batch=batch, lanes=2, graphs=graphs, frame_size=(H, W))
    want = T.track_streams(est, flat, batch=batch, lanes=2, graphs=graphs, frame_size=(H, W))
    for s, ((p, sm), (wp, ws)) in enumerate(zip(got, want)):
        assert np.isfinite(p).all()
        print(f"graphs {graphs} stream {s}: poses differ by at most {np.abs(p - wp).max():.3g}, smoothed by {np.abs(sm - ws).max():.3g}")
    for (p, sm), (wp, ws) in zip(got, want):
        np.testing.assert_array_equal(p, wp)
        np.testing.assert_array_equal(sm, ws)


def test_push_with_lens_frames_does_not_synchronise(scene, monkeypatch):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    seqs = _seqs(frames, 3, 4, seed=1)
    cams = [[_camera_frame(f, Ks[s], device=s == 2) for f in q] for s, q in enumerate(seqs)]
    I._meshes.clear()                                    # the first push builds and uploads the mesh
    counts = {"n": 0}
    at_push = []

    def counted(fn):
        def f(*a, **k):
            counts["n"] += 1
            return fn(*a, **k)
        return f
    monkeypatch.setattr(torch.Tensor, "cpu", counted(torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "item", counted(torch.Tensor.item))
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", counted(torch.cuda.Event.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize))
    push = T.StreamTracker.push
    monkeypatch.setattr(T.StreamTracker, "push", lambda self, *a, **k: (push(self, *a, **k), at_push.append(counts["n"]))[0])
    res = T.track_streams(est, cams, batch=2, lanes=2, frame_size=(H, W))
    assert len(at_push) == 4 and at_push[-1] == 0, at_push
    assert counts["n"] > 0 and all(np.isfinite(p).all() for p, _ in res)
    assert len(I._meshes) == len({q[0].K.tobytes() for q in cams})       # one mesh per camera, built and uploaded inside the first pushes
