"""The tracker with crops="source" on the MI355X (gen6d_amd/tracking.py; the kernel itself: tests/test_frame_crop_gpu.py),
on 2x camera-native NV12 / BGRA frames of the scene of tests/test_track_streams_gpu.py: graphs against eager ticks, every tracked frame
against one eager `query_batch_source` step with the same source, same-size frames against the canvas mode, a lane shared by two
groups, and that its push does not synchronise."""
import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import tracking as T
from test_frame_crop_cpu import native2x
from test_track_streams_gpu import _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

_cuda = lambda a: torch.from_numpy(a).cuda()


def _natives(frames, S, seed=0):
    seqs = _seqs(frames, S, 4, seed=seed)
    return seqs, [[native2x(f, ("nv12", "bgra")[(s + t) % 2]) for t, f in enumerate(q)] for s, q in enumerate(seqs)]


def _run(est, native, S, **kw):
    tr = T.StreamTracker(est, S, batch=2, lanes=2, crops="source", **kw)
    tr._records = []
    for t in range(max(len(q) for q in native)):
        ids = [s for s in range(S) if t < len(native[s])]
        tr.push(ids, [native[s][t] for s in ids])
    res = tr._collect([len(q) for q in native])
    tr._check_range()
    return res


def _check_source_steps(est, native, res, H, W, bar=3e-4):
    """Every tracked frame is one eager query_batch step from the previous pose, cutting from the same source."""
    chain = est.device_chain()
    for s, (poses, smooth) in enumerate(res):
        assert np.isfinite(poses).all() and np.isfinite(smooth).all()
        for t in range(1, len(poses)):
            img, K = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda"), torch.empty((1, 3, 3), device="cuda")
            staged = I.ingest_frames_keep([native[s][t]], img, K)[1]
            one = chain.query_batch_source(img, K, I.SourceTable.of(staged), pose_init=_cuda(poses[t - 1])[None], refine_iter=1)
            np.testing.assert_allclose(poses[t], one["pose"][0].cpu().numpy(), atol=bar, err_msg=f"stream {s} frame {t}")


def test_tracker_graphs_match_eager_and_per_stream_steps(scene):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    _, native = _natives(frames, 4)
    g = _run(est, native, 4, frame_size=(H, W), graphs=True)
    e = T.track_streams(est, native, batch=2, lanes=2, graphs=False, frame_size=(H, W), crops="source")
    for (pg, sg), (pe, se) in zip(g, e):
        np.testing.assert_allclose(pg, pe, atol=3e-4)
        np.testing.assert_allclose(sg, se, atol=3e-4)
    _check_source_steps(est, native, g, H, W)


def test_tracker_two_groups_share_a_lane(scene):
    """S = 6 at batch 2 on two lanes: groups 0 and 2 take turns on lane 0's static frame table and slot map."""
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    _, native = _natives(frames, 6, seed=2)
    _check_source_steps(est, native, _run(est, native, 6, frame_size=(H, W), graphs=True), H, W)


def test_tracker_same_size_frames_match_canvas_mode(scene):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    seqs = _seqs(frames, 4, 4)
    native = [[I.Frame(f) for f in q] for q in seqs]
    source = T.track_streams(est, native, batch=2, lanes=2, frame_size=(H, W), crops="source")
    canvas = T.track_streams(est, native, batch=2, lanes=2, frame_size=(H, W))
    for (ps, ss), (pc, sc) in zip(source, canvas):
        np.testing.assert_allclose(ps, pc, atol=3e-4)
        np.testing.assert_allclose(ss, sc, atol=3e-4)


def test_push_with_source_crops_does_not_synchronise(scene, monkeypatch):
    """test_ingest_gpu.test_push_with_frame_size_does_not_synchronise in "source" mode."""
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    seqs, native = _natives(frames, 3, seed=1)
    native[2] = [I.Frame(torch.from_numpy(np.ascontiguousarray(f)).cuda()) for f in seqs[2]]          # a device-resident stream
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
    push = T.StreamTracker.push
    monkeypatch.setattr(T.StreamTracker, "push", lambda self, *a, **k: (push(self, *a, **k), at_push.append(counts["n"]))[0])
    res = T.track_streams(est, native, batch=2, lanes=2, frame_size=(H, W), crops="source")
    assert len(at_push) == 4 and at_push[-1] == 0, at_push
    assert counts["n"] > 0 and all(np.isfinite(p).all() for p, _ in res)
