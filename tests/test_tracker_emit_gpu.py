"""StreamTracker.push with sinks on the MI355X: camera-native frames into NV12 device sinks with graphs and eager ticks, bit for bit the
numpy restatement (tests/test_emit_cpu.py) of the numpy ingest's canvas with the corners read back from the device; emitting changes no
pose; a push with sinks does not synchronise and host sinks are valid after wait_emitted alone."""
import numpy as np
import pytest
import torch

from gen6d_amd import emit as E
from gen6d_amd import eval as EV
from gen6d_amd import tracking as T
from test_emit_cpu import assert_sink, np_emit, visible_object_pts
from test_ingest_cpu import np_ingest
from test_ingest_gpu import _native
from test_track_streams_gpu import _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def object_pts(scene):
    """Object points whose box is in view under the scene's first pose, computed once for the module's tracker tests."""
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    probe = T.StreamTracker(est, 1, batch=1, graphs=False)
    probe.push([0], [frames[0]])
    return visible_object_pts(probe.result()[0][0], EV.pseudo_K(H, W), H, W)


def _tracker(est, pts, graphs, S, batch, H, W):
    return lambda: T.StreamTracker(est, S, batch=batch, lanes=2, graphs=graphs, frame_size=(H, W), object_pts=pts)


@pytest.mark.parametrize("graphs", [True, False])
def test_tracker_emits_native_frames_into_nv12_sinks(scene, object_pts, graphs):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    S, batch = 4, 2
    K = EV.pseudo_K(H, W)
    seqs = _seqs(frames, S, 4)
    native = [[_native(f, ("nv12", "bgra")[(s + t) % 2]) for t, f in enumerate(q)] for s, q in enumerate(seqs)]
    make = _tracker(est, object_pts, graphs, S, batch, H, W)
    plain, tr = make(), make()
    Kd = torch.from_numpy(np.repeat(K[None], S, 0)).cuda()
    ident = torch.arange(S, dtype=torch.int32, device="cuda")
    drawn = 0
    for t in range(4):
        ids = [s for s in range(S) if t < len(seqs[s])]
        plain.push(ids, [native[s][t] for s in ids])
        sinks = [[E.Sink(torch.full((H * 3 // 2, W), 7, dtype=torch.uint8, device="cuda"), "nv12", pose="raw"),
                  E.Sink(torch.full((H * 3 // 2 + 3, W + 32), 7, dtype=torch.uint8, device="cuda")[:H * 3 // 2], "nv12", width=W, matrix="bt709")]
                 for _ in ids]
        tr.push(ids, [native[s][t] for s in ids], sinks=sinks)
        tr.wait_emitted()
        rp, rs = plain.result(), tr.result()
        for s in ids:                                    # emitting changes no pose
            np.testing.assert_array_equal(rs[s][0], rp[s][0], err_msg=f"stream {s} frame {t}")
            np.testing.assert_array_equal(rs[s][1], rp[s][1], err_msg=f"stream {s} frame {t} (smoothed)")
        corners = {}
        for name, table in (("raw", tr.pose_table), ("smooth", tr.smooth_table)):
            q, ok = E.project_corners(table, Kd, ident, tr.box)
            corners[name] = (q.cpu().numpy(), ok.cpu().numpy())
        for s, pair in zip(ids, sinks):
            canvas = np_ingest(native[s][t], H, W)
            for k in pair:
                q, ok = corners[k.pose]
                drawn += int(ok[s])
                assert_sink(k, np_emit(canvas, q[s] if ok[s] else None, k), f"stream {s} frame {t} {k.pose}")
    assert drawn > 0                                     # the boxes were in view: the comparison covered drawn pictures


def test_push_with_sinks_does_not_synchronise(scene, object_pts, monkeypatch):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    S = 3
    K = EV.pseudo_K(H, W)
    seqs = _seqs(frames, S, 4, seed=1)
    native = [[_native(f, ("nv12", "bgra")[(s + t) % 2]) for t, f in enumerate(q)] for s, q in enumerate(seqs)]
    tr = _tracker(est, object_pts, True, S, 2, H, W)()
    host = [[E.Sink(torch.full((H * 3 // 2, W), 7, dtype=torch.uint8).pin_memory(), "nv12"),
             E.Sink(torch.full((H, W, 4), 7, dtype=torch.uint8).pin_memory(), "bgra32", pose="raw")] for _ in range(S)]
    counts = {"n": 0}

    def counted(fn):
        def f(*a, **k):
            counts["n"] += 1
            return fn(*a, **k)
        return f
    monkeypatch.setattr(torch.Tensor, "cpu", counted(torch.Tensor.cpu))
    monkeypatch.setattr(torch.Tensor, "item", counted(torch.Tensor.item))
    monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize))
    T_ = min(len(q) for q in seqs)
    for t in range(T_):
        tr.push(list(range(S)), [native[s][t] for s in range(S)], sinks=host)
    assert counts["n"] == 0
    tr.wait_emitted([0, 1, 2])
    assert counts["n"] == 0                              # events of the lanes involved, no device-wide synchronise
    monkeypatch.undo()
    for pair in host:                                    # what the sinks hold right after wait_emitted, before anything else can wait
        for k in pair:
            k.plane0 = k.plane0.clone()
            k.plane1 = None if k.plane1 is None else k.plane1.clone()
    Kd = torch.from_numpy(np.repeat(K[None], S, 0)).cuda()
    ident = torch.arange(S, dtype=torch.int32, device="cuda")
    for s in range(S):
        canvas = np_ingest(native[s][T_ - 1], H, W)
        for k in host[s]:
            q, ok = E.project_corners(tr.pose_table if k.pose == "raw" else tr.smooth_table, Kd, ident, tr.box)
            q, ok = q.cpu().numpy(), ok.cpu().numpy()
            assert_sink(k, np_emit(canvas, q[s] if ok[s] else None, k), f"host sink of stream {s}, {k.pose}")
    tr.result()
