"""gen6d_amd.tracking on the CPU: the eager tracker (graphs=False) with the chain ops replaced by tests/ref_ops.py and the two tracking
ops by the numpy versions below (the host algebra of gen6d_amd/geometry.py on the tables' memory).  Checks the schedule of
predict.py:56-59, that every frame equals one step of DeviceChain.query from the tracker's previous pose, the smoothing, different
stream lengths, subset pushes, reset and the argument errors."""
import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import eval as EV
from gen6d_amd import geometry as G
from gen6d_amd import ops
from gen6d_amd import tracking as T


def np_track_gather(pose_table, slot_stream, parking_pose):
    P, park = pose_table.numpy(), parking_pose.reshape(12).numpy()
    return torch.from_numpy(np.stack([park if s < 0 else P[s] for s in slot_stream.tolist()]).reshape(-1, 3, 4).astype(np.float32))


def np_track_commit(pose, K, slot_stream, reset, box, num, std, pose_table, hist, hist_count, smooth_table, out=None):
    B = slot_stream.shape[0]
    out = torch.zeros((B, 2, 3, 4), dtype=torch.float32) if out is None else out
    P, Ks, bx = pose.reshape(B, 3, 4).numpy().astype(np.float64), K.reshape(B, 3, 3).numpy().astype(np.float64), box.numpy().astype(np.float64)
    H, C = hist.numpy(), hist_count.numpy()
    for b, s in enumerate(slot_stream.tolist()):
        if s < 0:
            continue
        n0 = 0 if reset else int(C[s])
        new = n0 % num
        H[s, new] = G.project_points(bx, P[b], Ks[b])[0]
        C[s] = n0 + 1
        n = min(n0 + 1, num)
        sm = G.pnp(bx, G.weighted_points([H[s, (new - i) % num] for i in reversed(range(n))], num, std), Ks[b], P[b])
        pose_table[s] = torch.from_numpy(P[b].reshape(12).astype(np.float32))
        smooth_table[s] = torch.from_numpy(sm.reshape(12).astype(np.float32))
        out[b, 0] = torch.from_numpy(P[b].astype(np.float32))
        out[b, 1] = torch.from_numpy(sm.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def scene():
    from gen6d_amd.synth_db import SyntheticDatabase
    from test_estimator_cpu import make_estimator
    mp = pytest.MonkeyPatch()
    ref_ops.patch_ops(mp)
    db = SyntheticDatabase(n_views=24, size=(96, 128), focal=140.0)
    est = make_estimator(refine_iter=2, damped=True)
    est.build(db, "all")
    _, que_ids = db.get_split("all")
    frames = [db.get_image(i) for i in que_ids[:4]]
    Ks = [db.get_K(i) for i in que_ids[:4]]
    mp.undo()
    return est, frames, Ks


@pytest.fixture
def patched(monkeypatch):
    ref_ops.patch_ops(monkeypatch)
    monkeypatch.setattr(ops, "track_gather", np_track_gather)
    monkeypatch.setattr(ops, "track_commit", np_track_commit)


def _it(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _smoothed(box, poses, Ks, num=5, std=2.5):
    """predict.py:62-66 on the host over the whole history (not a ring)."""
    hist, out = [], []
    for p, K in zip(poses, Ks):
        p, K = np.asarray(p, np.float64), np.asarray(K, np.float64)
        hist.append(G.project_points(box, p, K)[0])
        out.append(G.pnp(box, G.weighted_points(hist, num, std), K, p))
    return np.asarray(out)


def test_schedule_and_one_step_per_frame(scene, patched, monkeypatch):
    est, frames, Ks = scene
    calls = []
    orig = est.refiner._step
    monkeypatch.setattr(est.refiner, "_step", lambda *a, **k: (calls.append(a[0].shape[0]), orig(*a, **k))[1])
    seq = [frames[1], frames[1], frames[2]]
    (poses, smooth), = T.track_streams(est, [seq], [Ks[1]], batch=2, graphs=False)
    # 2 steps on the first frame (query_batch of the one new stream), then 1 per frame on the group's batch of 2 slots
    assert calls == [1, 1, 2, 2]
    assert poses.shape == (3, 3, 4) and smooth.shape == (3, 3, 4) and np.isfinite(poses).all() and np.isfinite(smooth).all()
    chain = est.device_chain()
    first = chain.query(_it(seq[0]), _it(Ks[1]))["pose"].numpy()
    np.testing.assert_allclose(poses[0], first, atol=2e-4)
    for t in (1, 2):
        one = chain.query(_it(seq[t]), _it(Ks[1]), pose_init=_it(poses[t - 1]), refine_iter=1)["pose"].numpy()
        np.testing.assert_allclose(poses[t], one, atol=2e-4)
    np.testing.assert_allclose(smooth[0], poses[0], atol=1e-5)               # one frame: the PnP of its own corners
    box = G.box_corners(EV.get_ref_point_cloud(est.refiner.ref_database))
    np.testing.assert_allclose(smooth, _smoothed(box, poses, [Ks[1]] * 3), atol=1e-5)


def test_lengths_subsets_and_reset(scene, patched):
    est, frames, Ks = scene
    chain = est.device_chain()
    seqs = [[frames[0], frames[1], frames[2], frames[3]], [frames[2]], [frames[3], frames[1]]]
    res = T.track_streams(est, seqs, [Ks[0], None, np.stack([Ks[3], Ks[1]])], batch=2, lanes=2, graphs=False)
    assert [r[0].shape[0] for r in res] == [4, 1, 2]
    h, w = frames[0].shape[:2]
    Kseq = [[Ks[0]] * 4, [EV.pseudo_K(h, w)], [Ks[3], Ks[1]]]
    # first frames: streams 0 and 1 (group 0) share one query_batch, stream 2 has its own
    firsts = chain.query_batch(torch.stack([_it(seqs[0][0]), _it(seqs[1][0])]), torch.stack([_it(Kseq[0][0]), _it(Kseq[1][0])]))["pose"]
    firsts = list(firsts.numpy()) + [chain.query(_it(seqs[2][0]), _it(Kseq[2][0]))["pose"].numpy()]
    for s, (poses, smooth) in enumerate(res):
        np.testing.assert_allclose(poses[0], firsts[s], atol=2e-4)
        np.testing.assert_allclose(smooth[0], poses[0], atol=1e-5)
        for t in range(1, len(poses)):
            one = chain.query(_it(seqs[s][t]), _it(Kseq[s][t]), pose_init=_it(poses[t - 1]), refine_iter=1)["pose"].numpy()
            np.testing.assert_allclose(poses[t], one, atol=2e-4)
    # subset pushes and a reset mid-run on a tracker: streams 0 and 3 share group 0 / 1 with unused slots
    tr = T.StreamTracker(est, 4, batch=2, lanes=2, graphs=False)
    tr.push([0, 3], [frames[0], frames[1]], [Ks[0], Ks[1]])
    r0 = tr.result()
    assert set(r0) == {0, 3}
    tr.push([3], [frames[2]], [Ks[2]])
    r1 = tr.result([3])
    one = chain.query(_it(frames[2]), _it(Ks[2]), pose_init=_it(r0[3][0]), refine_iter=1)["pose"].numpy()
    np.testing.assert_allclose(r1[3][0], one, atol=2e-4)
    np.testing.assert_array_equal(tr.result([0])[0][0], r0[0][0])          # untouched by the other group's tick
    tr.reset([3])
    tr.push([0, 3], [frames[1], frames[3]], [Ks[1], Ks[3]])
    r2 = tr.result()
    full = chain.query(_it(frames[3]), _it(Ks[3]))["pose"].numpy()
    np.testing.assert_allclose(r2[3][0], full, atol=2e-4)                   # started over: detection + 2 steps
    np.testing.assert_allclose(r2[3][1], r2[3][0], atol=1e-5)               # ... with a fresh smoothing history
    assert int(tr.hist_count[3]) == 1 and int(tr.hist_count[0]) == 2
    one = chain.query(_it(frames[1]), _it(Ks[1]), pose_init=_it(r0[0][0]), refine_iter=1)["pose"].numpy()
    np.testing.assert_allclose(r2[0][0], one, atol=2e-4)


def test_errors(scene, patched):
    est, frames, Ks = scene
    with pytest.raises(ValueError):
        T.StreamTracker(est, 4, batch=33, graphs=False)
    with pytest.raises(ValueError):
        T.StreamTracker(est, 4, graphs=True)                                # no GPU here
    tr = T.StreamTracker(est, 4, batch=2, graphs=False)
    with pytest.raises(ValueError):
        tr.push([4], [frames[0]])
    with pytest.raises(ValueError):
        tr.push([-1], [frames[0]])
    with pytest.raises(ValueError):
        tr.push([1, 1], [frames[0], frames[0]])
    tr.push([1], [frames[0]])
    with pytest.raises(ValueError):
        tr.push([2], [np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(ValueError):
        tr.push([2], [frames[0].astype(np.float32)])
    with pytest.raises(ValueError):
        tr.result([2])
    with pytest.raises(ValueError):
        tr.reset([7])
    refiner = est.refiner
    try:
        est.refiner = None
        with pytest.raises(ValueError):
            T.StreamTracker(est, 4, graphs=False)
    finally:
        est.refiner = refiner
