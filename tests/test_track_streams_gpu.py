"""gen6d_amd.tracking on the MI355X: the track_gather / track_commit kernels against the numpy host code, captured lanes against the
eager ticks and against per-stream DeviceChain.query(pose_init=...) steps, 32 streams in one graph, subset pushes, a reset while other
lanes are in flight, no synchronisation inside track_streams, and its fp16 pair range fallback."""
import numpy as np
import pytest
import torch

from gen6d_amd import eval as EV
from gen6d_amd import geometry as G
from gen6d_amd import ops, synth
from gen6d_amd import tracking as T
from test_split16_range_cpu import reparam
from test_track_streams_cpu import np_track_commit, np_track_gather

pytestmark = pytest.mark.gpu

GAINS = {2: 2.0 ** -10, 4: 2.0 ** 18}


def _db():
    from gen6d_amd.synth_db import SyntheticDatabase
    return SyntheticDatabase(n_views=24, size=(96, 128), focal=140.0)


def _est(db, refine_iter=2):
    from test_estimator_cpu import make_estimator
    est = make_estimator("cuda", refine_iter=refine_iter, damped=True)
    est.build(db, "all")
    return est


@pytest.fixture(scope="module")
def scene():
    db = _db()
    est = _est(db)
    _, que_ids = db.get_split("all")
    frames = [db.get_image(i) for i in que_ids]
    Ks = [db.get_K(i) for i in que_ids]
    return db, est, frames, Ks


def _it(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_kernels_match_host_code():
    rng = np.random.RandomState(0)
    poses, Ks = synth.fibonacci_cameras(12, radius=3.0, focal=300.0, size=256)
    box = G.box_corners(rng.uniform(-0.5, 0.5, (100, 3))).astype(np.float32)
    S, B, num, std = 6, 5, 3, 1.5
    dev = {k: torch.zeros(sh, dtype=dt, device="cuda") for k, sh, dt in
           [("P", (S, 12), torch.float32), ("Sm", (S, 12), torch.float32), ("H", (S, num, 8, 2), torch.float64), ("C", (S,), torch.int32)]}
    host = {k: v.cpu() for k, v in dev.items()}
    park = torch.from_numpy(poses[11].reshape(12)).cuda()
    maps = [[0, 1, 2, 3, 4], [5, -1, 2, -1, 0], [0, 1, 2, 3, 4], [-1, -1, 3, -1, -1], [4, 3, 2, 1, 0], [0, 5, 1, 2, 3]]
    for f, m in enumerate(maps):
        pose = np.stack([synth.perturb_pose(poses[(k + f) % 11], rng.uniform(-3, 3), rng.uniform(-0.03, 0.03)) for k in range(B)])
        K = np.stack([Ks[k] for k in range(B)]).astype(np.float32)
        mt = torch.tensor(m, dtype=torch.int32)
        reset = f == 2
        g = ops.track_gather(dev["P"], mt.cuda(), park)
        gh = np_track_gather(host["P"], mt, park.cpu())
        np.testing.assert_array_equal(g.cpu().numpy(), gh.numpy())
        out = torch.full((B, 2, 3, 4), 7.0, device="cuda")
        ops.track_commit(_it(pose), _it(K), mt.cuda(), reset, _it(box), num, std, dev["P"], dev["H"], dev["C"], dev["Sm"], out=out)
        oh = np_track_commit(torch.from_numpy(pose), torch.from_numpy(K), mt, reset, torch.from_numpy(box), num, std, host["P"], host["H"],
                             host["C"], host["Sm"], out=torch.full((B, 2, 3, 4), 7.0))
        np.testing.assert_allclose(out.cpu().numpy(), oh.numpy(), rtol=0, atol=1e-5)
        np.testing.assert_array_equal(dev["C"].cpu().numpy(), host["C"].numpy())
        np.testing.assert_allclose(dev["H"].cpu().numpy(), host["H"].numpy(), rtol=1e-12, atol=1e-9)
        for k in ("P", "Sm"):
            np.testing.assert_allclose(dev[k].cpu().numpy(), host[k].numpy(), rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        ops.track_commit(_it(pose), _it(K), mt.cuda(), False, _it(box), num + 1, std, dev["P"], dev["H"], dev["C"], dev["Sm"])
    with pytest.raises(ValueError):
        ops.track_gather(dev["P"], mt.cuda().long(), park)


def _seqs(frames, S, T_, seed=0):
    rng = np.random.RandomState(seed)
    return [[frames[(s * 3 + t) % len(frames)] for t in range(T_ - rng.randint(0, 2))] for s in range(S)]


def _check_one_step(chain, seqs, Kseq, res, bar=3e-4):
    for s, (poses, smooth) in enumerate(res):
        assert np.isfinite(poses).all() and np.isfinite(smooth).all()
        for t in range(1, len(poses)):
            one = chain.query(_it(seqs[s][t]), _it(Kseq[s][t]), pose_init=_it(poses[t - 1]), refine_iter=1)["pose"].cpu().numpy()
            np.testing.assert_allclose(poses[t], one, atol=bar, err_msg=f"stream {s} frame {t}")


def test_graphs_match_eager_and_per_stream_steps(scene):
    db, est, frames, Ks = scene
    seqs = _seqs(frames, 5, 4)
    Kss = [Ks[s] for s in range(5)]
    g = T.track_streams(est, seqs, Kss, batch=2, lanes=2, graphs=True)
    e = T.track_streams(est, seqs, Kss, batch=2, lanes=2, graphs=False)
    for (pg, sg), (pe, se) in zip(g, e):
        np.testing.assert_allclose(pg, pe, atol=3e-4)
        np.testing.assert_allclose(sg, se, atol=3e-4)
    _check_one_step(est.device_chain(), seqs, [[K] * len(q) for K, q in zip(Kss, seqs)], g)
    box = G.box_corners(EV.get_ref_point_cloud(est.refiner.ref_database))
    for (poses, smooth), K in zip(g, Kss):          # the device smoothing against predict.py's on the host, from the same raw poses
        hist, ref = [], []
        for p in poses.astype(np.float64):
            hist.append(G.project_points(box, p, K.astype(np.float64))[0])
            ref.append(G.pnp(box, G.weighted_points(hist, 5, 2.5), K.astype(np.float64), p))
        np.testing.assert_allclose(smooth, np.asarray(ref), atol=1e-5)


def test_32_streams_one_graph_and_subset_pushes(scene):
    db, est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    tr = T.StreamTracker(est, 32, batch=32, lanes=1)
    ids = list(range(32))
    tr.push(ids, [frames[s % len(frames)] for s in ids])
    first = tr.result()
    tr.push(ids, [frames[(s + 1) % len(frames)] for s in ids])
    second = tr.result()
    chain = est.device_chain()
    K = EV.pseudo_K(h, w)
    for s in (0, 13, 31):
        one = chain.query(_it(frames[(s + 1) % len(frames)]), _it(K), pose_init=_it(first[s][0]), refine_iter=1)["pose"].cpu().numpy()
        np.testing.assert_allclose(second[s][0], one, atol=3e-4)
    sub = [3, 17, 30]
    for k in range(2):                                 # partial ticks: the other 29 slots park, no pair map leaves the window
        tr.push(sub, [frames[(s + 2 + k) % len(frames)] for s in sub])
    r = tr.result()                                    # raises if a range record tripped
    assert all(np.isfinite(r[s][0]).all() and np.isfinite(r[s][1]).all() for s in sub)
    np.testing.assert_array_equal(r[0][0], second[0][0])
    assert est.refiner.range_fallbacks == 0


def test_reset_while_other_lanes_in_flight(scene):
    db, est, frames, Ks = scene
    n = len(frames)
    tr = T.StreamTracker(est, 6, batch=2, lanes=3)
    ids = list(range(6))
    for k in range(3):
        if k == 2:
            tr.reset([3])                              # no synchronisation: lanes 0 and 2 keep running
        tr.push(ids, [frames[(s + k) % n] for s in ids], [Ks[(s + k) % n] for s in ids])
    r = tr.result()
    assert int(tr.hist_count[3]) == 1 and int(tr.hist_count[2]) == 3
    np.testing.assert_allclose(r[3][1], r[3][0], atol=1e-5)
    # stream 3 started over alone in its lane's init chunk: the full chain on that frame
    full = est.device_chain().query(_it(frames[5 % n]), _it(Ks[5 % n]))["pose"].cpu().numpy()
    np.testing.assert_allclose(r[3][0], full, atol=3e-4)


def test_track_streams_does_not_synchronise(scene, monkeypatch):
    db, est, frames, Ks = scene
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
    res = T.track_streams(est, _seqs(frames, 3, 4, seed=1), batch=2, lanes=2)
    assert len(at_push) == 4 and at_push[-1] == 0, at_push
    assert counts["n"] > 0 and all(np.isfinite(p).all() for p, _ in res)


def test_range_fallback_of_track_streams():
    db = _db()
    est = _est(db)
    sd = reparam(synth.synth_state_dict("refiner"), GAINS, prefix="feature_net.backbone.features")
    est.refiner.load_state_dict(synth.damp_refiner_head(sd))
    _, que_ids = db.get_split("all")
    seqs = [[db.get_image(i) for i in que_ids[:3]], [db.get_image(i) for i in que_ids[3:5]]]
    Ks = [db.get_K(que_ids[0]), db.get_K(que_ids[3])]
    res = T.track_streams(est, seqs, Ks, batch=4, lanes=1)           # 4 slots x 7 crops: the trunk on the pairs (f43 calls)
    assert est.refiner.range_fallbacks == 1
    est.refiner.cfg["fp32_cores"] = True               # the recompute's routes: the refiner on fp32, the others on their pairs
    try:
        host = [T.host_track(est, q, [K] * len(q)) for q, K in zip(seqs, Ks)]
    finally:
        est.refiner.cfg.pop("fp32_cores")
    for (p, s), (hp, hs) in zip(res, host):
        np.testing.assert_allclose(p, hp, atol=1e-5)
        np.testing.assert_allclose(s, hs, atol=1e-5)
    est.refiner.load_state_dict(synth.damp_refiner_head(sd))        # exponents back to 0: the maps leave the window again
    tr = T.StreamTracker(est, 2, batch=4, lanes=1)
    tr.push([0, 1], [seqs[0][0], seqs[1][0]], Ks)
    tr.push([0, 1], [seqs[0][1], seqs[1][1]], Ks)
    with pytest.raises(RuntimeError, match="window"):
        tr.result()
