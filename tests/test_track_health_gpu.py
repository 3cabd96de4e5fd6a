"""Track health on the MI355X: g6d_track_gate / g6d_track_health / g6d_track_verify against the numpy restatement of
tests/test_track_health_cpu.py, and the tracker with a HealthPolicy in captured lanes: a lax policy against no policy, a forced loss and
its re-acquisition beside undisturbed lane mates, a NaN in the pose table, the detector's check, and the picture a LOST stream emits.

The scene's networks carry random weights and hold the object centre at a depth of 0 +- 1e-3 under the scene's intrinsics (see the note
in the CPU file), so a stream can go BEHIND the camera at any frame.  Tests that need every stream alive feed long-lens intrinsics and
assert on the health-free tracker's poses that all frames stay in front; one case keeps the scene's intrinsics and takes from the
health-free tracker where BEHIND must fire."""
import numpy as np
import pytest
import torch

from gen6d_amd import emit as E
from gen6d_amd import ops, synth
from gen6d_amd import tracking as T
from test_emit_cpu import assert_sink, np_corners, np_emit
from test_track_health_cpu import (clear_of_thresholds, compare_with_plain, depth, long_lens, np_centre, np_track_gate, np_track_health,
                                   np_track_verify, np_verify_gates)
from test_track_streams_gpu import _it, _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

BAR = 3e-4                                  # the project's bar for batched rows against single ones (test_track_streams_gpu.py)


def _margin(center):
    """Two poses within BAR of each other hold the centre's depth R[2] . c + t_z within BAR (|c|_1 + 1) of each other."""
    return BAR * (1.0 + float(np.abs(np.asarray(center, np.float64)).sum()))


def test_kernels_match_numpy():
    rng = np.random.RandomState(0)
    poses, Ks = synth.fibonacci_cameras(12, radius=3.0, focal=300.0, size=256)
    S, B, diam, ref_px = 6, 5, 1.3, 140.0
    c = np.array([0.04, -0.02, 0.03], np.float32)
    pol = T.HealthPolicy(patience=2, min_px=100.0, max_px=0.55, margin=0.1, max_rot_deg=2.0, max_shift=0.06, max_log2_scale=0.03,
                         verify_shift=0.05, verify_log2_scale=0.2, verify_patience=2)
    dev = {"P": torch.zeros((S, 12), device="cuda"), "H": torch.zeros((S, 4), dtype=torch.int32, device="cuda"),
           "M": torch.zeros((S, 12), device="cuda")}
    host = {k: v.cpu() for k, v in dev.items()}
    park, ct = torch.from_numpy(poses[11].reshape(12)), torch.from_numpy(c)
    maps = [[0, 1, 2, 3, 4], [5, -1, 2, -1, 0], [0, 1, 2, 3, 4], [-1, -1, 3, -1, -1], [4, 3, 2, 1, 0], [0, 5, 1, 2, 3], [0, 1, 2, 3, 4],
            [5, 4, -1, 1, 0], [2, 3, 4, 5, 0]]
    seen, stats, checked = set(), set(), set()
    for f, m in enumerate(maps):
        reset = f in (0, 1, 5)
        mt = torch.tensor(m, dtype=torch.int32)
        if f == 4:                                             # a poisoned row: the gate loses the stream, the gather parks it
            for t in (dev["P"], host["P"]):
                t[2, 9] = float("inf")
        if reset:
            eff_d, eff_h, prev_d, prev_h = mt.cuda(), mt, None, None
        else:
            eff_d = ops.track_gate(dev["P"], dev["H"], mt.cuda())
            eff_h = np_track_gate(host["P"], host["H"], mt)
            np.testing.assert_array_equal(eff_d.cpu().numpy(), eff_h.numpy())
            np.testing.assert_array_equal(dev["H"].cpu().numpy(), host["H"].numpy())
            prev_d = ops.track_gather(dev["P"], eff_d, park.cuda()).reshape(B, 12)
            prev_h = prev_d.cpu()
            assert torch.isfinite(prev_h).all()
        new = np.zeros((B, 3, 4), np.float32)
        for b, s in enumerate(m):
            base = poses[(b + f) % 11] if reset or s < 0 or not host["P"][s].any() or not torch.isfinite(host["P"][s]).all() else \
                host["P"][s].reshape(3, 4).numpy()
            new[b] = synth.perturb_pose(base, rng.choice([-1, 1]) * rng.uniform(0.5, 3.0), rng.choice([-1, 1]) * rng.uniform(0.005, 0.03))
        if f in (1, 3):
            new[2, 1, 1] = float("nan")
        if f in (5, 6):
            new[1, :, 3] *= -1                                 # behind the camera
        K = np.stack([Ks[k] for k in range(B)]).astype(np.float32)
        pic = torch.tensor([[256 - 8 * b, 200 + 4 * b] for b in range(B)], dtype=torch.int32) if f % 2 else None
        newt, Kt = torch.from_numpy(new).reshape(B, 12), torch.from_numpy(K).reshape(B, 9)
        cm_d, dr_d = ops.track_health(prev_d, newt.cuda(), Kt.cuda(), None if pic is None else pic.cuda(), (256, 256), eff_d, reset, ct.cuda(),
                                      diam, pol, dev["H"], dev["M"])
        chk = []
        cm_h, dr_h = np_track_health(prev_h, newt, Kt, pic, (256, 256), eff_h, reset, ct, diam, pol, host["H"], host["M"], check=chk)
        for fl, mm, w, h in chk:
            assert clear_of_thresholds(mm, fl, w, h, pol, reset), (f, fl, mm)
            seen.add(fl)
        np.testing.assert_array_equal(cm_d.cpu().numpy(), cm_h.numpy())
        np.testing.assert_array_equal(dr_d.cpu().numpy(), dr_h.numpy())
        np.testing.assert_array_equal(dev["H"].cpu().numpy(), host["H"].numpy())
        np.testing.assert_allclose(dev["M"].cpu().numpy(), host["M"].numpy(), rtol=1e-6, atol=0)
        for b, s in enumerate(cm_h.tolist()):                  # (the commit itself is track_commit's business: the raw pose only)
            if s >= 0:
                host["P"][s] = newt[b]
                dev["P"][s] = newt[b].cuda()
        if f % 3 == 1 or f == 6:                               # the detector's check of what was just committed
            det = np.zeros((B, 5), np.float32)
            for b, s in enumerate(cm_h.tolist()):
                src = host["P"][s if s >= 0 else 0].reshape(3, 4).numpy().astype(np.float64)
                u, v, _, d = np_centre(src, K[b].astype(np.float64), c.astype(np.float64), diam)
                det[b] = [u + rng.uniform(-0.1, 0.1) * d, v + rng.uniform(-0.1, 0.1) * d, d / ref_px * 2.0 ** rng.uniform(-0.4, 0.4), 1, b]
                fl, mm = np_verify_gates(det[b].astype(np.float64), src, K[b].astype(np.float64), c.astype(np.float64), diam, ref_px, pol)
                assert all(abs(x - t) > 1e-6 * t for x, t in zip(mm, (pol.verify_shift, pol.verify_log2_scale)))
            dt = torch.from_numpy(det)
            ops.track_verify(dt.cuda(), dev["P"], Kt.cuda(), cm_d, ct.cuda(), diam, ref_px, pol, dev["H"], dev["M"])
            np_track_verify(dt, host["P"], Kt, cm_h, ct, diam, ref_px, pol, host["H"], host["M"])
            np.testing.assert_array_equal(dev["H"].cpu().numpy(), host["H"].numpy())
            np.testing.assert_allclose(dev["M"].cpu().numpy(), host["M"].numpy(), rtol=1e-6, atol=0)
            checked |= set((host["H"][:, 3] & 768).tolist())
        stats |= set(host["H"][:, 0].tolist())
    assert {0, T.NONFINITE, T.BEHIND} <= seen and len(seen) >= 5 and {T.TRACKING, T.SUSPECT, T.LOST} <= stats, (seen, stats)
    assert len(checked) >= 2, checked                          # checks passed and failed
    with pytest.raises(ValueError):
        ops.track_gate(dev["P"], dev["H"], mt.cuda().long())
    with pytest.raises(ValueError):
        ops.track_health(None, newt.cuda(), Kt.cuda(), None, (256, 256), mt.cuda(), False, ct.cuda(), diam, pol, dev["H"], dev["M"])
    with pytest.raises(ValueError):
        ops.track_health(None, newt.cuda(), Kt.cuda(), None, None, mt.cuda(), True, ct.cuda(), diam, pol, dev["H"], dev["M"])
    with pytest.raises(ValueError):
        ops.track_verify(dt.cuda()[:, :4].contiguous(), dev["P"], Kt.cuda(), mt.cuda(), ct.cuda(), diam, ref_px, pol, dev["H"], dev["M"])


def test_lax_policy_in_captured_lanes(scene):
    """5 streams x 4 frames, batch 2 x 2 lanes, graphs, behind long-lens intrinsics that keep every pose of the health-free tracker in
    front of the camera: all 20 frames within the batch bar of the tracker without health, every status TRACKING."""
    db, est, frames, Ks = scene
    seqs = [q[:4] for q in _seqs(frames, 5, 5)]
    Kss = [long_lens(Ks[s]) for s in range(5)]
    center = est.ref_info["center"]
    plain = T.track_streams(est, seqs, Kss, batch=2, lanes=2, graphs=True)
    assert all(len(p) == 4 and depth(x, center) > 10 * _margin(center) for p, _ in plain for x in p)
    lax = T.track_streams(est, seqs, Kss, batch=2, lanes=2, graphs=True, health=T.HealthPolicy.lax())
    for (p, s), (ph, sh, st) in zip(plain, lax):
        np.testing.assert_allclose(ph, p, atol=BAR)
        np.testing.assert_allclose(sh, s, atol=BAR)
        assert st.tolist() == [T.TRACKING] * 4
    assert est.refiner.range_fallbacks == 0


def test_lax_policy_keeps_the_hard_gates(scene):
    """The scene's own intrinsics: where the health-free tracker puts the centre behind the camera the stream is LOST, equal before."""
    db, est, frames, Ks = scene
    seqs = [q[:4] for q in _seqs(frames, 5, 5)]
    Kss = [Ks[s] for s in range(5)]
    plain = T.track_streams(est, seqs, Kss, batch=2, lanes=2, graphs=True)
    lax = T.track_streams(est, seqs, Kss, batch=2, lanes=2, graphs=True, health=T.HealthPolicy.lax())
    center = est.ref_info["center"]
    n = compare_with_plain(plain, lax, center, lambda a, b: np.testing.assert_allclose(a, b, atol=BAR), margin=_margin(center))
    assert n >= 1 and any(T.LOST in st.tolist() for _, _, st in lax)


def _front_frame(est, frames, Ks, K_step=None):
    """The first scene frame whose acquisition, and one step from it (under K_step), hold the centre clearly in front: by the chain alone."""
    chain, center = est.device_chain(), est.ref_info["center"]
    for i in range(len(frames)):
        first = chain.query(_it(frames[i]), _it(Ks[i]))["pose"]
        Kn = Ks[i] if K_step is None else K_step(Ks[i])
        step = chain.query(_it(frames[i]), _it(Kn), pose_init=first, refine_iter=1)["pose"]
        if min(depth(first.cpu().numpy(), center), depth(step.cpu().numpy(), center)) > 2 * _margin(center):
            return i, first.cpu().numpy()
    pytest.fail("no scene frame keeps the object centre in front of the camera")


@pytest.mark.parametrize("batch", [4, 32])
def test_forced_loss_and_reacquisition_beside_lane_mates(scene, batch):
    """One stream of a lane is fed intrinsics of 1000 x the focal length on its tracked frames 1..2: its projected diameter is 1000 x its
    lane mates' and fails LARGE (the threshold sits 40 x above any mate's and 25 x below the stream's as long as depths lie in
    [2.4e-5, 2.4e-2]; they are ~1e-3).  patience 2, lag 1: SUSPECT at frame 1, LOST at 2, re-acquired at 2 + lag = 3."""
    db, est, frames, Ks = scene
    big = lambda K: (K * np.array([[1000.0, 1, 1], [1, 1000.0, 1], [1, 1, 1]])).astype(np.float32)
    i0, first = _front_frame(est, frames, Ks, big)
    victim, n = 1, len(frames)
    h, w = frames[0].shape[:2]
    pol = T.HealthPolicy.lax(max_px=1e7 / max(h, w), patience=2, lag=1)
    seqs = [[frames[i0 if s == victim else (s + t) % n] for t in range(4)] for s in range(batch)]
    KB = [np.stack([Ks[i0 if s == victim else (s + t) % n] for t in range(4)]) for s in range(batch)]
    KA = [k.copy() for k in KB]
    KA[victim][1:3] = big(Ks[i0])
    A = T.track_streams(est, seqs, KA, batch=batch, lanes=1, graphs=True, health=pol)
    Bc = T.track_streams(est, seqs, KB, batch=batch, lanes=1, graphs=True, health=pol)
    Tr, Su, Lo = T.TRACKING, T.SUSPECT, T.LOST
    p, s, st = A[victim]
    assert st.tolist() == [Tr, Su, Lo, Tr], st
    for t in (1, 2):
        np.testing.assert_array_equal(p[t], p[0])              # none of the bad frames was committed
    np.testing.assert_allclose(p[3], first, atol=BAR)          # alone in its init chunk: the full chain on that frame
    np.testing.assert_allclose(s[3], p[3], atol=1e-5)          # ... with a fresh smoothing history
    for m in range(batch):                                     # the parked slot shares every launch with its lane mates
        if m != victim:
            assert A[m][2].tolist() == Bc[m][2].tolist(), m
            np.testing.assert_allclose(A[m][0], Bc[m][0], atol=BAR, err_msg=f"lane mate {m}")
            np.testing.assert_allclose(A[m][1], Bc[m][1], atol=BAR, err_msg=f"lane mate {m}")
    assert est.refiner.range_fallbacks == 0


def _pushes(frames, Ks, ids, k):
    """Frame k of every stream behind long-lens intrinsics: every stream stays in front of the camera (the tests assert it)."""
    n = len(frames)
    return [frames[(s + k) % n] for s in ids], [long_lens(Ks[s % n]) for s in ids]


def test_nan_in_the_pose_table(scene):
    db, est, frames, Ks = scene
    S = 8
    tr = T.StreamTracker(est, S, batch=8, lanes=1, graphs=True, health=T.HealthPolicy.lax())
    ids = list(range(S))
    for k in range(2):
        tr.push(ids, *_pushes(frames, Ks, ids, k))
    before = tr.health()
    assert all(before[s].status == T.TRACKING for s in ids), before
    good = tr.result()
    victim = 3
    tr.pose_table[victim, 3] = float("nan")
    tr.push(ids, *_pushes(frames, Ks, ids, 2))
    r = tr.result()                                            # does not raise: the value reached no network and no range record
    after = tr.health()
    assert after[victim].status == T.LOST and after[victim].flags == T.NONFINITE
    for s in ids:
        if s != victim:                                        # the lane mates went on: a new, finite, committed frame
            assert after[s].status == T.TRACKING and np.isfinite(r[s][0]).all() and np.isfinite(r[s][1]).all()
            assert not np.array_equal(r[s][0], good[s][0]) and int(tr.hist_count[s]) == 3
    assert int(tr.hist_count[victim]) == 2 and est.refiner.range_fallbacks == 0
    K = long_lens(Ks[victim])
    first = est.device_chain().query(_it(frames[0]), _it(K))["pose"].cpu().numpy()
    tr.push([victim], [frames[0]], [K])                        # the host has just read the status: this push re-acquires
    np.testing.assert_allclose(tr.result([victim])[victim][0], first, atol=BAR)
    assert tr.health([victim])[victim].status == T.TRACKING


def test_detector_check(scene):
    db, est, frames, Ks = scene
    S = 8
    chain, ids = est.device_chain(), list(range(8))
    tr = T.StreamTracker(est, S, batch=8, lanes=1, graphs=True, health=T.HealthPolicy.lax(verify_every=1))
    for k in range(2):
        tr.push(ids, *_pushes(frames, Ks, ids, k))
    hl = tr.health()
    lane = tr._lanes[0]
    assert lane.commit.cpu().tolist() == ids                   # every stream committed its tracked frame and was checked
    det = chain.detect_batch(lane.img).cpu().numpy().astype(np.float64)
    P, K, c = tr.pose_table.cpu().numpy().astype(np.float64), lane.K.cpu().numpy().astype(np.float64), est.ref_info["center"].astype(np.float64)
    for s in ids:
        _, m = np_verify_gates(det[s], P[s].reshape(3, 4), K[s], c, tr.diameter, tr.ref_px, tr.policy)
        np.testing.assert_allclose(hl[s].measures[7:9], m, rtol=1e-4, atol=0)
        assert hl[s].status == T.TRACKING and hl[s].vbad == 0 and not hl[s].flags & 768
    # a check that cannot pass: one failure after the first tracked frame, LOST after the second (verify_patience = 2)
    tr = T.StreamTracker(est, S, batch=8, lanes=1, graphs=True, health=T.HealthPolicy.lax(verify_every=1, verify_shift=-1.0, verify_patience=2))
    for k in range(3):
        tr.push(ids, *_pushes(frames, Ks, ids, k))
        hl = tr.health()
        want = [(T.TRACKING, 0, 0), (T.TRACKING, 1, T.VERIFY_POS), (T.LOST, 2, T.VERIFY_POS)][k]
        for s in ids:
            assert (hl[s].status, hl[s].vbad, hl[s].flags) == want, (k, s, hl[s])


def test_emit_follows_the_status(scene):
    """A SUSPECT stream's sink shows the box of its last good pose, a LOST stream's the bare picture although its table row still holds
    that pose.  The stream is given a database pose as its committed pose (the scene's own poses project outside the corner range) and
    every tracked frame fails SHIFT: SUSPECT at push 1, LOST at push 2 (patience 2), both in the lane's captured tick."""
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    tr = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=True, health=T.HealthPolicy.lax(max_shift=-1.0, patience=2, lag=2))
    tr.push([0, 1], [frames[0], frames[1]], [long_lens(Ks[0]), long_lens(Ks[1])])
    assert tr.health([1])[1].status == T.TRACKING
    pose = np.asarray(est.ref_info["poses"][0], np.float32).reshape(3, 4)
    K = np.asarray(est.ref_info["Ks"][0], np.float32).reshape(3, 3)
    tr.pose_table[1] = torch.from_numpy(pose.reshape(12)).cuda()
    q, ok, _ = np_corners(tr.box.cpu().numpy(), pose, K)
    assert ok == 1
    sinks = [E.Sink(torch.full((H * 3 // 2, W), 7, dtype=torch.uint8, device="cuda"), "nv12", pose="raw") for _ in range(2)]
    for k in range(2):
        tr.push([0, 1], [frames[0], frames[k + 2]], [K, K], sinks=[None, sinks[k]])
    tr.result()
    h = tr.health([1])[1]
    assert (h.status, h.bad, h.flags) == (T.LOST, 2, T.SHIFT) and int(tr.hist_count[1]) == 1
    np.testing.assert_array_equal(tr.pose_table[1].cpu().numpy(), pose.reshape(12))          # the good pose is still there
    assert_sink(sinks[0], np_emit(frames[2], q, sinks[0]), "SUSPECT stream: the last good box")
    assert_sink(sinks[1], np_emit(frames[3], None, sinks[1]), "LOST stream: no box")
