"""Track health (gen6d_amd.tracking.HealthPolicy) without a GPU.  `np_track_gate`, `np_track_health` and
`np_track_verify` restate the specification of the three kernels in numpy on the tables' memory (tests/test_track_health_gpu.py holds the
kernels against them); the arithmetic of gen6d_amd/csrc/pose_algebra.h is built for the host (tests/track_health_shim.cpp) and checked
against them; the eager tracker runs with tests/ref_ops.py and the numpy track ops patched in; the kernels' compiler metadata is pinned
at zero scratch and zero spills."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import lib, ops, synth
from gen6d_amd import tracking as T
from test_track_streams_cpu import _it, np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
GATE_FIELDS = ("min_px", "max_px", "margin", "max_rot_deg", "max_shift", "max_log2_scale")


# ---------------------------------------------------------------------------------------------------------------- numpy restatement
def np_centre(pose, K, c, diameter):
    """X = R c + t -> (u, v, z, d_px)."""
    X = pose[:, :3] @ c + pose[:, 3]
    q = K @ X
    with np.errstate(all="ignore"):
        return q[0] / X[2], q[1] / X[2], X[2], 0.5 * (K[0, 0] + K[1, 1]) * diameter / X[2]


def np_gates(prev, cur, K, w, h, c, diameter, pol):
    """One candidate pose (float64 arrays; prev None: an acquisition) -> (flag bits 0..7, measures [7])."""
    m = np.zeros(7)
    if not np.isfinite(cur).all():
        return T.NONFINITE, m
    u, v, z, d = np_centre(cur, K, c, diameter)
    m[2] = z
    if not z > 0:
        return T.BEHIND, m
    m[0], m[1], m[3] = u, v, d
    f = 0
    if not d >= pol.min_px:
        f |= T.SMALL
    if not d <= pol.max_px * max(w, h):
        f |= T.LARGE
    mg = pol.margin * d
    if not (u >= -mg and u <= w + mg and v >= -mg and v <= h + mg):
        f |= T.OUTSIDE
    if prev is not None:
        m[4] = np.degrees(np.arccos(np.clip((np.sum(cur[:, :3] * prev[:, :3]) - 1.0) / 2.0, -1.0, 1.0)))
        if not m[4] <= pol.max_rot_deg:
            f |= T.ROT
        up, vp, zp, _ = np_centre(prev, K, c, diameter)
        if not zp > 0:
            f |= T.SCALE
        else:
            m[5] = np.hypot(u - up, v - vp) / d
            m[6] = abs(np.log2(zp / z))
            if not m[5] <= pol.max_shift:
                f |= T.SHIFT
            if not m[6] <= pol.max_log2_scale:
                f |= T.SCALE
    return f, m


def np_update(row, f, reset, patience):
    """(status, bad, vbad, flags) in place -> (commit, draw)."""
    if reset:
        row[0], row[1], row[2] = (T.LOST if f else T.TRACKING), 0, 0
    elif f & (T.NONFINITE | T.BEHIND):
        row[0] = T.LOST
    elif f:
        row[1] += 1
        row[0] = T.LOST if row[1] >= patience else T.SUSPECT
    else:
        row[0], row[1] = T.TRACKING, 0
    row[3] = (row[3] & 768) | f
    return f == 0, row[0] != T.LOST


def clear_of_thresholds(m, f, w, h, pol, reset, rel=1e-6):
    """The condition the comparisons of two implementations rest on: no measure lies within `rel` of its threshold."""
    def far(x, thr):
        return not np.isfinite(thr) or abs(x - thr) > rel * max(abs(thr), abs(x))
    if f & T.NONFINITE:
        return True
    if f & T.BEHIND or abs(m[2]) <= rel:
        return abs(m[2]) > rel
    mg = pol.margin * m[3]
    ok = far(m[3], pol.min_px) and far(m[3], pol.max_px * max(w, h))
    ok = ok and all(far(x, t) for x, t in ((m[0], -mg), (m[0], w + mg), (m[1], -mg), (m[1], h + mg)))
    if not reset:
        ok = ok and far(m[4], pol.max_rot_deg) and far(m[5], pol.max_shift) and far(m[6], pol.max_log2_scale)
    return ok


def _np64(t, shape):
    return t.reshape(shape).numpy().astype(np.float64)


def np_track_gate(pose_table, health, slot_stream, slot_eff=None):
    B = slot_stream.shape[0]
    slot_eff = torch.empty((B,), dtype=torch.int32) if slot_eff is None else slot_eff
    Hh, P = health.numpy(), pose_table.numpy()
    for b, s in enumerate(slot_stream.tolist()):
        eff = -1
        if s >= 0 and Hh[s, 0] != T.LOST:
            if np.isfinite(P[s]).all():
                eff = s
            else:
                Hh[s, 0], Hh[s, 3] = T.LOST, T.NONFINITE
        slot_eff[b] = eff
    return slot_eff


def np_track_health(pose_prev, pose_new, K, pic, size, slot_eff, reset, center, diameter, policy, health, measures, slot_commit=None,
                    slot_draw=None, check=None):
    """ops.track_health on host memory.  check: a list that receives (flags, measures, w, h) of every evaluated slot."""
    B = slot_eff.shape[0]
    slot_commit = torch.empty((B,), dtype=torch.int32) if slot_commit is None else slot_commit
    slot_draw = torch.empty((B,), dtype=torch.int32) if slot_draw is None else slot_draw
    Pn, Ks, c = _np64(pose_new, (B, 3, 4)), _np64(K, (B, 3, 3)), _np64(center, (3,))
    Pp = None if reset else _np64(pose_prev, (B, 3, 4))
    Hh, M = health.numpy(), measures.numpy()
    for b, s in enumerate(slot_eff.tolist()):
        slot_commit[b] = slot_draw[b] = -1
        if s < 0:
            continue
        w, h = (float(size[0]), float(size[1])) if pic is None else (float(pic[b, 0]), float(pic[b, 1]))
        f, m = np_gates(None if reset else Pp[b], Pn[b], Ks[b], w, h, c, float(diameter), policy)
        if check is not None:
            check.append((f, m, w, h))
        commit, draw = np_update(Hh[s], f, bool(reset), policy.patience)
        M[s, :7] = m.astype(np.float32)
        slot_commit[b] = s if commit else -1
        slot_draw[b] = s if draw else -1
    return slot_commit, slot_draw


def np_verify_gates(det, pose, K, c, diameter, ref_px, pol):
    u, v, _, d = np_centre(pose, K, c, diameter)
    m = np.array([np.hypot(det[0] - u, det[1] - v) / d, abs(np.log2(det[2] * ref_px / d))])
    return (0 if m[0] <= pol.verify_shift else T.VERIFY_POS) | (0 if m[1] <= pol.verify_log2_scale else T.VERIFY_SCALE), m


def np_verify_update(row, f, patience):
    if f:
        row[2] += 1
        if row[2] >= patience:
            row[0] = T.LOST
    else:
        row[2] = 0
    row[3] = (row[3] & 255) | f


def np_track_verify(det, pose_table, K, slot_commit, center, diameter, ref_px, policy, health, measures):
    B = slot_commit.shape[0]
    D, Ks, c, P = _np64(det, (B, 5)), _np64(K, (B, 3, 3)), _np64(center, (3,)), pose_table.numpy().astype(np.float64)
    Hh, M = health.numpy(), measures.numpy()
    for b, s in enumerate(slot_commit.tolist()):
        if s < 0:
            continue
        f, m = np_verify_gates(D[b], P[s].reshape(3, 4), Ks[b], c, float(diameter), float(ref_px), policy)
        np_verify_update(Hh[s], f, policy.verify_patience)
        M[s, 7:9] = m.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the algebra, on the host
D_ = C.POINTER(C.c_double)
I_ = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def th(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("th") / "track_health.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "track_health_shim.cpp"), "-o", so],
                   check=True)
    l = C.CDLL(so)
    l.h_gates.argtypes = [D_, D_, D_, C.c_double, C.c_double, D_, C.c_double, D_, D_]
    l.h_verify.argtypes = [D_, D_, D_, D_, C.c_double, C.c_double, C.c_double, C.c_double, D_]
    l.h_update.argtypes = [C.c_int, C.c_int, C.c_int, I_, I_]
    l.h_verify_update.argtypes = [C.c_int, C.c_int, I_]
    return l


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(D_)


def h_gates(th, prev, cur, K, w, h, c, diameter, pol):
    keep = [_d(cur), _d(K), _d(c), _d([getattr(pol, n) for n in GATE_FIELDS])]
    pp = None if prev is None else _d(prev)
    m = np.zeros(7)
    f = th.h_gates(None if pp is None else pp[1], keep[0][1], keep[1][1], w, h, keep[2][1], diameter, keep[3][1], m.ctypes.data_as(D_))
    return f, m


def _scene(n=8):
    """Cameras around the object, float32 poses as the tables hold them; the tracked pose of camera i is a perturbed neighbour."""
    poses, Ks = synth.fibonacci_cameras(n, radius=3.0, focal=400.0, size=320)
    c = np.array([0.05, -0.03, 0.02])
    prev = [p.astype(np.float64) for p in poses]
    cur = [synth.perturb_pose(p, 2.0 + 0.3 * i, 0.03).astype(np.float64) for i, p in enumerate(poses)]
    return prev, cur, [K.astype(np.float64) for K in Ks], c, 1.2, 320.0, 320.0


def _pol(**kw):
    return T.HealthPolicy(**kw)


def test_each_gate_alone_raises_its_bit(th):
    prev, cur, Ks, c, diam, w, h = _scene()
    behind = [np.concatenate([p[:, :3], -p[:, 3:]], 1) for p in cur]
    nonfin = [p.copy() for p in cur]
    for i, p in enumerate(nonfin):
        p.reshape(12)[i % 12] = [np.nan, np.inf, -np.inf][i % 3]
    far_K = [K + np.array([[0, 0, 1000.0], [0, 0, 0], [0, 0, 0]]) for K in Ks]
    cases = [  # (expected flags, policy, candidate poses, intrinsics)
        (0, _pol(), cur, Ks),
        (T.NONFINITE, _pol(), nonfin, Ks),
        (T.BEHIND, _pol(), behind, Ks),
        (T.SMALL, _pol(min_px=1e4), cur, Ks),
        (T.LARGE, _pol(max_px=1e-3), cur, Ks),
        (T.OUTSIDE, _pol(), cur, far_K),
        (T.ROT, _pol(max_rot_deg=0.01), cur, Ks),
        (T.SHIFT, _pol(max_shift=-1.0), cur, Ks),
        (T.SCALE, _pol(max_log2_scale=-1.0), cur, Ks),
        (T.SMALL | T.ROT | T.SCALE, _pol(min_px=1e4, max_rot_deg=0.01, max_log2_scale=0.01), cur, Ks),
        (0, T.HealthPolicy.lax(), cur, far_K),
    ]
    for want, pol, cand, KK in cases:
        for reset in (False, True):
            for i in range(len(cur)):
                pv = None if reset else prev[i]
                f, m = np_gates(pv, cand[i], KK[i], w, h, c, diam, pol)
                assert clear_of_thresholds(m, f, w, h, pol, reset), (want, i, m)
                assert f == (want & 31 if reset else want), (want, reset, i, f, m)
                fh, mh = h_gates(th, pv, cand[i], KK[i], w, h, c, diam, pol)
                assert fh == f
                np.testing.assert_allclose(mh, m, rtol=1e-9, atol=0)
                if f == 0 and not reset and KK is Ks:  # a plausible frame: in the picture, a few degrees, a small move
                    assert 0 < m[0] < w and 0 < m[1] < h and 1.9 < m[4] < 5 and 0 < m[5] < 1 and 0 < m[6] < 0.1 and m[3] > 100
    # a previous centre behind the camera fails SCALE alone and leaves shift and log2_scale 0
    pb = np.concatenate([prev[0][:, :3], -prev[0][:, 3:]], 1)
    f, m = np_gates(pb, cur[0], Ks[0], w, h, c, diam, T.HealthPolicy.lax())
    fh, mh = h_gates(th, pb, cur[0], Ks[0], w, h, c, diam, T.HealthPolicy.lax())
    assert f == fh == T.SCALE and m[5] == m[6] == mh[5] == mh[6] == 0 and m[4] > 0
    # a NaN threshold cannot be built
    with pytest.raises(ValueError):
        _pol(max_shift=float("nan"))


def _run(th, steps, patience, row=(0, 0, 0, 0)):
    """[(flags, reset)] through the header's update and numpy's -> the rows after every step and (commit, draw)."""
    a, b, out = np.array(row, np.int32), np.array(row, np.int32), []
    for f, reset in steps:
        cd = np.zeros(2, np.int32)
        th.h_update(f, int(reset), patience, a.ctypes.data_as(I_), cd.ctypes.data_as(I_))
        commit, draw = np_update(b, f, reset, patience)
        np.testing.assert_array_equal(a, b)
        assert (bool(cd[0]), bool(cd[1])) == (commit, draw)
        out.append((tuple(int(x) for x in b), commit, draw))
    return out


def test_state_machine(th):
    Tr, Su, Lo = T.TRACKING, T.SUSPECT, T.LOST
    # patience 3: two bad frames are forgiven by a good one, three in a row are not; LOST stays LOST on bad frames
    r = _run(th, [(0, True), (T.SHIFT, False), (T.ROT, False), (0, False), (T.SHIFT, False), (T.SHIFT, False), (T.SMALL, False),
                  (T.SMALL, False)], 3)
    assert [x[0][0] for x in r] == [Tr, Su, Su, Tr, Su, Su, Lo, Lo]
    assert [x[0][1] for x in r] == [0, 1, 2, 0, 1, 2, 3, 4]
    assert [x[1] for x in r] == [True, False, False, True, False, False, False, False]       # only good frames are committed
    assert [x[2] for x in r] == [True] * 6 + [False] * 2                                       # a SUSPECT stream is still drawn
    assert [x[0][3] for x in r] == [0, T.SHIFT, T.ROT, 0, T.SHIFT, T.SHIFT, T.SMALL, T.SMALL]
    # patience 1: the first bad frame loses the stream
    r = _run(th, [(0, True), (0, False), (T.OUTSIDE, False)], 1)
    assert [x[0][0] for x in r] == [Tr, Tr, Lo] and r[2][0][1] == 1
    # hard failures do not wait for patience and do not count as bad frames
    for hard in (T.NONFINITE, T.BEHIND):
        r = _run(th, [(0, True), (hard, False)], 5)
        assert r[1][0] == (Lo, 0, 0, hard) and r[1][1:] == (False, False)
    # an acquisition: passes -> TRACKING, fails -> LOST at once; the counters restart either way
    assert _run(th, [(0, True)], 3, row=(Lo, 3, 1, T.SHIFT | T.VERIFY_POS))[0] == ((Tr, 0, 0, T.VERIFY_POS), True, True)
    assert _run(th, [(T.SMALL, True)], 3, row=(Lo, 3, 1, T.SHIFT))[0] == ((Lo, 0, 0, T.SMALL), False, False)
    # the health update replaces bits 0..7 and keeps 8..9
    assert _run(th, [(T.ROT, False)], 3, row=(Tr, 0, 1, T.SCALE | T.VERIFY_SCALE))[0][0] == (Su, 1, 1, T.ROT | T.VERIFY_SCALE)
    # the check: a failure counts, verify_patience consecutive ones lose the stream, a pass clears the count and both bits; bits 0..7 stay
    a, b = np.array([Su, 1, 0, T.SHIFT], np.int32), np.array([Su, 1, 0, T.SHIFT], np.int32)
    want = [(T.VERIFY_POS, (Su, 1, 1, T.SHIFT | T.VERIFY_POS)), (0, (Su, 1, 0, T.SHIFT)), (T.VERIFY_SCALE, (Su, 1, 1, T.SHIFT | T.VERIFY_SCALE)),
            (T.VERIFY_POS | T.VERIFY_SCALE, (Lo, 1, 2, T.SHIFT | T.VERIFY_POS | T.VERIFY_SCALE))]
    for f, row in want:
        th.h_verify_update(f, 2, a.ctypes.data_as(I_))
        np_verify_update(b, f, 2)
        assert tuple(a) == tuple(b) == row


def test_verify_gates_and_tables(th):
    prev, cur, Ks, c, diam, w, h = _scene()
    ref_px = 150.0
    for i, (p, K) in enumerate(zip(cur, Ks)):
        u, v, _, d = np_centre(p, K, c, diam)
        for det, want, pol in [((u + 3, v - 4, d / ref_px * 1.1), 0, _pol()),
                               ((u + 3 * d, v, d / ref_px), T.VERIFY_POS, _pol()),
                               ((u, v + 1, 4.0 * d / ref_px), T.VERIFY_SCALE, _pol()),
                               ((u + 2 * d, v + 2 * d, 0.2 * d / ref_px), T.VERIFY_POS | T.VERIFY_SCALE, _pol()),
                               ((u + 2 * d, v + 2 * d, 0.2 * d / ref_px), 0, T.HealthPolicy.lax())]:
            f, m = np_verify_gates(np.array(det), p, K, c, diam, ref_px, pol)
            assert f == want
            assert all(not np.isfinite(t) or abs(x - t) > 1e-6 * t for x, t in zip(m, (pol.verify_shift, pol.verify_log2_scale)))
            keep = [_d(det), _d(p), _d(K), _d(c)]
            mh = np.zeros(2)
            fh = th.h_verify(*[k[1] for k in keep], diam, ref_px, pol.verify_shift, pol.verify_log2_scale, mh.ctypes.data_as(D_))
            assert fh == f
            np.testing.assert_allclose(mh, m, rtol=1e-9, atol=0)
    # the three table functions on a small table: who writes what
    S, B = 4, 3
    P = torch.from_numpy(np.stack([p.reshape(12) for p in prev[:S]]).astype(np.float32))
    Hh = torch.tensor([[T.TRACKING, 0, 0, 0], [T.LOST, 3, 0, T.SHIFT], [T.SUSPECT, 1, 1, T.ROT | T.VERIFY_POS], [T.TRACKING, 0, 0, 0]],
                      dtype=torch.int32)
    M = torch.zeros((S, 12))
    P[3, 7] = float("nan")
    eff = np_track_gate(P, Hh, torch.tensor([3, 1, 2], dtype=torch.int32))
    assert eff.tolist() == [-1, -1, 2] and Hh[3].tolist() == [T.LOST, 0, 0, T.NONFINITE] and Hh[1].tolist() == [T.LOST, 3, 0, T.SHIFT]
    assert np_track_gate(P, Hh, torch.tensor([0, -1, 2], dtype=torch.int32)).tolist() == [0, -1, 2]
    Kt = torch.from_numpy(np.stack(Ks[:B]).astype(np.float32))
    new = torch.from_numpy(np.stack([cur[0], cur[1], cur[2]]).astype(np.float32))
    old = torch.from_numpy(np.stack([prev[0], prev[1], prev[2]]).astype(np.float32))
    ct = torch.from_numpy(c.astype(np.float32))
    commit, draw = np_track_health(old, new, Kt, None, (w, h), torch.tensor([0, -1, 2], dtype=torch.int32), False, ct, diam, _pol(), Hh, M)
    assert commit.tolist() == [0, -1, 2] and draw.tolist() == [0, -1, 2]
    assert Hh[2].tolist() == [T.TRACKING, 0, 1, T.VERIFY_POS] and Hh[1].tolist() == [T.LOST, 3, 0, T.SHIFT]     # bits 8..9 and vbad kept
    assert (M[0, :7] != 0).all() and (M[1] == 0).all() and (M[:, 7:] == 0).all()
    det = torch.zeros((B, 5))
    for b in (0, 2):
        u, v, _, d = np_centre(P[[0, 0, 2][b]].reshape(3, 4).numpy().astype(np.float64), Ks[b], c, diam)
        det[b, :3] = torch.tensor([u + (0 if b else 5 * d), v, d / ref_px])
    Hh[0, 3] = T.SMALL
    np_track_verify(det, P, Kt, commit, ct, diam, ref_px, _pol(), Hh, M)
    assert Hh[0].tolist() == [T.TRACKING, 0, 1, T.SMALL | T.VERIFY_POS] and Hh[2].tolist() == [T.TRACKING, 0, 0, 0]
    assert abs(float(M[0, 7]) - 5.0) < 1e-5 and float(M[2, 7]) < 1e-6 and (M[1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the tracker, eager
# The synthetic scene's networks carry random weights: the detector reports a size ratio of ~4e4, so every pose of this scene holds the
# object centre at a depth of 0 +- 1e-3 and about a third of all frames put it BEHIND the camera, which no policy forgives.  The tests
# that need every stream alive therefore feed long-lens intrinsics (`long_lens`: the chain's depth scales with the focal length) and
# assert on the health-free tracker's poses that every frame stays in front; the scene's own intrinsics serve the case where BEHIND must
# fire, read from a reference that does not know about health (the plain tracker, DeviceChain.query).
def depth(pose, center):
    p = np.asarray(pose, np.float64).reshape(3, 4)
    return float(p[2, :3] @ np.asarray(center, np.float64).reshape(3) + p[2, 3])


def long_lens(K, mul=1000.0):
    """The same camera with `mul` times the focal length: the chain's depth of the object centre scales with it (~3e-5 x mul on this
    scene), which puts the centre clearly in front of the camera."""
    return (np.asarray(K, np.float32) * np.array([[mul, 1, 1], [1, mul, 1], [1, 1, 1]])).astype(np.float32)


def compare_with_plain(plain, lax, center, same, margin=1e-6):
    """A lax policy changes nothing but BEHIND: per stream, every frame before the first one whose plain pose is not in front of the
    camera is `same` as the plain tracker's and TRACKING; that frame is LOST and repeats the previous poses (zero at frame 0).  A depth
    within `margin` of 0 is undecided and ends the stream's comparison.  -> the number of frames compared as equal."""
    n = 0
    for (p, s), (ph, sh, st) in zip(plain, lax):
        assert ph.shape == p.shape and sh.shape == s.shape and st.dtype == np.int32 and st.shape == (len(p),)
        for t in range(len(p)):
            z = depth(p[t], center)
            if abs(z) <= margin:
                break
            if z <= 0:
                assert st[t] == T.LOST, (t, z)
                np.testing.assert_array_equal(ph[t], ph[t - 1] if t else 0 * ph[t])
                np.testing.assert_array_equal(sh[t], sh[t - 1] if t else 0 * sh[t])
                break
            assert st[t] == T.TRACKING, (t, z)
            same(ph[t], p[t])
            same(sh[t], s[t])
            n += 1
    return n


@pytest.fixture
def patched(monkeypatch):
    ref_ops.patch_ops(monkeypatch)
    for name, fn in (("track_gather", np_track_gather), ("track_commit", np_track_commit), ("track_gate", np_track_gate),
                     ("track_health", np_track_health), ("track_verify", np_track_verify)):
        monkeypatch.setattr(ops, name, fn)


def _spy_full_path(monkeypatch, chain, who, log):
    """Record stream 0's push count of the tracker who[0] at every full-path (detection + selection) query_batch call, and the number of
    streams in the call."""
    orig = chain.query_batch

    def spy(imgs, Ks, pose_init=None, refine_iter=None):
        if pose_init is None:
            log.append((who[0]._frames[0], imgs.shape[0]))
        return orig(imgs, Ks, pose_init=pose_init, refine_iter=refine_iter)
    monkeypatch.setattr(chain, "query_batch", spy)


LAX_SEQS = [[2, 1, 2, 0], [2, 3], [3, 1, 0], [0]]               # scene frame per stream and tick


def test_lax_policy_changes_nothing(scene, patched):
    """Streams that stay in front of the camera (long-lens intrinsics; checked on the health-free tracker's poses): every frame
    array_equal to the tracker without health, every status TRACKING."""
    est, frames, Ks = scene
    seqs = [[frames[i] for i in q] for q in LAX_SEQS]
    KK = [long_lens(Ks[q[0]]) for q in LAX_SEQS]
    plain = T.track_streams(est, seqs, KK, batch=2, lanes=2, graphs=False)
    assert all(depth(x, est.ref_info["center"]) > 1e-3 for p, _ in plain for x in p)
    lax = T.track_streams(est, seqs, KK, batch=2, lanes=2, graphs=False, health=T.HealthPolicy.lax())
    for (p, s), (ph, sh, st) in zip(plain, lax):
        np.testing.assert_array_equal(ph, p)
        np.testing.assert_array_equal(sh, s)
        assert st.dtype == np.int32 and st.tolist() == [T.TRACKING] * len(p)


def test_lax_policy_keeps_the_hard_gates(scene, patched):
    """The scene's own intrinsics: where the health-free tracker puts the centre behind the camera the stream is LOST, equal before."""
    est, frames, Ks = scene
    seqs = [[frames[i] for i in q] for q in LAX_SEQS]
    KK = [Ks[2], None, Ks[3], Ks[0]]
    plain = T.track_streams(est, seqs, KK, batch=2, lanes=2, graphs=False)
    assert any(depth(x, est.ref_info["center"]) < 0 for p, _ in plain for x in p)
    lax = T.track_streams(est, seqs, KK, batch=2, lanes=2, graphs=False, health=T.HealthPolicy.lax())
    assert compare_with_plain(plain, lax, est.ref_info["center"], np.testing.assert_array_equal) >= 1
    assert any(T.LOST in st.tolist() for _, _, st in lax)


def test_forced_loss_and_reacquisition_schedule(scene, patched, monkeypatch):
    est, frames, Ks = scene
    chain = est.device_chain()
    # every tracked frame fails SHIFT: acquired at push 0, SUSPECT at 1, LOST at 2.  With lag 1 the host acts on tick 2 at push
    # 2 + lag = 3 and re-acquires there; the same again from push 3: 6, 9.
    tr = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, health=T.HealthPolicy.lax(max_shift=-1.0, patience=2, lag=1))
    log, who = [], [tr]
    _spy_full_path(monkeypatch, chain, who, log)
    seen = []
    first = chain.query(_it(frames[2]), _it(Ks[2]))["pose"]     # the reference: the acquisition and a step from it stay in front
    step = chain.query(_it(frames[2]), _it(Ks[2]), pose_init=first, refine_iter=1)["pose"]
    assert depth(first.numpy(), est.ref_info["center"]) > 3e-4 and depth(step.numpy(), est.ref_info["center"]) > 3e-4
    for k in range(10):
        tr.push([0], [frames[2]], [Ks[2]])
        row = tr.health_table[0].tolist()
        seen.append(row[0])
        if k in (1, 2):
            assert int(tr.hist_count[0]) == 1               # none of the bad frames was committed
            assert row[3] == T.SHIFT
    assert log == [(0, 1), (3, 1), (6, 1), (9, 1)]
    Tr, Su, Lo = T.TRACKING, T.SUSPECT, T.LOST
    assert seen == [Tr, Su, Lo] * 3 + [Tr]
    tr.push([0], [frames[2]], [Ks[2]])
    h = tr.health([0])[0]
    assert (h.status, h.bad, h.flags) == (Su, 1, T.SHIFT) and h.measures.shape == (12,) and h.measures[3] > 0
    np.testing.assert_allclose(tr.result([0])[0][0], first.numpy(), atol=2e-4)     # push 9 re-acquired; push 10 was not committed
    # an acquisition that fails is not committed and is tried again at every reacquire_every-th push of the stream
    tr = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, health=T.HealthPolicy.lax(min_px=1e9, reacquire_every=3, lag=1))
    log.clear()
    who[0] = tr
    for k in range(10):
        tr.push([0], [frames[2]], [Ks[2]])
        assert int(tr.hist_count[0]) == 0 and tr.health_table[0].tolist() == [Lo, 0, 0, T.SMALL]
    assert [p for p, _ in log] == [0, 3, 6, 9]
    assert not tr.result([0])[0][0].any()
    # reset clears the mirror entry and the next push starts over whatever the lag
    tr.health()
    assert tr._mirror.status[0, 0] == Lo
    tr.reset([0])
    assert tr._mirror.status[0, 0] == T.NONE
    tr.push([0], [frames[2]], [Ks[2]])
    assert log[-1][0] == 10
    # lag 2 (the default) acts one push later, lag 0 behaves as lag 1
    for lag, want in ((2, [0, 4, 8]), (0, [0, 3, 6, 9])):
        tr = T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, health=T.HealthPolicy.lax(max_shift=-1.0, patience=2, lag=lag))
        log.clear()
        who[0] = tr
        for k in range(10):
            tr.push([0], [frames[2]], [Ks[2]])
        assert [p for p, _ in log] == want, lag


def test_nan_row_is_parked(scene, patched, monkeypatch):
    est, frames, Ks = scene

    def run(poison):
        tr = T.StreamTracker(est, 3, batch=4, lanes=1, graphs=False, health=T.HealthPolicy.lax())
        src = [3, 3, 2]                                        # (scene frames whose first poses stay in front of the camera)
        for k in range(2):
            tr.push([0, 1, 2], [frames[i] for i in src], [Ks[i] for i in src])
        if poison:
            assert tr.health([1])[1].status == T.TRACKING
            tr.pose_table[1, 6] = float("nan")
        tr.push([0, 1, 2], [frames[i] for i in src], [Ks[i] for i in src])
        return tr
    finite = []
    orig = est.refiner._step

    def step(*a, **k):
        finite.append(all(bool(torch.isfinite(t).all()) for t in a if torch.is_tensor(t)))
        return orig(*a, **k)
    monkeypatch.setattr(est.refiner, "_step", step)
    clean, bad = run(False), run(True)
    assert finite and all(finite)                              # nothing non-finite reached the refiner
    hb = bad.health()
    assert hb[1].status == T.LOST and hb[1].flags == T.NONFINITE and int(bad.hist_count[1]) == 2
    hc = clean.health()
    assert hb[0][:4] == hc[0][:4] and hb[2][:4] == hc[2][:4] and hc[1].status != T.LOST
    np.testing.assert_array_equal(bad.hist_count[[0, 2]].numpy(), clean.hist_count[[0, 2]].numpy())
    rc, rb = clean.result(), bad.result()                      # result() does not raise; the lane's other streams are unchanged
    for s in (0, 2):
        np.testing.assert_array_equal(rb[s][0], rc[s][0])
        np.testing.assert_array_equal(rb[s][1], rc[s][1])
    assert np.isnan(rb[1][0]).sum() == 1                       # the row itself is left for the re-acquisition to overwrite
    bad.push([1], [frames[3]], [Ks[3]])                        # the host has just read the status: the next push re-acquires
    assert bad.health([1])[1].status == T.TRACKING and np.isfinite(bad.result([1])[1][0]).all()


def test_track_streams_reports_status_and_repeats_poses(scene, patched):
    est, frames, Ks = scene
    pol = T.HealthPolicy.lax(max_shift=-1.0, patience=2, lag=1)
    seqs = [[frames[2]] * 6, [frames[2]] * 2]                  # (a frame whose acquisition and the step from it stay in front)
    res = T.track_streams(est, seqs, [Ks[2], Ks[2]], batch=2, lanes=1, graphs=False, health=pol)
    chain = est.device_chain()
    Tr, Su, Lo = T.TRACKING, T.SUSPECT, T.LOST
    p, s, st = res[0]
    assert st.tolist() == [Tr, Su, Lo, Tr, Su, Lo] and res[1][2].tolist() == [Tr, Su]
    both = chain.query_batch(torch.stack([_it(frames[2])] * 2), torch.stack([_it(Ks[2])] * 2))["pose"].numpy()
    np.testing.assert_allclose(p[0], both[0], atol=2e-4)       # the two streams share their first query_batch
    np.testing.assert_allclose(p[3], chain.query(_it(frames[2]), _it(Ks[2]))["pose"].numpy(), atol=2e-4)     # re-acquired alone at frame 3
    for t, t0 in ((1, 0), (2, 0), (4, 3), (5, 3)):
        np.testing.assert_array_equal(p[t], p[t0])
        np.testing.assert_array_equal(s[t], s[t0])
    assert p[0].any() and s[3].any()
    # all zero before the first commit
    (p, s, st), = T.track_streams(est, [seqs[1]], [Ks[2]], batch=2, graphs=False, health=T.HealthPolicy.lax(min_px=1e9))
    assert st.tolist() == [Lo, Lo] and not p.any() and not s.any()


def test_argument_errors(scene, patched):
    est, frames, Ks = scene
    for kw in ({"patience": 0}, {"verify_patience": 0}, {"reacquire_every": 0}, {"lag": -1}, {"verify_every": -1}, {"patience": 1.5},
               {"min_px": float("nan")}, {"patience": float("inf")}, {"lag": "2"}, {"lag": True}, {"max_shift": "1"}, {"margin": None}):
        with pytest.raises(ValueError):
            T.HealthPolicy(**kw)
    lax = T.HealthPolicy.lax()
    assert all(getattr(lax, n) in (INF, -INF) for n in GATE_FIELDS + ("verify_shift", "verify_log2_scale")) and lax.patience == 3
    d = T.HealthPolicy()
    assert (d.patience, d.min_px, d.max_px, d.margin, d.max_rot_deg, d.max_shift, d.max_log2_scale, d.verify_every, d.verify_shift,
            d.verify_log2_scale, d.verify_patience, d.reacquire_every, d.lag) == (3, 8.0, 4.0, 0.5, 45.0, 1.0, 1.0, 0, 1.0, 1.5, 2, 1, 2)
    with pytest.raises(ValueError):
        T.StreamTracker(est, 2, batch=2, graphs=False, health={"patience": 3})
    with pytest.raises(ValueError):
        T.StreamTracker(est, 2, batch=2, graphs=False).health()
    tr = T.StreamTracker(est, 2, batch=2, graphs=False, health=lax)
    with pytest.raises(ValueError):
        tr.health([2])
    assert tr.health() == {}


def test_ops_refuse_host_tensors_and_bad_arguments():
    """The product ops have no CPU path, and the C entry points reject null and out-of-range arguments before any HIP call."""
    z = lambda *sh, dt=torch.float32: torch.zeros(sh, dtype=dt)
    m = z(2, dt=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.track_gate(z(3, 12), z(3, 4, dt=torch.int32), m)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.track_health(z(2, 12), z(2, 12), z(2, 9), None, (8, 8), m, False, z(3), 1.0, T.HealthPolicy(), z(3, 4, dt=torch.int32), z(3, 12))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.track_verify(z(2, 5), z(3, 12), z(2, 9), m, z(3), 1.0, 100.0, T.HealthPolicy(), z(3, 4, dt=torch.int32), z(3, 12))
    l = lib.load()
    a = C.c_void_p(64)                                          # never dereferenced: the checks come first
    assert l.g6d_track_gate(None, a, a, a, 1, None) == -1 and l.g6d_track_gate(a, a, a, a, 0, None) == -1
    g = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    assert l.g6d_track_health(None, a, a, a, 0, 0, a, 0, a, 1.0, 1, *g, a, a, a, a, 1, None) == -1        # no pose_prev without reset
    assert l.g6d_track_health(a, a, a, None, 0, 8, a, 0, a, 1.0, 1, *g, a, a, a, a, 1, None) == -1         # neither pic nor W, H
    assert l.g6d_track_health(a, a, a, a, 0, 0, a, 0, a, 1.0, 0, *g, a, a, a, a, 1, None) == -1            # patience
    assert l.g6d_track_health(a, a, a, a, 0, 0, a, 0, a, 0.0, 1, *g, a, a, a, a, 1, None) == -1            # diameter
    assert l.g6d_track_verify(a, a, a, a, a, 1.0, 0.0, 1.0, 1.0, 1, a, a, 1, None) == -1                   # ref_px
    assert l.g6d_track_verify(a, a, a, a, a, 1.0, 1.0, 1.0, 1.0, 0, a, a, 1, None) == -1                   # verify_patience


# ---------------------------------------------------------------------------------------------------------------- no scratch
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_have_no_scratch(tmp_path):
    """Latency-class kernels with the poses in registers: no scratch and no spills.  Compiler metadata; cross-compiles without a GPU."""
    out = tmp_path / "track_health.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(ROOT, "gen6d_amd", "csrc", "track_health.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = out.read_text().split("\n  - .agpr_count")                     # one metadata block per kernel
    for kernel in ("track_gate_kernel", "track_health_kernel", "track_verify_kernel"):
        body, = [b for b in blocks[1:] if re.search(r"\.name:\s+\S*" + kernel, b)]
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", body).group(1))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, kernel
