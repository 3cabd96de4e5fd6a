"""The tracking algebra of gen6d_amd/csrc/pose_algebra.h (box projection, predict.py's weighted corner mean, PnP by Levenberg-Marquardt),
built for the host and checked against the numpy versions in gen6d_amd/geometry.py, which the eager tracker and the tests use as the
oracle.  No GPU needed: the header is plain C++ in float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gen6d_amd import geometry as G
from gen6d_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ta(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ta") / "track_algebra.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "track_algebra_shim.cpp"), "-o", so],
                   check=True)
    return C.CDLL(so)


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(D)


def _project(ta, box, pose, K):
    keep = [_d(box), _d(pose), _d(K)]
    uv = np.zeros((8, 2))
    ta.t_box_project(*[k[1] for k in keep], uv.ctypes.data_as(D))
    return uv


def _weighted(ta, frames, num, std):
    f, pf = _d(frames)
    out = np.zeros((8, 2))
    ta.t_weighted(pf, len(frames), num, C.c_double(std), out.ctypes.data_as(D))
    return out


def _pnp(ta, box, uv, K, init):
    keep = [_d(box), _d(uv), _d(K), _d(init)]
    out = np.zeros((3, 4))
    it = ta.t_pnp(*[k[1] for k in keep], out.ctypes.data_as(D))
    return out, it


def _grad(ta, box, uv, K, pose):
    keep = [_d(box), _d(uv), _d(K), _d(pose)]
    acc = np.zeros(28)
    ta.t_pnp_sums(*[k[1] for k in keep], acc.ctypes.data_as(D))
    return acc[21:27], acc[27]


def _scene(seed=0, n=6):
    """Camera poses around an object box of the synthetic database's scale, with their intrinsics."""
    rng = np.random.RandomState(seed)
    poses, Ks = synth.fibonacci_cameras(n, radius=3.0, focal=400.0, size=320)
    pts = rng.uniform(-0.4, 0.4, (200, 3)) * np.array([1.0, 0.7, 0.5])
    poses = np.stack([np.concatenate([G.rodrigues(G.rotation_log(q[:, :3])), q[:, 3:]], 1) for q in poses.astype(np.float64)])  # exact rotations
    return G.box_corners(pts), poses, Ks.astype(np.float64), rng


def test_box_corners_order():
    pts = np.array([[0.0, 1.0, -2.0], [3.0, -1.0, 5.0], [1.0, 0.0, 0.0]])
    b = G.box_corners(pts)
    np.testing.assert_array_equal(b[0], [0, -1, -2])
    np.testing.assert_array_equal(b[1], [0, 1, -2])
    np.testing.assert_array_equal(b[2], [3, 1, -2])
    np.testing.assert_array_equal(b[3], [3, -1, -2])
    np.testing.assert_array_equal(b[4:, 2], [5, 5, 5, 5])
    np.testing.assert_array_equal(b[4:, :2], b[:4, :2])


def test_projection_matches_geometry(ta):
    box, poses, Ks, _ = _scene()
    for p, K in zip(poses, Ks):
        np.testing.assert_allclose(_project(ta, box, p, K), G.project_points(box, p, K)[0], rtol=0, atol=1e-12)
    # the depth clamp of geometry.project_points: a corner 5e-5 in front of the camera divides by 1e-4
    p = np.concatenate([np.eye(3), [[0.0], [0.0], [0.0]]], 1)
    K = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1]])
    box2 = box.copy()
    box2[3] = [0.01, -0.02, 5e-5]
    uv = _project(ta, box2, p, K)
    np.testing.assert_allclose(uv, G.project_points(box2, p, K)[0], rtol=1e-14, atol=1e-12)
    np.testing.assert_allclose(uv[3], [(100 * 0.01 + 50 * 5e-5) / 1e-4, (100 * -0.02 + 40 * 5e-5) / 1e-4], rtol=1e-14)


@pytest.mark.parametrize("n", range(1, 8))
def test_weighted_mean_matches_predict(ta, n):
    rng = np.random.RandomState(n)
    frames = rng.uniform(0, 640, (n, 8, 2))
    num, std = 5, 2.5
    # predict.py weighted_pts, the weights written out: newest 1, i steps older exp(-(i/std)^2), last `num` frames only
    m = min(n, num)
    w = np.array([np.exp(-((m - 1 - k) / std) ** 2) for k in range(m)])
    expect = np.sum(frames[n - m:] * w[:, None, None], 0) / w.sum()
    np.testing.assert_allclose(G.weighted_points(list(frames), num, std), expect, rtol=0, atol=1e-12)
    np.testing.assert_allclose(_weighted(ta, frames, num, std), expect, rtol=0, atol=1e-12)
    np.testing.assert_allclose(_weighted(ta, frames, 3, 1.0), G.weighted_points(list(frames), 3, 1.0), rtol=0, atol=1e-12)
    if n == 1:
        np.testing.assert_array_equal(_weighted(ta, frames, num, std), frames[0])


def test_rodrigues_round_trip(ta):
    rng = np.random.RandomState(3)
    for th in [0.0, 1e-9, 1e-3, 0.5, 2.0, np.pi - 1e-6, np.pi]:
        a = rng.randn(3)
        r = a / np.linalg.norm(a) * th
        R = G.rodrigues(r)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
        np.testing.assert_allclose(G.rodrigues(G.rotation_log(R)), R, atol=1e-12)
        Rh = np.zeros(9); lr = np.zeros(3)
        ta.t_rodrigues(_d(r)[1], Rh.ctypes.data_as(D))
        np.testing.assert_allclose(Rh.reshape(3, 3), R, atol=1e-15)
        ta.t_rot_log(_d(R)[1], lr.ctypes.data_as(D))
        np.testing.assert_allclose(lr, G.rotation_log(R), atol=1e-12)
        if th < 3:
            np.testing.assert_allclose(lr, r, atol=1e-9)


def test_pnp_noise_free_recovers_pose(ta):
    box, poses, Ks, rng = _scene(1)
    for p, K in zip(poses, Ks):
        uv = G.project_points(box, p, K)[0]
        init = synth.perturb_pose(p, 3.0, 0.03).astype(np.float64)
        got, it = _pnp(ta, box, uv, K, init)
        assert 1 <= it <= 20
        np.testing.assert_allclose(got, p, rtol=0, atol=1e-9)
        np.testing.assert_allclose(G.pnp(box, uv, K, init), p, rtol=0, atol=1e-9)


def test_pnp_noisy_is_a_minimum_and_matches_numpy(ta):
    box, poses, Ks, rng = _scene(2)
    for p, K in zip(poses, Ks):
        uv = G.project_points(box, p, K)[0] + rng.randn(8, 2) * 1.5
        init = synth.perturb_pose(p, 2.0, 0.02).astype(np.float64)
        got, _ = _pnp(ta, box, uv, K, init)
        np.testing.assert_allclose(got, G.pnp(box, uv, K, init), rtol=0, atol=1e-9)
        np.testing.assert_allclose(got[:, :3] @ got[:, :3].T, np.eye(3), atol=1e-12)
        g, err = _grad(ta, box, uv, K, got)
        _, g_np, err_np = G.pnp_normal_equations(box, uv, K, np.concatenate([G.rotation_log(got[:, :3]), got[:, 3]]))
        np.testing.assert_allclose(g, g_np, rtol=1e-9, atol=1e-9)
        assert np.abs(g).max() <= 1e-6 * max(1.0, err), (g, err)
        x = np.concatenate([G.rotation_log(got[:, :3]), got[:, 3]])
        for _ in range(100):
            xp = x + rng.randn(6) * np.r_[1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3] * rng.uniform(0.01, 1)
            assert G.pnp_normal_equations(box, uv, K, xp)[2] >= err - 1e-9 * err


def test_pnp_from_refined_float32_pose(ta):
    """The kernel starts from a float32 refined pose whose rotation is orthogonal to ~1e-7 only."""
    box, poses, Ks, rng = _scene(4)
    for p, K in zip(poses, Ks):
        uv = G.project_points(box, p, K)[0] + rng.randn(8, 2) * 0.5
        init = synth.perturb_pose(p, 2.0, 0.02).astype(np.float32).astype(np.float64)
        np.testing.assert_allclose(_pnp(ta, box, uv, K, init)[0], G.pnp(box, uv, K, init), rtol=0, atol=1e-9)


def test_pnp_matches_cv2(ta):
    cv2 = pytest.importorskip("cv2")
    box, poses, Ks, rng = _scene(5)
    for p, K in zip(poses, Ks):
        uv = G.project_points(box, p, K)[0] + rng.randn(8, 2) * 0.5
        ok, rv, tv = cv2.solvePnP(box, uv, K, np.zeros((8, 1)), flags=cv2.SOLVEPNP_ITERATIVE)
        assert ok
        ref = np.concatenate([cv2.Rodrigues(rv)[0], tv.reshape(3, 1)], 1)
        got, _ = _pnp(ta, box, uv, K, synth.perturb_pose(p, 0.02, 0.02).astype(np.float64))
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
