"""g6d_frame_ingest on the MI355X against the numpy restatement of its integer specification (tests/test_ingest_cpu.py), bit for bit:
every format and rotation, several ratios, pitched sources, host- and device-resident planes, one launch of 32 mixed frames into
scattered slots; the tracker with `frame_size` on camera-native frames (graphs and eager ticks) and that its push does not synchronise."""
import numpy as np
import pytest
import torch

from gen6d_amd import eval as EV
from gen6d_amd import ingest as I
from gen6d_amd import tracking as T
from test_ingest_cpu import np_ingest, nv12_of, pitched, rgb_to
from test_track_streams_gpu import _check_one_step, _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

FORMATS = ("rgb24", "bgr24", "rgba32", "bgra32", "nv12")


def make_frame(rng, h, w, fmt, rotate=0, extra=0, device=False, K=None, matrix="bt601", split=False):
    """A random picture of the format as a Frame: `extra` bytes of row padding (255s); planes in host numpy arrays, device tensors
    (device=True) or pinned host tensors (device="pinned"); nv12 as one buffer or (split) as two planes."""
    mv = {False: lambda a: a, True: lambda a: torch.from_numpy(a).cuda(), "pinned": lambda a: torch.from_numpy(a).pin_memory()}[device]
    if fmt == "nv12":
        buf = np.full((h * 3 // 2, w + extra), 255, np.uint8)
        buf[:, :w] = rng.randint(0, 256, (h * 3 // 2, w))
        if split:
            return I.Frame(mv(np.ascontiguousarray(buf[:h])), fmt, width=w, uv=mv(np.ascontiguousarray(buf[h:])), rotate=rotate, K=K, matrix=matrix)
        return I.Frame(mv(buf), fmt, width=w, rotate=rotate, K=K, matrix=matrix)
    src = rgb_to(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), fmt, rng)
    if extra:
        return I.Frame(mv(pitched(src, extra)), fmt, width=w, rotate=rotate, K=K)
    return I.Frame(mv(src), fmt, rotate=rotate, K=K)


def run(frames, H, W, B=None, slots=None, fill=0):
    B = len(frames) if B is None else B
    out = torch.full((B, H, W, 3), fill, dtype=torch.uint8, device="cuda")
    K = torch.full((B, 3, 3), -7.0, device="cuda")
    I.ingest_frames(frames, out, K, slots=slots)
    return out.cpu().numpy(), K.cpu().numpy()


def expect_K(frame, H, W):
    return np.asarray(I.plan(frame, (H, W))[2], np.float64).astype(np.float32)


def test_every_format_and_rotation_matches_numpy():
    rng = np.random.RandomState(0)
    for canvas in ((96, 128), (50, 67)):                # dword-aligned canvas rows and the byte-store path
        frames = []
        for fmt in FORMATS:
            for rot in (0, 90, 180, 270):
                K = np.array([[900.0, 0, 150], [0, 905.0, 110], [0, 0, 1]]) if rot == 90 else None
                frames.append(make_frame(rng, 2 * rng.randint(60, 140), 2 * rng.randint(60, 140), fmt, rot, extra=int(rng.randint(0, 3)) * 7,
                                         device=(False, True, "pinned")[rng.randint(0, 3)], K=K, matrix=("bt601", "bt709")[rot == 180], split=rot == 270))
        got, Ks = run(frames, *canvas)
        for i, f in enumerate(frames):
            np.testing.assert_array_equal(got[i], np_ingest(f, *canvas), err_msg=f"{canvas} {f.fmt} rotate {f.rotate}")
            np.testing.assert_array_equal(Ks[i], expect_K(f, *canvas))


@pytest.mark.parametrize("src_hw", [(960, 1280), (1297, 1733), (480, 640), (185, 246), (487, 651), (120, 160)])
@pytest.mark.parametrize("fmt", ["bgr24", "nv12"])
def test_ratios_match_numpy(src_hw, fmt):
    rng = np.random.RandomState(1)
    h, w = src_hw if fmt != "nv12" else (src_hw[0] & ~1, src_hw[1] & ~1)
    host, dev = make_frame(rng, h, w, fmt, extra=5), make_frame(rng, h, w, fmt, device=True)
    got, _ = run([host, dev], 480, 640)
    np.testing.assert_array_equal(got[0], np_ingest(host, 480, 640))
    np.testing.assert_array_equal(got[1], np_ingest(dev, 480, 640))


def test_32_mixed_frames_into_scattered_slots():
    rng = np.random.RandomState(2)
    H, W, B = 96, 128, 40
    frames = [make_frame(rng, 2 * rng.randint(20, 160), 2 * rng.randint(20, 160), FORMATS[rng.randint(0, 5)], 90 * int(rng.randint(0, 4)),
                         extra=int(rng.randint(0, 2)) * 11, device=(False, True, "pinned")[rng.randint(0, 3)], matrix=("bt601", "bt709")[rng.randint(0, 2)],
                         K=None if rng.randint(0, 2) else np.array([[700.0, 0, 99], [0, 700.0, 77], [0, 0, 1]])) for _ in range(32)]
    slots = [int(s) for s in rng.permutation(B)[:32]]
    got, Ks = run(frames, H, W, B=B, slots=slots, fill=77)
    for f, s in zip(frames, slots):
        np.testing.assert_array_equal(got[s], np_ingest(f, H, W), err_msg=f"slot {s}: {f.fmt} {f.width}x{f.height} rotate {f.rotate}")
        np.testing.assert_array_equal(Ks[s], expect_K(f, H, W))
    for s in set(range(B)) - set(slots):
        assert (got[s] == 77).all() and (Ks[s] == -7.0).all(), f"slot {s} was touched"


def test_full_hd_nv12():
    rng = np.random.RandomState(3)
    assert I.canvas_for(960, 1080, 1920) == (540, 960)
    f = make_frame(rng, 1080, 1920, "nv12", extra=128, matrix="bt709")
    got, Ks = run([f], 540, 960)
    np.testing.assert_array_equal(got[0], np_ingest(f, 540, 960))
    np.testing.assert_array_equal(Ks[0], EV.pseudo_K(540, 960))


def _native(frame, kind):
    """A scene frame [h,w,3] -> a 2x larger camera-style Frame of the same picture, built on the host."""
    big = np.repeat(np.repeat(frame, 2, 0), 2, 1)
    h, w = big.shape[:2]
    if kind == "bgra":
        return I.Frame(pitched(rgb_to(big, "bgra32"), 24), "bgra32", width=w)
    g = frame.astype(np.int64)                          # BT.601 limited range, one chroma sample per original pixel = per 2x2 block
    Y = ((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16
    U = ((-38 * g[..., 0] - 74 * g[..., 1] + 112 * g[..., 2] + 128) >> 8) + 128
    V = ((112 * g[..., 0] - 94 * g[..., 1] - 18 * g[..., 2] + 128) >> 8) + 128
    Yb = np.repeat(np.repeat(Y, 2, 0), 2, 1)
    return I.Frame(nv12_of(Yb.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8), pitch=w + 32), "nv12", width=w)


@pytest.mark.parametrize("graphs", [True, False])
def test_tracker_on_native_frames(scene, graphs):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    assert (H, W) == (96, 128)
    S, batch = 4, 2                                      # two groups, one per lane: a lane's slots hold one group's frames after a push
    seqs = _seqs(frames, S, 4)
    native = [[_native(f, ("nv12", "bgra")[(s + t) % 2]) for t, f in enumerate(q)] for s, q in enumerate(seqs)]
    ingested = [[np_ingest(f, H, W) for f in q] for q in native]
    np.testing.assert_array_equal(ingested[0][1], seqs[0][1])        # BGRA at exactly 2x: the mean of four equal taps is the scene's frame
    tr = T.StreamTracker(est, S, batch=batch, lanes=2, graphs=graphs, frame_size=(H, W))
    tr._records = []
    for t in range(4):
        ids = [s for s in range(S) if t < len(seqs[s])]
        tr.push(ids, [native[s][t] for s in ids])
        if t:                                            # tracked frames sit in the lanes' static slots, bit for bit the numpy ingest
            for s in ids:
                lane = tr._lanes[(s // batch) % 2]
                np.testing.assert_array_equal(lane.img[s % batch].cpu().numpy(), ingested[s][t], err_msg=f"stream {s} frame {t}")
                np.testing.assert_array_equal(lane.K[s % batch].cpu().numpy(), EV.pseudo_K(H, W))
    res = tr._collect([len(q) for q in seqs])
    tr._check_range()
    Kseq = [[EV.pseudo_K(H, W)] * len(q) for q in seqs]
    _check_one_step(est.device_chain(), ingested, Kseq, res)
    again = T.track_streams(est, native, batch=batch, lanes=2, graphs=graphs, frame_size=(H, W))
    for (p, s), (ap, as_) in zip(res, again):
        np.testing.assert_allclose(ap, p, atol=3e-4)
        np.testing.assert_allclose(as_, s, atol=3e-4)


def test_push_with_frame_size_does_not_synchronise(scene, monkeypatch):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    seqs = _seqs(frames, 3, 4, seed=1)
    native = [[_native(f, ("nv12", "bgra")[(s + t) % 2]) for t, f in enumerate(q)] for s, q in enumerate(seqs)]
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
    res = T.track_streams(est, native, batch=2, lanes=2, frame_size=(H, W))
    assert len(at_push) == 4 and at_push[-1] == 0, at_push
    assert counts["n"] > 0 and all(np.isfinite(p).all() for p, _ in res)
