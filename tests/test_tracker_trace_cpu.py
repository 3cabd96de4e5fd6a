"""The launch schedule of gen6d_amd.tracking.StreamTracker, pinned: which op runs when, on which shapes and with which slot maps.  The
eager tracker runs on the patched ops (tests/ref_ops.py and the numpy stand-ins of the track, ingest and emit ops) with a recorder round
every `ops.track_*`, `ingest.ingest_frames`, `emit.emit_frames` and the chain's `query_batch` / `detect_batch`; the whole trace of each
configuration equals tests/golden/tracker_trace.json, which tests/golden/make_golden_tracker_trace.py wrote with this file's recorder
before the tracker's host class was restructured.  The configurations are chosen so that every recorded integer follows from the policy
and the schedule and none from float rounding: behind long-lens intrinsics and lax gates every frame passes (asserted), with
max_shift = -1 every tracked frame fails."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import ref_ops
from gen6d_amd import emit as E
from gen6d_amd import ingest as I
from gen6d_amd import ops
from gen6d_amd import tracking as T
from test_emit_cpu import np_frame_emit, np_track_corners
from test_ingest_cpu import np_frame_ingest
from test_track_health_cpu import LAX_SEQS, long_lens, np_track_gate, np_track_health, np_track_verify
from test_track_streams_cpu import np_track_commit, np_track_gather, scene  # noqa: F401  (scene: the module's fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracker_trace.json")
STANDINS = {"track_gather": np_track_gather, "track_commit": np_track_commit, "track_gate": np_track_gate, "track_health": np_track_health,
            "track_verify": np_track_verify, "track_corners": np_track_corners, "frame_ingest": np_frame_ingest, "frame_emit": np_frame_emit}
KW = dict(batch=2, lanes=2, graphs=False)


def describe(v, contents=False):
    """A call's argument as JSON: a tensor's shape (and the contents of a slot map or of the picture sizes), flags, counts and names as
    they are, lists element-wise, anything else (floats, policies, frames, sinks) by its type's name."""
    if torch.is_tensor(v):
        return {"shape": list(v.shape), "map": v.tolist()} if contents else {"shape": list(v.shape)}
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (list, tuple)):
        return [describe(x, contents) for x in v]
    return type(v).__name__


def install(mp, est):
    """Patch the stand-ins in and wrap every launch of the tracker -> the list that receives [name, {parameter: description}, maps the
    op returned] per call.  A call is described after it ran, so the slot maps it wrote are in."""
    ref_ops.patch_ops(mp)
    for name, fn in STANDINS.items():
        mp.setattr(ops, name, fn)
    trace, chain = [], est.device_chain()

    def wrap(owner, name):
        fn = getattr(owner, name)
        sig = inspect.signature(fn)

        def recorded(*a, **kw):
            out = fn(*a, **kw)
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()                             # the call as the op sees it, however its arguments were passed
            args = {k: describe(v, k.startswith("slot_") or k == "pic") for k, v in bound.arguments.items()}
            trace.append([name, args, describe(out, True) if name in ("track_gate", "track_health") else None])
            return out
        mp.setattr(owner, name, recorded)
    for owner, name in [(ops, n) for n in sorted(vars(ops)) if n.startswith("track_")] + [(I, "ingest_frames"), (E, "emit_frames"),
                                                                                          (chain, "query_batch"), (chain, "detect_batch")]:
        wrap(owner, name)
    return trace


def _native(f, kind, K):
    """A scene frame as a camera-native one: as it is, or twice the size and only its left half (a picture half the canvas wide) or its
    top half (half the canvas high)."""
    h, w = f.shape[:2]
    f = (f, f[:, :w // 2], f[:h // 2])[kind]
    return I.Frame(np.ascontiguousarray(np.repeat(np.repeat(f, 2, 0), 2, 1) if kind else f), K=K)


def _seqs(frames, Ks, native=False):
    """The health tests' stream lengths -> (frames per stream, long-lens intrinsics per stream; with `native` they travel in the frames)."""
    if native:
        return [[_native(frames[i], (s + t) % 3, long_lens(Ks[i])) for t, i in enumerate(q)] for s, q in enumerate(LAX_SEQS)], None
    return [[frames[i] for i in q] for q in LAX_SEQS], [long_lens(Ks[q[0]]) for q in LAX_SEQS]


def _drive(est, seqs, Ks, hw, **kw):
    """track_streams' pushes on a tracker, with one sink per stream and push and a second, raw one on stream 0 -> the tracker."""
    tr = T.StreamTracker(est, len(seqs), **KW, **kw)
    sink = lambda **k: E.Sink(torch.zeros(tuple(hw) + (3,), dtype=torch.uint8), "rgb24", **k)
    for t in range(max(len(q) for q in seqs)):
        ids = [s for s, q in enumerate(seqs) if t < len(q)]
        tr.push(ids, [seqs[s][t] for s in ids], None if Ks is None else [Ks[s] for s in ids],
                sinks=[[sink()] + ([sink(pose="raw")] if s == 0 else []) for s in ids])
    return tr


def _all_tracking(res):
    assert all(st.tolist() == [T.TRACKING] * len(st) for _, _, st in res)


def plain(est, frames, Ks):
    T.track_streams(est, *_seqs(frames, Ks), **KW)


def frame_size(est, frames, Ks):
    T.track_streams(est, _seqs(frames, Ks, True)[0], frame_size=frames[0].shape[:2], **KW)


def sinks(est, frames, Ks):
    _drive(est, *_seqs(frames, Ks), frames[0].shape[:2])


def verify(est, frames, Ks):
    _all_tracking(T.track_streams(est, *_seqs(frames, Ks), health=T.HealthPolicy.lax(verify_every=2), **KW))


def forced_loss(est, frames, Ks):
    tr = T.StreamTracker(est, 2, health=T.HealthPolicy.lax(max_shift=-1.0, patience=2, lag=1), **KW)
    seen = []
    for k in range(11):
        if k == 10:
            tr.reset([0])
        tr.push([0], [frames[2]], [Ks[2]])
        seen.append(int(tr.health_table[0, 0]))
    assert seen == [T.TRACKING, T.SUSPECT, T.LOST] * 3 + [T.TRACKING] * 2


def everything(est, frames, Ks):
    """Beyond the five single features: native frames, sinks and a checking policy together, where the three uses of a frame's picture
    size meet."""
    hw = frames[0].shape[:2]
    tr = _drive(est, *_seqs(frames, Ks, True), hw, frame_size=hw, health=T.HealthPolicy.lax(verify_every=2))
    assert all(h.status == T.TRACKING for h in tr.health().values())


CONFIGS = {f.__name__: f for f in (plain, frame_size, sinks, verify, forced_loss, everything)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_schedule(scene, monkeypatch, name):
    est, frames, Ks = scene
    trace = install(monkeypatch, est)
    CONFIGS[name](est, frames, Ks)
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = json.loads(json.dumps(trace))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs"
    assert len(got) == len(want)
