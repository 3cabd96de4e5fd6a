"""Batched multi-stream tracking (reference predict.py:49-72) on the device-resident chain.

The reference's video loop runs the full pipeline on the first frame and one refinement step from the previous pose on every later
frame, then smooths the result for display: the object's 3-D box is projected under each pose, the corners of the last frames are
averaged with Gaussian weights (weighted_pts) and a pose is solved back from them (cv2.solvePnP).  `StreamTracker` runs that loop for
many streams (cameras or clients watching one object) at once:

  * stream s sits in slot s % batch of group s // batch; the group runs on lane (s // batch) % lanes, one HIP stream per lane, so a
    stream's consecutive frames are ordered by its lane's stream with no events;
  * a stream's first frame (after creation or `reset`) goes through detection, selection and cfg['refine_iter'] steps in
    `DeviceChain.query_batch` (chunks of <= 8 queries) and is committed with its history restarted; every later frame is one of the
    group's slots in a tick: gather (previous raw pose per slot) -> `track_iter` refinement steps -> commit (csrc/pose_chain.hip);
  * each lane has one captured hipGraph of the tick (captured lazily, after warm-up runs on an all-unused slot map) with static image,
    K and slot-map buffers that are filled on the lane's stream before each replay; unused slots (id -1) refine the parking pose
    (DeviceChain.ref_poses[0]) and are not committed;
  * per-stream state is device-resident: last raw and smoothed pose, and the ring of the last `smooth_num` frames' box corners;
  * with `frame_size=(H, W)` the tracker takes camera-native frames (`gen6d_amd.ingest.Frame`: any size, any of its eleven pixel formats,
    pitched, rotated, with or without a calibrated `ingest.Lens`, mixed within one push): one g6d_frame_ingest launch per lane and tick
    (g6d_frame_ingest_mesh when a frame has a lens: it is undistorted on the way) scales them into the lane's static image
    slots and writes their intrinsics, in place of the per-slot copies;
  * with `sinks` a push also writes what predict.py writes per frame: the working-resolution picture with the projected box drawn on it
    (raw and / or smoothed pose), in an encoder's or a display's format, into device or pinned host buffers the caller names
    (`gen6d_amd.emit.Sink`).  After the lane's tick (or the commit of an init chunk) the corners are projected on the device and ONE
    g6d_frame_emit launch per lane and tick fills that lane's sinks, stream-ordered on the lane's stream, outside the captured graph
    (DESIGN.md §4.18).  A tracker used without sinks launches nothing of this.  A sink with view="source" receives the camera's own
    frame (full resolution, not turned) with the box drawn in its pixel grid instead: the lane's ingest keeps its frame table on the
    device, the corners are projected once more under the sources' intrinsics and ONE g6d_frame_emit_source launch per lane and tick
    fills those sinks.  A push without source-view sinks launches nothing of this;
  * with `crops="source"` (needs `frame_size`) the networks' query crops, the refiner's look-at crop of every step and the selector's
    crop of a first frame, are cut from the camera-native pictures instead of the working-resolution canvas: the lane's ingest keeps
    its frame table, the tick copies it into a static table beside a slot -> record map, and ONE g6d_frame_crop launch stands where
    each of those warp launches stood, inside the tick's graph.  Frames with a lens keep their canvas crops.  The
    default `crops="canvas"` launches what it always launched;
  * with `minify="area"` (needs `frame_size`) what shrinks is filtered instead of point-sampled: the tick's and the
    first frames' ingest is g6d_frame_ingest_area (an exact-integer box filter on every axis that shrinks; frames with a lens keep the
    mesh rule unless the lens is Lens(minify="area"): n x n sub-samples per canvas pixel through the mesh), and with `crops="source"` the crops are g6d_frame_crop_area (n x n samples per crop pixel, n per slot from the crop's
    own footprint, at most 8), in the same places of the same graph; with `crops="canvas"` the crops stay g6d_warp_batch.  The default
    `minify="point"` launches what it always launched;
  * with `health=HealthPolicy(...)` every stream carries a status (TRACKING / SUSPECT / LOST) that the device keeps: a gate parks lost
    streams and non-finite table rows before the gather, a health launch judges every refined pose before the commit (a bad frame is
    not committed), the detector can check the committed poses every n-th tick, and the host, which sees the status with a fixed lag,
    sends lost streams through the acquisition path again.  A tracker without a policy launches nothing of this.

`track_streams` is the one-call form for whole sequences, with one synchronisation at the end and the networks' fp16 pair range guard.
"""
import collections
import contextlib
import dataclasses
import math

import numpy as np
import torch

from . import emit as E
from . import eval as EV
from . import geometry as G
from . import ingest as I
from . import ops
from .network import refiner as _refiner

INIT_CHUNK = 8          # first frames per query_batch call: the batch size query_batch's detection + selection path is tested at


# health[s] = (status, bad, vbad, flags), include/gen6d_hip.h
NONE, TRACKING, SUSPECT, LOST = 0, 1, 2, 3
NONFINITE, BEHIND, SMALL, LARGE, OUTSIDE, ROT, SHIFT, SCALE, VERIFY_POS, VERIFY_SCALE = (1 << i for i in range(10))

Health = collections.namedtuple("Health", "status bad vbad flags measures")


@dataclasses.dataclass(frozen=True)
class HealthPolicy:
    """When is a stream still tracking its object, and what happens when it is not.

    The defaults are policy, not measurements: nobody has run real sequences through this tracker, only the synthetic database, so
    treat them as a starting point for your cameras.  A threshold of inf disables its gate; a negative motion threshold never passes.

    patience: consecutive bad frames before a stream is LOST.  min_px / max_px: smallest projected object diameter in picture pixels /
    largest in units of the longer picture side.  margin: how far the projected centre may lie outside the picture, in projected
    diameters.  max_rot_deg, max_shift (projected diameters), max_log2_scale (|log2(z_prev / z_new)|): the motion between the last
    committed pose and the refined one.  verify_every: 0 is off; otherwise on every n-th tick of a group of slots the detector checks the poses
    that tick committed: its position within verify_shift projected diameters of the projected centre and its size within verify_log2_scale octaves
    of the projected one, LOST after verify_patience consecutive failed checks.  reacquire_every: pushes of a LOST stream between
    acquisition attempts.  lag: the host acts on the status of a lane's tick t at push t + lag: push p waits for tick p - lag, so at
    most `lag` ticks of a lane are in flight, the one being enqueued included (0 behaves as 1: a tick's status cannot be known before
    the tick is enqueued)."""
    patience: int = 3
    min_px: float = 8.0
    max_px: float = 4.0
    margin: float = 0.5
    max_rot_deg: float = 45.0
    max_shift: float = 1.0
    max_log2_scale: float = 1.0
    verify_every: int = 0
    verify_shift: float = 1.0
    verify_log2_scale: float = 1.5
    verify_patience: int = 2
    reacquire_every: int = 1
    lag: int = 2

    def __post_init__(self):
        for name in ("patience", "verify_patience", "reacquire_every", "lag", "verify_every"):
            if not isinstance(getattr(self, name), (int, np.integer)) or isinstance(getattr(self, name), bool):
                raise ValueError(f"HealthPolicy: {name} must be an integer")
        if self.patience < 1 or self.verify_patience < 1 or self.reacquire_every < 1:
            raise ValueError("HealthPolicy: patience, verify_patience and reacquire_every must be >= 1")
        if self.lag < 0 or self.verify_every < 0:
            raise ValueError("HealthPolicy: lag and verify_every must be >= 0")
        for name in ("min_px", "max_px", "margin", "max_rot_deg", "max_shift", "max_log2_scale", "verify_shift", "verify_log2_scale"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or math.isnan(float(v)):
                raise ValueError(f"HealthPolicy: {name} must be a number (inf disables the gate), not NaN")

    @classmethod
    def lax(cls, **kw):
        """Every soft gate infinite: only a non-finite pose or an object centre behind the camera loses a stream."""
        inf = float("inf")
        soft = dict(min_px=-inf, max_px=inf, margin=inf, max_rot_deg=inf, max_shift=inf, max_log2_scale=inf, verify_shift=inf,
                    verify_log2_scale=inf)
        soft.update(kw)
        return cls(**soft)


# A frame on its way through a lane: frame is the ingest.Frame (K None) with frame_size, else the uploaded image beside its uploaded K;
# slot is stream % batch in a tick and the index in its chunk in an init.
_Entry = collections.namedtuple("_Entry", "stream slot frame K")
# track_streams: out [n,2,3,4] of a tick or an init chunk, rows [(row, stream, frame)]; with a policy the committed map and the status
_Record = collections.namedtuple("_Record", "out rows commit status")


class _Lane:                                   # what a tick touches
    def __init__(self, stream):
        self.stream, self.graph, self.img, self.K, self.map, self.out = stream, None, None, None, None, None
        self.source = self.staged = None       # crops="source": the static ingest.SourceTable; the Staged of the lane's last tick
        self.emitted = None                    # event recorded after the lane's last emit (wait_emitted)
        self.eff = self.commit = self.draw = self.pic = None   # health: slot maps and picture sizes of the tick (static)
        self.ticks = {}                        # health: ticks per group of slots (the detector's check runs on every n-th)


@contextlib.contextmanager
def _Serial(stream):
    """The tracker's launches run on the lane's stream with whole ticks in flight: no intra-step stream forks (ops.SERIAL, as
    DeviceChain.capture)."""
    old, ops.SERIAL = ops.SERIAL, True
    try:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            yield
    finally:
        ops.SERIAL = old


class _HealthMirror:
    """The host's view of the device's health table, a fixed lag behind it: the status the host routes on.  rows: per
    lane the streams whose groups run on it; pinned: the lanes' rings of snapshot buffers are pinned host memory (a GPU tracker)."""

    def __init__(self, policy, rows, pinned):
        S, ring = sum(len(r) for r in rows), policy.lag + 1
        self.policy, self.rows = policy, rows
        self.status = np.zeros((S, 4), np.int32)               # (status, bad, vbad, flags) per stream as the host last saw them
        self._fresh = [0] * S                  # the lane push index of the stream's last acquisition: older snapshots do not count
        self._attempt = [0] * S                # the stream's own push index of its last acquisition
        self._seen_ok = [False] * S            # the view has shown the stream alive since that acquisition
        self.n, self.consumed = [0] * len(rows), [0] * len(rows)       # pushes each lane worked in / whose snapshots are consumed
        buf = lambda: torch.zeros((S, 4), dtype=torch.int32).pin_memory() if pinned else torch.zeros((S, 4), dtype=torch.int32)
        self.snap = [[buf() for _ in range(ring)] for _ in rows]
        self.events = [[None] * ring for _ in rows]

    def _take(self, s, row):
        self.status[s] = row
        self._seen_ok[s] = self._seen_ok[s] or int(row[0]) in (TRACKING, SUSPECT)

    def due(self, s, frame):
        """A stream the view shows LOST takes the acquisition path at the first push (its own push index: `frame`) after the host learnt
        of the loss, and after a failed attempt at every reacquire_every-th push of the stream."""
        return self.status[s, 0] == LOST and (self._seen_ok[s] or frame - self._attempt[s] >= self.policy.reacquire_every)

    def acquired(self, s, lane, frame):        # an acquisition on this lane: what the view held about the stream is history
        self.status[s], self._fresh[s], self._attempt[s], self._seen_ok[s] = 0, self.n[lane], frame, False

    def forget(self, s):                       # reset
        self.status[s], self._seen_ok[s] = 0, False

    def consume(self):
        """Top of a push (a lane's push number n): wait for the snapshot of the lane's push n - lag and take its rows."""
        lag = self.policy.lag
        for li, rows in enumerate(self.rows):
            while self.consumed[li] <= self.n[li] - max(lag, 1):
                i, k = self.consumed[li], self.consumed[li] % (lag + 1)
                if self.events[li][k] is not None:
                    self.events[li][k].synchronize()
                snap = self.snap[li][k].numpy()
                for s in rows:
                    if self._fresh[s] <= i:
                        self._take(s, snap[s])
                self.consumed[li] += 1

    def snapshot(self, lane, table, stream):
        """End of a lane's work in a push: the health table travels to the next buffer of the lane's ring, ordered on its stream."""
        k = self.n[lane] % len(self.snap[lane])
        with _Serial(stream):
            self.snap[lane][k].copy_(table, non_blocking=True)
            if stream is not None:
                self.events[lane][k] = torch.cuda.Event()
                self.events[lane][k].record(stream)
        self.n[lane] += 1

    def refresh(self, table):
        """health(): the table as read after a synchronisation; every snapshot in flight is older."""
        for s, row in enumerate(table):
            self._take(s, row)
        self.consumed = list(self.n)


class StreamTracker:
    def __init__(self, estimator, max_streams, batch=8, lanes=2, track_iter=1, smooth_num=5, smooth_std=2.5, object_pts=None,
                 graphs=True, frame_size=None, health=None, crops="canvas", minify="point"):
        if estimator.refiner is None:
            raise ValueError("StreamTracker: the estimator has no refiner (tracking refines every frame)")
        self.max_streams, self.batch, self.nlanes = int(max_streams), int(batch), int(lanes)
        self.track_iter, self.num, self.std = int(track_iter), int(smooth_num), float(smooth_std)
        if self.max_streams < 1 or self.nlanes < 1 or self.track_iter < 1:
            raise ValueError("StreamTracker: max_streams, lanes and track_iter must be >= 1")
        if not 1 <= self.batch <= _refiner.MAX_BATCH:
            raise ValueError(f"StreamTracker: 1 <= batch <= {_refiner.MAX_BATCH} expected")
        if not 1 <= self.num <= 64 or not self.std > 0:
            raise ValueError("StreamTracker: 1 <= smooth_num <= 64 and smooth_std > 0 expected")
        if health is not None and not isinstance(health, HealthPolicy):
            raise ValueError("StreamTracker: health must be a HealthPolicy or None")
        self.policy, self.est, self.chain = health, estimator, estimator.device_chain()
        self.dev = torch.device(estimator.device)
        self.cuda = self.dev.type == "cuda"
        if graphs and not self.cuda:
            raise ValueError("StreamTracker: graphs=True needs the GPU (graphs=False runs the same ticks eagerly)")
        self.graphs = bool(graphs)
        pts = EV.get_ref_point_cloud(estimator.refiner.ref_database) if object_pts is None else object_pts
        self.box_np = G.box_corners(pts)
        self.box = torch.from_numpy(self.box_np.astype(np.float32)).to(self.dev)
        S = self.max_streams
        self.pose_table, self.smooth_table = (torch.zeros((S, 12), dtype=torch.float32, device=self.dev) for _ in range(2))
        self.hist = torch.zeros((S, self.num, 8, 2), dtype=torch.float64, device=self.dev)
        self.hist_count = torch.zeros(S, dtype=torch.int32, device=self.dev)
        self.parking = self.chain.ref_poses[0].contiguous()
        self._lanes = [_Lane(torch.cuda.Stream(device=self.dev) if self.cuda else None) for _ in range(self.nlanes)]
        self._mirror = None                    # the host's lagged view of the health table (_HealthMirror), with a policy
        tables = [self.box, self.pose_table, self.smooth_table, self.hist, self.hist_count]
        if health is not None:
            tables += self._health_state()
        if self.cuda:
            for ln in self._lanes:             # the tables live as long as the tracker; their blocks outlive no lane's pending work
                for t in tables:
                    t.record_stream(ln.stream)
        self._started, self._shape = [False] * S, None
        self._frames = [0] * S                 # frames pushed per stream
        self.frame_size = None                 # (H, W): frames of any size and format are ingested into H x W images on the device
        if frame_size is not None:
            if len(frame_size) != 2 or min(int(v) for v in frame_size) < 1:
                raise ValueError("StreamTracker: frame_size must be (H, W) with H, W >= 1")
            self.frame_size = (int(frame_size[0]), int(frame_size[1]))
            self._shape = self.frame_size + (3,)
        if crops not in ("canvas", "source"):
            raise ValueError(f"StreamTracker: crops must be \"canvas\" or \"source\", not {crops!r}")
        if crops == "source" and self.frame_size is None:
            raise ValueError("StreamTracker: crops=\"source\" needs a tracker with frame_size (without it the canvas is the only source "
                             "there is)")
        self.source_crops = crops == "source"  # the query crops are cut from the camera-native pictures (g6d_frame_crop)
        if minify not in I.MINIFY:
            raise ValueError(f"StreamTracker: minify must be \"point\" or \"area\", not {minify!r}")
        if minify == "area" and self.frame_size is None:
            raise ValueError("StreamTracker: minify=\"area\" needs a tracker with frame_size (without it nothing is scaled: the frames "
                             "arrive at the canvas size)")
        self.minify = minify                   # "area": the ingest and the source crops filter where they shrink
        self._records = None                   # track_streams: [_Record]
        self._sinks = {}                       # the running push: stream id -> [Sink, ...]
        for net in self._nets():               # maps of earlier unchecked calls do not count against the tracker
            t = net.__dict__.get("_range")
            if t is not None and t.names:
                t.clear()

    # ------------------------------------------------------------------ public API
    def push(self, stream_ids, imgs, Ks=None, sinks=None):
        """Enqueue one frame per listed stream: imgs uint8 [H,W,3] (numpy or device tensors; one shape per tracker), Ks [3,3] per stream
        (None: predict.py's pseudo K).  A tracker with `frame_size` takes `ingest.Frame`s of any size and format instead (plain [h,w,3]
        arrays count as rgb24 frames); their intrinsics travel in Frame.K, so Ks must be None.
        sinks: None, or one entry per stream id: an `emit.Sink`, a list of them (predict.py writes the raw and the smoothed picture of a
        frame) or None.  Each sink receives the stream's working-resolution frame with the box of this frame's pose drawn on it; the
        picture's size is the frame's `ingest.plan` with `frame_size`, the whole image otherwise.  Device sinks are written on the lane's
        stream; host sinks are valid after `wait_emitted` or `result`.  Sinks with view="source" (mixed freely with the others)
        receive the stream's `ingest.Frame` of this push as the camera delivered it, with the box in source pixels; they need a
        tracker with `frame_size` and a frame without a lens (ValueError before anything is launched).  Does not synchronise."""
        ids = self._ids(stream_ids)
        if len(imgs) != len(ids) or (Ks is not None and len(Ks) != len(ids)):
            raise ValueError("StreamTracker.push: one image (and K) per stream id expected")
        self._sinks = self._sink_lists(ids, sinks)
        source = {s for s, lst in self._sinks.items() if any(k.view == "source" for k in lst)}
        if source and self.frame_size is None:
            self._sinks = {}
            raise ValueError("StreamTracker.push: a source-view sink needs a tracker with frame_size (without it the canvas is the only "
                             "source there is)")
        if self.frame_size is not None:
            if Ks is not None:
                raise ValueError("StreamTracker.push: a tracker with frame_size takes the intrinsics in Frame.K, not in Ks")
            frames = [im if isinstance(im, I.Frame) else I.Frame(self._rgb(im)) for im in imgs]
            Ks = [None] * len(ids)
            for s, f in zip(ids, frames):
                if s in source and f.lens is not None:
                    self._sinks = {}
                    raise ValueError(f"StreamTracker.push: stream {s}'s frame has a lens, so its source picture is distorted (a straight "
                                     "box edge is a curve in it); the source view of lens frames is out of scope, use a canvas sink")
        else:
            frames = [self._frame(im) for im in imgs]
            Ks = [EV.pseudo_K(*self._shape[:2])] * len(ids) if Ks is None else Ks
        groups = {}
        for s, f, K in zip(ids, frames, Ks):
            groups.setdefault(s // self.batch, []).append((s, f, K))
        cur = torch.cuda.current_stream(self.dev) if self.cuda else None
        mirror = self._mirror
        if mirror is not None:
            mirror.consume()                   # before any lane work: the wait stays clear of a capture
        worked = {}
        for g in sorted(groups):
            li, lane = g % self.nlanes, self._lanes[g % self.nlanes]
            if cur is not None:
                lane.stream.wait_stream(cur)
            with _Serial(lane.stream):
                ents = [self._entry(s, f, K, lane) for s, f, K in groups[g]]
                fresh = {e.stream for e in ents if not self._started[e.stream] or
                         (mirror is not None and mirror.due(e.stream, self._frames[e.stream]))}
                track = [e for e in ents if e.stream not in fresh]
                init = [e for e in ents if e.stream in fresh]
                if mirror is not None:
                    worked[li] = lane
                    for e in init:
                        mirror.acquired(e.stream, li, self._frames[e.stream])
                if track:
                    self._tick(lane, track)
                for c0 in range(0, len(init), INIT_CHUNK):
                    self._init(init[c0:c0 + INIT_CHUNK])
                if self.cuda and any(e.stream in self._sinks for e in ents):
                    lane.emitted = torch.cuda.Event()
                    lane.emitted.record(lane.stream)
        for li, lane in worked.items():        # the last thing on the lane's stream in this push
            mirror.snapshot(li, self.health_table, lane.stream)
        self._sinks = {}
        for s in ids:
            self._started[s] = True
            self._frames[s] += 1

    def health(self, stream_ids=None):
        """Synchronise and refresh the host's status mirror -> {id: Health(status, bad, vbad, flags, measures [12] float32)} of each
        stream (stream_ids None: every stream that has a frame).  Needs a tracker with a HealthPolicy."""
        if self._mirror is None:
            raise ValueError("StreamTracker.health: the tracker has no HealthPolicy")
        ids = [s for s in range(self.max_streams) if self._frames[s]] if stream_ids is None else self._ids(stream_ids)
        if self.cuda:
            torch.cuda.synchronize(self.dev)
        Hh, M = self.health_table.cpu().numpy(), self.measures.cpu().numpy()
        self._mirror.refresh(Hh)
        return {s: Health(int(Hh[s, 0]), int(Hh[s, 1]), int(Hh[s, 2]), int(Hh[s, 3]), M[s].copy()) for s in ids}

    def result(self, stream_ids=None):
        """Synchronise -> {id: (pose [3,4], smoothed [3,4])} float32 numpy of each stream's latest frame (stream_ids None: every stream
        that has one).  Raises RuntimeError if an fp16 pair map of the networks left the representable window since the last check:
        the poses since then cannot be trusted (reset the streams; the maps' exponents are updated for the frames that follow).  The
        error covers the frames emitted into sinks since the last check as well: their boxes were drawn from those poses."""
        if self.cuda:
            torch.cuda.synchronize(self.dev)
        self._check_range()
        ids = [s for s in range(self.max_streams) if self._frames[s]] if stream_ids is None else self._ids(stream_ids)
        for s in ids:
            if not self._frames[s]:
                raise ValueError(f"StreamTracker.result: stream {s} has no frame")
        P, Sm = self.pose_table.cpu().numpy(), self.smooth_table.cpu().numpy()
        return {s: (P[s].reshape(3, 4).copy(), Sm[s].reshape(3, 4).copy()) for s in ids}

    def wait_emitted(self, stream_ids=None):
        """Block the host until the sinks of the listed streams' pushes (None: of every stream) are filled: waits on the events of the
        lanes involved, not on the device.  Host sinks are valid after it (or after `result`); it does not run the range check."""
        lanes = self._lanes if stream_ids is None else [self._lanes[(s // self.batch) % self.nlanes] for s in self._ids(stream_ids)]
        for ln in lanes:
            if ln.emitted is not None:
                ln.emitted.synchronize()

    def reset(self, stream_ids):
        """The next frame of these streams starts over: detection, selection, full refinement, fresh smoothing history."""
        for s in self._ids(stream_ids):
            self._started[s] = False
            if self._mirror is not None:
                self._mirror.forget(s)

    # ------------------------------------------------------------------ internals
    def _health_state(self):
        S, pol = self.max_streams, self.policy
        self.health_table = torch.zeros((S, 4), dtype=torch.int32, device=self.dev)
        self.measures = torch.zeros((S, 12), dtype=torch.float32, device=self.dev)
        self.diameter = float(np.linalg.norm(np.asarray(self.box_np[6], np.float64) - np.asarray(self.box_np[0], np.float64)))
        info = self.est.ref_info               # the object's mean projected diameter in the reference views, float64
        P, Kr = np.asarray(info["poses"], np.float64).reshape(-1, 3, 4), np.asarray(info["Ks"], np.float64).reshape(-1, 3, 3)
        z = P[:, 2, :3] @ np.asarray(info["center"], np.float64).reshape(3) + P[:, 2, 3]
        self.ref_px = float(np.mean(0.5 * (Kr[:, 0, 0] + Kr[:, 1, 1]) * self.diameter / z))
        self._mirror = _HealthMirror(pol, [[s for s in range(S) if (s // self.batch) % self.nlanes == li] for li in range(self.nlanes)],
                                     self.cuda)
        return [self.health_table, self.measures]              # (recorded on the lanes' streams with the other tables)

    def _nets(self):
        return [n for n in (self.est.detector, self.est.selector, self.est.refiner) if n is not None]

    def _ids(self, stream_ids):
        ids = [int(s) for s in stream_ids]
        for s in ids:
            if not 0 <= s < self.max_streams:
                raise ValueError(f"StreamTracker: stream id {s} outside [0, {self.max_streams})")
        if len(set(ids)) != len(ids):
            raise ValueError("StreamTracker: a stream id is listed twice")
        return ids

    @staticmethod
    def _sink_lists(ids, sinks):
        """push's `sinks` -> {stream id: [Sink, ...]} for the streams that have any."""
        if sinks is None:
            return {}
        sinks = list(sinks)
        if len(sinks) != len(ids):
            raise ValueError("StreamTracker.push: sinks must be None or hold one entry (Sink, list of Sinks or None) per stream id")
        out = {}
        for s, ent in zip(ids, sinks):
            lst = [] if ent is None else ([ent] if isinstance(ent, E.Sink) else list(ent))
            if any(not isinstance(k, E.Sink) for k in lst):
                raise ValueError("StreamTracker.push: a sinks entry is an emit.Sink, a list of them or None")
            if lst:
                out[s] = lst
        return out

    def _entry(self, s, frame, K, lane):
        if K is None:                          # an ingest.Frame: uploaded and converted by the lane's ingest launch
            return _Entry(s, None, frame, None)
        K = K.reshape(3, 3).float() if torch.is_tensor(K) else np.asarray(K, np.float32).reshape(3, 3)
        return _Entry(s, None, self._upload(frame, lane), self._upload(K, lane))

    def _picture(self, e):
        """The picture (h, w) of an entry inside its canvas: what the ingest plans for a Frame, a plain image fills the canvas."""
        return I.plan(e.frame, self._shape[:2])[:2] if isinstance(e.frame, I.Frame) else tuple(e.frame.shape[:2])

    def _pic(self, ents, n):
        """int32 [n,2]: the picture (w, h) in each entry's slot, the whole canvas in a slot without an entry (g6d_track_health's pic)."""
        h, w = self._shape[:2]
        pic = np.tile(np.asarray([w, h], np.int32), (n, 1))
        for e in ents:
            pic[e.slot] = self._picture(e)[::-1]
        return pic

    def _corners(self, K9, slot_map, sinks):
        """The box under the raw / smoothed poses just committed -> (pts [2,n,8,2], valid [2,n]): one g6d_track_corners launch per
        corner set that one of `sinks` names (a set is read only by sinks that name it)."""
        n = slot_map.shape[0]
        pts = torch.empty((2, n, 8, 2), dtype=torch.int32, device=self.dev)
        valid = torch.empty((2, n), dtype=torch.int32, device=self.dev)
        for name, table in (("raw", self.pose_table), ("smooth", self.smooth_table)):
            if any(k.box and k.pose == name for k in sinks):
                ops.track_corners(table, K9, slot_map, self.box, pts[E.POSES[name]], valid[E.POSES[name]])
        return pts, valid

    def _wants_source(self, ents):
        return any(k.view == "source" for e in ents for k in self._sinks.get(e.stream, ()))

    def _emit(self, imgs, K9, slot_map, ents, staged=None):
        """Project the box under the raw / smoothed poses just committed and fill the sinks of these streams on the current (lane's)
        stream.  Canvas sinks: at most two g6d_track_corners launches and one g6d_frame_emit launch.  Source-view sinks (staged: the
        frame table the ingest of `ents` kept): one pinned upload of the sources' intrinsics, at most two more g6d_track_corners
        launches under them, with the same slot map and therefore the same health behaviour, and one g6d_frame_emit_source launch."""
        todo = [(i, e, k) for i, e in enumerate(ents) for k in self._sinks.get(e.stream, ())]
        canvas = [(e, k) for _, e, k in todo if k.view == "canvas"]
        if canvas:
            pts, valid = self._corners(K9, slot_map, [k for _, k in canvas])
            sizes = [self._picture(e) for e, _ in canvas]
            E.emit_frames(imgs, pts, valid, [k for _, k in canvas], slots=[e.slot for e, _ in canvas], pic_sizes=sizes)
        source = [(i, e, k) for i, e, k in todo if k.view == "source"]
        if source:
            Ks = np.tile(np.eye(3, dtype=np.float32).reshape(9), (slot_map.shape[0], 1))      # rows of slots nobody draws stay harmless
            for _, e, _ in source:
                Ks[e.slot] = I.source_K(e.frame, self._shape[:2]).astype(np.float32).reshape(9)
            pts, valid = self._corners(self._upload(Ks), slot_map, [k for _, _, k in source])
            E.emit_source_frames(staged, pts, valid, [k for _, _, k in source], sources=[i for i, _, _ in source])

    @staticmethod
    def _rgb(im):
        im = im if torch.is_tensor(im) else np.asarray(im)
        if im.dtype not in (np.uint8, torch.uint8) or len(im.shape) != 3 or im.shape[2] != 3:
            raise ValueError("StreamTracker: frames must be uint8 [H,W,3]")
        return im

    def _frame(self, im):
        im = self._rgb(im)
        self._shape = self._shape or tuple(im.shape)       # the first frame sets the tracker's shape
        if tuple(im.shape) != self._shape:
            raise ValueError(f"StreamTracker: frame shape {tuple(im.shape)} differs from the tracker's {self._shape}")
        return im

    def _upload(self, a, lane=None):
        """Host arrays -> device on the current (lane's) stream, through pinned memory: no host stall on the stream; device tensors are
        recorded on the lane's stream."""
        if torch.is_tensor(a) and a.device.type == "cuda":
            a.record_stream(lane.stream)
            return a.contiguous()
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.pin_memory().to(self.dev, non_blocking=True) if self.cuda else t.to(self.dev)

    def _statics(self, lane):
        if lane.img is None:
            B, (h, w) = self.batch, self._shape[:2]
            lane.img = torch.zeros((B, h, w, 3), dtype=torch.uint8, device=self.dev)
            lane.K = torch.from_numpy(np.repeat(EV.pseudo_K(h, w)[None], B, 0)).to(self.dev)
            lane.map = torch.full((B,), -1, dtype=torch.int32, device=self.dev)
            if self.source_crops:              # B frame records and the slot -> record map the tick's graph reads (-1: the canvas)
                lane.source = I.SourceTable(torch.zeros(B * I.RECORD_BYTES, dtype=torch.uint8, device=self.dev),
                                            torch.full((B,), -1, dtype=torch.int32, device=self.dev))
            if self.policy is not None:
                lane.eff, lane.commit, lane.draw = (torch.full((B,), -1, dtype=torch.int32, device=self.dev) for _ in range(3))
                lane.pic = torch.tensor([[w, h]] * B, dtype=torch.int32, device=self.dev)

    def _ingest(self, frames, out, K_out, slots=None):
        """The ingest of a tick or of first frames whose frame table nobody reads afterwards: `ingest_frames` as always, or with
        minify="area" the filtered launch (`ingest_frames_keep` carries the switch; its table is dropped)."""
        if self.minify == "area":
            I.ingest_frames_keep(frames, out, K_out, slots=slots, minify=self.minify)
        else:
            I.ingest_frames(frames, out, K_out, slots=slots)

    def _judge(self, prev, pose, K9, pic, size, slot_map, commit=None, draw=None):
        """The health step between a refinement from the gathered poses `prev` (None: an acquisition) and its commit -> (slot_commit,
        slot_draw): a frame that fails its gates is not committed, a LOST stream is not drawn.  Without a policy: the slot map itself."""
        if self.policy is None:
            return slot_map, slot_map
        n = slot_map.shape[0]
        return ops.track_health(None if prev is None else prev.reshape(n, 12), pose.reshape(n, 12), K9, pic, size, slot_map, prev is None,
                                self.chain.center, self.diameter, self.policy, self.health_table, self.measures, commit, draw)

    def _tick_fn(self, lane):
        """(gate ->) gather -> track_iter refinement steps (query_batch's refine loop) (-> health) -> commit of the frames that passed,
        on the lane's static buffers -> (out, slot_commit, slot_draw).  The gate parks lost streams and non-finite rows."""
        eff, K9 = lane.map, lane.K.reshape(self.batch, 9)
        if self.policy is not None:
            eff = ops.track_gate(self.pose_table, self.health_table, lane.map, lane.eff)
        pose0 = ops.track_gather(self.pose_table, eff, self.parking)
        if lane.source is None:
            r = self.chain.query_batch(lane.img, lane.K, pose_init=pose0, refine_iter=self.track_iter)
        else:
            r = self.chain.query_batch_source(lane.img, lane.K, lane.source, pose_init=pose0, refine_iter=self.track_iter,
                                              minify=self.minify)
        commit, draw = self._judge(pose0, r["pose"], K9, lane.pic, None, eff, lane.commit, lane.draw)
        return ops.track_commit(r["pose"], K9, commit, False, self.box, self.num, self.std, self.pose_table, self.hist, self.hist_count,
                                self.smooth_table), commit, draw

    def _capture(self, lane, warmup=2):
        lane.map.fill_(-1)
        if lane.source is not None:            # warm-up and capture run on the canvases: the table holds no frame yet
            lane.source.rec.fill_(-1)
        for _ in range(warmup):
            self._tick_fn(lane)
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            lane.out = self._tick_fn(lane)
        finally:
            graph.capture_end()
        lane.graph = graph

    def _tick(self, lane, ents):
        self._statics(lane)
        ents = [e._replace(slot=e.stream % self.batch) for e in ents]
        m = np.full(self.batch, -1, np.int32)
        m[[e.slot for e in ents]] = [e.stream for e in ents]
        if self.graphs and lane.graph is None:
            self._capture(lane)
        staged = None
        if self.frame_size is not None:        # one launch fills the named slots of the static image and K buffers
            if self.source_crops or self._wants_source(ents):      # ... and leaves its frame table on the device for the source-view
                staged = I.ingest_frames_keep([e.frame for e in ents], lane.img, lane.K, slots=[e.slot for e in ents],
                                              minify=self.minify)[1]                                           # emit and crops
            else:
                self._ingest([e.frame for e in ents], lane.img, lane.K, slots=[e.slot for e in ents])
        else:
            for e in ents:
                lane.img[e.slot].copy_(e.frame)
                lane.K[e.slot].copy_(e.K)
        lane.map.copy_(self._upload(m))
        if lane.source is not None:            # the graph reads the planes after push has returned: the Staged lives until the next tick
            lane.source.load(staged)
            lane.staged = staged
        if lane.pic is not None:               # (a policy's static buffer)
            lane.pic.copy_(self._upload(self._pic(ents, self.batch)))
        if self.graphs:
            lane.graph.replay()
        out, commit, draw = lane.out if self.graphs else self._tick_fn(lane)
        judged = commit is not lane.map        # (_judge hands the map itself back when there is no policy)
        if judged:
            g = ents[0].stream // self.batch   # groups that share a lane count their own ticks: each is checked every n-th time
            lane.ticks[g] = lane.ticks.get(g, 0) + 1
            if self.policy.verify_every and lane.ticks[g] % self.policy.verify_every == 0:
                self._verify(lane)
        if self._records is not None:
            self._records.append(_Record(out.clone(), [(e.slot, e.stream, self._frames[e.stream]) for e in ents],
                                         commit.clone() if judged else None, self.health_table[:, 0].clone() if judged else None))
        if self._sinks:
            self._emit(lane.img, lane.K.reshape(self.batch, 9), draw, ents, staged)

    def _verify(self, lane):
        """The detector's check of the poses this tick committed: the detection half of query_batch on the lane's image batch in chunks
        of <= INIT_CHUNK images and one g6d_track_verify launch per chunk, eager on the lane's stream after the tick's graph.  The
        tick's slot_draw is not recomputed: a stream this check has just lost still shows this frame's (committed) box and loses it
        from the next frame on."""
        K9 = lane.K.reshape(self.batch, 9)
        for c0 in range(0, self.batch, INIT_CHUNK):
            c1 = min(c0 + INIT_CHUNK, self.batch)
            det = self.chain.detect_batch(lane.img[c0:c1])
            ops.track_verify(det, self.pose_table, K9[c0:c1], lane.commit[c0:c1], self.chain.center, self.diameter, self.ref_px,
                             self.policy, self.health_table, self.measures)

    def _init(self, ents):
        n, (H, W) = len(ents), self._shape[:2]
        ents = [e._replace(slot=i) for i, e in enumerate(ents)]
        native, staged = self.frame_size is not None, None
        if native:
            imgs = torch.empty((n,) + self._shape, dtype=torch.uint8, device=self.dev)
            Ks = torch.empty((n, 3, 3), dtype=torch.float32, device=self.dev)
            if self.source_crops or self._wants_source(ents):
                staged = I.ingest_frames_keep([e.frame for e in ents], imgs, Ks, minify=self.minify)[1]
            else:
                self._ingest([e.frame for e in ents], imgs, Ks)
        else:
            imgs = torch.stack([e.frame for e in ents], 0)
            Ks = torch.stack([e.K for e in ents], 0)
        r = (self.chain.query_batch_source(imgs, Ks, I.SourceTable.of(staged), minify=self.minify) if self.source_crops else
             self.chain.query_batch(imgs, Ks))
        pose, K9 = r["pose"].reshape(n, 12), Ks.reshape(n, 9)
        ids = self._upload(np.asarray([e.stream for e in ents], np.int32))
        pic = self._upload(self._pic(ents, n)) if native and self.policy is not None else None
        commit, draw = self._judge(None, pose, K9, pic, (W, H), ids)
        judged = commit is not ids             # an acquisition that fails its gates is not committed (its rows of out stay 0): still LOST
        out = ops.track_commit(pose, K9, commit, True, self.box, self.num, self.std, self.pose_table, self.hist, self.hist_count,
                               self.smooth_table, out=torch.zeros((n, 2, 3, 4), dtype=torch.float32, device=self.dev) if judged else None)
        if self._records is not None:
            self._records.append(_Record(out, [(e.slot, e.stream, self._frames[e.stream]) for e in ents], commit if judged else None,
                                         self.health_table[:, 0].clone() if judged else None))
        if self._sinks:
            self._emit(imgs, K9, draw, ents, staged)

    def _check_range(self):
        bad = []
        for net in self._nets():
            t = net.__dict__.get("_range")
            if t is None or not t.names:
                continue
            a = t.read()
            t.clear()
            out = {n: v for n, v in a.items() if ops.pair_out_of_window(v, t.e[t.names[n]])}
            if out:
                t.set_exponents({n: ops.pair_exponent(v, t.e[t.names[n]]) for n, v in out.items()})
                bad.append(f"{type(net).__name__}: " + ", ".join(f"{n} max |v| = {v:g}" for n, v in out.items()))
        if bad:
            raise RuntimeError("StreamTracker: fp16 pair maps left the representable window since the last check (" + "; ".join(bad) +
                               "); the poses since then cannot be trusted — reset the streams")

    def _collect(self, lengths):
        """track_streams: one synchronisation, one read-back -> per stream (poses [T,3,4], smoothed [T,3,4])."""
        if self.cuda:
            torch.cuda.synchronize(self.dev)
        recs = self._records
        rows = torch.cat([r.out.reshape(-1, 2, 12) for r in recs], 0).cpu().numpy() if recs else np.zeros((0, 2, 12))
        res = [(np.zeros((T, 3, 4), np.float32), np.zeros((T, 3, 4), np.float32)) for T in lengths]
        if self.policy is not None:            # ... and status [T]; a frame that was not committed repeats the previous frame's poses
            res = [r + (np.zeros(len(r[0]), np.int32),) for r in res]
        judged = bool(recs) and recs[0].commit is not None
        commits = torch.cat([r.commit for r in recs], 0).cpu().numpy() if judged else None
        status = torch.stack([r.status for r in recs], 0).cpu().numpy() if judged else None
        base = 0
        for i, rec in enumerate(recs):
            for row, s, f in rec.rows:
                if judged:
                    res[s][2][f] = status[i, s]
                    if commits[base + row] < 0:
                        res[s][0][f], res[s][1][f] = (res[s][0][f - 1], res[s][1][f - 1]) if f else (0, 0)
                        continue
                res[s][0][f] = rows[base + row, 0].reshape(3, 4)
                res[s][1][f] = rows[base + row, 1].reshape(3, 4)
            base += rec.out.shape[0]
        return res


def _stream_Ks(Ks, seqs):
    out = []
    for s, frames in enumerate(seqs):
        k = None if Ks is None else Ks[s]
        if k is None:
            out.append([EV.pseudo_K(*np.asarray(f).shape[:2]) for f in frames])
            continue
        k = np.asarray(k, np.float32)
        if k.shape == (3, 3):
            out.append([k] * len(frames))
        elif k.shape == (len(frames), 3, 3):
            out.append(list(k))
        else:
            raise ValueError(f"track_streams: Ks of stream {s} must be [3,3] or [T,3,3]")
    return out


def _ingest_to_host(frames, frame_size, device, minify="point"):
    """Frames of any format -> ([H,W,3] uint8 arrays, [3,3] float32 Ks) through the device ingest (track_streams' rare fallback path),
    by the tracker's own `minify` rule, so that a recomputed sequence sees the pictures the tracker saw."""
    imgs, Ks = [], []
    for f in frames:
        img = torch.empty((1, int(frame_size[0]), int(frame_size[1]), 3), dtype=torch.uint8, device=device)
        K = torch.empty((1, 3, 3), dtype=torch.float32, device=device)
        frame = [f if isinstance(f, I.Frame) else I.Frame(StreamTracker._rgb(f))]
        if minify == "area":
            I.ingest_frames_keep(frame, img, K, minify=minify)
        else:
            I.ingest_frames(frame, img, K)
        imgs.append(img[0].cpu().numpy())
        Ks.append(K[0].cpu().numpy())
    return imgs, Ks


def host_track(estimator, frames, Ks, track_iter=1, smooth_num=5, smooth_std=2.5, box=None):
    """One stream through the host-driven loop of predict.py:49-72: `estimator.predict` per frame (first frame: cfg['refine_iter'] steps,
    later frames: `track_iter` steps from the previous pose) and the numpy box smoothing + PnP -> (poses [T,3,4], smoothed [T,3,4])."""
    box = G.box_corners(EV.get_ref_point_cloud(estimator.refiner.ref_database)) if box is None else box
    poses, smooth, hist, pose, it0 = [], [], [], None, estimator.cfg["refine_iter"]
    try:
        for im, K in zip(frames, Ks):
            if pose is not None:
                estimator.cfg["refine_iter"] = track_iter
            pose, _ = estimator.predict(np.asarray(im), K, pose_init=pose)
            K64, p64 = np.asarray(K, np.float64), np.asarray(pose, np.float32).astype(np.float64)
            hist.append(G.project_points(box, p64, K64)[0])
            poses.append(pose)
            smooth.append(G.pnp(box, G.weighted_points(hist, smooth_num, smooth_std), K64, p64))
    finally:
        estimator.cfg["refine_iter"] = it0
    return np.asarray(poses, np.float32).reshape(-1, 3, 4), np.asarray(smooth, np.float32).reshape(-1, 3, 4)


def track_streams(estimator, streams, Ks=None, **tracker_kw):
    """S frame sequences (possibly of different lengths; uint8 [H,W,3] frames of one shape) -> per stream (poses [T,3,4], smoothed
    [T,3,4]) float32 for every frame.  Ks: None (predict.py's pseudo K) or per stream one [3,3] or one per frame [T,3,3].  With
    `frame_size=(H, W)` the frames are `ingest.Frame`s (or [h,w,3] arrays) of any size and format, carry their own K, and Ks stays None;
    `crops="source"` then cuts the networks' query crops from them (StreamTracker), also when the sequences are recomputed, and
    `minify="area"` filters what shrinks, in the ticks and in the recomputation alike.  Frame t of
    every stream that has one is pushed in tick t; one synchronisation at the end.  Runs under the estimator's range guard: if an fp16
    pair map left the window, the sequences are recomputed by the host-driven loop (`host_track`) with those networks on fp32.
    With `health=HealthPolicy(...)` every stream's tuple is (poses, smoothed, status [T] int32): the status after each frame; a frame
    that was not committed repeats the previous frame's poses (all zero before the first commit).  The host-driven recomputation has
    no health notion: it reports every frame as TRACKING."""
    seqs = [list(s) for s in streams]
    kw = dict(tracker_kw)
    native = kw.get("frame_size") is not None
    if native and Ks is not None:
        raise ValueError("track_streams: with frame_size the intrinsics travel in Frame.K, not in Ks")
    Kss = None if native else _stream_Ks(Ks, seqs)

    def run(**over):
        tr = StreamTracker(estimator, len(seqs), **{**kw, **over})
        tr._records = []
        for t in range(max((len(s) for s in seqs), default=0)):
            ids = [s for s in range(len(seqs)) if t < len(seqs[s])]
            tr.push(ids, [seqs[s][t] for s in ids], None if native else [Kss[s][t] for s in ids])
        return tr._collect([len(s) for s in seqs])

    def recompute():
        box = None if kw.get("object_pts") is None else G.box_corners(kw["object_pts"])
        # the host loop takes plain arrays: native frames are ingested on the device one by one and read back
        host = ([_ingest_to_host(frames, kw["frame_size"], estimator.device, kw.get("minify", "point")) for frames in seqs] if native
                else zip(seqs, Kss))
        return [host_track(estimator, fr, Kh, kw.get("track_iter", 1), kw.get("smooth_num", 5), kw.get("smooth_std", 2.5), box)
                for fr, Kh in host]
    if kw.get("crops", "canvas") == "source":
        # the host-driven loop sees canvases only: the recomputation is the same ticks run eagerly, which follow the networks' routes
        return estimator._range_guarded(run, lambda: run(graphs=False))
    if kw.get("health") is None:
        return estimator._range_guarded(run, recompute)
    return estimator._range_guarded(run, lambda: [r + (np.full(len(r[0]), TRACKING, np.int32),) for r in recompute()])
