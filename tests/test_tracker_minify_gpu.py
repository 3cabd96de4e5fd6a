"""The tracker with minify="area" on the MI355X (gen6d_amd/tracking.py; the kernels themselves:
tests/test_ingest_area_gpu.py, tests/test_frame_crop_area_gpu.py), on camera-native frames 2x and 3x the canvas of the scene of
tests/test_track_streams_gpu.py: graphs against eager ticks, a stream's first frame against the stand-alone composition
(ingest_frames_keep + query_batch_source, both with minify="area"), and the switch against the default."""
import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import tracking as T
from test_track_streams_gpu import _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu


def _enlarged(frame, k, rng):
    """A scene frame [h,w,3] -> a camera-style bgr24 Frame k times its size whose k x k blocks average to about the frame's pixels and
    hold detail the point rule picks one sample of: noise of +-40 levels around every pixel."""
    big = np.repeat(np.repeat(frame.astype(np.int64), k, 0), k, 1) + rng.randint(-40, 41, (frame.shape[0] * k, frame.shape[1] * k, 1))
    return I.Frame(np.ascontiguousarray(np.clip(big, 0, 255).astype(np.uint8)[..., ::-1]), "bgr24")


def _natives(frames, S):
    rng = np.random.RandomState(5)
    return [[_enlarged(f, 2 + (s + t) % 2, rng) for t, f in enumerate(q)] for s, q in enumerate(_seqs(frames, S, 3, seed=3))]


def test_area_tracker_graphs_match_eager_and_differ_from_point(scene):
    db, est, frames, Ks = scene
    H, W = frames[0].shape[:2]
    native = _natives(frames, 3)
    kw = dict(batch=2, lanes=2, frame_size=(H, W), crops="source")
    g = T.track_streams(est, native, graphs=True, minify="area", **kw)
    e = T.track_streams(est, native, graphs=False, minify="area", **kw)
    for (pg, sg), (pe, se) in zip(g, e):
        assert np.isfinite(pg).all() and np.isfinite(sg).all()
        np.testing.assert_allclose(pg, pe, atol=3e-4)
        np.testing.assert_allclose(sg, se, atol=3e-4)
    # a stream's first frame is the stand-alone composition with the same switch
    chain = est.device_chain()
    # (per group of `batch` streams, as the tracker acquires them: the networks' routes depend on the batch)
    for group in ((0, 1), (2,)):
        n = len(group)
        img, K = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda"), torch.empty((n, 3, 3), device="cuda")
        staged = I.ingest_frames_keep([native[s][0] for s in group], img, K, minify="area")[1]
        one = chain.query_batch_source(img, K, I.SourceTable.of(staged), minify="area")
        for i, s in enumerate(group):
            np.testing.assert_allclose(g[s][0][0], one["pose"][i].cpu().numpy(), atol=3e-4, err_msg=f"stream {s}")
    # the switch is wired: the point-sampled tracker sees other pictures and other crops of the same frames
    p = T.track_streams(est, native, graphs=True, **kw)
    assert max(np.abs(pa - pp).max() for (pa, _), (pp, _) in zip(g, p)) > 3e-4        # (the bar under which two runs count as equal above)
