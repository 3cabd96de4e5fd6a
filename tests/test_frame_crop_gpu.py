"""g6d_frame_crop on the MI355X against the numpy restatement of its rule (tests/test_frame_crop_cpu.py) in float64, under the project's
warp rule; slots without a source against g6d_warp_batch, bit for bit; the launcher's argument checks.  The tracker's side of
crops="source" is in tests/test_tracker_source_crops_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from test_frame_crop_cpu import homographies, np_crop, records_of_frames, source_frame, warp_rule

pytestmark = pytest.mark.gpu

_cuda = lambda a: torch.from_numpy(a).cuda()


def _case(rng, rot, B, rec, kinds):
    """Frames of `kinds` turned by `rot`, ingested into their slots of B noise canvases (97 x 129, turned with the frames) ->
    (frames, staged, imgs, rec, hinv): everything on the device but the frames' host copies the restatement reads."""
    H, W = (129, 97) if rot in (90, 270) else (97, 129)
    make = {"rgb24": lambda: source_frame(rng, 50, 70, "rgb24", rot, mv=_cuda),
            "bgra32": lambda: source_frame(rng, 97, 129, "bgra32", rot, extra=24, mv=_cuda),
            "nv12": lambda: source_frame(rng, 388, 516, "nv12", rot, extra=32, matrix=("bt601", "bt709")[rot in (90, 270)], split=True, mv=_cuda)}
    frames = [make[k]() for k in kinds]
    imgs = _cuda(rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8))
    Ks = torch.empty((B, 3, 3), device="cuda")
    slots = [rec.index(i) for i in range(len(frames))]
    staged = I.ingest_frames_keep(frames, imgs, Ks, slots=slots)[1]
    np.testing.assert_array_equal(I.SourceTable.slot_records(staged), rec)
    # the crop magnifies the canvas 1.5x to 5x and looks past its edge
    hinv = homographies(rng, B, zoom=(1.5, 5.0), shift=(-10, 30))
    return frames, staged, imgs, hinv


def _against_numpy(frames, staged, imgs, rec, hinv, dh, dw, what):
    H, W = imgs.shape[1:3]
    recs, host = records_of_frames(frames, H, W), imgs.cpu().numpy()
    want = np_crop(recs, rec, host, hinv, dh, dw, np.float64) * 255
    w32 = np_crop(recs, rec, host, hinv, dh, dw, np.float32).astype(np.float64) * 255
    differ = (np.rint(w32) != np.rint(want)).mean()
    outside = (want == 0).all(1).mean()
    print(f"input condition ({what}): the float32 and float64 restatements differ on {100 * differ:.3f} % of the grey levels; "
          f"{100 * outside:.1f} % of the destination lies outside the source")
    assert differ < 0.005 and 0.02 < outside < 0.9
    got = ops.frame_crop(staged.table, _cuda(np.asarray(rec, np.int32)), imgs, _cuda(hinv), dh, dw)
    assert got.shape == (len(rec), 3, dh, dw) and got.dtype == torch.float32
    warp_rule(got.cpu().numpy().astype(np.float64) * 255, want, what)
    return got


@pytest.mark.parametrize("rot", [0, 90, 180, 270])
def test_kernel_matches_the_float64_restatement(rot):
    rng = np.random.RandomState(40 + rot)
    rec, dh, dw = [2, -1, 0, 1, -1], 40, 72            # non-square, no multiple of the 64 x 4 tile
    frames, staged, imgs, hinv = _case(rng, rot, 5, rec, ["rgb24", "bgra32", "nv12"])
    got = _against_numpy(frames, staged, imgs, rec, hinv, dh, dw, f"rotate {rot}")
    # slots without a source: g6d_warp_batch on the same canvas and map, bit for bit
    canvas = ops.warp_batch(imgs, None, torch.arange(5, dtype=torch.int32, device="cuda"), _cuda(hinv), dh, dw)
    assert torch.equal(got[1], canvas[1]) and torch.equal(got[4], canvas[4])
    assert not torch.equal(got[0], canvas[0])


def test_one_slot_128_square():
    rng = np.random.RandomState(50)
    frames, staged, imgs, hinv = _case(rng, 0, 1, [0], ["nv12"])
    _against_numpy(frames, staged, imgs, [0], hinv, 128, 128, "128 x 128")


@pytest.mark.parametrize("dh,dw", [(40, 72), (128, 128)])
def test_slots_without_a_source_equal_warp_batch(dh, dw):
    rng = np.random.RandomState(60)
    B = 5
    imgs = _cuda(rng.randint(0, 256, (B, 96, 128, 3)).astype(np.uint8))
    hinv = _cuda(homographies(rng, B, zoom=(0.5, 5.0)))
    table = torch.zeros(I.RECORD_BYTES, dtype=torch.uint8, device="cuda")          # never read
    rec = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((B, 3, dh, dw), -7.0, device="cuda")
    got = ops.frame_crop(table, rec, imgs, hinv, dh, dw, out=out)
    assert got is out
    want = ops.warp_batch(imgs, None, torch.arange(B, dtype=torch.int32, device="cuda"), hinv, dh, dw)
    assert torch.equal(got, want)
    assert 0.02 < (want == 0).all(1).float().mean().item() < 0.9


def test_bad_arguments_are_rejected_without_a_launch():
    l = lib.load()
    buf = (C.c_uint8 * 96)()
    p = C.addressof(buf)
    for args in ((None, p, p, 1, 8, 8, p, p, 4, 4), (p, None, p, 1, 8, 8, p, p, 4, 4), (p, p, None, 1, 8, 8, p, p, 4, 4),
                 (p, p, p, 1, 8, 8, None, p, 4, 4), (p, p, p, 1, 8, 8, p, None, 4, 4), (p, p, p, 0, 8, 8, p, p, 4, 4),
                 (p, p, p, 1, 0, 8, p, p, 4, 4), (p, p, p, 1, 8, 0, p, p, 4, 4), (p, p, p, 1, 8, 8, p, p, 0, 4), (p, p, p, 1, 8, 8, p, p, 4, 0)):
        assert l.g6d_frame_crop(*args, None) == -1, args                           # G6D_EINVAL before any HIP call
    imgs = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    table = torch.zeros(2 * I.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    rec = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    hinv = torch.eye(3, device="cuda").reshape(1, 9).repeat(2, 1)
    assert ops.frame_crop(table, rec, imgs, hinv, 4, 4).shape == (2, 3, 4, 4)
    for bad in (lambda: ops.frame_crop(table[1:], rec, imgs, hinv, 4, 4),                                 # misaligned table
                lambda: ops.frame_crop(table, rec.long(), imgs, hinv, 4, 4),
                lambda: ops.frame_crop(table, rec[:1], imgs, hinv, 4, 4),
                lambda: ops.frame_crop(table, rec, imgs.float(), hinv, 4, 4),
                lambda: ops.frame_crop(table, rec, imgs, hinv[:1], 4, 4),
                lambda: ops.frame_crop(table, rec, imgs, hinv, 0, 4),
                lambda: ops.frame_crop(table, rec, imgs, hinv, 4, 4, out=torch.zeros((2, 3, 4, 5), device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_crop(table.cpu(), rec.cpu(), imgs.cpu(), hinv.cpu(), 4, 4)
