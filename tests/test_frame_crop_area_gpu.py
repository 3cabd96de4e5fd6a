"""g6d_frame_crop_area on the MI355X: against the numpy restatement of its rule (tests/test_minify_cpu.py np_crop_area) in float64 under
the project's warp rule, with the shapes and the record mix of tests/test_frame_crop_gpu.py and maps that minify; bit equality with
g6d_frame_crop where a crop magnifies (n = 1), slots without a source included; the cap; the launcher's argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from test_frame_crop_cpu import homographies, records_of_frames, source_frame, warp_rule
from test_minify_cpu import np_crop_area, np_samples_per_slot

pytestmark = pytest.mark.gpu

_cuda = lambda a: torch.from_numpy(a).cuda()
ZOOM = (1 / 6, 1 / 1.6)                                # a crop pixel covers 1.6 to 6 canvas pixels
# seeds for which the restatement alone meets the input condition below (checked on the CPU: _inputs with mv = identity)
SEEDS = {0: 100, 90: 190, 180: 280, 270: 370, "square": 150}


def _inputs(rng, rot, B, kinds, zoom, mv):
    """test_frame_crop_gpu._case without the ingest: frames of `kinds` turned by `rot`, B noise canvases (97 x 129, turned with the
    frames) and B maps -> (frames, imgs uint8 numpy, hinv).  The canvases of slots with a record are never read."""
    H, W = (129, 97) if rot in (90, 270) else (97, 129)
    make = {"rgb24": lambda: source_frame(rng, 50, 70, "rgb24", rot, mv=mv),
            "bgra32": lambda: source_frame(rng, 97, 129, "bgra32", rot, extra=24, mv=mv),
            "nv12": lambda: source_frame(rng, 388, 516, "nv12", rot, extra=32, matrix=("bt601", "bt709")[rot in (90, 270)], split=True, mv=mv)}
    frames = [make[k]() for k in kinds]
    imgs = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    return frames, imgs, homographies(rng, B, zoom=zoom, shift=(-10, 30))


def input_condition(frames, imgs, rec, hinv, dh, dw, what, max_n=8):
    """test_frame_crop_gpu's input condition on the restatement alone -> (float64 grey levels, n per slot)."""
    H, W = imgs.shape[1:3]
    recs = records_of_frames(frames, H, W)
    want = np_crop_area(recs, rec, imgs, hinv, dh, dw, max_n, np.float64) * 255
    w32 = np_crop_area(recs, rec, imgs, hinv, dh, dw, max_n, np.float32).astype(np.float64) * 255
    differ = (np.rint(w32) != np.rint(want)).mean()
    outside = (want == 0).all(1).mean()
    ns = np_samples_per_slot(recs, rec, H, W, hinv, dh, dw, max_n)
    print(f"input condition ({what}): n per slot {ns}; the float32 and float64 restatements differ on {100 * differ:.3f} % of the grey "
          f"levels; {100 * outside:.1f} % of the destination lies outside the source")
    assert differ < 0.005 and 0.02 < outside < 0.9
    return want, ns


def _table(frames, rec, B, H, W):
    """The frames' records on the device (planned for the canvas, as ingest_frames_keep leaves them) and the slot map."""
    imgs = torch.zeros((B, H, W, 3), dtype=torch.uint8, device="cuda")
    staged = I.ingest_frames_keep(frames, imgs, torch.empty((B, 3, 3), device="cuda"), slots=[rec.index(i) for i in range(len(frames))])[1]
    np.testing.assert_array_equal(I.SourceTable.slot_records(staged), rec)
    return staged


@pytest.mark.parametrize("rot", [0, 90, 180, 270])
def test_kernel_matches_the_float64_restatement(rot):
    rng = np.random.RandomState(SEEDS[rot])
    rec, dh, dw = [2, -1, 0, 1, -1], 40, 72            # non-square, no multiple of the 64 x 4 tile
    frames, imgs, hinv = _inputs(rng, rot, 5, ["rgb24", "bgra32", "nv12"], ZOOM, _cuda)
    want, ns = input_condition(frames, imgs, rec, hinv, dh, dw, f"rotate {rot}")
    assert all(2 <= ns[b] <= 6 for b in (1, 3, 4)) and ns[0] == 8      # canvas and same-size slots; the 4x larger nv12 source is capped
    staged = _table(frames, rec, 5, *imgs.shape[1:3])
    got = ops.frame_crop_area(staged.table, _cuda(np.asarray(rec, np.int32)), _cuda(imgs), _cuda(hinv), dh, dw)
    assert got.shape == (5, 3, dh, dw) and got.dtype == torch.float32
    warp_rule(got.cpu().numpy().astype(np.float64) * 255, want, f"rotate {rot}")


def test_one_slot_128_square():
    rng = np.random.RandomState(SEEDS["square"])
    frames, imgs, hinv = _inputs(rng, 0, 1, ["nv12"], ZOOM, _cuda)
    want, ns = input_condition(frames, imgs, [0], hinv, 128, 128, "128 x 128")
    assert 6 <= ns[0] <= 8                            # the 4x larger source: at least 4 x 1.6 source pixels per crop pixel
    staged = _table(frames, [0], 1, *imgs.shape[1:3])
    got = ops.frame_crop_area(staged.table, _cuda(np.zeros(1, np.int32)), _cuda(imgs), _cuda(hinv), 128, 128)
    warp_rule(got.cpu().numpy().astype(np.float64) * 255, want, "128 x 128")


@pytest.mark.parametrize("rot", [0, 270])
def test_magnifying_crops_equal_the_point_crop(rot):
    """n = 1 in every slot: g6d_frame_crop's bits, for slots with a source and for slots served from their canvas."""
    rng = np.random.RandomState(160 + rot)
    rec, dh, dw = [2, -1, 0, 1, -1], 40, 72
    frames, imgs, hinv = _inputs(rng, rot, 5, ["rgb24", "bgra32", "bgra32"], (1.5, 5.0), _cuda)
    H, W = imgs.shape[1:3]
    assert np_samples_per_slot(records_of_frames(frames, H, W), rec, H, W, hinv, dh, dw, 8) == [1] * 5
    staged = _table(frames, rec, 5, H, W)
    args = (staged.table, _cuda(np.asarray(rec, np.int32)), _cuda(imgs), _cuda(hinv), dh, dw)
    want = ops.frame_crop(*args)
    out = torch.full((5, 3, dh, dw), -7.0, device="cuda")
    got = ops.frame_crop_area(*args, max_n=8, out=out)
    assert got is out and torch.equal(got, want)
    assert 0.02 < (want == 0).all(1).float().mean().item() < 0.9


def test_max_n_caps_the_samples():
    rng = np.random.RandomState(170)
    rec, dh, dw = [0, -1], 16, 24
    frames, imgs, hinv = _inputs(rng, 0, 2, ["bgra32"], (1 / 5, 1 / 4), _cuda)
    H, W = imgs.shape[1:3]
    recs = records_of_frames(frames, H, W)
    assert min(np_samples_per_slot(recs, rec, H, W, hinv, dh, dw, 8)) >= 4
    staged = _table(frames, rec, 2, H, W)
    args = (staged.table, _cuda(np.asarray(rec, np.int32)), _cuda(imgs), _cuda(hinv), dh, dw)
    got2, got8 = ops.frame_crop_area(*args, max_n=2), ops.frame_crop_area(*args, max_n=8)
    warp_rule(got2.cpu().numpy().astype(np.float64) * 255, np_crop_area(recs, rec, imgs, hinv, dh, dw, 2, np.float64) * 255, "max_n = 2")
    warp_rule(got8.cpu().numpy().astype(np.float64) * 255, np_crop_area(recs, rec, imgs, hinv, dh, dw, 8, np.float64) * 255, "max_n = 8")
    assert torch.equal(ops.frame_crop_area(*args, max_n=1), ops.frame_crop(*args))
    assert not torch.equal(got2, got8)


def test_degenerate_maps_take_one_sample():
    """A parked slot's map may be anything: NaN, zero and overflowing maps give g6d_frame_crop's values (NaN compares unequal: bytes)."""
    imgs = _cuda(np.random.RandomState(171).randint(0, 256, (3, 32, 48, 3)).astype(np.uint8))
    hinv = torch.tensor([[float("nan")] * 9, [0.0] * 9, [3e38, 0, 0, 0, 3e38, 0, 0, 0, 1e-38]], device="cuda")
    table = torch.zeros(I.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    rec = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    got, want = ops.frame_crop_area(table, rec, imgs, hinv, 20, 28), ops.frame_crop(table, rec, imgs, hinv, 20, 28)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_bad_arguments_are_rejected_without_a_launch():
    l = lib.load()
    buf = (C.c_uint8 * 96)()
    p = C.addressof(buf)
    for args in ((None, p, p, 1, 8, 8, p, p, 4, 4, 8), (p, None, p, 1, 8, 8, p, p, 4, 4, 8), (p, p, None, 1, 8, 8, p, p, 4, 4, 8),
                 (p, p, p, 1, 8, 8, None, p, 4, 4, 8), (p, p, p, 1, 8, 8, p, None, 4, 4, 8), (p, p, p, 0, 8, 8, p, p, 4, 4, 8),
                 (p, p, p, 1, 0, 8, p, p, 4, 4, 8), (p, p, p, 1, 8, 0, p, p, 4, 4, 8), (p, p, p, 1, 8, 8, p, p, 0, 4, 8),
                 (p, p, p, 1, 8, 8, p, p, 4, 0, 8), (p, p, p, 1, 8, 8, p, p, 4, 4, 0), (p, p, p, 1, 8, 8, p, p, 4, 4, 9)):
        assert l.g6d_frame_crop_area(*args, None) == -1, args                      # G6D_EINVAL before any HIP call
    imgs = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    table = torch.zeros(2 * I.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    rec = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    hinv = torch.eye(3, device="cuda").reshape(1, 9).repeat(2, 1)
    assert ops.frame_crop_area(table, rec, imgs, hinv, 4, 4).shape == (2, 3, 4, 4)
    for bad in (lambda: ops.frame_crop_area(table[1:], rec, imgs, hinv, 4, 4),                            # misaligned table
                lambda: ops.frame_crop_area(table, rec.long(), imgs, hinv, 4, 4),
                lambda: ops.frame_crop_area(table, rec[:1], imgs, hinv, 4, 4),
                lambda: ops.frame_crop_area(table, rec, imgs.float(), hinv, 4, 4),
                lambda: ops.frame_crop_area(table, rec, imgs, hinv[:1], 4, 4),
                lambda: ops.frame_crop_area(table, rec, imgs, hinv, 0, 4),
                lambda: ops.frame_crop_area(table, rec, imgs, hinv, 4, 4, max_n=0),
                lambda: ops.frame_crop_area(table, rec, imgs, hinv, 4, 4, max_n=9),
                lambda: ops.frame_crop_area(table, rec, imgs, hinv, 4, 4, out=torch.zeros((2, 3, 4, 5), device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_crop_area(table.cpu(), rec.cpu(), imgs.cpu(), hinv.cpu(), 4, 4)
