"""g6d_frame_ingest_area on the MI355X against the numpy restatement of its exact-integer rule (tests/test_minify_cpu.py), bit for bit.
The frames go through the stand-alone entry as hand-made G6dFrame records, so the picture size inside the canvas is free: every
format, turn, a mixed pair of axes, an integer ratio, a footprint of thousands of taps, the largest sums, the two identities (a frame
that does not shrink: g6d_frame_ingest's bytes; a lens frame: g6d_frame_ingest_mesh's) and the launcher's argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from test_minify_cpu import np_ingest_area
from test_pixel_formats_cpu import random_frame

pytestmark = pytest.mark.gpu

_cuda = lambda a: torch.from_numpy(a).cuda()


def table_of(frames, sizes, slots=None):
    """Frames with device planes -> the device table of their records, frame i placed as an out_w x out_h = sizes[i] picture in slot i."""
    t = (lib.G6dFrame * len(frames))()
    for i, (e, f, (ow, oh)) in enumerate(zip(t, frames, sizes)):
        e.plane0, e.plane1 = f.plane0.data_ptr(), (None if f.plane1 is None else f.plane1.data_ptr())
        e.pitch0, e.pitch1, e.width, e.height = f.pitch, f.uv_pitch, f.width, f.height
        e.format, e.rotate, e.matrix, e.slot, e.out_w, e.out_h = I.FORMATS[f.fmt], f.rotate, I.MATRICES[f.matrix], (i if slots is None else slots[i]), ow, oh
        e.K[:] = [float(9 * i + k) for k in range(9)]
    return _cuda(np.frombuffer(t, np.uint8).copy())


def run_area(frames, sizes, H, W, fill=7):
    B = len(frames)
    out = torch.full((B, H, W, 3), fill, dtype=torch.uint8, device="cuda")
    K = torch.full((B, 3, 3), -1.0, device="cuda")
    table = table_of(frames, sizes)
    assert ops.frame_ingest_area(table, None, B, out, K) is out
    np.testing.assert_array_equal(K.cpu().numpy().reshape(B, 9), np.arange(9 * B, dtype=np.float32).reshape(B, 9))
    return out, table


def check(frames, sizes, H, W):
    got = run_area(frames, sizes, H, W)[0].cpu().numpy()
    for i, (f, (ow, oh)) in enumerate(zip(frames, sizes)):
        np.testing.assert_array_equal(got[i], np_ingest_area(f, H, W, ow, oh), err_msg=f"frame {i}: {f.fmt} rotate {f.rotate}")
    return got


# (height, width) of the source -> (out_h, out_w): every axis shrinks by a ratio that is no integer
FORMAT_CASES = {"rgb24": ((37, 50), (17, 23)), "bgr24": ((101, 131), (40, 57)), "rgba32": ((97, 129), (61, 83)), "bgra32": ((388, 516), (97, 129)),
                "nv12": ((388, 516), (90, 125)), "yuyv422": ((51, 70), (22, 31)), "uyvy422": ((200, 300), (77, 101)), "i420": ((120, 160), (50, 70)),
                "yv12": ((260, 350), (97, 120)), "p010": ((98, 130), (41, 53)), "gray8": ((385, 511), (96, 128))}


def test_all_eleven_formats_in_one_launch():
    rng = np.random.RandomState(70)
    assert set(FORMAT_CASES) == set(I.FORMATS)
    frames, sizes = [], []
    for k, (fmt, ((h, w), (oh, ow))) in enumerate(FORMAT_CASES.items()):
        frames.append(random_frame(rng, fmt, h, w, matrix=list(I.MATRICES)[k % 4], extra=6, split=k % 2 == 0, mv=_cuda))
        sizes.append((ow, oh))
    got = check(frames, sizes, 97, 129)                # W % 4 != 0: the byte-store path
    assert (got[0, 17:] == 0).all() and (got[0, :, 23:] == 0).all() and got[0, :17, :23].any()   # black outside the picture


@pytest.mark.parametrize("rot", [0, 90, 180, 270])
def test_rotations(rot):
    rng = np.random.RandomState(71 + rot)
    H, W = (129, 100) if rot in (90, 270) else (100, 129)              # W % 4 == 0 at the quarter turns: the dword-store path
    turned = lambda oh, ow: (oh, ow) if rot in (90, 270) else (ow, oh)  # (out_w, out_h) of a picture that is ow x oh before the turn
    frames = [random_frame(rng, fmt, h, w, matrix=m, extra=4, rotate=rot, mv=_cuda)
              for fmt, (h, w), m in (("bgr24", (120, 200), "bt601"), ("nv12", (150, 260), "bt709"), ("yuyv422", (99, 180), "bt601-full"),
                                     ("p010", (70, 96), "bt709-full"), ("gray8", (301, 257), "bt601"))]
    sizes = [turned(50, 83), turned(61, 100), turned(43, 77), turned(33, 41), turned(97, 100)]
    check(frames, sizes, H, W)


def test_mixed_axes_integer_ratio_and_a_wide_source():
    rng = np.random.RandomState(75)
    mixed = random_frame(rng, "rgb24", 40, 100, extra=3, mv=_cuda)     # 40 rows grow to 60, 100 columns shrink to 37
    check([mixed], [(37, 60)], 64, 40)
    block = rng.randint(0, 256, (48, 64, 3)).astype(np.uint8)          # 64 x 48 -> 16 x 12: the round-half-up mean of every 4 x 4 block
    got = check([I.Frame(_cuda(block), "rgb24")], [(16, 12)], 12, 16)
    np.testing.assert_array_equal(got[0], (2 * block.astype(np.int64).reshape(12, 4, 16, 4, 3).sum((1, 3)) + 16) // 32)
    wide = rng.randint(0, 256, (2, 8192)).astype(np.uint8)             # 8192 x 2 -> 3 x 1: 2731 or 2732 taps per row and pixel
    check([I.Frame(_cuda(wide), "gray8")], [(3, 1)], 8, 128)
    stripes = np.zeros((32, 64, 3), np.uint8)                          # the picture the point rule turns black (4:1)
    stripes[:, 0::4] = stripes[:, 3::4] = 255
    f = I.Frame(_cuda(stripes), "rgb24")
    assert (check([f], [(16, 8)], 8, 16) == 128).all()
    out, K = torch.zeros((1, 8, 16, 3), dtype=torch.uint8, device="cuda"), torch.zeros((1, 3, 3), device="cuda")
    assert (ops.frame_ingest(table_of([f], [(16, 8)]), 1, out, K) == 0).all()


def test_the_largest_sums_saturate():
    """8192 x 8192 all 255 into 8191 x 8191: D = 2^26, Sigma = 255 * 2^26 (the 64-bit sum at its largest, the division at its worst
    divisor); the 130 x 9 canvas sees the picture's corner."""
    white = torch.full((8192, 8192), 255, dtype=torch.uint8, device="cuda")
    out = run_area([I.Frame(white, "gray8")], [(8191, 8191)], 9, 130)[0]
    assert (out == 255).all()


def test_frames_that_do_not_shrink_equal_the_plain_ingest_and_lens_frames_the_mesh_ingest():
    rng = np.random.RandomState(76)
    H, W = 97, 129
    frames = [random_frame(rng, "nv12", 96, 128, extra=8, mv=_cuda), random_frame(rng, "bgra32", 40, 60, extra=4, mv=_cuda),
              random_frame(rng, "i420", 50, 64, matrix="bt709-full", rotate=90, mv=_cuda), random_frame(rng, "rgb24", 200, 300, mv=_cuda)]
    sizes = [(128, 96), (129, 86), (60, 77), (129, 86)]                # same size, magnified, magnified and turned; the last one shrinks
    got, table = run_area(frames, sizes, H, W)
    want = torch.full_like(got, 7)
    ops.frame_ingest(table, 4, want, torch.zeros((4, 3, 3), device="cuda"))
    assert torch.equal(got[:3], want[:3]) and not torch.equal(got[3], want[3])
    # through ingest.ingest_frames_keep: a lens frame keeps the mesh rule bit for bit beside a frame that is filtered
    K = np.array([[300.0, 0, 150], [0, 300.0, 100], [0, 0, 1]])
    lens = I.Frame(frames[3].plane0.reshape(200, 300, 3), K=K, lens=I.Lens("brown", (-0.1, 0.02, 0.001, -0.0005)))
    pair = [lens, frames[3]]
    area, point = (torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    Ka, Kp = (torch.zeros((2, 3, 3), device="cuda") for _ in range(2))
    I.ingest_frames_keep(pair, area, Ka, minify="area")
    I.ingest_frames(pair, point, Kp)
    assert torch.equal(area[0], point[0]) and area[0].any() and torch.equal(Ka, Kp)
    np.testing.assert_array_equal(area[1].cpu().numpy(), np_ingest_area(frames[3], H, W))
    assert not torch.equal(area[1], point[1])


def test_bad_arguments_are_rejected_without_a_launch():
    l = lib.load()
    buf = (C.c_uint8 * 96)()
    p = C.addressof(buf)
    for args in ((None, None, 1, p, 1, 8, 8, p), (p, None, -1, p, 1, 8, 8, p), (p, None, 1, None, 1, 8, 8, p), (p, None, 1, p, 0, 8, 8, p),
                 (p, None, 1, p, 1, 0, 8, p), (p, None, 1, p, 1, 8, 0, p), (p, None, 1, p, 1, 8, 8, None)):
        assert l.g6d_frame_ingest_area(*args, None) == -1, args                    # G6D_EINVAL before any HIP call
    out = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    K = torch.zeros((2, 3, 3), device="cuda")
    table = torch.zeros(2 * I.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    table.view(torch.int32)[[11, 35]] = -1                                         # both records name no slot: nothing is written
    assert ops.frame_ingest_area(table, None, 2, out, K) is out and not out.any()
    meshes = torch.zeros(2 * C.sizeof(lib.G6dMesh), dtype=torch.uint8, device="cuda")
    for bad in (lambda: ops.frame_ingest_area(table[1:], None, 1, out, K),                                # misaligned table
                lambda: ops.frame_ingest_area(table, None, 3, out, K),                                    # more frames than records
                lambda: ops.frame_ingest_area(table, meshes[:24], 2, out, K),                             # a mesh table too short
                lambda: ops.frame_ingest_area(table, meshes.float(), 2, out, K),
                lambda: ops.frame_ingest_area(table, None, 2, out.float(), K),
                lambda: ops.frame_ingest_area(table, None, 2, out, K[:1])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_ingest_area(table.cpu(), None, 2, out.cpu(), K.cpu())
