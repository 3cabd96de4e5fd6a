"""g6d_frame_emit and g6d_track_corners on the MI355X against the numpy restatement of their specification (tests/test_emit_cpu.py), bit
for bit: every format and both matrices, pitched and offset planes, sinks larger and smaller than the picture, odd sizes, boxes partly and
wholly outside, an invalid and a degenerate box, 32 sinks into scattered slots in one launch, full-HD sinks, host sinks.  The tracker with
sinks is covered by tests/test_tracker_emit_gpu.py."""
import numpy as np
import pytest
import torch

from gen6d_amd import emit as E
from gen6d_amd import geometry as G
from gen6d_amd import ingest as I
from gen6d_amd import ops, synth
from test_emit_cpu import BOX, assert_sink, np_corners, np_emit

pytestmark = pytest.mark.gpu

FORMATS = ("rgb24", "bgr24", "rgba32", "bgra32", "nv12")


def make_sink(rng, fmt, w, h, extra=0, offset=0, where="device", **kw):
    """A sink of the format inside a buffer prefilled with 7s: `extra` bytes of row padding, `offset` bytes before the first row; in device
    memory, in pinned host memory ("pinned"), or nv12 as two separate planes (split=True)."""
    split = kw.pop("split", False)
    mk = lambda n: (torch.full((n,), 7, dtype=torch.uint8).pin_memory() if where == "pinned" else torch.full((n,), 7, dtype=torch.uint8, device="cuda"))
    bpp = I.BPP[fmt]
    pitch = w * bpp + extra
    if fmt == "nv12" and split:
        return E.Sink(mk(offset + h * pitch)[offset:], fmt, width=w, height=h, pitch=pitch, uv=mk(h // 2 * (w + 16)), uv_pitch=w + 16, **kw)
    rows = h * 3 // 2 if fmt == "nv12" else h
    return E.Sink(mk(offset + rows * pitch)[offset:], fmt, width=w, height=h, pitch=pitch, **kw)


def corner_sets(B, H, W):
    """[2,B,8,2] corners and [2,B] validity: boxes inside, partly outside, wholly outside, invalid, degenerate (two corners on a pixel)."""
    rng = np.random.RandomState(5)
    pts, valid = np.zeros((2, B, 8, 2), np.int32), np.ones((2, B), np.int32)
    for k in range(2):
        for b in range(B):
            kind = (b + k) % 5
            q = np.stack([rng.randint(2, W - 2, 8), rng.randint(2, H - 2, 8)], -1)
            if kind == 1:
                q = q * 3 - [W, H]                                   # partly outside, long edges crossing the picture
            elif kind == 2:
                q = q + [3 * W, -2 * H]                              # wholly outside
            elif kind == 3:
                valid[k, b] = 0
            elif kind == 4:
                q[1] = q[0]
                q[6] = q[2]                                          # degenerate edges 0-1 and 2-6
            pts[k, b] = q
    return pts, valid


def run_and_check(imgs, pts, valid, sinks, slots, sizes, msg=""):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    E.emit_frames(d(imgs), d(pts), d(valid), sinks, slots=slots, pic_sizes=sizes)
    torch.cuda.synchronize()
    for s, b, hw in zip(sinks, slots, sizes):
        k = E.POSES[s.pose]
        assert_sink(s, np_emit(imgs[b], pts[k, b] if valid[k, b] else None, s, hw), f"{msg} slot {b} {s.fmt} {s.width}x{s.height} {s.pose}")


def test_every_format_and_matrix_matches_numpy():
    rng = np.random.RandomState(0)
    for H, W in ((96, 128), (50, 67), (33, 260)):        # dword-aligned canvas rows, the byte path, more than two tiles across
        B = 6
        imgs = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        pts, valid = corner_sets(B, H, W)
        pts[0, 0] = BOX
        sinks, slots, sizes = [], [], []
        for fi, fmt in enumerate(FORMATS):
            for v in range(6):
                even = 2 if fmt == "nv12" else 1
                w, h = ((W, H), (W + 37, H + 11), (W - 21, H - 9), (W, H), (W + 4, H), (W - 1, H + 1))[v]
                w, h = w // even * even, h // even * even
                sinks.append(make_sink(rng, fmt, w, h, extra=(0, 13, 8, 3, 0, 16)[v], offset=(0, 5, 0, 64, 2, 0)[v], matrix=("bt601", "bt709")[v % 2],
                                       pose=("raw", "smooth")[(v + fi) % 2], where="pinned" if v == 3 else "device", split=v == 4))
                slots.append((v + fi) % B)
                sizes.append(((H, W), (H, W), (H - 3, W - 5), (H - 1, W - 1), (H, W), (H // 2, W // 2))[v])   # odd pictures included
        sinks.append(make_sink(rng, "rgb24", W, H, thickness=7, dot_radius=5, line_color=(10, 200, 30), dot_color=(1, 2, 3)))
        sinks.append(make_sink(rng, "nv12", W // 2 * 2, H // 2 * 2, thickness=1, dot_radius=0, box=True))
        sinks.append(make_sink(rng, "bgra32", W, H, box=False))
        slots += [1, 1, 0]
        sizes += [(H, W)] * 3
        run_and_check(imgs, pts, valid, sinks, slots, sizes, f"canvas {H}x{W}")
    # the row padding and the bytes before a device sink are not written
    s = make_sink(rng, "rgb24", 40, 20, extra=9, offset=3)
    run_and_check(imgs, pts, valid, [s], [0], [(H, W)])
    whole = torch.as_strided(s.plane0, (3 + 20 * 129,), (1,), 0).cpu().numpy()
    assert (whole[:3] == 7).all() and (whole[3:][:19 * 129].reshape(19, 129)[:, 120:] == 7).all()
    # a pitched host sink travels in one copy: the bytes before it are kept, its row padding receives zeros, never stale device memory
    s = make_sink(rng, "rgb24", 40, 20, extra=9, offset=3, where="pinned")
    run_and_check(imgs, pts, valid, [s], [0], [(H, W)])
    whole = torch.as_strided(s.plane0, (3 + 20 * 129,), (1,), 0).numpy()
    assert (whole[:3] == 7).all() and (whole[3:][:19 * 129].reshape(19, 129)[:, 120:] == 0).all()


def test_32_sinks_into_scattered_slots():
    rng = np.random.RandomState(2)
    H, W, B = 96, 128, 40
    imgs = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    pts, valid = corner_sets(B, H, W)
    sinks, slots, sizes = [], [int(s) for s in rng.permutation(B)[:32]], []
    for i in range(32):
        fmt = FORMATS[rng.randint(0, 5)]
        w, h = int(rng.randint(20, 200)) & ~1, int(rng.randint(20, 160)) & ~1
        sinks.append(make_sink(rng, fmt, w, h, extra=int(rng.randint(0, 2)) * 11, where=("device", "pinned")[rng.randint(0, 2)],
                               matrix=("bt601", "bt709")[rng.randint(0, 2)], pose=("raw", "smooth")[rng.randint(0, 2)]))
        sizes.append((int(rng.randint(H // 2, H + 1)), int(rng.randint(W // 2, W + 1))))
    run_and_check(imgs, pts, valid, sinks, slots, sizes)


@pytest.mark.parametrize("canvas", [(540, 960), (1080, 1920)])
def test_full_hd_nv12_sink(canvas):
    """A 1080p NV12 sink from a 540x960 canvas (four times the canvas's tiles: the strided walk, black padding) and from a 1080p one."""
    rng = np.random.RandomState(3)
    H, W = canvas
    imgs = rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    pts, valid = corner_sets(2, H, W)
    pts[1, 1] = BOX * (H // 60) + [W // 3, H // 4]
    valid[1, 1] = 1
    sinks = [make_sink(rng, "nv12", 1920, 1080, extra=128, matrix="bt709"), make_sink(rng, "rgb24", 1920, 1080)]
    run_and_check(imgs, pts, valid, sinks, [1, 1], [(H, W), (H - 1, W - 3)], f"canvas {H}x{W}")


def test_track_corners_against_float64_numpy():
    """Equal to numpy's float64 projection except where the float64 coordinate lies within 1e-6 of a rounding boundary; such coordinates
    are capped at 1 % of all tested (numpy alone: random poses put a coordinate that close to k + 0.5 about once in 500,000)."""
    rng = np.random.RandomState(0)
    poses, Ks = synth.fibonacci_cameras(40, radius=3.0, focal=300.0, size=256)
    box = G.box_corners(rng.uniform(-0.5, 0.5, (100, 3))).astype(np.float32)
    S, B = 64, 32
    table = np.stack([synth.perturb_pose(poses[s % 40], rng.uniform(-5, 5), rng.uniform(-0.05, 0.05)) for s in range(S)]).reshape(S, 12).astype(np.float32)
    table[5, 11] = -3.0                                                 # behind the camera
    table[6, 3] = 400.0                                                 # far outside the corner range
    table[7, 0] = np.nan
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    near = total = 0
    for rep in range(4):
        m = rng.permutation(S)[:B].astype(np.int32)
        m[rng.randint(0, B, 3)] = -1
        if rep == 0:
            m[:3] = (5, 6, 7)
        K = np.stack([Ks[b % 40] for b in range(B)]).astype(np.float32)
        pts = torch.full((B, 8, 2), 99, dtype=torch.int32, device="cuda")
        got, ok = ops.track_corners(d(table), d(K), d(m), d(box), pts=pts)
        assert got is pts
        got, ok = got.cpu().numpy(), ok.cpu().numpy()
        for b, s in enumerate(m):
            if s < 0:
                assert ok[b] == 0 and not got[b].any()
                continue
            q, v, uv = np_corners(box, table[s], K[b])
            assert ok[b] == v, (rep, b, s)
            if not v:
                assert not got[b].any()
                continue
            edge = np.abs(uv + 0.5 - np.rint(uv + 0.5)) <= 1e-6
            near += int(edge.sum())
            total += edge.size
            np.testing.assert_array_equal(got[b][~edge], q[~edge], err_msg=f"slot {b} stream {s}")
            assert (np.abs(got[b] - q) <= 1).all()
        if rep == 0:
            assert list(ok[:3]) == [0, 0, 0]
    assert total > 1000 and near * 100 <= total
    with pytest.raises(ValueError):
        ops.track_corners(d(table), d(K), d(m).long(), d(box))
    with pytest.raises(ValueError):
        ops.frame_emit(torch.zeros(71, dtype=torch.uint8, device="cuda"), 1, torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"),
                       torch.zeros((1, 1, 8, 2), dtype=torch.int32, device="cuda"), torch.zeros((1, 1), dtype=torch.int32, device="cuda"))
