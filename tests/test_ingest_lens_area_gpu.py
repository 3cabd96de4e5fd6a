"""Lens frames of g6d_frame_ingest_area on the MI355X against the numpy restatement of the supersampling rule
(tests/test_ingest_lens_area_cpu.py), bit for bit.  Most frames go through the stand-alone entry as hand-made G6dFrame / G6dMesh records, so
the picture is 150 x 52 inside a 160 x 56 canvas at every turn (it crosses a tile edge in x and in y, the last tile of a row is partial) and
samples_log2 is free; a 150 x 52 picture in a 157 x 56 canvas has byte-store rows.  Formats x turns x n, every mesh step, a border that
cuts through pixels, a mixed launch through ingest_frames_keep, the two consequences against the kernels they reduce to, a guarded arena,
and the tracker."""
import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from guarded import arena
from test_ingest_cpu import nv12_of
from test_ingest_lens_area_cpu import SUITE_LENS, ZERO, np_ingest_lens_area, np_mesh_area_coords, np_mesh_area_picture
from test_ingest_lens_cpu import BARREL, PINCUSHION, camera
from test_minify_cpu import np_ingest_area, record_rgb
from test_pixel_formats_cpu import host_record, random_frame
from test_track_streams_gpu import _seqs, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_cuda = lambda a: torch.from_numpy(a).to(DEV)
PW, PH = 150, 52                                         # the picture
H, W = 56, 160                                           # the canvas: 2 x 7 tiles of 128 x 8


def lens_frame(rng, fmt, k, rot, lens=SUITE_LENS, f=0.55, tol=1 / 16, matrix="bt601", lo=0, **kw):
    """A noise frame k times the picture (turned back by `rot`) of a camera with `lens`, focal length f times the longer side."""
    w, h = (PH * k, PW * k) if rot in (90, 270) else (PW * k, PH * k)
    cam = dict(rotate=rot, K=camera(w, h, f * max(w, h)), lens=I.Lens(lens[0], lens[1], tol=tol, minify="area"))
    if lo:                                               # (rgb24 only) no pixel darker than lo
        return I.Frame(_cuda(rng.randint(lo, 256, (h, w, 3)).astype(np.uint8)), **cam)
    return random_frame(rng, fmt, h, w, matrix=matrix, mv=_cuda, **cam, **kw)


def mesh_for(f):
    """-> (nodes, step_log2, L the host would choose) of a lens frame whose picture is PW x PH."""
    nodes, lg = f.lens.mesh(f.K, f.width, f.height, f.rotate, PW, PH)
    return nodes, lg, I.Lens.samples_log2(nodes, lg, f.width, f.height)


def tables(frames, meshes, slots=None, keep=None):
    """Device frames + per frame (nodes, step_log2, L) or None -> the device frame table and mesh table, every picture PW x PH."""
    t, m = (lib.G6dFrame * len(frames))(), (lib.G6dMesh * len(frames))()
    for i, (f, ms) in enumerate(zip(frames, meshes)):
        e = t[i]
        e.plane0, e.plane1 = f.plane0.data_ptr(), (None if f.plane1 is None else f.plane1.data_ptr())
        e.pitch0, e.pitch1, e.width, e.height = f.pitch, f.uv_pitch, f.width, f.height
        e.format, e.rotate, e.matrix, e.slot, e.out_w, e.out_h = I.FORMATS[f.fmt], f.rotate, I.MATRICES[f.matrix], (i if slots is None else slots[i]), PW, PH
        e.K[:] = [float(9 * i + j) for j in range(9)]
        if ms is not None:
            nodes = ms[0] if torch.is_tensor(ms[0]) else _cuda(np.ascontiguousarray(ms[0]))
            keep.append(nodes)
            m[i].nodes, m[i].ny, m[i].nx, m[i].step_log2, m[i].samples_log2 = nodes.data_ptr(), nodes.shape[0], nodes.shape[1], ms[1], ms[2]
    return _cuda(np.frombuffer(t, np.uint8).copy()), _cuda(np.frombuffer(m, np.uint8).copy())


def run(frames, meshes, Hc=H, Wc=W, out=None, fill=7):
    keep = []
    table, mtable = tables(frames, meshes, keep=keep)
    if out is None:
        out = torch.full((len(frames), Hc, Wc, 3), fill, dtype=torch.uint8, device=DEV)
    K = torch.full((len(frames), 3, 3), -1.0, device=DEV)
    assert ops.frame_ingest_area(table, mtable, len(frames), out, K) is out
    got = out.cpu().numpy()                               # (synchronises: `keep` lives until here)
    np.testing.assert_array_equal(K.cpu().numpy().reshape(-1, 9), np.arange(9 * len(frames), dtype=np.float32).reshape(-1, 9))
    return got, table, mtable, keep


def want(f, ms, Hc=H, Wc=W):
    nodes = ms[0].cpu().numpy() if torch.is_tensor(ms[0]) else ms[0]
    return np_mesh_area_picture(record_rgb(host_record(f, Hc, Wc)), nodes, ms[1], ms[2], PW, PH, Hc, Wc)


def check(frames, meshes, Hc=H, Wc=W):
    got = run(frames, meshes, Hc, Wc)[0]
    for i, (f, ms) in enumerate(zip(frames, meshes)):
        np.testing.assert_array_equal(got[i], want(f, ms, Hc, Wc), err_msg=f"frame {i}: {f.fmt} {f.width}x{f.height} rotate {f.rotate} step {1 << ms[1]} L {ms[2]}")
        assert got[i, :PH, :PW].any() and not got[i, PH:].any() and not got[i, :, PW:].any()
    return got


FORMATS = ("rgb24", "nv12", "yuyv422", "p010", "i420", "bgra32")
TURNS = (0, 90, 180, 270)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_formats_turns_and_sample_counts(k):
    """Sources 300 x 104 (n = 2), 600 x 208 (n = 4) and 1200 x 416 (n = 8) behind the suite's lens: at 2:1 every format at every turn, at
    4:1 every format once and at 8:1 the first four, every turn among them (the restatement of an 8:1 frame sums half a million samples)."""
    rng = np.random.RandomState(40 + k)
    pairs = [(fmt, rot) for fmt in FORMATS for rot in TURNS] if k == 2 else [(fmt, TURNS[(i + k // 8) % 4]) for i, fmt in enumerate(FORMATS[:6 if k == 4 else 4])]
    frames = [lens_frame(rng, fmt, k, rot, extra=(0, 6)[i % 2], matrix=list(I.MATRICES)[i % 4], split=i % 3 == 0) for i, (fmt, rot) in enumerate(pairs)]
    meshes = [mesh_for(f) for f in frames]
    assert {1 << ms[2] for ms in meshes} == {k}                      # the host's choice
    check(frames, meshes)


def test_byte_store_rows_and_every_sample_count_on_one_source():
    """W = 157: no canvas row but every fourth starts on a dword, and the last thread of a row has one pixel.  The field is the kernel's
    to obey, whatever the ratio: L = 1, 2, 3 and a value past the clamp on a 4:1 source."""
    rng = np.random.RandomState(50)
    frames = [lens_frame(rng, fmt, 4, rot, extra=3) for fmt, rot in (("nv12", 0), ("rgb24", 270), ("uyvy422", 180), ("p010", 90), ("gray8", 0))]
    meshes = [mesh_for(f)[:2] + (L,) for f, L in zip(frames, (1, 2, 3, 3, 1))]
    check(frames, meshes, 56, 157)
    past = [mesh_for(f)[:2] + (L,) for f, L in zip(frames[:2], (9, -4))]       # clamped to 3 and to 0
    got = run(frames[:2], past, 56, 157)[0]
    np.testing.assert_array_equal(got[0], want(frames[0], past[0][:2] + (3,), 56, 157))
    np.testing.assert_array_equal(got[1], want(frames[1], past[1][:2] + (0,), 56, 157))


@pytest.mark.parametrize("tol,step", [(1 / 64, 2), (1 / 16, 4), (1 / 4, 8), (4.0, 16)])
def test_every_mesh_step(tol, step):
    """The strong barrel lens at f = 0.4 of the longer side; tol chooses the step.  Step 2: every other pixel reaches into the cell before
    its own; step 16: a tile inside one row of cells, its pixels of rows 16 m reaching into the row above."""
    rng = np.random.RandomState(51)
    frames = [lens_frame(rng, fmt, 4, rot, lens=BARREL, f=0.4, tol=tol, extra=2) for fmt, rot in (("nv12", 0), ("bgra32", 90), ("yv12", 180))]
    meshes = [mesh_for(f) for f in frames]
    assert {1 << ms[1] for ms in meshes} == {step}, [1 << ms[1] for ms in meshes]
    check(frames, meshes)


def test_a_border_that_cuts_through_pixels():
    """The pincushion lens at f = 0.52 ws looks past the source at the corners: black sub-samples count as 0 in a pixel's mean, so the
    border is a ramp.  No source pixel is black itself (values 17..255)."""
    rng = np.random.RandomState(52)
    frames = [lens_frame(rng, "rgb24", 4, 0, lens=PINCUSHION, f=0.52, lo=17), lens_frame(rng, "nv12", 2, 90, lens=PINCUSHION, f=0.52)]
    meshes = [mesh_for(f) for f in frames]
    got = check(frames, meshes)
    f, (nodes, lg, L) = frames[0], meshes[0]
    fx, fy = np_mesh_area_coords(nodes, lg, L, PW, PH)
    inside = (fx >= -1024) & (fx <= (f.width - 1) * 2048 + 1024) & (fy >= -1024) & (fy <= (f.height - 1) * 2048 + 1024)
    share = inside.reshape(PH, 1 << L, PW, 1 << L).mean((1, 3))
    assert ((share > 0) & (share < 1)).sum() > 20 and (share == 0).mean() > 0.05 and (share == 1).mean() > 0.3
    assert not got[0, :PH, :PW][share == 0].any() and got[0, :PH, :PW][share == 1].all(-1).all()


def test_three_rules_in_one_launch_into_scattered_slots():
    """ingest_frames_keep(minify="area") on a plain frame that shrinks, a lens frame with the default and two with minify="area" (8:1 and
    2:1): each slot holds its own rule's bytes, slots no frame names keep theirs."""
    rng = np.random.RandomState(53)
    I._meshes.clear()
    Hc, Wc, B = 56, 160, 7
    K = camera(600, 208, 330.0)
    plain = random_frame(rng, "nv12", 208, 600, extra=8, mv=_cuda)
    default = random_frame(rng, "i420", 208, 600, mv=_cuda, K=K, lens=I.Lens(*SUITE_LENS))
    area8 = random_frame(rng, "bgr24", 416, 1200, extra=3, mv=_cuda, K=camera(1200, 416, 660.0), lens=I.Lens(*SUITE_LENS, minify="area"))
    area2 = random_frame(rng, "p010", 300, 104, mv=_cuda, rotate=270, K=camera(104, 300, 165.0), lens=I.Lens(*SUITE_LENS, minify="area"))
    frames, slots = [plain, default, area8, area2], [5, 0, 3, 6]
    out = torch.full((B, Hc, Wc, 3), 9, dtype=torch.uint8, device=DEV)
    Ko = torch.full((B, 3, 3), -7.0, device=DEV)
    I.ingest_frames_keep(frames, out, Ko, slots=slots, minify="area")
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[5], np_ingest_area(plain, Hc, Wc))
    np.testing.assert_array_equal(got[0], np_ingest_lens_rgb(default, Hc, Wc))
    np.testing.assert_array_equal(got[3], np_ingest_lens_area(area8, Hc, Wc))
    np.testing.assert_array_equal(got[6], np_ingest_lens_area(area2, Hc, Wc))
    for s in (1, 2, 4):
        assert (got[s] == 9).all() and (Ko[s] == -7.0).all()
    for f, s in zip(frames, slots):
        np.testing.assert_array_equal(Ko[s].cpu().numpy(), I.plan(f, (Hc, Wc))[2].astype(np.float32))
    point = torch.zeros_like(out)                                       # under "point" the setting changes nothing
    I.ingest_frames(frames, point, Ko, slots=slots)
    assert torch.equal(point[0], out[0]) and not torch.equal(point[3], out[3])
    np.testing.assert_array_equal(point[3].cpu().numpy(), np_ingest_lens_area(area8, Hc, Wc, L=0))


def np_ingest_lens_rgb(frame, Hc, Wc):
    """np_ingest_lens for a frame of any format: the mesh rule is the supersampling rule with one sample (test_ingest_lens_area_cpu)."""
    return np_ingest_lens_area(frame, Hc, Wc, L=0)


def test_one_sample_equals_the_mesh_entry():
    """Consequence 1 on the device: samples_log2 = 0 through g6d_frame_ingest_area gives g6d_frame_ingest_mesh's bytes."""
    rng = np.random.RandomState(54)
    frames = [lens_frame(rng, fmt, 4, rot, extra=4) for fmt, rot in (("nv12", 0), ("rgba32", 90), ("yuyv422", 270))]
    meshes = [mesh_for(f)[:2] + (0,) for f in frames]
    got, table, mtable, keep = run(frames, meshes)
    ref = torch.full((3, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    ops.frame_ingest_mesh(table, mtable, 3, ref, torch.zeros((3, 3, 3), device=DEV))
    np.testing.assert_array_equal(got, ref.cpu().numpy())
    np.testing.assert_array_equal(got[0], want(frames[0], meshes[0]))


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_a_lens_that_does_nothing_equals_the_area_entry(k):
    """Consequence 2 on the device: k x k block means, the bytes g6d_frame_ingest_area writes for the same frames without a lens."""
    rng = np.random.RandomState(56 + k)
    K = np.array([[0.7 * PW * k, 0, 0.41 * PW * k], [0, 0.66 * PW * k, 0.57 * PH * k], [0, 0, 1.0]])
    zf = [random_frame(rng, fmt, PH * k, PW * k, extra=6, mv=_cuda, K=K, lens=I.Lens(*ZERO, minify="area")) for fmt in ("rgb24", "nv12", "p010")]
    zm = [mesh_for(f) for f in zf]
    assert all(ms[1] == 4 and 1 << ms[2] == k for ms in zm)
    lens_bytes, table, _, _ = run(zf, zm)
    bare = torch.full((3, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    ops.frame_ingest_area(table, None, 3, bare, torch.zeros((3, 3, 3), device=DEV))
    np.testing.assert_array_equal(lens_bytes, bare.cpu().numpy())
    np.testing.assert_array_equal(lens_bytes[0], want(zf[0], zm[0]))


def test_inside_guarded_arenas():
    """The canvas and the mesh nodes in arenas (tests/guarded.py): nothing is written beside the canvas, and a node read from a guard
    (2^31 - 1: far outside every source) would turn pixels black that the restatement has."""
    rng = np.random.RandomState(55)
    frames = [lens_frame(rng, "nv12", 4, 0, lens=BARREL, f=0.4, tol=1 / 64), lens_frame(rng, "rgb24", 2, 180, tol=4.0)]
    meshes = [mesh_for(f) for f in frames]
    assert [ms[1] for ms in meshes] == [1, 4]
    node_arenas = [arena(ms[0].shape, torch.int32, device=DEV) for ms in meshes]
    in_arena = [(a.set(torch.from_numpy(ms[0])), ms[1], ms[2]) for a, ms in zip(node_arenas, meshes)]
    canvas = arena((2, H, W, 3), torch.uint8, device=DEV)
    canvas.view.fill_(7)
    got = run(frames, in_arena, out=canvas.view)[0]
    for i, (f, ms) in enumerate(zip(frames, meshes)):
        np.testing.assert_array_equal(got[i], want(f, ms))
    assert canvas.untouched(), canvas.touched()[:8]
    assert all(a.untouched() for a in node_arenas)


# ---------------------------------------------------------------------------------------------------------------- tracker
LENS = I.Lens("brown", (-0.12, 0.03, 0.001, -0.0005, 0.0), minify="area")
UP = np.array([[2.0, 0, 0.5], [0, 2.0, 0.5], [0, 0, 1]])          # the scene's pixel coordinates -> those of the 2x larger source


def _camera_frame(frame, K, device=False):
    """test_ingest_lens_gpu._camera_frame with the area setting: a scene frame [h,w,3] -> the 2x larger pitched NV12 frame of a camera
    with LENS (BT.601 limited range, one chroma sample per scene pixel)."""
    g = frame.astype(np.int64)
    Y = ((66 * g[..., 0] + 129 * g[..., 1] + 25 * g[..., 2] + 128) >> 8) + 16
    U = ((-38 * g[..., 0] - 74 * g[..., 1] + 112 * g[..., 2] + 128) >> 8) + 128
    V = ((112 * g[..., 0] - 94 * g[..., 1] - 18 * g[..., 2] + 128) >> 8) + 128
    w = 2 * frame.shape[1]
    buf = nv12_of(np.repeat(np.repeat(Y, 2, 0), 2, 1).astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8), pitch=w + 32)
    return I.Frame(torch.from_numpy(buf).cuda() if device else buf, "nv12", width=w, K=UP @ np.asarray(K, np.float64), lens=LENS)


@pytest.mark.parametrize("graphs", [True, False])
def test_tracker_on_area_lens_frames(scene, graphs):
    """StreamTracker(minify="area") on 2:1 lens frames (n = 2) returns exactly the poses of one fed the restatement's canvases as plain
    canvas-sized frames (which do not shrink: the area ingest gives them their own bytes)."""
    db, est, frames, Ks = scene
    Hs, Ws = frames[0].shape[:2]
    seqs = _seqs(frames, 4, 3)
    cams = [[_camera_frame(f, Ks[s], device=(s + t) % 2 == 1) for t, f in enumerate(q)] for s, q in enumerate(seqs)]
    flat = [[I.Frame(np_ingest_lens_area(f, Hs, Ws), K=I.plan(f, (Hs, Ws))[2]) for f in q] for q in cams]
    first = cams[0][0]
    nodes, lg = first.lens.mesh(first.K, first.width, first.height, 0, Ws, Hs)
    assert I.Lens.samples_log2(nodes, lg, first.width, first.height) == 1
    # the filter changes the picture the networks see (by little: the source is the scene with every pixel doubled, 4.7 % of the bytes)
    assert (flat[0][0].plane0.reshape(Hs, Ws, 3) != np_ingest_lens_area(first, Hs, Ws, L=0)).mean() > 0.01
    got = T.track_streams(est, cams, batch=2, lanes=2, graphs=graphs, frame_size=(Hs, Ws), minify="area")
    ref = T.track_streams(est, flat, batch=2, lanes=2, graphs=graphs, frame_size=(Hs, Ws), minify="area")
    for (p, sm), (wp, ws) in zip(got, ref):
        assert np.isfinite(p).all()
        np.testing.assert_array_equal(p, wp)
        np.testing.assert_array_equal(sm, ws)
