"""Lens frames under minify="area" (include/gen6d_hip.h at g6d_frame_ingest_area) on the CPU: n x n sub-samples per canvas
pixel through the mesh.  `np_mesh_area_picture` restates the rule in numpy on a source's converted pixels, `np_frame_ingest_mesh_area`
has the signature of ops.frame_ingest_area (host tables).  Checks the rule's two consequences (samples_log2 = 0: the mesh rule; a lens that
does nothing over an integer ratio: the plain area rule's block means), the rule against a float64 computation that knows no mesh, the
sample count, the host path on patched ops, and that the ABI did not move.  The tap conversions, the mesh rule and the plain area rule
are those of the existing restatements, imported."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from test_frame_crop_cpu import records_of_table
from test_ingest_cpu import np_frame_ingest, pitched
from test_ingest_lens_cpu import camera, np_frame_ingest_mesh, np_ingest_lens, np_mesh_coords
from test_minify_cpu import np_frame_ingest_area, np_ingest_area, record_rgb
from test_pixel_formats_cpu import host_record, random_frame, rgb_table

SUITE_LENS = ("brown", (-0.12, 0.03, 0.001, -0.0005))    # the lens of the suite's tracker tests
ZERO = ("brown", (0.0, 0.0, 0.0, 0.0))


# ---------------------------------------------------------------------------------------------------------------- the restatement
def np_mesh_area_coords(nodes, lg, L, out_w, out_h):
    """int32 nodes [ny,nx,2] -> (fx, fy) int64 [out_h * n, out_w * n] in 1/2048 source pixels: sub-sample (k, l) of pixel (X, Y) at
    [Y n + l, X n + k].  Exact integers, as the header writes them."""
    n, g = 1 << L, 1 << lg
    G, s = 2 * n * g, 2 * (1 + L + lg) + 5
    ny, nx = nodes.shape[:2]
    U = (2 * n * np.arange(out_w)[:, None] + 2 * np.arange(n)[None, :] + 1 - n).reshape(-1)
    V = (2 * n * np.arange(out_h)[:, None] + 2 * np.arange(n)[None, :] + 1 - n).reshape(-1)
    c, r = np.clip(U // G, 0, nx - 2), np.clip(V // G, 0, ny - 2)                # (floor division)
    i, j = (U - c * G)[None, :], (V - r * G)[:, None]
    assert (i < G).all() and (j < G).all() and i.min() > -n and j.min() > -n     # negative only at the left / top edge, by less than half a pixel
    m = nodes.astype(np.int64)
    r, c = r[:, None], c[None, :]
    out = []
    for a in (0, 1):
        S = (G - i) * (G - j) * m[r, c, a] + i * (G - j) * m[r, c + 1, a] + (G - i) * j * m[r + 1, c, a] + i * j * m[r + 1, c + 1, a]
        assert np.abs(S).max() < 2 ** 52
        out.append((S + (1 << (s - 1))) >> s)
    return out


def np_mesh_area_picture(rgb, nodes, lg, L, out_w, out_h, H, W):
    """A source's converted pixels rgb [hs,ws,3] (every tap converted by its format's rule: the picture at integer positions) + mesh +
    samples_log2 -> the [H,W,3] canvas."""
    hs, ws = rgb.shape[:2]
    n = 1 << L
    ow, oh = min(out_w, W), min(out_h, H)
    canvas = np.zeros((H, W, 3), np.uint8)
    if ow < 1 or oh < 1:
        return canvas
    fx, fy = np_mesh_area_coords(nodes, lg, L, ow, oh)
    inside = (fx >= -1024) & (fx <= (ws - 1) * 2048 + 1024) & (fy >= -1024) & (fy <= (hs - 1) * 2048 + 1024)
    fx, fy = np.clip(fx, 0, (ws - 1) * 2048), np.clip(fy, 0, (hs - 1) * 2048)
    x0, a, y0, b = fx >> 11, (fx & 2047)[..., None], fy >> 11, (fy & 2047)[..., None]
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    p = rgb.astype(np.int64)
    A = (2048 - a) * (2048 - b) * p[y0, x0] + a * (2048 - b) * p[y0, x1] + (2048 - a) * b * p[y1, x0] + a * b * p[y1, x1]   # not rounded
    assert A.max() < 2 ** 30
    A = np.where(inside[..., None], A, 0)                                        # a black sample
    total = A.reshape(oh, n, ow, n, 3).sum((1, 3))
    assert total.max() < 2 ** 37
    canvas[:oh, :ow] = ((total + (1 << (21 + 2 * L))) >> (22 + 2 * L)).astype(np.uint8)
    return canvas


def np_frame_ingest_mesh_area(table, meshes, n, out, K_out):
    """ops.frame_ingest_area on host memory with the field read: a frame whose mesh has nodes and samples_log2 > 0 by the rule above,
    every other frame as test_minify_cpu.np_frame_ingest_area has it (mesh rule / plain area rule)."""
    fsize, msize = C.sizeof(lib.G6dFrame), C.sizeof(lib.G6dMesh)
    B, H, W = out.shape[:3]
    mesh = (lib.G6dMesh * n).from_buffer_copy(meshes.numpy()[:n * msize].tobytes()) if meshes is not None else [None] * n
    raw = (lib.G6dFrame * n).from_buffer_copy(table.numpy()[:n * fsize].tobytes())
    for k, (r, m) in enumerate(zip(raw, mesh)):
        L = 0 if m is None or not m.nodes else min(max(m.reserved, 0), 3)
        if L == 0:
            np_frame_ingest_area(table[k * fsize:(k + 1) * fsize], None if meshes is None else meshes[k * msize:(k + 1) * msize], 1, out, K_out)
            continue
        if not 0 <= r.slot < B:
            continue
        plain, keep = rgb_table(table[k * fsize:(k + 1) * fsize], 1)
        e = records_of_table(plain)[0]
        assert 1 <= m.step_log2 <= 4 and m.nx >= -(-e.out_w >> m.step_log2) + 1 and m.ny >= -(-e.out_h >> m.step_log2) + 1
        nodes = np.ctypeslib.as_array((C.c_int32 * (m.ny * m.nx * 2)).from_address(m.nodes)).reshape(m.ny, m.nx, 2)
        out.numpy()[r.slot] = np_mesh_area_picture(record_rgb(e), nodes, m.step_log2, L, e.out_w, e.out_h, H, W)
        K_out.numpy()[r.slot] = np.asarray(list(r.K), np.float32).reshape(3, 3)
    return out


_meshes = {}     # (lens, K, size, turn, picture) -> (nodes, step_log2) of this session


def mesh_of(frame, H, W):
    """-> (nodes, step_log2, out_w, out_h) of a lens frame planned for an H x W canvas, by ingest.Lens.mesh (tests/test_ingest_lens_cpu.py
    holds that against its own restatement)."""
    out_h, out_w, _ = I.plan(frame, (H, W))
    key = (frame.lens, frame.K.tobytes(), frame.width, frame.height, frame.rotate, out_w, out_h)
    if key not in _meshes:
        _meshes[key] = frame.lens.mesh(frame.K, frame.width, frame.height, frame.rotate, out_w, out_h)
    return _meshes[key] + (out_w, out_h)


def np_ingest_lens_area(frame, H, W, L=None):
    """One ingest.Frame with a lens (any format, host or device planes) -> its [H,W,3] canvas by the rule; L: the host's choice unless given."""
    nodes, lg, out_w, out_h = mesh_of(frame, H, W)
    if L is None:
        L = I.Lens.samples_log2(nodes, lg, frame.width, frame.height)
    e = host_record(frame, H, W)
    return np_mesh_area_picture(record_rgb(e), nodes, lg, L, out_w, out_h, H, W)


def zero_lens_frame(img, k, fmt="rgb24", minify="area"):
    """img [h*k, w*k, 3]: a frame k times an h x w picture with a lens that does nothing and an off-centre K."""
    hs, ws = img.shape[:2]
    K = np.array([[0.7 * ws, 0, 0.41 * ws], [0, 0.66 * ws, 0.57 * hs], [0, 0, 1.0]])
    return I.Frame(img, fmt, K=K, lens=I.Lens(*ZERO, minify=minify))


# ---------------------------------------------------------------------------------------------------------------- 1: the two consequences
@pytest.mark.parametrize("lg", [1, 2, 3, 4])
def test_one_sample_is_the_mesh_rule(lg):
    """L = 0: U = 2X, G = 2g, S four times the mesh rule's and s two more: the same coordinates at every pixel, on a random mesh (which
    no lens would produce: the identity is one of integers)."""
    rng = np.random.RandomState(10 + lg)
    out_w, out_h = 150, 52
    g = 1 << lg
    nodes = rng.randint(-2 ** 30, 2 ** 30 + 1, (-(-out_h // g) + 1, -(-out_w // g) + 1, 2)).astype(np.int32)
    for got, want in zip(np_mesh_area_coords(nodes, lg, 0, out_w, out_h), np_mesh_coords(nodes, lg, out_w, out_h)):
        np.testing.assert_array_equal(got, want)


def test_one_sample_gives_the_mesh_rules_bytes():
    rng = np.random.RandomState(15)
    H, W = 56, 160
    f = I.Frame(rng.randint(0, 256, (208, 600, 3)).astype(np.uint8), K=camera(600, 208, 330.0), lens=I.Lens(*SUITE_LENS))
    got = np_ingest_lens_area(f, H, W, L=0)
    np.testing.assert_array_equal(got, np_ingest_lens(f, H, W))
    assert got.any()


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_a_lens_that_does_nothing_gives_the_plain_area_rule(k):
    """Consequence 2: zero coefficients, new_K = K, a source exactly k times the 150 x 52 picture, mesh step 16, n = k: every sub-sample
    lands on one source pixel with fraction 0, so the pixel is the round-half-up mean of its k x k block."""
    rng = np.random.RandomState(20 + k)
    H, W = 52, 150
    img = rng.randint(0, 256, (H * k, W * k, 3)).astype(np.uint8)
    f = zero_lens_frame(img, k)
    nodes, lg, out_w, out_h = mesh_of(f, H, W)
    assert (lg, out_w, out_h) == (4, W, H)
    L = I.Lens.samples_log2(nodes, lg, f.width, f.height)
    assert 1 << L == k
    fx, fy = np_mesh_area_coords(nodes, lg, L, out_w, out_h)
    assert not (fx & 2047).any() and not (fy & 2047).any()
    np.testing.assert_array_equal(fx >> 11, np.broadcast_to(np.arange(W * k), fx.shape))
    got = np_ingest_lens_area(f, H, W)
    np.testing.assert_array_equal(got, np_ingest_area(I.Frame(img), H, W))
    np.testing.assert_array_equal(got, (2 * img.astype(np.int64).reshape(H, k, W, k, 3).sum((1, 3)) + k * k) // (2 * k * k))


# ---------------------------------------------------------------------------------------------------------------- 2: a float64 computation without a mesh
def smooth(u, v):
    """Three slow waves, one per channel."""
    return np.stack([127.5 + 100 * np.sin(2 * np.pi * u / 211) * np.cos(2 * np.pi * v / 173), 127.5 + 110 * np.cos(2 * np.pi * (u + v) / 257),
                     127.5 + 90 * np.sin(2 * np.pi * (u - 2 * v) / 301)], -1)


def test_against_float64_on_the_model_itself():
    """The suite's lens at 4:1 (600 x 208 -> 150 x 52) on a smooth picture whose horizontally and vertically neighbouring pixels differ by
    at most D levels, against the mean over the same n^2 positions of the float64 bilinear sample at Lens.source_coords: no mesh, no
    fixed point.  The mesh is within e = tol max(ws/wt, hs/ht) + 2^-12 + 2^-16 source pixels of the model per axis (the step choice, the
    rounding of f to 1/2048, the rounding of the nodes to 1/65536), a bilinear surface moves by at most D per source pixel along an axis,
    so |got - oracle| <= 2 D e + 1 (the last 1: the rounding of the result and of the oracle's uint8 picture is inside it).  The barrel
    lens pulls every sample inside the source (asserted), so nothing is excluded for the border.  Row 0 and column 0 are excluded, and
    only those: (150 + 52 - 1) / (150 * 52) = 2.6 % of the pixels; their outer sub-samples extrapolate the first cell over less than half a
    canvas pixel, which tol does not cover; the bit-exact tests cover them."""
    hs, ws, H, W = 208, 600, 52, 150
    v, u = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
    img = np.rint(smooth(u, v)).astype(np.uint8)
    D = max(np.abs(np.diff(img.astype(int), axis=0)).max(), np.abs(np.diff(img.astype(int), axis=1)).max())
    K = camera(ws, hs, 330.0)
    f = I.Frame(img, K=K, lens=I.Lens(*SUITE_LENS, minify="area"))
    nodes, lg, out_w, out_h = mesh_of(f, H, W)
    assert (out_w, out_h) == (W, H)
    L = I.Lens.samples_log2(nodes, lg, ws, hs)
    n = 1 << L
    assert n == 4
    got = np_ingest_lens_area(f, H, W).astype(np.float64)
    off = (2 * np.arange(n) + 1 - n) / (2 * n)
    X = (np.arange(W)[:, None] + off[None, :]).reshape(-1)
    Y = (np.arange(H)[:, None] + off[None, :]).reshape(-1)
    ud, vd = f.lens.source_coords(K, ws, hs, 0, W, H, *np.meshgrid(X, Y))
    assert ud.min() >= 0 and ud.max() <= ws - 1 and vd.min() >= 0 and vd.max() <= hs - 1        # no sample meets the border or a clamp
    x0, y0 = np.minimum(np.floor(ud).astype(int), ws - 2), np.minimum(np.floor(vd).astype(int), hs - 2)
    a, b = (ud - x0)[..., None], (vd - y0)[..., None]
    p = img.astype(np.float64)
    val = (1 - a) * (1 - b) * p[y0, x0] + a * (1 - b) * p[y0, x0 + 1] + (1 - a) * b * p[y0 + 1, x0] + a * b * p[y0 + 1, x0 + 1]
    oracle = val.reshape(H, n, W, n, 3).mean((1, 3))
    e = f.lens.tol * max(ws / W, hs / H) + 2.0 ** -12 + 2.0 ** -16
    bound = 2 * D * e + 1
    err = np.abs(got - oracle)
    print(f"D = {D}, e = {e:.4f}, bound {bound:.3f}; largest distance {err[1:, 1:].max():.3f} (row 0 / column 0: {max(err[0].max(), err[:, 0].max()):.3f}); "
          f"mesh step {1 << lg}")
    assert D <= 8 and err[1:, 1:].max() <= bound
    point = np_ingest_lens(f, H, W).astype(np.float64)
    assert np.abs(point - got).max() > 0                                                       # (the point rule is another picture)


# ---------------------------------------------------------------------------------------------------------------- 3: the sample count
def test_sample_count():
    """M = source pixels per canvas pixel over the node pairs inside the source: zero lenses at 1:1, 2:1, 3:1, 4:1, 8:1 give n = 1, 2, 4,
    4, 8 (M = k exactly between nodes inside the source; the thresholds 1.5, 3, 6 are half open: M = 3 is 4).  The suite's barrel lens at
    4:1 compresses towards the edge: M just under 4, n = 4."""
    H, W = 52, 150
    for k, n in ((1, 1), (2, 2), (3, 4), (4, 4), (8, 8)):
        f = zero_lens_frame(np.zeros((H * k, W * k, 3), np.uint8), k)
        nodes, lg, _, _ = mesh_of(f, H, W)
        assert 1 << I.Lens.samples_log2(nodes, lg, f.width, f.height) == n, k
    f = I.Frame(np.zeros((208, 600, 3), np.uint8), K=camera(600, 208, 330.0), lens=I.Lens(*SUITE_LENS))
    nodes, lg, _, _ = mesh_of(f, H, W)
    m = nodes.astype(np.int64)
    ok = (m[..., 0] >= -32768) & (m[..., 0] <= 600 * 65536 - 32768) & (m[..., 1] >= -32768) & (m[..., 1] <= 208 * 65536 - 32768)
    dx = np.abs(np.diff(m, axis=1)).max(-1)[ok[:, 1:] & ok[:, :-1]].max()
    dy = np.abs(np.diff(m, axis=0)).max(-1)[ok[1:] & ok[:-1]].max()
    M = max(dx, dy) / (65536 << lg)
    print(f"barrel at 4:1: M = {M:.4f}, step {1 << lg}")
    assert 3.5 < M < 4 and I.Lens.samples_log2(nodes, lg, 600, 208) == 2
    # no pair inside the source: n = 1; thresholds on hand-made meshes of step 2 (unit = 2 * 65536 per source pixel per canvas pixel)
    far = np.full((3, 3, 2), 2 ** 30, np.int32)
    assert I.Lens.samples_log2(far, 1, 64, 64) == 0
    for span, want in ((1.49, 0), (1.5, 1), (2.99, 1), (3.0, 2), (5.99, 2), (6.0, 3), (40.0, 3)):
        pair = np.zeros((1, 2, 2), np.int32)
        pair[0, 1, 0] = int(round(span * 2 * 65536))
        assert I.Lens.samples_log2(pair, 1, 512, 64) == want, span
        assert I.Lens.samples_log2(pair.transpose(1, 0, 2)[..., ::-1].copy(), 1, 64, 512) == want, span   # a vertical pair, in y


# ---------------------------------------------------------------------------------------------------------------- 4: the host path
def test_three_rules_in_one_call_and_the_field_on_area_calls_only(monkeypatch):
    rng = np.random.RandomState(30)
    H, W = 56, 160
    I._meshes.clear()
    K = camera(600, 208, 330.0)
    img = rng.randint(0, 256, (208, 600, 3)).astype(np.uint8)
    plain = random_frame(rng, "nv12", 208, 600, extra=8)
    default = I.Frame(img, K=K, lens=I.Lens(*SUITE_LENS))
    area = I.Frame(pitched(img[..., ::-1].copy(), 5), "bgr24", width=600, K=K, lens=I.Lens(*SUITE_LENS, minify="area"))
    frames, slots = [plain, default, area], [3, 0, 2]
    assert default.lens != area.lens and hash(default.lens) != hash(area.lens) and default.lens == I.Lens(*SUITE_LENS, minify="point")
    seen = []

    def fields(meshes, n):
        return [m.reserved for m in (lib.G6dMesh * n).from_buffer_copy(meshes.numpy()[:n * C.sizeof(lib.G6dMesh)].tobytes())]
    monkeypatch.setattr(ops, "frame_ingest_area", lambda t, m, n, o, k: (seen.append(("area", fields(m, n))), np_frame_ingest_mesh_area(t, m, n, o, k))[1])
    monkeypatch.setattr(ops, "frame_ingest_mesh", lambda t, m, n, o, k: (seen.append(("mesh", fields(m, n))), np_frame_ingest_mesh(t, m, n, o, k))[1])
    monkeypatch.setattr(ops, "frame_ingest", np_frame_ingest)
    out, Ko = torch.full((4, H, W, 3), 9, dtype=torch.uint8), torch.zeros((4, 3, 3))
    I.ingest_frames_keep(frames, out, Ko, slots=slots, minify="area")
    L = I.Lens.samples_log2(*mesh_of(area, H, W)[:2], 600, 208)
    assert L == 2 and seen == [("area", [0, 0, L])]
    got = out.numpy()
    np.testing.assert_array_equal(got[3], np_ingest_area(plain, H, W))
    np.testing.assert_array_equal(got[0], np_ingest_lens(default, H, W))
    np.testing.assert_array_equal(got[2], np_ingest_lens_area(area, H, W))
    assert (got[1] == 9).all() and (got[2] != np_ingest_lens(area, H, W)).mean() > 0.5
    # a point call writes 0 for every frame and gives both lens frames the mesh rule's bytes
    point = torch.zeros((4, H, W, 3), dtype=torch.uint8)
    I.ingest_frames(frames, point, Ko, slots=slots)
    assert seen[1:] == [("mesh", [0, 0, 0])]
    np.testing.assert_array_equal(point.numpy()[0], got[0])
    np.testing.assert_array_equal(point.numpy()[2], np_ingest_lens(area, H, W))
    assert len(I._meshes) == 2                                                  # the two settings are two cache entries, each built once
    m = lib.G6dMesh(samples_log2=0)
    m.samples_log2 = 3
    assert m.reserved == m.samples_log2 == 3 and [n for n, _ in lib.G6dMesh._fields_] == ["nodes", "nx", "ny", "step_log2", "reserved"]


def test_a_bad_setting_is_rejected():
    for bad in ("box", None, "AREA", 1):
        with pytest.raises(ValueError, match="minify"):
            I.Lens(*ZERO, minify=bad)
    assert I.Lens(*ZERO).minify == "point" and I.Lens("brown", (0, 0, 0, 0), None, 1 / 16) == I.Lens(*ZERO)


# ---------------------------------------------------------------------------------------------------------------- 5: ABI
def test_abi_did_not_move():
    l = lib.load()
    assert l.g6d_abi_version() == 12
    assert (l.g6d_sizeof_frame_desc(), l.g6d_sizeof_mesh_desc(), l.g6d_sizeof_sink_desc()) == (96, 24, 72)
    assert (C.sizeof(lib.G6dFrame), C.sizeof(lib.G6dMesh), C.sizeof(lib.G6dSink)) == (96, 24, 72)
    assert lib.G6dMesh.reserved.offset == 20
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gen6d_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\s*\*)\s*(g6d_\w+)\s*\(", header, re.M))
    assert set(lib.SIGNATURES) <= declared and len(lib.SIGNATURES) == 84            # the entry points of the commit before this rule: none added (82nd - 84th: g6d_conv_route, g6d_conv16_direct_route, g6d_wino_multi_route, later host-only reports)
    assert re.search(r"int32_t samples_log2;", header) and not re.search(r"int32_t reserved;", header)


# ---------------------------------------------------------------------------------------------------------------- 6: the kernels' resources
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_area_kernels_have_no_scratch_and_eight_waves(tmp_path):
    """Compiler metadata (cross-compiles without a GPU): the supersampling tile's 64-bit sums and coordinates stay in registers, and it
    costs frame_ingest_area_kernel, whose plain tiles it would slow down as a branch (profiles/r33_lens_area.md), nothing: both kernels
    stay at 64 VGPRs or fewer, 8 waves per SIMD."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "ingest.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(root, "gen6d_amd", "csrc", "ingest.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    for kernel in ("frame_ingest_area_kernel", "frame_ingest_lens_area_kernel"):
        (name, body), = re.findall(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % kernel, text, re.S)
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            assert int(re.search(r"\.%s:\s+(\d+)" % key, body).group(1)) == 0, (name, key)
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1)) <= 64, name
