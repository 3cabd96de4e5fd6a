"""minify="area" (include/gen6d_hip.h) restated in numpy, and the host logic around it.
1: g6d_frame_ingest_area's exact-integer rule (`np_frame_ingest_area`): its weights, its two consequences (a frame that does not shrink
   gets the plain rule's bytes; an integer ratio gives block means), the picture the point rule turns black, the largest sums.
2: g6d_frame_crop_area's rule (`np_crop_area`): the samples per slot, and n = 1 against test_frame_crop_cpu.np_crop.
3: the tracker's switch on patched ops: errors, and which entry points each mode calls.  4: ABI.
The tap conversions are those of the existing restatements (test_ingest_cpu, test_pixel_formats_cpu, test_frame_crop_cpu), imported."""
import ctypes as C

import numpy as np
import pytest
import torch

from gen6d_amd import ingest as I
from gen6d_amd import lib, ops
from gen6d_amd import tracking as T
from test_frame_crop_cpu import _tap_rgb, homographies, native2x, np_crop, patched, records_of_frames, records_of_table, source_frame  # noqa: F401
from test_ingest_cpu import _axis, np_frame_ingest, np_ingest_picture
from test_ingest_lens_cpu import np_frame_ingest_mesh
from test_pixel_formats_cpu import host_record, random_frame, rgb_table
from test_track_streams_cpu import scene  # noqa: F401  (the module's fixture)


# ---------------------------------------------------------------------------------------------------------------- the ingest's rule
def axis_taps(t, T_, S):
    """Target coordinate t of an axis with T_ picture pixels over S source pixels -> (tap indices, weights, D_axis), int64."""
    if S <= T_:                                        # no shrink: the plain rule's two taps
        i0, i1, a = (int(v[0]) for v in _axis(np.asarray([t]), T_, S))
        return np.array([i0, i1]), np.array([2048 - a, a]), 2048
    lo, hi = t * S, (t + 1) * S                        # [t S, (t+1) S) in units of 1/T_ source pixel
    i = np.arange(lo // T_, (hi - 1) // T_ + 1)
    return i, np.minimum((i + 1) * T_, hi) - np.maximum(i * T_, lo), S


def axis_matrix(ts, T_, S, cols):
    """-> ([len(ts), cols] int64 weights of source pixels 0 .. cols-1, D_axis); every tap of `ts` must lie below `cols`."""
    M, D = np.zeros((len(ts), cols), np.int64), None
    for k, t in enumerate(ts):
        i, w, D = axis_taps(int(t), T_, S)
        assert i.max() < cols
        np.add.at(M[k], i, w)
    return M, D


def area_picture(rgb, ws, hs, wt, ht, txs, tys):
    """The rule on unrotated target coordinates txs x tys of the wt x ht picture of a ws x hs source whose converted pixels are rgb
    [rows, cols, 3] (the top-left part of the source is enough when the taps stay inside it) -> uint8 [len(tys), len(txs), 3]."""
    rgb = np.asarray(rgb).astype(np.int64)
    Mx, Dx = axis_matrix(txs, wt, ws, rgb.shape[1])
    My, Dy = axis_matrix(tys, ht, hs, rgb.shape[0])
    rows = np.einsum("xw,hwc->hxc", Mx, rgb)                         # the inner sums
    assert rows.max() <= 255 * 2 ** 13
    sigma = np.einsum("yh,hxc->yxc", My, rows)
    D = Dx * Dy
    assert sigma.max() <= 255 * D <= 255 * 2 ** 26
    return ((2 * sigma + D) // (2 * D)).astype(np.uint8)


def np_area_canvas(rgb, rot, out_w, out_h, H, W):
    """A source's converted picture rgb [hs,ws,3] -> the [H,W,3] canvas: scaled to the out_w x out_h picture by the area rule, turned."""
    hs, ws = rgb.shape[:2]
    wt, ht = (out_h, out_w) if rot in (90, 270) else (out_w, out_h)
    ow, oh = min(out_w, W), min(out_h, H)
    canvas = np.zeros((H, W, 3), np.uint8)
    if ow < 1 or oh < 1:
        return canvas
    pic = area_picture(rgb, ws, hs, wt, ht, np.arange(wt), np.arange(ht))
    Y, X = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    x, y = {0: (X, Y), 90: (Y, ht - 1 - X), 180: (wt - 1 - X, ht - 1 - Y), 270: (wt - 1 - Y, X)}[rot]
    canvas[:oh, :ow] = pic[y, x]
    return canvas


def record_rgb(e):
    """A record of the first five formats under matrix 0 / 1 (host_record and rgb_table make every other one such a record) -> its
    converted picture [hs,ws,3]: the ingest's tap rule at the integer positions, i.e. the same-size, unturned plain ingest."""
    return np_ingest_picture(e.p0, e.p1, e.pitch0, e.pitch1, e.width, e.height, e.format, 0, e.matrix, e.width, e.height, e.height, e.width)


def np_ingest_area(frame, H, W, out_w=None, out_h=None):
    """One ingest.Frame of any format (host or device planes) -> its [H,W,3] canvas by the area rule; out_w x out_h: the planned
    picture unless given."""
    e = host_record(frame, H, W)
    return np_area_canvas(record_rgb(e), e.rotate, e.out_w if out_w is None else out_w, e.out_h if out_h is None else out_h, H, W)


def np_frame_ingest_area(table, meshes, n, out, K_out):
    """ops.frame_ingest_area on host memory: a frame whose mesh has nodes through the mesh rule, every other one through the area rule."""
    fsize, msize = C.sizeof(lib.G6dFrame), C.sizeof(lib.G6dMesh)
    plain, keep = rgb_table(table, n)
    ents = records_of_table(plain[:n * fsize])
    raw = (lib.G6dFrame * n).from_buffer_copy(table.numpy()[:n * fsize].tobytes())
    mesh = (lib.G6dMesh * n).from_buffer_copy(meshes.numpy()[:n * msize].tobytes()) if meshes is not None else [None] * n
    B, H, W = out.shape[:3]
    for k, (e, r, m) in enumerate(zip(ents, raw, mesh)):
        if m is not None and m.nodes:
            np_frame_ingest_mesh(plain[k * fsize:(k + 1) * fsize], meshes[k * msize:(k + 1) * msize], 1, out, K_out)
        elif 0 <= r.slot < B:
            out.numpy()[r.slot] = np_area_canvas(record_rgb(e), e.rotate, e.out_w, e.out_h, H, W)
            K_out.numpy()[r.slot] = np.asarray(list(r.K), np.float32).reshape(3, 3)
    return out


def _pairs():
    rng = np.random.RandomState(1)
    edge = [1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 540, 960, 1080, 1920, 2160, 3840, 4095, 4096, 4097, 8190, 8191, 8192]
    return [(s, t) for s in edge for t in edge] + [tuple(int(v) for v in rng.randint(1, 8193, 2)) for _ in range(400)]


def test_weights_sum_to_the_axis_denominator_and_stay_inside_the_source():
    rng = np.random.RandomState(2)
    for S, T_ in _pairs():
        ts = sorted({0, 1, T_ // 2, T_ - 2, T_ - 1} & set(range(T_))) + [int(t) for t in rng.randint(0, T_, 3)]
        for t in ts:
            i, w, D = axis_taps(t, T_, S)
            assert D == (S if S > T_ else 2048) and w.sum() == D, (S, T_, t)
            assert 0 <= i.min() and i.max() <= S - 1, (S, T_, t)
            if S > T_:
                assert w.min() >= 1 and w.max() <= T_ and (np.diff(i) == 1).all(), (S, T_, t)
        if S > T_ and T_ <= 64:                        # the footprints tile the axis: every source pixel weighs T_ in all
            M, _ = axis_matrix(range(T_), T_, S, S)
            assert (M.sum(0) == T_).all(), (S, T_)


@pytest.mark.parametrize("rot", [0, 90, 180, 270])
def test_a_frame_that_does_not_shrink_equals_the_plain_rule(rot):
    rng = np.random.RandomState(3 + rot)
    for fmt, (hs, ws), (H, W) in (("rgb24", (23, 37), (23, 37)), ("nv12", (26, 38), (61, 97)), ("bgra32", (20, 30), (45, 31))):
        f = source_frame(rng, hs, ws, fmt, rot, extra=3)
        if rot in (90, 270):
            H, W = W, H
        e = host_record(f, H, W)
        wt, ht = (e.out_h, e.out_w) if rot in (90, 270) else (e.out_w, e.out_h)
        assert ws <= wt and hs <= ht
        want = np_ingest_picture(e.p0, e.p1, e.pitch0, e.pitch1, e.width, e.height, e.format, rot, e.matrix, e.out_w, e.out_h, H, W)
        np.testing.assert_array_equal(np_ingest_area(f, H, W), want)


def test_the_picture_the_point_rule_turns_black():
    """S = 4 T, columns 255, 0, 0, 255: the point rule blends columns 4t+1 and 4t+2, the area rule all four (mean 127.5, half up)."""
    hs, ws = 32, 64
    src = np.zeros((hs, ws, 3), np.uint8)
    src[:, 0::4] = src[:, 3::4] = 255
    f = I.Frame(src, "rgb24")
    H, W = hs // 4, ws // 4
    e = host_record(f, H, W)
    assert (e.out_h, e.out_w) == (H, W)
    point = np_ingest_picture(e.p0, e.p1, e.pitch0, e.pitch1, ws, hs, 0, 0, 0, W, H, H, W)
    assert (point == 0).all()
    assert (np_ingest_area(f, H, W) == 128).all()


def test_an_integer_ratio_gives_round_half_up_block_means():
    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, (48, 64, 3)).astype(np.uint8)
    for k in (2, 4):
        H, W = 48 // k, 64 // k
        blocks = src.astype(np.int64).reshape(H, k, W, k, 3).sum((1, 3))
        np.testing.assert_array_equal(np_ingest_area(I.Frame(src), H, W), (2 * blocks + k * k) // (2 * k * k))
    # one axis by 3, the other magnified: the mixed case keeps the plain taps on the axis that grows
    got = np_area_canvas(src, 0, 100, 16, 16, 100)
    rows = src.astype(np.int64).reshape(16, 3, 64, 3).sum(1)
    x0, x1, a = _axis(np.arange(100), 100, 64)
    want = (2 * ((2048 - a)[None, :, None] * rows[:, x0] + a[None, :, None] * rows[:, x1]) + 3 * 2048) // (2 * 3 * 2048)
    np.testing.assert_array_equal(got, want)


def test_the_largest_sums_saturate_exactly():
    """S = 8192, T = 8191 on both axes: D = 2^26, Sigma = 255 * 2^26; a canvas corner (its taps lie in the source's corner)."""
    white = np.full((12, 12, 3), 255, np.uint8)
    got = area_picture(white, 8192, 8192, 8191, 8191, np.arange(9), np.arange(9))
    assert (got == 255).all()
    far = area_picture(np.full((2, 2, 3), 255, np.uint8), 8192, 8192, 8191, 8191, [0], [0])
    assert far.shape == (1, 1, 3)
    i, w, D = axis_taps(8190, 8191, 8192)
    assert list(i) == [8190, 8191] and list(w) == [1, 8191] and D == 8192


def test_all_eleven_formats_go_through_their_tap_rule():
    """A 2:1 area ingest of a frame of every format equals the block means of its converted picture (consequence 2 on real taps)."""
    rng = np.random.RandomState(6)
    for k, fmt in enumerate(I.FORMATS):
        f = random_frame(rng, fmt, 16, 24, matrix=list(I.MATRICES)[k % 4], extra=4)
        rgb = record_rgb(host_record(f, 16, 24)).astype(np.int64)
        want = (2 * rgb.reshape(8, 2, 12, 2, 3).sum((1, 3)) + 4) // 8
        np.testing.assert_array_equal(np_ingest_area(f, 8, 12), want, err_msg=fmt)


# ---------------------------------------------------------------------------------------------------------------- the crop's rule
def _view(records, r, H, W, ft):
    """Slot view of record r (the canvas when r < 0) -> (sw, sh, turn, ax, bx, ay, by, tap)."""
    if r < 0:
        return W, H, (lambda cx, cy: (cx, cy)), ft(1), ft(0), ft(1), ft(0), None
    e = records[r]
    wt, ht = (e.out_h, e.out_w) if e.rotate in (90, 270) else (e.out_w, e.out_h)
    turn = {0: lambda cx, cy: (cx, cy), 90: lambda cx, cy: (cy, ft(ht - 1) - cx), 180: lambda cx, cy: (ft(wt - 1) - cx, ft(ht - 1) - cy),
            270: lambda cx, cy: (ft(wt - 1) - cy, cx)}[e.rotate]
    ax, ay = ft(e.width) / ft(wt), ft(e.height) / ft(ht)
    return e.width, e.height, turn, ax, ft(0.5) * ax - ft(0.5), ay, ft(0.5) * ay - ft(0.5), e


def _position(h, x, y, view, ft):
    """Steps 1 - 3 of g6d_frame_crop's rule in `ft`: crop coordinates (arrays) -> the source position before the clamp."""
    _, _, turn, ax, bx, ay, by, e = view
    X, Y, Wd = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.where(Wd != 0, ft(1) / Wd, ft(0))
        px, py = turn(X * iw, Y * iw)
        if e is None:                                  # the canvas: f = p * 1 + 0 = p exactly
            return px, py
        fma = lambda p, a, b: (np.asarray(p, np.float64) * np.float64(a) + np.float64(b)).astype(ft)   # (np_crop's note on step 3)
        return fma(px, ax, bx), fma(py, ay, by)


def np_samples_per_slot(records, rec, H, W, hinv, dh, dw, max_n):
    """n per slot, float32 as the kernel: the longer of the two steps of one crop pixel at the crop's centre, in source pixels."""
    ft, out = np.float32, []
    for b, r in enumerate(rec):
        h = np.asarray(hinv[b], np.float32).reshape(9)
        view = _view(records, int(r), H, W, ft)
        cx, cy = ft(0.5) * ft(dw - 1), ft(0.5) * ft(dh - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            p, px, py = (np.stack(_position(h, ft(cx + dx), ft(cy + dy), view, ft)).astype(np.float32) for dx, dy in ((0, 0), (1, 0), (0, 1)))
            m = np.fmax(np.hypot(*(px - p)), np.hypot(*(py - p)))            # (fmaxf: a NaN only if both are)
        out.append(int(min(np.floor(m + ft(0.5)), max_n)) if np.isfinite(m) and m >= 1.5 else 1)
    return out


def np_crop_area(records, rec, imgs, hinv, dh, dw, max_n=8, dtype=np.float32):
    """g6d_frame_crop_area's rule, the samples in `dtype` (n per slot always in float32) -> [B,3,dh,dw] of that dtype.  The body is
    np_crop's with the sample position a real number; with n = 1 it is np_crop (tested below)."""
    ft = np.dtype(dtype).type
    B, H, W = imgs.shape[:3]
    ns = np_samples_per_slot(records, rec, H, W, hinv, dh, dw, max_n)
    yy, xx = np.meshgrid(np.arange(dh).astype(ft), np.arange(dw).astype(ft), indexing="ij")
    out = np.zeros((B, 3, dh, dw), ft)
    for b in range(B):
        h = np.asarray(hinv[b], np.float32).reshape(9).astype(ft)
        r, n = int(rec[b]), ns[b]
        view = _view(records, r, H, W, ft)
        sw, sh = view[0], view[1]
        if r < 0:
            flat = imgs[b].reshape(-1).astype(np.int64)
            tap = lambda xi, yi: np.stack([flat[(yi * W + xi) * 3 + c] for c in range(3)], -1)
        else:
            tap = lambda xi, yi, e=records[r]: _tap_rgb(e, xi, yi)
        acc = np.zeros((dh, dw, 3), ft)
        for j in range(n):
            for i in range(n):
                x, y = xx + ft(2 * i + 1 - n) / ft(2 * n), yy + ft(2 * j + 1 - n) / ft(2 * n)
                fx, fy = _position(h, x, y, view, ft)
                fx, fy = np.fmin(np.fmax(fx, ft(-4)), ft(sw + 4)), np.fmin(np.fmax(fy, ft(-4)), ft(sh + 4))
                x0f, y0f = np.floor(fx), np.floor(fy)
                x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
                a, bb = fx - x0f, fy - y0f
                vx0, vx1, vy0, vy1 = (x0 >= 0) & (x0 < sw), (x0 + 1 >= 0) & (x0 + 1 < sw), (y0 >= 0) & (y0 < sh), (y0 + 1 >= 0) & (y0 + 1 < sh)
                xc0, xc1, yc0, yc1 = np.clip(x0, 0, sw - 1), np.clip(x0 + 1, 0, sw - 1), np.clip(y0, 0, sh - 1), np.clip(y0 + 1, 0, sh - 1)
                one = ft(1)
                w00, w01 = np.where(vx0 & vy0, (one - a) * (one - bb), 0), np.where(vx1 & vy0, a * (one - bb), 0)
                w10, w11 = np.where(vx0 & vy1, (one - a) * bb, 0), np.where(vx1 & vy1, a * bb, 0)
                acc = acc + (w00[..., None] * tap(xc0, yc0).astype(ft) + w01[..., None] * tap(xc1, yc0).astype(ft) +
                             w10[..., None] * tap(xc0, yc1).astype(ft) + w11[..., None] * tap(xc1, yc1).astype(ft))
        assert acc.dtype == ft
        out[b] = (np.clip(np.rint(acc / ft(n * n)), 0, 255) / ft(255)).transpose(2, 0, 1)
    return out


def np_frame_crop_area(table, rec, imgs, hinv, dh, dw, max_n=8, out=None):
    """ops.frame_crop_area on host memory."""
    plain, keep = rgb_table(table, table.numel() // C.sizeof(lib.G6dFrame))
    r = torch.from_numpy(np_crop_area(records_of_table(plain), rec.numpy(), imgs.numpy(), hinv.reshape(-1, 9).numpy(), dh, dw, max_n))
    if out is not None:
        out.copy_(r)
        return out
    return r


def scale_map(zoom, n=1):
    """Crop -> canvas maps that magnify the canvas `zoom` times (zoom < 1: one crop pixel covers 1 / zoom canvas pixels)."""
    return np.asarray([[1 / zoom, 0, 3, 0, 1 / zoom, 2, 0, 0, 1]] * n, np.float32)


def test_samples_per_slot():
    H, W, dh, dw = 96, 128, 20, 28
    for zoom, want in ((1 / 1.4, 1), (1 / 2.6, 3), (1 / 5, 5), (1 / 20, 8), (2.0, 1)):
        assert np_samples_per_slot([], [-1], H, W, scale_map(zoom), dh, dw, 8) == [want], zoom
    assert np_samples_per_slot([], [-1], H, W, scale_map(1 / 20), dh, dw, 3) == [3]
    assert np_samples_per_slot([], [-1], H, W, np.full((1, 9), np.nan, np.float32), dh, dw, 8) == [1]
    assert np_samples_per_slot([], [-1], H, W, np.zeros((1, 9), np.float32), dh, dw, 8) == [1]
    assert np_samples_per_slot([], [-1], H, W, np.asarray([[3e38, 0, 0, 0, 3e38, 0, 0, 0, 1e-38]], np.float32), dh, dw, 8) == [1]   # not finite
    # a source record twice the canvas doubles the footprint of the same map, also when it is turned
    for rot in (0, 90):
        f = source_frame(np.random.RandomState(7), 192, 256, "rgb24", rot)
        Hc, Wc = (128, 96) if rot else (96, 128)
        assert np_samples_per_slot(records_of_frames([f], Hc, Wc), [0, -1], Hc, Wc, scale_map(1 / 2.6, 2), dh, dw, 8) == [5, 3]


def test_one_sample_is_the_point_crop():
    rng = np.random.RandomState(8)
    H, W, dh, dw = 32, 48, 20, 28
    imgs = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    frames = [source_frame(rng, 26, 38, "nv12", 90, extra=4), source_frame(rng, 40, 60, "bgra32")]
    recs = records_of_frames(frames, H, W)
    hinv = homographies(rng, 3, zoom=(1.5, 4.0), shift=(-3, 12))        # magnifying: n = 1 in every slot
    assert np_samples_per_slot(recs, [0, -1, 1], H, W, hinv, dh, dw, 8) == [1, 1, 1]
    for dtype in (np.float32, np.float64):
        np.testing.assert_array_equal(np_crop_area(recs, [0, -1, 1], imgs, hinv, dh, dw, 8, dtype), np_crop(recs, [0, -1, 1], imgs, hinv, dh, dw, dtype))
    # ... and a cap of 1 makes any crop the point crop
    small = homographies(rng, 3, zoom=(0.2, 0.4), shift=(-3, 12))
    assert min(np_samples_per_slot(recs, [0, -1, 1], H, W, small, dh, dw, 8)) >= 2
    np.testing.assert_array_equal(np_crop_area(recs, [0, -1, 1], imgs, small, dh, dw, 1), np_crop(recs, [0, -1, 1], imgs, small, dh, dw))


def test_supersampled_crop_of_stripes_is_grey():
    """What the feature is for, on the crop side: one-pixel stripes under a 4x minifying crop are their mean, not one of the two levels."""
    H, W, dh, dw = 64, 64, 8, 8
    img = np.zeros((1, H, W, 3), np.uint8)
    img[:, :, 0::2] = 255
    hinv = np.asarray([[4, 0, 8, 0, 4, 8, 0, 0, 1]], np.float32)         # the pixel centres fall on even columns: white
    point = np_crop([], [-1], img, hinv, dh, dw) * 255
    area = np_crop_area([], [-1], img, hinv, dh, dw) * 255
    assert np.abs(point - 127.5).min() > 100
    assert np.abs(area - 127.5).max() <= 0.5


# ---------------------------------------------------------------------------------------------------------------- tracker
@pytest.fixture
def patched_area(monkeypatch, patched):
    """test_frame_crop_cpu's `patched` (its list receives the point crops) plus the two new entries -> {"ingest": n calls, "crop": [...]}."""
    calls = {"point": patched, "ingest": [], "crop": [], "warp": []}

    def ingest(table, meshes, n, out, K_out):
        calls["ingest"].append(n)
        return np_frame_ingest_area(table, meshes, n, out, K_out)

    def crop(table, rec, imgs, hinv, dh, dw, max_n=8, out=None):
        calls["crop"].append((rec.numpy().copy(), dh, max_n))
        return np_frame_crop_area(table, rec, imgs, hinv, dh, dw, max_n, out)
    warp = ops.warp_batch

    def warp_batch(*a, **k):
        calls["warp"].append(1)
        return warp(*a, **k)
    monkeypatch.setattr(ops, "frame_ingest_area", ingest)
    monkeypatch.setattr(ops, "frame_crop_area", crop)
    monkeypatch.setattr(ops, "warp_batch", warp_batch)
    plain = {"n": 0}
    for name in ("frame_ingest", "frame_ingest_mesh"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, fn=fn, **k: (plain.__setitem__("n", plain["n"] + 1), fn(*a, **k))[1])
    calls["plain"] = plain
    return calls


def test_tracker_option_errors(scene, patched_area):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    with pytest.raises(ValueError, match="frame_size"):
        T.StreamTracker(est, 2, batch=2, graphs=False, minify="area")
    with pytest.raises(ValueError, match="minify"):
        T.StreamTracker(est, 2, batch=2, graphs=False, frame_size=(h, w), minify="box")
    with pytest.raises(ValueError, match="minify"):
        T.track_streams(est, [[frames[0]]], batch=2, graphs=False, frame_size=(h, w), minify=None)
    with pytest.raises(ValueError, match="minify"):
        I.ingest_frames_keep([I.Frame(frames[0])], torch.zeros((1, h, w, 3), dtype=torch.uint8), torch.zeros((1, 3, 3)), minify="box")
    assert not patched_area["ingest"] and not patched_area["crop"] and not patched_area["point"]


def _push2(tr, frames):
    tr.push([0, 1], [native2x(frames[0], "nv12"), native2x(frames[1], "bgra")])
    tr.push([0, 1], [native2x(frames[1], "nv12"), native2x(frames[2], "bgra")])
    r = tr.result()
    assert all(np.isfinite(r[s][0]).all() for s in (0, 1))
    return r


def test_default_calls_neither_new_entry(scene, patched_area):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    _push2(T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, frame_size=(h, w), crops="source"), frames)
    assert not patched_area["ingest"] and not patched_area["crop"]
    assert patched_area["plain"]["n"] == 2 and patched_area["point"]


def test_area_with_canvas_crops_filters_the_ingest_only(scene, patched_area):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    _push2(T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, frame_size=(h, w), minify="area"), frames)
    assert patched_area["ingest"] == [2, 2] and patched_area["plain"]["n"] == 0
    assert not patched_area["crop"] and not patched_area["point"] and patched_area["warp"]


def test_area_with_source_crops_calls_both_new_entries(scene, patched_area):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    steps, size, rs = est.cfg["refine_iter"], est.device_chain().size, est.device_chain().refine_size
    got = _push2(T.StreamTracker(est, 2, batch=2, lanes=1, graphs=False, frame_size=(h, w), crops="source", minify="area"), frames)
    assert patched_area["ingest"] == [2, 2] and patched_area["plain"]["n"] == 0 and not patched_area["point"]
    # the first frames' selector crop and refinement steps, then one tracked step: every one with both records and the cap of 8
    assert [(list(r), d, m) for r, d, m in patched_area["crop"]] == [([0, 1], size, 8)] + [([0, 1], rs, 8)] * (steps + 1)
    assert set(got) == {0, 1}


def test_track_streams_recompute_path_uses_the_area_ingest(scene, patched_area, monkeypatch):
    est, frames, Ks = scene
    h, w = frames[0].shape[:2]
    native = [[native2x(frames[0], "nv12"), native2x(frames[1], "bgra")]]
    want = T.track_streams(est, native, batch=2, lanes=1, graphs=False, frame_size=(h, w), minify="area")
    first = len(patched_area["ingest"])
    assert first == 2 and patched_area["plain"]["n"] == 0
    left = [True]
    monkeypatch.setattr(est.refiner, "range_check", lambda: left.pop() if left else False)      # the window is left once
    got = T.track_streams(est, native, batch=2, lanes=1, graphs=False, frame_size=(h, w), minify="area")
    # the run, then host_track's frames one by one through _ingest_to_host: all by the area rule, none by the plain one
    assert patched_area["ingest"][first:] == [1, 1] + [1, 1] and patched_area["plain"]["n"] == 0
    # (the host loop runs the networks on other routes than the ticks: its poses are near the tracker's, not equal to them)
    assert np.isfinite(got[0][0]).all() and got[0][0].shape == want[0][0].shape
    imgs, _ = T._ingest_to_host(native[0], (h, w), "cpu", "area")      # ... and it sees the pictures the tracker saw
    for img, f in zip(imgs, native[0]):
        np.testing.assert_array_equal(img, np_ingest_area(f, h, w))


def test_stand_in_matches_the_picture_rule_and_keeps_lens_frames(scene, patched_area):
    """ingest_frames_keep(minify="area") end to end on the host: a shrinking frame by the area rule, a lens frame by the mesh rule."""
    est, frames, Ks = scene
    I._meshes.clear()
    h, w = frames[0].shape[:2]
    big = native2x(frames[0], "bgra")
    lens = I.Frame(frames[1], K=np.asarray(Ks[1], np.float64), lens=I.Lens("brown", (0.05, -0.01, 0.0, 0.0)))
    out, K = torch.zeros((2, h, w, 3), dtype=torch.uint8), torch.zeros((2, 3, 3))
    I.ingest_frames_keep([big, lens], out, K, minify="area")
    np.testing.assert_array_equal(out[0].numpy(), frames[0])           # 2 x 2 blocks of equal pixels: their mean is the pixel
    want = torch.zeros((2, h, w, 3), dtype=torch.uint8)
    I.ingest_frames([big, lens], want, torch.zeros((2, 3, 3)))
    np.testing.assert_array_equal(out[1].numpy(), want[1].numpy())
    assert patched_area["ingest"] == [2]


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_is_additive():
    l = lib.load()
    assert hasattr(l, "g6d_frame_ingest_area") and hasattr(l, "g6d_frame_crop_area")
    assert l.g6d_abi_version() == 12
    assert (l.g6d_sizeof_frame_desc(), l.g6d_sizeof_mesh_desc(), l.g6d_sizeof_sink_desc()) == (96, 24, 72)
    assert (C.sizeof(lib.G6dFrame), C.sizeof(lib.G6dMesh), C.sizeof(lib.G6dSink)) == (96, 24, 72)
    buf = (C.c_uint8 * 96)()
    p = C.addressof(buf)
    for args in ((None, None, 1, p, 1, 8, 8, p), (p, None, -1, p, 1, 8, 8, p), (p, None, 1, None, 1, 8, 8, p), (p, None, 1, p, 0, 8, 8, p),
                 (p, None, 1, p, 1, 0, 8, p), (p, None, 1, p, 1, 8, 0, p), (p, None, 1, p, 1, 8, 8, None)):
        assert l.g6d_frame_ingest_area(*args, None) == -1, args                    # G6D_EINVAL before any HIP call
    assert l.g6d_frame_ingest_area(p, None, 0, p, 1, 8, 8, p, None) == 0           # no frames: nothing to launch
    for args in ((None, p, p, 1, 8, 8, p, p, 4, 4, 8), (p, p, p, 1, 8, 8, p, None, 4, 4, 8), (p, p, p, 0, 8, 8, p, p, 4, 4, 8),
                 (p, p, p, 1, 8, 8, p, p, 0, 4, 8), (p, p, p, 1, 8, 8, p, p, 4, 4, 0), (p, p, p, 1, 8, 8, p, p, 4, 4, 9)):
        assert l.g6d_frame_crop_area(*args, None) == -1, args
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_crop_area(torch.zeros(96, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 8, 8, 3), dtype=torch.uint8),
                            torch.zeros((1, 9)), 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_ingest_area(torch.zeros(96, dtype=torch.uint8), None, 1, torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 3, 3)))
