"""Device-side frame ingest (reference prepare.py:16-42 `video2image` + predict.py:45,52-54): camera-native frames -> the uint8 RGB
working-resolution images and intrinsics the networks take, in ONE launch of g6d_frame_ingest (csrc/ingest.hip) for any number of frames.

A `Frame` describes one picture as a camera or a video decoder delivers it: packed rgb24 / bgr24 / rgba32 / bgra32, packed 4:2:2
(yuyv422 / uyvy422), NV12, planar 4:2:0 (i420 / yv12), 10-bit P010 or 8-bit mono (gray8), limited or full range, any size up to
8192, any row pitch, host or device memory, optionally turned by quarter turns.  `plan` places it in a canvas (scaled to fit, top-left
corner) and maps its intrinsics; `ingest_frames` uploads what lives on the host through pinned memory without blocking and launches once.
A Frame with a `Lens` (a calibrated distortion model beside its K) is undistorted in the same launch (g6d_frame_ingest_mesh): the host
evaluates the model once per camera into a coarse mesh of fixed-point source coordinates, the kernel interpolates it with integers.
The reference's `--resolution R` is `canvas_for(R, h, w)`; its `--transpose` is rotate=180 with cv2 >= 4.5 (two flips) and
rotate=90 with older versions (transpose + horizontal flip).  The scaling is the integer bilinear of DESIGN.md §4.17, not cv2's float one.
"""
import collections
import ctypes as C
import dataclasses

import numpy as np
import torch

from . import eval as EV
from . import lib as _lib
from . import ops

FORMATS = {"rgb24": 0, "bgr24": 1, "rgba32": 2, "bgra32": 3, "nv12": 4, "yuyv422": 5, "uyvy422": 6, "i420": 7, "yv12": 8, "p010": 9, "gray8": 10}
MATRICES = {"bt601": 0, "bt709": 1, "bt601-full": 2, "bt709-full": 3}     # limited range, full range
BPP = {"rgb24": 3, "bgr24": 3, "rgba32": 4, "bgra32": 4, "nv12": 1, "yuyv422": 2, "uyvy422": 2, "i420": 1, "yv12": 1, "p010": 2,
       "gray8": 1}                                       # bytes per luma sample (per pixel for the packed formats)
PACKED_422 = ("yuyv422", "uyvy422")
SEMI_PLANAR = ("nv12", "p010")                           # a Y plane and one plane of interleaved UV pairs
PLANAR = ("i420", "yv12")                                # a Y plane and two chroma planes
READ_ONLY = ("p010", "gray8")                            # formats a Frame can have and a Sink cannot
MAX_SIZE = 8192
RECORD_BYTES = C.sizeof(_lib.G6dFrame)                   # one record of a frame table
LENS_MODELS = {"brown": (4, 5, 8), "fisheye": (4,)}      # model -> admissible numbers of coefficients
MESH_STEPS = (16, 8, 4, 2)
MESH_CACHE = 64                                          # device meshes kept per process (one per camera, plan and device)


def _strides(a):
    return tuple(a.stride()) if torch.is_tensor(a) else a.strides


def _u8(a, what):
    if not torch.is_tensor(a):
        a = np.asarray(a)
    if a.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"Frame: {what} must be uint8")
    if not 1 <= a.ndim <= 3:
        raise ValueError(f"Frame: {what} must have 1 to 3 dimensions")
    return a


def _bytes(a, what, fmt):
    """_u8 that also takes the uint16 samples of a p010 frame: the same memory as little-endian bytes (the last dimension doubles)."""
    if not torch.is_tensor(a):
        a = np.asarray(a)
    if fmt == "p010" and a.dtype in (np.uint16, getattr(torch, "uint16", None)) and a.ndim >= 1:
        if torch.is_tensor(a):
            a = (a if a.stride(-1) == 1 else a.contiguous()).view(torch.uint8)
        else:
            a = (a if a.strides[-1] == 2 else np.ascontiguousarray(a)).astype("<u2", copy=False).view(np.uint8)
    return _u8(a, what)


def _rows(a, inner):
    """a ([rows, bytes] or [rows, w, c]) -> (a with unit-stride rows, pitch in bytes); copies only a layout a pitch cannot describe."""
    st = _strides(a)
    ok = st[-1] == 1 and (a.ndim == 2 or st[1] == inner) and (a.shape[0] == 1 or st[0] >= a.shape[1] * (inner if a.ndim == 3 else 1))
    if not ok:
        a = a.contiguous() if torch.is_tensor(a) else np.ascontiguousarray(a)
        st = _strides(a)
    return a, int(st[0])


def _span(a, row_bytes, rows, pitch, offset=0):
    """Flat view of `rows` rows of `row_bytes` bytes, `pitch` apart, inside a's memory (checked against a's extent)."""
    need = (rows - 1) * pitch + row_bytes
    st, sh = _strides(a), a.shape
    extent = 1 + sum((n - 1) * s for n, s in zip(sh, st))
    if offset + need > extent:
        raise ValueError(f"Frame: the buffer holds {extent} bytes, {offset + need} are needed for {rows} rows of pitch {pitch}")
    if torch.is_tensor(a):
        return torch.as_strided(a, (need,), (1,), a.storage_offset() + offset)
    base = np.lib.stride_tricks.as_strided(a, (extent,), (1,))
    return base[offset:offset + need]


@dataclasses.dataclass(frozen=True)
class Lens:
    """A lens distortion model in OpenCV's conventions, immutable and hashable; goes with a Frame's K: Frame(..., K=K, lens=Lens(...)).
    With (x, y) normalised undistorted coordinates and r2 = x^2 + y^2:
      "brown", coeffs k1 k2 p1 p2 [k3 [k4 k5 k6]]: rad = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
        xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2), yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y;
      "fisheye", coeffs k1 k2 k3 k4: t = atan(r), td = t (1 + k1 t^2 + k2 t^4 + k3 t^6 + k4 t^8), (xd, yd) = (td / r) (x, y) (factor 1 at r = 0).
    The ingested picture is the scaled virtual pinhole picture of the source's size with intrinsics new_K (default: the frame's K, as
    cv2.undistort); pixels that look past the source's edge are black.  tol: the mesh's largest distance to the model in canvas pixels.
    minify: "point" samples the source once per canvas pixel in every call; "area" makes a call that is itself minify="area"
    (ingest_frames_keep, StreamTracker, track_streams) average n x n sub-samples per canvas pixel through the mesh, n = 1 / 2 / 4 / 8 chosen
    per mesh by `samples_log2` (include/gen6d_hip.h), and changes nothing in a point call."""
    model: str
    coeffs: tuple
    new_K: tuple = None
    tol: float = 1 / 16
    minify: str = "point"

    def __post_init__(self):
        if self.model not in LENS_MODELS:
            raise ValueError(f"Lens: unknown model {self.model!r} (one of {sorted(LENS_MODELS)})")
        if self.minify not in ("point", "area"):
            raise ValueError(f"Lens: minify must be \"point\" or \"area\", not {self.minify!r}")
        c = tuple(float(v) for v in np.asarray(self.coeffs, np.float64).reshape(-1))
        if len(c) not in LENS_MODELS[self.model]:
            raise ValueError(f"Lens: a {self.model} lens takes {' / '.join(map(str, LENS_MODELS[self.model]))} coefficients, not {len(c)}")
        if not np.isfinite(c).all() or not (np.isfinite(self.tol) and self.tol > 0):
            raise ValueError("Lens: finite coefficients and a positive tol expected")
        K = self.new_K
        if K is not None:
            K = tuple(float(v) for v in np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, np.float64).reshape(9))
        for name, v in (("coeffs", c), ("new_K", K), ("tol", float(self.tol))):       # normalised: equal lenses compare and hash equal
            object.__setattr__(self, name, v)

    def distort(self, x, y):
        """Normalised undistorted (x, y) -> normalised distorted (xd, yd), float64."""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        r2 = x * x + y * y
        if self.model == "fisheye":
            k1, k2, k3, k4 = self.coeffs
            r = np.sqrt(r2)
            t = np.arctan(r)
            t2 = t * t
            td = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r > 0, td / np.where(r > 0, r, 1.0), 1.0)
            return x * s, y * s
        k1, k2, p1, p2, k3, k4, k5, k6 = self.coeffs + (0.0,) * (8 - len(self.coeffs))
        with np.errstate(divide="ignore", invalid="ignore"):
            rad = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
            return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y

    def source_coords(self, K, ws, hs, rotate, out_w, out_h, X, Y):
        """Canvas pixel coordinates (X, Y) of the out_w x out_h picture of a ws x hs source -> the source coordinates (ud, vd) the lens
        puts them at, float64: undo the quarter turn, the scaling u = (x + 0.5) ws / wt - 0.5, new_K^-1, the model, K."""
        wt, ht = (out_h, out_w) if rotate in (90, 270) else (out_w, out_h)
        X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
        x, y = {0: (X, Y), 90: (Y, ht - 1 - X), 180: (wt - 1 - X, ht - 1 - Y), 270: (wt - 1 - Y, X)}[rotate]
        u, v = (x + 0.5) * ws / wt - 0.5, (y + 0.5) * hs / ht - 0.5
        K = np.asarray(K, np.float64).reshape(3, 3)
        Ni = np.linalg.inv(K if self.new_K is None else np.asarray(self.new_K, np.float64).reshape(3, 3))
        with np.errstate(divide="ignore", invalid="ignore"):
            w = Ni[2, 0] * u + Ni[2, 1] * v + Ni[2, 2]
            xd, yd = self.distort((Ni[0, 0] * u + Ni[0, 1] * v + Ni[0, 2]) / w, (Ni[1, 0] * u + Ni[1, 1] * v + Ni[1, 2]) / w)
            w = K[2, 0] * xd + K[2, 1] * yd + K[2, 2]
            return (K[0, 0] * xd + K[0, 1] * yd + K[0, 2]) / w, (K[1, 0] * xd + K[1, 1] * yd + K[1, 2]) / w

    def mesh(self, K, ws, hs, rotate, out_w, out_h):
        """-> (nodes int32 [ny, nx, 2], step_log2): source coordinates in 1/65536 pixels at the canvas pixels (g c, g r), c = 0 ..
        ceil(out_w / g), r likewise, clamped to +-2^30 (a coordinate that is not finite counts as far outside).  g = 2^step_log2 is the
        largest of 16, 8, 4, 2 at which the bilinear interpolation of the nodes stays within tol * max(ws / wt, hs / ht) source pixels
        (tol canvas pixels) of the model at every cell's centre and edge midpoints."""
        wt, ht = (out_h, out_w) if rotate in (90, 270) else (out_w, out_h)
        at = lambda X, Y: np.stack(self.source_coords(K, ws, hs, rotate, out_w, out_h, X, Y), -1)
        bound = self.tol * max(ws / wt, hs / ht)
        for g in MESH_STEPS:
            xs, ys = np.arange(-(-out_w // g) + 1, dtype=np.float64) * g, np.arange(-(-out_h // g) + 1, dtype=np.float64) * g
            m = at(*np.meshgrid(xs, ys))
            xc, yc = xs[:-1] + g / 2, ys[:-1] + g / 2
            with np.errstate(invalid="ignore"):
                miss = max(np.abs(at(*np.meshgrid(xc, ys)) - (m[:, :-1] + m[:, 1:]) / 2).max(),                 # horizontal edges
                           np.abs(at(*np.meshgrid(xs, yc)) - (m[:-1] + m[1:]) / 2).max(),                       # vertical edges
                           np.abs(at(*np.meshgrid(xc, yc)) - (m[:-1, :-1] + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]) / 4).max())
            if miss <= bound:                                        # (a NaN fails this)
                fixed = np.clip(np.rint(np.nan_to_num(m, nan=np.inf) * 65536.0), -2.0 ** 30, 2.0 ** 30)
                return np.ascontiguousarray(fixed.astype(np.int32)), g.bit_length() - 1
        raise ValueError(f"{self!r}: a mesh of step 2 misses the model by {miss:.3g} source pixels at a {ws} x {hs} source in a {out_w} x "
                         f"{out_h} picture, more than tol allows ({bound:.3g})")

    @staticmethod
    def samples_log2(nodes, step_log2, ws, hs):
        """-> L: a minify="area" lens averages 2^L x 2^L sub-samples per canvas pixel of this mesh (int32 nodes [ny, nx, 2], `mesh`).
        Over the horizontally and vertically adjacent node pairs whose two nodes lie inside [-0.5, ws - 0.5] x [-0.5, hs - 0.5], M is the
        largest max(|dx|, |dy|) / (65536 g): the source pixels one canvas pixel spans.  n = 1 for M < 1.5, 2 for M < 3, 4 for M < 6, else
        8; 1 when there is no such pair.  Exact integers."""
        m = np.asarray(nodes).astype(np.int64)
        inside = (m[..., 0] >= -32768) & (m[..., 0] <= ws * 65536 - 32768) & (m[..., 1] >= -32768) & (m[..., 1] <= hs * 65536 - 32768)
        span = 0
        for a, b, ok in ((m[:, :-1], m[:, 1:], inside[:, :-1] & inside[:, 1:]), (m[:-1], m[1:], inside[:-1] & inside[1:])):
            if ok.any():
                span = max(span, int(np.abs(b - a).max(-1)[ok].max()))
        unit = 65536 << step_log2                                    # M = span / unit
        return sum(2 * span >= k * unit for k in (3, 6, 12))


class Frame:
    """One source picture.  data: uint8 numpy array or torch tensor (host or device), [H,W,C] (C = 3 / 4 / 2 / 1 as the format says; sizes
    and the pitch are taken from it), [rows, row bytes] or a flat buffer (give width / height / pitch).  Formats:
      rgb24 / bgr24 / rgba32 / bgra32   packed, 3 / 4 bytes per pixel;
      yuyv422 / uyvy422                 packed 4:2:2, 2 bytes per pixel ([H,W,2] or rows of bytes); even width, any height;
      nv12                              one [H*3/2, pitch] buffer (Y rows, then H/2 rows of interleaved UV) or `data` = Y plane and `uv` = UV
                                        plane ([H/2, bytes] or [H/2, W/2, 2]); even sizes;
      i420 / yv12                       planar 4:2:0, Y then U then V (yv12: V then U): one [H*3/2, pitch] buffer of contiguous planes (even
                                        pitch, the chroma pitch is pitch / 2) or `data` = Y plane and `uv` = the two chroma planes stacked,
                                        [H, uv_pitch]; even sizes.  Three separately allocated planes are out of scope;
      p010                              nv12's layout with 16-bit little-endian samples (value = word >> 6): uint16 arrays, or uint8 byte
                                        buffers with width / height / pitch; pitches are in BYTES and even;
      gray8                             [H,W], or rows of bytes with a width.
    rotate: quarter turns clockwise applied after scaling (0 / 90 / 180 / 270).  K: the camera's intrinsics in SOURCE pixel coordinates, or
    None for predict.py's pseudo intrinsics of the ingested picture.  matrix (YUV formats): "bt601" / "bt709" (limited range),
    "bt601-full" / "bt709-full" (full range, e.g. MJPEG-sourced YUV).  lens: the camera's `Lens` (needs K): the ingested picture is the
    undistorted one, and its intrinsics come from the lens's new_K."""

    def __init__(self, data, fmt="rgb24", width=None, height=None, pitch=None, rotate=0, K=None, uv=None, uv_pitch=None, matrix="bt601",
                 lens=None):
        if fmt not in FORMATS:
            raise ValueError(f"Frame: unknown format {fmt!r} (one of {sorted(FORMATS)})")
        if matrix not in MATRICES:
            raise ValueError(f"Frame: unknown matrix {matrix!r} (one of {sorted(MATRICES)})")
        if rotate not in (0, 90, 180, 270):
            raise ValueError(f"Frame: rotate must be 0, 90, 180 or 270, not {rotate!r}")
        if lens is not None and not isinstance(lens, Lens):
            raise ValueError("Frame: lens must be an ingest.Lens")
        if lens is not None and K is None:
            raise ValueError("Frame: a frame with a lens must carry the camera's K")
        bpp = BPP[fmt]
        semi, planar = fmt in SEMI_PLANAR, fmt in PLANAR      # chroma beside the luma plane: one interleaved plane / two planes
        two = semi or planar
        if uv is not None and not two:
            raise ValueError(f"Frame: uv is the chroma of an nv12 / p010 / i420 / yv12 frame; a {fmt} frame is one packed plane")
        d = _bytes(data, "data", fmt)
        if d.ndim == 3:
            if two or d.shape[2] != bpp:
                raise ValueError(f"Frame: a {fmt} frame cannot be a {tuple(d.shape)} array")
            d, p = _rows(d, bpp)
            h, w = d.shape[:2]
        elif d.ndim == 2:
            d, p = _rows(d, 1)
            if two and uv is None:
                if d.shape[0] % 3:
                    raise ValueError(f"Frame: a one-buffer {fmt} frame has H*3/2 rows")
                h = d.shape[0] * 2 // 3
            else:
                h = d.shape[0]
            w = width if width is not None else d.shape[1] // bpp
        else:
            if width is None or height is None:
                raise ValueError("Frame: a flat buffer needs width and height")
            if not (torch.is_tensor(d) or d.flags.c_contiguous) or _strides(d)[0] != 1:
                d = d.contiguous() if torch.is_tensor(d) else np.ascontiguousarray(d)
            h, w, p = height, width, (pitch if pitch is not None else int(width) * bpp)
        if (width is not None and int(width) != w) or (height is not None and int(height) != h):
            raise ValueError(f"Frame: width / height {width} x {height} given, the data says {w} x {h}")
        if pitch is not None and d.ndim > 1 and int(pitch) != p and d.shape[0] > 1:
            raise ValueError(f"Frame: pitch {pitch} given, the array's rows are {p} bytes apart")
        w, h, p = int(w), int(h), int(p)
        if not (1 <= w <= MAX_SIZE and 1 <= h <= MAX_SIZE):
            raise ValueError(f"Frame: size {w} x {h} outside 1..{MAX_SIZE}")
        if p < w * bpp:
            raise ValueError(f"Frame: pitch {p} is smaller than a row of {w} {fmt} pixels")
        if fmt in PACKED_422 and w % 2:
            raise ValueError(f"Frame: a {fmt} frame has an even width, not {w}")
        self.fmt, self.width, self.height, self.pitch, self.rotate, self.matrix = fmt, w, h, p, int(rotate), matrix
        self.K = None if K is None else np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, np.float64).reshape(3, 3)
        self.lens = lens
        self.plane0 = _span(d, w * bpp, h, p)
        self.plane1, self.uv_pitch = None, 0
        if two:
            if w % 2 or h % 2:
                raise ValueError(f"Frame: an {fmt} frame has even width and height, not {w} x {h}")
            if fmt == "p010" and p % 2:
                raise ValueError(f"Frame: a p010 pitch is in bytes and even, not {p}")
            # plane1: h/2 rows of interleaved pairs, or the two chroma planes one after the other (h/2 + h/2 rows of w/2 bytes)
            crow, crows = (w * bpp, h // 2) if semi else (w // 2, h)
            if uv is None:
                if planar and p % 2:
                    raise ValueError(f"Frame: a one-buffer {fmt} frame has an even pitch (its chroma pitch is half of it), not {p}")
                up = p if semi else p // 2
                if uv_pitch is not None and int(uv_pitch) != up:
                    raise ValueError(f"Frame: a one-buffer {fmt} frame has one pitch" + (" (the chroma pitch is half of it)" if planar else ""))
                self.uv_pitch = up
                self.plane1 = _span(d, crow, crows, up, offset=p * h)
            else:
                u = _bytes(uv, "uv", fmt)
                if type(u) is not type(d) or (torch.is_tensor(u) and u.device != d.device):
                    raise ValueError("Frame: data and uv must live in the same kind of memory")
                if u.ndim == 1:
                    up = int(uv_pitch) if uv_pitch is not None else crow
                else:
                    u, up = _rows(u, 2 * bpp)
                    if u.shape[0] != crows or (u.ndim == 3 and (planar or u.shape[1] != w // 2 or u.shape[2] != 2 * bpp)):
                        raise ValueError(f"Frame: uv plane {tuple(u.shape)} does not belong to a {w} x {h} {fmt} frame")
                    if uv_pitch is not None and int(uv_pitch) != up and u.shape[0] > 1:
                        raise ValueError(f"Frame: uv_pitch {uv_pitch} given, the array's rows are {up} bytes apart")
                if up < crow:
                    raise ValueError(f"Frame: uv pitch {up} is smaller than a chroma row of a {w} pixel wide {fmt} frame ({crow} bytes)")
                if fmt == "p010" and up % 2:
                    raise ValueError(f"Frame: a p010 pitch is in bytes and even, not {up}")
                self.uv_pitch = up
                self.plane1 = _span(u, crow, crows, up)

    @property
    def on_device(self):
        return torch.is_tensor(self.plane0) and self.plane0.device.type != "cpu"

    def rotated_size(self):
        """(height, width) of the source after the rotation."""
        return (self.width, self.height) if self.rotate in (90, 270) else (self.height, self.width)


def canvas_for(resolution, h, w, rotate=0):
    """(H, W) of the image the reference's video2image makes of an h x w frame at --resolution (prepare.py:27-29), turned by `rotate`."""
    ratio = resolution / max(h, w)
    H, W = int(ratio * h), int(ratio * w)
    return (W, H) if rotate in (90, 270) else (H, W)


def pixel_map(frame, out_h, out_w):
    """3x3 affine map (float64) from SOURCE pixel coordinates to pixel coordinates of the ingested out_h x out_w picture: the half-pixel
    centre scaling u' = (u + 0.5) * wt / ws - 0.5 followed by the rotation's pixel map (include/gen6d_hip.h)."""
    wt, ht = (out_h, out_w) if frame.rotate in (90, 270) else (out_w, out_h)
    sx, sy = wt / frame.width, ht / frame.height
    S = np.array([[sx, 0, 0.5 * sx - 0.5], [0, sy, 0.5 * sy - 0.5], [0, 0, 1]], np.float64)
    R = {0: [[1, 0, 0], [0, 1, 0], [0, 0, 1]], 90: [[0, -1, ht - 1], [1, 0, 0], [0, 0, 1]],
         180: [[-1, 0, wt - 1], [0, -1, ht - 1], [0, 0, 1]], 270: [[0, 1, 0], [-1, 0, wt - 1], [0, 0, 1]]}[frame.rotate]
    return np.asarray(R, np.float64) @ S


def plan(frame, canvas_hw):
    """-> (out_h, out_w, K'): the size of the scaled and rotated picture that fits the canvas with the source's aspect ratio (it sits at the
    top-left corner) and its intrinsics, float64: A @ K for a frame with K (A @ new_K of its lens), predict.py's pseudo K of the picture
    otherwise."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    if H < 1 or W < 1:
        raise ValueError("plan: the canvas must be at least 1 x 1")
    hs, ws = frame.rotated_size()
    if H * ws <= W * hs:
        out_h, out_w = H, max(1, H * ws // hs)
    else:
        out_w, out_h = W, max(1, W * hs // ws)
    if frame.K is None:
        return out_h, out_w, EV.pseudo_K(out_h, out_w).astype(np.float64)
    K = frame.K if frame.lens is None or frame.lens.new_K is None else np.asarray(frame.lens.new_K, np.float64).reshape(3, 3)
    return out_h, out_w, pixel_map(frame, out_h, out_w) @ K


def source_K(frame, canvas_hw):
    """Intrinsics (float64 [3,3]) of the frame's own, unturned pixel grid under which a pose found on the canvas projects into the SOURCE
    picture (emit.Sink(view="source")): Frame.K if the frame has one, else inv(pixel_map) @ pseudo_K of the planned picture.  Either
    way pixel_map @ source_K is the K' that `plan` hands the networks: the pose is the same, only the pixel grid differs, quarter turn
    included.  A frame with a lens has no such K (its source is distorted: a straight box edge is a curve in it)."""
    if frame.lens is not None:
        raise ValueError("source_K: a frame with a lens has a distorted source picture; the source view of lens frames is out of scope")
    if frame.K is not None:
        return frame.K.copy()
    out_h, out_w, K = plan(frame, canvas_hw)
    return np.linalg.inv(pixel_map(frame, out_h, out_w)) @ K


class Staged:
    """What `ingest_frames_keep` leaves on the device: `table`, the uint8 tensor of the call's n lib.G6dFrame records (record i
    is frames[i]; its `slot` field is the frame's canvas slot), for launches that read the source pictures again
    (emit.emit_source_frames, ops.frame_crop through a `SourceTable`).  It keeps the staging buffer and the device-resident planes referenced; `batch` is the canvas count B."""

    def __init__(self, table, frames, slots, batch):
        self.table, self.frames, self.slots, self.batch = table, frames, slots, batch
        self.n, self.device = len(frames), table.device


class SourceTable:
    """The source pictures of a batch of canvases, for launches that cut from them (`DeviceChain.query_batch_source`,
    ops.frame_crop): `table`, a uint8 tensor of lib.G6dFrame records, and `rec` int32 [B]: the record of canvas slot b, or -1 for a slot
    without one, which is served from its canvas.  Both live on the device and are read there, so a captured graph can hold them.
    `SourceTable.of(staged)` pairs a `Staged` table with the map of its slots; `load(staged)` refills a static pair (a lane's, read by
    its captured graph) with them.  The kernel cannot check rec against the table (a wrong value is an out-of-bounds read): the map is
    built on the host and checked there, before it travels."""

    def __init__(self, table, rec):
        self.table, self.rec = table, rec

    @staticmethod
    def _upload(rec, n, dev):
        """Host map (int32 numpy) of a table of n records -> device tensor on the current stream, no synchronisation."""
        if rec.size and int(rec.max()) >= n:
            raise ValueError(f"SourceTable: a slot names record {int(rec.max())} of a table of {n}")
        t = torch.from_numpy(rec)
        return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)

    @staticmethod
    def slot_records(staged):
        """-> int32 [B] numpy, B the canvas count of the ingest: rec[slot of frame i] = i, -1 elsewhere.  A frame with a `Lens` gets -1
        as well: its source picture is distorted, the canvas is the undistorted one."""
        rec = np.full(staged.batch, -1, np.int32)
        for i, (f, s) in enumerate(zip(staged.frames, staged.slots)):
            if f.lens is None:
                rec[s] = i
        return rec

    @classmethod
    def of(cls, staged):
        """The table an `ingest_frames_keep` call left, with its slot map uploaded on the current stream (no synchronisation)."""
        return cls(staged.table, cls._upload(cls.slot_records(staged), staged.n, staged.device))

    def load(self, staged):
        """Copy the table and the slot map of an `ingest_frames_keep` call into this pair's own buffers, on the current stream.  The
        caller keeps `staged` alive as long as launches read this pair: the records point into its planes."""
        if staged.table.numel() > self.table.numel() or staged.batch != self.rec.numel():
            raise ValueError(f"SourceTable.load: {staged.n} records for {staged.batch} slots do not fit a table of "
                             f"{self.table.numel() // RECORD_BYTES} records and {self.rec.numel()} slots")
        self.table[:staged.table.numel()].copy_(staged.table)
        self.rec.copy_(self._upload(self.slot_records(staged), staged.n, staged.device))


def _host(p):
    return p.numpy() if torch.is_tensor(p) else p


_meshes = collections.OrderedDict()     # (device, lens, K, ws, hs, rotate, out_w, out_h) -> _Mesh, least recently used first


class _Mesh:
    """A lens mesh on its way to / in device memory: host (int32 [ny, nx, 2], until uploaded), nodes (the device tensor), step_log2,
    samples_log2 (what an area call writes into the mesh record: 0 for a lens with minify="point") and the stream and event of the
    upload (a launch on another stream waits for the event on the device)."""

    def __init__(self, host, step_log2, samples_log2=0):
        self.host, self.step_log2, self.samples_log2, self.nodes, self.stream, self.event = host, step_log2, samples_log2, None, None, None


def _mesh_key(frame, out_h, out_w, dev):
    return (dev, frame.lens, frame.K.tobytes(), frame.width, frame.height, frame.rotate, out_w, out_h)


MINIFY = ("point", "area")                               # how a picture that shrinks is sampled


def ingest_frames(frames, out, K_out, slots=None, stream=None):
    """frames (Frame objects) -> out[slot] uint8 [B,H,W,3] and K_out[slot] float32 [B,3,3], slot i by default; one launch on `stream` (the
    current stream if None).  Host-resident planes and the descriptor table are gathered in one pinned staging buffer and travel in one
    non-blocking copy (copying planes that already are pinned one by one was measured slower); device-resident planes
    are recorded on the stream.  Frames with a lens make it one launch of g6d_frame_ingest_mesh instead: a camera's mesh is built on its
    first frame, travels in the same copy and stays on the device.  Does not synchronise.  Slots no frame names keep their content.
    The scaling is the point-sampled bilinear rule; `ingest_frames_keep(..., minify="area")` filters a picture that shrinks."""
    return _ingest(frames, out, K_out, slots, stream, False)


def ingest_frames_keep(frames, out, K_out, slots=None, stream=None, minify="point"):
    """`ingest_frames` that returns (out, staged): `staged` (a `Staged`) holds the device-resident frame table of this call and keeps the
    staging buffer and the device planes alive, so that a later launch on the same stream can read the source pictures again
    (emit.emit_source_frames).  The launch is the same.
    minify: "point" is the bilinear rule, which reads two source pixels per axis however far the picture shrinks; "area" makes it one
    launch of g6d_frame_ingest_area, with or without lenses: every axis that shrinks is box-filtered with exact integer weights, a frame
    that does not shrink gets the same bytes as under "point", a frame whose `Lens` has minify="area" is supersampled through its mesh
    (n x n sub-samples per canvas pixel, `Lens.samples_log2`), and a frame whose lens keeps the default keeps the mesh rule's bytes.
    (`ingest_frames` keeps its parameters as they are, the default tracker's recorded launch schedule lists them: a caller that wants
    the filtered ingest and not the table takes `ingest_frames_keep(..., minify="area")[0]`; keeping the table costs nothing.)"""
    return _ingest(frames, out, K_out, slots, stream, True, minify)


def _ingest(frames, out, K_out, slots, stream, keep, minify="point"):
    if minify not in MINIFY:
        raise ValueError(f"ingest_frames_keep: minify must be \"point\" or \"area\", not {minify!r}")
    frames = list(frames)
    n = len(frames)
    if out.dim() != 4 or out.shape[3] != 3:
        raise ValueError("ingest_frames: out must be a uint8 [B,H,W,3] tensor")
    B, H, W = out.shape[:3]
    slots = list(range(n)) if slots is None else [int(s) for s in slots]
    if len(slots) != n or len(set(slots)) != n or any(not 0 <= s < B for s in slots):
        raise ValueError(f"ingest_frames: one distinct slot in [0, {B}) per frame expected")
    dev = out.device
    cuda = dev.type == "cuda"
    size = C.sizeof(_lib.G6dFrame)
    table = (_lib.G6dFrame * max(n, 1))()
    mtable = (_lib.G6dMesh * max(n, 1))()      # used when some frame has a lens
    staged = []                                # host planes: (frame index, field, bytes)
    meshes, fresh = {}, {}                     # frame index -> _Mesh; key -> _Mesh built in this call (cached once it is uploaded)
    for i, f in enumerate(frames):
        if not isinstance(f, Frame):
            raise ValueError("ingest_frames: Frame objects expected")
        out_h, out_w, K = plan(f, (H, W))
        e = table[i]
        e.pitch0, e.pitch1, e.width, e.height = f.pitch, f.uv_pitch, f.width, f.height
        e.format, e.rotate, e.matrix, e.slot, e.out_w, e.out_h = FORMATS[f.fmt], f.rotate, MATRICES[f.matrix], slots[i], out_w, out_h
        e.K[:] = np.asarray(K, np.float64).astype(np.float32).reshape(9).tolist()
        for field, p in (("plane0", f.plane0), ("plane1", f.plane1)):
            if p is None:
                continue
            if f.on_device:
                if p.device != dev:
                    raise ValueError(f"ingest_frames: frame {i} lives on {p.device}, out on {dev}")
                setattr(e, field, p.data_ptr())
            else:
                staged.append((i, field, _host(p)))
        if f.lens is not None:
            key = _mesh_key(f, out_h, out_w, dev)
            m = _meshes.get(key) or fresh.get(key)
            if m is None:
                nodes, lg = f.lens.mesh(f.K, f.width, f.height, f.rotate, out_w, out_h)
                m = fresh[key] = _Mesh(nodes, lg, Lens.samples_log2(nodes, lg, f.width, f.height) if f.lens.minify == "area" else 0)
            elif key in _meshes:
                _meshes.move_to_end(key)                             # most recently used
            meshes[i] = m
    if n == 0:
        return (out, Staged(torch.empty(0, dtype=torch.uint8, device=dev), [], [], B)) if keep else out
    # layout of the upload (one pinned buffer, one copy): staged planes | new meshes | table | mesh table
    offs, total = [], 0
    for p in [p for _, _, p in staged] + [m.host.reshape(-1).view(np.uint8) for m in fresh.values()]:
        offs.append(total)
        total += (p.shape[0] + 255) & ~255
    toff = total
    moff = toff + n * size
    total = moff + (n * C.sizeof(_lib.G6dMesh) if meshes else 0)
    ctx = torch.cuda.stream(stream) if (cuda and stream is not None) else None
    if ctx is not None:
        ctx.__enter__()
    try:
        if cuda:
            cur = torch.cuda.current_stream(dev)
            for f in frames:
                if f.on_device:
                    f.plane0.record_stream(cur)
                    if f.plane1 is not None:
                        f.plane1.record_stream(cur)
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            buf = torch.empty(total, dtype=torch.uint8, device=dev)
        else:
            host = buf = torch.empty(total, dtype=torch.uint8)
        hn, base = host.numpy(), buf.data_ptr()
        for (i, field, p), off in zip(staged, offs):
            hn[off:off + p.shape[0]] = p
            setattr(table[i], field, base + off)
        for m, off in zip(fresh.values(), offs[len(staged):]):
            hn[off:off + m.host.nbytes] = m.host.reshape(-1).view(np.uint8)
            m.nodes = torch.empty(m.host.shape, dtype=torch.int32, device=dev)
        for i, m in meshes.items():
            mtable[i].nodes, mtable[i].ny, mtable[i].nx, mtable[i].step_log2 = m.nodes.data_ptr(), m.nodes.shape[0], m.nodes.shape[1], m.step_log2
            mtable[i].samples_log2 = m.samples_log2 if minify == "area" else 0
        hn[toff:moff] = np.frombuffer(table, np.uint8, n * size)
        if meshes:
            hn[moff:] = np.frombuffer(mtable, np.uint8, total - moff)
        if cuda:
            buf.copy_(host, non_blocking=True)
        for (key, m), off in zip(fresh.items(), offs[len(staged):]):  # out of the staging buffer into the mesh's own memory, on this stream
            m.nodes.view(-1).copy_(buf[off:off + m.host.nbytes].view(torch.int32))
            m.host = None
            if cuda:
                m.stream, m.event = cur, torch.cuda.Event()
                m.event.record(cur)
            _meshes[key] = m
        while len(_meshes) > MESH_CACHE:
            _meshes.popitem(last=False)
        if cuda:
            for m in meshes.values():
                if m.stream != cur:                                   # uploaded on another lane's stream: this launch waits for it on the device
                    cur.wait_event(m.event)
                    m.nodes.record_stream(cur)
        if minify == "area":
            ops.frame_ingest_area(buf[toff:moff], buf[moff:] if meshes else None, n, out, K_out)
        elif meshes:
            ops.frame_ingest_mesh(buf[toff:moff], buf[moff:], n, out, K_out)
        else:
            ops.frame_ingest(buf[toff:], n, out, K_out)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return (out, Staged(buf[toff:moff], frames, slots, B)) if keep else out
