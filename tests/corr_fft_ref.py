"""numpy restatement of the frequency-domain correlation (gen6d_amd/csrc/corr_fft.hip, corr_fft_plan.h), step for step: overlap-save over
T x T windows, radix-2 decimation-in-frequency FFTs with two real sequences per complex transform (two window rows; spectrum columns 0 and
T/2; two output rows), the per-bin complex products as one real GEMM against B' = [Wr | -Wi ; Wi | Wr], the inverse scaled by 1 / T^2.
Every array keeps the dtype it is called with: float64 is the check of the algorithm (tests/test_corr_fft_plan_cpu.py), float32 shows the
error the same arithmetic has in the kernels' precision (tests/test_corr_fft_gpu.py sets its bars from it)."""
import numpy as np


def bit_reverse(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def fft_dif(re, im):
    """Forward DFT along the last axis (a power of two), sum_x z[x] e^{-2 pi i k x / n}, in the arrays' dtype; natural order out."""
    n, dt = re.shape[-1], re.dtype
    lead = re.shape[:-1]
    re, im = re.copy(), im.copy()
    h = n // 2
    while h >= 1:
        r, i = re.reshape(lead + (n // (2 * h), 2, h)), im.reshape(lead + (n // (2 * h), 2, h))
        ang = 2 * np.pi * (np.arange(h) * (n // 2 // h)) / n
        c, s = np.cos(ang).astype(dt), np.sin(ang).astype(dt)
        ur, ui, vr, vi = r[..., 0, :], i[..., 0, :], r[..., 1, :], i[..., 1, :]
        dr, di = ur - vr, ui - vi
        re = np.stack([ur + vr, dr * c + di * s], -2).reshape(lead + (n,))
        im = np.stack([ui + vi, di * c - dr * s], -2).reshape(lead + (n,))
        h //= 2
    br = bit_reverse(n)
    return re[..., br], im[..., br]


def ifft_dif(re, im):
    """Unscaled inverse DFT along the last axis: the forward routine with real and imaginary parts exchanged."""
    i, r = fft_dif(im, re)
    return r, i


def tile_list(H, W, T, K):
    """(y0, x0) of every tile in row, column order: the first output pixel; the window starts K // 2 before it."""
    V = T - K + 1
    return [(ty * V, tx * V) for ty in range(-(-H // V)) for tx in range(-(-W // V))]


def windows(x, T, K):
    """x [H, W, C] -> [tiles, T, T, C] windows, zero outside the map."""
    H, W, C = x.shape
    R = K // 2
    pad = np.zeros((H + 2 * T, W + 2 * T, C), x.dtype)
    pad[T:T + H, T:T + W] = x
    return np.stack([pad[T + y0 - R:T + y0 - R + T, T + x0 - R:T + x0 - R + T] for y0, x0 in tile_list(H, W, T, K)])


def forward(win):
    """[tiles, T, T, C] real windows -> X [bins, tiles, 2, C]: bin = ky (T/2 + 1) + kx, plane 0 re, plane 1 im."""
    nt, T, _, C = win.shape
    hb, half = T // 2 + 1, np.asarray(0.5, win.dtype)
    w = np.moveaxis(win, 2, -1)                                          # tiles, y, c, x
    zr, zi = fft_dif(w[:, 0::2], w[:, 1::2])                             # rows 2g + i rows 2g+1
    k = np.arange(hb)
    nk = (T - k) % T
    ar, ai = half * (zr[..., k] + zr[..., nk]), half * (zi[..., k] - zi[..., nk])
    br, bi = half * (zi[..., k] + zi[..., nk]), half * (zr[..., nk] - zr[..., k])
    rr = np.empty((nt, T, C, hb), win.dtype); ri = np.empty_like(rr)
    rr[:, 0::2], rr[:, 1::2], ri[:, 0::2], ri[:, 1::2] = ar, br, ai, bi
    rr, ri = np.moveaxis(rr, 1, -1), np.moveaxis(ri, 1, -1)             # tiles, c, kx, y
    fr, fi = np.empty_like(rr), np.empty_like(ri)
    fr[:, :, 1:T // 2], fi[:, :, 1:T // 2] = fft_dif(rr[:, :, 1:T // 2], ri[:, :, 1:T // 2])
    zr, zi = fft_dif(rr[:, :, 0], rr[:, :, T // 2])                      # columns 0 and T/2 are real: one complex transform
    k = np.arange(T)
    nk = (T - k) % T
    fr[:, :, 0], fi[:, :, 0] = half * (zr[..., k] + zr[..., nk]), half * (zi[..., k] - zi[..., nk])
    fr[:, :, T // 2], fi[:, :, T // 2] = half * (zi[..., k] + zi[..., nk]), half * (zr[..., nk] - zr[..., k])
    X = np.stack([fr, fi], 1)                                            # tiles, plane, c, kx, ky
    return np.ascontiguousarray(X.transpose(4, 3, 0, 1, 2)).reshape(T * hb, nt, 2, C)


def spectra(w, T):
    """w [R, K, K, C] filters -> B' [bins, 2 C, 2 R] float64 (np.fft of the zero-extended filters): row c = [Wr | -Wi], row C + c = [Wi | Wr]."""
    R, K, _, C = w.shape
    z = np.zeros((R, C, T, T))
    z[:, :, :K, :K] = np.asarray(w, np.float64).transpose(0, 3, 1, 2)
    Wf = np.fft.rfft2(z)                                                 # r, c, ky, kx
    Wr, Wi = Wf.real.transpose(2, 3, 1, 0).reshape(-1, C, R), Wf.imag.transpose(2, 3, 1, 0).reshape(-1, C, R)
    return np.concatenate([np.concatenate([Wr, -Wi], 2), np.concatenate([Wi, Wr], 2)], 1)


def gemm(X, B):
    """X [bins, tiles, 2, C], B' [bins, 2 C, 2 R] -> Y [bins, tiles, 2 R] in X's dtype."""
    bins, nt = X.shape[:2]
    return np.matmul(X.reshape(bins, nt, -1), B.astype(X.dtype))


def inverse(Y, T, V):
    """Y [bins, tiles, 2 R] -> [tiles, V, V, R]: inverse real FFT / T^2, positions [0, V)^2 (V even)."""
    hb = T // 2 + 1
    nt, R = Y.shape[1], Y.shape[2] // 2
    y = Y.reshape(T, hb, nt, 2, R).transpose(2, 4, 3, 1, 0)              # tiles, r, plane, kx, ky
    yr, yi = y[:, :, 0], y[:, :, 1]
    gr, gi = np.empty_like(yr), np.empty_like(yi)
    gr[:, :, 1:T // 2], gi[:, :, 1:T // 2] = ifft_dif(yr[:, :, 1:T // 2], yi[:, :, 1:T // 2])
    a, b = ifft_dif(yr[:, :, 0] - yi[:, :, T // 2], yi[:, :, 0] + yr[:, :, T // 2])        # Y[., 0] + i Y[., T/2]: both inverses are real
    gr[:, :, 0], gi[:, :, 0], gr[:, :, T // 2], gi[:, :, T // 2] = a, 0, b, 0
    gr, gi = np.moveaxis(gr[..., :V], -1, 2), np.moveaxis(gi[..., :V], -1, 2)             # tiles, r, y, kx
    ar, ai, br, bi = gr[:, :, 0::2], gi[:, :, 0::2], gr[:, :, 1::2], gi[:, :, 1::2]
    zr, zi = np.empty(ar.shape[:-1] + (T,), Y.dtype), np.empty(ar.shape[:-1] + (T,), Y.dtype)
    zr[..., :hb], zi[..., :hb] = ar - bi, ai + br
    m = np.arange(1, T // 2)
    zr[..., T - m], zi[..., T - m] = (ar + bi)[..., m], (br - ai)[..., m]
    ra, rb = ifft_dif(zr, zi)                                            # re: rows 2g, im: rows 2g + 1
    out = np.empty((nt, R, V, V), Y.dtype)
    sc = np.asarray(1.0 / (T * T), Y.dtype)
    out[:, :, 0::2], out[:, :, 1::2] = ra[..., :V] * sc, rb[..., :V] * sc
    return out.transpose(0, 2, 3, 1)


def scatter(tiles_out, H, W, T, K):
    """[tiles, V, V, R] -> [H, W, R]: every tile's corner cut at the map's edge."""
    V = T - K + 1
    out = np.zeros((H, W, tiles_out.shape[-1]), tiles_out.dtype)
    for t, (y0, x0) in enumerate(tile_list(H, W, T, K)):
        h, w = min(V, H - y0), min(V, W - x0)
        out[y0:y0 + h, x0:x0 + w] = tiles_out[t, :h, :w]
    return out


def corr_fft(x, w, T=32, dtype=np.float64):
    """x [H, W, C], w [R, K, K, C] -> the "same" correlation [H, W, R] through the whole route in `dtype`."""
    K = w.shape[1]
    H, W, _ = x.shape
    X = forward(windows(np.asarray(x, dtype), T, K))
    Y = gemm(X, spectra(w, T).astype(dtype))
    return scatter(inverse(Y, T, T - K + 1), H, W, T, K)
