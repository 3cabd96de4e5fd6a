"""The frequency-domain correlation (gen6d_amd/csrc/corr_fft.hip) on the GPU, launch by launch and end to end.

  forward   corrfft_fwd_kernel against float64 rfft2 of the windows (interior and edge tiles, two channel groups)
  gemm      corrfft_gemm_kernel against the float64 einsum (two blocks, a partly filled wave)
  inverse   corrfft_inv_kernel against float64 irfft2 (partial tiles on both axes)
            each at 8x the error the fp32 numpy restatement (tests/corr_fft_ref.py) shows on the same data, relative to the range of the
            float64 result: the margin covers the order of the sums.  Measured (profiles/r29_corr_fft.md).
  route     ops.corr_fft_multi against float64 conv2d at 2e-6 of the output range (the bar of the pair kernels), and against
            ops.corr16_multi on the same inputs within 4e-6."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_fft_ref as R
from gen6d_amd import ops
from test_conv16_gpu import _rand, _split

pytestmark = pytest.mark.gpu

T, K, V, BINS = 32, 15, 18, 32 * 17


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def _report(what, got, restated, bar):
    print(f"corr_fft {what}: kernel {got:.3e}, fp32 restatement {restated:.3e}, bar {bar:.3e} (of the float64 result's range)")


def test_forward_kernel():
    """45 x 45: nine tiles, the centre one interior (its window 11 .. 42 lies in the map), the others cut on one or two sides; 19 x 37: windows
    that leave the map on all four sides.  64 channels = two channel groups."""
    g = torch.Generator().manual_seed(3)
    xs = [torch.relu(_rand(g, 1, 45, 45, 64)), torch.relu(_rand(g, 2, 19, 37, 64))]
    plan = ops.corr_fft_plan([(x.shape[0], x.shape[1], x.shape[2]) for x in xs], 64)
    assert plan["tiles"] == 9 + 2 * 6 and plan["bins"] == BINS and plan["V"] == V
    X = torch.full((BINS * plan["tiles"] * 2 * 64,), float("nan"), device="cuda")
    ops.corr_fft_fwd([x.cuda() for x in xs], X)
    got = X.cpu().numpy().reshape(BINS, plan["tiles"], 2, 64)
    win = np.concatenate([R.windows(img.numpy().astype(np.float64), T, K) for x in xs for img in x])            # tiles, T, T, C
    f = np.fft.rfft2(win, axes=(1, 2))                                                                          # tiles, ky, kx, C
    ref = np.stack([f.real, f.imag], 0).transpose(2, 3, 1, 0, 4).reshape(BINS, plan["tiles"], 2, 64)
    restated = _rel(R.forward(win.astype(np.float32)), ref)
    err = _rel(got, ref)
    _report("forward", err, restated, 8 * restated)
    assert np.isfinite(got).all() and err <= 8 * restated


def test_gemm_kernel():
    """M = 150 rows: two blocks of 128, the second with one wave of 22 live rows; K' = 128, asymmetric random operands."""
    g = torch.Generator().manual_seed(4)
    M, Cin = 150, 64
    X = _rand(g, BINS, M, 2 * Cin)
    B = _rand(g, BINS, 2 * Cin, 64)
    Y = torch.full((BINS * M * 64,), float("nan"), device="cuda")
    ops.corr_fft_gemm(X.cuda(), B.cuda(), Y, M, Cin)
    got = Y.cpu().numpy().reshape(BINS, M, 64)
    ref = np.einsum("bmk,bkn->bmn", X.numpy().astype(np.float64), B.numpy().astype(np.float64))
    restated = _rel(R.gemm(X.numpy().reshape(BINS, M, 2, Cin), B.numpy()), ref)
    err = _rel(got, ref)
    _report("gemm", err, restated, 8 * restated)
    assert np.isfinite(got).all() and err <= 8 * restated


def test_inverse_kernel():
    """Spectra of random real tiles (Hermitian, as the products are) on a 19 x 37 map of two images: partial tiles on both axes; pixels the
    map does not have are not written (the outputs sit in a NaN-filled buffer with a guard row behind)."""
    rng = np.random.default_rng(5)
    N, H, W = 2, 19, 37
    nt = N * 2 * 3
    tiles = rng.standard_normal((nt, T, T, 32))
    f = np.fft.rfft2(tiles, axes=(1, 2))                                                                        # tiles, ky, kx, r
    Y64 = np.stack([f.real, f.imag], 0).transpose(2, 3, 1, 0, 4).reshape(BINS, nt, 64)
    Y32 = Y64.astype(np.float32)
    buf = torch.full((N * H * W * 32 + 32 * W,), float("nan"), device="cuda")
    out = buf[:N * H * W * 32].view(N, 1, H, W, 32)
    ops.corr_fft_inv(torch.from_numpy(Y32).cuda(), [out])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[N * H * W * 32:]).all())
    corner = np.fft.irfft2(Y32.astype(np.float64).reshape(T, 17, nt, 2, 32)[:, :, :, 0] + 1j * Y32.astype(np.float64).reshape(T, 17, nt, 2, 32)[:, :, :, 1],
                           s=(T, T), axes=(0, 1)).transpose(2, 0, 1, 3)[:, :V, :V]                              # tiles, V, V, r
    ref = np.stack([R.scatter(corner[n * 6:(n + 1) * 6], H, W, T, K) for n in range(N)])
    rest = R.inverse(Y32, T, V)
    restated = _rel(np.stack([R.scatter(rest[n * 6:(n + 1) * 6], H, W, T, K) for n in range(N)]), ref)
    got = out[:, 0].cpu().numpy()
    err = _rel(got, ref)
    _report("inverse", err, restated, 8 * restated)
    assert np.isfinite(got).all() and err <= 8 * restated


ROUTE = [([(2, 19, 37), (2, 5, 40)], 64), ([(1, 18, 36)], 512)]


@pytest.mark.parametrize("segs,Cin", ROUTE, ids=["19x37+5x40x64", "18x36x512"])
def test_route_against_conv2d_and_corr16(segs, Cin):
    """ReLU'd inputs, filters scaled as in test_lowp_gpu.py; two chunks of one query where the segments hold two."""
    g = torch.Generator().manual_seed(7 + Cin)
    w = _rand(g, 32, K * K, Cin, scale=(1.0 / (K * K * Cin)) ** 0.5 * 3)
    xs = [torch.relu(_rand(g, *s, Cin)) for s in segs]
    spectra = ops.corr_fft_spectra(w.cuda())
    w4 = w.double().reshape(32, K, K, Cin).permute(0, 3, 1, 2)
    refs = [F.conv2d(x.double().permute(0, 3, 1, 2), w4, None, padding=K // 2).permute(0, 2, 3, 1) for x in xs]
    rng_ = max(float(r.abs().max()) for r in refs)
    pair = [torch.empty((s[0], 1, s[1], s[2], 32), device="cuda") for s in segs]
    ops.corr16_multi([_split(x).cuda() for x in xs], ops.corr16_pack(w.cuda(), 3), pair)
    for chunk in (None, 1):
        outs = [torch.full((s[0], 1, s[1], s[2], 32), float("nan"), device="cuda") for s in segs]
        ops.corr_fft_multi([x.cuda() for x in xs], spectra, outs, chunk=chunk)
        err = max(float((o[:, 0].cpu().double() - r).abs().max()) for o, r in zip(outs, refs)) / rng_
        d16 = max(float((o - p).abs().max()) for o, p in zip(outs, pair)) / rng_
        print(f"corr_fft route {segs} x {Cin} chunk {chunk}: {err:.3e} of range against float64 conv2d, {d16:.3e} against corr16_multi")
        assert err <= 2e-6, err
        assert d16 <= 4e-6, d16


def test_refusals():
    x = torch.zeros((1, 20, 20, 48), device="cuda")
    with pytest.raises(RuntimeError, match="Cin % 32"):
        ops.corr_fft_fwd([x], torch.zeros(BINS * 4 * 2 * 48, device="cuda"))
    with pytest.raises(RuntimeError, match="T = 32"):
        ops.corr_fft_fwd([torch.zeros((1, 20, 20, 64), device="cuda")], torch.zeros(64 * 33 * 2 * 64, device="cuda"), T=64)
    with pytest.raises(ValueError, match="channels-last"):
        ops.corr_fft_fwd([x.half()], torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match="smaller"):
        ops.corr_fft_fwd([torch.zeros((1, 20, 20, 64), device="cuda")], torch.zeros(BINS * 4 * 2 * 64 - 1, device="cuda"))
    with pytest.raises(ValueError, match="smaller"):
        ops.corr_fft_inv(torch.zeros(BINS * 4 * 64 - 1, device="cuda"), [torch.zeros((1, 1, 20, 20, 32), device="cuda")])
    big = ops.corr_fft_plan([(16, 88, 116), (16, 60, 80), (16, 44, 60), (16, 32, 40)], 512)
    assert big["tiles"] == 1168 and big["spectrum_bytes"] >= 2 ** 31 and big["max_queries"] == 13 and big["tiles_per_query"] == 73
