"""corrfft_gemm_kernel (gen6d_amd/csrc/corr_fft.hip) at its row and K edges, all 544 bins, against the float64 einsum.

Rows.  A wave owns 64 rows (two 32-row MFMA tiles); up to 128 rows a bin is one block of two waves, beyond that blocks of four waves
(256 rows): M = 1, 31 .. 33, 63 .. 65 (row tile, wave), 127 .. 129 (the two-wave block and the change of kernel), 193 (a wave that starts
right below M), 255 .. 257 (the four-wave block), 292 (the headline's chunk of four queries), 513 (2 B + 1: three blocks, one live row in the
last).  K.  A step is 32 of the K' = 2 Cin values, the ring holds two (small block) or three (large block) steps: Cin = 32, 64, 96, 160
give 2, 4, 6, 10 steps — the shortest accepted, and counts that are and are not multiples of either depth; Cin = 512 (32 steps) once.

Per case: the bar of tests/test_corr_fft_gpu.py (8 x the error of the fp32 numpy restatement tests/corr_fft_ref.py on the same data, of
the float64 result's range); Y sits in front of sentinel rows that must keep their bits; a second call gives the same bits.  One case
runs inside tests/guarded.py arenas (NaN all round, operands at 16 mod 256) with a partial last block."""
import pytest
import torch

import corr_fft_ref as R
from gen6d_amd import ops
from guarded import arena

pytestmark = pytest.mark.gpu

BINS = 32 * 17
MS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 255, 256, 257, 292, 513)
CINS = (32, 64, 96, 160)
SENTINEL_ROWS = 64
_SENT = -12345.678


@pytest.fixture(scope="module")
def pool():
    """One draw for all cases: a case takes the first M rows and the first 2 Cin values of each row (asymmetric, uniform in [-1, 1))."""
    g = torch.Generator().manual_seed(31)
    X = torch.rand((BINS, max(MS), 2 * max(CINS)), generator=g) * 2 - 1
    B = torch.rand((BINS, 2 * max(CINS), 64), generator=g) * 2 - 1
    return X, B


def _errors(got, Xc, Bc, M, Cin):
    """(kernel error, error of the fp32 restatement), both of the range of the float64 einsum; the kernel's result must be finite."""
    ref = torch.einsum("bmk,bkn->bmn", Xc.double(), Bc.double())
    scale = ref.abs().max()
    rest = torch.from_numpy(R.gemm(Xc.numpy().reshape(BINS, M, 2, Cin), Bc.numpy()))
    assert rest.dtype == torch.float32 and bool(torch.isfinite(got).all())
    return float((got.reshape(BINS, M, 64).double() - ref).abs().max() / scale), float((rest.double() - ref).abs().max() / scale)


def _check(Xc, Bc, M, Cin, what):
    """Xc [BINS, M, 2 Cin], Bc [BINS, 2 Cin, 64] on the host; runs the kernel twice and applies every per-case check."""
    n = BINS * M * 64
    Xd, Bd = Xc.reshape(-1).cuda(), Bc.reshape(-1).cuda()
    Y = [torch.full((n + SENTINEL_ROWS * 64,), _SENT, device="cuda") for _ in range(2)]
    for y in Y:
        ops.corr_fft_gemm(Xd, Bd, y, M, Cin)
    torch.cuda.synchronize()
    sent = torch.full((SENTINEL_ROWS * 64,), _SENT).view(torch.int32)
    for y in Y:
        assert torch.equal(y[n:].cpu().view(torch.int32), sent), f"{what}: rows behind Y were written"
    assert torch.equal(Y[0][:n].view(torch.int32), Y[1][:n].view(torch.int32)), f"{what}: two calls differ"
    err, restated = _errors(Y[0][:n].cpu(), Xc, Bc, M, Cin)
    print(f"corr_fft gemm {what}: kernel {err:.3e}, fp32 restatement {restated:.3e}, bar {8 * restated:.3e} (of the float64 result's range)")
    assert err <= 8 * restated, (what, err, restated)


@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("M", MS)
def test_gemm_edges(pool, M, Cin):
    X, B = pool
    _check(X[:, :M, :2 * Cin].contiguous(), B[:, :2 * Cin].contiguous(), M, Cin, f"M={M} Cin={Cin}")


def test_gemm_cin512():
    """The headline's K' = 1024 (32 steps through the ring) at M = 65: a second wave with one live row."""
    g = torch.Generator().manual_seed(32)
    M, Cin = 65, 512
    _check(torch.rand((BINS, M, 2 * Cin), generator=g) * 2 - 1, torch.rand((BINS, 2 * Cin, 64), generator=g) * 2 - 1, M, Cin, "M=65 Cin=512")


def test_gemm_in_guarded_arenas(pool):
    """M = 300, Cin = 96: a full block of 256 rows and a last block of 44 (one wave with rows, three without, all of which still request
    row M - 1 and their share of B').  X, B' and Y each in an arena of their own: NaN in front, behind, and in every element of Y."""
    M, Cin = 300, 96
    Xp, Bp = pool
    Xc, Bc = Xp[:, :M, :2 * Cin].contiguous(), Bp[:, :2 * Cin].contiguous()
    ax = arena((Xc.numel(),), torch.float32, device="cuda")
    ab = arena((Bc.numel(),), torch.float32, device="cuda")
    ay = arena((BINS * M * 64,), torch.float32, device="cuda")
    ax.set(Xc.reshape(-1)); ab.set(Bc.reshape(-1))
    assert ax.view.data_ptr() % 256 == 16 and ab.view.data_ptr() % 256 == 16 and ay.view.data_ptr() % 256 == 16
    ops.corr_fft_gemm(ax.view, ab.view, ay.view, M, Cin)
    torch.cuda.synchronize()
    assert ax.untouched() and ab.untouched(), "an input arena was written"
    assert ay.untouched(), f"stores outside Y: {ay.touched()[:8]}"
    assert ay.unwritten() == 0
    err, restated = _errors(ay.view.cpu(), Xc, Bc, M, Cin)
    print(f"corr_fft gemm guarded M={M} Cin={Cin}: kernel {err:.3e}, fp32 restatement {restated:.3e}, bar {8 * restated:.3e}")
    assert err <= 8 * restated, (err, restated)
