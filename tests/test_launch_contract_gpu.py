"""The accept side of the argument checks that tests/test_launch_contract_cpu.py brought into the launchers: for every new check the
nearest call that must still be ACCEPTED, on real operands, with its result held to tests/ref_ops.py in float64 under the bar and metric of
that entry point's existing test (tests/test_glue_edges_gpu.py::_check).  Tiny shapes; no violating call is issued here.

Boundary values that an existing GPU test already runs are not repeated (profiles/r32_launch_contract.md names the test for each):
vps_norm with c_off + 3 == ld, affine_act_add with ld == C on all three operands, the conv / conv16 / corr16 / corr_fft shapes.  The reach
checks (products that leave an int) have their nearest accepted call at 2^30 elements: that side is decided on the host from integers
alone and stays in the CPU table."""
import pytest
import torch

import ref_ops
from parity_log import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from gen6d_amd import lib, ops as _ops
    lib.load()
    assert torch.cuda.is_available()
    return _ops


_WORST = {}


@pytest.fixture(autouse=True)
def _log_worst(request):
    _WORST.clear()
    yield
    for (entry, tol), err in _WORST.items():
        record(request.node.name, entry, err, tol)


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _d(t):
    return t.detach().cpu().double() if t is not None else None


def _check(entry, got, want, tol, what=""):
    """tests/test_glue_edges_gpu.py::_check: largest absolute error over the largest reference magnitude."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
    _WORST[(entry, tol)] = max(_WORST.get((entry, tol), 0.0), err)
    print(f"{entry} {what}: rel-to-max error {err:.3e} (bar {tol})")
    assert err <= tol, f"{entry} {what}: rel-to-max error {err:.3e} > {tol}"


@pytest.mark.parametrize("Cc", [7, 16])
def test_layernorm_dense_rows(ops, Cc):
    """ld_in == C and ld_out == C (the new checks refuse ld < C); rows offset by +100 as in test_layernorm_edges."""
    g = torch.Generator().manual_seed(192)
    n = 5
    x, gam, bet = _rand(g, n, Cc) + 100.0, 0.5 + torch.rand(Cc, generator=g), _rand(g, Cc)
    ref = torch.empty((n, Cc), dtype=torch.float64)
    ref_ops.layernorm(_d(x), _d(gam), _d(bet), ref)
    xg, out = x.cuda(), torch.empty((n, Cc), device="cuda")
    assert xg.stride(0) == Cc and out.stride(0) == Cc
    ops.layernorm(xg, gam.cuda(), bet.cuda(), out)
    _check("layernorm", out, ref, 1e-5, f"C {Cc} ld == C")


@pytest.mark.parametrize("an", [1, 5])
def test_max_an_add_dense_rows(ops, an):
    """ld_in == C and ld_out == C, C = 12 (not a multiple of the block), a batch of 2."""
    g = torch.Generator().manual_seed(191)
    rfn, Cc, B = 3, 12, 2
    x, emb = _rand(g, B * rfn * an, Cc), _rand(g, rfn, Cc)
    out = torch.empty((B * rfn, Cc), device="cuda")
    ref = torch.empty((B * rfn, Cc), dtype=torch.float64)
    ops.max_an_add(x.cuda(), rfn, an, emb.cuda(), out, batch=B)
    ref_ops.max_an_add(_d(x), rfn, an, _d(emb), ref, batch=B)
    _check("max_an_add", out, ref, 1e-6, f"an {an} ld == C")


@pytest.mark.parametrize("hs,ws", [(3, 5), (20, 13)])
def test_detector_decode_densest_strides(ops, hs, ws):
    """ld_s == 1, ld_o == 2, ld_c == 1: three dense maps of their own (the new checks refuse anything below); a batch of 2, the maximum
    in the last cell of query 0 and in the first of query 1."""
    g = torch.Generator().manual_seed(182)
    B, P = 2, hs * ws
    sc, off, scl = _rand(g, B * P, 1), _rand(g, B * P, 2), _rand(g, B * P, 1)
    sc[P - 1, 0] = 5.0
    sc[P, 0] = 5.0
    scg, offg, sclg = sc.cuda(), off.cuda(), scl.cuda()
    assert (scg.stride(0), offg.stride(0), sclg.stride(0)) == (1, 2, 1)
    res = ops.detector_decode(scg, offg, sclg, hs, ws, 8, batch=B)
    ref = ref_ops.detector_decode(_d(sc), _d(off), _d(scl), hs, ws, 8, batch=B)
    assert res[:, 3:].cpu().tolist() == [[float(ws - 1), float(hs - 1)], [0.0, 0.0]], "detection cell"
    _check("detector_decode", res, ref, 1e-6, f"{hs}x{ws} dense")


@pytest.mark.parametrize("pool", [0, 1, 2])
def test_affine_act_pool_dense_rows(ops, pool):
    """ld_in == C and ld_out == C with one table (affine_per_n == 0, the value next to the refused -1); pool 2 is the full-window mean
    whose H * W the launcher now bounds."""
    g = torch.Generator().manual_seed(150 + pool)
    N, H, W, C = 2, 4, 6, 8
    x = _rand(g, N, 1, H, W, C)
    sc, sh = 0.5 + torch.rand((1, C), generator=g), _rand(g, 1, C)
    shape = {0: (N, 1, H, W, C), 1: (N, 1, H // 2, W // 2, C), 2: (N, 1, 1, 1, C)}[pool]
    out, ref = torch.empty(shape, device="cuda"), torch.empty(shape, dtype=torch.float64)
    ops.affine_act_pool(x.cuda(), out, sc.cuda(), sh.cuda(), per_n=False, relu=True, pool=pool)
    ref_ops.affine_act_pool(_d(x), ref, _d(sc), _d(sh), per_n=False, relu=True, pool=pool)
    _check("affine_act_pool", out, ref, 1e-6, f"pool {pool} ld == C")


@pytest.mark.parametrize("factor", [1, 3])
def test_upsample_bilinear_dense_rows(ops, factor):
    """ld_in == C and ld_out == C, one table; factor 1 (the smallest accepted) and 3."""
    g = torch.Generator().manual_seed(160 + factor)
    N, H, W, C = 2, 3, 5, 8
    x = _rand(g, N, 1, H, W, C)
    sc, sh = 0.5 + torch.rand((1, C), generator=g), _rand(g, 1, C)
    out = torch.empty((N, 1, H * factor, W * factor, C), device="cuda")
    ref = torch.empty((N, 1, H * factor, W * factor, C), dtype=torch.float64)
    ops.upsample_bilinear(x.cuda(), out, factor, sc.cuda(), sh.cuda(), per_n=False)
    ref_ops.upsample_bilinear(_d(x), ref, factor, _d(sc), _d(sh), per_n=False)
    _check("upsample_bilinear", out, ref, 1e-6, f"x{factor} ld == C")


def test_affine_act_add_dense_residual(ops):
    """ld_in == ld_res == ld_out == C with a residual and one table: the exact fit of all three strides the launcher now checks."""
    g = torch.Generator().manual_seed(193)
    n, Cc = 6, 12
    x, res = _rand(g, n, Cc), _rand(g, n, Cc)
    sc, sh = 0.5 + torch.rand((1, Cc), generator=g), _rand(g, 1, Cc)
    o, ro = torch.empty((n, Cc), device="cuda"), torch.empty((n, Cc), dtype=torch.float64)
    ops.affine_act_add(x.cuda(), o, sc.cuda(), sh.cuda(), relu=True, residual=res.cuda())
    ref_ops.affine_act_add(_d(x), ro, _d(sc), _d(sh), relu=True, residual=_d(res))
    _check("affine_act_add", o, ro, 1e-6, "ld == C, residual")


@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_gemv_every_activation(ops, act):
    """act 0, 1 and 2, the whole documented range (3 and -1 are refused now), through BOTH entry points that got the check:
    ops.linear_gemv calls g6d_linear_gemv_batch (B = 9: its row-per-block kernel twice); g6d_linear_gemv itself is called through the
    binding with B = 8, its documented maximum."""
    from gen6d_amd import lib
    g = torch.Generator().manual_seed(196)
    B, K, O = 9, 36, 5
    x, W, b = _rand(g, B, K), _rand(g, O, K, scale=K ** -0.5), _rand(g, O, scale=0.1)
    ref = ref_ops.linear_gemv(_d(x), _d(W), _d(b), act)
    xg, Wg, bg = x.cuda(), W.cuda(), b.cuda()
    out = ops.linear_gemv(xg, Wg, bg, act)
    _check("linear_gemv_batch", out, ref, 1e-5, f"act {act}")
    out8 = torch.empty((8, O), device="cuda")
    lib.check(lib.load().g6d_linear_gemv(ops._ptr(xg), 8, K, ops._ptr(Wg), ops._ptr(bg), O, act, ops._ptr(out8), ops._stream()), "g6d_linear_gemv")
    _check("linear_gemv", out8, ref[:8], 1e-5, f"act {act}, B = 8")
