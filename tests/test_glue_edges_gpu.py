"""The glue kernels (elementwise.hip, selector.hip, detector.hip, refiner_volume.hip, warp.hip, the chain kernels of pose_chain.hip)
away from the product's single square, aligned shape: every entry point against tests/ref_ops.py evaluated in float64 on the CPU at
non-square maps, channel counts off the tiles, ragged groups, strided views and the sizes around each kernel's internal thresholds.

The bars are those of the existing test of the same entry point (tests/test_kernels_gpu.py, tests/test_chain_gpu.py), with the same
metric: largest error relative to the reference's largest magnitude.  Where a check depends on a property of the INPUT (a clip that
binds, a well-conditioned score maximum, a reference that float32 reproduces), that property is asserted on the CPU first."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_ops
from parity_log import record

pytestmark = pytest.mark.gpu

nrm = torch.nn.functional.normalize


@pytest.fixture(scope="module")
def ops():
    from gen6d_amd import lib, ops as _ops
    lib.load()                      # fails loudly if the HIP library is missing
    assert torch.cuda.is_available()
    return _ops


_WORST = {}


@pytest.fixture(autouse=True)
def _log_worst(request):
    """Worst error / bar of every entry point a test touched goes to the parity log (also when the test fails)."""
    _WORST.clear()
    yield
    for (entry, tol), err in _WORST.items():
        record(request.node.name, entry, err, tol)


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _d(t):
    return t.detach().cpu().double() if t is not None else None


def _err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def _check(entry, got, want, tol, what=""):
    """The metric of tests/test_kernels_gpu.py::_check; the figure is printed and kept for the parity log before it is judged."""
    err = _err(got, want)
    _WORST[(entry, tol)] = max(_WORST.get((entry, tol), 0.0), err)
    print(f"{entry} {what}: rel-to-max error {err:.3e} (bar {tol})")
    assert err <= tol, f"{entry} {what}: rel-to-max error {err:.3e} > {tol}"


# ------------------------------------------------------------------------------------------------ affine / pool / up-sampling
def _tables(g, N, C, per_n):
    groups = (N + int(per_n) - 1) // int(per_n) if per_n else 1
    return 0.5 + torch.rand((groups, C), generator=g), _rand(g, groups, C)


@pytest.mark.parametrize("per_n", [False, True, 2])
@pytest.mark.parametrize("N,H,W,C,pool", [(5, 6, 10, 20, 0), (5, 6, 10, 20, 1), (5, 6, 10, 20, 2), (2, 2, 2, 4, 1), (3, 1, 7, 8, 0), (3, 1, 7, 8, 2)])
def test_affine_act_pool_edges(ops, N, H, W, C, pool, per_n):
    """Non-square maps, C below one wave's 16-byte pieces, H = 1, ragged table groups (per_n = 2 on 5 images: 3 tables, the last serves
    one image); input a channel slice at offset 8 of an ld = C + 16 buffer, output a slice of an ld = C + 8 buffer."""
    g = torch.Generator().manual_seed(50 + N + pool)
    xbuf = _rand(g, N, 1, H, W, C + 16)
    sc, sh = _tables(g, N, C, per_n)
    shape = {0: (N, 1, H, W, C), 1: (N, 1, H // 2, W // 2, C), 2: (N, 1, 1, 1, C)}[pool]
    xg = xbuf.cuda()
    xv = xg[..., 8:8 + C]
    obuf = torch.full(shape[:-1] + (C + 8,), -777.0, device="cuda")
    out = obuf[..., 4:4 + C]
    ref = torch.empty(shape, dtype=torch.float64)
    for relu in (True, False):
        ops.affine_act_pool(xv, out, sc.cuda(), sh.cuda(), per_n=per_n, relu=relu, pool=pool)
        ref_ops.affine_act_pool(_d(xbuf[..., 8:8 + C]), ref, _d(sc), _d(sh), per_n=per_n, relu=relu, pool=pool)
        _check("affine_act_pool", out, ref, 1e-6, f"pool {pool} per_n {per_n} relu {relu}")
    assert (obuf[..., :4] == -777.0).all() and (obuf[..., 4 + C:] == -777.0).all(), "wrote outside the channel slice"
    out2 = torch.empty((N, 1, H, W, C), device="cuda")                 # identity affine: the input itself, bit for bit
    ops.affine_act_pool(xv, out2)
    assert torch.equal(out2.cpu(), xbuf[..., 8:8 + C])


@pytest.mark.parametrize("mode", ["plain", "one-table", "per_n2"])
@pytest.mark.parametrize("N,H,W,C,factor", [(3, 5, 9, 12, 1), (3, 5, 9, 12, 2), (3, 5, 9, 12, 3), (3, 5, 9, 12, 4),
                                            (2, 1, 6, 8, 2), (2, 1, 6, 8, 3), (2, 6, 1, 8, 2), (2, 6, 1, 8, 3)])
def test_upsample_bilinear_edges(ops, N, H, W, C, factor, mode):
    g = torch.Generator().manual_seed(60 + H + factor)
    xbuf = _rand(g, N, 1, H, W, C + 4)
    per_n = 2 if mode == "per_n2" else False
    sc, sh = _tables(g, N, C, per_n) if mode != "plain" else (None, None)
    xg = xbuf.cuda()
    xv = xg[..., :C]
    obuf = torch.zeros((N, 1, H * factor, W * factor, C + 16), device="cuda")
    out = obuf[..., 8:8 + C]
    dv = lambda t: t.cuda() if t is not None else None
    ops.upsample_bilinear(xv, out, factor, dv(sc), dv(sh), per_n=per_n)
    ref = torch.empty((N, 1, H * factor, W * factor, C), dtype=torch.float64)
    ref_ops.upsample_bilinear(_d(xbuf[..., :C]), ref, factor, _d(sc), _d(sh), per_n=per_n)
    _check("upsample_bilinear", out, ref, 1e-6, f"{H}x{W} x{factor} {mode}")
    assert (obuf[..., :8] == 0).all() and (obuf[..., 8 + C:] == 0).all(), "wrote outside the channel slice"
    if factor == 1:                                                     # no interpolation: the affine alone, bit for bit
        alone = torch.empty((N, 1, H, W, C), device="cuda")
        ops.affine_act_pool(xv, alone, dv(sc), dv(sh), per_n=per_n, relu=False, pool=0)
        assert torch.equal(out, alone)


# ------------------------------------------------------------------------------------------------ layout change, L2 norm, statistics
@pytest.mark.parametrize("N,Cc,H,W,ld,l2", [(2, 100, 3, 5, 104, False), (2, 100, 3, 5, 104, True), (1, 7, 5, 13, 7, False)])
def test_nchw_to_nhwc_edges(ops, N, Cc, H, W, ld, l2):
    """C and HW both off the 64 x 64 tile (HW = 65 crosses one), ld_out > C."""
    g = torch.Generator().manual_seed(70)
    x = _rand(g, N, Cc, H, W)
    obuf = torch.full((N, 1, H, W, ld), -777.0, device="cuda")
    out = obuf[..., :Cc]
    ops.nchw_to_nhwc(x.cuda(), out, l2)
    ref = torch.empty((N, 1, H, W, Cc), dtype=torch.float64)
    ref_ops.nchw_to_nhwc(_d(x), ref, l2)
    _check("nchw_to_nhwc", out, ref, 1e-6, f"C {Cc} HW {H * W} ld {ld} l2norm {l2}")
    assert (obuf[..., Cc:] == -777.0).all()


def test_l2norm_rows_edges(ops):
    g = torch.Generator().manual_seed(71)
    x = _rand(g, 5, 7)                                                   # rows of 7 floats: the scalar path
    got = ops.l2norm_rows(x.cuda())
    _check("l2norm_rows", got, ref_ops.l2norm_rows(_d(x)), 1e-6, "[5][7]")
    y = _rand(g, 6, 20)
    y[3] = 0.0                                                           # an all-zero row stays zero (eps 1e-12), nothing turns non-finite
    got = ops.l2norm_rows(y.cuda())
    assert torch.isfinite(got).all() and (got[3] == 0).all()
    _check("l2norm_rows", got, ref_ops.l2norm_rows(_d(y)), 1e-6, "[6][20] with a zero row")


@pytest.mark.parametrize("n", [1, 257])
def test_stats_finalize_edges(ops, n):
    g = torch.Generator().manual_seed(72)
    count, eps = 100.0, 1e-5
    st = torch.rand((1, n, 2), generator=g, dtype=torch.float64)
    st[..., 0] = (st[..., 0] - 0.5) * 200
    st[..., 1] = st[..., 0] ** 2 / 100 + st[..., 1] * 50 + 1
    # channel n - 1: E[x^2] - mean^2 a little below zero in float64 (cancellation): the variance is clamped, scale = 1 / sqrt(eps)
    st[0, n - 1, 0] = 300.0
    st[0, n - 1, 1] = 900.0 * (1 - 1e-12)
    var = st[0, n - 1, 1] / count - (st[0, n - 1, 0] / count) ** 2
    assert -1e-10 < var.item() < 0.0
    sc, sh = ops.stats_finalize(st.cuda(), count, eps)
    rsc, rsh = ref_ops.stats_finalize(st, count, eps)
    _check("stats_finalize", sc, rsc, 1e-6, f"scale n {n}"); _check("stats_finalize", sh, rsh, 1e-6, f"shift n {n}")
    assert abs(sc[0, n - 1].item() * eps ** 0.5 - 1.0) <= 1e-6


# ------------------------------------------------------------------------------------------------ selector similarity
def _selector_case(seed, hws, D, qn, C, dg_mult=1):
    """The shard's D hypotheses are the first of Dg = dg_mult * D global ones.  Queries as in tests/test_kernels_gpu.py
    (normalize(rand + 0.3)); the references carry the same offset, so that every score row has a clearly positive maximum also on
    the 1- and 4-position levels (input condition of the vps check, asserted by the caller)."""
    g = torch.Generator().manual_seed(seed)
    refs_g = [nrm(_rand(g, dg_mult * D, hw, C) + 0.3, dim=2) for hw in hws]
    ques = [nrm(_rand(g, qn, hw, C) + 0.3, dim=2) for hw in hws]
    return refs_g, [r[:D].contiguous() for r in refs_g], ques


def _selector_truth(refs_g, refs, ques):
    """float64: score maps / vps per (level, query) from the shard, product statistics from the materialised global product."""
    out = []
    for rg, r, q in zip(refs_g, refs, ques):
        per_q = []
        for i in range(q.shape[0]):
            smap, vps = ref_ops.selector_scan(_d(q[i]), _d(r))
            prod = _d(rg) * _d(q[i])[None]
            mean, var = prod.mean((0, 1)), prod.var((0, 1), unbiased=False)
            per_q.append((smap, vps, 1 / torch.sqrt(var + 1e-5), -mean / torch.sqrt(var + 1e-5)))
        out.append(per_q)
    return out


def _score_condition(truth):
    return min(p[0].max(1)[0].min().item() for lev in truth for p in lev)


HW_A, HW_B = [25, 9, 1], [100, 36, 4]
SELECTOR_CASES = [
    # hws, D, qn, C, Dg / D, knob sel_rowq (None: the product rule — query rows in registers for batches at C = 512)
    (HW_A, 1, 1, 512, 1, None), (HW_A, 5, 3, 512, 3, None), (HW_A, 13, 5, 512, 1, None), (HW_A, 13, 8, 512, 1, None),
    (HW_B, 1, 8, 512, 1, None), (HW_B, 5, 1, 512, 1, None), (HW_B, 13, 3, 512, 1, None), (HW_B, 5, 5, 512, 3, None),
    (HW_A, 5, 1, 512, 1, 0), (HW_B, 13, 3, 512, 1, 0), (HW_B, 13, 1, 512, 3, 1), (HW_A, 5, 3, 512, 1, 1),
    (HW_A, 5, 3, 64, 1, None), (HW_B, 13, 3, 64, 3, None),            # C != 512: the non-ROWQ batch path, lanes >= 16 idle
]
SELECTOR_SEEDS = {(25, 5, 3, 64): 604}                                 # (seed 602 of the rule below gives a score maximum of 0.035 on the one-position level)


@pytest.mark.parametrize("hws,D,qn,C,dgm,rowq", SELECTOR_CASES,
                         ids=[f"hw{c[0][0]}_D{c[1]}_q{c[2]}_C{c[3]}_dg{c[4]}_rowq{c[5]}" for c in SELECTOR_CASES])
def test_selector_levels_edges(ops, hws, D, qn, C, dgm, rowq, knob):
    if rowq is not None:
        knob("sel_rowq", rowq)
    refs_g, refs, ques = _selector_case(SELECTOR_SEEDS.get((hws[0], D, qn, C), 500 + 7 * D + qn + C), hws, D, qn, C, dgm)
    truth = _selector_truth(refs_g, refs, ques)
    cond = _score_condition(truth)
    print(f"input condition: min over (level, query, hypothesis) of max_hw S = {cond:.4f}")
    assert cond >= 0.05, "score maxima too small for a well-conditioned S / max S: pick another seed"
    Dg = dgm * D
    rd = [r.cuda() for r in refs]
    sums = [ops.selector_ref_sums(r.cuda()) for r in refs_g]             # statistics over the Dg global hypotheses
    for l, rg in enumerate(refs_g):
        rr1, rr2 = ref_ops.selector_ref_sums(_d(rg))
        _check("selector_ref_sums", sums[l][0], rr1, 1e-12, f"r1 level {l}"); _check("selector_ref_sums", sums[l][1], rr2, 1e-12, f"r2 level {l}")
    qd = [q.cuda() for q in ques]
    if qn == 1:                                                          # a 2-D query: results without the query axis
        vps, sc, sh, maps = ops.selector_levels([q[0] for q in qd], rd, sums, Dg, want_maps=True)
        vps, sc, sh, maps = vps[None], sc[None], sh[None], [m[None] for m in maps]
    else:
        vps, sc, sh, maps = ops.selector_levels(qd, rd, sums, Dg, want_maps=True)
    assert vps.shape == (qn, 3, D) and sc.shape == (qn, 3, C) and [tuple(m.shape) for m in maps] == [(qn, D, hw) for hw in hws]
    for q in range(qn):
        for l in range(3):
            smap, rvps, rsc, rsh = truth[l][q]
            _check("selector_levels", maps[l][q], smap, 2e-6, f"score map q{q} l{l}")
            _check("selector_levels", vps[q, l], rvps, 1e-5, f"vps q{q} l{l}")
            _check("selector_levels", sc[q, l], rsc, 1e-5, f"scale q{q} l{l}")
            _check("selector_levels", sh[q, l], rsh, 1e-5, f"shift q{q} l{l}")
        if qn > 1:                                                       # every query of a batch against its own single-query launch
            v1, sc1, sh1, m1 = ops.selector_levels([t[q].contiguous() for t in qd], rd, sums, Dg, want_maps=True)
            _check("selector_levels", vps[q], v1, 2e-6, "vps vs single"); _check("selector_levels", sc[q], sc1, 1e-6, "scale vs single")
            _check("selector_levels", sh[q], sh1, 1e-6, "shift vs single")
            for l in range(3):
                _check("selector_levels", maps[l][q], m1[l], 2e-6, "score map vs single")
    # the single-level entry points at the same shapes (first query)
    for l in range(3):
        smap, rvps, rsc, rsh = truth[l][0]
        q0 = qd[l][0].contiguous()
        sm1, vp1 = ops.selector_scan(q0, rd[l])
        _check("selector_scan", sm1, smap, 2e-6, f"score map l{l}"); _check("selector_scan", vp1, rvps, 1e-5, f"vps l{l}")
        s1, h1 = ops.selector_prod_affine(q0, sums[l][0], sums[l][1], Dg)
        _check("selector_prod_affine", s1[0], rsc, 1e-5, f"scale l{l}"); _check("selector_prod_affine", h1[0], rsh, 1e-5, f"shift l{l}")


@pytest.mark.parametrize("HW", [1, 9, 25, 100])
def test_selector_prod_affine_narrow(ops, HW):
    """C = 20: less than one 64-channel block, not a multiple of 16."""
    refs_g, refs, ques = _selector_case(540 + HW, [HW], 5, 1, 20, 3)
    _, _, rsc, rsh = _selector_truth(refs_g, refs, ques)[0][0]
    r1, r2 = ops.selector_ref_sums(refs_g[0].cuda())
    sc, sh = ops.selector_prod_affine(ques[0][0].cuda(), r1, r2, 15)
    _check("selector_prod_affine", sc[0], rsc, 1e-5, f"scale HW {HW} C 20"); _check("selector_prod_affine", sh[0], rsh, 1e-5, f"shift HW {HW} C 20")


# ------------------------------------------------------------------------------------------------ detector glue
DET_STATS = [[36.264317, 13.151907], [13910.291, 5345.965], [829.70807, 387.98788]]


@pytest.mark.parametrize("sigmas", [3, 30])
@pytest.mark.parametrize("rfn", [1, 5])
@pytest.mark.parametrize("hc,wc,hs,ws", [(8, 12, 5, 9), (4, 4, 16, 12), (12, 20, 12, 20)])
def test_detector_assemble_edges(ops, hc, wc, hs, ws, rfn, sigmas):
    """Down-sampling, 4x up-sampling and the same size, hs != ws, a batch of 2, all four scale slots.  At 30 sigma the clip binds."""
    g = torch.Generator().manual_seed(80 + hs + rfn)
    B, clip = 2, 10.0
    stacked = torch.zeros((B * hs * ws, rfn, 12), device="cuda")
    rstacked = torch.zeros((B * hs * ws, rfn, 12), dtype=torch.float64)
    for si in range(4):                                                  # own maps for every scale slot
        s = [_rand(g, B * (hc >> l) * (wc >> l), rfn, scale=sigmas * DET_STATS[l][1]) + DET_STATS[l][0] for l in range(3)]
        clipped = torch.cat([((t.double() - DET_STATS[l][0]) / DET_STATS[l][1]).abs().flatten() > clip for l, t in enumerate(s)]).double().mean().item()
        print(f"input condition: {100 * clipped:.1f} % of the normalised taps are clipped at {sigmas} sigma")
        assert (0.05 <= clipped <= 0.95) if sigmas == 30 else clipped == 0.0
        ops.detector_assemble(s[0].cuda(), s[1].cuda(), s[2].cuda(), hc, wc, DET_STATS, clip, hs, ws, si, stacked, batch=B)
        ref_ops.detector_assemble(_d(s[0]), _d(s[1]), _d(s[2]), hc, wc, DET_STATS, clip, hs, ws, si, rstacked, batch=B)
    _check("detector_assemble", stacked, rstacked, 1e-5, f"{hc}x{wc} -> {hs}x{ws} rfn {rfn} at {sigmas} sigma")
    assert stacked.abs().max() <= clip + 1e-6


@pytest.mark.parametrize("rfn", [1, 5, 48, 100, 256])
def test_detector_score_mlp_max_edges(ops, rfn):
    """rfn that does not divide 256 (idle threads behind the last whole pixel of a block), P = 53 not a multiple of any 256 / rfn."""
    g = torch.Generator().manual_seed(81)
    P = 53
    stacked = _rand(g, P, rfn, 12, scale=3.0)
    w0, b0, w1, b1 = _rand(g, 64, 12, scale=0.3), _rand(g, 64, scale=0.1), _rand(g, 64, 64, scale=0.2), _rand(g, 64, scale=0.1)
    out = ops.detector_score_mlp_max(stacked.cuda(), w0.cuda(), b0.cuda(), w1.cuda(), b1.cuda())
    ref = ref_ops.detector_score_mlp_max(_d(stacked), _d(w0), _d(b0), _d(w1), _d(b1))
    _check("detector_score_mlp_max", out, ref, 1e-5, f"rfn {rfn}")


@pytest.mark.parametrize("hs,ws", [(3, 5), (5, 9), (20, 13)])
def test_detector_decode_edges(ops, hs, ws):
    """Fewer than 256 and more than 256 cells, hs != ws, a batch of 3 through strided column views: the maximum in the first cell, in
    the last cell, and all scores equal (the first cell wins)."""
    g = torch.Generator().manual_seed(82)
    B, P = 3, hs * ws
    o4 = _rand(g, B * P, 4)
    o4[0, 0] = 5.0
    o4[2 * P - 1, 0] = 5.0
    o4[2 * P:, 0] = 0.25
    og = o4.cuda()
    res = ops.detector_decode(og[:, 0:1], og[:, 2:4], og[:, 1:2], hs, ws, 8, batch=B)
    rres = ref_ops.detector_decode(_d(o4)[:, 0:1], _d(o4)[:, 2:4], _d(o4)[:, 1:2], hs, ws, 8, batch=B)
    assert res.shape == (B, 5)
    assert res[:, 3:].cpu().tolist() == [[0.0, 0.0], [float(ws - 1), float(hs - 1)], [0.0, 0.0]], "detection cell"
    _check("detector_decode", res, rres, 1e-6, f"{hs}x{ws}")


# ------------------------------------------------------------------------------------------------ selector tail
@pytest.mark.parametrize("D,B,ld,c_off", [(1, 1, 516, 512), (40, 2, 3, 0), (300, 2, 516, 512), (300, 1, 3, 0)])
def test_vps_norm_edges(ops, D, B, ld, c_off):
    """D = 1, D > 256 (two trips of the block), c_off = 0 into rows of 3 floats, a constant channel (its output is exactly 0)."""
    g = torch.Generator().manual_seed(90 + D)
    vps = _rand(g, B, 3, D, scale=20) + 30
    vps[B - 1, 1] = 17.25
    feats = torch.full((B * D, ld), -777.0, device="cuda"); rfeats = torch.full((B * D, ld), -777.0, dtype=torch.float64)
    ops.vps_norm(vps.cuda() if B > 1 else vps[0].cuda(), feats, c_off)
    ref_ops.vps_norm(_d(vps) if B > 1 else _d(vps[0]), rfeats, c_off)
    _check("vps_norm", feats[:, c_off:c_off + 3], rfeats[:, c_off:c_off + 3], 1e-5, f"D {D} batch {B} ld {ld}")
    assert (feats[:, :c_off] == -777.0).all() and (feats[:, c_off + 3:] == -777.0).all(), "wrote outside its three columns"
    assert (feats[(B - 1) * D:, c_off + 1] == 0).all(), "constant channel"
    if D == 1:
        assert (feats[:, c_off:c_off + 3] == 0).all()


@pytest.mark.parametrize("an", [1, 7])
def test_max_an_add_edges(ops, an):
    g = torch.Generator().manual_seed(91)
    rfn, Cc, B = 3, 20, 2
    xbuf, emb = _rand(g, B * rfn * an, 32), _rand(g, rfn, Cc)
    obuf = torch.full((B * rfn, 28), -777.0, device="cuda")
    rout = torch.empty((B * rfn, Cc), dtype=torch.float64)
    ops.max_an_add(xbuf.cuda()[:, 4:24], rfn, an, emb.cuda(), obuf[:, 4:24], batch=B)
    ref_ops.max_an_add(_d(xbuf[:, 4:24]), rfn, an, _d(emb), rout, batch=B)
    _check("max_an_add", obuf[:, 4:24], rout, 1e-6, f"an {an}")
    assert (obuf[:, :4] == -777.0).all() and (obuf[:, 24:] == -777.0).all()


@pytest.mark.parametrize("Cc", [7, 100, 512])
def test_layernorm_edges(ops, Cc):
    """C below one wave, C not a multiple of 64; rows offset by +100 (float32 torch on the CPU stays within 2.6e-6 of float64 there);
    strided input and output; in place (include/gen6d_hip.h allows out == in)."""
    g = torch.Generator().manual_seed(92)
    n = 5
    xbuf = _rand(g, n, Cc + 9) + 100.0
    gam, bet = 0.5 + torch.rand(Cc, generator=g), _rand(g, Cc)
    rln = torch.empty((n, Cc), dtype=torch.float64)
    ref_ops.layernorm(_d(xbuf[:, 5:5 + Cc]), _d(gam), _d(bet), rln)
    xg = xbuf.cuda()
    obuf = torch.full((n, Cc + 3), -777.0, device="cuda")
    ops.layernorm(xg[:, 5:5 + Cc], gam.cuda(), bet.cuda(), obuf[:, 2:2 + Cc])
    _check("layernorm", obuf[:, 2:2 + Cc], rln, 1e-5, f"C {Cc} strided")
    assert (obuf[:, :2] == -777.0).all() and (obuf[:, 2 + Cc:] == -777.0).all()
    ops.layernorm(xg[:, 5:5 + Cc], gam.cuda(), bet.cuda(), xg[:, 5:5 + Cc])
    _check("layernorm", xg[:, 5:5 + Cc], rln, 1e-5, f"C {Cc} in place")
    assert torch.equal(xg[:, :5].cpu(), xbuf[:, :5]) and torch.equal(xg[:, 5 + Cc:].cpu(), xbuf[:, 5 + Cc:])


@pytest.mark.parametrize("variant", ["no-scale", "no-residual", "strided-residual", "ragged-groups"])
def test_affine_act_add_edges(ops, variant):
    g = torch.Generator().manual_seed(93)
    n, Cc = 7, 20
    x, resbuf = _rand(g, n, Cc), _rand(g, n, Cc + 12)
    rpg = 3 if variant == "ragged-groups" else 0                         # 7 rows in groups of 3: three tables, the last serves one row
    groups = 3 if rpg else 1
    sc, sh = (None, None) if variant == "no-scale" else (0.5 + torch.rand((groups, Cc), generator=g), _rand(g, groups, Cc))
    res = None if variant == "no-residual" else (resbuf[:, 8:8 + Cc] if variant == "strided-residual" else resbuf[:, :Cc].contiguous())
    dv = lambda t: t.cuda() if t is not None else None
    resg = None if res is None else (resbuf.cuda()[:, 8:8 + Cc] if variant == "strided-residual" else res.cuda())
    o = torch.empty((n, Cc), device="cuda"); ro = torch.empty((n, Cc), dtype=torch.float64)
    ops.affine_act_add(x.cuda(), o, dv(sc), dv(sh), relu=True, residual=resg, rows_per_group=rpg)
    ref_ops.affine_act_add(_d(x), ro, _d(sc), _d(sh), relu=True, residual=_d(res), rows_per_group=rpg)
    _check("affine_act_add", o, ro, 1e-6, variant)


# Operands scaled by ATT_SCALE sharpen the softmax (the logits grow with its square).  ATT_SCALE = 3 is the largest of {2, 3, 4, 6} at
# which float32 ref_ops.attention on the CPU stays under a quarter of the 1e-5 bar against float64 on every case below (measured:
# 1.0e-6 at 2, 2.3e-6 at 3, 5.1e-6 at 4, 8.6e-6 at 6), so the bar still measures the kernel and not the conditioning of the input.
ATT_SCALE = 3.0


@pytest.mark.parametrize("scale", [1.0, ATT_SCALE])
@pytest.mark.parametrize("heads,Cc", [(8, 64), (8, 512), (4, 512), (1, 64)])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_attention_edges(ops, n, heads, Cc, scale):
    """Token counts around the block kernel's limit of 64 (65 and heads of 128 channels take the wave-per-token kernel), a batch of 2,
    q / k / v as column slices of one buffer."""
    g = torch.Generator().manual_seed(94 + n)
    B = 2
    qkv = _rand(g, B * n, 3 * Cc) * scale
    qd = _d(qkv)
    ratt = torch.empty((B * n, Cc), dtype=torch.float64)
    ref_ops.attention(qd[:, :Cc], qd[:, Cc:2 * Cc], qd[:, 2 * Cc:], heads, ratt, batch=B)
    r32 = torch.empty((B * n, Cc))
    ref_ops.attention(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], heads, r32, batch=B)
    noise = _err(r32, ratt)
    print(f"float32 reference vs float64: {noise:.2e} at scale {scale}")
    qg = qkv.cuda()
    obuf = torch.full((B * n, Cc + 8), -777.0, device="cuda")
    ops.attention(qg[:, :Cc], qg[:, Cc:2 * Cc], qg[:, 2 * Cc:], heads, obuf[:, :Cc], batch=B)
    _check("attention", obuf[:, :Cc], ratt, 1e-5, f"n {n} heads {heads} C {Cc} scale {scale}")
    assert (obuf[:, Cc:] == -777.0).all()


# ------------------------------------------------------------------------------------------------ refiner volume
VOLUME_CASES = [
    # rfn, C, fh, fw, h_in, w_in, sn
    (8, 32, 12, 20, 96, 160, 6),        # C <= 4 * rfn: lanes that own no channel still hand their view's footprint on
    (3, 64, 20, 12, 160, 96, 6),        # portrait
    (6, 256, 16, 24, 128, 192, 5),      # two 128-channel trips
    (2, 132, 9, 7, 72, 56, 5),          # a ragged second trip, odd maps
    (1, 64, 12, 20, 96, 160, 5),        # one reference: std 0; sn = 5: 125 voxels leave dead half-waves in the last block
]


def _volume_case(rfn, h_in, w_in):
    from gen6d_amd import synth
    case = synth.refiner_case(rfn=rfn)
    S = torch.diag(torch.tensor([w_in / 128.0, h_in / 128.0, 1.0]))      # the 128 x 128 cameras on an h_in x w_in image
    return S @ case["ref_Ks"][0], case["ref_poses"][0].contiguous(), (S @ case["Ks_in"][0]).contiguous(), case["poses_in"][0].contiguous()


@pytest.mark.parametrize("rfn,Cc,fh,fw,h_in,w_in,sn", VOLUME_CASES)
def test_refiner_volume_edges(ops, rfn, Cc, fh, fw, h_in, w_in, sn):
    from gen6d_amd import synth
    g = torch.Generator().manual_seed(95)
    ref_Ks, ref_poses, K_in, pose_in = _volume_case(rfn, h_in, w_in)
    ref_Ks = ref_Ks.contiguous()
    feats = _rand(g, rfn + 1, fh, fw, Cc)
    projs = torch.cat([ref_Ks @ ref_poses, (K_in @ pose_in)[None]], 0).contiguous()
    rot = pose_in[:, :3].contiguous()
    lin = torch.linspace(-1, 1, sn)
    nv = sn ** 3
    # input condition: a good part of the voxels, not all, project inside the query view (interior and zero-padding taps both matter)
    grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(nv, 3).double() @ _d(rot)
    X = grid @ _d(projs[-1])[:, :3].T + _d(projs[-1])[:, 3]
    u, v = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    inside = ((u >= 0) & (u <= w_in - 1) & (v >= 0) & (v <= h_in - 1)).double().mean().item()
    print(f"input condition: {100 * inside:.1f} % of the voxels project inside the query view")
    assert 0.5 <= inside <= 0.9
    rm = torch.empty((nv, 2 * Cc), dtype=torch.float64); rs = torch.empty((nv, Cc), dtype=torch.float64)
    ref_ops.refiner_volume(_d(feats), _d(projs), _d(rot), _d(lin), h_in, w_in, rm, rs)
    if rfn == 1:
        assert (rs == 0).all()
    fg, lg = feats.cuda(), lin.cuda()
    mean_in = torch.full((nv, 2 * Cc), -777.0, device="cuda"); std = torch.full((nv, Cc), -777.0, device="cuda")
    ops.refiner_volume(fg, projs.cuda(), rot.cuda(), lg, h_in, w_in, mean_in, std)
    _check("refiner_volume", mean_in[:, :Cc], rm[:, :Cc], 2e-4, "mean"); _check("refiner_volume", mean_in[:, Cc:], rm[:, Cc:], 2e-4, "query")
    _check("refiner_volume", std, rs, 2e-4, "std")
    m2 = torch.full_like(mean_in, -777.0); s2 = torch.full_like(std, -777.0)
    ops.refiner_volume_kp(fg, ref_Ks.cuda(), ref_poses.cuda(), K_in.cuda(), pose_in.cuda(), lg, h_in, w_in, m2, s2)
    _check("refiner_volume_kp", m2[:, :Cc], rm[:, :Cc], 2e-4, "mean"); _check("refiner_volume_kp", m2[:, Cc:], rm[:, Cc:], 2e-4, "query")
    _check("refiner_volume_kp", s2, rs, 2e-4, "std")
    # a batch of 3 queries (own views, cameras and input poses) in one launch equals the three single launches
    B = 3
    fb = torch.stack([feats, feats.flip(0), feats * 0.5], 0).contiguous().cuda()
    Kb = torch.stack([ref_Ks] * B, 0).contiguous().cuda()
    Pb = torch.stack([ref_poses, ref_poses.flip(0), ref_poses], 0).contiguous().cuda()
    Kin = torch.stack([K_in] * B, 0).contiguous().cuda()
    pin = torch.stack([pose_in, torch.from_numpy(synth.perturb_pose(pose_in.numpy(), 3.0, 0.02)), pose_in], 0).contiguous().cuda()
    mb = torch.empty((B, nv, 2 * Cc), device="cuda"); sb = torch.empty((B, nv, Cc), device="cuda")
    ops.refiner_volume_kp(fb, Kb, Pb, Kin, pin, lg, h_in, w_in, mb, sb)
    for b in range(B):
        ops.refiner_volume_kp(fb[b].contiguous(), Kb[b].contiguous(), Pb[b].contiguous(), Kin[b].contiguous(), pin[b].contiguous(), lg, h_in, w_in, m2, s2)
        assert torch.equal(mb[b], m2) and torch.equal(sb[b], s2), f"batched volume {b} differs from its single launch"


# ------------------------------------------------------------------------------------------------ warps
def _warp_rule(got, want, what):
    """The rule of tests/test_chain_gpu.py::test_warp_batch_matches_single_warps on grey levels: rounding ties only."""
    d = (got.double() - want.double()).abs()
    print(f"{what}: max {d.max().item():.3f} levels, {100 * (d > 0.5).double().mean().item():.3f} % off by more than 1/2")
    assert d.max() <= 1.001 and (d > 0.5).double().mean() < 0.01, what


def _homographies(rng, n):
    """Destination -> source maps that leave part of the 40 x 72 destination outside the source."""
    hinv = []
    for _ in range(n):
        a, s = rng.uniform(-0.6, 0.6), rng.uniform(0.6, 1.4)
        M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-10, 30)], [s * np.sin(a), s * np.cos(a), rng.uniform(-10, 30)],
                      [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])
        hinv.append(np.linalg.inv(M).reshape(9))
    return torch.from_numpy(np.asarray(hinv, np.float32))


def _images(n, sh, sw, ch, seed):
    from gen6d_amd import synth
    im = torch.from_numpy(synth.synth_images(n, sh, sw, seed))
    return {1: im[..., :1], 3: im, 4: torch.cat([im, im[..., 1:2]], -1)}[ch].contiguous()


@pytest.mark.parametrize("with_single", [True, False])
@pytest.mark.parametrize("sh,sw", [(96, 128), (32, 48)])
@pytest.mark.parametrize("ch", [1, 4])
def test_warp_batch_edges(ops, ch, sh, sw, with_single):
    """Non-square 40 x 72 destination, 1 and 4 channels, a source smaller than the destination, no single image (all idx >= 0)."""
    dh, dw, B = 40, 72, 4
    imgs, que = _images(5, sh, sw, ch, 33), _images(1, sh, sw, ch, 34)[0]
    hinv = _homographies(np.random.RandomState(3 + sh), B)
    idx = torch.tensor([-1, 3, 0, 4] if with_single else [2, 3, 0, 4], dtype=torch.int32)
    single = que if with_single else None
    want = ref_ops.warp_batch(imgs, single, idx, hinv, dh, dw, dtype=torch.float64)
    w32 = ref_ops.warp_batch(imgs, single, idx, hinv, dh, dw)
    differ = ((w32.double() * 255).round() != (want * 255).round()).double().mean().item()
    outside = (want == 0).all(1).double().mean().item()
    print(f"input condition: float32 and float64 references differ on {100 * differ:.3f} % of the grey levels; {100 * outside:.1f} % of the destination "
          "lies outside the source")
    assert differ < 0.005 and 0.02 < outside < 0.9
    got = ops.warp_batch(imgs.cuda(), single.cuda() if with_single else None, idx.cuda(), hinv.cuda(), dh, dw)
    assert got.shape == (B, ch, dh, dw)
    _warp_rule(got.cpu() * 255, want * 255, "warp_batch")
    for b in range(B):                                                   # the one-image entry point on the same maps
        src = que if int(idx[b]) < 0 else imgs[int(idx[b])]
        H = np.linalg.inv(hinv[b].double().numpy().reshape(3, 3))
        one = ops.warp_perspective(src.cuda(), H, dh, dw)
        _warp_rule(one.cpu(), ref_ops.warp_perspective(src, H, dh, dw, dtype=torch.float64), "warp_perspective")


# ------------------------------------------------------------------------------------------------ chain kernels
def _dev(t):
    return t.cuda() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).cuda()


@pytest.mark.parametrize("n_sub,ref_num", [(128, 8), (40, 6), (1, 1)])
def test_chain_kernels_batch_edges(ops, n_sub, ref_num):
    """Three queries with their own detections, logits (one with a tie), intrinsics and input poses in one launch of every chain kernel:
    each equals its own batch = 1 launch bit for bit (the per-query pointer offsets) and the host algebra to the bars of
    tests/test_chain_gpu.py; the largest view table (128) with the largest selection (8), and the smallest (1, 1)."""
    from gen6d_amd import geometry as G, synth
    B = 3
    poses, Ks = synth.fibonacci_cameras(n_sub, radius=3.0, focal=250.0, size=160)
    rng = np.random.RandomState(4)
    center = np.array([0.04, -0.03, 0.02], np.float32)
    det = torch.tensor([[83.5, 61.25, 1.37, 10.0, 7.0], [40.25, 90.5, 0.8, 5.0, 11.0], [120.0, 33.75, 2.1, 15.0, 4.0]])
    h_ref, h_dev = ref_ops.chain_crop_from_detection(det, 128), ops.chain_crop_from_detection(det.cuda(), 128)
    np.testing.assert_allclose(h_dev.cpu().numpy(), h_ref.numpy(), rtol=1e-5, atol=1e-5)
    logits = torch.from_numpy(rng.randn(B, n_sub).astype(np.float32))
    angles = torch.from_numpy((rng.rand(B, n_sub) - 0.5).astype(np.float32))
    if n_sub > 30:
        logits[1, 7] = logits[1, 23] = logits[1].max() + 1                # tie: the first maximum wins
    rp, rk = torch.from_numpy(poses).reshape(-1, 12), torch.from_numpy(Ks).reshape(-1, 9)
    qK = torch.stack([torch.from_numpy(Ks[0] * np.array([[f], [f], [1.0]], np.float32)).reshape(9) for f in (1.2, 0.9, 1.05)], 0)
    p_ref, s_ref = ref_ops.chain_pose_from_selection(det, logits, angles, rp, rk, qK, torch.from_numpy(center))
    p_dev, s_dev = ops.chain_pose_from_selection(det.cuda(), logits.cuda(), angles.cuda(), rp.cuda(), rk.cuda(), qK.cuda(), _dev(center))
    assert torch.equal(s_dev[:, 0].cpu(), s_ref[:, 0]) and (n_sub <= 30 or int(s_dev[1, 0]) == 7)
    np.testing.assert_allclose(p_dev.cpu().numpy(), p_ref.numpy(), atol=2e-5)
    diameter = 1.3
    nscale, noff = 2 / diameter, -(2 / diameter) * center
    sub = np.stack([G.normalize_pose(p.astype(np.float64), nscale, noff) for p in poses]).astype(np.float32)
    norm = torch.from_numpy(np.concatenate([[nscale], noff]).astype(np.float32))
    pick = [9 % n_sub, 21 % n_sub, 3 % n_sub]
    pose_in = torch.stack([torch.from_numpy(synth.perturb_pose(poses[i], r, t)).reshape(12) for i, (r, t) in zip(pick, [(5.0, 0.03), (-4.0, 0.01), (2.5, -0.02)])], 0)
    subt = torch.from_numpy(sub).reshape(-1, 12)
    g_ref, i_ref = ref_ops.chain_refine_prepare(pose_in, qK, norm, 128, 0.05, subt, rk, ref_num)
    g_dev, i_dev = ops.chain_refine_prepare(pose_in.cuda(), qK.cuda(), norm.cuda(), 128, 0.05, subt.cuda(), rk.cuda(), ref_num)
    assert g_dev.shape == (B, 42 + 30 * ref_num) and np.array_equal(i_dev.cpu().numpy(), i_ref.numpy())
    np.testing.assert_allclose(g_dev.cpu().numpy(), g_ref.numpy(), rtol=2e-4, atol=2e-4)
    rot = nrm(torch.from_numpy(rng.randn(B, 4).astype(np.float32)), dim=1)
    off = torch.tensor([[0.03, -0.02], [-0.05, 0.01], [0.0, 0.04]])
    scl = torch.tensor([[0.21], [-0.1], [0.05]])
    u_ref = ref_ops.chain_refine_update(rot, off, scl, g_ref, norm)
    u_dev = ops.chain_refine_update(rot.cuda(), off.cuda(), scl.cuda(), g_ref.cuda(), norm.cuda())
    np.testing.assert_allclose(u_dev.cpu().numpy(), u_ref.numpy(), atol=2e-5)
    for b in range(B):                                                   # every query against its own single launch: bit-equal
        assert torch.equal(ops.chain_crop_from_detection(det[b].cuda(), 128)[0], h_dev[b])
        p1, s1 = ops.chain_pose_from_selection(det[b].cuda(), logits[b].cuda(), angles[b].cuda(), rp.cuda(), rk.cuda(), qK[b].cuda(), _dev(center))
        assert torch.equal(p1, p_dev[b]) and torch.equal(s1, s_dev[b])
        g1, i1 = ops.chain_refine_prepare(pose_in[b].cuda(), qK[b].cuda(), norm.cuda(), 128, 0.05, subt.cuda(), rk.cuda(), ref_num)
        assert torch.equal(g1, g_dev[b]) and torch.equal(i1, i_dev[b])
        u1 = ops.chain_refine_update(rot[b].cuda(), off[b].cuda(), scl[b].cuda(), g_ref[b].cuda(), norm.cuda())
        assert torch.equal(u1, u_dev[b])


# ------------------------------------------------------------------------------------------------ small linear layers
@pytest.mark.parametrize("B,K,O", [(2, 516, 3), (9, 516, 5), (1, 4, 1)])
@pytest.mark.parametrize("mfma", [2, 1, 0], ids=["matrix-cores", "product-rule", "vector-alu"])
def test_linear_gemv_small(ops, B, K, O, mfma, knob):
    """K not a multiple of any slice, O below every row group: the row-per-block kernel under all three values of the knob (9 rows: 8 + 1)."""
    knob("gemv_mfma", mfma)
    g = torch.Generator().manual_seed(96)
    x, W, b = _rand(g, B, K), _rand(g, O, K, scale=K ** -0.5), _rand(g, O, scale=0.1)
    out = ops.linear_gemv(x.cuda(), W.cuda(), b.cuda(), 2)
    _check("linear_gemv", out, ref_ops.linear_gemv(_d(x), _d(W), _d(b), 2), 1e-5, f"{B}x{K}x{O}")


# ------------------------------------------------------------------------------------------------ launcher checks
def _rejected(ops, name, *args):
    """Calls the C entry point with the torch stream appended; the launcher must refuse with G6D_EINVAL before any launch."""
    from gen6d_amd import lib
    with pytest.raises(RuntimeError, match="G6D_EINVAL"):
        lib.check(getattr(lib.load(), name)(*args, ops._stream()), name)


def test_glue_launchers_reject_bad_args(ops):
    p = ops._ptr
    z = torch.zeros(4096, device="cuda")
    ms = (C.c_float * 6)(0, 1, 0, 1, 0, 1)
    for hs, ws in [(0, 4), (4, 0), (-1, 4)]:
        _rejected(ops, "g6d_detector_assemble", p(z), p(z), p(z), 4, 4, 1, ms, 10.0, hs, ws, 0, 12, p(z), 1)
    for H, W in [(0, 4), (4, 0), (4, -2)]:
        _rejected(ops, "g6d_upsample_bilinear", p(z), 4, None, None, 0, 1, H, W, 4, 2, p(z), 4)
    for fh, fw, h_in, w_in in [(0, 4, 32, 32), (4, 0, 32, 32), (4, 4, 0, 32), (4, 4, 32, -1)]:
        _rejected(ops, "g6d_refiner_volume", p(z), p(z), p(z), p(z), 1, fh, fw, 4, h_in, w_in, 2, p(z), p(z))
        _rejected(ops, "g6d_refiner_volume_kp", p(z), p(z), p(z), p(z), p(z), p(z), 1, fh, fw, 4, h_in, w_in, 2, p(z), p(z), 1)
    _rejected(ops, "g6d_refiner_volume", p(z), p(z), p(z), p(z), 1, 4, 4, 0, 32, 32, 2, p(z), p(z))          # C = 0
    _rejected(ops, "g6d_attention", p(z), p(z), p(z), 12, 2, 16, 2, p(z), 16, 1)                             # ld < C
    _rejected(ops, "g6d_attention", p(z), p(z), p(z), 16, 2, 16, 2, p(z), 12, 1)                             # ld_out < C
    # checks the launchers had before
    x = torch.zeros((1, 1, 3, 4, 4), device="cuda")
    with pytest.raises(RuntimeError, match="G6D_EINVAL"):                # 2x2 pooling of an odd height
        ops.affine_act_pool(x, torch.zeros((1, 1, 1, 2, 4), device="cuda"), pool=1)
    w0, b0, w1 = torch.zeros((64, 12), device="cuda"), torch.zeros(64, device="cuda"), torch.zeros((64, 64), device="cuda")
    with pytest.raises(RuntimeError, match="G6D_EINVAL"):                # more references than a block has threads
        ops.detector_score_mlp_max(torch.zeros((2, 257, 12), device="cuda"), w0, b0, w1, b0)
    pose, K, norm = torch.zeros(12, device="cuda"), torch.zeros(9, device="cuda"), torch.ones(4, device="cuda")
    with pytest.raises(RuntimeError, match="G6D_EINVAL"):                # n_sub > 128
        ops.chain_refine_prepare(pose, K, norm, 128, 0.05, torch.zeros((129, 12), device="cuda"), torch.zeros((129, 9), device="cuda"), 6)
    with pytest.raises(RuntimeError, match="G6D_EINVAL"):                # ref_num > n_sub
        ops.chain_refine_prepare(pose, K, norm, 128, 0.05, torch.zeros((3, 12), device="cuda"), torch.zeros((3, 9), device="cuda"), 4)
