"""Range control of the fp32 path's fp16 hi / lo pair maps (G6dRange16, ops.RangeTable / PairMap, ParamBank.range_guarded):

  producers   the five pair producers write split16(v * 2^-e) and record max |v| (integer max of the bits: NaN / inf recorded)
  consumers   conv16_direct_multi / corr16_multi read pair maps of any exponent at the 2e-6-of-range bar of the unscaled pairs
  legacy      the entry points without a range and the _ex entry points with exponents 0 give identical bits
  detector    the 480x640x32 headline with exact power-of-two gains on two trunk layers: one recompute on the fp32 routes, then the
              updated exponents keep the next call on the pair kernels, both calls at the headline's bars; a reload drops the state
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gen6d_amd import ops, synth
from test_conv16_gpu import CASES, MODE, _join, _rand, _split
from test_networks_gpu import _net, _vs_golden
from test_split16_range_cpu import reparam

pytestmark = pytest.mark.gpu

NONFINITE = 0x7F800000


def _rec(table, slot):
    return int(table.rec[slot].item()) & 0xFFFFFFFF


def _bits_max(t):
    return int(t.float().abs().contiguous().view(torch.int32).max().item()) & 0xFFFFFFFF


def _gains(g, C):
    return torch.exp(torch.empty(C).uniform_(np.log(1e-4), np.log(1e3), generator=g))


def _check_pairs(p, v, e):
    """(hi + lo) 2^e against the fp32 values v for |v| >= 2^-4 max|v|: 2^-22 relative, plus the fp16 subnormal grid of the lo plane."""
    v = v.double().cpu()
    got = _join(p.cpu()) * 2.0 ** e
    a = float(v.abs().max())
    m = v.abs() >= a / 16
    err = (got - v).abs()
    assert bool(torch.isfinite(got).all())
    assert bool((err[m] <= 2.0 ** -22 * v.abs()[m] + 2.0 ** (e - 25)).all()), float((err[m] / v.abs()[m]).max())


def _table(e):
    t = ops.RangeTable(torch.device("cuda"))
    s = t.slot("x")
    t.set_exponents({"x": e})
    return t, s


@pytest.mark.parametrize("mag", [2.0 ** 20, 2.0 ** -12])
def test_producer_conv16(mag):
    g = torch.Generator().manual_seed(5)
    x = _rand(g, 2, 16, 24, 64)
    w = _rand(g, 128, 9, 64, scale=0.1) * (_gains(g, 128) * (mag / 1e3))[:, None, None]     # largest output ~ mag
    b = torch.zeros(128)
    filt = ops.conv16_pack(w.cuda(), 3)
    xin = _split(x).cuda()
    full, pool = ops.conv16_direct_multi([xin], filt, b.cuda(), relu=True, full=torch.float32, pool=torch.float32)
    e = ops.pair_exponent(float(full[0].abs().max()))
    assert e != 0
    t, s = _table(e)
    f16, p16 = ops.conv16_direct_multi([xin], filt, b.cuda(), relu=True, full="t16", pool="t16", rng=(t, s))
    torch.cuda.synchronize()
    assert isinstance(f16[0], ops.PairMap) and f16[0].slot == s
    _check_pairs(f16[0].data, full[0], e)
    _check_pairs(p16[0].data, pool[0], e)
    assert _rec(t, s) == _bits_max(full[0])
    # a NaN operand is recorded as non-finite
    xin[0, 3, 5, 0, 7] = float("nan")
    t.clear()
    ops.conv16_direct_multi([xin], filt, b.cuda(), relu=False, full="t16", rng=(t, s))
    assert _rec(t, s) > NONFINITE


@pytest.mark.parametrize("mag", [2.0 ** 20, 2.0 ** -12])
def test_producer_vgg_conv1(mag):
    g = torch.Generator().manual_seed(6)
    x = torch.rand((1, 3, 64, 96), generator=g).cuda()
    w = (_rand(g, 64, 3, 3, 3, scale=0.3) * (_gains(g, 64) * mag)[:, None, None, None]).cuda()
    b = (_rand(g, 64) * mag).cuda()
    ref = ops.vgg_conv1_pool_nhwc(x, w, b)                  # the same kernel with an fp32 result
    e = ops.pair_exponent(float(ref.abs().max()))
    t, s = _table(e)
    p = ops.vgg_conv1_pool_nhwc16(x, w, b, mode=3, rng=(t, s))
    torch.cuda.synchronize()
    _check_pairs(p.data, ref, e)
    assert _rec(t, s) == _bits_max(ref)
    x[0, 1, 10, 10] = float("inf")
    t.clear()
    ops.vgg_conv1_pool_nhwc16(x, w.abs(), b.abs(), mode=3, rng=(t, s))
    assert _rec(t, s) >= NONFINITE


@pytest.mark.parametrize("mag", [2.0 ** 20, 2.0 ** -12])
def test_producer_product_split16(mag):
    g = torch.Generator().manual_seed(7)
    D, P, C, qn = 11, 40, 64, 2
    ref = _rand(g, D, P, C).cuda()
    que = _rand(g, qn, P, C).cuda()
    scale = (_gains(g, C) * mag).repeat(qn, 1).cuda()
    shift = (_rand(g, qn, C) * mag).cuda()
    v = ((ref[None] * que[:, None]).double() * scale[:, None, None].double() + shift[:, None, None].double()).float().reshape(qn * D, P, C)
    e = ops.pair_exponent(float(v.abs().max()))
    t, s = _table(e)
    p = ops.product_split16(ref, que, scale, shift, 3, rng=(t, s))
    torch.cuda.synchronize()
    _check_pairs(p.data, v, e)
    assert abs(ops.bits_to_float([_rec(t, s)])[0] / float(v.abs().max()) - 1) <= 2.0 ** -22
    que[1, 3, 9] = float("nan")
    t.clear()
    ops.product_split16(ref, que, scale, shift, 3, rng=(t, s))
    assert _rec(t, s) > NONFINITE


@pytest.mark.parametrize("mag", [2.0 ** 20, 2.0 ** -12])
@pytest.mark.parametrize("pool", [False, True])
def test_producer_affine_split16(mag, pool):
    g = torch.Generator().manual_seed(8)
    N, H, W, C = 3, 10, 12, 64
    x = _rand(g, N, 1, H, W, C).cuda()
    scale = (_gains(g, C) * mag).repeat(N, 1).cuda()
    shift = (_rand(g, N, C) * mag).cuda()
    u = (x[:, 0].double() * scale[:, None, None].double() + shift[:, None, None].double()).float().clamp_min(0)
    v = F.max_pool2d(u.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) if pool else u
    e = ops.pair_exponent(float(v.abs().max()))
    t, s = _table(e)
    p = ops.affine_split16(x, scale, shift, 1, True, pool, 3, rng=(t, s))
    torch.cuda.synchronize()
    _check_pairs(p.data, v, e)
    assert abs(ops.bits_to_float([_rec(t, s)])[0] / float(v.abs().max()) - 1) <= 2.0 ** -22
    x[1, 0, 2, 3, 5] = float("inf")
    t.clear()
    ops.affine_split16(x, scale.abs(), shift, 1, True, pool, 3, rng=(t, s))
    assert _rec(t, s) >= NONFINITE


@pytest.mark.parametrize("e", [-20, -12, 0, 12, 20])
@pytest.mark.parametrize("Cout", [64, 128])
def test_consumer_conv16(e, Cout):
    g = torch.Generator().manual_seed(9 + Cout)
    x = _rand(g, 2, 16, 16, 64) * 2.0 ** e
    w = _rand(g, Cout, 9, 64, scale=(3.0 / (9 * 64)) ** 0.5)
    t, s = _table(e)
    xin = ops.PairMap(_split(x * 2.0 ** -e).cuda(), t, s)
    full, _ = ops.conv16_direct_multi([xin], ops.conv16_pack(w.cuda(), 3), None, relu=False, full=torch.float32)
    w4 = w.double().reshape(Cout, 3, 3, 64).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4, None, padding=1).permute(0, 2, 3, 1)
    err = float((full[0].cpu().double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-6, err


@pytest.mark.parametrize("e", [-20, -12, 0, 12, 20])
def test_consumer_conv16_3d(e):
    g = torch.Generator().manual_seed(19)
    x = _rand(g, 1, 8, 8, 8, 64) * 2.0 ** e
    w = _rand(g, 128, 27, 64, scale=(3.0 / (27 * 64)) ** 0.5)
    t, s = _table(e)
    xin = ops.PairMap(_split(x * 2.0 ** -e).cuda(), t, s)
    full, _ = ops.conv16_direct_multi([xin], ops.conv16_pack(w.cuda(), 3), None, relu=False, full=torch.float32, kd=3)
    w5 = w.double().reshape(128, 3, 3, 3, 64).permute(0, 4, 1, 2, 3)
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w5, None, padding=1).permute(0, 2, 3, 4, 1)
    err = float((full[0].cpu().double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-6, err


@pytest.mark.parametrize("e", [-20, -12, 0, 12, 20])
@pytest.mark.parametrize("k", [15, 7])
def test_consumer_corr16(e, k):
    g = torch.Generator().manual_seed(29 + k)
    T, Cin = k * k, 64
    w = _rand(g, 32, T, Cin, scale=(3.0 / (T * Cin)) ** 0.5)
    x = _rand(g, 1, 20, 28, Cin) * 2.0 ** e
    t, s = _table(e)
    out = torch.empty((1, 1, 20, 28, 32), device="cuda")
    ops.corr16_multi([ops.PairMap(_split(x * 2.0 ** -e).cuda(), t, s)], ops.corr16_pack(w.cuda(), 3), [out])
    w4 = w.double().reshape(32, k, k, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4, None, padding=k // 2).permute(0, 2, 3, 1)
    err = float((out[:, 0].cpu().double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 2e-6, err


@pytest.mark.parametrize("case", CASES)
def test_ex_entry_points_bit_identical(case):
    """Without a range (the _ex entry points with a NULL G6dRange16, which the legacy symbols forward to) and with exponents 0 and a
    record: the same bits."""
    c = case
    kd = c.get("kd", 1)
    g = torch.Generator().manual_seed(41 + c["Cin"])
    xs = [_split(_rand(g, *s_, c["Cin"])).cuda() for s_ in c["segs"]]
    w = _rand(g, c["Cout"], 9 * kd, c["Cin"], scale=(3.0 / (9 * kd * c["Cin"])) ** 0.5)
    filt = ops.conv16_pack(w.cuda(), MODE["pairs"])
    bias = _rand(g, c["Cout"]).cuda()
    typ = {"t16": "t16", "f32": torch.float32, None: None}
    kw = dict(relu=c["relu"], full=typ[c["full"]], pool=typ[c["pool"]], kd=kd)
    t, s = _table(0)
    outs = []
    for rng, inputs in ((None, xs), ((t, s), [ops.PairMap(x, t, s) for x in xs])):
        st = torch.zeros((64, c["Cout"], 2), dtype=torch.float64, device="cuda") if c.get("stats") else None
        fu, po = ops.conv16_direct_multi(inputs, filt, bias, stats=st, rows_per_group=c.get("rpg", 0), rng=rng, **kw)
        unwrap = lambda ts: [(q.data if isinstance(q, ops.PairMap) else q) for q in ts]
        outs.append((unwrap(fu), unwrap(po), st))
    (fa, pa, sa), (fb, pb, sb) = outs
    for a, b in zip(fa + pa, fb + pb):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert sa is None or torch.equal(sa, sb)
    # corr16 and the three elementwise producers
    for k in (15, 7):
        wc = ops.corr16_pack(_rand(g, 32, k * k, 64, scale=0.05).cuda(), 3)
        xc = _split(_rand(g, 1, 18, 22, 64)).cuda()
        o1, o2 = (torch.empty((1, 1, 18, 22, 32), device="cuda") for _ in range(2))
        ops.corr16_multi([xc], wc, [o1])
        ops.corr16_multi([ops.PairMap(xc, t, s)], wc, [o2])
        assert torch.equal(o1, o2)
    ref, que = _rand(g, 9, 30, 64).cuda(), _rand(g, 2, 30, 64).cuda()
    sc, sh = _rand(g, 2, 64).cuda(), _rand(g, 2, 64).cuda()
    assert torch.equal(ops.product_split16(ref, que, sc, sh, 3), ops.product_split16(ref, que, sc, sh, 3, rng=(t, s)).data)
    xa = _rand(g, 2, 1, 8, 10, 64).cuda()
    for pool in (False, True):
        assert torch.equal(ops.affine_split16(xa, sc, sh, 1, True, pool, 3), ops.affine_split16(xa, sc, sh, 1, True, pool, 3, rng=(t, s)).data)
    img = torch.rand((1, 3, 40, 56), generator=g).cuda()
    w0, b0 = _rand(g, 64, 3, 3, 3, scale=0.3).cuda(), _rand(g, 64).cuda()
    assert torch.equal(ops.vgg_conv1_pool_nhwc16(img, w0, b0, mode=3), ops.vgg_conv1_pool_nhwc16(img, w0, b0, mode=3, rng=(t, s)).data)


# ---- the detector headline with exact power-of-two gains on two trunk layers -------------------------------------------------------------
GAINS = {2: 2.0 ** -10, 4: 2.0 ** 18}          # trunk layer -> gain of its BN output (slots "trunk2" / "trunk4")


def _detect(net, case):
    data = {"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}}
    with torch.no_grad():
        return net.range_guarded(lambda: net(data))


def _check_head(out, g):
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        _vs_golden(out[k], g[k], what=f"range gains 480x640x32/{k}", relative=True)
    assert np.array_equal(out["que_select_id"].cpu().numpy(), g["que_select_id"])


def test_detector_headline_with_gains(golden):
    g = golden("det_head")
    case = synth.detector_case(32, 480, 640)
    net = _net("detector")
    net.load_state_dict(reparam(synth.synth_state_dict("detector"), GAINS))
    ops.PROFILE = []
    try:
        out1 = _detect(net, case)
        assert net.range_fallbacks == 1
        out2 = _detect(net, case)
        names = [p[3] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert any(n.startswith("conv16x3") for n in names)
    assert net.range_fallbacks == 1
    rep = net.range_report()
    assert rep["trunk2"]["e"] != 0 and rep["trunk4"]["e"] != 0, rep
    for o in (out1, out2):
        assert all(bool(torch.isfinite(o[k]).all()) for k in ("scores", "select_pr_offset", "select_pr_scale"))
        _check_head(o, g)


def test_detector_reload_drops_range_state():
    """A reparameterised state dict loaded into an instance that ran the original weights gives a fresh instance's outputs."""
    case = synth.detector_case(32, 480, 640)
    sd = synth.synth_state_dict("detector")
    used = _net("detector")
    _detect(used, case)
    used.load_state_dict(reparam(sd, GAINS))
    fresh = _net("detector")
    fresh.load_state_dict(reparam(sd, GAINS))
    a, b = _detect(used, case), _detect(fresh, case)
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        assert torch.equal(a[k], b[k]), k
    assert used.range_report() == fresh.range_report()


# ---- the public paths: estimator, pipeline, sharded mode, reloads --------------------------------------------------------------------
def test_estimator_guard_recomputes_out_of_window_calls():
    """Gen6DEstimator.predict with gains on two detector trunk layers: the first call falls back once and returns finite results equal
    to the original weights' within the fp32-class bar; the next call runs on the pairs with updated exponents and needs no fallback."""
    from gen6d_amd.synth_db import SyntheticDatabase
    from test_estimator_cpu import make_estimator
    db = SyntheticDatabase(n_views=24, size=(96, 128), focal=140.0)
    _, que_ids = db.get_split("all")
    img, K = db.get_image(que_ids[1]), db.get_K(que_ids[1])
    base = make_estimator("cuda", refine_iter=1, damped=True)
    base.build(db, "all")
    pose0, inter0 = base.predict(img, K)
    est = make_estimator("cuda", refine_iter=1, damped=True)
    est.detector.load_state_dict(reparam(synth.synth_state_dict("detector"), GAINS))
    est.build(db, "all")
    for call in range(2):
        pose, inter = est.predict(img, K)
        assert est.detector.range_fallbacks == 1, call
        assert np.isfinite(pose).all() and inter["sel_ref_idx"] == inter0["sel_ref_idx"]
        np.testing.assert_allclose(inter["det_position"], inter0["det_position"], rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(pose, pose0, atol=1e-4)
    assert est.detector.range_report()["trunk4"]["e"] != 0


def test_pipeline_rows_with_gains_and_range_check(golden):
    """TensorPipeline with reparameterised detector and refiner trunks: range_check() reports the detector, the recomputed rows match
    the original weights' rows (1e-4 of each column's range) and the reference's arg-max, and a second check reports nothing."""
    from gen6d_amd.pipeline import TensorPipeline
    g = golden("pipeline_rows")
    dev = torch.device("cuda", 0)
    fulls = synth.imgs_to_tensor(synth.synth_images(4, 480, 640, seed=100)).to(dev)
    crops = synth.imgs_to_tensor(synth.synth_images(4, 128, 128, seed=200)).to(dev)

    def rows(pipe):
        return torch.cat([pipe.query(fulls[j:j + 1], crops[j:j + 1]).clone() for j in range(4)], 0).cpu().numpy()
    base = TensorPipeline(dev)
    base.build()
    r0 = rows(base)
    pipe = TensorPipeline(dev)
    pipe.detector.load_state_dict(reparam(pipe.state_dicts["detector"], GAINS))
    pipe.refiner.load_state_dict(reparam(pipe.state_dicts["refiner"], GAINS, prefix="feature_net.backbone.features"))
    pipe.build()
    rows(pipe)
    assert "detector" in pipe.range_check()
    r = rows(pipe)
    assert pipe.range_check() == []
    rng = np.maximum(np.abs(r0).max(0), 1.0)
    assert (np.abs(r - r0) <= 1e-4 * rng).all(), float((np.abs(r - r0) / rng).max())
    assert np.array_equal(r[:, 3], g["rows"][:, 3])


def test_sharded_mode_raises_instead_of_falling_back():
    case = synth.detector_case(32, 480, 640)
    net = _net("detector")
    net.load_state_dict(reparam(synth.synth_state_dict("detector"), GAINS))
    with torch.no_grad():
        net({"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}})
    net.sharded = True                        # (what set_shard sets; the collectives themselves are not needed for the check)
    with pytest.raises(RuntimeError, match="sharded"):
        net.range_check()
    assert net.range_fallbacks == 0


def test_selector_and_refiner_reload_drop_filter_caches():
    """New weights loaded into instances that ran the old ones give a fresh instance's outputs (the 16-bit filter caches of the
    selector's products / stacks and the refiner's feature net were keyed on data_ptr(), which load_state_dict keeps)."""
    case = synth.selector_case(32, 5)
    crops = synth.imgs_to_tensor(synth.synth_images(2, 128, 128, seed=200)).cuda()
    imgs = synth.imgs_to_tensor(synth.synth_images(7, 128, 128, seed=300)).cuda()

    def run(kind, net):
        with torch.no_grad():
            if kind == "selector":
                net.extract_ref_feats(case["ref_imgs"].cuda(), case["ref_poses"].cuda(), case["object_center"].cuda(), case["object_vert"].cuda())
                return net.compute_view_point_feats(crops)[0]
            return net.run_feature_net(imgs)
    for kind in ("selector", "refiner"):
        used = _net(kind)
        run(kind, used)
        new = synth.synth_state_dict(kind, 7)
        used.load_state_dict(new)
        fresh = _net(kind)
        fresh.load_state_dict(new)
        a, b = run(kind, used), run(kind, fresh)
        assert torch.equal(a, b), kind
        assert used.range_report().keys() == fresh.range_report().keys()
