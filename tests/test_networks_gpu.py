"""Stage-level parity on a real MI355X: the drop-in Detector / ViewpointSelector / VolumeRefiner (HIP kernels through
the C ABI) against (a) the golden vectors produced by the reference's own modules and (b) the CPU oracle in fp32 and
fp64 on the same seeded inputs.

Acceptance: the reference's own fp32 path is only accurate to ~1e-3 on selector logits (13 stacked
instance norms), so a tensor passes when  |new - ref64| <= max(tol, 1.5 * |ref32 - ref64|)  with tol = 1e-4 absolute
(north_star: "within 1e-4 fp32 on logits"; scaled by the tensor's range when that exceeds 1), and arg-max indices must
be identical."""
import numpy as np
import pytest
import torch

from conftest import assert_pinned
from gen6d_amd import synth
from oracle import gen6d_oracle as O

pytestmark = pytest.mark.gpu


def _net(kind, **cfg):
    from gen6d_amd import lib
    from gen6d_amd.network import name2network
    lib.load()
    net = name2network[kind]({"name": "t", **cfg}).eval()
    net.load_state_dict(synth.synth_state_dict(kind, an=cfg.get("selector_angle_num", 5)))
    return net.cuda()


def _cuda(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def _accept(new, ref32, ref64, tol=1e-4, what="", relative=False):
    """|new - ref64|.max() <= max(tol, 1.5 * |ref32 - ref64|.max()), ABSOLUTE by default (north_star: "within 1e-4 fp32 on
    logits"); `relative=True` divides by max(|ref64|.max(), 1) and is used only for the detector's un-normalised score /
    offset / scale maps.  Every achieved error goes to the parity log (profiles/r02_parity.md)."""
    import inspect
    from parity_log import record
    new, ref32, ref64 = (np.asarray(t.detach().cpu().double() if torch.is_tensor(t) else t, dtype=np.float64) for t in (new, ref32, ref64))
    rng = max(np.abs(ref64).max(), 1.0) if relative else 1.0
    e_new, e_ref = np.abs(new - ref64).max() / rng, np.abs(ref32 - ref64).max() / rng
    name = next((f.function for f in inspect.stack()[1:] if f.function.startswith("test_")), inspect.stack()[1].function)
    record(name, what, e_new, max(tol, 1.5 * e_ref), e_ref, "relative to range" if relative else "absolute")
    assert e_new <= max(tol, 1.5 * e_ref), f"{what}: err {e_new:.3e} vs reference-fp32 noise {e_ref:.3e}"
    return e_new, e_ref


def _vs_golden(new, gold, ref32=None, ref64=None, tol=1e-4, what="", relative=False):
    """HIP path against the REFERENCE'S OWN output (golden fixture, inputs pinned by hash): |new - gold|.max() <= max(tol, 1.5 x
    |ref32 - ref64|.max()) — the golden is an fp32 evaluation, so it carries the reference's own fp32 noise, which the oracle pair
    measures on this host.  Absolute by default, `relative` = of the golden's range (detector maps)."""
    import inspect
    from parity_log import record
    f = lambda t: np.asarray(t.detach().cpu().double() if torch.is_tensor(t) else t, dtype=np.float64)
    new, gold = f(new), f(gold)
    rng = max(np.abs(gold).max(), 1.0) if relative else 1.0
    noise = np.abs(f(ref32) - f(ref64)).max() / rng if ref32 is not None else 0.0
    err = np.abs(new - gold).max() / rng
    caller = next((f.function for f in inspect.stack()[1:] if f.function.startswith("test_")), inspect.stack()[1].function)
    record(caller, what + " vs reference golden", err, max(tol, 1.5 * noise), noise if ref32 is not None else None,
           "relative to range" if relative else "absolute")
    assert err <= max(tol, 1.5 * noise), f"{what} vs reference golden: err {err:.3e} (fp32 noise of the reference {noise:.3e})"
    return err


def _check_detector(g, net, tag):
    """net on the golden case `tag` against the reference's golden and the fp32 / fp64 oracle."""
    case = synth.detector_case(int(g["rfn"]), int(g["hq"]), int(g["wq"]))
    with torch.no_grad():
        out = net({"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}})
        sd = synth.synth_state_dict("detector"); sd64 = O.to_double(sd)
        o32 = O.detector_detect(sd, case["que_imgs"], O.detector_ref_feats(sd, case["ref_imgs"]))
        o64 = O.detector_detect(sd64, case["que_imgs"].double(), O.detector_ref_feats(sd64, case["ref_imgs"].double()))
        p64, s64 = O.detector_parse(o64)
    assert_pinned(g, case, sd, tag)
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        _accept(out[k], o32[k], o64[k], what=f"{tag}/{k}", relative=True)
        _vs_golden(out[k], g[k], o32[k], o64[k], what=f"{tag}/{k}", relative=True)
    assert np.array_equal(out["que_select_id"].cpu().numpy(), g["que_select_id"])
    assert np.array_equal(out["que_select_id"].cpu().numpy(), o64["que_select_id"].numpy())
    np.testing.assert_allclose(out["positions"].cpu().numpy(), p64.numpy(), rtol=1e-3, atol=5e-2)
    np.testing.assert_allclose(out["scales"].cpu().numpy(), s64.numpy(), rtol=5e-3)


@pytest.mark.parametrize("tag", ["det_small", "det_mid"])
def test_detector(golden, tag):
    _check_detector(golden(tag), _net("detector"), tag)


@pytest.mark.parametrize("tag", ["det_small", "det_mid"])
def test_per_scale_detector_path(golden, tag, monkeypatch):
    """The per-scale path (one trunk pass and one correlation launch per level and scale, _detect_batch(multi=False): what a pyramid
    beyond the 2^29-float reach of one launch runs) meets test_detector's bars."""
    from gen6d_amd.network.detector import Detector
    batch = Detector._detect_batch
    monkeypatch.setattr(Detector, "_detect_batch", lambda self, que_imgs, multi=True: batch(self, que_imgs, multi=False))
    _check_detector(golden(tag), _net("detector"), tag)


def test_fp32_cores_config(golden):
    """cfg 'fp32_cores': every product of the fp32 path on the fp32 matrix cores — no direct 16-bit kernel (conv16 / corr16) launches,
    where the default configuration runs the detector's pyramid trunk, its 15x15 / 7x7 correlations and the selector's products on them —
    and the fp32 golden bars still hold (det_mid: 32 references, sel_small)."""
    from gen6d_amd import ops

    def names(fn):
        ops.PROFILE = []
        try:
            fn()
            return [p[3] for p in ops.PROFILE]
        finally:
            ops.PROFILE = None
    g = golden("det_mid")
    assert any(n.startswith("conv16") for n in names(lambda: _check_detector(g, _net("detector"), "det_mid")))
    assert not any(n.startswith("conv16") for n in names(lambda: _check_detector(g, _net("detector", fp32_cores=True), "det_mid")))
    g = golden("sel_small")
    res = []
    assert not any(n.startswith("conv16") for n in names(lambda: res.append(_selector_case(int(g["rfn"]), int(g["an"]), fp32_cores=True))))
    out, (l32, a32), (l64, a64) = res[0]
    _vs_golden(out["ref_vp_logits"], g["logits"], l32, l64, what="sel_small fp32_cores/logits")
    _vs_golden(out["angles_pr"], g["angles"], a32, a64, what="sel_small fp32_cores/angles")
    assert np.array_equal(out["ref_vp_logits"].argmax(1).cpu().numpy(), g["logits"].argmax(1))


def _selector_case(rfn, an, **cfg):
    case = synth.selector_case(rfn, an)
    net = _net("selector", selector_angle_num=an, **cfg)
    sd = synth.synth_state_dict("selector", an=an); sd64 = O.to_double(sd)
    with torch.no_grad():
        out = net({"ref_imgs": case["ref_imgs"].cuda(), "ref_imgs_info": {"poses": case["ref_poses"].cuda()},
                   "object_center": case["object_center"].cuda(), "object_vert": case["object_vert"].cuda(),
                   "que_imgs_info": {"imgs": case["que_imgs"].cuda()}, "eval": True})
        c32, e32 = O.selector_ref_state(sd, case["ref_imgs"], case["ref_poses"], case["object_center"], case["object_vert"])
        l32, a32 = O.selector_forward(sd, case["que_imgs"], c32, e32)
        c64, e64 = O.selector_ref_state(sd64, case["ref_imgs"].double(), case["ref_poses"].double(),
                                        case["object_center"].double(), case["object_vert"].double())
        l64, a64 = O.selector_forward(sd64, case["que_imgs"].double(), c64, e64)
    return out, (l32, a32), (l64, a64)


@pytest.mark.parametrize("tag", ["sel_small", "sel_mid"])
def test_selector_golden(golden, tag):
    g = golden(tag)
    out, (l32, a32), (l64, a64) = _selector_case(int(g["rfn"]), int(g["an"]))
    an = int(g["an"])
    assert_pinned(g, synth.selector_case(int(g["rfn"]), an), synth.synth_state_dict("selector", an=an), tag)
    _accept(out["ref_vp_logits"], l32, l64, what="logits")
    _accept(out["angles_pr"], a32, a64, what="angles")
    _vs_golden(out["ref_vp_logits"], g["logits"], l32, l64, what=f"{tag}/logits")
    _vs_golden(out["angles_pr"], g["angles"], a32, a64, what=f"{tag}/angles")
    assert np.array_equal(out["ref_vp_logits"].argmax(1).cpu().numpy(), g["logits"].argmax(1))
    assert np.array_equal(out["ref_vp_logits"].argmax(1).cpu().numpy(), l64.argmax(1).numpy())


def test_selector_headline_64x5():
    """BASELINE config: 64 reference views x 5 rotations, one 128x128 query."""
    out, (l32, a32), (l64, a64) = _selector_case(64, 5)
    e_new, e_ref = _accept(out["ref_vp_logits"], l32, l64, what="logits")
    _accept(out["angles_pr"], a32, a64, what="angles")
    print(f"selector 64x5: logits err vs fp64 {e_new:.2e} (reference fp32 path: {e_ref:.2e})")
    assert np.array_equal(out["ref_vp_logits"].argmax(1).cpu().numpy(), l64.argmax(1).numpy())


def test_selector_numpy_api():
    an, rfn = 5, 8
    net = _net("selector", selector_angle_num=an)
    refs = synth.synth_images(rfn, 128, 128, 1)
    rots = synth.rotated_copies(refs, an)
    poses, _ = synth.fibonacci_cameras(rfn)
    net.load_ref_imgs(rots, poses, np.zeros(3), np.array([0.0, 0.0, 1.0]))
    res = net.select_que_imgs(synth.synth_images(2, 128, 128, 5))
    assert res["ref_idx"].shape == (2,) and res["ref_idx"].dtype == np.int64
    assert res["angles"].shape == (2,) and res["scores"].shape == (2, rfn)
    assert np.array_equal(res["ref_idx"], res["scores"].argmax(1))


def test_refiner(golden):
    g = golden("ref_step")
    net = _net("refiner")
    c = synth.refiner_case()
    sd = synth.synth_state_dict("refiner"); sd64 = O.to_double(sd)
    with torch.no_grad():
        out = net({"que_imgs_info": {"imgs": c["que_imgs"].cuda(), "Ks_in": c["Ks_in"].cuda(), "poses_in": c["poses_in"].cuda()},
                   "ref_imgs_info": {"imgs": c["ref_imgs"].cuda(), "Ks": c["ref_Ks"].cuda(), "poses": c["ref_poses"].cuda()},
                   "inference": True})
        o32 = O.refiner_forward(sd, c["que_imgs"], c["Ks_in"], c["poses_in"], c["ref_imgs"], c["ref_Ks"], c["ref_poses"])
        d = lambda t: t.double()
        o64 = O.refiner_forward(sd64, d(c["que_imgs"]), d(c["Ks_in"]), d(c["poses_in"]), d(c["ref_imgs"]), d(c["ref_Ks"]), d(c["ref_poses"]))
    assert_pinned(g, c, sd, "ref_step")
    for k in ("rotation", "offset", "scale"):
        _accept(out[k], o32[k], o64[k], what=k)
        _vs_golden(out[k], g[k], o32[k], o64[k], what=f"ref_step/{k}")


def test_refiner_feature_volume_intermediates(golden):
    """K12/K13 against the reference's own construct_feature_volume (sub-sampled golden slices)."""
    g = golden("ref_step")
    net = _net("refiner")
    c = _cuda(synth.refiner_case())
    with torch.no_grad():
        feats = net.run_feature_net(torch.cat([c["ref_imgs"][0], c["que_imgs"]], 0))
        np.testing.assert_allclose(feats[-1, :, :, :8].permute(2, 0, 1).cpu().numpy(), g["que_feats"][0], atol=2e-4)
        from gen6d_amd import ops
        projs = torch.cat([c["ref_Ks"][0] @ c["ref_poses"][0], c["Ks_in"] @ c["poses_in"]], 0).contiguous()
        lin = torch.linspace(-1, 1, 32, device="cuda")
        mean_in = torch.empty((32 ** 3, 256), device="cuda"); std = torch.empty((32 ** 3, 128), device="cuda")
        ops.refiner_volume(feats.contiguous(), projs, c["poses_in"][0, :, :3].contiguous(), lin, 128, 128, mean_in, std)
    v = lambda t: t.view(32, 32, 32, -1)[::4, ::4, ::4, :8].permute(3, 0, 1, 2).cpu().numpy()
    np.testing.assert_allclose(v(mean_in[:, :128]), g["vol_mean"][0], atol=3e-4)
    np.testing.assert_allclose(v(mean_in[:, 128:]), g["vol_in"][0], atol=3e-4)
    np.testing.assert_allclose(v(std), g["vol_std"][0], atol=3e-4)


def test_selector_36_rotations():
    """BASELINE config 2 variant: 36 in-plane rotations (reachable only with selector_angle_num=36 weights)."""
    out, (l32, a32), (l64, a64) = _selector_case(12, 36)
    _accept(out["ref_vp_logits"], l32, l64, what="logits an=36")
    _accept(out["angles_pr"], a32, a64, what="angles an=36")
    assert np.array_equal(out["ref_vp_logits"].argmax(1).cpu().numpy(), l64.argmax(1).numpy())


@pytest.mark.parametrize("rfn,an", [(4, 5), (3, 1), (5, 3)])
def test_selector_small_and_ragged(rfn, an):
    """Edge shapes: few reference views (the reference's InstanceNorm1d over the reference axis raises for one and is
    ill-conditioned for two), a
    single rotation, sizes that are not multiples of any tile."""
    out, (l32, a32), (l64, a64) = _selector_case(rfn, an)
    assert out["ref_vp_logits"].shape == (1, rfn)
    _accept(out["ref_vp_logits"], l32, l64, tol=2e-4, what="logits")
    _accept(out["angles_pr"], a32, a64, tol=2e-4, what="angles")


@pytest.mark.parametrize("rfn,hq,wq", [(1, 64, 96), (5, 72, 104), (32, 128, 128)])
def test_detector_ragged_sizes(rfn, hq, wq):
    """Query sizes that are multiples of 8 but not of 32 (every scale is padded up to x32 internally), odd ref counts."""
    net = _net("detector")
    case = synth.detector_case(rfn, hq, wq)
    sd = synth.synth_state_dict("detector"); sd64 = O.to_double(sd)
    with torch.no_grad():
        out = net({"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}})
        o32 = O.detector_detect(sd, case["que_imgs"], O.detector_ref_feats(sd, case["ref_imgs"]))
        o64 = O.detector_detect(sd64, case["que_imgs"].double(), O.detector_ref_feats(sd64, case["ref_imgs"].double()))
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        assert out[k].shape == o64[k].shape
        _accept(out[k], o32[k], o64[k], what=f"{rfn}x{hq}x{wq}/{k}", relative=True)
    assert np.array_equal(out["que_select_id"].cpu().numpy(), o64["que_select_id"].numpy())


def test_multi_query_batch():
    """qn = 3 queries in one call keep the reference's [qn, ...] contracts (selector and detector)."""
    net = _net("selector")
    case = synth.selector_case(8, 5)
    ques = synth.imgs_to_tensor(synth.synth_images(3, 128, 128, 77)).cuda()
    with torch.no_grad():
        net.extract_ref_feats(case["ref_imgs"].cuda(), case["ref_poses"].cuda(), case["object_center"].cuda(), case["object_vert"].cuda())
        logits, angles = net.compute_view_point_feats(ques)
        one = net.compute_view_point_feats(ques[1:2])
    assert logits.shape == (3, 8) and angles.shape == (3, 8)
    np.testing.assert_allclose(logits[1].cpu().numpy(), one[0][0].cpu().numpy(), atol=1e-4)   # atomics order, MIOpen batch algo


def test_selector_reference_permutation_equivariance_full_size():
    """Size-independent property at the headline size (64 refs x 5 rotations): permuting the reference views permutes
    logits and angles the same way (every cross-reference op — InstanceNorm statistics, attention — is symmetric in the
    references, and `object_forward` is pinned by keeping view 0 first)."""
    an, rfn = 5, 64
    case = synth.selector_case(rfn, an)
    net = _net("selector", selector_angle_num=an)
    perm = torch.cat([torch.zeros(1, dtype=torch.long), 1 + torch.randperm(rfn - 1, generator=torch.Generator().manual_seed(5))])
    with torch.no_grad():
        args = (case["object_center"].cuda(), case["object_vert"].cuda())
        net.extract_ref_feats(case["ref_imgs"].cuda(), case["ref_poses"].cuda(), *args)
        l0, a0 = net.compute_view_point_feats(case["que_imgs"].cuda())
        net.extract_ref_feats(case["ref_imgs"][:, perm].cuda(), case["ref_poses"][perm].cuda(), *args)
        l1, a1 = net.compute_view_point_feats(case["que_imgs"].cuda())
    np.testing.assert_allclose(l1.cpu().numpy(), l0[:, perm.cuda()].cpu().numpy(), atol=2e-4)
    np.testing.assert_allclose(a1.cpu().numpy(), a0[:, perm.cuda()].cpu().numpy(), atol=2e-4)
    assert int(perm[l1.argmax(1)[0]]) == int(l0.argmax(1)[0])


def test_detector_reference_permutation_invariance_full_size():
    """Headline detector size (480x640 query, 32 refs): the max over references makes every output invariant to the
    order of the reference views."""
    case = synth.detector_case(32, 480, 640)
    net = _net("detector")
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        o0 = net({"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}})
        o1 = net({"ref_imgs_info": {"imgs": case["ref_imgs"][perm].cuda()}, "que_imgs_info": {"imgs": case["que_imgs"].cuda()}})
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        rng = o0[k].abs().max().item()
        assert (o0[k] - o1[k]).abs().max().item() <= 2e-5 * max(rng, 1.0), k
    assert torch.equal(o0["que_select_id"], o1["que_select_id"])
    assert o0["scores"].shape == (1, 1, 60, 80)


@pytest.mark.parametrize("switches", ["attr:gen6d_amd.ops.FUSED_FINALIZE=0", "library_trunk",
                                      "knob:conv_wino=0,knob:conv_wino43=0,knob:conv_patch=0"],
                         ids=["separate-finalize", "library-trunk", "generic-conv-only"])
def test_alternative_paths_keep_parity(switches):
    """Other kernels / launch structures for the same function (selected through tests/conftest.py's G6D_TEST_SWITCHES: library knobs,
    package attributes, the MIOpen trunk of tools/): the golden detector / selector / refiner tests must pass on them too."""
    import os
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "test_detector and det_small or test_selector_golden and sel_small or test_refiner"],
                         env=dict(os.environ, G6D_TEST_SWITCHES=switches), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


def test_captured_graph_survives_larger_eager_work_on_its_stream():
    """The InstanceNorm statistics arena is keyed by the launching stream and cleared up to its high-water mark by eager calls; a captured
    clear keeps its size.  A graph captured with 2 queries must still be right after an EAGER batch of 8 queries has dirtied more of the same
    stream's arena (round 5: captured clears cover the whole arena)."""
    case = synth.selector_case(8, 5)
    net = _net("selector")
    q2 = synth.imgs_to_tensor(synth.synth_images(2, 128, 128, seed=61)).cuda()
    q8 = synth.imgs_to_tensor(synth.synth_images(8, 128, 128, seed=62)).cuda()
    stream = torch.cuda.Stream()
    with torch.no_grad():
        net.extract_ref_feats(case["ref_imgs"].cuda(), case["ref_poses"].cuda(), case["object_center"].cuda(), case["object_vert"].cuda())
        want = net.compute_view_point_feats(q2)[0].clone()
        stream.wait_stream(torch.cuda.current_stream())
        g_in = q2.clone()
        with torch.cuda.stream(stream):
            for _ in range(2):
                net.compute_view_point_feats(g_in)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            g_out = net.compute_view_point_feats(g_in)[0]
        with torch.cuda.stream(stream):
            graph.replay()
            first = g_out.clone()
            net.compute_view_point_feats(q8)                 # eager, same stream, four times the statistics
            graph.replay()
            second = g_out.clone()
        torch.cuda.synchronize()
    assert float((first - want).abs().max()) <= 1e-4
    assert float((second - want).abs().max()) <= 1e-4, "the replay after larger eager work on the stream differs: stale statistics"
