"""The routes onto the implicit-GEMM kernel's fp16 hi / lo pair mode (ops.conv(pairs=...), conv_igemm_kernel<., MM = 3>):
(1) VolumeRefiner.run_volume_net at 4 volumes with the "igemmV" entries of refiner.ROUTES on, against the fp32_cores route on the same
    features, at the bar test_refiner_volume_pairs_gpu uses for the same comparison (1e-4 absolute); the listed layers are booked as
    `conv16x3 igemm` launches and with fp32_cores none is;
(2) the selector's logits at 2 queries x 8 references x 5 rotations against fp32_cores: same arg-max, difference under the selector
    goldens' bar (1e-4 absolute), with the candidate `fuse0` put into selector.SELECTOR_IGEMM_PAIR_LAYERS (empty by default) and booked on
    the pair mode;
(3) emptying the lists restores the parent's launches (the names in ops.PROFILE);
(4) an operand forced out of the fp16 window takes the fp32-core fallback and is counted in range_fallbacks."""
import pytest
import torch

from gen6d_amd import synth
from routes import forced_routes, igemm_layers, without
from test_networks_gpu import _net
from test_refiner_volume_pairs_gpu import _features, _volume_code

pytestmark = pytest.mark.gpu


def _igemm(labels):
    return [l for l in labels if l.startswith("conv16x3 igemm")]


@pytest.fixture(scope="module")
def volume_runs():
    """The volume net at 4 volumes, once per route: (code, labels) of fp32_cores and of the default route."""
    args = _features(4)
    want, labels32, _ = _volume_code(_net("refiner", fp32_cores=True), args)
    net = _net("refiner")
    got, labels, _ = _volume_code(net, args)
    return args, (want, labels32), (got, labels), net


def test_volume_net_igemm_pairs_against_fp32_cores(volume_runs):
    _, (want, labels32), (got, labels), net = volume_runs
    assert not _igemm(labels32), labels32
    booked = _igemm(labels)
    assert len(booked) == len(igemm_layers()), labels
    assert all("k=3x3x3" in l and "aff" in l for l in booked)
    assert net.range_check() is False
    assert {f"{n}.igemm" for n in igemm_layers()} <= set(net.range_report())
    err = float((got - want).abs().max())
    print(f"volume net, 4 volumes: igemm + halo-patch pair routes against fp32_cores, max abs difference {err:.3e} of codes up to "
          f"{float(want.abs().max()):.3e} (bar 1e-4)")
    assert err <= 1e-4, err


def test_empty_list_restores_the_launches(volume_runs):
    args, _, (_, labels), _ = volume_runs
    with forced_routes(without("igemm")):
        _, plain, _ = _volume_code(_net("refiner"), args)
    assert not _igemm(plain)
    # the same launches in the same order: a listed layer's label only gains the prefix
    assert [l[len("conv16x3 igemm "):] if l.startswith("conv16x3 igemm ") else l for l in labels] == plain


def _selector_logits(monkeypatch=None, **cfg):
    from gen6d_amd import ops
    rfn, an = 8, 5
    case = synth.selector_case(rfn, an)
    net = _net("selector", selector_angle_num=an, **cfg)
    que2 = synth.imgs_to_tensor(synth.synth_images(2, 128, 128, seed=5)).cuda()
    with torch.no_grad():
        net({"ref_imgs": case["ref_imgs"].cuda(), "ref_imgs_info": {"poses": case["ref_poses"].cuda()},
             "object_center": case["object_center"].cuda(), "object_vert": case["object_vert"].cuda(),
             "que_imgs_info": {"imgs": case["que_imgs"].cuda()}, "eval": True})
        ops.PROFILE = []
        try:
            logits, _ = net.compute_view_point_feats(que2)
            torch.cuda.synchronize()
            labels = [e[3] for e in ops.PROFILE]
        finally:
            ops.PROFILE = None
    return logits.cpu(), labels, net


def test_selector_fuse0_pairs_against_fp32_cores(monkeypatch):
    from gen6d_amd.network import selector
    want, labels32, _ = _selector_logits(fp32_cores=True)
    monkeypatch.setattr(selector, "SELECTOR_IGEMM_PAIR_LAYERS", ("fuse0",))      # the candidate layer (not listed by default)
    got, labels, net = _selector_logits()
    assert not _igemm(labels32)
    assert len(_igemm(labels)) == 1 and "in=1x4x4x768" in _igemm(labels)[0], labels
    assert net.range_check() is False
    err = float((got - want).abs().max())
    print(f"selector 2 queries x 8x5: logits against fp32_cores, max abs difference {err:.3e} (bar 1e-4)")
    assert torch.equal(got.argmax(1), want.argmax(1))
    assert err <= 1e-4, err
    monkeypatch.setattr(selector, "SELECTOR_IGEMM_PAIR_LAYERS", ())
    _, plain, _ = _selector_logits()
    assert not _igemm(plain)
    assert [l[len("conv16x3 igemm "):] if l.startswith("conv16x3 igemm ") else l for l in labels] == plain


def test_out_of_window_operand_takes_the_fallback(volume_runs):
    """conv1's operand forced out of the window: it sits behind an InstanceNorm, so no input scaling moves it; instead the exponent of
    conv1's slot is set to -40, which puts every operand above the window (v * 2^40 >= 2^15).  range_check reports the slot,
    range_guarded recomputes on the fp32-core routes and counts the fallback."""
    args, (want, _), _, _ = volume_runs
    net = _net("refiner")
    t = net.range_table()
    t.set_exponents({"volume.conv1.igemm": -40})

    def run():
        return _volume_code(net, args)
    before = net.range_fallbacks
    code, labels, _ = net.range_guarded(run)
    assert net.range_fallbacks == before + 1
    assert not any(l.startswith("conv16") for l in labels), "the recompute runs on the fp32-core routes"
    assert float((code - want).abs().max()) <= 1e-4
    assert t.e[t.names["volume.conv1.igemm"]] != -40, "the slot's exponent is re-chosen from the record"
