"""The refiner's 2-D feature net on the fp16 hi / lo pair kernel (VolumeRefiner.run_feature_net, big calls of the fp32 path): the route
itself — which launches a call books — and its result against the CPU oracle in fp32 and float64 with the acceptance rule of
test_networks_gpu.py (|new - ref64| <= max(1e-4, 1.5 |ref32 - ref64|)), on the seven crops of synth.refiner_case(); with cfg
fp32_cores the same call must book no 16-bit launch and meet the same rule; and a batched step of 4 queries (28 crops: where the pair
route starts by itself) must agree with the four single-query steps, which run the fp32-core feature net."""
import numpy as np
import pytest
import torch

from gen6d_amd import synth
from oracle import gen6d_oracle as O
from routes import forced_routes, with_pairs
from test_networks_gpu import _accept, _net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    c = synth.refiner_case()
    imgs = torch.cat([c["ref_imgs"][0], c["que_imgs"]], 0)                       # the seven crops of one step, query last
    sd = synth.synth_state_dict("refiner")
    with torch.no_grad():
        r32 = O.refiner_feature_net(sd, imgs).permute(0, 2, 3, 1)
        r64 = O.refiner_feature_net(O.to_double(sd), imgs.double()).permute(0, 2, 3, 1)
    return imgs, r32, r64


def _profiled(net, imgs):
    from gen6d_amd import ops
    ops.PROFILE = []
    try:
        with torch.no_grad():
            out = net.run_feature_net(imgs.cuda(), f43=True)
        torch.cuda.synchronize()
        labels = [e[3] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return out, labels


ALL_BRANCHES = ("conv0", "conv1", "conv2", "conv_out")
ALL_ON_PAIRS = [f"featnet.{b}.{i}" for b in ALL_BRANCHES for i in (0, 3)]


def test_pair_route_books_conv16x3_and_meets_the_oracle(case):
    """All four branches on pairs (whatever subset the product routes, refiner.ROUTES: every branch's route stays tested)."""
    from gen6d_amd.network import refiner
    imgs, r32, r64 = case
    product = tuple(b for b in ALL_BRANCHES if all("pair" in refiner.ROUTES[f"featnet.{b}.{i}"] for i in (0, 3)))
    with forced_routes(with_pairs(ALL_ON_PAIRS)):
        net = _net("refiner")
        out, labels = _profiled(net, imgs)
    layers = [l for l in labels if l.startswith("conv16x3 direct") and l.endswith(" stats")]      # (the trunk's launches carry no statistics)
    assert len(layers) == 8, labels
    assert not any("wino3x3" in l or "conv N=" in l for l in labels), labels                      # no Winograd / implicit-GEMM entry at all
    _accept(out, r32, r64, what="feature net on pairs, 7 crops")
    assert net.range_check() is False
    want = {"featnet.f3", "featnet.f5", "featnet.f7", "featnet.cat"} | {f"featnet.{b}.mid" for b in ALL_BRANCHES}      # one slot per pair producer
    assert want <= set(net.range_report())
    if tuple(product) != ALL_BRANCHES:                          # the product's mix of routes: its branches on pairs, the others as before
        net2 = _net("refiner")
        out2, labels2 = _profiled(net2, imgs)
        assert len([l for l in labels2 if l.startswith("conv16x3 direct") and l.endswith(" stats")]) == 2 * len(product), labels2
        assert len([l for l in labels2 if "conv N=" in l]) == 8 - 2 * len(product), labels2
        _accept(out2, r32, r64, what="feature net, the product's branches on pairs, 7 crops")
        assert net2.range_check() is False


def test_fp32_cores_books_no_16_bit_launch(case):
    imgs, r32, r64 = case
    net = _net("refiner", fp32_cores=True)
    out, labels = _profiled(net, imgs)
    assert not any("conv16" in l for l in labels), labels
    assert len([l for l in labels if "conv N=" in l]) == 8, labels
    _accept(out, r32, r64, what="feature net on the fp32 cores, 7 crops")


def test_batched_step_agrees_with_single_query_steps():
    c = synth.refiner_case()
    qn, rfn = 4, c["ref_imgs"].shape[1]
    # four different queries: the case's crops, shifted by a few pixels per query
    que = torch.cat([torch.roll(c["que_imgs"], (3 * i, -2 * i), (2, 3)) for i in range(qn)], 0).cuda()
    refs = torch.stack([torch.roll(c["ref_imgs"][0], (-i, 2 * i), (2, 3)) for i in range(qn)], 0).cuda()
    rep = lambda t: t.expand(qn, *t.shape[1:]).contiguous().cuda()
    Ks, poses, rKs, rposes = rep(c["Ks_in"]), rep(c["poses_in"]), rep(c["ref_Ks"]), rep(c["ref_poses"])
    assert tuple(refs.shape) == (qn, rfn, 3, 128, 128)
    with forced_routes(with_pairs(ALL_ON_PAIRS)), torch.no_grad():
        net = _net("refiner")
        rot, off, scl = net._step(que, Ks, poses, refs, rKs, rposes)
        assert net.range_check() is False
        for q in range(qn):
            r1, o1, s1 = net._step(que[q:q + 1], Ks[q], poses[q], refs[q], rKs[q], rposes[q])
            for name, a, b in (("rotation", rot[q], r1[0]), ("offset", off[q], o1[0]), ("scale", scl[q], s1[0])):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=1e-4, err_msg=f"query {q} {name}")
