"""The refiner's 32^3 volume stage on the fp16 hi / lo pair kernel.
(1) g6d_refiner_volume_kp_pairs against g6d_refiner_volume_kp on the same inputs — 2 queries, 2 references, a small volume whose voxels
partly project outside the feature maps: hi + lo, scaled back by each map's own exponent (non-zero here), within 2^-21 of the map's range
of the fp32 entry's values (the bar of test_pair_handover_gpu), the recorded maxima those of the fp32 values bit for bit, nothing written
outside the two maps.
(2) VolumeRefiner.run_volume_net at 4 volumes: the pair route against the fp32_cores route on the same features, at the feature net's
bar (test_refiner_featnet_pairs_gpu: 1e-4 absolute); the route must actually be taken (the depth-folded pair launches of the listed layers booked, no
F(4x4,3x3) launch on the 32^3 stage) and must not be taken with fp32_cores."""
import pytest
import torch

from gen6d_amd import synth
from test_networks_gpu import _net

pytestmark = pytest.mark.gpu

GUARD_EL = 4096
E_MEAN, E_STD = -1, -3


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def test_pair_volumes_equal_the_fp32_volumes():
    import ctypes as C
    from gen6d_amd import lib, ops
    g = torch.Generator().manual_seed(7)
    B, rfn, fh, fw, Cc, sn, h_in, w_in = 2, 2, 6, 5, 12, 5, 24, 20          # (C = 12: lanes 3.. of a half-wave hold no channel)
    feats = _rand(g, B, rfn + 1, fh, fw, Cc).cuda()
    K = torch.tensor([[30.0, 0, w_in / 2], [0, 30.0, h_in / 2], [0, 0, 1]])
    ang = torch.tensor(0.3)
    R = torch.tensor([[torch.cos(ang), 0, torch.sin(ang)], [0, 1, 0], [-torch.sin(ang), 0, torch.cos(ang)]])

    def pose(tx, tz):
        return torch.cat([R, torch.tensor([[tx], [0.1], [tz]])], 1)
    ref_Ks = K.expand(B, rfn, 3, 3).contiguous().cuda()
    ref_poses = torch.stack([torch.stack([pose(0.2 * (r + q), 2.5 + 0.5 * r) for r in range(rfn)]) for q in range(B)]).contiguous().cuda()
    K_in = K.expand(B, 3, 3).contiguous().cuda()
    pose_in = torch.stack([pose(-0.4 * q, 2.0) for q in range(B)]).contiguous().cuda()
    lin = torch.linspace(-1, 1, sn).cuda()
    vox = sn ** 3
    mean32 = torch.empty((B, vox, 2 * Cc), device="cuda")
    std32 = torch.empty((B, vox, Cc), device="cuda")
    ops.refiner_volume_kp(feats, ref_Ks, ref_poses, K_in, pose_in, lin, h_in, w_in, mean32, std32)
    q = mean32[..., Cc:]
    outside = (q == 0).all(-1)
    assert bool(outside.any()) and not bool(outside.all()), "the case must hold voxels outside and inside the query's feature map"

    table = ops.RangeTable(torch.device("cuda"))
    table.set_exponents({"mean": E_MEAN, "std": E_STD})
    table.clear()
    nm, ns = B * vox * 4 * Cc, B * vox * 2 * Cc
    bm = torch.full((nm + 2 * GUARD_EL,), float("nan"), dtype=torch.float16, device="cuda")
    bs = torch.full((ns + 2 * GUARD_EL,), float("nan"), dtype=torch.float16, device="cuda")
    ra_m, ra_s = table.arg(-1, table.slot("mean")), table.arg(-1, table.slot("std"))
    lib.check(lib.load().g6d_refiner_volume_kp_pairs(
        C.c_void_p(feats.data_ptr()), C.c_void_p(ref_Ks.data_ptr()), C.c_void_p(ref_poses.data_ptr()), C.c_void_p(K_in.data_ptr()),
        C.c_void_p(pose_in.data_ptr()), C.c_void_p(lin.data_ptr()), rfn, fh, fw, Cc, h_in, w_in, sn, C.c_void_p(bm[GUARD_EL:].data_ptr()),
        C.c_void_p(bs[GUARD_EL:].data_ptr()), B, C.byref(ra_m), C.byref(ra_s), ops._stream()), "g6d_refiner_volume_kp_pairs")
    torch.cuda.synchronize()
    rec = table.read()
    for name, buf, n, want, e in (("mean", bm, nm, mean32, E_MEAN), ("std", bs, ns, std32, E_STD)):
        b = buf.cpu()
        assert bool(torch.isnan(b[:GUARD_EL]).all() and torch.isnan(b[GUARD_EL + n:]).all()), f"{name}: wrote outside the map"
        planes = b[GUARD_EL:GUARD_EL + n].view(B, vox, 2, -1).double()
        val = (planes[:, :, 0] + planes[:, :, 1]) * 2.0 ** e
        w = want.cpu()
        rng = float(w.abs().max())
        err = float((val - w.double()).abs().max()) / rng
        print(f"{name}: error / range {err:.3e} (bar {2.0 ** -21:.3e}), recorded {rec[name]} vs {rng}")
        assert err <= 2.0 ** -21, (name, err)                   # (NaN — an element never written — fails here too)
        assert rec[name] == rng, (name, "recorded maximum", rec[name], rng)


def _features(qn):
    c = synth.refiner_case()
    rfn = c["ref_imgs"].shape[1]
    g = torch.Generator().manual_seed(5)
    feats = (torch.rand((qn, rfn + 1, 32, 32, 128), generator=g) * 2 - 1).cuda()          # (any feature maps: the volume stage is under test)
    rep = lambda t: t.expand(qn, *t.shape[1:]).contiguous().cuda()
    return feats, rep(c["ref_Ks"]), rep(c["ref_poses"]), rep(c["Ks_in"]), rep(c["poses_in"])


def _volume_code(net, args, sn=32):
    from gen6d_amd import ops
    ops.PROFILE = []
    try:
        with torch.no_grad():
            ops.stats_arena_begin(args[0].device)
            mean_in, std = net.feature_volumes(*args, 128, 128, sn)
            code = net.run_volume_net(mean_in, std, sn)
        torch.cuda.synchronize()
        labels = [e[3] for e in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return code, labels, isinstance(mean_in, ops.PairMap)


def test_volume_net_pair_route_against_fp32_cores():
    from gen6d_amd.network import refiner
    qn = 4
    assert qn >= refiner.F43_MIN_QUERIES
    args = _features(qn)
    cores = _net("refiner", fp32_cores=True)
    want, labels32, pairs32 = _volume_code(cores, args)
    assert not pairs32 and not any("conv16" in l for l in labels32), labels32
    net = _net("refiner")
    got, labels, pairs = _volume_code(net, args)
    n16 = 4 + len([k for k in ("volume.conv0", "volume.conv2") if "pair" in refiner.ROUTES[k]])      # two layers per embed, and conv0 / conv2 where they are listed
    folded = [l for l in labels if l.startswith("conv16x3 direct") and "k=3x3x3" in l]
    assert pairs and len(folded) == n16, labels                 # the route is taken: every listed layer booked on the pair kernel
    assert net.range_check() is False
    assert {"volume.mean_in", "volume.std", "volume.mean_embed.mid", "volume.var_embed.mid"} <= set(net.range_report())
    err = float((got - want).abs().max())
    print(f"volume net, {qn} volumes: pair route against fp32_cores, max abs difference {err:.3e} of codes up to {float(want.abs().max()):.3e} (bar 1e-4)")
    assert tuple(got.shape) == tuple(want.shape) == (qn, 64, 512)
    assert err <= 1e-4, err
