"""The detector's "fft" correlation route (Detector.corr_routes(h, w, qn), ops.corr_fft_multi): which calls take it, that a batch on it
meets the detector bars of test_networks_gpu.py with the golden's detection cell, and that it captures into a graph."""
import numpy as np
import pytest
import torch

from conftest import assert_pinned
from gen6d_amd import ops, synth
from gen6d_amd.network.detector import CORR_FFT_MIN_QUERIES
from oracle import gen6d_oracle as O
from test_networks_gpu import _accept, _net, _vs_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mid(golden):
    """det_mid (160 x 192 query, 32 references): the case, and the fp32 / fp64 oracle results of its one query, computed once."""
    g = golden("det_mid")
    case = synth.detector_case(int(g["rfn"]), int(g["hq"]), int(g["wq"]))
    sd = synth.synth_state_dict("detector")
    sd64 = O.to_double(sd)
    with torch.no_grad():
        o32 = O.detector_detect(sd, case["que_imgs"], O.detector_ref_feats(sd, case["ref_imgs"]))
        o64 = O.detector_detect(sd64, case["que_imgs"].double(), O.detector_ref_feats(sd64, case["ref_imgs"].double()))
    assert_pinned(g, case, sd, "det_mid")
    return g, case, o32, o64


def _loaded(case, **cfg):
    net = _net("detector", **cfg)
    with torch.no_grad():
        net.load_impl(case["ref_imgs"].cuda())
    return net


def test_routes(mid):
    _, case, _, _ = mid
    h, w = case["que_imgs"].shape[2:]
    net = _loaded(case)
    assert CORR_FFT_MIN_QUERIES >= 4
    base = net.corr_routes(h, w)
    assert base == ["corr16", "corr16", "patch"]
    assert net.corr_routes(h, w, CORR_FFT_MIN_QUERIES - 1) == base and net.corr_routes(h, w, 1) == base
    assert net.corr_routes(h, w, CORR_FFT_MIN_QUERIES) == ["fft", "corr16", "patch"]
    assert net.corr_routes(h, w, 16) == ["fft", "corr16", "patch"]
    for mode in ("bf16", "fp16"):                                  # reduced precision: as without qn
        with ops.math_mode(mode):
            assert net.corr_routes(h, w, 16) == net.corr_routes(h, w) == base
    cores = _loaded(case, fp32_cores=True)
    assert cores.corr_routes(h, w, 16) == cores.corr_routes(h, w) and "fft" not in cores.corr_routes(h, w, 16)
    net.set_shard(0, 1, force_collectives=True)
    assert net.corr_routes(h, w, 16) == base
    net.set_shard(0, 1)
    assert _loaded(case, corr_fft=False).corr_routes(h, w, 16) == base
    assert _loaded(case, corr_fft=True).corr_routes(h, w, 1) == ["fft", "corr16", "patch"]
    # 24 references: no corr16, so no fft either
    few = _net("detector")
    with torch.no_grad():
        few.load_impl(case["ref_imgs"][:24].cuda())
    assert "fft" not in few.corr_routes(h, w, 16)


def test_batch_on_the_fft_route_meets_the_detector_bars(mid):
    """det_mid's query replicated to the threshold batch: every row at the bars of test_networks_gpu.py::test_detector, the golden's cell;
    the 15x15 level ran as the three corr_fft launches and no 15x15 corr16 launch."""
    g, case, o32, o64 = mid
    qn = CORR_FFT_MIN_QUERIES
    net = _net("detector")
    que = case["que_imgs"].repeat(qn, 1, 1, 1).cuda()
    ops.PROFILE = []
    try:
        with torch.no_grad():
            out = net({"ref_imgs_info": {"imgs": case["ref_imgs"].cuda()}, "que_imgs_info": {"imgs": que}})
        torch.cuda.synchronize()
        names = [p[3] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert sum(n.startswith("corr_fft fwd") for n in names) == sum(n.startswith("corr_fft gemm") for n in names) \
        == sum(n.startswith("corr_fft inv") for n in names) >= 1
    assert not any("corr" in n and "k=15x15" in n for n in names) and any("corr" in n and "k=7x7" in n for n in names)
    p64, s64 = O.detector_parse(o64)
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        rep = lambda t: np.repeat(np.asarray(t.double() if torch.is_tensor(t) else t, np.float64), qn, 0)
        _accept(out[k], rep(o32[k]), rep(o64[k]), what=f"det_mid x{qn} fft/{k}", relative=True)
        _vs_golden(out[k], rep(g[k]), rep(o32[k]), rep(o64[k]), what=f"det_mid x{qn} fft/{k}", relative=True)
    ids = out["que_select_id"].cpu().numpy()
    assert np.array_equal(ids, np.repeat(g["que_select_id"], qn, 0)) and np.array_equal(ids, np.repeat(o64["que_select_id"].numpy(), qn, 0))
    np.testing.assert_allclose(out["positions"].cpu().numpy(), np.repeat(p64.numpy(), qn, 0), rtol=1e-3, atol=5e-2)
    np.testing.assert_allclose(out["scales"].cpu().numpy(), np.repeat(s64.numpy(), qn, 0), rtol=5e-3)


def test_captured_graph_on_the_fft_route(mid):
    """A graph of the threshold batch replayed on two different inputs equals the eager rows of those inputs."""
    _, case, _, _ = mid
    qn = CORR_FFT_MIN_QUERIES
    h, w = case["que_imgs"].shape[2:]
    net = _loaded(case)
    assert net.corr_routes(h, w, qn)[0] == "fft"
    qa = synth.imgs_to_tensor(synth.synth_images(qn, h, w, seed=71)).cuda()
    qb = synth.imgs_to_tensor(synth.synth_images(qn, h, w, seed=72)).cuda()
    stream = torch.cuda.Stream()
    keys = ("scores", "select_pr_offset", "select_pr_scale", "que_select_id")
    with torch.no_grad():
        want = [{k: net.detect_impl(q)[k].clone() for k in keys} for q in (qa, qb)]
        g_in = qa.clone()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(2):
                net.detect_impl(g_in)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            g_out = net.detect_impl(g_in)
        got = []
        with torch.cuda.stream(stream):
            for q in (qa, qb):
                g_in.copy_(q)
                graph.replay()
                got.append({k: g_out[k].clone() for k in keys})
        torch.cuda.synchronize()
    assert not torch.equal(want[0]["scores"], want[1]["scores"])
    for wnt, gt in zip(want, got):
        for k in keys:
            print(f"graph replay {k}: max |diff| {float((wnt[k].double() - gt[k].double()).abs().max()):.3e}")
            assert torch.equal(wnt[k], gt[k]), k
