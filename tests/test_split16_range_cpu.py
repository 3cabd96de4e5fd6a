"""Range control of the fp16 pair maps, host side: the exponent rule and the window test at their edges, the five _ex entry points
declared and bound, and the exact power-of-two reparameterisation the GPU tests load (tests/test_split16_range_gpu.py)."""
import math
import re

import numpy as np
import pytest
import torch

from gen6d_amd import lib, ops, synth


def reparam(sd, gains, prefix="backbone.features"):
    """A state dict with the same network function: the BatchNorm after VGG conv i scales its output by gains[i] (a power of two:
    gamma and beta times g), conv i + 1 takes weights / g.  ReLU and max-pool are positively homogeneous, every scaling is exact."""
    convs = sorted((int(k.split(".")[-2]) for k, v in sd.items() if k.startswith(prefix) and k.endswith(".weight") and v.dim() == 4))
    out = {k: v.clone() for k, v in sd.items()}
    for i, g in gains.items():
        assert math.frexp(g)[0] == 0.5, "power-of-two gains only"
        bn = f"{prefix}.{convs[i] + 1}"
        out[f"{bn}.weight"] *= g
        out[f"{bn}.bias"] *= g
        out[f"{prefix}.{convs[i + 1]}.weight"] /= g
    return out


def reparam_channels(sd, gains, prefix="backbone.features"):
    """reparam with a vector of power-of-two gains per layer: channel c of the BatchNorm after VGG conv i scales by gains[i][c] (gamma[c]
    and beta[c] times g[c]), conv i + 1 takes weight[:, c] / g[c].  ReLU and max-pool act per channel and are positively homogeneous, so
    every scaling is exact and the network function is unchanged."""
    convs = sorted((int(k.split(".")[-2]) for k, v in sd.items() if k.startswith(prefix) and k.endswith(".weight") and v.dim() == 4))
    out = {k: v.clone() for k, v in sd.items()}
    for i, g in gains.items():
        g = torch.as_tensor(g, dtype=torch.float32)
        assert bool((torch.frexp(g)[0] == 0.5).all()), "power-of-two gains only"
        bn = f"{prefix}.{convs[i] + 1}"
        assert g.shape == out[f"{bn}.weight"].shape
        out[f"{bn}.weight"] *= g
        out[f"{bn}.bias"] *= g
        out[f"{prefix}.{convs[i + 1]}.weight"] /= g.view(1, -1, 1, 1)
    return out


@pytest.mark.parametrize("a,e", [
    (0.0, 0), (2.0 ** -4, 0), (1.0, 0), (math.nextafter(2.0 ** 14, 0), 0),
    (2.0 ** 14, 14), (2.0 ** 20 * 1.5, 20), (math.nextafter(2.0 ** -4, 0), -5), (2.0 ** -12, -12), (3e-40, -100), (3e38, 100)])
def test_exponent_rule(a, e):
    assert ops.pair_exponent(a) == e
    if a:
        s = math.ldexp(a, -e)
        assert (2.0 ** -4 <= s < 2.0 ** 14) if e == 0 else (1.0 <= s < 2.0 or abs(e) == ops.PAIR_EXP_MAX)


def test_exponent_rule_nonfinite_keeps_exponent():
    for bits in (0x7F800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF & 0x7FFFFFFF):
        a = float(ops.bits_to_float([bits])[0])
        assert not math.isfinite(a)
        assert ops.pair_exponent(a, 7) == 7
        assert ops.pair_out_of_window(a, 0)


def test_window_edges():
    assert not ops.pair_out_of_window(0.0, 0)
    assert not ops.pair_out_of_window(2.0 ** -4, 0)
    assert ops.pair_out_of_window(math.nextafter(2.0 ** -4, 0), 0)
    assert not ops.pair_out_of_window(math.nextafter(2.0 ** 15, 0), 0)
    assert ops.pair_out_of_window(2.0 ** 15, 0)
    assert not ops.pair_out_of_window(2.0 ** 30, 20) and ops.pair_out_of_window(2.0 ** 35, 20)
    assert not ops.pair_out_of_window(2.0 ** -20, -20) and ops.pair_out_of_window(2.0 ** -25, -20)
    # the exponent the rule gives puts any finite non-zero record back into the window
    for a in (2.0 ** -30, 1e-3, 0.06, 7.0, 2.0 ** 14.5, 1e9):
        assert not ops.pair_out_of_window(a, ops.pair_exponent(a))


def test_bits_to_float():
    assert ops.bits_to_float([0x3F800000])[0] == 1.0
    assert ops.bits_to_float([-1 & 0x7FFFFFFF])[0] != ops.bits_to_float([-1 & 0x7FFFFFFF])[0]   # NaN


NEW = ["g6d_conv16_direct_multi_ex", "g6d_corr16_multi_ex", "g6d_product_split16_ex", "g6d_affine_split16_ex", "g6d_vgg_conv1_pool_nhwc16_ex"]


def test_ex_entry_points_declared_and_bound():
    import os
    text = open(os.path.join(os.path.dirname(lib.__file__), "..", "include", "gen6d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        base = name[:-3]
        # one extra argument, the G6dRange16 pointer, in front of the stream
        assert lib.SIGNATURES[name] == lib.SIGNATURES[base][:-1] + [lib.C.c_void_p, lib.C.c_void_p], name
        assert callable(getattr(lib.load(), name))
    assert re.search(r"typedef struct G6dRange16\s*\{[^}]*exps;[^}]*rec;[^}]*slot_in, slot_out;\s*\}", text)
    assert lib.C.sizeof(lib.G6dRange16) == 24


def test_pair_inputs_of_one_launch_share_a_slot():
    t = ops.RangeTable.__new__(ops.RangeTable)
    a, b = ops.PairMap(None, t, 0), ops.PairMap(None, t, 1)
    with pytest.raises(ValueError):
        ops._pair_inputs([a, b])
    with pytest.raises(ValueError):
        ops._pair_inputs([a, torch.zeros(1)])
    assert ops._pair_inputs([a, ops.PairMap(None, t, 0)])[1:] == (t, 0)


def test_reparameterised_detector_is_the_same_function():
    from oracle import gen6d_oracle as O
    sd = synth.synth_state_dict("detector")
    sd2 = reparam(sd, {2: 2.0 ** -10, 4: 2.0 ** 18})
    assert any(not torch.equal(sd[k], sd2[k]) for k in sd)
    case = synth.detector_case(4, 64, 96)
    with torch.no_grad():
        outs = [O.detector_detect(s, case["que_imgs"], O.detector_ref_feats(s, case["ref_imgs"])) for s in (sd, sd2)]
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        np.testing.assert_allclose(outs[1][k].numpy(), outs[0][k].numpy(), rtol=1e-6, atol=1e-6 * float(outs[0][k].abs().max()))
    assert torch.equal(outs[0]["que_select_id"], outs[1]["que_select_id"])
