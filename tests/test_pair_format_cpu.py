"""The fp16 hi / lo pair format where the channels of a map differ in scale, on the CPU (tests/pair_format.py):

  the restatement   pair_format.split is the split of ref_ops._to_pairs and of ops._split_hi_lo, bit for bit
  delta, bound      the a-priori bounds hold elementwise: delta across fp16's normal and subnormal range, bound for every pattern of
                    channel exponents, a spread of A = 0 / 4 / 8 / 12 binades and maps at the bottom, the middle and the trunk's level
                    of the keep window
  the envelope      the error of the FORMAT ALONE (no accumulation error) relative to the output range over (largest |v|, A), written to
                    the parity log; a map stored with its maximum in [2^12, 2^13) keeps the 2e-6 bar at A = 12
  reparametrisation reparam_channels (per-channel power-of-two gains on a BatchNorm, undone in the next conv) leaves the detector's
                    function unchanged through the oracle"""
import numpy as np
import pytest
import torch

import pair_format as pf
import ref_ops
from gen6d_amd import ops, synth
from parity_log import record
from test_split16_range_cpu import reparam_channels

BAR = 2e-6
LEAD, CIN, COUT = (2, 16, 16), 64, 128            # the envelope's case: 2 x 16 x 16 x 64 -> 128, 3 x 3, ReLU'd inputs
TOPS = [pf.TOP_BOTTOM, 1.0, 8.0]
SPREADS = [0, 4, 8, 12]


def _case(pattern, A, top, seed=3):
    g = torch.Generator().manual_seed(seed)
    return pf.spread_operands(g, LEAD, CIN, COUT, 9, pf.exponents(pattern, CIN, A), top=top, relu=True)


def test_split_is_the_projects_split():
    g = torch.Generator().manual_seed(1)
    mag = 2.0 ** torch.randint(-30, 16, (4096, 64), generator=g).double()
    v = ((torch.rand((4096, 64), generator=g) * 2 - 1).double() * mag).float()
    v[0, :8] = torch.tensor([0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 65504.0, -2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 1.0 + 2.0 ** -11])
    hi, lo = pf.split(v)
    want = ref_ops._to_pairs(v)
    assert torch.equal(hi.to(torch.float16).view(torch.int16), want[..., 0, :].view(torch.int16))
    assert torch.equal(lo.to(torch.float16).view(torch.int16), want[..., 1, :].view(torch.int16))
    assert torch.equal(hi, want[..., 0, :].double()) and torch.equal(lo, want[..., 1, :].double())
    assert torch.equal(pf.pairs_tensor(v).view(torch.int16), want.contiguous().view(torch.int16))
    # the filters: split of w S in float64, S from the filter exponent
    for scale in (1.0, 1e-3, 300.0):
        w = (torch.rand((128, 9, 64), generator=g) * 2 - 1) * scale * 2.0 ** pf.exponents("mixed", 64, 12).float()
        whi, wlo, inv = ops._split_hi_lo(w)
        S = pf.filter_scale(w)
        assert inv == 1.0 / S
        hi, lo = pf.split(w.double() * S)
        assert torch.equal(hi.to(torch.float16).view(torch.int16), whi.view(torch.int16))
        assert torch.equal(lo.to(torch.float16).view(torch.int16), wlo.view(torch.int16))
        assert bool(torch.isfinite(whi.float()).all())


def test_delta_holds_across_the_fp16_range():
    g = torch.Generator().manual_seed(2)
    ex = torch.randint(-40, 16, (1 << 18,), generator=g).double()
    u = (torch.rand(ex.shape, generator=g) * 2 - 1).double() * 2.0 ** ex
    u = torch.cat([u, 2.0 ** torch.arange(-40.0, 16.0).double(), 2.0 ** torch.arange(-40.0, 15.0).double() * (1 + 2.0 ** -11),
                   torch.tensor([0.0, 65504.0, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -3, 2.0 ** -3 * (1 - 2.0 ** -12)], dtype=torch.float64)])
    u = u.float().double()                                    # (fp32 values: what the kernels split)
    hi, lo = pf.split(u)
    err = (u - (hi + lo)).abs()
    assert bool((err <= pf.delta(u)).all()), float((err / pf.delta(u)).max())
    # below 2^-3 the lo plane sits on the subnormal grid: the floor is reached, whatever the value's size
    small = u.abs() < 2.0 ** -3
    assert float(err[small].max()) > 2.0 ** -26 and float(err[small].max()) <= 2.0 ** -25


@pytest.mark.parametrize("top", TOPS, ids=["bottom", "1", "8"])
@pytest.mark.parametrize("A", SPREADS)
@pytest.mark.parametrize("pattern", pf.PATTERNS)
def test_bound_holds(pattern, A, top):
    x, w = _case(pattern, A, top)
    assert float(x.abs().max()) == np.float32(top) and ops.pair_exponent(float(x.abs().max())) == 0
    diff = (pf.emulate(x, w) - pf.conv64(x, w)).abs()
    b = pf.bound(x, w)
    ratio = float((diff / b).max())
    print(f"{pattern} A={A} top={top:g}: worst |emulate - conv64| / bound {ratio:.3f}")
    assert bool((diff <= b).all()), ratio


def test_envelope():
    """The table of the profile: the format's own error / output range for the "mixed" pattern, by the map's largest |v| (e = 0) and A.
    Recorded, not bounded: the format loses the bar where its floor 2^(e-25) per activation is amplified by the small channels' large
    weights.  Asserted: what follows from the format — A = 0 keeps the bar in every row, and so does the top of the window."""
    rows = {}
    for top in TOPS + [2.0 ** 13]:
        for A in SPREADS:
            x, w = _case("mixed", A, top)
            ref = pf.conv64(x, w)
            err = float((pf.emulate(x, w) - ref).abs().max()) / float(ref.abs().max())
            f32 = float((torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.reshape(COUT, 3, 3, CIN).permute(0, 3, 1, 2), padding=1)
                         .permute(0, 2, 3, 1).double() - ref).abs().max()) / float(ref.abs().max())
            rows[top, A] = err
            record("test_envelope", f"format alone, mixed, max |v| = {top:g}, A = {A} (restatement - float64 / range)", err, BAR, f32,
                   note="recorded; ref_fp32_noise = a plain fp32 convolution of the same operands")
            print(f"max |v| {top:<12g} A {A:2d}: restatement {err:.2e}   plain fp32 conv {f32:.2e}")
    assert all(rows[top, 0] <= BAR for top in TOPS + [2.0 ** 13])
    assert all(rows[2.0 ** 13, A] <= BAR for A in SPREADS)
    # the blind spot itself, so that the table cannot silently go stale: the floor 2^-25 under weights 2^A / top is 2^(A-25) / top per
    # product against a range of order one — an order of magnitude past the bar in these two cells
    assert rows[pf.TOP_BOTTOM, 8] > BAR and rows[1.0, 12] > BAR


@pytest.mark.parametrize("top", TOPS, ids=["bottom", "1", "8"])
@pytest.mark.parametrize("pattern", pf.PATTERNS)
def test_high_in_the_window_keeps_the_bar(pattern, top):
    """Derived, not measured: with max |v| 2^-e in [2^12, 2^13) a channel 2^-12 below the map's maximum still peaks at >= 1, so delta is
    2^-22 relative for every activation above 2^-3 of its channel's peak and at most 2^-25 of that peak below.  The spread case then has
    the bound of the uniform case, 3 x 2^-22 conv(|u|, |w|) (+ 2^-25 per small activation), which the uniform cases meet with the margin
    test_bound_holds shows (a quarter of the bound at worst; conv(|u|, |w|) is 3 to 4 output ranges here, so the worst case itself is
    2.6e-6 and the restatement lies below 7e-7)."""
    x, w = _case(pattern, 12, top)
    e = pf.high_exponent(float(x.abs().max()))
    assert 2.0 ** 12 <= float(x.abs().max()) * 2.0 ** -e < 2.0 ** 13
    ref = pf.conv64(x, w)
    rng = float(ref.abs().max())
    err = float((pf.emulate(x, w, e) - ref).abs().max()) / rng
    worst = float(pf.bound(x, w, e).max()) / rng
    print(f"{pattern} top={top:g} e={e}: restatement {err:.2e}, bound {worst:.2e} of range; at e = 0: "
          f"{float((pf.emulate(x, w) - ref).abs().max()) / rng:.2e}")
    record("test_high_in_the_window_keeps_the_bar", f"format alone, {pattern}, A = 12, max |v| = {top:g} stored at e = {e}", err, BAR)
    assert err <= BAR


def test_reparameterised_channels_are_the_same_function():
    from oracle import gen6d_oracle as O
    sd = synth.synth_state_dict("detector")
    gains = {2: pf.mixed_gains(256, 12), 4: pf.mixed_gains(512, 12)}
    assert all(len(set(g.tolist())) == 13 for g in gains.values())
    sd2 = reparam_channels(sd, gains)
    changed = [k for k in sd if not torch.equal(sd[k], sd2[k])]
    assert len(changed) == 6, changed                         # gamma, beta and the next conv's weight, twice
    case = synth.detector_case(4, 64, 96)
    with torch.no_grad():
        outs = [O.detector_detect(s, case["que_imgs"], O.detector_ref_feats(s, case["ref_imgs"])) for s in (sd, sd2)]
    for k in ("scores", "select_pr_offset", "select_pr_scale"):
        np.testing.assert_allclose(outs[1][k].numpy(), outs[0][k].numpy(), rtol=1e-6, atol=1e-6 * float(outs[0][k].abs().max()))
    assert torch.equal(outs[0]["que_select_id"], outs[1]["que_select_id"])
