"""The fp16 hi / lo pair format restated once, in float64 on the CPU (plain helper: no fixtures, no GPU).

  split      u -> hi = rn16(u), lo = rn16(u - hi), subnormals kept: the rule of csrc/pair16.h (c16_pair_split), of ref_ops._to_pairs and of
             ops._split_hi_lo
  delta      the a-priori bound of |u - (hi + lo)|: 2^-22 |u| while lo is a normal fp16 number, the subnormal grid's half step 2^-25 below
  emulate    the pair kernels' arithmetic WITHOUT rounding: the float64 convolutions hi.hi + hi.lo + lo.hi of split(x 2^-e) and split(w S),
             times 2^e / S, S = 2^ops.pair_filter_exponent(w) — what is left between it and a kernel is fp32 accumulation alone
  bound      the elementwise worst case of |emulate - the float64 convolution of the fp32 operands|
  spread_operands / exponents
             operands whose channel scales differ: channel c of x times top 2^-a[c], input channel c of w times 2^+a[c] / top, so every
             product is that of the uniform case while the map's small channels sink towards (and below) the lo plane's subnormal grid

Layout: x [N, H, W, Cin] or [N, D, H, W, Cin] channels-last, w [Cout, taps, Cin] with tap = ((kz) kh + ky) kw + kx, k = (kd, kh, kw)."""
import torch
import torch.nn.functional as F

PATTERNS = ("mixed", "slice", "outlier")
TOP_BOTTOM = 2.0 ** -4 * (1 + 2.0 ** -10)          # a map whose largest |v| sits just inside the bottom of the keep window [2^-4, 2^14)
OUTLIER = 13                                       # the channel that carries the map in the "outlier" pattern (inside an 8-vector)


def split(u):
    """float64 (hi, lo) with hi = rn16(u), lo = rn16(u - hi); fp16 subnormals kept."""
    u = torch.as_tensor(u).double()
    hi = u.to(torch.float16).double()
    lo = (u - hi).to(torch.float16).double()
    return hi, lo


def delta(u):
    """max(2^-22 |u|, 2^-25) >= |u - (hi + lo)|: |u - hi| <= 2^-11 |u| and the same again for lo while both are normal; the subnormal grid
    2^-24 rounds to within 2^-25."""
    return torch.clamp(torch.as_tensor(u).double().abs() * 2.0 ** -22, min=2.0 ** -25)


def exponents(pattern, Cin, A):
    """The per-channel exponents a[c] in 0..A of a pattern:
      mixed    a[c] = 5 c mod (A + 1): neighbours inside an 8-vector, a 16-channel k-step and a 32-channel slice all differ (where 5
               divides A + 1 — A = 4 — the stride is 3: with 5 every exponent would be 0)
      slice    the LAST 32-channel slice at A (its lo plane is subnormal or zero throughout), the rest at 0; a 32-channel map is that slice
      outlier  channel 13 at 0, all others at A: one channel carries the map's maximum"""
    c = torch.arange(Cin)
    if pattern == "mixed":
        return ((5 if (A + 1) % 5 else 3) * c) % (A + 1)
    if pattern == "slice":
        return torch.where(c >= Cin - 32, A, 0)
    if pattern == "outlier":
        return torch.where(c == OUTLIER % Cin, 0, A)
    raise ValueError(pattern)


def spread_operands(g, lead, Cin, Cout, taps, a, top=1.0, relu=True):
    """fp32 x [*lead, Cin], w [Cout, taps, Cin]: uniform(-1, 1) values (x after a ReLU if `relu`) with every channel of x normalised to a
    largest |value| of exactly 1, then channel c of x times top 2^-a[c] and input channel c of w times 2^a[c] / top; w carries the
    sqrt(3 / (taps Cin)) scale of the family's uniform cases.  The largest |x| is therefore top 2^-min(a) whatever the seed."""
    a = torch.as_tensor(a).double()
    x = (torch.rand((*lead, Cin), generator=g) * 2 - 1).double()
    if relu:
        x = x.clamp_min(0)
    x = x / x.abs().reshape(-1, Cin).amax(0)
    w = (torch.rand((Cout, taps, Cin), generator=g) * 2 - 1).double() * (3.0 / (taps * Cin)) ** 0.5
    return (x * (top * 2.0 ** -a)).float(), (w * (2.0 ** a / top)).float()


def _conv(x, w, k, stride, pad, bias=None):
    """float64 convolution, channels-last in and out."""
    x, w = x.double(), w.double()
    two_d = x.dim() == 4
    if two_d:
        x = x.unsqueeze(1)
    Cout, taps, Cin = w.shape
    assert taps == k[0] * k[1] * k[2]
    w5 = w.reshape(Cout, k[0], k[1], k[2], Cin).permute(0, 4, 1, 2, 3)
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w5, None if bias is None else bias.double(), stride=stride, padding=pad).permute(0, 2, 3, 4, 1)
    return (y[:, 0] if two_d else y).contiguous()


def _geom(k, stride, pad):
    k = (1, k, k) if isinstance(k, int) else tuple(k)
    stride = (1, 1, 1) if stride is None else ((1, stride, stride) if isinstance(stride, int) else tuple(stride))
    pad = tuple(i // 2 for i in k) if pad is None else ((0, pad, pad) if isinstance(pad, int) else tuple(pad))
    return k, stride, pad


def conv64(x, w, k=3, stride=None, pad=None, bias=None):
    """The float64 convolution of the fp32 operands themselves: the reference every pair test is held to.  k: an int (k x k, "same"
    padding by default: the 3x3 layers and the k x k correlation) or (kd, kh, kw)."""
    return _conv(x, w, *_geom(k, stride, pad), bias=bias)


def filter_scale(w):
    from gen6d_amd import ops
    return 2.0 ** ops.pair_filter_exponent(w)


def emulate(x, w, e=0, k=3, stride=None, pad=None, bias=None):
    """The pair kernels' arithmetic without rounding: (hi.hi + hi.lo + lo.hi) 2^e / S in float64 (+ bias)."""
    return emulate_pairs(*split(x.double() * 2.0 ** -e), w, e, k, stride, pad, bias)


def emulate_pairs(xh, xl, w, e=0, k=3, stride=None, pad=None, bias=None):
    """emulate on the planes (hi, lo) of a stored pair map of exponent e — a map some kernel wrote, read back."""
    k, stride, pad = _geom(k, stride, pad)
    S = filter_scale(w)
    wh, wl = split(w.double() * S)
    y = (_conv(xh, wh + wl, k, stride, pad) + _conv(xl, wh, k, stride, pad)) * (2.0 ** e / S)      # (the sum wh + wl is exact in float64)
    return y if bias is None else y + bias.double()


def bound(x, w, e=0, k=3, stride=None, pad=None):
    """Elementwise worst case of |emulate - conv64|.  With u = x 2^-e, v = w S and their pairs u', v':  u v - (u' v' - lo_u lo_v) =
    (u - u') v + u' (v - v') + lo_u lo_v, and |lo| <= 2^-11 |.|, so the three terms are conv(delta(u), |v|), conv(|u|, delta(v)) and
    2^-22 conv(|u|, |v|) (second-order terms aside), times 2^e / S."""
    k, stride, pad = _geom(k, stride, pad)
    S = filter_scale(w)
    u, v = x.double() * 2.0 ** -e, w.double() * S
    b = _conv(delta(u), v.abs(), k, stride, pad) + _conv(u.abs(), delta(v), k, stride, pad) + 2.0 ** -22 * _conv(u.abs(), v.abs(), k, stride, pad)
    return b * (2.0 ** e / S)


def high_exponent(amax):
    """The exponent that stores a map of largest |v| = amax with amax 2^-e in [2^12, 2^13): high in the window, every channel down to
    2^-12 of the map still has a normal lo plane."""
    import math
    return math.frexp(float(amax))[1] - 1 - 12


def mixed_gains(C, A, lift=1.0):
    """Per-channel power-of-two gains lift 2^-a[c] with the "mixed" exponents (for test_split16_range_cpu.reparam_channels)."""
    return (lift * 2.0 ** -exponents("mixed", C, A).double()).float()


def pairs_tensor(x, e=0):
    """fp32 x -> the fp16 pair map [..., 2, C] of x 2^-e as the kernels read it."""
    hi, lo = split(x.double() * 2.0 ** -e)
    return torch.stack([hi.to(torch.float16), lo.to(torch.float16)], -2).contiguous()
