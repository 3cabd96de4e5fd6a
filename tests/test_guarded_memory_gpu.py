"""Every map kernel inside guarded arenas (tests/guarded.py): no entry point reads or writes outside its operands.

Each case runs ONE call twice.

  guarded run   every device-pointer operand sits in its own arena: NaN guards before, after and in the `ld - C` gap of every row, the base
                at 16 mod 256 bytes (16-byte aligned and no more), the loosest row strides the launcher accepts (`ld_in = Cin + 4` for fp32
                maps, `Cin + 8` for 16-bit ones, `ld_out = Cout + 8`; dense where the launcher demands dense).  Outputs are NaN in every
                element.  Asserted: (1) every output element is finite and none still holds the fill, (2) the output meets the bar of the
                entry's existing test against its float64 reference (the bar is quoted with file and test beside every case), (3) every
                guard of every arena holds the fill bit for bit.
  plain run     the same call, same values, same row strides, on plain torch allocations (512-byte aligned, zeros in the gaps).
                Asserted: (4) the outputs of the two runs are bit-identical.

(4) is not asserted where the result passes through floating-point atomics, whose order is not fixed — (2) alone holds there:
  * `stats` accumulators of conv_igemm (csrc/conv_igemm.hip:550,569-570: atomicAdd of the block's sums into the fp64 table), of the
    LDS-patch kernel (csrc/conv_patch.hip:330-331), of the Winograd kernels reached through ops.conv (csrc/wino_conv.hip:454,462,
    csrc/wino43_conv.hip:693,701, csrc/wino16_conv.hip:118,126) and of conv16_direct (csrc/conv16_common.h:206,230-231).  The MAP
    such a launch writes does not pass through them and is compared bit for bit.
No split launch adds its partials with atomics: the last block of a tile adds them in slice order (tests/test_kernels_gpu.py,
CONV_CASES "split launches finish inside the kernel"), so split cases are compared bit for bit too.

CASES is the table tests/test_guarded_cpu.py holds against gen6d_amd.lib.SIGNATURES: every entry point that takes map pointers is named
by at least one case here."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_ops
from guarded import arena, arena_numel

pytestmark = pytest.mark.gpu

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _d(t):
    return t.detach().cpu().double() if t is not None else None


def _bits(t):
    t = t.detach().contiguous()
    return t.view(_INT[t.element_size()])


SLAB_BYTES = 64 << 20


class Place:
    """Hands a case its device operands: arenas in the guarded run, plain torch allocations of the same strides in the plain run.  The
    operands of a run are cut from ONE allocation (operands above an eighth of it get their own): the multi-map launchers refuse maps that
    lie more than 2^29 floats apart (csrc/seg_table.h), which separate torch allocations of a long-lived process do.  Every arena keeps
    its own guards; a plain operand starts 512-byte aligned and sits among zeros."""

    def __init__(self, guarded):
        self.guarded, self.arenas, self.keep = guarded, [], []              # keep: no operand is freed (and its memory reused) before the launch
        self.slab, self.used = None, 0

    def _carve(self, numel, dtype):
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = numel * item
        start = (self.used + 511) // 512 * 512
        if nbytes > SLAB_BYTES // 8 or start + nbytes > SLAB_BYTES:
            return None
        if self.slab is None:
            self.slab = torch.empty(SLAB_BYTES, dtype=torch.uint8, device="cuda")
            assert self.slab.data_ptr() % 512 == 0
        self.used = start + nbytes
        return self.slab[start:start + nbytes].view(dtype)

    def _plain(self, shape, dtype, ld, values):
        shape = tuple(int(n) for n in shape)
        wide = shape if (ld is None or len(shape) < 2) else shape[:-1] + (int(ld),)
        numel = int(np.prod(wide))
        flat = self._carve(numel, dtype)
        flat = flat.zero_() if flat is not None else torch.zeros(numel, dtype=dtype, device="cuda")
        t = flat.view(wide)[..., :shape[-1]] if len(shape) >= 2 else flat
        if values is not None:
            t.copy_(values.to(dtype).reshape(shape))
        elif dtype.is_floating_point:
            t.fill_(float("nan"))
        self.keep.append(t)
        return t

    def _arena(self, shape, dtype, ld):
        return arena(shape, dtype, ld=ld, device="cuda", buf=self._carve(arena_numel(shape, dtype, ld=ld), dtype))

    def inp(self, values, ld=None, name="in"):
        """An input holding the CPU tensor `values` (None stays None)."""
        if values is None:
            return None
        if not self.guarded:
            return self._plain(values.shape, values.dtype, ld, values)
        a = self._arena(values.shape, values.dtype, ld)
        a.set(values)
        self.arenas.append((name, a, False))
        return a.view

    def out(self, shape, dtype=torch.float32, ld=None, name="out", init=None):
        """An output: NaN in every element, or — an operand the call updates or writes a part of — holding `init`."""
        if not self.guarded:
            return self._plain(shape, dtype, ld, init)
        a = self._arena(shape, dtype, ld)
        if init is not None:
            a.set(init)
        self.arenas.append((name, a, init is None))
        return a.view


class Case:
    def __init__(self, id, entries, fn, atomics=()):
        self.id, self.entries, self.fn, self.atomics = id, tuple(entries), fn, tuple(atomics)


CASES = []


def case(id, *entries, atomics=()):
    """Registers fn(P, knob) -> (outs, refs): outs {name: device tensor}; refs() -> {name: (float64 reference, bar) or check(got)}.
    atomics: names of the outputs that pass through floating-point atomics (module docstring)."""
    def deco(fn):
        CASES.append(Case(id, entries, fn, atomics))
        return fn
    return deco


def covered_entries():
    return {e for c in CASES for e in c.entries}


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def _ops():
    from gen6d_amd import ops
    return ops


def _call(name, *args):
    """The C entry point `name` with torch's stream appended."""
    from gen6d_amd import lib, ops
    lib.check(getattr(lib.load(), name)(*args, ops._stream()), name)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _ws():
    ws = _ops().workspace(torch.device("cuda", torch.cuda.current_device()))
    return _p(ws), ws.numel() * 4


# ================================================================================================ implicit GEMM (g6d_conv_igemm[_ex])
# Bars: tests/test_kernels_gpu.py::_run_conv_case (= tests/conv_case.py::run_conv_case) — 2e-5 rel-to-max for the map and both statistics (4e-5 on the Winograd kernel);
# tests/test_wino43_gpu.py::test_conv_on_wino43_kernel — 1e-5 map, 2e-5 statistics on the F(4x4,3x3) kernel.
def _conv(id, c, entries=("g6d_conv_igemm",), bar=2e-5, sbar=None, wino=None, label=None, hbm=None, knobs=(), mode=0):
    sbar = sbar if sbar is not None else bar

    @case(id, *entries, atomics=("stats",))
    def fn(P, knob):
        ops = _ops()
        for k_, v_ in knobs:
            knob(k_, v_)
        g = torch.Generator().manual_seed(17)
        N, D, H, W, Cin, Cout = c["N"], c.get("D", 1), c["H"], c["W"], c["Cin"], c["Cout"]
        k, s, p = c.get("k", (1, 3, 3)), c.get("s", (1, 1, 1)), c.get("p", (0, 1, 1))
        Do, Ho, Wo = [(i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((D, H, W), k, s, p)]
        per_n = int(c.get("per_n", 0))
        xc = _rand(g, N, D, H, W, Cin)
        T = k[0] * k[1] * k[2]
        wc = _rand(g, Cout, T, Cin, scale=(1.0 / (T * Cin)) ** 0.5)
        bc = _rand(g, Cout, scale=0.1)
        mulc = _rand(g, H, W, Cin) if c.get("mul") else None
        groups = (N + per_n - 1) // per_n if per_n else 1
        scc = (0.5 + torch.rand((groups, Cin), generator=g)) if c.get("aff") else None
        shc = _rand(g, groups, Cin, scale=0.3) if c.get("aff") else None
        M = N * Do * Ho * Wo
        rpg = c.get("rpg", 0)
        G = M // rpg if rpg else 1
        x = P.inp(xc, ld=c.get("ld_in", Cin + 4), name="x")
        w, bias, mul = P.inp(wc, name="w"), P.inp(bc, name="bias"), P.inp(mulc, name="mul")
        sc, sh = P.inp(scc, name="in_scale"), P.inp(shc, name="in_shift")
        out = P.out((N, Do, Ho, Wo, Cout), ld=c.get("ld_out", Cout + 8), name="out")
        stats = P.out((G, Cout, 2), torch.float64, name="stats", init=torch.zeros((G, Cout, 2), dtype=torch.float64)) if c.get("stats") else None
        extra = {}
        if wino == "f2":
            from gen6d_amd.network.backbone import winograd_filters_taps
            extra["w_wino"] = P.inp(winograd_filters_taps(wc, k[0]), name="w_wino")
        elif wino == "f4":
            from gen6d_amd.network.backbone import winograd43_filters_taps
            extra["w_wino43"] = P.inp(winograd43_filters_taps(wc, k[0]), name="w_wino43")
        ops.PROFILE, ops.PROFILE_HBM = [], {}
        try:
            with ops.math_mode(mode):
                ops.conv(x, w, bias, out, ksize=k, stride=s, pad=p, mul=mul, in_scale=sc, in_shift=sh, in_relu=bool(c.get("relu")), per_n=per_n,
                         out_act=c.get("act", 0), stats=stats, rows_per_group=rpg, split_k=c.get("split", 0), **extra)
            torch.cuda.synchronize()
            if label is not None:                                  # the route, as the existing test of that route asserts it
                assert ops.PROFILE and ops.PROFILE[0][3].startswith(label), f"route: {ops.PROFILE[0][3] if ops.PROFILE else None!r}, not {label!r}"
                assert label or not ops.PROFILE[0][3].startswith("wino"), f"route: {ops.PROFILE[0][3]!r}"
            if hbm is not None:
                assert (hbm in ops.PROFILE_HBM) and not ops.PROFILE, "the layer did not take the narrow-output kernel"
        finally:
            ops.PROFILE = ops.PROFILE_HBM = None

        def refs():
            ref = torch.empty((N, Do, Ho, Wo, Cout), dtype=torch.float64)
            rstats = torch.zeros((G, Cout, 2), dtype=torch.float64) if stats is not None else None
            ref_ops.conv(_d(xc), _d(wc), _d(bc), ref, ksize=k, stride=s, pad=p, mul=_d(mulc), in_scale=_d(scc), in_shift=_d(shc),
                         in_relu=bool(c.get("relu")), per_n=per_n, out_act=c.get("act", 0), stats=rstats, rows_per_group=rpg)
            r = {"out": (ref, bar)}
            if stats is not None:
                r["stats"] = lambda got: [_assert_rel(got[..., i], rstats[..., i], sbar, f"{id} stats[{i}]") for i in (0, 1)]
            return r
        o = {"out": out}
        if stats is not None:
            o["stats"] = stats
        return o, refs
    return fn


def _assert_rel(got, want, bar, what):
    err = _rel(got, want)
    print(f"GUARDED {what}: rel-to-max error {err:.3e} (bar {bar})")
    assert err <= bar, f"{what}: rel-to-max error {err:.3e} > {bar}"


_GEN = dict(N=2, H=9, W=13, Cin=40, Cout=40)             # M = 234: one full and one cut 128-row tile, the images straddle it; Cin = 32 + 8
_conv("igemm-generic", _GEN, label="")
_conv("igemm-generic-mul", dict(_GEN, mul=True, aff=True), label="")
_conv("igemm-generic-affine", dict(_GEN, aff=True, relu=True), label="")
_conv("igemm-generic-affine-per-image", dict(_GEN, aff=True, relu=True, per_n=1), label="")
_conv("igemm-generic-stats", dict(_GEN, stats=True, rpg=117), label="")
_conv("igemm-3d-stride2", dict(N=1, D=5, H=5, W=5, Cin=32, Cout=32, k=(3, 3, 3), s=(2, 2, 2), p=(1, 1, 1)), label="")
_conv("igemm-1x1", dict(N=3, H=1, W=1, Cin=64, Cout=64, k=(1, 1, 1), p=(0, 0, 0)), label="")
_conv("igemm-split5", dict(N=1, H=10, W=10, Cin=512, Cout=96, split=5, act=1), label="")
_conv("igemm-narrow-1", dict(N=2, H=5, W=8, Cin=64, Cout=1, act=1), hbm="conv_narrow", knobs=(("conv_narrow", 1),))
_conv("igemm-narrow-4", dict(N=3, H=9, W=13, Cin=192, Cout=4, ld_out=8), hbm="conv_narrow", knobs=(("conv_narrow", 1),))
_conv("igemm-position-major", dict(N=515, H=5, W=3, Cin=20, Cout=40, act=2), label="", knobs=(("conv_patch", 0), ("conv_pm", 2)))
_conv("igemm-lds-patch", dict(N=1, D=15, H=17, W=16, Cin=32, Cout=64, k=(3, 3, 3), p=(1, 1, 1)), label="")
# ops.conv(w_wino=...) / (w_wino43=...): tests/test_kernels_gpu.py::test_conv_on_winograd_kernel (knob wino_min_work = 0, bar 4e-5),
# tests/test_wino43_gpu.py::test_conv_on_wino43_kernel (every w43_map, bars 1e-5 / 2e-5)
_W3 = dict(N=2, D=5, H=9, W=11, Cin=16, Cout=64, k=(3, 3, 3), p=(1, 1, 1), act=1, stats=True, rpg=495)
_conv("conv-wino-f2-3d", _W3, bar=4e-5, wino="f2", label="wino3x3 conv", knobs=(("wino_min_work", 0),))
_conv("conv-wino-f2-2d-affine", dict(N=2, H=9, W=11, Cin=8, Cout=64, aff=True, relu=True, per_n=1), bar=4e-5, wino="f2", label="wino3x3 conv",
      knobs=(("wino_min_work", 0),))
for _m in (2, 1, 0):
    _conv(f"conv-wino-f4-map{_m}", _W3, bar=1e-5, sbar=2e-5, wino="f4", label="wino3x3 F43", knobs=(("w43_map", _m),))
_conv("conv-wino-f4-2d", dict(N=2, H=9, W=11, Cin=8, Cout=64, aff=True, relu=True), bar=1e-5, wino="f4", label="wino3x3 F43")


# 16-bit Winograd kernel through ops.conv in a reduced-precision mode: tests/test_lowp_gpu.py::test_conv_wino16_family, TOL = 2e-2 (bf16) /
# 3e-3 (fp16) of the output range (tests/test_lowp_gpu.py:16); the layer's 16-bit filters come from an arena as well
LOWP_TOL = {1: 2e-2, 2: 3e-3}
_T16 = {1: torch.bfloat16, 2: torch.float16, 3: torch.float16}


def _conv_wino16(id, mode, two_waves):
    @case(id, "g6d_conv_igemm")
    def fn(P, knob):
        from gen6d_amd.network.backbone import winograd_filters16_taps, winograd_filters_taps
        ops = _ops()
        knob("wino_min_work", 0)
        knob("wino16_2w", two_waves)
        g = torch.Generator().manual_seed(27)
        N, H, W, Cin, Cout = 2, 9, 11, 16, 64
        xc, wc, bc = _rand(g, N, 1, H, W, Cin), _rand(g, Cout, 9, Cin, scale=(1.0 / (9 * Cin)) ** 0.5 * 3), _rand(g, Cout, scale=0.2)
        x, w, bias = P.inp(xc, ld=Cin + 4, name="x"), P.inp(wc, name="w"), P.inp(bc, name="bias")
        # the fp32 Winograd pack holds ZEROS: the label "wino3x3 conv" is the fp32 kernel's too, and a fall-back to it would return the bias alone
        u = P.inp(torch.zeros_like(winograd_filters_taps(wc, 1)), name="w_wino")
        u.__dict__["_g6d_u16"] = {mode: P.inp(winograd_filters16_taps(wc, 1, _T16[mode]), name="w_wino16")}
        out = P.out((N, 1, H, W, Cout), ld=Cout + 8, name="out")
        ops.PROFILE = []
        try:
            with ops.math_mode(mode):
                ops.conv(x, w, bias, out, ksize=(1, 3, 3), pad=(0, 1, 1), w_wino=u)
            assert ops.PROFILE[0][3].startswith("wino3x3 conv"), ops.PROFILE[0][3]
        finally:
            ops.PROFILE = None

        def refs():
            ref = torch.empty((N, 1, H, W, Cout), dtype=torch.float64)
            ref_ops.conv(_d(xc), _d(wc), _d(bc), ref, ksize=(1, 3, 3), pad=(0, 1, 1))
            return {"out": (ref, LOWP_TOL[mode])}
        return {"out": out}, refs


for _mode, _nm in ((1, "bf16"), (2, "fp16")):
    for _tw in (1, 0):
        _conv_wino16(f"conv-wino16-{_nm}-2w{_tw}", _mode, _tw)


# ================================================================================================ Winograd trunk launchers, called directly
# Bars: tests/test_kernels_gpu.py::test_wino_conv3x3 / test_wino_conv3x3_multi 3e-5; tests/test_wino43_gpu.py::test_wino43_conv3x3_multi 1e-5;
# tests/test_lowp_gpu.py::test_wino16_conv3x3_multi TOL[mode] against float64 and 3e-4 against the restatement of the kernel's arithmetic.
def _wino_segs(P, xs_cpu, Cin, Cout, full, pool, ld_in, ld_out):
    from gen6d_amd import lib
    segs = (lib.G6dWinoSeg * len(xs_cpu))()
    ys, yps = [], []
    for i, xc in enumerate(xs_cpu):
        N, H, W = xc.shape[:3]
        x = P.inp(xc, ld=ld_in, name=f"x{i}")
        y = P.out((N, H, W, Cout), ld=ld_out, name=f"full{i}") if full else None              # every segment's output in its OWN arena
        yp = P.out((N, H // 2, W // 2, Cout), ld=ld_out, name=f"pool{i}") if pool else None
        ys.append(y); yps.append(yp)
        segs[i] = lib.G6dWinoSeg(in_=x.data_ptr(), out_full=y.data_ptr() if full else None, out_pool=yp.data_ptr() if pool else None, N=N, H=H, W=W,
                                 ld_in=ld_in, ld_full=ld_out if full else 0, ld_pool=ld_out if pool else 0)
    return segs, ys, yps


def _conv2d_refs(xs_cpu, w, b, relu, full, pool, bar):
    r = {}
    for i, xc in enumerate(xs_cpu):
        ref = F.conv2d(xc.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)
        if relu:
            ref = F.relu(ref)
        if full:
            r[f"full{i}"] = (ref.permute(0, 2, 3, 1), bar)
        if pool:
            r[f"pool{i}"] = (F.max_pool2d(ref, 2, 2).permute(0, 2, 3, 1), bar)
    return r


def _wino_trunk(id, entry, kind, sizes, Cin, Cout, relu=True, full=True, pool=True, knobs=(), seed=1000):
    @case(id, entry)
    def fn(P, knob):
        from gen6d_amd.network import backbone as B
        for k_, v_ in knobs:
            knob(k_, v_)
        g = torch.Generator().manual_seed(seed + Cin)
        w = _rand(g, Cout, Cin, 3, 3, scale=(2.0 / (9 * Cin)) ** 0.5 * 1.7)
        b = _rand(g, Cout, scale=0.3)
        xs_cpu = [_rand(g, n, h, ww, Cin) for n, h, ww in sizes]
        if kind in (1, 2):
            xs_cpu = [F.relu(x) for x in xs_cpu]
        ld_in, ld_out = Cin + 4, Cout + 8
        bias = P.inp(b, name="bias")
        wsp, wsb = _ws()
        if entry == "g6d_wino_conv3x3":
            xc = xs_cpu[0]
            N, H, W = xc.shape[:3]
            x, U = P.inp(xc, ld=ld_in, name="x"), P.inp(B.winograd_filters(w), name="U")
            y = P.out((N, H, W, Cout), ld=ld_out, name="full0") if full else None
            yp = P.out((N, H // 2, W // 2, Cout), ld=ld_out, name="pool0") if pool else None
            _call(entry, _p(x), N, H, W, Cin, ld_in, _p(U), _p(bias), Cout, int(relu), _p(y), ld_out, _p(yp), ld_out, wsp, wsb)
            ys, yps = [y], [yp]
        else:
            segs, ys, yps = _wino_segs(P, xs_cpu, Cin, Cout, full, pool, ld_in, ld_out)
            if kind == "f2":
                _call(entry, segs, len(sizes), Cin, _p(P.inp(B.winograd_filters(w), name="U")), _p(bias), Cout, int(relu), wsp, wsb)
            elif kind == "f4":
                _call(entry, segs, len(sizes), Cin, _p(P.inp(B.winograd43_filters(w), name="U43")), _p(bias), Cout, int(relu), wsp, wsb)
            else:
                U16 = B.winograd_filters16(w, _T16[kind])
                _call(entry, segs, len(sizes), Cin, _p(P.inp(U16, name="U16")), _p(bias), Cout, int(relu), kind, wsp, wsb)
        outs = {f"full{i}": y for i, y in enumerate(ys) if y is not None}
        outs.update({f"pool{i}": y for i, y in enumerate(yps) if y is not None})

        def refs():
            if kind not in (1, 2):
                return _conv2d_refs(xs_cpu, w, b, relu, full, pool, 3e-5 if kind == "f2" else 1e-5)
            r = _conv2d_refs(xs_cpu, w, b, relu, full, pool, LOWP_TOL[kind])
            rys, ryps = ref_ops.wino16_conv3x3_multi([x.double() for x in xs_cpu], B.winograd_filters16(w, _T16[kind]), b, relu=relu, full=full, pool=pool)

            def own(name, restated, rng):
                def check(got):
                    e64 = (got.cpu().double() - r[name][0]).abs().max().item() / rng
                    e = (got.cpu().double() - restated.double()).abs().max().item() / rng
                    print(f"GUARDED {id} {name}: {e64:.3e} of range against float64 (bar {LOWP_TOL[kind]}), {e:.3e} against the restatement (bar 3e-4)")
                    assert e64 <= LOWP_TOL[kind] and e <= 3e-4, (name, e64, e)
                return check
            res = {}
            for i in range(len(xs_cpu)):                          # (both errors are of the range of the full map, as in the existing test)
                ref = F.conv2d(xs_cpu[i].double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)
                rng = (F.relu(ref) if relu else ref).abs().max().item()
                if full:
                    res[f"full{i}"] = own(f"full{i}", rys[i], rng)
                if pool:
                    res[f"pool{i}"] = own(f"pool{i}", ryps[i], rng)
            return res
        return outs, refs


_wino_trunk("wino-single-full-pool", "g6d_wino_conv3x3", "f2", [(2, 9, 11)], 8, 64)
_MULTI = [(1, 9, 11), (2, 5, 6)]
_wino_trunk("wino-multi", "g6d_wino_conv3x3_multi", "f2", _MULTI, 8, 64)
for _wide in (0, 2):                                              # (block shapes: Cout % 128 == 0, tests/test_kernels_gpu.py:600-603)
    _wino_trunk(f"wino-multi-wide{_wide}", "g6d_wino_conv3x3_multi", "f2", _MULTI, 8, 128, knobs=(("wino_wide", _wide),))
_wino_trunk("wino43-multi", "g6d_wino43_conv3x3_multi", "f4", _MULTI, 8, 64, seed=4343)
for _mode, _nm in ((1, "bf16"), (2, "fp16")):
    for _tw in (1, 0):
        _wino_trunk(f"wino16-multi-{_nm}-2w{_tw}", "g6d_wino16_conv3x3_multi", _mode, [(2, 9, 11)], 16, 64, knobs=(("wino16_2w", _tw),), seed=300)


# ================================================================================================ correlations
# Bars: tests/test_kernels_gpu.py::test_corr2d_patch / test_corr2d_patch_multi 2e-5, ::test_corr2d_wino_multi 4e-5;
# tests/test_wino43_gpu.py::test_corr2d_wino43_multi(_7x7_on_9x9_blocks) 2e-5; tests/test_lowp_gpu.py::test_corr2d_patch16_multi 2e-5 against
# the correlation of the rounded operands and TOL[mode] against float64.
def _corr_ref(xc, w, k):
    ref = torch.empty(tuple(xc.shape[:-1]) + (w.shape[0],), dtype=torch.float64)
    ref_ops.corr2d_patch(_d(xc), _d(w), ref, k)
    return ref


def _corr_patch(id, H, W, Cin, Cout, k):
    @case(id, "g6d_corr2d_patch")
    def fn(P, knob):
        g = torch.Generator().manual_seed(21)
        xc, w = _rand(g, 1, 1, H, W, Cin), _rand(g, Cout, k * k, Cin, scale=(1.0 / (k * k * Cin)) ** 0.5)
        out = P.out((1, 1, H, W, Cout), ld=Cout + 8, name="out")
        _ops().corr2d_patch(P.inp(xc, ld=Cin + 4, name="x"), P.inp(w, name="w"), out, k)
        return {"out": out}, lambda: {"out": (_corr_ref(xc, w, k), 2e-5)}


_corr_patch("corr-patch-5x5-k3", 5, 5, 36, 3, 3)
_corr_patch("corr-patch-8x40-k15", 8, 40, 64, 8, 15)
_corr_patch("corr-patch-17x33-k7", 17, 33, 96, 32, 7)


def _corr_multi(id, entry, sizes, N, Cin, Cout, k, kind, bar, mode=0):
    """The G6dCorrSeg table is filled here and the C entry called directly: the ops wrappers take dense maps only for a batched or multi-map
    table (ops._corr_table), the launchers take ld_in >= Cin in multiples of 4 and ld_out >= Cout (csrc/seg_table.h:54-55)."""
    @case(id, entry)
    def fn(P, knob):
        from gen6d_amd import lib
        from gen6d_amd.network import backbone as B
        ops = _ops()
        g = torch.Generator().manual_seed(900 + Cin + k)
        w = _rand(g, Cout, k * k, Cin, scale=(1.0 / (k * k * Cin)) ** 0.5 * (3 if mode else 1))
        xs_cpu = [_rand(g, N, 1, h, ww, Cin) for h, ww in sizes]
        if mode:
            xs_cpu = [F.relu(x) for x in xs_cpu]
        ld_in, ld_out = Cin + 4, Cout + 8
        xs = [P.inp(x, ld=ld_in, name=f"x{i}") for i, x in enumerate(xs_cpu)]
        outs = [P.out((N, 1, h, ww, Cout), ld=ld_out, name=f"out{i}") for i, (h, ww) in enumerate(sizes)]
        segs = (lib.G6dCorrSeg * len(sizes))()
        for i, (h, ww) in enumerate(sizes):
            segs[i] = lib.G6dCorrSeg(in_=xs[i].data_ptr(), out=outs[i].data_ptr(), H=h, W=ww, ld_in=ld_in, ld_out=ld_out, N=N, reserved_=0)
        wsp, wsb = _ws()
        if kind == "patch":
            wd = P.inp(ops.corr_filters16(w, k, _T16[mode]), name="w16") if mode else P.inp(w, name="w")
            _call(entry, segs, len(sizes), Cin, _p(wd), Cout, k, k, wsp, wsb, mode)
        elif kind == "f2":
            _call(entry, segs, len(sizes), Cin, _p(P.inp(B.winograd_corr_filters(w, k), name="U")), Cout, 5, wsp, wsb)
        elif kind == "f4":
            _call(entry, segs, len(sizes), Cin, _p(P.inp(B.winograd43_corr_filters(w, k), name="U43")), Cout, 5, wsp, wsb)
        else:
            U, kb = B.winograd43_corr_filters_padded(w, k)
            assert kb == 3
            _call(entry, segs, len(sizes), Cin, _p(P.inp(U, name="U43")), Cout, 3, wsp, wsb)

        def refs():
            if not mode:
                return {f"out{i}": (_corr_ref(x, w, k), bar) for i, x in enumerate(xs_cpu)}
            dt = _T16[mode]
            w4 = w.double().reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)
            w4r = w.to(dt).double().reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)

            def check(x):
                def f(got):
                    xin = x[:, 0].permute(0, 3, 1, 2)
                    ref = F.conv2d(xin.double(), w4, padding=k // 2).permute(0, 2, 3, 1)
                    own = F.conv2d(xin.to(dt).double(), w4r, padding=k // 2).permute(0, 2, 3, 1)
                    gg, rng = got.cpu().double()[:, 0], ref.abs().max().item()
                    e_own, e_ref = (gg - own).abs().max().item() / rng, (gg - ref).abs().max().item() / rng
                    print(f"GUARDED {id}: {e_own:.3e} of range against the rounded operands (bar 2e-5), {e_ref:.3e} against float64 (bar {LOWP_TOL[mode]})")
                    assert e_own <= 2e-5 and e_ref <= LOWP_TOL[mode], (e_own, e_ref)
                return f
            return {f"out{i}": check(x) for i, x in enumerate(xs_cpu)}
        return {f"out{i}": o for i, o in enumerate(outs)}, refs


_SZ = [(22, 30), (9, 13)]
_corr_multi("corr-patch-multi-k7", "g6d_corr2d_patch_multi", [(17, 33), (8, 8)], 2, 96, 32, 7, "patch", 2e-5)
_corr_multi("corr-patch-multi-k3", "g6d_corr2d_patch_multi", [(5, 5), (9, 13)], 1, 36, 3, 3, "patch", 2e-5)
for _mode, _nm in ((1, "bf16"), (2, "fp16")):
    _corr_multi(f"corr-patch16-multi-{_nm}-k15", "g6d_corr2d_patch16_multi", [(8, 40), (9, 13)], 2, 64, 8, 15, "patch", None, mode=_mode)
    _corr_multi(f"corr-patch16-multi-{_nm}-k7", "g6d_corr2d_patch16_multi", [(17, 33)], 1, 96, 32, 7, "patch", None, mode=_mode)
_corr_multi("corr-wino-multi", "g6d_corr2d_wino_multi", _SZ, 3, 64, 32, 15, "f2", 4e-5)
_corr_multi("corr-wino43-multi-k15", "g6d_corr2d_wino43_multi", _SZ, 3, 64, 32, 15, "f4", 2e-5)
_corr_multi("corr-wino43-multi-k7", "g6d_corr2d_wino43_multi", _SZ, 3, 64, 32, 7, "f4pad", 2e-5)


# ================================================================================================ frequency-domain correlation
# Bars: tests/test_corr_fft_gpu.py — 8x the error of the fp32 numpy restatement (tests/corr_fft_ref.py) on the same data, of the float64
# result's range.  fwd and inv are called directly: the ops wrappers take dense maps only, the launchers take ld_in >= Cin, ld_out >= 32.
FFT_T, FFT_K, FFT_V, FFT_BINS = 32, 15, 18, 32 * 17


def _fft_check(id, what, ref, restated):
    def f(got):
        g = got.cpu().numpy().astype(np.float64).reshape(ref.shape)
        err = float(np.abs(g - ref).max() / np.abs(ref).max())
        print(f"GUARDED {id} {what}: {err:.3e} of range, fp32 restatement {restated:.3e}, bar {8 * restated:.3e}")
        assert err <= 8 * restated, (err, restated)
    return f


@case("corr-fft-fwd", "g6d_corr_fft_fwd")
def _fft_fwd(P, knob):
    import corr_fft_ref as R
    from gen6d_amd import lib
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    N, H, W, Cin = 2, 19, 37, 64
    xc = torch.relu(_rand(g, N, H, W, Cin))
    plan = ops.corr_fft_plan([(N, H, W)], Cin)
    x = P.inp(xc, ld=68, name="x")
    X = P.out((plan["spectrum_bytes"] // 4,), name="X")
    assert X.numel() == FFT_BINS * plan["tiles"] * 2 * Cin
    segs = (lib.G6dCorrSeg * 1)(lib.G6dCorrSeg(in_=x.data_ptr(), out=None, H=H, W=W, ld_in=68, ld_out=32, N=N, reserved_=0))
    _call("g6d_corr_fft_fwd", segs, 1, Cin, FFT_K, FFT_T, _p(X))

    def refs():
        win = np.concatenate([R.windows(img.numpy().astype(np.float64), FFT_T, FFT_K) for img in xc])
        f = np.fft.rfft2(win, axes=(1, 2))
        ref = np.stack([f.real, f.imag], 0).transpose(2, 3, 1, 0, 4).reshape(FFT_BINS, plan["tiles"], 2, Cin)
        restated = float(np.abs(np.asarray(R.forward(win.astype(np.float32)), np.float64) - ref).max() / np.abs(ref).max())
        return {"X": _fft_check("corr-fft-fwd", "spectrum", ref, restated)}
    return {"X": X}, refs


def _fft_gemm(id, Cin):
    @case(id, "g6d_corr_fft_gemm")
    def fn(P, knob):
        import corr_fft_ref as R
        g = torch.Generator().manual_seed(4)
        M = 150
        Xc, Bc = _rand(g, FFT_BINS, M, 2 * Cin), _rand(g, FFT_BINS, 2 * Cin, 64)
        Y = P.out((FFT_BINS * M * 64,), name="Y")
        _ops().corr_fft_gemm(P.inp(Xc.reshape(-1), name="X"), P.inp(Bc.reshape(-1), name="B"), Y, M, Cin)

        def refs():
            ref = np.einsum("bmk,bkn->bmn", Xc.numpy().astype(np.float64), Bc.numpy().astype(np.float64))
            rest = R.gemm(Xc.numpy().reshape(FFT_BINS, M, 2, Cin), Bc.numpy())
            restated = float(np.abs(np.asarray(rest, np.float64) - ref).max() / np.abs(ref).max())
            return {"Y": _fft_check(id, "product", ref, restated)}
        return {"Y": Y}, refs


_fft_gemm("corr-fft-gemm-cin32", 32)
_fft_gemm("corr-fft-gemm-cin64", 64)


@case("corr-fft-inv", "g6d_corr_fft_inv")
def _fft_inv(P, knob):
    import corr_fft_ref as R
    from gen6d_amd import lib
    rng = np.random.default_rng(5)
    N, H, W = 2, 19, 37
    nt = N * 2 * 3
    tiles = rng.standard_normal((nt, FFT_T, FFT_T, 32))
    f = np.fft.rfft2(tiles, axes=(1, 2))
    Y32 = np.stack([f.real, f.imag], 0).transpose(2, 3, 1, 0, 4).reshape(FFT_BINS, nt, 64).astype(np.float32)
    Y = P.inp(torch.from_numpy(Y32).reshape(-1), name="Y")
    out = P.out((N, H, W, 32), ld=40, name="out")
    segs = (lib.G6dCorrSeg * 1)(lib.G6dCorrSeg(in_=None, out=out.data_ptr(), H=H, W=W, ld_in=32, ld_out=40, N=N, reserved_=0))
    _call("g6d_corr_fft_inv", segs, 1, 32, FFT_K, FFT_T, _p(Y))

    def refs():
        y = Y32.astype(np.float64).reshape(FFT_T, 17, nt, 2, 32)
        corner = np.fft.irfft2(y[:, :, :, 0] + 1j * y[:, :, :, 1], s=(FFT_T, FFT_T), axes=(0, 1)).transpose(2, 0, 1, 3)[:, :FFT_V, :FFT_V]
        ref = np.stack([R.scatter(corner[n * 6:(n + 1) * 6], H, W, FFT_T, FFT_K) for n in range(N)])
        rest = R.inverse(Y32, FFT_T, FFT_V)
        rs = np.stack([R.scatter(rest[n * 6:(n + 1) * 6], H, W, FFT_T, FFT_K) for n in range(N)])
        restated = float(np.abs(np.asarray(rs, np.float64) - ref).max() / np.abs(ref).max())
        return {"out": _fft_check("corr-fft-inv", "maps", ref, restated)}
    return {"out": out}, refs


# ================================================================================================ conv_igemm on fp16 hi / lo pairs
# g6d_conv_igemm_ex, variants 3 / 4 / 5 (tests/test_conv_igemm_presplit_gpu.py: cases "1x1-40rows" and "s2", BAR = 2e-6 of the output range for
# the map and the sums, tests/test_conv_igemm_pairs_gpu.py:15).  The pre-split filter pack of variants 4 / 5 and the pair map of variant 5
# come from arenas; the range table (64 int32 exponents and records, ops.RangeTable) is the library's own allocation.
PAIR_BAR = 2e-6


def _split(x):
    hi = x.to(torch.float16)
    return torch.stack([hi, (x - hi.float()).to(torch.float16)], -2).contiguous()


def _igemm_pairs(id, name, variant, wide=False):
    @case(id, "g6d_conv_igemm_ex", atomics=("stats",))
    def fn(P, knob):
        from test_conv_igemm_presplit_gpu import _case
        ops = _ops()
        c = _case(name)
        xc, wc, bc = c["x"], c["w"], c["b"]
        N, D, H, W, Cin = xc.shape
        Cout = wc.shape[0]
        Do, Ho, Wo = [(i + 2 * p - kk) // s + 1 for i, p, kk, s in zip((D, H, W), c["pad"], c["k"], c["stride"])]
        t = ops.RangeTable(torch.device("cuda", 0))
        w = P.inp(wc, name="w")
        e = ops.pair_filter_exponent(wc)
        w.__dict__["_g6d_w_exp"] = e
        if variant >= 4:
            u = wc.double() * 2.0 ** e
            hi = u.to(torch.float16)
            lo = (u - hi.double()).to(torch.float16)
            pk = torch.stack([hi.view(Cout, -1, Cin // 32, 32), lo.view(Cout, -1, Cin // 32, 32)], 3).contiguous()
            w.__dict__["_g6d_w_pairs"] = (e, P.inp(pk, name="w_pairs"))
        if variant == 5 and wide:                                 # channels [8, 8 + Cin) of a pair map 16 channels wider: ld_in = 2 (Cin + 16), the lo
            Ct = Cin + 16                                         # plane ld_in / 2 on (include/gen6d_hip.h:113-116); the other channels hold 1000
            m = torch.full((N, D, H, W, 2, Ct), 1000.0, dtype=torch.float16)
            m[..., 8:8 + Cin] = _split(xc)
            x16 = P.inp(m.reshape(N, D, H, W, 2 * Ct), name="x16").view(N, D, H, W, 2, Ct)[..., 8:8 + Cin]
            x = ops.PairMap(x16, t, t.slot("a"))
        elif variant == 5:                                        # a pair map some producer wrote: exponent 0, rows of both planes
            x16 = P.inp(_split(xc).reshape(N, D, H, W, 2 * Cin), name="x16").view(N, D, H, W, 2, Cin)
            x = ops.PairMap(x16, t, t.slot("a"))
        else:
            x = P.inp(xc, ld=Cin + 4, name="x")
        out = P.out((N, Do, Ho, Wo, Cout), ld=Cout + 8, name="out")
        G = c.get("groups", 0)
        stats = P.out((G, Cout, 2), torch.float64, name="stats", init=torch.zeros((G, Cout, 2), dtype=torch.float64)) if G else None
        ops.PROFILE = []
        try:
            ops.conv(x, w, P.inp(bc, name="bias"), out, ksize=c["k"], stride=c["stride"], pad=c["pad"], stats=stats, rows_per_group=c.get("rows", 0),
                     pairs=(t, t.slot("a"), variant))
            assert ops.PROFILE[-1][3].startswith("conv16x3 igemm"), ops.PROFILE[-1][3]
        finally:
            ops.PROFILE = None

        def refs():
            from test_conv_igemm_presplit_gpu import _ref
            _, ref, _ = _ref(name)
            rng = float(ref.abs().max())
            r = {"out": (ref, PAIR_BAR)}
            if G:
                def sums(got):
                    rows = c["rows"]
                    r3 = ref.reshape(G, rows, Cout)
                    e1 = float((got.cpu()[:, :, 0] - r3.sum(1)).abs().max()) / rows / rng
                    e2 = float((got.cpu()[:, :, 1] - (r3 * r3).sum(1)).abs().max()) / rows / rng ** 2
                    print(f"GUARDED {id} sums {e1:.3e}, squares {e2:.3e} (bar {PAIR_BAR})")
                    assert e1 <= PAIR_BAR and e2 <= PAIR_BAR, (e1, e2)
                r["stats"] = sums
            return r
        o = {"out": out}
        if G:
            o["stats"] = stats
        return o, refs


for _v in (3, 4, 5):
    _igemm_pairs(f"igemm-pairs-v{_v}-1x1", "1x1-40rows", _v)
    _igemm_pairs(f"igemm-pairs-v{_v}-3d-stride2", "s2", _v)
_igemm_pairs("igemm-pairs-v5-1x1-slice", "1x1-40rows", 5, wide=True)
_igemm_pairs("igemm-pairs-v5-3d-stride2-slice", "s2", 5, wide=True)


# ================================================================================================ 16-bit direct convolution, correlation, first layer
# g6d_conv16_direct_multi_ex: tests/test_conv16w_edges_gpu.py (halo-patch, two-tile Cout = 64, statistics; bars 2e-6 of range for pairs + 2^-21
# for a pair output, 2e-5 + half an ulp for the 16-bit modes), tests/test_conv16w_depth_gpu.py (depth-folded, BAR = 2e-6), tests/test_conv16_gpu.py
# (per-tap kernels under knob conv16_halo = 0, same bars).  The inputs, the filter pack and the bias now sit in arenas as well; the launcher takes
# ld_in >= Cin (pairs: 2 Cin) in multiples of 8 (csrc/conv16_direct.hip:59-64): ld_in = that + 8, outputs ld = width + 8.
ULP16 = {1: 2.0 ** -8, 2: 2.0 ** -11, 3: 2.0 ** -21}


def _conv16(id, segs, Cin, Cout, mode=3, full="f32", pool=None, relu=True, gi=0, halo=1, kd=1, layout=1):
    @case(id, "g6d_conv16_direct_multi_ex", atomics=("stats",))
    def fn(P, knob):
        from gen6d_amd import lib
        ops = _ops()
        knob("conv16_halo", halo)
        pair = mode == 3
        g = torch.Generator().manual_seed(11 + Cin + 5 * len(segs) + segs[0][0])
        taps = 9 * kd
        wc = _rand(g, Cout, taps, Cin, scale=(1.0 / (taps * Cin)) ** 0.5 * 3)
        bc = _rand(g, Cout, scale=0.2)
        xs = [_rand(g, *s, Cin) for s in segs]
        if kd == 3:
            xs = [x * (1.0 + torch.arange(x.shape[0]).view(-1, 1, 1, 1, 1)) for x in xs]
        if not pair:
            wc, xs = wc.to(_T16[mode]).float(), [x.to(_T16[mode]).float() for x in xs]
        filt = ops.conv16_pack(wc, mode, layout)
        if kd == 3 and layout == 2:
            N0, D0, H0, W0 = segs[0]
            assert ops.conv16_direct_plan(N0, H0, W0, Cin, Cout, 3, stats_rows=D0 * H0 * W0 if gi else 0, D=D0) == 1, "not the halo-patch kernel"
        elif kd == 1 and halo and full is not None:
            plan = ops.conv16_direct_plan(*segs[0], Cin, Cout, mode, stats_rows=gi * segs[0][1] * segs[0][2] if gi else 0,
                                          full=torch.float32 if full == "f32" else "t16")
            assert plan in (1, 2), f"plan {plan}: not the halo-patch kernel"
        fdata, bias = P.inp(filt.data, name="filters"), P.inp(bc, name="bias")
        code = {None: 0, "t16": 3 if pair else 1, "f32": 2}
        st = lib.G6dConv16Seg * len(xs)
        sg = st()
        outs = {}
        stats, rpg = None, 0
        if gi:
            s0 = segs[0]
            px = s0[1] * s0[2] * (s0[3] if kd == 3 else 1)
            G = s0[0] // gi
            stats = P.out((G, Cout, 2), torch.float64, name="stats", init=torch.zeros((G, Cout, 2), dtype=torch.float64))
            rpg = gi * px
            outs["stats"] = stats
        for i, xc in enumerate(xs):
            lead = tuple(xc.shape[:-1])
            N, D, H, W = (lead[0], 1, lead[1], lead[2]) if kd == 1 else lead
            x16 = _split(xc).reshape(lead + (2 * Cin,)) if pair else xc.to(_T16[mode])
            ld_in = (2 if pair else 1) * Cin + 8
            x = P.inp(x16, ld=ld_in, name=f"x{i}")

            def make(kind, ld_lead, nm):
                if kind is None:
                    return None, 0
                width = Cout * (2 if pair and kind == "t16" else 1)
                t = P.out(ld_lead + (width,), _T16[mode] if kind == "t16" else torch.float32, ld=width + 8, name=nm)
                outs[nm] = t
                return t, width + 8
            f, ldf = make(full, lead, f"full{i}")
            q, ldq = make(pool, (N, H // 2, W // 2), f"pool{i}")
            sg[i] = lib.G6dConv16Seg(in_=x.data_ptr(), out_full=f.data_ptr() if f is not None else None, out_pool=q.data_ptr() if q is not None else None,
                                     N=N, D=D, H=H, W=W, ld_in=ld_in, ld_full=ldf, ld_pool=ldq)
        _call("g6d_conv16_direct_multi_ex", sg, len(xs), Cin, _p(fdata), int(filt.layout), float(filt.acc_scale), _p(bias), Cout, kd, int(relu),
              code[full], code[pool], mode, _p(stats), int(rpg), None)

        def refs():
            base = 2e-6 if pair else 2e-5
            r = {}
            for i, xc in enumerate(xs):
                if kd == 1:
                    w4 = wc.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
                    ref = F.conv2d(xc.double().permute(0, 3, 1, 2), w4, bc.double(), padding=1).permute(0, 2, 3, 1)
                else:
                    w5 = wc.double().reshape(Cout, 3, 3, 3, Cin).permute(0, 4, 1, 2, 3)
                    ref = F.conv3d(xc.double().permute(0, 4, 1, 2, 3), w5, bc.double(), padding=1).permute(0, 2, 3, 4, 1)
                if relu:
                    ref = F.relu(ref)
                rng = float(ref.abs().max())
                if gi and i == 0:
                    G = stats.shape[0]
                    n = ref.numel() / (G * Cout)

                    def sums(got, ref=ref, rng=rng, n=n, G=G):
                        e1 = float((got.cpu()[:, :, 0] - ref.reshape(G, -1, Cout).sum(1)).abs().max()) / n / rng
                        e2 = float((got.cpu()[:, :, 1] - (ref * ref).reshape(G, -1, Cout).sum(1)).abs().max()) / n / rng ** 2
                        print(f"GUARDED {id} statistics {e1:.3e} (bar {base}), squares {e2:.3e} (bar {2 * base})")
                        assert e1 <= base and e2 <= 2 * base, (e1, e2)
                    r["stats"] = sums

                def chk(kind, want, nm, rng=rng):
                    tol = base + (ULP16[mode] if kind == "t16" else 0.0)

                    def f(got):
                        m = got.cpu().double()
                        val = m[..., :Cout] + m[..., Cout:] if (pair and kind == "t16") else m
                        e = float((val - want).abs().max()) / rng
                        print(f"GUARDED {id} {nm}: error / range {e:.3e} (bar {tol:.3e})")
                        assert e <= tol, (nm, e, tol)
                    return f
                if full is not None:
                    r[f"full{i}"] = chk(full, ref, f"full{i}")
                if pool is not None:
                    r[f"pool{i}"] = chk(pool, F.max_pool2d(ref.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), f"pool{i}")
            return r
        return outs, refs


_conv16("conv16-halo-overhang-pool", [(2, 22, 30)], 64, 128, full="f32", pool="t16")                  # test_conv16w_edges_gpu "overhang-pool"
_conv16("conv16-halo-two-tile-odd", [(5, 8, 8)], 64, 64, relu=False)                                 # "banded8-odd-partial"
_conv16("conv16-halo-two-tile-stats", [(6, 8, 8)], 64, 64, relu=False, gi=2)                          # "banded8-odd-stats"
_conv16("conv16-halo-banded4", [(17, 4, 4)], 64, 64, relu=False)                                     # "banded4-partial"
_conv16("conv16-halo-fp16-pool-stats", [(2, 24, 30)], 64, 128, mode=2, full=None, pool="t16", gi=1)  # "fp16-pool-stats"
_conv16("conv16-halo-bf16", [(3, 16, 24)], 64, 256, mode=1, full="t16", pool="t16", gi=1)            # "bf16-pool-full-stats"
_conv16("conv16-depth-folded", [(2, 2, 18, 20)], 32, 64, relu=False, gi=1, kd=3, layout=2)           # test_conv16w_depth_gpu D2-18x20-32to64
_conv16("conv16-depth-folded-pairs-out", [(2, 3, 16, 24)], 32, 128, relu=False, full="t16", kd=3, layout=2)
_conv16("conv16-per-tap-pairs", [(3, 6, 10), (3, 4, 4)], 64, 128, full="f32", pool="t16", halo=0)    # test_conv16_gpu cases 1 / 4, per-tap kernels
_conv16("conv16-per-tap-fp16", [(2, 6, 36)], 64, 128, mode=2, full="t16", pool="f32", halo=0)
_conv16("conv16-per-tap-3d", [(2, 8, 8, 8)], 64, 128, relu=False, gi=1, kd=3, halo=0)                # test_conv16_gpu case 8


# g6d_corr16_multi_ex, the table filled here (ops.corr16_multi takes dense maps only; the launcher takes ld_in >= Cin (pairs: 2 Cin) in multiples
# of 8 and ld_full >= 32, csrc/corr16.hip:243-244): tests/test_conv16_gpu.py::test_corr16_multi, bar 2e-6 of range for pairs, 2e-5 for the 16-bit modes
def _corr16(id, N, sizes, Cin, k, mode):
    @case(id, "g6d_corr16_multi_ex")
    def fn(P, knob):
        from gen6d_amd import lib
        ops = _ops()
        pair = mode == 3
        g = torch.Generator().manual_seed(77 + Cin + k)
        wc = _rand(g, 32, k * k, Cin, scale=(3.0 / (k * k * Cin)) ** 0.5)
        xs = [_rand(g, N, h, ww, Cin) for h, ww in sizes]
        if not pair:
            wc, xs = wc.to(_T16[mode]).float(), [x.to(_T16[mode]).float() for x in xs]
        filt = ops.corr16_pack(wc, mode)
        fdata = P.inp(filt.data, name="filters")
        ld_in, ld_out = (2 if pair else 1) * Cin + 8, 40
        segs = (lib.G6dConv16Seg * len(sizes))()
        outs = []
        for i, (x, (h, ww)) in enumerate(zip(xs, sizes)):
            x16 = P.inp(_split(x).reshape(N, h, ww, 2 * Cin) if pair else x.to(_T16[mode]), ld=ld_in, name=f"x{i}")
            outs.append(P.out((N, 1, h, ww, 32), ld=ld_out, name=f"out{i}"))
            segs[i] = lib.G6dConv16Seg(in_=x16.data_ptr(), out_full=outs[i].data_ptr(), out_pool=None, N=N, D=1, H=h, W=ww, ld_in=ld_in, ld_full=ld_out, ld_pool=0)
        _call("g6d_corr16_multi_ex", segs, len(sizes), Cin, _p(fdata), float(filt.acc_scale), 32, k, mode, None)

        def refs():
            w4 = wc.double().reshape(32, k, k, Cin).permute(0, 3, 1, 2)
            return {f"out{i}": (F.conv2d(x.double().permute(0, 3, 1, 2), w4, None, padding=k // 2).permute(0, 2, 3, 1).unsqueeze(1), 2e-6 if pair else 2e-5)
                    for i, x in enumerate(xs)}
        return {f"out{i}": o for i, o in enumerate(outs)}, refs


_corr16("corr16-pairs-k15", 3, [(22, 30), (9, 13)], 64, 15, 3)
_corr16("corr16-pairs-k7", 2, [(3, 31), (7, 15), (15, 7), (31, 3)], 96, 7, 3)
_corr16("corr16-fp16-k15", 2, [(9, 13), (15, 7)], 96, 15, 2)
_corr16("corr16-bf16-k7", 2, [(11, 15)], 128, 7, 1)


# g6d_vgg_conv1_pool_nhwc16_ex: tests/test_conv16_gpu.py::test_vgg_conv1_pool_nhwc16 — the fp32 kernel's result rounded (pairs: split) once, bit
# for bit; here against the float64 layer at that kernel's bar (1e-5, tests/test_kernels_gpu.py::test_vgg_conv1_pool_nhwc) plus the format's step
def _conv1_16(id, mode):
    @case(id, "g6d_vgg_conv1_pool_nhwc16_ex")
    def fn(P, knob):
        g = torch.Generator().manual_seed(5)
        N, H, W = 2, 33, 67
        xc, wc, bc = torch.rand((N, 3, H, W), generator=g), _rand(g, 64, 3, 3, 3, scale=0.3), _rand(g, 64, scale=0.1)
        mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        width = 128 if mode == 3 else 64
        out = P.out((N, H // 2, W // 2, width), _T16[mode], name="out")
        _call("g6d_vgg_conv1_pool_nhwc16_ex", _p(P.inp(xc, name="x")), N, H, W, _p(P.inp(wc, name="w")), _p(P.inp(bc, name="bias")), 3, 64,
              (C.c_float * 3)(*mean), (C.c_float * 3)(*std), _p(out), mode, None)

        def refs():
            xn = (xc.double() - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
            ref = F.max_pool2d(F.relu(F.conv2d(xn, wc.double(), bc.double(), padding=1)), 2, 2).permute(0, 2, 3, 1)

            def f(got):
                m = got.cpu().double()
                val = m[..., :64] + m[..., 64:] if mode == 3 else m
                e = _rel(val, ref)
                print(f"GUARDED {id}: rel-to-max error {e:.3e} (bar {1e-5 + ULP16[mode]:.3e})")
                assert e <= 1e-5 + ULP16[mode], e
            return {"out": f}
        return {"out": out}, refs


for _mode, _nm in ((3, "pairs"), (2, "fp16"), (1, "bf16")):
    _conv1_16(f"vgg-conv1-nhwc16-{_nm}", _mode)


# ================================================================================================ pair producers (csrc/split16.hip)
# Bars: hi + lo within 2^-21 of the map's range (pairs), half an fp16 ulp 2^-11 (mode 2): tests/test_pair_handover_gpu.py:66; against the float64
# reference of the fp32 kernel each repeats, whose own bar (1e-6, tests/test_glue_edges_gpu.py) is added.  Slice producers write channels
# [8, 8 + C) of a map 8 channels wider on both sides: the whole wider row is the operand (a pair map's row holds both planes), it starts out
# holding a finite pattern, and every element outside the slice must still hold it.
SLICE_FILL = 1000.0


def _slice_map(P, pixels_shape, Cc, mode, name="out"):
    Ct = Cc + 16
    width = 2 * Ct if mode == 3 else Ct
    init = torch.full(tuple(pixels_shape) + (width,), SLICE_FILL, dtype=_T16[mode])
    return P.out(tuple(pixels_shape) + (width,), _T16[mode], name=name, init=init), Ct, width


def _slice_check(id, Cc, Ct, mode, want, fp32_bar):
    bar = fp32_bar + (2.0 ** -21 if mode == 3 else 2.0 ** -11)

    def f(got):
        m = got.cpu().double().reshape(-1, 2 if mode == 3 else 1, Ct)
        val = m[:, :, 8:8 + Cc].sum(1)
        e = _rel(val, want.reshape(-1, Cc))
        print(f"GUARDED {id}: rel-to-max error {e:.3e} (bar {bar:.3e})")
        assert e <= bar, e
        rest = m.clone()
        rest[:, :, 8:8 + Cc] = SLICE_FILL
        assert bool((rest == SLICE_FILL).all()), f"{id}: wrote outside its channel slice"
    return f


def _affine_to(id, mode):
    @case(id, "g6d_affine_split16_to")
    def fn(P, knob):
        N, H, W, Cc = 3, 4, 4, 64
        g = torch.Generator().manual_seed(17)
        xc = _rand(g, N, 1, H, W, Cc, scale=2.0)
        scc, shc = _rand(g, N, Cc) * 0.2 + 0.3, _rand(g, N, Cc, scale=0.2)
        out, Ct, width = _slice_map(P, (N, H, W), Cc, mode)
        _call("g6d_affine_split16_to", _p(P.inp(xc, ld=Cc + 4, name="x")), Cc + 4, _p(P.inp(scc, name="scale")), _p(P.inp(shc, name="shift")), 1, 0, 0,
              N, H, W, Cc, _p(out), width, Ct, 8, mode, None)

        def refs():
            want = torch.empty((N, 1, H, W, Cc), dtype=torch.float64)
            ref_ops.affine_act_pool(_d(xc), want, _d(scc), _d(shc), per_n=True)
            return {"out": _slice_check(id, Cc, Ct, mode, want, 1e-6)}
        return {"out": out}, refs


def _upsample_to(id, mode, factor):
    @case(id, "g6d_upsample_bilinear_split16")
    def fn(P, knob):
        N, Cc = 3, 64
        H = W = 8 // factor
        g = torch.Generator().manual_seed(29 + factor)
        xc = _rand(g, N, 1, H, W, Cc, scale=2.0)
        scc, shc = _rand(g, N, Cc) * 0.2 + 0.3, _rand(g, N, Cc, scale=0.2)
        out, Ct, width = _slice_map(P, (N, 8, 8), Cc, mode)
        _call("g6d_upsample_bilinear_split16", _p(P.inp(xc, ld=Cc + 4, name="x")), Cc + 4, _p(P.inp(scc, name="scale")), _p(P.inp(shc, name="shift")), 1,
              N, H, W, Cc, factor, _p(out), width, Ct, 8, mode, None)

        def refs():
            want = torch.empty((N, 1, 8, 8, Cc), dtype=torch.float64)
            ref_ops.upsample_bilinear(_d(xc), want, factor, _d(scc), _d(shc), per_n=True)
            return {"out": _slice_check(id, Cc, Ct, mode, want, 1e-6)}
        return {"out": out}, refs


for _mode, _nm in ((3, "pairs"), (2, "fp16")):
    _affine_to(f"affine-split16-to-{_nm}", _mode)
    _upsample_to(f"upsample-split16-x2-{_nm}", _mode, 2)
_upsample_to("upsample-split16-x4-pairs", 3, 4)


def _dense16_check(id, Cc, mode, want, fp32_bar):
    bar = fp32_bar + (2.0 ** -21 if mode == 3 else 2.0 ** -11)

    def f(got):
        m = got.cpu().double().reshape(-1, 2 if mode == 3 else 1, Cc)
        e = _rel(m.sum(1), want.reshape(-1, Cc))
        print(f"GUARDED {id}: rel-to-max error {e:.3e} (bar {bar:.3e})")
        assert e <= bar, e
    return f


def _l2norm16(id, mode, Cc):
    @case(id, "g6d_l2norm_split16")
    def fn(P, knob):
        g = torch.Generator().manual_seed(3 + Cc)
        xc = _rand(g, 2, 3, 5, Cc)
        xc[0, 1, 2] = 0.0
        out = P.out((30, (2 if mode == 3 else 1) * Cc), _T16[mode], name="out")
        _call("g6d_l2norm_split16", _p(P.inp(xc.reshape(30, Cc), ld=Cc + 4, name="x")), Cc + 4, 30, Cc, _p(out), mode, None)
        return {"out": out}, lambda: {"out": _dense16_check(id, Cc, mode, F.normalize(xc.double(), dim=-1), 1e-6)}


_l2norm16("l2norm-split16-pairs-256", 3, 256)
_l2norm16("l2norm-split16-fp16-512", 2, 512)


def _affine16(id, mode, pool):
    """tests/test_conv16_gpu.py::test_affine_split16: 3e-7 (pairs) / 1e-3 (fp16) of the largest value against ref_ops.affine_act_pool."""
    @case(id, "g6d_affine_split16_ex")
    def fn(P, knob):
        g = torch.Generator().manual_seed(9)
        N, H, W, Cc = 6, 8, 12, 64
        xc = _rand(g, N, 1, H, W, Cc)
        scc, shc = 0.5 + torch.rand((3, Cc), generator=g), _rand(g, 3, Cc, scale=0.4)
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        out = P.out((N, Ho, Wo, (2 if mode == 3 else 1) * Cc), _T16[mode], name="out")
        _call("g6d_affine_split16_ex", _p(P.inp(xc, ld=Cc + 4, name="x")), Cc + 4, _p(P.inp(scc, name="scale")), _p(P.inp(shc, name="shift")), 2, 1, int(pool),
              N, H, W, Cc, _p(out), mode, None)

        def refs():
            want = torch.empty((N, 1, Ho, Wo, Cc), dtype=torch.float64)
            ref_ops.affine_act_pool(_d(xc), want, _d(scc), _d(shc), per_n=2, relu=True, pool=1 if pool else 0)
            tol = 3e-7 if mode == 3 else 1e-3

            def f(got):
                m = got.cpu().double().reshape(-1, 2 if mode == 3 else 1, Cc)
                e = _rel(m.sum(1), want.reshape(-1, Cc))
                print(f"GUARDED {id}: rel-to-max error {e:.3e} (bar {tol})")
                assert e <= tol, e
            return {"out": f}
        return {"out": out}, refs


_affine16("affine-split16-pairs", 3, False)
_affine16("affine-split16-pairs-pool", 3, True)
_affine16("affine-split16-fp16-pool", 2, True)


def _product16(id, mode):
    """tests/test_conv16_gpu.py::test_product_split16_and_cout64: 3e-7 (pairs) / 1e-3 (fp16) of the largest value of the product."""
    @case(id, "g6d_product_split16_ex")
    def fn(P, knob):
        g = torch.Generator().manual_seed(5)
        qn, D, hw, Cc = 2, 5, 35, 64
        refc, quec = _rand(g, D, hw, Cc), _rand(g, qn, hw, Cc)
        scc, shc = 0.5 + torch.rand((qn, Cc), generator=g), _rand(g, qn, Cc, scale=0.3)
        out = P.out((qn * D, hw, (2 if mode == 3 else 1) * Cc), _T16[mode], name="out")
        _call("g6d_product_split16_ex", _p(P.inp(refc, name="ref")), _p(P.inp(quec, name="que")), _p(P.inp(scc, name="scale")), _p(P.inp(shc, name="shift")),
              _p(out), qn, D, hw, Cc, mode, None)

        def refs():
            want = ((refc.double()[None] * quec.double()[:, None]) * scc.double()[:, None, None] + shc.double()[:, None, None]).reshape(qn * D, hw, Cc)
            tol = 3e-7 if mode == 3 else 1e-3

            def f(got):
                m = got.cpu().double().reshape(-1, 2 if mode == 3 else 1, Cc)
                e = _rel(m.sum(1), want.reshape(-1, Cc))
                print(f"GUARDED {id}: rel-to-max error {e:.3e} (bar {tol})")
                assert e <= tol, e
            return {"out": f}
        return {"out": out}, refs


_product16("product-split16-pairs", 3)
_product16("product-split16-fp16", 2)


# ================================================================================================ glue kernels
# Shapes and bars: the smallest case of each entry in tests/test_glue_edges_gpu.py (metric: rel-to-max, its _check), or, where that module has
# none, of tests/test_kernels_gpu.py; the bar is quoted beside each case.
def _tables(g, N, Cc, per_n):
    groups = (N + int(per_n) - 1) // int(per_n) if per_n else 1
    return 0.5 + torch.rand((groups, Cc), generator=g), _rand(g, groups, Cc)


def _affine_pool(id, pool, per_n):
    @case(id, "g6d_affine_act_pool")                              # test_affine_act_pool_edges, 1e-6
    def fn(P, knob):
        N, H, W, Cc = 5, 6, 10, 20
        g = torch.Generator().manual_seed(50 + N + pool)
        xc = _rand(g, N, 1, H, W, Cc)
        scc, shc = _tables(g, N, Cc, per_n)
        shape = {0: (N, 1, H, W, Cc), 1: (N, 1, H // 2, W // 2, Cc), 2: (N, 1, 1, 1, Cc)}[pool]
        out = P.out(shape, ld=Cc + 8, name="out")
        _ops().affine_act_pool(P.inp(xc, ld=Cc + 4, name="x"), out, P.inp(scc, name="scale"), P.inp(shc, name="shift"), per_n=per_n, relu=True, pool=pool)

        def refs():
            ref = torch.empty(shape, dtype=torch.float64)
            ref_ops.affine_act_pool(_d(xc), ref, _d(scc), _d(shc), per_n=per_n, relu=True, pool=pool)
            return {"out": (ref, 1e-6)}
        return {"out": out}, refs


_affine_pool("affine-act-pool-none", 0, 2)
_affine_pool("affine-act-pool-max", 1, True)
_affine_pool("affine-act-pool-mean", 2, False)


def _upsample(id, factor):
    @case(id, "g6d_upsample_bilinear")                            # test_upsample_bilinear_edges, 1e-6; the last row and column of the last image are outputs
    def fn(P, knob):
        N, H, W, Cc = 3, 5, 9, 12
        g = torch.Generator().manual_seed(60 + H + factor)
        xc = _rand(g, N, 1, H, W, Cc)
        scc, shc = _tables(g, N, Cc, 2)
        out = P.out((N, 1, H * factor, W * factor, Cc), ld=Cc + 8, name="out")
        _ops().upsample_bilinear(P.inp(xc, ld=Cc + 4, name="x"), out, factor, P.inp(scc, name="scale"), P.inp(shc, name="shift"), per_n=2)

        def refs():
            ref = torch.empty((N, 1, H * factor, W * factor, Cc), dtype=torch.float64)
            ref_ops.upsample_bilinear(_d(xc), ref, factor, _d(scc), _d(shc), per_n=2)
            return {"out": (ref, 1e-6)}
        return {"out": out}, refs


_upsample("upsample-bilinear-x2", 2)
_upsample("upsample-bilinear-x3", 3)


def _nchw(id, N, Cc, H, W, ld, l2):
    @case(id, "g6d_nchw_to_nhwc")                                 # test_nchw_to_nhwc_edges, 1e-6
    def fn(P, knob):
        g = torch.Generator().manual_seed(70)
        xc = _rand(g, N, Cc, H, W)
        out = P.out((N, 1, H, W, Cc), ld=ld, name="out")
        _ops().nchw_to_nhwc(P.inp(xc.reshape(-1), name="x").view(N, Cc, H, W), out, l2)

        def refs():
            ref = torch.empty((N, 1, H, W, Cc), dtype=torch.float64)
            ref_ops.nchw_to_nhwc(_d(xc), ref, l2)
            return {"out": (ref, 1e-6)}
        return {"out": out}, refs


_nchw("nchw-to-nhwc-l2norm", 2, 100, 3, 5, 108, True)
_nchw("nchw-to-nhwc-odd", 1, 7, 5, 13, 15, False)


def _l2rows(id, rows, Cc, ld):
    @case(id, "g6d_l2norm_rows")                                  # test_l2norm_rows_edges, 1e-6; in place: the rows are input and output
    def fn(P, knob):
        g = torch.Generator().manual_seed(71)
        xc = _rand(g, rows, Cc)
        xc[rows // 2] = 0.0
        x = P.out((rows, Cc), ld=ld, name="x", init=xc)
        _call("g6d_l2norm_rows", _p(x), rows, Cc, ld)
        return {"x": x}, lambda: {"x": (F.normalize(xc.double(), dim=-1), 1e-6)}


_l2rows("l2norm-rows-vector", 6, 20, 24)
_l2rows("l2norm-rows-scalar", 5, 7, 7)


@case("bias-relu-pool-nchw", "g6d_bias_relu_pool_nchw")           # tests/test_kernels_gpu.py::test_bias_relu_pool_nchw, 1e-6; odd sizes pool with floor
def _brp(P, knob):
    g = torch.Generator().manual_seed(13)
    N, Cc, H, W = 2, 32, 7, 7
    xc, bc = _rand(g, N, Cc, H, W), _rand(g, Cc)
    out = P.out((N * Cc * (H // 2) * (W // 2),), name="out")
    _call("g6d_bias_relu_pool_nchw", _p(P.inp(xc.reshape(-1), name="x")), _p(P.inp(bc, name="bias")), N, Cc, H, W, 1, 1, _p(out))
    return {"out": out}, lambda: {"out": (ref_ops.bias_relu_pool_nchw(_d(xc), _d(bc), True, True).reshape(-1), 1e-6)}


def _conv1(id, entry):
    @case(id, entry)                                              # tests/test_kernels_gpu.py::test_vgg_conv1_pool(_nhwc), 1e-5; 33 x 67: odd, pooled with floor
    def fn(P, knob):
        g = torch.Generator().manual_seed(5)
        N, H, W = 2, 33, 67
        xc = torch.rand((N, 3, H, W), generator=g) if entry.endswith("norm") else _rand(g, N, 3, H, W)
        wc, bc = _rand(g, 64, 3, 3, 3, scale=0.3), _rand(g, 64, scale=0.2)
        mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        out = P.out((N * 64 * (H // 2) * (W // 2),), name="out")
        args = [_p(P.inp(xc.reshape(-1), name="x")), N, H, W, _p(P.inp(wc.reshape(-1), name="w")), _p(P.inp(bc, name="bias")), 3, 64]
        if entry.endswith("norm"):
            args += [(C.c_float * 3)(*mean), (C.c_float * 3)(*std)]
        _call(entry, *args, _p(out))

        def refs():
            xd = xc.double()
            if entry.endswith("norm"):
                xd = (xd - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
            ref = F.max_pool2d(F.relu(F.conv2d(xd, wc.double(), bc.double(), padding=1)), 2, 2)
            if "nhwc" in entry:
                ref = ref.permute(0, 2, 3, 1)
            return {"out": (ref.reshape(-1), 1e-5)}
        return {"out": out}, refs


_conv1("vgg-conv1-pool", "g6d_vgg_conv1_pool")
_conv1("vgg-conv1-pool-nhwc", "g6d_vgg_conv1_pool_nhwc")
_conv1("vgg-conv1-pool-nhwc-norm", "g6d_vgg_conv1_pool_nhwc_norm")


# ---- selector similarity: test_selector_levels_edges (score maps 2e-6, vps / scale / shift 1e-5, reference sums 1e-12); the smallest case with a
# channel tail is (HW_A, D = 5, qn = 3, C = 64, Dg = D) under its seed 604
def _sel_case():
    from test_glue_edges_gpu import SELECTOR_SEEDS, _selector_case, _selector_truth
    hws, D, qn, Cc = [25, 9, 1], 5, 3, 64
    refs_g, refs, ques = _selector_case(SELECTOR_SEEDS[(25, 5, 3, 64)], hws, D, qn, Cc, 1)
    return hws, D, qn, Cc, refs, ques, lambda: _selector_truth(refs_g, refs, ques)


@case("selector-ref-sums", "g6d_selector_ref_sums")
def _sel_sums(P, knob):
    hws, D, qn, Cc, refs, ques, _ = _sel_case()
    r1, r2 = P.out((hws[0], Cc), torch.float64, name="r1"), P.out((hws[0], Cc), torch.float64, name="r2")
    _call("g6d_selector_ref_sums", _p(P.inp(refs[0], name="refs")), D, hws[0], Cc, _p(r1), _p(r2))

    def rf():
        a, b = ref_ops.selector_ref_sums(_d(refs[0]))
        return {"r1": (a, 1e-12), "r2": (b, 1e-12)}
    return {"r1": r1, "r2": r2}, rf


@case("selector-prod-affine", "g6d_selector_prod_affine")
def _sel_pa(P, knob):
    hws, D, qn, Cc, refs, ques, truth = _sel_case()
    a, b = ref_ops.selector_ref_sums(_d(refs[0]))
    sc, sh = P.out((1, Cc), name="scale"), P.out((1, Cc), name="shift")
    _call("g6d_selector_prod_affine", _p(P.inp(ques[0][0], name="que")), _p(P.inp(a, name="r1")), _p(P.inp(b, name="r2")), D, hws[0], Cc, C.c_double(1e-5),
          _p(sc), _p(sh))

    def rf():
        _, _, rsc, rsh = truth()[0][0]
        return {"scale": (rsc[None], 1e-5), "shift": (rsh[None], 1e-5)}
    return {"scale": sc, "shift": sh}, rf


@case("selector-scan", "g6d_selector_scan")
def _sel_scan(P, knob):
    hws, D, qn, Cc, refs, ques, truth = _sel_case()
    smap, vps = P.out((D, hws[0]), name="score_map"), P.out((D,), name="vps")
    _call("g6d_selector_scan", _p(P.inp(ques[0][0], name="que")), _p(P.inp(refs[0], name="refs")), D, hws[0], Cc, _p(smap), _p(vps))

    def rf():
        rs, rv, _, _ = truth()[0][0]
        return {"score_map": (rs, 2e-6), "vps": (rv, 1e-5)}
    return {"score_map": smap, "vps": vps}, rf


@case("selector-levels", "g6d_selector_levels")
def _sel_levels(P, knob):
    hws, D, qn, Cc, refs, ques, truth = _sel_case()
    L = len(hws)
    sums = [ref_ops.selector_ref_sums(_d(r)) for r in refs]
    qd = [P.inp(q, name=f"que{l}") for l, q in enumerate(ques)]
    rd = [P.inp(r, name=f"refs{l}") for l, r in enumerate(refs)]
    r1 = [P.inp(s[0], name=f"r1_{l}") for l, s in enumerate(sums)]
    r2 = [P.inp(s[1], name=f"r2_{l}") for l, s in enumerate(sums)]
    maps = [P.out((qn, D, hw), name=f"map{l}") for l, hw in enumerate(hws)]
    vps, sc, sh = P.out((qn, L, D), name="vps"), P.out((qn, L, Cc), name="scale"), P.out((qn, L, Cc), name="shift")
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    _call("g6d_selector_levels", L, qn, arr(qd), arr(rd), arr(r1), arr(r2), (C.c_int * L)(*hws), D, D, Cc, C.c_double(1e-5), arr(maps), _p(vps), _p(sc), _p(sh))

    def rf():
        t = truth()
        r = {f"map{l}": (torch.stack([t[l][q][0] for q in range(qn)]), 2e-6) for l in range(L)}

        def per_level(idx, bar, what):
            def f(got):
                for q in range(qn):
                    for l in range(L):
                        _assert_rel(got[q, l], t[l][q][idx], bar, f"selector-levels {what} q{q} l{l}")
            return f
        r["vps"], r["scale"], r["shift"] = per_level(1, 1e-5, "vps"), per_level(2, 1e-5, "scale"), per_level(3, 1e-5, "shift")
        return r
    o = {f"map{l}": m for l, m in enumerate(maps)}
    o.update(vps=vps, scale=sc, shift=sh)
    return o, rf


# ---- refiner volume: test_refiner_volume_edges, 2e-4; (rfn 2, C 132, 9 x 7 maps, sn 5): a ragged second channel trip, odd maps, 125 voxels
def _vol_inputs():
    """The cameras of tests/test_glue_edges_gpu.py::_volume_case with the query view's principal point moved so that one voxel projects into
    the LAST pixel cell of the last feature map (the query's): its x + 1 and y + 1 taps are the ones that would stray behind `feats`.
    Asserted from the float64 projection of the float32 operands."""
    from test_glue_edges_gpu import _volume_case
    rfn, Cc, fh, fw, h_in, w_in, sn = 2, 132, 9, 7, 72, 56, 5
    g = torch.Generator().manual_seed(95)
    ref_Ks, ref_poses, K_in, pose_in = _volume_case(rfn, h_in, w_in)
    lin = torch.linspace(-1, 1, sn)

    def cells(K):
        X = (torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3).double() @ pose_in[:, :3].double()) @ \
            (K.double() @ pose_in.double())[:, :3].T + (K.double() @ pose_in.double())[:, 3]
        u, v = X[:, 0] / X[:, 2].clamp(min=1e-4), X[:, 1] / X[:, 2].clamp(min=1e-4)
        return u, v, (u + 0.5) / w_in * fw - 0.5, (v + 0.5) / h_in * fh - 0.5             # image coordinates, feature-map coordinates
    u, v, _, _ = cells(K_in)
    j = int(torch.argmax(u / w_in + v / h_in))
    K_in = K_in.clone()
    K_in[0, 2] += float((fw - 0.25) / fw * w_in - 0.5 - u[j])                            # voxel j -> feature coordinates (fw - 0.75, fh - 0.75)
    K_in[1, 2] += float((fh - 0.25) / fh * h_in - 0.5 - v[j])
    u, v, fx, fy = cells(K_in)
    last = (fx.floor() == fw - 1) & (fy.floor() == fh - 1)
    inside = ((u >= 0) & (u <= w_in - 1) & (v >= 0) & (v <= h_in - 1)).double().mean().item()
    assert int(last.sum()) >= 1, "no voxel samples the last row and column of the query's feature map"
    assert 0.25 <= inside <= 0.95, f"{100 * inside:.0f} % of the voxels inside the query view: interior and zero-padding taps must both occur"
    feats = _rand(g, rfn + 1, fh, fw, Cc)
    return rfn, Cc, fh, fw, h_in, w_in, sn, ref_Ks.contiguous(), ref_poses, K_in.contiguous(), pose_in, feats, lin


def _vol_ref(Cc, sn, feats, ref_Ks, ref_poses, K_in, pose_in, lin, h_in, w_in):
    projs = torch.cat([ref_Ks @ ref_poses, (K_in @ pose_in)[None]], 0).contiguous()
    rm, rs = torch.empty((sn ** 3, 2 * Cc), dtype=torch.float64), torch.empty((sn ** 3, Cc), dtype=torch.float64)
    ref_ops.refiner_volume(_d(feats), _d(projs), _d(pose_in[:, :3].contiguous()), _d(lin), h_in, w_in, rm, rs)
    return rm, rs


def _volume(id, entry):
    @case(id, entry)
    def fn(P, knob):
        ops = _ops()
        rfn, Cc, fh, fw, h_in, w_in, sn, ref_Ks, ref_poses, K_in, pose_in, feats, lin = _vol_inputs()
        nv = sn ** 3
        fg, lg = P.inp(feats, name="feats"), P.inp(lin, name="lin")
        if entry == "g6d_refiner_volume":
            mean_in, std = P.out((nv, 2 * Cc), name="mean_in"), P.out((nv, Cc), name="std")
            projs = torch.cat([ref_Ks @ ref_poses, (K_in @ pose_in)[None]], 0).contiguous()
            ops.refiner_volume(fg, P.inp(projs, name="projs"), P.inp(pose_in[:, :3].contiguous(), name="rot"), lg, h_in, w_in, mean_in, std)
        elif entry == "g6d_refiner_volume_kp":
            mean_in, std = P.out((nv, 2 * Cc), name="mean_in"), P.out((nv, Cc), name="std")
            ops.refiner_volume_kp(fg, P.inp(ref_Ks, name="ref_Ks"), P.inp(ref_poses, name="ref_poses"), P.inp(K_in, name="K_in"), P.inp(pose_in, name="pose_in"),
                                  lg, h_in, w_in, mean_in, std)
        else:                                                     # pair maps [voxel][2][2C] / [voxel][2][C]: the row is both planes
            mean_in, std = P.out((nv, 4 * Cc), torch.float16, name="mean_in"), P.out((nv, 2 * Cc), torch.float16, name="std")
            _call(entry, _p(fg), _p(P.inp(ref_Ks, name="ref_Ks")), _p(P.inp(ref_poses, name="ref_poses")), _p(P.inp(K_in, name="K_in")),
                  _p(P.inp(pose_in, name="pose_in")), _p(lg), rfn, fh, fw, Cc, h_in, w_in, sn, _p(mean_in), _p(std), 1, None, None)

        def refs():
            rm, rs = _vol_ref(Cc, sn, feats, ref_Ks, ref_poses, K_in, pose_in, lin, h_in, w_in)
            if entry != "g6d_refiner_volume_kp_pairs":
                return {"mean_in": (rm, 2e-4), "std": (rs, 2e-4)}
            # (tests/test_refiner_volume_pairs_gpu.py holds the pairs to 2^-21 of the fp32 entry's range; against float64 the fp32 entry's 2e-4 is added)

            def pairs(want, width):
                def f(got):
                    m = got.cpu().double().reshape(nv, 2, width)
                    _assert_rel(m.sum(1), want, 2e-4 + 2.0 ** -21, f"{id} {width}")
                return f
            return {"mean_in": pairs(rm, 2 * Cc), "std": pairs(rs, Cc)}
        return {"mean_in": mean_in, "std": std}, refs


_volume("refiner-volume", "g6d_refiner_volume")
_volume("refiner-volume-kp", "g6d_refiner_volume_kp")
_volume("refiner-volume-kp-pairs", "g6d_refiner_volume_kp_pairs")


# ---- detector glue
DET_STATS = [[36.264317, 13.151907], [13910.291, 5345.965], [829.70807, 387.98788]]


@case("detector-assemble", "g6d_detector_assemble")               # test_detector_assemble_edges (8, 12) -> (5, 9), rfn 5, 3 sigma, 1e-5
def _det_asm(P, knob):
    hc, wc, hs, ws, rfn, B, clip = 8, 12, 5, 9, 5, 2, 10.0
    g = torch.Generator().manual_seed(80 + hs + rfn)
    s = [_rand(g, B * (hc >> l) * (wc >> l), rfn, scale=3 * DET_STATS[l][1]) + DET_STATS[l][0] for l in range(3)]
    # slot 1 of 4: the other nine channels of every row belong to the other scales and must keep what they hold
    stacked = P.out((B * hs * ws, rfn, 12), name="stacked", init=torch.zeros((B * hs * ws, rfn, 12)))
    _ops().detector_assemble(P.inp(s[0], name="s0"), P.inp(s[1], name="s1"), P.inp(s[2], name="s2"), hc, wc, DET_STATS, clip, hs, ws, 1, stacked, batch=B)

    def refs():
        r = torch.zeros((B * hs * ws, rfn, 12), dtype=torch.float64)
        ref_ops.detector_assemble(_d(s[0]), _d(s[1]), _d(s[2]), hc, wc, DET_STATS, clip, hs, ws, 1, r, batch=B)
        return {"stacked": (r, 1e-5)}
    return {"stacked": stacked}, refs


@case("detector-score-mlp-max", "g6d_detector_score_mlp_max")      # test_detector_score_mlp_max_edges rfn 5, P = 53, 1e-5
def _det_mlp(P, knob):
    g = torch.Generator().manual_seed(81)
    Pn, rfn = 53, 5
    st = _rand(g, Pn, rfn, 12, scale=3.0)
    w0, b0, w1, b1 = _rand(g, 64, 12, scale=0.3), _rand(g, 64, scale=0.1), _rand(g, 64, 64, scale=0.2), _rand(g, 64, scale=0.1)
    out = P.out((Pn, 64), name="out")
    _call("g6d_detector_score_mlp_max", _p(P.inp(st, name="stacked")), Pn, rfn, 12, _p(P.inp(w0, name="w0")), _p(P.inp(b0, name="b0")), _p(P.inp(w1, name="w1")),
          _p(P.inp(b1, name="b1")), _p(out))
    return {"out": out}, lambda: {"out": (ref_ops.detector_score_mlp_max(_d(st), _d(w0), _d(b0), _d(w1), _d(b1)), 1e-5)}


@case("detector-decode", "g6d_detector_decode")                   # test_detector_decode_edges 20 x 13 (more than 256 cells), batch 3, column views, 1e-6
def _det_dec(P, knob):
    g = torch.Generator().manual_seed(82)
    hs, ws, B = 20, 13, 3
    Pn = hs * ws
    o4 = _rand(g, B * Pn, 4)
    o4[0, 0] = 5.0
    o4[2 * Pn - 1, 0] = 5.0
    o4[2 * Pn:, 0] = 0.25
    og = P.inp(o4, name="heads")
    res = P.out((B, 5), name="result")
    _call("g6d_detector_decode", _p(og[:, 0:1]), 4, _p(og[:, 2:4]), 4, _p(og[:, 1:2]), 4, hs, ws, 8, _p(res), B)
    return {"result": res}, lambda: {"result": (ref_ops.detector_decode(_d(o4)[:, 0:1], _d(o4)[:, 2:4], _d(o4)[:, 1:2], hs, ws, 8, batch=B), 1e-6)}


@case("resize-bilinear-pyramid", "g6d_resize_bilinear_pyramid")    # tests/test_kernels_gpu.py::test_resize_bilinear_pyramid (3, 45, 77), 1e-4 against fp64
def _resize(P, knob):
    g = torch.Generator().manual_seed(3)
    N, H, W = 3, 45, 77
    sizes = [(64, 109), (23, 39), (16, 27)]                          # up-sampling, a width that is no multiple of 4, down-sampling
    xc = torch.rand((N, 3, H, W), generator=g)
    outs = [P.out((N * 3 * h * w,), name=f"out{i}") for i, (h, w) in enumerate(sizes)]
    n = len(sizes)
    _call("g6d_resize_bilinear_pyramid", _p(P.inp(xc.reshape(-1), name="x")), N * 3, H, W, n, (C.c_int * n)(*[s[0] for s in sizes]),
          (C.c_int * n)(*[s[1] for s in sizes]), (C.c_void_p * n)(*[o.data_ptr() for o in outs]))
    return {f"out{i}": o for i, o in enumerate(outs)}, \
        lambda: {f"out{i}": (F.interpolate(xc.double(), size=sz, mode="bilinear").reshape(-1), 1e-4) for i, sz in enumerate(sizes)}


# ---- selector tail
@case("vps-norm", "g6d_vps_norm")                                  # test_vps_norm_edges (D 300, B 2, ld 516, c_off 512), 1e-5
def _vps(P, knob):
    D, B, ld, c_off = 300, 2, 516, 512
    g = torch.Generator().manual_seed(90 + D)
    vps = _rand(g, B, 3, D, scale=20) + 30
    feats = P.out((B * D, ld), name="feats", init=torch.full((B * D, ld), -777.0))
    _ops().vps_norm(P.inp(vps, name="vps"), feats, c_off)

    def refs():
        r = torch.full((B * D, ld), -777.0, dtype=torch.float64)
        ref_ops.vps_norm(_d(vps), r, c_off)

        def f(got):
            _assert_rel(got[:, c_off:c_off + 3], r[:, c_off:c_off + 3], 1e-5, "vps-norm")
            assert bool((got[:, :c_off] == -777.0).all()) and bool((got[:, c_off + 3:] == -777.0).all()), "wrote outside its three columns"
        return {"feats": f}
    return {"feats": feats}, refs


@case("max-an-add", "g6d_max_an_add")                              # test_max_an_add_edges an 7, 1e-6
def _maa(P, knob):
    g = torch.Generator().manual_seed(91)
    rfn, Cc, B, an = 3, 20, 2, 7
    xc, emb = _rand(g, B * rfn * an, Cc), _rand(g, rfn, Cc)
    out = P.out((B * rfn, Cc), ld=Cc + 8, name="out")
    _ops().max_an_add(P.inp(xc, ld=Cc + 4, name="x"), rfn, an, P.inp(emb, name="embed"), out, batch=B)

    def refs():
        r = torch.empty((B * rfn, Cc), dtype=torch.float64)
        ref_ops.max_an_add(_d(xc), rfn, an, _d(emb), r, batch=B)
        return {"out": (r, 1e-6)}
    return {"out": out}, refs


def _attention(id, n, heads, Cc):
    @case(id, "g6d_attention")                                     # test_attention_edges, 1e-5: n = 3 on the block kernel, n = 65 on the wave-per-token kernel
    def fn(P, knob):
        g = torch.Generator().manual_seed(94 + n)
        B = 2
        qkv = _rand(g, B * n, 3 * Cc)
        q = P.inp(qkv, name="qkv")                                 # q / k / v: column slices of one buffer, row stride 3 C
        out = P.out((B * n, Cc), ld=Cc + 8, name="out")
        _ops().attention(q[:, :Cc], q[:, Cc:2 * Cc], q[:, 2 * Cc:], heads, out, batch=B)

        def refs():
            qd = _d(qkv)
            r = torch.empty((B * n, Cc), dtype=torch.float64)
            ref_ops.attention(qd[:, :Cc], qd[:, Cc:2 * Cc], qd[:, 2 * Cc:], heads, r, batch=B)
            return {"out": (r, 1e-5)}
        return {"out": out}, refs


_attention("attention-block-kernel", 3, 8, 64)
_attention("attention-wave-kernel", 65, 8, 64)


def _layernorm(id, Cc):
    @case(id, "g6d_layernorm")                                     # test_layernorm_edges, 1e-5 (rows offset by +100 as there)
    def fn(P, knob):
        g = torch.Generator().manual_seed(92)
        n = 5
        xc = _rand(g, n, Cc) + 100.0
        gam, bet = 0.5 + torch.rand(Cc, generator=g), _rand(g, Cc)
        out = P.out((n, Cc), ld=Cc + 3, name="out")
        _ops().layernorm(P.inp(xc, ld=Cc + 9, name="x"), P.inp(gam, name="gamma"), P.inp(bet, name="beta"), out)

        def refs():
            r = torch.empty((n, Cc), dtype=torch.float64)
            ref_ops.layernorm(_d(xc), _d(gam), _d(bet), r)
            return {"out": (r, 1e-5)}
        return {"out": out}, refs


_layernorm("layernorm-7", 7)
_layernorm("layernorm-100", 100)


@case("affine-act-add", "g6d_affine_act_add")                      # test_affine_act_add_edges "ragged-groups" with a strided residual, 1e-6
def _aaa(P, knob):
    g = torch.Generator().manual_seed(93)
    n, Cc, rpg = 7, 20, 3
    xc, resc = _rand(g, n, Cc), _rand(g, n, Cc)
    scc, shc = 0.5 + torch.rand((3, Cc), generator=g), _rand(g, 3, Cc)
    out = P.out((n, Cc), ld=Cc + 8, name="out")
    _ops().affine_act_add(P.inp(xc, ld=Cc + 4, name="x"), out, P.inp(scc, name="scale"), P.inp(shc, name="shift"), relu=True,
                          residual=P.inp(resc, ld=Cc + 12, name="residual"), rows_per_group=rpg)

    def refs():
        r = torch.empty((n, Cc), dtype=torch.float64)
        ref_ops.affine_act_add(_d(xc), r, _d(scc), _d(shc), relu=True, residual=_d(resc), rows_per_group=rpg)
        return {"out": (r, 1e-6)}
    return {"out": out}, refs


def _gemv(id, entry, B, K, O, mfma):
    @case(id, entry)                                               # test_linear_gemv_small (9, 516, 5) / tests/test_kernels_gpu.py::test_linear_gemv, 1e-5
    def fn(P, knob):
        knob("gemv_mfma", mfma)
        g = torch.Generator().manual_seed(96)
        xc, Wc, bc = _rand(g, B, K), _rand(g, O, K, scale=K ** -0.5), _rand(g, O, scale=0.1)
        out = P.out((B, O), name="out")
        args = [_p(P.inp(xc, name="x")), B, K, _p(P.inp(Wc, name="W")), _p(P.inp(bc, name="bias")), O, 2, _p(out)]
        if entry.endswith("batch"):
            args += list(_ws())
        _call(entry, *args)
        return {"out": out}, lambda: {"out": (ref_ops.linear_gemv(_d(xc), _d(Wc), _d(bc), 2), 1e-5)}


_gemv("linear-gemv", "g6d_linear_gemv", 2, 516, 3, 0)
for _m, _nm in ((2, "matrix-cores"), (0, "vector-alu")):
    _gemv(f"linear-gemv-batch-rows-{_nm}", "g6d_linear_gemv_batch", 9, 516, 5, _m)
    _gemv(f"linear-gemv-batch-slices-{_nm}", "g6d_linear_gemv_batch", 11, 8192, 64, _m)


# ---- warps (byte pixels: guards of 0xff).  The rule of test_warp_batch_edges::_warp_rule on grey levels: at most one level off, and more than
# half a level off on fewer than 1 % of the values (rounding ties)
def _warp_rule(got, want, what):
    d = (got.double() - want.double()).abs()
    print(f"GUARDED {what}: max {d.max().item():.3f} levels, {100 * (d > 0.5).double().mean().item():.3f} % off by more than 1/2")
    assert d.max() <= 1.001 and (d > 0.5).double().mean() < 0.01, what


def _cover(sh, sw, dh, dw):
    """Destination -> source map under which the destination covers the source exactly: its last pixel samples the source's last row and column."""
    return torch.tensor([(sw - 1) / (dw - 1), 0.0, 0.0, 0.0, (sh - 1) / (dh - 1), 0.0, 0.0, 0.0, 1.0])


def _warp_batch(id, ch, with_single):
    @case(id, "g6d_warp_batch")
    def fn(P, knob):
        from test_glue_edges_gpu import _homographies, _images
        dh, dw, B, sh, sw = 40, 72, 4, 32, 48
        imgs, que = _images(5, sh, sw, ch, 33), _images(1, sh, sw, ch, 34)[0]
        hinv = _homographies(np.random.RandomState(3 + sh), B)
        hinv[3] = _cover(sh, sw, dh, dw)                          # entry 3 reads image 4, the last of the stack, down to its last row and column
        idx = torch.tensor([-1, 3, 0, 4] if with_single else [2, 3, 0, 4], dtype=torch.int32)
        out = P.out((B, ch, dh, dw), name="out")
        _ops().warp_batch(P.inp(imgs, name="stack"), P.inp(que, name="single") if with_single else None, P.inp(idx, name="idx"), P.inp(hinv, name="hinv"),
                          dh, dw, out=out)

        def refs():
            want = ref_ops.warp_batch(imgs, que if with_single else None, idx, hinv, dh, dw, dtype=torch.float64)
            return {"out": lambda got: _warp_rule(got.cpu() * 255, want * 255, id)}
        return {"out": out}, refs


_warp_batch("warp-batch-1ch", 1, True)
_warp_batch("warp-batch-4ch", 4, False)


def _warp_one(id, ch, out_float, cover):
    @case(id, "g6d_warp_perspective")
    def fn(P, knob):
        from test_glue_edges_gpu import _homographies, _images
        dh, dw, sh, sw = 40, 72, 32, 48
        src = _images(1, sh, sw, ch, 34)[0]
        hinv = _cover(sh, sw, dh, dw) if cover else _homographies(np.random.RandomState(3 + sh), 1)[0]
        out = P.out((dh, dw, ch), torch.float32 if out_float else torch.uint8, name="out",
                    init=None if out_float else torch.full((dh, dw, ch), 255, dtype=torch.uint8))
        _call("g6d_warp_perspective", _p(P.inp(src, name="src")), sh, sw, ch, (C.c_float * 9)(*hinv.tolist()), _p(out), dh, dw, int(out_float),
              C.c_float(1.0 / 255.0))

        def refs():
            H = np.linalg.inv(hinv.double().numpy().reshape(3, 3))
            want = ref_ops.warp_perspective(src, H, dh, dw, out_float=out_float, dtype=torch.float64)
            return {"out": lambda got: _warp_rule(got.cpu() * (255 if out_float else 1), want * (255 if out_float else 1), id)}
        return {"out": out}, refs


_warp_one("warp-perspective-u8-3ch-cover", 3, False, True)
_warp_one("warp-perspective-float-1ch", 1, True, False)


# ================================================================================================ the test
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guarded(c, knob):
    try:
        _run(c, knob)
    except RuntimeError as e:                                        # a device fault leaves the context unusable: nothing more is started on it
        if any(s in str(e).lower() for s in ("illegal memory access", "hip error", "hiperror", "device-side assert")):
            pytest.exit(f"{c.id}: device fault, the session ends here: {e}", returncode=3)
        raise


def _run(c, knob):
    from gen6d_amd import lib
    lib.load()
    P = Place(True)
    outs, refs = c.fn(P, knob)
    torch.cuda.synchronize()
    layout = "; ".join(f"{n}: {a.describe()}" for n, a, _ in P.arenas)
    print(f"GUARDED {c.id} [{', '.join(c.entries)}] {layout}")
    for name, t in outs.items():                                     # (1)
        if t.dtype.is_floating_point:
            assert bool(torch.isfinite(t).all()), f"{c.id}: output {name} holds non-finite values " \
                f"({int((~torch.isfinite(t)).sum())} of {t.numel()}, first at {(~torch.isfinite(t)).nonzero()[0].tolist()})"
    for name, a, whole in P.arenas:
        if whole:
            assert a.unwritten() == 0, f"{c.id}: {a.unwritten()} elements of output {name} were never written"
    for name, ref in refs().items():                                 # (2)
        if callable(ref):
            ref(outs[name])
            continue
        want, bar = ref
        err = _rel(outs[name], want)
        print(f"GUARDED {c.id} {name}: rel-to-max error {err:.3e} (bar {bar})")
        assert err <= bar, f"{c.id}: {name} rel-to-max error {err:.3e} > {bar}"
    for name, a, _ in P.arenas:                                      # (3)
        assert a.untouched(), f"{c.id}: guard of {name} touched at offsets {a.touched()[:8]} from the operand ({a.describe()})"
    Q = Place(False)
    plain, _ = c.fn(Q, knob)                                         # (4)
    torch.cuda.synchronize()
    for name, t in outs.items():
        if name in c.atomics:
            continue
        same = torch.equal(_bits(t), _bits(plain[name]))
        print(f"GUARDED {c.id} {name}: bit-equal to the plain run: {same}")
        assert same, f"{c.id}: {name} differs from the run on plain allocations " \
            f"(max |diff| {float((t.double() - plain[name].double()).abs().max()):.3e})"
