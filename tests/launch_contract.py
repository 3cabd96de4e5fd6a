"""The argument contract of every launcher of libgen6d_hip.so (include/gen6d_hip.h), as a table: per entry point of
gen6d_amd.lib.SIGNATURES one BASELINE call that the launcher must accept and a list of SINGLE-FAULT VIOLATIONS that it must refuse before
any HIP call.  Host integer work only: tests/test_launch_contract_cpu.py runs the table where NO GPU is visible.

How a call is made without a GPU.  Device operands are fake addresses (non-null, 16-byte aligned, distinct, all cut from ONE fake base so
that the multi-map launchers' "within 2^29 / 2^30 / 2^31 floats of each other" rule holds); whatever a launcher itself dereferences on the
host (descriptors, segment tables, range records, mu_sigma, the pyramid's size arrays, the per-level arrays of g6d_selector_levels, the
homography of g6d_warp_perspective, mean / std of the first trunk layer) is real ctypes memory.  On a host without a GPU a call that passes
validation comes back G6D_ELAUNCH ("no ROCm-capable device"; the host-only plan functions: G6D_OK) and a refused call G6D_EINVAL / G6D_ENOSPC
with a fresh g6d_last_error().  `issue()` raises when a GPU is visible: a violation that a launcher failed to refuse would launch a kernel
on the fake pointers.

The table is written from the header comments and the kernels' access patterns, not from the launchers' `if`s.  Violation classes:
  null       a required pointer is NULL (optional ones are declared `O` / `ON` and passed as NULL in an extra ACCEPTED call)
  extent     a dimension or count is 0 / -1; a documented maximum + 1 (the maximum itself is accepted)
  stride     a row stride smaller than the row it holds, or off the vector width where the kernel uses 16-byte accesses
  alignment  base + 4 bytes for pointers read or written with 8- / 16-byte accesses (kernels with a scalar fallback ACCEPT it)
  reach      sizes whose element offset, work-item count or grid size leaves the type it is computed in
  mode       an enumeration outside its documented values
  pairing    scale without shift, a workspace that is missing / misaligned / too small for the route that needs it, ...

Argument kinds (the first element of each spec tuple, see the constructors below):
  P  required device pointer           O  optional device pointer, non-null in the baseline     ON  optional, NULL in the baseline
  H  required host array               HO optional host array                                   T   required host table of structs
  R  optional host G6dRange16 record   N  dimension / count >= 1 (0 and -1 are violations)      N0  count >= 0 (-1 is the violation)
  I  integer with hand-written cases   X  free integer: any value is meaningful (reason given)  F   float / double
  S  the stream (NULL = the default stream)
"""
import copy
import ctypes as C
import os
import re
import sys
from collections import namedtuple

if __name__ == "__main__":          # run as a script (the record of profiles/r32_launch_contract.md): the package sits one level up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gen6d_amd import lib

EINVAL, ENOSPC = -1, -2
CLASSES = ("null", "extent", "stride", "alignment", "reach", "mode", "pairing")
SENTINEL = b"set_knob: unknown knob"
EXEMPT = {"g6d_marker": "no operand: launches the empty marker kernel", "g6d_sizeof_frame_desc": "no argument",
          "g6d_sizeof_mesh_desc": "no argument", "g6d_sizeof_sink_desc": "no argument"}

FAKE_BASE, FAKE_STEP = 0x1000000000, 1 << 20        # every fake operand 1 MiB after the previous one: 64 of them span 2^24 floats
INT_MAX = 2 ** 31 - 1


def dev(k):
    """Fake device address number k: non-null, 16-byte aligned, distinct."""
    return FAKE_BASE + k * FAKE_STEP


Arg = namedtuple("Arg", "name kind base meta")
Case = namedtuple("Case", "entry cls label over expect")      # expect: "reject" / "accept"


def P(name, al=None): return Arg(name, "P", None, {"al": al})            # al: "req" base + 4 is refused, "scalar" base + 4 is accepted
def O(name, al=None, paired=False): return Arg(name, "O", None, {"al": al, "paired": paired})      # paired: NULL alone may break a pairing
def ON(name): return Arg(name, "ON", 0, {})
def H(name, ctype, values): return Arg(name, "H", list(values), {"ctype": ctype})
def HO(name, ctype, values): return Arg(name, "HO", list(values), {"ctype": ctype, "paired": False})
def T(name, struct, rows, fields): return Arg(name, "T", rows, {"struct": struct, "fields": fields})
def R(name): return Arg(name, "R", None, {})
def N(name, v): return Arg(name, "N", v, {})
def N0(name, v): return Arg(name, "N0", v, {})
def I(name, v): return Arg(name, "I", v, {})
def X(name, v, why): return Arg(name, "X", v, {"why": why})
def F(name, v): return Arg(name, "F", v, {})
def S(): return Arg("stream", "S", 0, {})


def rej(cls, label, **over): return ("reject", cls, label, over)
def acc(cls, label, **over): return ("accept", cls, label, over)
def rejk(cls, label, over): return ("reject", cls, label, over)         # overrides whose keys are not identifiers ("segs[0].H")
def acck(cls, label, over): return ("accept", cls, label, over)


def mx(name, m, cls="extent", **also):
    """A documented maximum: `m` is accepted, `m + 1` refused (`also`: what else has to change for the maximum to be reachable)."""
    return [("accept", cls, f"{name}={m} (max)", dict(also, **{name: m})), ("reject", cls, f"{name}={m + 1} (max+1)", dict(also, **{name: m + 1}))]


FLAG = "a flag: any value is meaningful"
ENTRIES = {}        # name -> (args, hand-written cases)


def E(name, args, cases=()):
    flat = []
    for c in cases:
        flat.extend(c if isinstance(c, list) else [c])
    k = 0
    out = []
    for a in args:
        if a.kind in ("P", "O"):
            a = a._replace(base=dev(k))
            k += 1
        out.append(a)
    ENTRIES[name] = (out, flat)


# ---------------------------------------------------------------------------------------------------------- struct field kinds
SEG_PTRS = 40       # table rows take their fake addresses from dev(40) upwards
WINO_FIELDS = {"in_": "P", "out_full": "O", "out_pool": "ON", "N": "N", "H": "N", "W": "N", "ld_in": "N", "ld_full": "N",
               "ld_pool": ("X", "not read while out_pool is NULL (the baseline); its own case sets out_pool")}
CORR_FIELDS = {"in_": "P", "out": "P", "H": "N", "W": "N", "ld_in": "N", "ld_out": "N", "N": "N", "reserved_": ("X", "reserved: not read")}
C16_FIELDS = {"in_": "P", "out_full": "O", "out_pool": "ON", "N": "N", "D": "N", "H": "N", "W": "N", "ld_in": "N", "ld_full": "N",
              "ld_pool": ("X", "not read while out_pool is NULL (the baseline); its own case sets out_pool")}


def wino_rows(cin, cout):
    return [dict(in_=dev(SEG_PTRS), out_full=dev(SEG_PTRS + 1), out_pool=0, N=1, H=8, W=8, ld_in=cin, ld_full=cout, ld_pool=0)]


def corr_rows(cin, cout, hw=16):
    return [dict(in_=dev(SEG_PTRS), out=dev(SEG_PTRS + 1), H=hw, W=hw, ld_in=cin, ld_out=cout, N=1, reserved_=0)]


def c16_rows(ld_in, ld_full, hw=8):
    return [dict(in_=dev(SEG_PTRS), out_full=dev(SEG_PTRS + 1), out_pool=0, N=1, D=1, H=hw, W=hw, ld_in=ld_in, ld_full=ld_full, ld_pool=0)]


def seg_reach(name, reach_log2, field="in_"):
    """One segment of a two-row table moved beyond the stated reach (floats) of the other, and just inside it."""
    far = dev(SEG_PTRS) + 4 * (1 << reach_log2)
    near = dev(SEG_PTRS) + 4 * ((1 << reach_log2) - (1 << 22))
    return [rejk("reach", f"{name}[1].{field} 2^{reach_log2} floats away", {f"{name}[+]": {field: far}}),
            acck("reach", f"{name}[1].{field} just inside 2^{reach_log2} floats", {f"{name}[+]": {field: near}})]


# ---------------------------------------------------------------------------------------------------------- G6dConv
CONV_FIELDS = {
    "in_": "P", "mul": "ON", "in_scale": "ON", "in_shift": "ON", "weight": "P", "bias": "ON", "out": "P", "stats": "ON", "workspace": "ON",
    "workspace_bytes": ("X", "0 with a NULL workspace disables splitting; any size is meaningful"),
    "N": "N", "Di": "N", "Hi": "N", "Wi": "N", "Cin": "N", "ld_in": "N", "Do": "N", "Ho": "N", "Wo": "N", "Cout": "N", "ld_out": "N",
    "kd": "N", "kh": "N", "kw": "N", "sd": "N", "sh": "N", "sw": "N",
    "pd": "I", "ph": "I", "pw": "I", "in_relu": "I", "in_affine_per_n": "I", "out_act": "I",
    "stat_rows_per_group": ("X", "not read while stats is NULL (the baseline)"),
    "split_k": ("X", "<= 0 chooses automatically, 1 never splits, > 1 forces: every value is meaningful"), "math_mode": "I",
    "weight_wino": "ON", "fin_scale": "ON", "fin_shift": "ON", "fin_counter": "ON",
    "fin_groups": ("X", "not read while fin_scale is NULL (the baseline)"), "in_image_mod": "I", "mul_group_images": "I",
    "reserved_": ("X", "w_exp: not read outside math_mode 3 - 5"), "weight_wino16": "ON", "weight_wino43": "ON",
    "fin_count": "F", "fin_eps": "F",
}


def conv_row():
    return [dict(in_=dev(SEG_PTRS), weight=dev(SEG_PTRS + 1), out=dev(SEG_PTRS + 2), N=1, Di=1, Hi=8, Wi=8, Cin=8, ld_in=8, Do=1, Ho=8, Wo=8,
                 Cout=32, ld_out=32, kd=1, kh=3, kw=3, sd=1, sh=1, sw=1, pd=0, ph=1, pw=1)]


def conv_cases():
    d = "desc[0]."
    return [
        rejk("extent", "pd=-1", {d + "pd": -1}), rejk("extent", "ph=-1", {d + "ph": -1}), rejk("extent", "pw=-1", {d + "pw": -1}),
        rejk("stride", "ld_in=4 < Cin=8", {d + "ld_in": 4}), rejk("stride", "ld_out=16 < Cout=32", {d + "ld_out": 16}),
        acck("stride", "ld_in == Cin, ld_out == Cout", {d + "ld_in": 8, d + "ld_out": 32}),
        rejk("mode", "out_act=3", {d + "out_act": 3}), rejk("mode", "out_act=-1", {d + "out_act": -1}), acck("mode", "out_act=2", {d + "out_act": 2}),
        rejk("mode", "math_mode=6", {d + "math_mode": 6}), rejk("mode", "math_mode=-1", {d + "math_mode": -1}),
        rejk("mode", "in_affine_per_n=-1", {d + "in_affine_per_n": -1}),
        rejk("mode", "in_image_mod=-1", {d + "in_image_mod": -1}), rejk("mode", "mul_group_images=-1", {d + "mul_group_images": -1}),
        rejk("pairing", "in_scale without in_shift", {d + "in_scale": dev(50)}),
        # the ReLU of the prologue is the one after the InstanceNorm affine: every kernel applies it inside its affine branch (the narrow
        # kernel has no prologue at all), so the flag alone would be dropped; with the affine any non-zero value means "on"
        rejk("pairing", "in_relu without in_scale", {d + "in_relu": 1}),
        acck("pairing", "in_relu with in_scale and in_shift", {d + "in_relu": 1, d + "in_scale": dev(50), d + "in_shift": dev(51)}),
        acck("pairing", "in_relu=-3 (any non-zero value) with the affine", {d + "in_relu": -3, d + "in_scale": dev(50), d + "in_shift": dev(51)}),
        acck("pairing", "in_scale with in_shift", {d + "in_scale": dev(50), d + "in_shift": dev(51)}),
        rejk("pairing", "fin_scale without stats", {d + "fin_scale": dev(50), d + "fin_shift": dev(51), d + "fin_counter": dev(52), d + "fin_groups": 1, d + "fin_count": 64.0}),
        rejk("pairing", "fin_scale without fin_shift", {d + "stats": dev(53), d + "fin_scale": dev(50), d + "fin_counter": dev(52), d + "fin_groups": 1, d + "fin_count": 64.0}),
        rejk("pairing", "workspace_bytes without a workspace", {d + "workspace_bytes": 1 << 20, d + "split_k": 2}),
        rejk("alignment", "in + 4 bytes", {d + "in_": dev(SEG_PTRS) + 4}), rejk("alignment", "weight + 4 bytes", {d + "weight": dev(SEG_PTRS + 1) + 4}),
        rejk("reach", "N * Hi * Wi * ld_in past 2^31 elements", {d + "N": 1 << 16, d + "Hi": 1 << 9, d + "Ho": 1 << 9, d + "Wi": 1 << 9, d + "Wo": 1 << 9}),
    ]


E("g6d_conv_igemm", [T("desc", lib.G6dConv, conv_row(), CONV_FIELDS), S()], conv_cases())
E("g6d_conv_igemm_ex", [T("desc", lib.G6dConv, conv_row(), CONV_FIELDS), R("range"), S()],
  conv_cases() + [rejk("pairing", "a range record with math_mode 0", {"range": {}})])
# g6d_conv_plan answers a question about a descriptor (bench.py books FLOPs with it): it launches nothing, dereferences none of the
# descriptor's pointers and documents no validation; the launch validates.  So only the descriptor pointer itself is in its contract.
PLAN_WHY = "g6d_conv_plan launches nothing and reads no operand: the descriptor is validated by g6d_conv_igemm"
PLAN_FIELDS = {f: ("ON" if t is C.c_void_p else ("X", PLAN_WHY)) for f, t in lib.G6dConv._fields_}
E("g6d_conv_plan", [T("desc", lib.G6dConv, conv_row(), PLAN_FIELDS)])
# g6d_conv_route is the launcher's own decision code run without the launch: it dereferences no operand either.  What it answers for a
# descriptor the launch refuses is that refusal (one example below); the rules themselves are stated once, in the launchers' tables above.
ROUTE_WHY = "g6d_conv_route launches nothing and reads no operand: it answers with g6d_conv_igemm's own verdict on the descriptor"
ROUTE_FIELDS = {f: ("ON" if t is C.c_void_p else ("X", ROUTE_WHY)) for f, t in lib.G6dConv._fields_}
E("g6d_conv_route", [T("desc", lib.G6dConv, conv_row(), ROUTE_FIELDS), H("route", C.c_int32, [0] * 8)],
  [rejk("pairing", "in_relu without in_scale: the launcher's refusal", {"desc[0].in_relu": 1}),
   acck("pairing", "in_relu with in_scale and in_shift", {"desc[0].in_relu": 1, "desc[0].in_scale": dev(50), "desc[0].in_shift": dev(51)})])

# ---------------------------------------------------------------------------------------------------------- correlations
WS = [ON("workspace"), X("workspace_bytes", 0, "0 with a NULL workspace disables splitting; any size is meaningful")]
E("g6d_corr2d_patch",
  [P("in", "req"), N("H", 16), N("W", 16), N("Cin", 8), N("ld_in", 8), P("wgt", "req"), N("Cout", 32), I("kh", 7), I("kw", 7), P("out"), N("ld_out", 32),
   *WS, I("math_mode", 0), S()],
  [rej("stride", "ld_in=4 < Cin", ld_in=4), rej("stride", "ld_in=10 off the vector width", ld_in=10), rej("stride", "ld_out=16 < Cout", ld_out=16),
   acc("stride", "ld == C", ld_in=8, ld_out=32), mx("Cout", 32, ld_out=36), acc("extent", "kw=31", kw=31), rej("extent", "kw=33", kw=33),
   rej("mode", "kh even", kh=6), rej("mode", "kw even", kw=6), rej("mode", "math_mode=3", math_mode=3), rej("mode", "math_mode=-1", math_mode=-1),
   acc("mode", "math_mode=2", math_mode=2), rej("extent", "Cin=6 not a multiple of 4", Cin=6),
   rej("reach", "H * W * ld_in = 2^30", H=1 << 14, W=1 << 13), acc("reach", "H * W * ld_in = 2^29", H=1 << 13, W=1 << 13)])


def corr_multi_cases(reach):
    return [rejk("stride", "ld_in=4 < Cin", {"segs[0].ld_in": 4}), rejk("stride", "ld_in off the vector width", {"segs[0].ld_in": 34}),
            rejk("stride", "ld_out=16 < Cout", {"segs[0].ld_out": 16}), mx("nseg", 4)[1], rej("extent", "nseg=0", nseg=0),
            acck("extent", "four maps", {"segs[+++]": {}}), rejk("alignment", "segs[0].in + 4 bytes", {"segs[0].in_": dev(SEG_PTRS) + 4}),
            *seg_reach("segs", reach)]


E("g6d_corr2d_patch_multi",
  [T("segs", lib.G6dCorrSeg, corr_rows(8, 32), CORR_FIELDS), I("nseg", 1), N("Cin", 8), P("wgt", "req"), N("Cout", 32), I("kh", 7), I("kw", 7), *WS,
   I("math_mode", 0), S()],
  corr_multi_cases(30) + [rej("mode", "kh even", kh=6), rej("mode", "kw even", kw=6), rej("extent", "kw=33", kw=33), acc("extent", "kw=31", kw=31),
                          rej("mode", "math_mode=3", math_mode=3), rej("mode", "math_mode=-1", math_mode=-1), mx("Cout", 32)[1]])
E("g6d_corr2d_patch16_multi",
  [T("segs", lib.G6dCorrSeg, corr_rows(32, 32), CORR_FIELDS), I("nseg", 1), N("Cin", 32), P("w16", "req"), N("Cout", 32), I("kh", 7), I("kw", 7), *WS,
   I("math_mode", 2), S()],
  corr_multi_cases(30) + [rej("mode", "kh even", kh=6), rej("mode", "kw even", kw=6), rej("extent", "kw=17", kw=17), acc("extent", "kw=15", kw=15),
                          rej("mode", "math_mode=0", math_mode=0), rej("mode", "math_mode=3", math_mode=3), acc("mode", "math_mode=1", math_mode=1),
                          rej("extent", "Cin=48 not a multiple of 32", Cin=48), mx("Cout", 32)[1]])
E("g6d_corr2d_wino_multi",
  [T("segs", lib.G6dCorrSeg, corr_rows(8, 32), CORR_FIELDS), I("nseg", 1), N("Cin", 8), P("U", "req"), N("Cout", 32), I("kblocks", 5), *WS, S()],
  corr_multi_cases(29) + [rej("mode", "kblocks=3", kblocks=3), rej("mode", "kblocks=0", kblocks=0), rej("extent", "Cin=12 not a multiple of 8", Cin=12),
                          rej("extent", "Cout=48 not a multiple of 32", Cout=48),
                          rejk("stride", "maps with different ld_in", {"segs[+]": {"ld_in": 16}})])
E("g6d_corr2d_wino43_multi",
  [T("segs", lib.G6dCorrSeg, corr_rows(8, 32), CORR_FIELDS), I("nseg", 1), N("Cin", 8), P("U43", "req"), N("Cout", 32), I("kblocks", 5), *WS, S()],
  corr_multi_cases(29) + [acc("mode", "kblocks=3", kblocks=3), rej("mode", "kblocks=4", kblocks=4), rej("mode", "kblocks=0", kblocks=0),
                          rej("extent", "Cin=12 not a multiple of 8", Cin=12), rej("extent", "Cout=48 not a multiple of 32", Cout=48)])

# ---------------------------------------------------------------------------------------------------------- elementwise glue
E("g6d_stats_finalize", [P("stats"), N("n", 8), F("count", 64.0), F("eps", 1e-5), P("scale"), P("shift"), S()],
  [rej("extent", "count=0", count=0.0), rej("extent", "count=-1", count=-1.0), rej("extent", "count=NaN", count=float("nan")),
   rej("reach", "n = 2^31 - 255: the grid's n + 255 leaves an int", n=INT_MAX - 254), acc("reach", "n = 2^31 - 256", n=INT_MAX - 255)])

AFFINE = [O("scale", "req", paired=True), O("shift", "req", paired=True), I("affine_per_n", 0)]
E("g6d_affine_act_pool",
  [P("in", "req"), N("ld_in", 8), *AFFINE, X("relu", 1, FLAG), I("pool", 0), N("N", 2), N("H", 4), N("W", 4), N("C", 8), P("out", "req"), N("ld_out", 8), S()],
  [rej("stride", "ld_in=4 < C=8", ld_in=4), rej("stride", "ld_out=4 < C=8", ld_out=4), rej("stride", "ld_in=10 off the vector width", ld_in=10),
   rej("stride", "ld_out=10 off the vector width", ld_out=10), acc("stride", "ld == C", ld_in=8, ld_out=8), rej("extent", "C=6 not a multiple of 4", C=6),
   rej("mode", "pool=3", pool=3), rej("mode", "pool=-1", pool=-1), acc("mode", "pool=1", pool=1), acc("mode", "pool=2", pool=2),
   rej("mode", "pool=1 on an odd map", pool=1, H=5), rej("mode", "affine_per_n=-1", affine_per_n=-1), acc("mode", "affine_per_n=1", affine_per_n=1),
   rej("pairing", "scale without shift", shift=0), acc("pairing", "neither scale nor shift", scale=0, shift=0),
   rej("reach", "pool=2: H * W = 2^31", pool=2, H=1 << 16, W=1 << 15), acc("reach", "pool=2: H * W = 2^30", pool=2, H=1 << 15, W=1 << 15)])
E("g6d_upsample_bilinear",
  [P("in", "req"), N("ld_in", 8), *AFFINE, N("N", 2), N("H", 4), N("W", 4), N("C", 8), N("factor", 2), P("out", "req"), N("ld_out", 8), S()],
  [rej("stride", "ld_in=4 < C=8", ld_in=4), rej("stride", "ld_out=4 < C=8", ld_out=4), rej("stride", "ld_in=10 off the vector width", ld_in=10),
   rej("stride", "ld_out=10 off the vector width", ld_out=10), acc("stride", "ld == C", ld_in=8, ld_out=8), rej("extent", "C=6 not a multiple of 4", C=6),
   rej("mode", "affine_per_n=-1", affine_per_n=-1), rej("pairing", "scale without shift", shift=0), acc("pairing", "neither scale nor shift", scale=0, shift=0),
   rej("reach", "H * factor = 2^31", H=1 << 16, factor=1 << 15), acc("reach", "H * factor = 2^30", H=1 << 15, factor=1 << 15),
   rej("reach", "W * factor = 2^31", W=1 << 16, factor=1 << 15)])
E("g6d_bias_relu_pool_nchw",
  [P("in", "scalar"), P("bias"), N("N", 2), N("C", 4), N("H", 6), N("W", 6), X("relu", 1, FLAG), X("pool", 1, "a flag: non-zero = 2x2 max-pool"),
   P("out", "scalar"), S()],
  [rej("extent", "pooling a one-row map", H=1), acc("extent", "pooling an odd map (floor)", H=5, W=7)])
E("g6d_l2norm_rows", [P("x", "scalar"), N("rows", 5), N("C", 8), N("ld", 8), S()],
  [rej("stride", "ld=4 < C=8", ld=4), acc("stride", "ld == C", ld=8), acc("stride", "scalar path: ld=7, C=7", ld=7, C=7),
   rej("stride", "vector path with C=6", C=6),
   rej("reach", "rows = 2^31 - 3: the grid's rows + 3 leaves an int", rows=INT_MAX - 2), acc("reach", "rows = 2^31 - 4", rows=INT_MAX - 3)])
E("g6d_nchw_to_nhwc", [P("in"), N("N", 2), N("C", 8), N("H", 4), N("W", 4), X("l2norm", 1, FLAG), P("out", "req"), N("ld_out", 8), S()],
  [rej("stride", "ld_out=4 < C=8", ld_out=4), acc("stride", "ld_out == C", ld_out=8), rej("stride", "l2norm with ld_out=10", ld_out=10),
   acc("stride", "no l2norm: ld_out=10", ld_out=10, l2norm=0), acc("alignment", "no l2norm: out + 4 bytes", out=dev(2) + 4, l2norm=0),
   rej("reach", "N * H * W = 2^31", N=1 << 11, H=1 << 10, W=1 << 10), acc("reach", "N * H * W = 2^30", N=1 << 10, H=1 << 10, W=1 << 10),
   rej("reach", "H * W = 2^31 - 63: the grid's HW + 63 leaves an int", N=1, H=1, W=INT_MAX - 62, l2norm=0),
   rej("reach", "N * H * W = 2^31 - 3 with l2norm: rows + 3 leaves an int", N=1, H=1, W=INT_MAX - 2),
   acc("reach", "H * W = 2^31 - 64", N=1, H=1, W=INT_MAX - 63),
   rej("reach", "C = 2^31 - 63: the grid's C + 63 leaves an int", C=INT_MAX - 62, ld_out=INT_MAX, l2norm=0),
   acc("reach", "C = 2^31 - 64", C=INT_MAX - 63, ld_out=INT_MAX - 63, l2norm=0)])
E("g6d_vps_norm", [P("vps"), N("D", 10), P("feats"), N("ld", 8), I("c_off", 5), N("batch", 1), S()],
  [rej("stride", "ld=7 < c_off + 3", ld=7), acc("stride", "ld == c_off + 3", ld=8, c_off=5), rej("extent", "c_off=-1", c_off=-1),
   rej("extent", "c_off=-5", c_off=-5), acc("extent", "c_off=0", c_off=0), mx("batch", 65535)])
E("g6d_max_an_add", [P("in"), N("ld_in", 8), N("rfn", 3), N("an", 5), N("C", 8), P("embed"), P("out"), N("ld_out", 8), N("batch", 1), S()],
  [rej("stride", "ld_in=1 < C=8", ld_in=1), rej("stride", "ld_out=1 < C=8", ld_out=1), acc("stride", "ld == C", ld_in=8, ld_out=8), mx("batch", 65535),
   rej("reach", "rfn * C = 2^31", rfn=1 << 16, C=1 << 15, ld_in=1 << 15, ld_out=1 << 15),
   acc("reach", "rfn * C = 2^30", rfn=1 << 15, C=1 << 15, ld_in=1 << 15, ld_out=1 << 15),
   rej("reach", "rfn * an = 2^31", rfn=1 << 16, an=1 << 15, C=4)])
E("g6d_attention", [P("q"), P("k"), P("v"), N("ld", 8), N("n", 5), N("C", 8), N("heads", 2), P("out"), N("ld_out", 8), N("batch", 1), S()],
  [rej("stride", "ld=4 < C=8", ld=4), rej("stride", "ld_out=4 < C=8", ld_out=4), acc("stride", "ld == C", ld=8, ld_out=8), mx("batch", 65535),
   rej("extent", "C=9 not a multiple of heads", C=9, ld=12, ld_out=12),
   rej("reach", "n * heads = 2^31", n=1 << 11, heads=1 << 20, C=1 << 20, ld=1 << 20, ld_out=1 << 20),
   acc("reach", "n * heads = 2^30", n=1 << 10, heads=1 << 20, C=1 << 20, ld=1 << 20, ld_out=1 << 20),
   rej("extent", "(C / heads + n) floats past the 60000-byte LDS bound", n=14997), acc("extent", "(C / heads + n) floats at the LDS bound", n=14996)])
E("g6d_layernorm", [P("in"), N("ld_in", 8), N("n", 5), N("C", 8), P("gamma"), P("beta"), F("eps", 1e-5), P("out"), N("ld_out", 8), S()],
  [rej("stride", "ld_in=1 < C=8", ld_in=1), rej("stride", "ld_out=1 < C=8", ld_out=1), acc("stride", "ld == C", ld_in=8, ld_out=8)])
E("g6d_affine_act_add",
  [P("in"), N("ld_in", 8), O("scale", paired=True), O("shift", paired=True), X("relu", 1, FLAG), O("residual"), I("ld_res", 8), N("n", 6), N("C", 8), P("out"), N("ld_out", 8),
   I("rows_per_group", 0), S()],
  [rej("stride", "ld_in=4 < C=8", ld_in=4), rej("stride", "ld_out=4 < C=8", ld_out=4), rej("stride", "ld_res=4 < C=8", ld_res=4),
   acc("stride", "ld == C", ld_in=8, ld_out=8, ld_res=8), acc("stride", "ld_res=0 without a residual", residual=0, ld_res=0),
   rej("pairing", "scale without shift", shift=0), acc("pairing", "neither scale nor shift", scale=0, shift=0),
   rej("mode", "rows_per_group=-1", rows_per_group=-1), acc("mode", "rows_per_group=3", rows_per_group=3),
   rej("reach", "n * C = 2^32", n=1 << 20, C=1 << 12, ld_in=1 << 12, ld_out=1 << 12, ld_res=1 << 12),
   rej("reach", "n * C = 2^31", n=1 << 19, C=1 << 12, ld_in=1 << 12, ld_out=1 << 12, ld_res=1 << 12),
   rej("reach", "n * C = 2^31 - 255: the grid's n * C + 255 leaves an int", n=1, C=INT_MAX - 254, ld_in=INT_MAX, ld_out=INT_MAX, ld_res=INT_MAX),
   acc("reach", "n * C = 2^31 - 256", n=1, C=INT_MAX - 255, ld_in=INT_MAX, ld_out=INT_MAX, ld_res=INT_MAX),
   acc("reach", "n * C = 2^30", n=1 << 18, C=1 << 12, ld_in=1 << 12, ld_out=1 << 12, ld_res=1 << 12)])
GEMV = [P("x", "req"), N("B", 2), N("K", 8), P("W", "req"), O("bias"), N("O", 4), I("act", 0), P("out")]
GEMV_CASES = [rej("extent", "K=6 not a multiple of 4", K=6), rej("mode", "act=3", act=3), rej("mode", "act=-1", act=-1), acc("mode", "act=2", act=2)]
E("g6d_linear_gemv", [*GEMV, S()], GEMV_CASES + [mx("B", 8)])
E("g6d_linear_gemv_batch", [*GEMV, *WS, S()],
  GEMV_CASES + [acc("extent", "B=33", B=33), acc("pairing", "a workspace too small for the split routes: the row-per-block kernel", B=4, K=4096, O=8,
                                                       workspace=dev(30), workspace_bytes=16)])

# ---------------------------------------------------------------------------------------------------------- first trunk layer
CONV1 = [P("in"), N("N", 1), I("H", 8), I("W", 8), P("w_oihw"), P("bias"), I("Cin", 3), I("Cout", 64)]
CONV1_CASES = [rej("extent", "H=1", H=1), rej("extent", "W=1", W=1), rej("extent", "H=0", H=0), rej("extent", "W=-1", W=-1), acc("extent", "H=W=2", H=2, W=2),
               acc("extent", "odd sizes (floor)", H=7, W=9), rej("mode", "Cin=4", Cin=4), rej("mode", "Cout=32", Cout=32), mx("N", 65535)]
MEAN_STD = [HO("mean_host", C.c_float, [0.485, 0.456, 0.406]), HO("std_host", C.c_float, [0.229, 0.224, 0.225])]
E("g6d_vgg_conv1_pool", [*CONV1, P("out"), S()], CONV1_CASES)
E("g6d_vgg_conv1_pool_nhwc", [*CONV1, P("out"), S()], CONV1_CASES)
E("g6d_vgg_conv1_pool_nhwc_norm", [*CONV1, H("mean_host", C.c_float, [0.485, 0.456, 0.406]), H("std_host", C.c_float, [0.229, 0.224, 0.225]), P("out"), S()],
  CONV1_CASES)
CONV1_16 = CONV1_CASES + [rej("mode", "math_mode=0", math_mode=0), rej("mode", "math_mode=4", math_mode=4), acc("mode", "math_mode=1", math_mode=1),
                          acc("mode", "math_mode=3", math_mode=3), rej("reach", "N * 64 * (H/2) * (W/2) = 2^30", N=1, H=1 << 13, W=1 << 13),
                          acc("reach", "N * 64 * (H/2) * (W/2) = 2^29", N=1, H=1 << 13, W=1 << 12)]
E("g6d_vgg_conv1_pool_nhwc16", [*CONV1, *MEAN_STD, P("out16"), I("math_mode", 2), S()], CONV1_16)
E("g6d_vgg_conv1_pool_nhwc16_ex", [*CONV1, *MEAN_STD, P("out16"), I("math_mode", 2), R("range"), S()], CONV1_16)

# ---------------------------------------------------------------------------------------------------------- 16-bit direct kernels
C16 = [I("nseg", 1), N("Cin", 64), P("W16", "req"), I("w_layout", 0)]
C16_TAIL = [ON("bias"), N("Cout", 128), I("kd", 1)]
C16_TYPES = [I("full_type", 1), I("pool_type", 0), I("math_mode", 2), ON("stats"), X("stat_rows_per_group", 0, "not read while stats is NULL (the baseline)")]


def c16_cases():
    return [rej("extent", "nseg=0", nseg=0), rej("extent", "nseg=5", nseg=5), acck("extent", "four segments", {"segs[+++]": {}}),
            rejk("stride", "ld_in=32 < Cin=64", {"segs[0].ld_in": 32}), rejk("stride", "ld_full=64 < Cout=128", {"segs[0].ld_full": 64}),
            rejk("stride", "ld_in=68: rows off 16 bytes", {"segs[0].ld_in": 68}), rejk("alignment", "segs[0].in + 4 bytes", {"segs[0].in_": dev(SEG_PTRS) + 4}),
            rej("extent", "Cin=32 not a multiple of 64", Cin=32), rej("extent", "Cout=96", Cout=96), rej("mode", "kd=2", kd=2), rej("mode", "kd=0", kd=0),
            rej("mode", "w_layout=2", w_layout=2), rej("mode", "w_layout=-1", w_layout=-1), rej("mode", "math_mode=0", math_mode=0),
            rej("mode", "math_mode=4", math_mode=4), acc("mode", "math_mode=1", math_mode=1), rej("mode", "full_type=4", full_type=4),
            rej("mode", "full_type=-1", full_type=-1), rej("mode", "full_type=3 outside math_mode 3", full_type=3), acc("mode", "full_type=2", full_type=2),
            rej("mode", "pool_type=4", pool_type=4), rej("pairing", "pool_type=1 without out_pool", pool_type=1),
            rejk("pairing", "no output at all", {"segs[0].out_full": 0, "full_type": 0}),
            rejk("mode", "segments with different D", {"segs[+]": {"D": 3}, "kd": 3})]


E("g6d_conv16_direct_multi", [T("segs", lib.G6dConv16Seg, c16_rows(64, 128), C16_FIELDS), *C16, F("acc_scale", 0.0), *C16_TAIL, X("relu", 1, FLAG), *C16_TYPES, S()],
  c16_cases())
E("g6d_conv16_direct_multi_ex",
  [T("segs", lib.G6dConv16Seg, c16_rows(64, 128), C16_FIELDS), *C16, F("acc_scale", 0.0), *C16_TAIL, X("relu", 1, FLAG), *C16_TYPES, R("range"), S()], c16_cases())
E("g6d_conv16_direct_plan", [T("segs", lib.G6dConv16Seg, c16_rows(64, 128), C16_FIELDS), *C16, *C16_TAIL[1:], *C16_TYPES], c16_cases())
# g6d_conv16_direct_route is g6d_conv16_direct_plan with the whole choice written out: the same decision code, so the same refusals; it launches
# nothing and reads no operand (the pointers are only tested for NULL and alignment, as the launch tests them), and it needs its out struct.
E("g6d_conv16_direct_route", [T("segs", lib.G6dConv16Seg, c16_rows(64, 128), C16_FIELDS), *C16, *C16_TAIL[1:], *C16_TYPES, H("route", C.c_int32, [0] * 34)],
  c16_cases())


def corr16_cases():
    return [rej("extent", "nseg=0", nseg=0), rej("extent", "nseg=5", nseg=5), rejk("stride", "ld_in=16 < Cin=32", {"segs[0].ld_in": 16}),
            rejk("stride", "ld_full=16 < 32", {"segs[0].ld_full": 16}), rejk("alignment", "segs[0].in + 4 bytes", {"segs[0].in_": dev(SEG_PTRS) + 4}),
            rejk("null", "segs[0].out_full NULL (required here)", {"segs[0].out_full": 0}), rejk("mode", "D=2", {"segs[0].D": 2}),
            rej("extent", "Cin=48 not a multiple of 32", Cin=48), rej("mode", "Cout=64", Cout=64), rej("mode", "k=9", k=9), rej("mode", "k=0", k=0),
            acc("mode", "k=15", k=15), rej("mode", "math_mode=0", math_mode=0), rej("mode", "math_mode=4", math_mode=4), acc("mode", "math_mode=1", math_mode=1)]


CORR16 = [T("segs", lib.G6dConv16Seg, c16_rows(32, 32, 16), C16_FIELDS), I("nseg", 1), N("Cin", 32), P("W16", "req"), F("acc_scale", 1.0), I("Cout", 32), I("k", 7),
          I("math_mode", 2)]
E("g6d_corr16_multi", [*CORR16, S()], corr16_cases())
E("g6d_corr16_multi_ex", [*CORR16, R("range"), S()], corr16_cases())

# ---------------------------------------------------------------------------------------------------------- split16 hand-over passes
PROD = [P("ref", "req"), P("que", "req"), P("scale", "req"), P("shift", "req"), P("out", "req"), N("qn", 2), N("D", 3), N("P", 16), N("C", 8), I("math_mode", 3)]
MM13 = [rej("mode", "math_mode=0", math_mode=0), rej("mode", "math_mode=4", math_mode=4), acc("mode", "math_mode=1", math_mode=1), acc("mode", "math_mode=2", math_mode=2)]
PROD_CASES = MM13 + [rej("extent", "C=12 not a multiple of 8", C=12)]
E("g6d_product_split16", [*PROD, S()], PROD_CASES)
E("g6d_product_split16_ex", [*PROD, R("range"), S()], PROD_CASES)
AFS = [P("in", "req"), N("ld_in", 8), *AFFINE, X("relu", 1, FLAG), X("pool", 0, "a flag: non-zero = 2x2 max-pool"), N("N", 2), N("H", 4), N("W", 4), N("C", 8),
       P("out", "req")]
AFS_CASES = MM13 + [rej("stride", "ld_in=4 < C=8", ld_in=4), rej("stride", "ld_in=10 off the vector width", ld_in=10), acc("stride", "ld_in == C", ld_in=8),
                    rej("extent", "C=12 not a multiple of 8", C=12, ld_in=12), rej("mode", "pooling an odd map", pool=1, H=5),
                    rej("mode", "affine_per_n=-1", affine_per_n=-1), rej("pairing", "scale without shift", shift=0),
                    acc("pairing", "neither scale nor shift", scale=0, shift=0)]
E("g6d_affine_split16", [*AFS, I("math_mode", 3), S()], AFS_CASES)
E("g6d_affine_split16_ex", [*AFS, I("math_mode", 3), R("range"), S()], AFS_CASES)
SLICE = [N("ld_out", 48), I("plane", 24), I("c_off", 8)]
SLICE_CASES = [rej("stride", "plane + c_off + C = 40 > ld_out = 32", ld_out=32), acc("stride", "plane + c_off + C == ld_out", ld_out=40),
               rej("stride", "ld_out=44 not a multiple of 8", ld_out=44), rej("stride", "plane=20 not a multiple of 8", plane=20),
               rej("stride", "plane=8 < c_off + C", plane=8), acc("stride", "plane == c_off + C", plane=16), rej("stride", "c_off=4 not a multiple of 8", c_off=4),
               rej("extent", "c_off=-8", c_off=-8), acc("extent", "c_off=0", c_off=0),
               rej("stride", "one plane: c_off + C = 16 > ld_out = 8", math_mode=2, ld_out=8), acc("stride", "one plane: c_off + C == ld_out", math_mode=2, ld_out=16)]
E("g6d_affine_split16_to", [*AFS, *SLICE, I("math_mode", 3), R("range"), S()], AFS_CASES + SLICE_CASES)
E("g6d_upsample_bilinear_split16",
  [P("in", "req"), N("ld_in", 8), *AFFINE, N("N", 2), N("H", 4), N("W", 4), N("C", 8), N("factor", 2), P("out", "req"), *SLICE, I("math_mode", 3), R("range"), S()],
  [c for c in AFS_CASES if "pool" not in c[3]] + SLICE_CASES + [rej("reach", "H * factor = 2^31", H=1 << 16, factor=1 << 15)])
E("g6d_l2norm_split16", [P("in", "req"), N("ld_in", 256), N("rows", 5), I("C", 256), P("out", "req"), I("math_mode", 3), R("range"), S()],
  MM13 + [rej("reach", "rows = 2^31 - 3: the grid's rows + 3 leaves an int", rows=INT_MAX - 2), acc("reach", "rows = 2^31 - 4", rows=INT_MAX - 3),
          rej("stride", "ld_in=128 < C=256", ld_in=128), rej("stride", "ld_in=258 off the vector width", ld_in=258), acc("stride", "ld_in == C", ld_in=256),
          rej("mode", "C=128", C=128), rej("mode", "C=0", C=0), acc("mode", "C=512", C=512, ld_in=512)])

# ---------------------------------------------------------------------------------------------------------- Winograd family
WINO_OUT = [rejk("pairing", "neither out_full nor out_pool", {"segs[0].out_full": 0}),
            acck("pairing", "out_pool only", {"segs[0].out_full": 0, "segs[0].out_pool": dev(SEG_PTRS + 2), "segs[0].ld_pool": 64}),
            rejk("stride", "ld_pool=32 < Cout", {"segs[0].out_pool": dev(SEG_PTRS + 2), "segs[0].ld_pool": 32}),
            rejk("extent", "pooling a one-row map", {"segs[0].out_pool": dev(SEG_PTRS + 2), "segs[0].ld_pool": 64, "segs[0].H": 1}),
            rejk("pairing", "segments with different kinds of output", {"segs[+]": {"out_pool": dev(SEG_PTRS + 2), "ld_pool": 64}})]


def wino_multi_cases(cin):
    return [rej("extent", "nseg=0", nseg=0), rej("extent", "nseg=5", nseg=5), acck("extent", "four segments", {"segs[+++]": {}}),
            rejk("stride", "ld_in < Cin", {"segs[0].ld_in": cin - 4}), rejk("stride", "ld_in off the vector width", {"segs[0].ld_in": cin + 2}),
            rejk("stride", "ld_full=32 < Cout=64", {"segs[0].ld_full": 32}), rejk("alignment", "segs[0].in + 4 bytes", {"segs[0].in_": dev(SEG_PTRS) + 4}),
            rej("extent", "Cin off the chunk size", Cin=cin + 4), rej("extent", "Cout=96 not a multiple of 64", Cout=96), *seg_reach("segs", 29), *WINO_OUT]


WINO_TAIL = [ON("bias"), N("Cout", 64), X("relu", 1, FLAG)]
E("g6d_wino_conv3x3",
  [P("in", "req"), N("N", 1), N("H", 8), N("W", 8), N("Cin", 8), N("ld_in", 8), P("U", "req"), *WINO_TAIL, O("out_full", paired=True), N("ld_full", 64), ON("out_pool"),
   X("ld_pool", 0, "not read while out_pool is NULL (the baseline); its own case sets out_pool"), *WS, S()],
  [rej("stride", "ld_in=4 < Cin=8", ld_in=4), rej("stride", "ld_in=10 off the vector width", ld_in=10), rej("stride", "ld_full=32 < Cout", ld_full=32),
   acc("stride", "ld == C", ld_in=8, ld_full=64), rej("extent", "Cin=12 not a multiple of 8", Cin=12, ld_in=12), rej("extent", "Cout=96", Cout=96, ld_full=96),
   rej("pairing", "neither out_full nor out_pool", out_full=0), acc("pairing", "out_pool only", out_full=0, out_pool=dev(20), ld_pool=64),
   rej("stride", "ld_pool=32 < Cout", out_pool=dev(20), ld_pool=32), rej("extent", "pooling a one-row map", out_pool=dev(20), ld_pool=64, H=1),
   rej("reach", "N * H * W * ld_in = 2^29", N=1 << 6, H=1 << 10, W=1 << 10), acc("reach", "N * H * W * ld_in = 2^28", N=1 << 5, H=1 << 10, W=1 << 10)])
E("g6d_wino_conv3x3_multi", [T("segs", lib.G6dWinoSeg, wino_rows(8, 64), WINO_FIELDS), I("nseg", 1), N("Cin", 8), P("U", "req"), *WINO_TAIL, *WS, S()],
  wino_multi_cases(8))
E("g6d_wino16_conv3x3_multi",
  [T("segs", lib.G6dWinoSeg, wino_rows(16, 64), WINO_FIELDS), I("nseg", 1), N("Cin", 16), P("U16", "req"), *WINO_TAIL, I("math_mode", 2), *WS, S()],
  wino_multi_cases(16) + [rej("mode", "math_mode=0", math_mode=0), rej("mode", "math_mode=3", math_mode=3), acc("mode", "math_mode=1", math_mode=1)])
E("g6d_wino43_conv3x3_multi", [T("segs", lib.G6dWinoSeg, wino_rows(8, 64), WINO_FIELDS), I("nseg", 1), N("Cin", 8), P("U43", "req"), *WINO_TAIL, *WS, S()],
  wino_multi_cases(8))
# g6d_wino_multi_route is the entry points' own argument checks, segment table and plan run without the launch: the same refusals as the
# launch `entry` stands for (baseline: 0 = g6d_wino_conv3x3_multi), nothing launched and no operand read, and it needs its out struct.  The
# G6dCorrSeg tables of entries 4 and 5 are issued by tests/test_wino_sweep_cpu.py (every correlation case, and the kblocks = 3 probe).
E("g6d_wino_multi_route",
  [I("entry", 0), T("segs", lib.G6dWinoSeg, wino_rows(8, 64), WINO_FIELDS), I("nseg", 1), N("Cin", 8), P("U", "req"), N("Cout", 64),
   X("kblocks", 0, "read for entries 4 and 5 only (G6dCorrSeg tables: tests/test_wino_sweep_cpu.py issues them, kblocks = 3 refused on entry 4)"),
   I("math_mode", 0), *WS, H("route", C.c_int64, [0] * 13)],
  wino_multi_cases(8) + [rej("mode", "entry=-1", entry=-1), rej("mode", "entry=6", entry=6), acc("mode", "entry=3: F(4x4,3x3)", entry=3),
                         acc("mode", "entry=1: the one-map launch on a one-row table", entry=1), rej("extent", "entry=1 with two rows", entry=1, nseg=2),
                         rejk("reach", "entry=1: N * H * W * ld_in = 2^29", {"entry": 1, "segs[0].N": 1 << 6, "segs[0].H": 1 << 10, "segs[0].W": 1 << 10}),
                         rejk("mode", "entry=2 with math_mode=0", {"entry": 2, "Cin": 16, "segs[0].ld_in": 16, "math_mode": 0}),
                         rejk("mode", "entry=2 with math_mode=3", {"entry": 2, "Cin": 16, "segs[0].ld_in": 16, "math_mode": 3}),
                         acck("mode", "entry=2 with math_mode=1", {"entry": 2, "Cin": 16, "segs[0].ld_in": 16, "math_mode": 1}),
                         rej("extent", "entry=2 with Cin=8 off the 16-channel chunk", entry=2, math_mode=2)])

# ---------------------------------------------------------------------------------------------------------- selector
SEL =[N("D", 6), N("HW", 16), N("C", 8)]
E("g6d_selector_ref_sums", [P("refs"), *SEL, P("r1"), P("r2"), S()],
  [rej("reach", "HW * C = 2^32", HW=1 << 16, C=1 << 16), rej("reach", "HW * C = 2^31", HW=1 << 16, C=1 << 15), acc("reach", "HW * C = 2^30", HW=1 << 15, C=1 << 15)])
E("g6d_selector_prod_affine", [P("que"), P("r1"), P("r2"), *SEL, F("eps", 1e-5), P("scale"), P("shift"), S()],
  [rej("reach", "C = 2^31 - 63: the grid's C + 63 leaves an int", C=INT_MAX - 62), acc("reach", "C = 2^31 - 64", C=INT_MAX - 63)])
E("g6d_selector_scan", [P("que", "req"), P("refs", "req"), *SEL, P("score_map"), P("vps"), S()],
  [rej("extent", "C=6 not a multiple of 4", C=6), rej("reach", "D * HW = 2^30 + 1 rows", D=(1 << 15) + 1, HW=1 << 15), rej("reach", "D * HW = 2^31", D=1 << 16, HW=1 << 15),
   acc("reach", "D * HW = 2^30", D=1 << 15, HW=1 << 15)])
LEV = [dev(40 + i) for i in range(18)]
E("g6d_selector_levels",
  [I("nlev", 3), N("qn", 2), H("que", C.c_void_p, LEV[0:3]), H("refs", C.c_void_p, LEV[3:6]), H("r1", C.c_void_p, LEV[6:9]), H("r2", C.c_void_p, LEV[9:12]),
   H("HW", C.c_int, [64, 16, 4]), N("D", 6), N("Dg", 6), N("C", 8), F("eps", 1e-5), H("score_maps", C.c_void_p, LEV[12:15]), P("vps"), P("scale"), P("shift"), S()],
  [rej("extent", "nlev=0", nlev=0), rej("extent", "nlev=-1", nlev=-1), mx("nlev", 3)[1], acc("extent", "nlev=1", nlev=1), mx("qn", 8),
   rejk("extent", "HW[1]=1025", {"HW[1]": 1025}), acck("extent", "HW[1]=1024", {"HW[1]": 1024}), rejk("extent", "HW[2]=0", {"HW[2]": 0}),
   rejk("extent", "HW[0]=-1", {"HW[0]": -1}), rej("extent", "C=6 not a multiple of 4", C=6),
   *[rejk("null", f"{n}[1] NULL", {f"{n}[1]": 0}) for n in ("que", "refs", "r1", "r2", "score_maps")],
   rejk("alignment", "que[0] + 4 bytes", {"que[0]": LEV[0] + 4}), rejk("alignment", "refs[2] + 4 bytes", {"refs[2]": LEV[5] + 4}),
   rejk("reach", "D * HW[0] = 2^30 + 2^10", {"D": (1 << 20) + 1, "Dg": (1 << 20) + 1, "HW[0]": 1024}),
   acck("reach", "D * HW[0] = 2^30", {"D": 1 << 20, "Dg": 1 << 20, "HW[0]": 1024}),
   rejk("reach", "D = 2^30 with HW = 1, 1, 1: D * parts over the levels and qn * nlev * D leave an int", {"D": 1 << 30, "Dg": 1 << 30, "HW": [1, 1, 1]}),
   rejk("reach", "qn * nlev * D + 3 = 2^31 + 2", {"qn": 8, "D": (1 << 28) // 3 + 1, "Dg": 1 << 27, "HW": [1, 1, 1]}),
   acck("reach", "D = 2^26 with HW = 1, 1, 1", {"D": 1 << 26, "Dg": 1 << 26, "HW": [1, 1, 1]})])

# ---------------------------------------------------------------------------------------------------------- refiner volume
VOL = [N("rfn", 5), N("fh", 8), N("fw", 8), N("C", 8), N("h_in", 32), N("w_in", 32), N("sn", 4)]
VOL_CASES = [mx("rfn", 8), mx("sn", 256), rej("extent", "C=6 not a multiple of 4", C=6),
             rej("reach", "fh * fw * C = 2^32", fh=1 << 12, fw=1 << 12, C=1 << 8), rej("reach", "fh * fw * C = 2^31: the tap offsets are ints", fh=1 << 12, fw=1 << 11, C=1 << 8),
             acc("reach", "fh * fw * C = 2^30", fh=1 << 11, fw=1 << 11, C=1 << 8)]
E("g6d_refiner_volume", [P("feats", "req"), P("projs"), P("rot_in"), P("lin"), *VOL, P("mean_in", "req"), P("std", "req"), S()], VOL_CASES)
KP = [P("feats", "req"), P("ref_Ks"), P("ref_poses"), P("K_in"), P("pose_in"), P("lin"), *VOL]
E("g6d_refiner_volume_kp", [*KP, P("mean_in", "req"), P("stdv", "req"), N("batch", 1), S()], VOL_CASES + [mx("batch", 65535)])
E("g6d_refiner_volume_kp_pairs", [*KP, P("mean_in16", "req"), P("std16", "req"), N("batch", 1), R("range_mean"), R("range_std"), S()],
  VOL_CASES + [mx("batch", 65535)])

# ---------------------------------------------------------------------------------------------------------- detector
E("g6d_detector_assemble",
  [P("s0"), P("s1"), P("s2"), N("hc", 8), N("wc", 8), N("rfn", 4), H("mu_sigma", C.c_float, [0, 1, 0, 1, 0, 1]), F("clip", 3.0), N("hs", 8), N("ws", 8),
   I("scale_idx", 3), I("nch", 12), P("stacked"), N("batch", 1), S()],
  [rej("extent", "hc=6 not a multiple of 4", hc=6), rej("extent", "wc=10 not a multiple of 4", wc=10), rej("mode", "scale_idx=-1", scale_idx=-1),
   rej("mode", "scale_idx=4 with nch=12", scale_idx=4), acc("mode", "scale_idx=0", scale_idx=0), rej("mode", "nch=11 with scale_idx=3", nch=11),
   rej("mode", "nch=0", nch=0), mx("batch", 65535), rej("reach", "hs * ws = 2^32", hs=1 << 16, ws=1 << 16, rfn=1),
   rej("reach", "hs * ws = 2^31: the kernel's pixel index is an int", hs=1 << 16, ws=1 << 15, rfn=1), acc("reach", "hs * ws = 2^30", hs=1 << 15, ws=1 << 15, rfn=1),
   rej("reach", "hs * ws * rfn = 2^40: more than 2^31 - 1 blocks of 256", hs=1 << 15, ws=1 << 15, rfn=1 << 10),
   acc("reach", "hs * ws * rfn = 2^38", hs=1 << 15, ws=1 << 15, rfn=1 << 8)])
E("g6d_detector_score_mlp_max", [P("stacked"), N("P", 10), N("rfn", 4), I("nch", 12), P("w0"), P("b0"), P("w1"), P("b1"), P("out"), S()],
  [mx("rfn", 256), rej("mode", "nch=9", nch=9), rej("mode", "nch=15", nch=15),
   rej("reach", "P = 2^31 - 255: the grid's P + ppb - 1 may leave an int", P=INT_MAX - 254), acc("reach", "P = 2^31 - 256", P=INT_MAX - 255)])
E("g6d_detector_decode",
  [P("scores"), N("ld_s", 1), P("offset"), I("ld_o", 2), P("scale"), N("ld_c", 1), N("hs", 6), N("ws", 7), X("pool_ratio", 8, "a scale factor of the result"),
   P("result"), N("batch", 1), S()],
  [rej("stride", "ld_o=1 < 2", ld_o=1), rej("stride", "ld_o=0", ld_o=0), rej("stride", "ld_o=-1", ld_o=-1), acc("stride", "densest strides 1, 2, 1", ld_s=1, ld_o=2, ld_c=1),
   rej("reach", "hs * ws = 2^32", hs=1 << 16, ws=1 << 16), rej("reach", "hs * ws = 2^31", hs=1 << 16, ws=1 << 15), acc("reach", "hs * ws = 2^30", hs=1 << 15, ws=1 << 15)])
E("g6d_resize_bilinear_pyramid",
  [P("src"), N("planes", 3), N("H", 16), N("W", 16), I("nscale", 2), H("hs", C.c_int, [8, 12]), H("ws", C.c_int, [8, 12]),
   H("dsts", C.c_void_p, [dev(40), dev(41)]), S()],
  [rej("extent", "nscale=0", nscale=0), rej("extent", "nscale=-1", nscale=-1), rejk("extent", "nscale=5", {"nscale": 5, "hs": [8] * 5, "ws": [8] * 5, "dsts": [dev(40 + i) for i in range(5)]}),
   acck("extent", "nscale=4", {"nscale": 4, "hs": [8] * 4, "ws": [8] * 4, "dsts": [dev(40 + i) for i in range(4)]}),
   rejk("extent", "hs[1]=0", {"hs[1]": 0}), rejk("extent", "ws[0]=-1", {"ws[0]": -1}), rejk("null", "dsts[1] NULL", {"dsts[1]": 0}),
   acck("alignment", "dsts[0] + 4 bytes (scalar path)", {"dsts[0]": dev(40) + 4}),
   rejk("reach", "2^32 work items", {"planes": 1 << 12, "hs[0]": 1 << 12, "ws[0]": 1 << 12})])
E("g6d_zero_bytes", [P("ptr", "req"), X("bytes", 64, "a byte count: any value is meaningful, 0 included"), S()], [acc("extent", "bytes=0", bytes=0)])

# ---------------------------------------------------------------------------------------------------------- warps and the chain
E("g6d_warp_perspective",
  [P("src"), N("sh", 8), N("sw", 8), N("ch", 3), H("hinv", C.c_float, [1, 0, 0, 0, 1, 0, 0, 0, 1]), P("dst"), N("dh", 6), N("dw", 6), X("out_float", 1, FLAG),
   F("out_scale", 1.0), S()],
  [mx("ch", 4), rej("reach", "dh * dw = 2^32", dh=1 << 16, dw=1 << 16), rej("reach", "dh * dw = 2^31", dh=1 << 16, dw=1 << 15), acc("reach", "dh * dw = 2^30", dh=1 << 15, dw=1 << 15)])
E("g6d_warp_batch", [O("stack", paired=True), O("single", paired=True), O("idx", paired=True), N("B", 2), N("sh", 8), N("sw", 8), N("ch", 3), P("hinv"), P("dst"), N("dh", 6), N("dw", 6), S()],
  [mx("ch", 4), rej("pairing", "neither stack nor single", stack=0, single=0, idx=0), rej("pairing", "stack without idx and without single", single=0, idx=0), acc("pairing", "single alone", stack=0, idx=0), acc("pairing", "stack and idx, no single", single=0),
   rej("reach", "dh * dw = 2^31", dh=1 << 16, dw=1 << 15), acc("reach", "dh * dw = 2^30", dh=1 << 15, dw=1 << 15)])
E("g6d_chain_crop_from_detection", [P("det"), F("size", 128.0), P("hinv"), N("batch", 1), S()], [rej("extent", "size=0", size=0.0), rej("extent", "size=-1", size=-1.0), rej("extent", "size=NaN", size=float("nan"))])
E("g6d_chain_pose_from_selection",
  [P("det"), P("logits"), P("angles"), N("rfn", 4), P("ref_poses"), P("ref_Ks"), P("que_K"), P("center"), P("pose_out"), P("sel_out"), N("batch", 1), S()])
E("g6d_chain_refine_prepare",
  [P("pose_in"), P("que_K"), P("norm"), F("size", 128.0), F("margin", 0.05), P("sub_poses"), P("sub_Ks"), N("n_sub", 16), N("ref_num", 6), P("geo"), P("ref_idx"),
   F("angle_step", 0.0), O("ref_bucket"), N("batch", 1), S()],
  [mx("n_sub", 128), mx("ref_num", 8), rej("extent", "ref_num > n_sub", n_sub=4, ref_num=5), acc("extent", "ref_num == n_sub", n_sub=4, ref_num=4),
   rej("extent", "size=0", size=0.0), rej("extent", "size=NaN", size=float("nan"))])
E("g6d_chain_refine_update", [P("rot"), P("off"), P("scl"), P("geo"), I("geo_floats", 222), P("norm"), P("pose_out"), N("batch", 1), S()],
  [rej("extent", "geo_floats=32: shorter than K_warp | pose_warp | pose_rect", geo_floats=32), acc("extent", "geo_floats=33", geo_floats=33),
   rej("extent", "geo_floats=0", geo_floats=0), rej("extent", "geo_floats=-1", geo_floats=-1)])

# ---------------------------------------------------------------------------------------------------------- tracking
E("g6d_track_gather", [P("pose_table"), P("slot_stream"), P("parking_pose"), P("pose_out"), N("batch", 2), S()])
E("g6d_track_commit",
  [P("pose"), P("K"), P("slot_stream"), X("reset", 0, FLAG), P("box"), N("num", 8), F("std", 2.0), P("pose_table"), P("hist"), P("hist_count"), P("smooth_table"),
   P("out"), N("batch", 2), S()],
  [mx("num", 64), rej("extent", "std=0", std=0.0), rej("extent", "std=-1", std=-1.0), rej("extent", "std=NaN", std=float("nan"))])
BATCH64 = [rej("reach", "batch = 2^31 - 63: the grid's batch + 63 leaves an int", batch=INT_MAX - 62), acc("reach", "batch = 2^31 - 64", batch=INT_MAX - 63)]
E("g6d_track_gate", [P("pose_table"), P("health"), P("slot_stream"), P("slot_eff"), N("batch", 2), S()], BATCH64)
GATES = [F("min_px", 8.0), F("max_px", 4.0), F("margin", 0.5), F("max_rot_deg", 30.0), F("max_shift", 0.5), F("max_log2_scale", 0.5)]
E("g6d_track_health",
  [O("pose_prev", paired=True), P("pose_new"), P("K"), O("pic"), I("W", 640), I("H", 480), P("slot_eff"), X("reset", 0, FLAG), P("center"), F("diameter", 0.2), N("patience", 3),
   *GATES, P("health"), P("measures"), P("slot_commit"), P("slot_draw"), N("batch", 2), S()],
  [rej("pairing", "no pose_prev without reset", pose_prev=0), acc("pairing", "no pose_prev with reset", pose_prev=0, reset=1),
   rej("pairing", "no pic and W=0", pic=0, W=0), rej("pairing", "no pic and H=-1", pic=0, H=-1), acc("pairing", "pic given: W, H not read", W=0, H=0),
   acc("pairing", "no pic, W and H >= 1", pic=0, W=1, H=1), rej("extent", "diameter=0", diameter=0.0), rej("extent", "diameter=NaN", diameter=float("nan")), *BATCH64])
E("g6d_track_verify",
  [P("det"), P("pose_table"), P("K"), P("slot_commit"), P("center"), F("diameter", 0.2), F("ref_px", 80.0), F("verify_shift", 0.5), F("verify_log2_scale", 0.5),
   N("verify_patience", 2), P("health"), P("measures"), N("batch", 2), S()],
  [rej("extent", "diameter=0", diameter=0.0), rej("extent", "ref_px=0", ref_px=0.0), rej("extent", "ref_px=NaN", ref_px=float("nan")), *BATCH64])
E("g6d_track_corners", [P("table"), P("K"), P("slot_stream"), P("box"), P("pts"), P("valid"), N("batch", 2), S()])

# ---------------------------------------------------------------------------------------------------------- frames (tables in DEVICE memory: fake)
CANVAS = [N("B", 2), N("H", 128), N("W", 128)]
TILES = [rej("reach", "tiles * n past 2^31 - 1", n=1 << 20, H=8192, W=8192), acc("reach", "tiles * n = 2^30", n=1 << 14, H=8192, W=8192),
         rej("reach", "H = W = 2^21: the tile count itself leaves an int", n=1, H=1 << 21, W=1 << 21), rej("reach", "W = 2^31 - 1", n=1, H=16, W=INT_MAX),
         acc("reach", "H = W = 2^19", n=1, H=1 << 19, W=1 << 19)]
E("g6d_frame_ingest", [P("frames"), N0("n", 2), P("out"), *CANVAS, P("K_out"), S()], [acc("extent", "n=0: nothing to do", n=0), *TILES])
E("g6d_frame_ingest_mesh", [P("frames"), P("meshes"), N0("n", 2), P("out"), *CANVAS, P("K_out"), S()], [acc("extent", "n=0: nothing to do", n=0), *TILES])
E("g6d_frame_ingest_area", [P("frames"), O("meshes"), N0("n", 2), P("out"), *CANVAS, P("K_out"), S()], [acc("extent", "n=0: nothing to do", n=0), *TILES])
E("g6d_frame_emit", [P("sinks"), N0("n", 2), P("imgs"), *CANVAS, P("pts"), P("valid"), S()], [acc("extent", "n=0: nothing to do", n=0), *TILES])
E("g6d_frame_emit_source", [P("sinks"), N0("n", 2), P("frames"), N("nf", 2), P("pts"), P("valid"), N("sets", 2), N("B", 2), N("max_w", 64), N("max_h", 48), S()],
  [acc("extent", "n=0: nothing to do", n=0), mx("sets", 2), mx("max_w", 8192), mx("max_h", 8192),
   rej("reach", "tiles * n past 2^31 - 1", n=1 << 20, max_w=8192, max_h=8192)])
CROP = [P("frames"), P("rec"), P("imgs"), *CANVAS, P("hinv"), P("dst"), N("dh", 32), N("dw", 32)]
CROP_CASES = [mx("B", 65535), rej("reach", "dh * dw tiles past 2^31 - 1", dh=INT_MAX, dw=INT_MAX), rej("reach", "dh = dw = 2^21", dh=1 << 21, dw=1 << 21), rej("reach", "dw = 2^31 - 1: the tile round-up leaves an int", dh=16, dw=INT_MAX),
              acc("reach", "dh = dw = 2^18", dh=1 << 18, dw=1 << 18)]
E("g6d_frame_crop", [*CROP, S()], CROP_CASES)
E("g6d_frame_crop_area", [*CROP, N("max_n", 4), S()], CROP_CASES + [mx("max_n", 8)])

# ---------------------------------------------------------------------------------------------------------- frequency-domain correlation
def fft_seg(reads_in, reads_out):
    f = dict(CORR_FIELDS)
    if not reads_in:
        f.update(in_="ON", ld_in=("X", "this launch does not read the maps' inputs"))
    if not reads_out:
        f.update(out="ON", ld_out=("X", "this launch does not write the maps' outputs"))
    rows = corr_rows(32, 32, 20)
    rows[0].update({} if reads_in else {"in_": 0}, **({} if reads_out else {"out": 0}))
    return T("segs", lib.G6dCorrSeg, rows, f)


FFT_KT = [rej("mode", "k=7", k=7), rej("mode", "k=0", k=0), rej("mode", "T=16", T=16), rej("mode", "T=0", T=0)]
FFT_SEGS = [rej("extent", "nseg=0", nseg=0), rej("extent", "nseg=5", nseg=5), acck("extent", "four maps", {"segs[+++]": {}})]
# (the plan is arithmetic on sizes: it reads no pointer of a segment and answers for any Cin, Cout >= 1 and any k < T it can tile)
E("g6d_corr_fft_plan", [fft_seg(False, False), I("nseg", 1), N("Cin", 32), N("Cout", 32), I("k", 15), I("T", 32), H("out", C.c_int64, [0] * 8)],
  FFT_KT[1:] + FFT_SEGS)
E("g6d_corr_fft_fwd", [fft_seg(True, False), I("nseg", 1), N("Cin", 32), I("k", 15), I("T", 32), P("X", "req"), S()],
  FFT_KT + FFT_SEGS + [rej("extent", "Cin=48 not a multiple of 32", Cin=48), rejk("stride", "ld_in=16 < Cin=32", {"segs[0].ld_in": 16}),
                       rejk("alignment", "segs[0].in + 4 bytes", {"segs[0].in_": dev(SEG_PTRS) + 4})])
E("g6d_corr_fft_gemm", [P("X", "req"), P("B", "req"), P("Y"), N("tiles", 4), N("Cin", 32), I("Cout", 32), I("T", 32), S()],
  [rej("mode", "T=16", T=16), rej("mode", "T=0", T=0), rej("mode", "Cout=16", Cout=16), rej("mode", "Cout=0", Cout=0), rej("extent", "Cin=48 not a multiple of 32", Cin=48)])
E("g6d_corr_fft_inv", [fft_seg(False, True), I("nseg", 1), I("Cout", 32), I("k", 15), I("T", 32), P("Y"), S()],
  FFT_KT + FFT_SEGS + [rej("mode", "Cout=16", Cout=16), rej("mode", "Cout=0", Cout=0), rejk("stride", "ld_out=16 < Cout=32", {"segs[0].ld_out": 16})])


# ========================================================================================================== case generation
def _field_kind(spec):
    return spec if isinstance(spec, str) else spec[0]


def cases_of(entry):
    """Every case of one entry point: the baseline, the mechanical null / extent / alignment / optional cases, and the hand-written ones."""
    args, hand = ENTRIES[entry]
    out = [Case(entry, "baseline", "baseline", {}, "accept")]
    for a in args:
        if a.kind in ("P", "H", "T"):
            out.append(Case(entry, "null", f"{a.name} NULL", {a.name: None}, "reject"))
        if a.kind in ("O", "HO"):
            # an optional pointer that takes part in a pairing may be refused when dropped alone (with a message; the hand cases state
            # which combinations are refused and which accepted); every other one MUST be accepted as NULL
            out.append(Case(entry, "null", f"optional {a.name} NULL", {a.name: None}, "any" if a.meta["paired"] else "accept"))
        if a.kind == "R":
            out.append(Case(entry, "null", f"optional {a.name} given", {a.name: {}}, "any" if entry == "g6d_conv_igemm_ex" else "accept"))
        if a.kind in ("P", "O") and a.meta["al"]:
            out.append(Case(entry, "alignment", f"{a.name} + 4 bytes", {a.name: a.base + 4}, "reject" if a.meta["al"] == "req" else "accept"))
        if a.kind == "N":
            out.append(Case(entry, "extent", f"{a.name}=0", {a.name: 0}, "reject"))
            out.append(Case(entry, "extent", f"{a.name}=-1", {a.name: -1}, "reject"))
        if a.kind == "N0":
            out.append(Case(entry, "extent", f"{a.name}=-1", {a.name: -1}, "reject"))
        if a.kind == "T":
            for f, spec in a.meta["fields"].items():
                k = _field_kind(spec)
                key = f"{a.name}[0].{f}"
                if k == "P":
                    out.append(Case(entry, "null", f"{key} NULL", {key: 0}, "reject"))
                if k == "N":
                    out.append(Case(entry, "extent", f"{key}=0", {key: 0}, "reject"))
                    out.append(Case(entry, "extent", f"{key}=-1", {key: -1}, "reject"))
    for expect, cls, label, over in hand:
        out.append(Case(entry, cls, label, over, expect))
    return out


def all_cases():
    return [c for e in ENTRIES for c in cases_of(e)]


def case_id(c):
    return f"{c.entry[4:]}-{c.cls}-{re.sub(r'[^A-Za-z0-9_=.+<>*^-]+', '_', c.label)}"


# ========================================================================================================== marshalling
def _apply(values, args, over):
    """values: name -> python value (deep copy of the baseline); over: the case's overrides."""
    kinds = {a.name: a for a in args}
    for key, v in over.items():
        m = re.fullmatch(r"(\w+)\[(\d+)\]\.(\w+)", key)
        if m:
            values[m.group(1)][int(m.group(2))][m.group(3)] = v
            continue
        m = re.fullmatch(r"(\w+)\[(\d+)\]", key)
        if m:
            values[m.group(1)][int(m.group(2))] = v
            continue
        m = re.fullmatch(r"(\w+)\[(\++)\]", key)          # append len("+") rows: copies of row 0 at their own addresses, `v` = field overrides of the LAST
        if m:
            name = m.group(1)
            rows = values[name]
            for i in range(len(m.group(2))):
                r = dict(rows[0])
                for f, spec in kinds[name].meta["fields"].items():
                    if _field_kind(spec) in ("P", "O") and r.get(f):
                        r[f] = r[f] + (i + 1) * 8 * FAKE_STEP
                rows.append(r)
            rows[-1].update(v)
            if "nseg" in values:
                values["nseg"] = len(rows)
            continue
        if key not in values:
            raise KeyError(f"override {key!r} names no argument")
        values[key] = v


def marshal(entry, over):
    """-> (ctypes argument list, keep-alive list) of `entry`'s baseline with `over` applied."""
    args, _ = ENTRIES[entry]
    values = {a.name: copy.deepcopy(a.base) for a in args}
    _apply(values, args, over)
    out, keep = [], []
    for a in args:
        v = values[a.name]
        if a.kind in ("P", "O", "ON", "S"):
            out.append(C.c_void_p(v or None))
        elif a.kind in ("H", "HO"):
            if v is None:
                out.append(None)
            else:
                ct = a.meta["ctype"]
                arr = (ct * max(len(v), 1))(*[(x or None) if ct is C.c_void_p else x for x in v])
                keep.append(arr)
                out.append(C.cast(arr, C.c_void_p))
        elif a.kind == "T":
            if v is None:
                out.append(None)
            else:
                st = a.meta["struct"]
                ftypes = dict(st._fields_)
                arr = (st * len(v))(*[st(**{k: (x or None) if ftypes[k] is C.c_void_p else x for k, x in row.items()}) for row in v])
                keep.append(arr)
                out.append(C.cast(arr, C.c_void_p))
        elif a.kind == "R":
            if v is None:
                out.append(None)
            else:
                rec = lib.G6dRange16(exps=v.get("exps"), rec=v.get("rec"), slot_in=v.get("slot_in", -1), slot_out=v.get("slot_out", -1))
                keep.append(rec)
                out.append(C.cast(C.pointer(rec), C.c_void_p))
        else:
            out.append(v)
    return out, keep


def _fix_pointer_types(entry, cargs):
    """ctypes wants POINTER(T) instances where SIGNATURES says so: cast the arrays."""
    sig = lib.SIGNATURES[entry]
    fixed = []
    for t, v in zip(sig, cargs):
        if v is not None and hasattr(t, "contents") and not isinstance(v, t):
            v = C.cast(v, t)
        fixed.append(v)
    return fixed


def issue(entry, over):
    """One call of `entry` with the baseline arguments and `over` -> (rc, message, message_rewritten).  Refuses to run where a GPU is visible."""
    import torch
    if torch.cuda.device_count() != 0:
        raise RuntimeError("tests/launch_contract.py issues calls on FAKE device pointers: never where a GPU is visible")
    l = lib.load()
    cargs, keep = marshal(entry, over)
    cargs = _fix_pointer_types(entry, cargs)
    l.g6d_set_knob(b"no_such_knob", 0.0)
    assert l.g6d_last_error() == SENTINEL
    rc = getattr(l, entry)(*cargs)
    msg = l.g6d_last_error()
    del keep
    return rc, msg.decode(errors="replace"), msg != SENTINEL


def outcome(entry, rc):
    """Accepted = not refused: G6D_ELAUNCH on this host; G6D_OK or a plan's answer from the host-only functions and from a launcher that has
    nothing to launch (n = 0 frames, 0 bytes)."""
    return "reject" if rc in (EINVAL, ENOSPC) else "accept"


def verdict(c):
    """-> (ok, text) of one case against the loaded library."""
    rc, msg, fresh = issue(c.entry, c.over)
    got = outcome(c.entry, rc)
    if c.expect == "any":                       # an optional pointer dropped alone: refused only as a broken pairing, and then with a message
        ok = got == "accept" or (got == "reject" and fresh)
    elif c.expect == "reject":
        ok = got == "reject" and fresh
    else:
        ok = got == "accept"
    return ok, f"{case_id(c)}: expected {c.expect}, got {got} (rc {rc}, {'fresh' if fresh else 'STALE'} message {msg!r})"


# ========================================================================================================== completeness
def completeness_errors():
    """What the table owes lib.SIGNATURES: -> list of complaints (empty = complete)."""
    bad = []
    for name, sig in lib.SIGNATURES.items():
        if name in EXEMPT:
            continue
        if name not in ENTRIES:
            bad.append(f"{name}: neither in the table nor exempt")
            continue
        args, _ = ENTRIES[name]
        if len(args) != len(sig):
            bad.append(f"{name}: {len(args)} arguments in the table, {len(sig)} in SIGNATURES")
            continue
        touched = set()                        # arguments and table fields that some REJECTED case changes
        for c in cases_of(name):
            if c.expect != "reject":
                continue
            for key, v in c.over.items():
                m = re.fullmatch(r"(\w+)\[(\d+|\++)\](?:\.(\w+))?", key)
                if not m:
                    touched.add(key)
                elif m.group(3):
                    touched.add(f"{m.group(1)}[0].{m.group(3)}")
                elif isinstance(v, dict):
                    touched.update(f"{m.group(1)}[0].{f}" for f in v)
                else:
                    touched.add(m.group(1))
        for a, t in zip(args, sig):
            is_ptr = t is C.c_void_p or hasattr(t, "contents")
            if is_ptr != (a.kind in ("P", "O", "ON", "H", "HO", "T", "R", "S")):
                bad.append(f"{name}.{a.name}: kind {a.kind} does not match the signature's {t.__name__}")
            if t in (C.c_int, C.c_size_t):
                if a.kind == "X":
                    if not a.meta["why"]:
                        bad.append(f"{name}.{a.name}: free without a reason")
                elif a.name not in touched:
                    bad.append(f"{name}.{a.name}: integer argument with no violation and no `free` declaration")
            if a.kind == "T":
                st = a.meta["struct"]
                if st not in (lib.G6dConv, lib.G6dWinoSeg, lib.G6dConv16Seg, lib.G6dCorrSeg):
                    bad.append(f"{name}.{a.name}: unexpected table type")
                for f, ft in st._fields_:
                    spec = a.meta["fields"].get(f)
                    if spec is None:
                        bad.append(f"{name}.{a.name}.{f}: field missing from the table")
                        continue
                    k = _field_kind(spec)
                    if ft is C.c_void_p:
                        if k not in ("P", "O", "ON"):
                            bad.append(f"{name}.{a.name}.{f}: pointer field needs a null case or an optional declaration")
                    elif ft in (C.c_int32, C.c_size_t):
                        if k == "X":
                            if not spec[1]:
                                bad.append(f"{name}.{a.name}.{f}: free without a reason")
                        elif f"{a.name}[0].{f}" not in touched:
                            bad.append(f"{name}.{a.name}.{f}: integer field with no violation and no `free` declaration")
    for name in ENTRIES:
        if name not in lib.SIGNATURES:
            bad.append(f"{name}: in the table, not in SIGNATURES")
    for name in EXEMPT:
        if name != "g6d_marker" and not name.startswith("g6d_sizeof_"):
            bad.append(f"{name}: only g6d_marker and the g6d_sizeof_* may be exempt")
    return bad


def declarations():
    """-> (optional, free): lists of (entry, argument, reason) for the record."""
    opt, free = [], []
    for name, (args, _) in ENTRIES.items():
        for a in args:
            if a.kind in ("O", "ON", "HO", "R"):
                opt.append((name, a.name, "NULL allowed (include/gen6d_hip.h)"))
            if a.kind == "X":
                free.append((name, a.name, a.meta["why"]))
            if a.kind == "T":
                for f, spec in a.meta["fields"].items():
                    if _field_kind(spec) in ("O", "ON"):
                        opt.append((name, f"{a.name}.{f}", "NULL allowed (include/gen6d_hip.h)"))
                    if _field_kind(spec) == "X":
                        free.append((name, f"{a.name}.{f}", spec[1]))
    return opt, free


def main(argv):
    """python tests/launch_contract.py [--lib PATH] [--counts]: run the whole table against a library and list what it gets wrong."""
    import time
    if "--lib" in argv:
        lib.LIB_PATH = argv[argv.index("--lib") + 1]
    if "--counts" in argv:
        for name in ENTRIES:
            n = {}
            for c in cases_of(name):
                n[c.cls] = n.get(c.cls, 0) + 1
            print(f"| `{name}` | " + " | ".join(str(n.get(k, 0)) for k in CLASSES) + " |")
        return 0
    t0 = time.time()
    cases = all_cases()
    wrong = 0
    for c in cases:
        ok, text = verdict(c)
        if not ok:
            wrong += 1
            print(text)
    print(f"{len(cases)} cases, {wrong} wrong, {time.time() - t0:.2f} s, library {lib.LIB_PATH}")
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
