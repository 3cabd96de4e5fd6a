"""The host side of the multi-map launches, pinned on the CPU from both sides of the C ABI.

Part A — the library's table validation.  Every multi entry point checks its segment table before its first HIP call, so a table built
from fake (16-byte aligned, non-null) addresses that carries a defect returns G6D_EINVAL on a machine without a GPU and g6d_last_error()
names the cause.  EVERY table below is invalid: no call here reaches a launch or hands a fake address to a kernel.
  * Order of the checks in the seven float entry points: arguments, then every segment, then the extents.  A bad last segment therefore
    hides an extent defect of an earlier one (pinned: `*_then_bad_last`), and a table that passes the extent check is launched — only the
    two F(4x4,3x3) entries check anything later (the filter bank's size), so only they can show on the CPU that an extent just below the
    bound is accepted (`in_below_bound` there ends in "filter bank exceeds 2^31 bytes").
  * Input addresses are 16-byte aligned and ld_in % 4 == 0, so the input extents of an otherwise valid table are multiples of 4 floats:
    "just below" the input bound is bound - 4.  Output extents have no such rule: bound - 1.
  * Two messages are corrected by the shared helper and recorded as such in MESSAGES: g6d_wino_conv3x3_multi tests 2^29 and used to say 2^30;
    g6d_wino16_conv3x3_multi said "bad segment" without the explanation its fp32 twin gives.

Part B — the Python wrappers (gen6d_amd/ops.py) over a recording fake of the library: entry point, every scalar argument, every segment
field (pointers as offsets from the tensors passed in or returned), the returned lists, PairMap wrapping, and the PROFILE / PROFILE_HBM
entries without their events.  The expected values are literals, taken from a run of the wrappers as they were before they were folded
onto shared builders."""
import ctypes as C

import pytest
import torch

from gen6d_amd import lib, ops

EINVAL = -1
BASE_IN, BASE_FULL, BASE_POOL, FAKE = 0x10000000, 0x200000000, 0x400000000, 0x70000000


# ======================================================================================================================================
# Part A: library validation
# ======================================================================================================================================
MESSAGES = {
    # entry: (bad arguments, bad segment, extent)
    "wino": ("wino_conv3x3_multi: bad args (1..4 segments, Cin % 8 == 0, Cout % 64 == 0)",
             "wino_conv3x3_multi: bad segment (all segments give the same kinds of output)",
             # corrected: the entry tests 2^29 (the reach of the buffer loads) and said "2^30" before
             "wino_conv3x3_multi: segments must lie within 2^29 floats of each other (allocate them from one buffer)"),
    "wino16": ("wino16_conv3x3_multi: bad args (1..4 segments, Cin % 16 == 0, Cout % 64 == 0, math_mode 1 or 2)",
               # corrected: said only "wino16_conv3x3_multi: bad segment" before
               "wino16_conv3x3_multi: bad segment (all segments give the same kinds of output)",
               "wino16_conv3x3_multi: segments must lie within 2^29 floats of each other (allocate them from one buffer)"),
    "wino43": ("wino43_conv3x3_multi: bad args (1..4 segments, Cin % 8 == 0, Cout % 64 == 0)",
               "wino43_conv3x3_multi: bad segment (all segments give the same kinds of output)",
               "wino43_conv3x3_multi: segments must lie within 2^29 floats of each other (allocate them from one buffer)"),
    "corr_wino": ("corr2d_wino_multi: bad args (1..4 map sizes, 15x15 = 5 blocks, Cin % 8 == 0, Cout % 32 == 0)",
                  "corr2d_wino_multi: bad map (all maps share ld_in)",
                  "corr2d_wino_multi: maps must lie within 2^29 floats of each other (allocate them from one buffer)"),
    "corr_wino43": ("corr2d_wino43_multi: bad args (1..4 map sizes, 15x15 = 5 blocks or 9x9 = 3 blocks, Cin % 8 == 0, Cout % 32 == 0)",
                    "corr2d_wino43_multi: bad map (all maps share ld_in)",
                    "corr2d_wino43_multi: maps must lie within 2^29 floats of each other (allocate them from one buffer)"),
    "corr_patch": ("corr2d_patch_multi: bad args (1..4 maps, Cout <= 32, odd kernel <= 31, Cin % 4 == 0)",
                   "corr2d_patch_multi: bad map",
                   "corr2d_patch_multi: maps must lie within 2^30 floats of each other (allocate them from one buffer)"),
    "corr_patch16": ("corr2d_patch16_multi: bad args (1..4 maps, Cin % 32 == 0, Cout <= 32, odd kernel <= 15, math_mode 1 or 2)",
                     "corr2d_patch16_multi: bad map",
                     "corr2d_patch16_multi: maps must lie within 2^30 floats of each other (allocate them from one buffer)"),
}
IN_BOUND = {"wino": 1 << 29, "wino16": 1 << 29, "wino43": 1 << 29, "corr_wino": 1 << 29, "corr_wino43": 1 << 29,
            "corr_patch": 1 << 30, "corr_patch16": 1 << 30}
OUT_BOUND = 1 << 31
WINO = ("wino", "wino16", "wino43")
CIN = 32


def _cout(entry):
    return 64 if entry in WINO else 32


def _call(entry, segs, nseg, Cin=CIN, Cout=None):
    """The entry point on `segs` with valid non-table arguments (fake filter / workspace addresses, stream 0)."""
    L = lib.load()
    Cout = _cout(entry) if Cout is None else Cout
    P = C.c_void_p
    rc = {
        "wino": lambda: L.g6d_wino_conv3x3_multi(segs, nseg, Cin, P(FAKE), P(FAKE + 4096), Cout, 1, P(FAKE + 8192), 1 << 20, None),
        "wino16": lambda: L.g6d_wino16_conv3x3_multi(segs, nseg, Cin, P(FAKE), P(FAKE + 4096), Cout, 1, 2, P(FAKE + 8192), 1 << 20, None),
        "wino43": lambda: L.g6d_wino43_conv3x3_multi(segs, nseg, Cin, P(FAKE), P(FAKE + 4096), Cout, 1, P(FAKE + 8192), 1 << 20, None),
        "corr_wino": lambda: L.g6d_corr2d_wino_multi(segs, nseg, Cin, P(FAKE), Cout, 5, P(FAKE + 8192), 1 << 20, None),
        "corr_wino43": lambda: L.g6d_corr2d_wino43_multi(segs, nseg, Cin, P(FAKE), Cout, 5, P(FAKE + 8192), 1 << 20, None),
        "corr_patch": lambda: L.g6d_corr2d_patch_multi(segs, nseg, Cin, P(FAKE), Cout, 3, 3, P(FAKE + 8192), 1 << 20, 0, None),
        "corr_patch16": lambda: L.g6d_corr2d_patch16_multi(segs, nseg, Cin, P(FAKE), Cout, 3, 3, P(FAKE + 8192), 1 << 20, 2, None),
    }[entry]()
    return rc, L.g6d_last_error().decode()


def _seg(entry, i=0, **kw):
    """A valid small segment (4x6 map, 2 images) of the entry's table type at fake addresses; keywords override fields.  `pool`:
    the Winograd entries' tables give full outputs, pooled outputs or both."""
    ld_in, Cout = kw.pop("ld_in", CIN), _cout(entry)
    f = dict(in_=BASE_IN + i * 0x100000, N=2, H=4, W=6, ld_in=ld_in)
    if entry in WINO:
        f.update(out_full=BASE_FULL + i * 0x100000, out_pool=None, ld_full=Cout, ld_pool=Cout)
        f.update(kw)
        return lib.G6dWinoSeg(**f)
    f.update(out=BASE_FULL + i * 0x100000, ld_out=Cout)
    for old, new in (("out_full", "out"), ("ld_full", "ld_out")):
        if old in kw:
            kw[new] = kw.pop(old)
    kw.pop("ld_pool", None)
    f.update(kw)
    return lib.G6dCorrSeg(**f)


def _table(entry, *segs):
    T = lib.G6dWinoSeg if entry in WINO else lib.G6dCorrSeg
    return (T * max(len(segs), 1))(*segs)


def _expect(entry, segs, which, **kw):
    rc, msg = _call(entry, _table(entry, *segs), len(segs), **kw)
    assert rc == EINVAL
    assert msg == (MESSAGES[entry][which] if isinstance(which, int) else which)


ENTRIES = list(MESSAGES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_segment_count(entry):
    four = [_seg(entry, i) for i in range(4)]
    for n in (0, 5, -1):
        rc, msg = _call(entry, _table(entry, *four), n)
        assert (rc, msg) == (EINVAL, MESSAGES[entry][0])
    rc, msg = _call(entry, None, 1)
    assert (rc, msg) == (EINVAL, MESSAGES[entry][0])


SEG_DEFECTS = {
    "null_input": dict(in_=None),
    "ld_in_below_Cin": dict(ld_in=CIN - 4),
    "ld_in_not_multiple_of_4": dict(ld_in=CIN + 2),
    "misaligned_input": dict(in_=BASE_IN + 0x100000 + 4),
    "ld_out_below_Cout": "ld_out",
    "N_zero": dict(N=0),
    "H_zero": dict(H=0),
    "W_negative": dict(W=-3),
}


@pytest.mark.parametrize("defect", list(SEG_DEFECTS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_segment_defect(entry, defect):
    """One defect at a time, in the first and in the last segment of a table that is valid otherwise."""
    kw = SEG_DEFECTS[defect]
    if kw == "ld_out":
        kw = dict(ld_full=_cout(entry) - 1)
    if entry in ("corr_wino", "corr_wino43") and "ld_in" in kw:
        # the shared-ld_in rule of these two must not be what fires: the whole table uses the defective row length
        _expect(entry, [_seg(entry, 0, ld_in=kw["ld_in"]), _seg(entry, 1, ld_in=kw["ld_in"])], 1)
        return
    _expect(entry, [_seg(entry, 0), _seg(entry, 1, **kw)], 1)
    _expect(entry, [_seg(entry, 0, **kw), _seg(entry, 1)], 1)
    _expect(entry, [_seg(entry, 0), _seg(entry, 1), _seg(entry, 2), _seg(entry, 3, **kw)], 1)


@pytest.mark.parametrize("entry", WINO)
def test_wino_output_kinds(entry):
    name = MESSAGES[entry][2].split(":")[0]
    # no output at all
    _expect(entry, [_seg(entry, 0, out_full=None)], f"{name}: no output")
    # mixed kinds: the first segment decides, a later one lacks / adds a kind
    _expect(entry, [_seg(entry, 0), _seg(entry, 1, out_full=None, out_pool=BASE_POOL)], 1)
    _expect(entry, [_seg(entry, 0), _seg(entry, 1, out_pool=BASE_POOL)], 1)
    _expect(entry, [_seg(entry, 0, out_pool=BASE_POOL), _seg(entry, 1)], 1)
    # pooled output: ld_pool below Cout, maps with H < 2 or W < 2 (the same maps pass without pooling: see the extent tests' 1x1 maps)
    _expect(entry, [_seg(entry, 0, out_pool=BASE_POOL), _seg(entry, 1, out_pool=BASE_POOL + 0x100000, ld_pool=63)], 1)
    _expect(entry, [_seg(entry, 0, out_pool=BASE_POOL), _seg(entry, 1, out_pool=BASE_POOL + 0x100000, H=1)], 1)
    _expect(entry, [_seg(entry, 0, out_full=None, out_pool=BASE_POOL, W=1)], 1)
    # ld_full is not looked at when no full output is asked for, ld_pool is: the defect that fires is the pooled one
    _expect(entry, [_seg(entry, 0, out_full=None, out_pool=BASE_POOL, ld_full=0, ld_pool=8)], 1)


@pytest.mark.parametrize("entry", ["corr_wino", "corr_wino43"])
def test_corr_wino_maps_share_ld_in(entry):
    _expect(entry, [_seg(entry, 0), _seg(entry, 1, ld_in=CIN + 4)], 1)
    _expect(entry, [_seg(entry, 0, ld_in=CIN + 4), _seg(entry, 1)], 1)
    _expect(entry, [_seg(entry, 0, out_full=None), _seg(entry, 1)], 1)        # a missing output is a bad map too


@pytest.mark.parametrize("entry", ["corr_patch", "corr_patch16"])
def test_corr_patch_maps_need_not_share_ld_in(entry):
    """The patch kernels take a row length per map: a table with two row lengths gets past the map checks (and is stopped here by the
    extent check of its second map, so that nothing is launched)."""
    far = _seg(entry, 1, ld_in=CIN + 4, in_=BASE_IN + 4 * IN_BOUND[entry])
    _expect(entry, [_seg(entry, 0), far], 2)
    _expect(entry, [_seg(entry, 0), _seg(entry, 1, out_full=None)], 1)


def _far_in(entry, extent):
    """A 1x1 map of one image whose input ends `extent` floats after BASE_IN."""
    return _seg(entry, 1, N=1, H=1, W=1, in_=BASE_IN + 4 * (extent - CIN))


def _far_out(entry, extent, pool=False):
    if pool:
        # (2x2: the smallest pooled map; the bound is applied to N * H * W * ld_pool)
        return _seg(entry, 1, N=1, H=2, W=2, out_full=None, out_pool=BASE_POOL + 4 * (extent - 4 * _cout(entry)))
    return _seg(entry, 1, N=1, H=1, W=1, out_full=BASE_FULL + 4 * (extent - _cout(entry)))


@pytest.mark.parametrize("entry", ENTRIES)
def test_input_extent(entry):
    B = IN_BOUND[entry]
    near, bad = _seg(entry, 0), _seg(entry, 2, in_=None)
    # at the bound, and beyond it: refused with the extent message — by one map that large, or by the distance between two
    _expect(entry, [near, _far_in(entry, B)], 2)
    _expect(entry, [_far_in(entry, B), near], 2)
    _expect(entry, [near, _far_in(entry, B + 4)], 2)
    big = {1 << 29: dict(N=1, H=4096, W=4096), 1 << 30: dict(N=2, H=4096, W=4096)}[B]
    _expect(entry, [_seg(entry, 0, **big)], 2)
    # the other entries' bound is not this entry's: 2^29 passes where 2^30 is the bound (second defect: a bad last map)
    if B == 1 << 30:
        _expect(entry, [near, _far_in(entry, 1 << 29), bad], 1)
    # just below the bound with a second, independent defect
    _expect(entry, [near, _far_in(entry, B - 4), bad], 1)
    # ... and the segment checks come first: the same defect hides an extent AT the bound
    _expect(entry, [near, _far_in(entry, B), bad], 1)


@pytest.mark.parametrize("entry", ["wino43", "corr_wino43"])
def test_input_extent_below_bound_is_accepted(entry):
    """The F(4x4,3x3) entries check the filter bank's size after the table: with Cin = 8192 and Cout = 2048 (a 2.4 GB bank) a table whose
    extent lies just below the bound gets that message, one at the bound the extent message."""
    Cin, Cout, B = 8192, 2048, 1 << 29

    def segs(extent):
        kw = dict(ld_in=Cin, ld_full=Cout, ld_pool=Cout)
        return [_seg(entry, 0, **kw), _seg(entry, 1, N=1, H=1, W=1, in_=BASE_IN + 4 * (extent - Cin), **kw)]
    _expect(entry, segs(B - 4), "wino43: filter bank exceeds 2^31 bytes", Cin=Cin, Cout=Cout)
    _expect(entry, segs(B), 2, Cin=Cin, Cout=Cout)
    # the same for the output bound
    kw = dict(ld_in=Cin, ld_full=Cout, ld_pool=Cout)

    def osegs(extent):
        return [_seg(entry, 0, **kw), _seg(entry, 1, N=1, H=1, W=1, out_full=BASE_FULL + 4 * (extent - Cout), **kw)]
    _expect(entry, osegs(OUT_BOUND - 1), "wino43: filter bank exceeds 2^31 bytes", Cin=Cin, Cout=Cout)
    _expect(entry, osegs(OUT_BOUND), 2, Cin=Cin, Cout=Cout)


@pytest.mark.parametrize("entry", ENTRIES)
def test_output_extent(entry):
    near, bad = _seg(entry, 0), _seg(entry, 2, in_=None)
    _expect(entry, [near, _far_out(entry, OUT_BOUND)], 2)
    _expect(entry, [_far_out(entry, OUT_BOUND), near], 2)
    _expect(entry, [near, _far_out(entry, OUT_BOUND - 1), bad], 1)
    _expect(entry, [near, _far_out(entry, OUT_BOUND), bad], 1)
    if entry in WINO:
        pnear, pbad = _seg(entry, 0, out_full=None, out_pool=BASE_POOL), _seg(entry, 2, in_=None, out_full=None, out_pool=BASE_POOL)
        _expect(entry, [pnear, _far_out(entry, OUT_BOUND, pool=True)], 2)
        _expect(entry, [pnear, _far_out(entry, OUT_BOUND - 1, pool=True), pbad], 1)


# ---- the 16-bit direct kernels: one pass over the table, every check per segment in turn -----------------------------------------------
def _seg16(i=0, **kw):
    f = dict(in_=BASE_IN + i * 0x100000, out_full=BASE_FULL + i * 0x100000, out_pool=None, N=2, D=1, H=4, W=6, ld_in=64, ld_full=128, ld_pool=0)
    f.update(kw)
    return lib.G6dConv16Seg(**f)


def _conv16(segs, nseg=None, Cin=64, Cout=128, kd=1, full_type=2, pool_type=0, mode=2, W16=FAKE):
    L = lib.load()
    t = (lib.G6dConv16Seg * max(len(segs), 1))(*segs)
    rc = L.g6d_conv16_direct_multi_ex(t, len(segs) if nseg is None else nseg, Cin, C.c_void_p(W16), 1, 1.0, None, Cout, kd, 1, full_type,
                                      pool_type, mode, None, 0, None, None)
    return rc, L.g6d_last_error().decode()


def _corr16(segs, nseg=None, Cin=32, mode=2, k=7, W16=FAKE):
    L = lib.load()
    t = (lib.G6dConv16Seg * max(len(segs), 1))(*segs)
    rc = L.g6d_corr16_multi_ex(t, len(segs) if nseg is None else nseg, Cin, C.c_void_p(W16), 1.0, 32, k, mode, None, None)
    return rc, L.g6d_last_error().decode()


def test_conv16_direct_segment_checks():
    ok = _seg16(0)
    four = [_seg16(i) for i in range(4)]
    for n in (0, 5):
        assert _conv16(four, nseg=n) == (EINVAL, "conv16_direct: 1..4 segments and filters expected")
    assert _conv16([ok], W16=None) == (EINVAL, "conv16_direct: 1..4 segments and filters expected")
    bad = "conv16_direct: bad segment"
    for kw in (dict(in_=None), dict(N=0), dict(H=0), dict(W=0), dict(D=0), dict(ld_in=56), dict(D=2)):
        assert _conv16([ok, _seg16(1, **kw)]) == (EINVAL, bad), kw
    assert _conv16([ok, _seg16(1, ld_in=32)], Cin=32, mode=3) == (EINVAL, bad)                   # pairs: two planes per row
    assert _conv16([_seg16(0, D=3), _seg16(1, D=2)], kd=3) == (EINVAL, bad)                      # one depth per table
    outs = "conv16_direct: outputs missing / odd map with pooling"
    for kw in (dict(out_full=None), dict(ld_full=120)):
        assert _conv16([ok, _seg16(1, **kw)]) == (EINVAL, outs), kw
    assert _conv16([_seg16(0, ld_full=256), _seg16(1, ld_full=128)], Cin=32, mode=3, full_type=3) == (EINVAL, outs)       # pair outputs: 2 Cout per row
    pool = dict(out_pool=BASE_POOL, ld_pool=128)
    for kw in (dict(out_pool=None), dict(ld_pool=64), dict(H=5), dict(W=7)):
        assert _conv16([_seg16(0, **pool), _seg16(1, **{**pool, **kw})], pool_type=2) == (EINVAL, outs), kw
    rows = "conv16_direct: 16-byte aligned rows expected"
    for kw in (dict(in_=BASE_IN + 8), dict(ld_in=68), dict(out_full=BASE_FULL + 8), dict(ld_full=132)):
        assert _conv16([ok, _seg16(1, **kw)]) == (EINVAL, rows), kw
    assert _conv16([_seg16(0, **pool), _seg16(1, **{**pool, "out_pool": BASE_POOL + 4})], pool_type=2) == (EINVAL, rows)
    # input extent: (N D H W + W + 1) pixels of ld_in 16-bit values reach 2^31 bytes at N H = 2^24 - 2 for W = 1, ld_in = 64
    far = "conv16_direct: a segment's input beyond 2 GB"
    assert _conv16([ok, _seg16(1, N=1, H=(1 << 24) - 2, W=1)]) == (EINVAL, far)
    assert _conv16([_seg16(0, N=1, H=(1 << 24) - 3, W=1), _seg16(1, in_=None)]) == (EINVAL, bad)      # one pixel less passes: the next segment's defect
    assert _conv16([ok, _seg16(1, W=1 << 18, H=2, ld_full=1 << 12)]) == (EINVAL, "conv16_direct: 32 output rows beyond 4 GB")


def test_corr16_segment_checks():
    def s(i=0, **kw):
        return _seg16(i, **{**dict(ld_in=32, ld_full=32), **kw})
    four = [s(i) for i in range(4)]
    for n in (0, 5):
        assert _corr16(four, nseg=n) == (EINVAL, "corr16: 1..4 segments and filters expected")
    assert _corr16([s()], W16=None) == (EINVAL, "corr16: 1..4 segments and filters expected")
    bad = "corr16: bad segment"
    for kw in (dict(in_=None), dict(out_full=None), dict(N=0), dict(D=2), dict(H=0), dict(W=0), dict(ld_in=24), dict(ld_full=24), dict(ld_in=36),
               dict(in_=BASE_IN + 8), dict(out_full=BASE_FULL + 4)):
        assert _corr16([s(0), s(1, **kw)]) == (EINVAL, bad), kw
        assert _corr16([s(0), s(1), s(2), s(3, **kw)], k=15) == (EINVAL, bad), kw
    assert _corr16([s(0), s(1, ld_in=32)], mode=3) == (EINVAL, bad)                  # pairs: two planes per row
    # input extent: N H W rows of ld_in = 32 16-bit values reach 2^31 bytes at 2^25 pixels
    far = "corr16: a segment's input beyond 2 GB"
    assert _corr16([s(0), s(1, N=1, H=1 << 25, W=1)]) == (EINVAL, far)
    assert _corr16([s(0, N=1, H=(1 << 25) - 1, W=1), s(1, in_=None)]) == (EINVAL, bad)    # one pixel less passes: the next segment's defect


# ======================================================================================================================================
# Part B: the Python wrappers over a recording fake of the library
# ======================================================================================================================================
STREAM = 0x5EED0


class _Event:
    def __init__(self, enable_timing=False):
        assert enable_timing
        self.records = 0

    def record(self):
        self.records += 1
        _Event.log.append("record")


class _FakeLib:
    """Every g6d_* function records (name, arguments as passed) and returns 0; g6d_conv_plan returns `plan`."""

    def __init__(self, log, plan=0):
        self.calls, self.log, self.plan = [], log, plan

    def __getattr__(self, name):
        if not name.startswith("g6d_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append(name)
            if name == "g6d_conv_plan":
                return self.plan
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def fake(monkeypatch):
    log = []
    f = _FakeLib(log)
    _Event.log = log
    ws = torch.zeros(64)
    monkeypatch.setattr(ops._lib, "load", lambda: f)
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(STREAM))
    monkeypatch.setattr(ops, "workspace", lambda device: ws)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(ops, "PROFILE", None)
    monkeypatch.setattr(ops, "PROFILE_HBM", None)
    monkeypatch.setattr(ops, "MATH_MODE", 0)
    f.ws = ws
    return f


def _names(prefix, v, out):
    """Flatten tensors / PairMaps / lists / tuples / dicts into {name: tensor}."""
    if isinstance(v, ops.PairMap):
        v = v.data
    if isinstance(v, torch.Tensor):
        out[prefix] = v
    elif isinstance(v, dict):
        for k, x in v.items():
            _names(f"{prefix}.{k}" if prefix else k, x, out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _names(f"{prefix}[{i}]", x, out)
    return out


def _where(addr, tensors):
    """An address -> "name+byte offset" inside a known tensor (an exact start wins), None for a null pointer."""
    if addr is None or addr == 0:
        return None
    if addr == STREAM:
        return "stream"
    for own in (True, False):             # the caller's tensors first: a caller-provided output is named by where it lies in the caller's buffer
        best = None
        for n, t in tensors.items():
            if n.startswith("ret") == own:
                continue
            off = addr - t.data_ptr()
            span = (t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()) if t.numel() else 0
            if off == 0:
                return n
            if 0 < off < span and (best is None or off < best[1]):
                best = (n, off)
        if best is not None:
            return f"{best[0]}+{best[1]}"
    raise AssertionError(f"pointer {addr:#x} is no tensor of this call")


def _canon(a, tensors):
    if hasattr(a, "_obj"):                                  # C.byref(struct)
        a = a._obj
    if isinstance(a, C.c_void_p):
        return _where(a.value, tensors)
    if isinstance(a, C.Structure):
        return {n: (_where(getattr(a, n), tensors) if ty is C.c_void_p else
                    (list(getattr(a, n)) if isinstance(getattr(a, n), C.Array) else getattr(a, n))) for n, ty in a._fields_}
    if isinstance(a, C.Array):
        return [_canon(x, tensors) for x in a]
    assert a is None or isinstance(a, (int, float)), type(a)
    return a


def _ret(v):
    """The returned structure: tensors as (shape, dtype, strides, element offset from the first tensor of their list when both are cut from
    one buffer), PairMaps tagged with their slot."""
    def one(t, first):
        if t is None:
            return None
        if isinstance(t, ops.PairMap):
            return ("PairMap", t.slot) + one(t.data, first)
        shared = first is not None and t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()       # cut from one buffer
        return (tuple(t.shape), str(t.dtype).replace("torch.", ""), tuple(t.stride()),
                (t.data_ptr() - first.data_ptr()) // t.element_size() if shared else None)
    if isinstance(v, (list, tuple)):
        if all(x is None or isinstance(x, (torch.Tensor, ops.PairMap)) for x in v) and any(x is not None for x in v):
            ts = [x.data if isinstance(x, ops.PairMap) else x for x in v if x is not None]
            return [one(x, ts[0]) for x in v]
        return [_ret(x) for x in v]
    return one(v, None) if v is not None else None


def _run(fake, inputs, call, profile=True, extra=None):
    """Run `call` once without and once with profiling; both must issue the same launch.  Returns the canonical record."""
    fake.calls.clear(); fake.log.clear()
    res0 = call()
    plain_calls, plain_log = list(fake.calls), list(fake.log)
    ts0 = _names("", dict(inputs, ret=res0, ws=fake.ws, **(extra() if extra else {})), {})
    rec0 = [(n, [_canon(a, ts0) for a in args]) for n, args in plain_calls]
    assert plain_log == [n for n, _ in plain_calls]                     # no events, no g6d_conv_plan without profiling
    fake.calls.clear(); fake.log.clear()
    ops.PROFILE, ops.PROFILE_HBM = [], {}
    try:
        res = call()
        prof, hbm = ops.PROFILE, ops.PROFILE_HBM
    finally:
        ops.PROFILE, ops.PROFILE_HBM = None, None
    ts = _names("", dict(inputs, ret=res, ws=fake.ws, **(extra() if extra else {})), {})
    rec = [(n, [_canon(a, ts) for a in args]) for n, args in fake.calls]
    assert rec == rec0 and _ret(res) == _ret(res0)
    for e in prof + [x for v in hbm.values() for x in v]:
        assert isinstance(e[1], _Event) and isinstance(e[2], _Event) and e[1] is not e[2] and e[1].records == e[2].records == 1
    return {"calls": rec, "ret": _ret(res), "log_plain": plain_log, "log": list(fake.log),
            "profile": [e[:1] + e[3:] for e in prof], "hbm": {k: [e[:1] + e[3:] for e in v] for k, v in hbm.items()}}


SHAPES = [(2, 9, 7), (1, 8, 8), (3, 5, 13)]


def _fill(ts):
    for i, t in enumerate(ts):
        t.fill_(float(i + 1))
    return ts


def _trunk_case(kind, full, pool, shapes=SHAPES):
    Cin, Cout = 16, 64
    xs = _fill(ops.alloc_like_segments([s + (Cin,) for s in shapes], "cpu"))
    bias = torch.zeros(Cout)
    if kind == "wino":
        U = torch.zeros((Cin // 8, 16, Cout, 8))
        return dict(xs=xs, U=U, bias=bias), lambda: ops.wino_conv3x3_multi(xs, U, bias, relu=True, full=full, pool=pool)
    if kind == "wino43":
        U = torch.zeros(ops.w43_shape(Cin // 8, Cout))
        return dict(xs=xs, U=U, bias=bias), lambda: ops.wino43_conv3x3_multi(xs, U, bias, relu=False, full=full, pool=pool)
    U = torch.zeros((Cin // 16, 16, Cout, 16), dtype=torch.bfloat16 if kind == "wino16bf" else torch.float16)
    return dict(xs=xs, U=U, bias=bias), lambda: ops.wino16_conv3x3_multi(xs, U, bias, relu=True, full=full, pool=pool)


def _corr_case(kind, N=2, shapes=((9, 7), (8, 8), (5, 13)), **kw):
    Cin, Cout = 32, 32
    xs = _fill(ops.alloc_like_segments([(N, 1, h, w, Cin) for h, w in shapes], "cpu"))
    outs = ops.alloc_like_segments([(N, 1, h, w, Cout) for h, w in shapes], "cpu")
    if kind == "patch":
        w = torch.zeros((Cout, 9, Cin))
        return dict(xs=xs, outs=outs, w=w), lambda: ops.corr2d_patch_multi(xs, w, outs, 3), lambda: dict(w16=w.__dict__.get("_g6d_c16", {}))
    if kind == "wino":
        U = torch.zeros((25 * (Cin // 8), 16, Cout, 8))
        return dict(xs=xs, outs=outs, U=U), lambda: ops.corr2d_wino_multi(xs, U, outs), None
    kb = kw.get("kblocks", 5)
    U = torch.zeros(ops.w43_shape(kb * kb * (Cin // 8), Cout))
    return dict(xs=xs, outs=outs, U=U), lambda: ops.corr2d_wino43_multi(xs, U, outs, **kw), None


def _c16_filters(mode, Cout, taps, Cin, k=None):
    f = ops.Conv16Filters(torch.zeros(Cout * taps * Cin * (2 if mode == 3 else 1), dtype=ops._T16[mode]), 1, mode, 0.25 if mode == 3 else 1.0,
                          Cout, taps, Cin)
    if k:
        f.k = k
    return f


def _cases():
    """name -> () -> (inputs, call, extra).  Built lazily: the PairMap cases allocate RangeTables."""
    c = {}
    for kind, full, pool in (("wino", True, True), ("wino", True, False), ("wino", False, True), ("wino43", True, True), ("wino43", False, True),
                             ("wino16bf", True, False), ("wino16", True, True)):
        c[f"{kind}_multi full={int(full)} pool={int(pool)}"] = lambda kind=kind, full=full, pool=pool: _trunk_case(kind, full, pool) + (None,)
    c["wino_multi one segment"] = lambda: _trunk_case("wino", True, False, shapes=[(1, 6, 5)]) + (None,)
    c["corr_patch_multi"] = lambda: _corr_case("patch")
    c["corr_patch_multi N=1 two maps"] = lambda: _corr_case("patch", N=1, shapes=((9, 7), (5, 13)))
    c["corr_wino_multi"] = lambda: _corr_case("wino")
    c["corr_wino43_multi"] = lambda: _corr_case("wino43")
    c["corr_wino43_multi N=1 kblocks=3 k_true=7"] = lambda: _corr_case("wino43", N=1, kblocks=3, k_true=7)

    def conv16_plain():
        filt = _c16_filters(2, 16, 9, 8)
        xs = [torch.zeros(s + (8,), dtype=torch.float16) for s in SHAPES[:2]]
        bias, stats = torch.zeros(16), torch.zeros((3, 16, 2), dtype=torch.float64)
        return dict(xs=xs, filt=filt.data, bias=bias, stats=stats), lambda: ops.conv16_direct_multi(
            xs, filt, bias, relu=False, full="t16", pool=torch.float32, stats=stats, rows_per_group=14), None
    c["conv16_direct_multi fp16 t16+pool32 stats"] = conv16_plain

    def conv16_pairs():
        table = ops.RangeTable("cpu")
        filt = _c16_filters(3, 16, 9, 8)
        xs = [ops.PairMap(torch.zeros(s + (2, 8), dtype=torch.float16), table, 5) for s in SHAPES]
        return dict(xs=[x.data for x in xs], filt=filt.data, rng=dict(exps=table.exps, rec=table.rec)), lambda: ops.conv16_direct_multi(
            xs, filt, None, full="t16", pool="t16", rng=(table, 7)), None
    c["conv16_direct_multi pairs rng"] = conv16_pairs

    def conv16_3d_strided():
        filt = _c16_filters(1, 16, 27, 8)
        xs = [torch.zeros((2, 3, 4, 5, 8), dtype=torch.bfloat16)]
        wide = torch.zeros((2, 3, 4, 5, 40))
        return dict(xs=xs, filt=filt.data, wide=wide), lambda: ops.conv16_direct_multi(
            xs, filt, None, full=torch.float32, kd=3, out_full=[wide[..., 8:24]]), None
    c["conv16_direct_multi 3-D strided out_full"] = conv16_3d_strided

    def conv16_given_dense():
        filt = _c16_filters(3, 16, 9, 8)
        xs = [torch.zeros(s + (2, 8), dtype=torch.float16) for s in SHAPES[:2]]
        buf = ops.alloc_like_segments([(s[0] * s[1] * s[2] * 2 * 16 // 2,) for s in SHAPES[:2]], "cpu")
        given = [b.view(torch.float16) for b in buf]
        return dict(xs=xs, filt=filt.data, given=given), lambda: ops.conv16_direct_multi(xs, filt, None, full="t16", out_full=given), None
    c["conv16_direct_multi pairs flat out_full"] = conv16_given_dense

    def corr16_plain():
        filt = _c16_filters(2, 32, 49, 32, k=7)
        xs = [torch.zeros(s + (32,), dtype=torch.float16) for s in SHAPES]
        outs = ops.alloc_like_segments([(s[0], 1, s[1], s[2], 32) for s in SHAPES], "cpu")
        return dict(xs=xs, outs=outs, filt=filt.data), lambda: ops.corr16_multi(xs, filt, outs), None
    c["corr16_multi fp16"] = corr16_plain

    def corr16_pairs():
        table = ops.RangeTable("cpu")
        filt = _c16_filters(3, 32, 225, 32, k=15)
        xs = [ops.PairMap(torch.zeros(s + (2, 32), dtype=torch.float16), table, 3) for s in SHAPES[:2]]
        outs = [torch.zeros(s + (32,)) for s in SHAPES[:2]]
        return dict(xs=[x.data for x in xs], outs=outs, filt=filt.data, rng=dict(exps=table.exps, rec=table.rec)), lambda: ops.corr16_multi(xs, filt, outs), None
    c["corr16_multi pairs"] = corr16_pairs

    def wino_single():
        wide = torch.zeros((2, 9, 7, 24))
        x, U, bias = wide[..., 4:20], torch.zeros((2, 16, 64, 8)), torch.zeros(64)
        return dict(wide=wide, U=U, bias=bias), lambda: ops.wino_conv3x3(x, U, bias, relu=False, full=True, pool=True), None
    c["wino_conv3x3 strided"] = wino_single
    c["wino_conv3x3 pool only"] = lambda: (lambda x, U, b: (dict(x=x, U=U, bias=b), lambda: ops.wino_conv3x3(x, U, b, full=False, pool=True), None))(
        torch.zeros((1, 8, 8, 16)), torch.zeros((2, 16, 64, 8)), torch.zeros(64))

    def corr_single():
        wide, w, out = torch.zeros((1, 1, 9, 7, 40)), torch.zeros((20, 25, 32)), torch.zeros((1, 1, 9, 7, 20))
        return dict(wide=wide, w=w, out=out), lambda: ops.corr2d_patch(wide[..., 8:], w, out, 5), None
    c["corr2d_patch"] = corr_single

    def hbm_users():
        ref, que, sc = torch.zeros((3, 10, 8)), torch.zeros((2, 10, 8)), torch.zeros((2, 8))
        x = torch.zeros((2, 1, 6, 4, 8))

        def call():
            return (ops.product_split16(ref, que, sc, sc, 2), ops.affine_split16(x, sc, sc, 1, True, True, 3),
                    ops.selector_scan(que[0], ref))
        return dict(ref=ref, que=que, sc=sc, x=x), call, None
    c["hbm users"] = hbm_users
    return c


def _conv_case(plan):
    x, w, out = torch.zeros((2, 1, 9, 7, 24))[..., :16], torch.zeros((32, 9, 16)), torch.zeros((2, 1, 9, 7, 32))
    mul, sc, stats = torch.zeros((9, 7, 16)), torch.zeros((1, 16)), torch.zeros((2, 32, 2), dtype=torch.float64)
    return dict(x=x, w=w, out=out, mul=mul, sc=sc, stats=stats), lambda: ops.conv(
        x, w, None, out, ksize=(1, 3, 3), pad=(0, 1, 1), mul=mul, in_scale=sc, in_shift=sc, in_relu=True, stats=stats, rows_per_group=63), None


def _special_cases():
    def patch16(fake):
        with ops.math_mode("fp16"):
            inputs, call, extra = _corr_case("patch")
            return _run(fake, inputs, call, extra=extra)

    def conv_plan(plan):
        def run(fake):
            fake.plan = plan
            inputs, call, extra = _conv_case(plan)
            return _run(fake, inputs, call)
        return run

    def conv_plain(fake):
        x, w, out = torch.zeros((3, 2, 4, 4, 8)), torch.zeros((8, 1, 8)), torch.zeros((3, 2, 4, 4, 8))
        return _run(fake, dict(x=x, w=w, out=out), lambda: ops.conv(x, w, None, out))
    c = {"corr_patch_multi fp16 -> the 16 entry": patch16}
    c.update({f"conv plan={p}": conv_plan(p) for p in (0, 2, 3, 4)})
    c["conv 1x1x1 plain"] = conv_plain
    return c


def _record(fake, name):
    if name in _special_cases():
        return _special_cases()[name](fake)
    inputs, call, extra = _cases()[name]()
    return _run(fake, inputs, call, extra=extra)


CASE_NAMES = list(_cases()) + list(_special_cases())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_wrapper_launch_is_pinned(fake, name):
    assert _record(fake, name) == EXPECTED[name]


def test_every_recorded_case_is_run():
    assert sorted(CASE_NAMES) == sorted(EXPECTED)
    entries = {c[0] for rec in EXPECTED.values() for c in rec["calls"]}
    assert {"g6d_wino_conv3x3_multi", "g6d_wino16_conv3x3_multi", "g6d_wino43_conv3x3_multi", "g6d_corr2d_wino_multi", "g6d_corr2d_wino43_multi",
            "g6d_corr2d_patch_multi", "g6d_corr2d_patch16_multi", "g6d_conv16_direct_multi_ex", "g6d_corr16_multi_ex", "g6d_wino_conv3x3",
            "g6d_corr2d_patch", "g6d_conv_igemm"} <= entries


def test_caller_provided_outputs_come_back(fake):
    """out_full tensors are returned as they were passed, corr outputs likewise; PairMaps carry the output slot of `rng`."""
    filt = _c16_filters(3, 16, 9, 8)
    table = ops.RangeTable("cpu")
    xs = [ops.PairMap(torch.zeros((1, 4, 4, 2, 8), dtype=torch.float16), table, 2)]
    given = [torch.zeros((1, 4, 4, 2, 16), dtype=torch.float16)]
    fulls, pools = ops.conv16_direct_multi(xs, filt, None, full="t16", pool=torch.float32, out_full=given, rng=(table, 9))
    assert isinstance(fulls[0], ops.PairMap) and fulls[0].data is given[0] and fulls[0].table is table and fulls[0].slot == 9
    assert isinstance(pools[0], torch.Tensor) and pools[0].dtype == torch.float32           # fp32 outputs stay plain
    ra = fake.calls[-1][1][-2]._obj
    assert (ra.slot_in, ra.slot_out, ra.exps, ra.rec) == (2, 9, table.exps.data_ptr(), table.rec.data_ptr())
    for kind in ("patch", "wino", "wino43"):
        inputs, call, _ = _corr_case(kind)
        assert call() is inputs["outs"]
    f2 = _c16_filters(2, 32, 49, 32, k=7)
    outs = [torch.zeros((1, 1, 4, 4, 32))]
    assert ops.corr16_multi([torch.zeros((1, 4, 4, 32), dtype=torch.float16)], f2, outs) is outs
    assert fake.calls[-1][1][-2] is None                                                     # no range without PairMaps


def test_wrapper_value_errors(fake):
    Cin, Cout = 16, 64
    x = torch.zeros((1, 6, 6, Cin))
    bias = torch.zeros(Cout)
    trunk = {"wino_conv3x3_multi": torch.zeros((2, 16, Cout, 8)), "wino43_conv3x3_multi": torch.zeros(ops.w43_shape(2, Cout)),
             "wino16_conv3x3_multi": torch.zeros((1, 16, Cout, 16), dtype=torch.float16)}
    for name, U in trunk.items():
        fn = getattr(ops, name)
        for xs in ([], [x] * 5):
            with pytest.raises(ValueError, match=f"{name}: 1..4 segments"):
                fn(xs, U, bias)
        with pytest.raises(ValueError, match=f"{name}: segments must be contiguous"):
            fn([x, torch.zeros((1, 6, 6, 2 * Cin))[..., :Cin]], U, bias)
        with pytest.raises(ValueError, match=f"{name}: segments must be contiguous"):
            fn([x, torch.zeros((1, 6, 6, Cin), dtype=torch.float64)], U, bias)
        with pytest.raises(ValueError, match=f"{name}: segments must be contiguous"):
            fn([x, torch.zeros((1, 6, 6, 2 * Cin))], U, bias)
        with pytest.raises(ValueError, match=f"{name}: U"):
            fn([x], U[..., :2], bias)
    with pytest.raises(ValueError, match="wino_conv3x3_multi: U"):
        ops.wino_conv3x3_multi([x], trunk["wino_conv3x3_multi"], torch.zeros(Cout + 1))
    with pytest.raises(ValueError, match="wino16_conv3x3_multi: U16 must be contiguous bfloat16 / float16"):
        ops.wino16_conv3x3_multi([x], trunk["wino16_conv3x3_multi"].float(), bias)
    m, o = torch.zeros((2, 1, 6, 6, 32)), torch.zeros((2, 1, 6, 6, 32))
    corr = {"corr2d_patch_multi": (torch.zeros((32, 9, 32)), (3,), "maps"), "corr2d_wino_multi": (torch.zeros((100, 16, 32, 8)), (), "map sizes"),
            "corr2d_wino43_multi": (torch.zeros(ops.w43_shape(100, 32)), (), "map sizes")}
    for name, (w, extra, noun) in corr.items():
        fn = getattr(ops, name)
        with pytest.raises(ValueError, match=f"{name}: 1..4 {noun}"):
            fn([m] * 5, w, [o] * 5, *extra)
        with pytest.raises(ValueError, match=f"{name}: 1..4 {noun}"):
            fn([m, m], w, [o], *extra)
        with pytest.raises(ValueError, match=f"{name}: shape mismatch"):
            fn([m], w, [torch.zeros((2, 1, 6, 5, 32))], *extra)
        with pytest.raises(ValueError, match=f"{name}: shape mismatch"):
            fn([torch.zeros((2, 1, 6, 6, 64))[..., :32]], w, [o], *extra)           # batched maps must be dense
        with pytest.raises(ValueError, match=f"{name}: shape mismatch"):
            fn([torch.zeros((1, 2, 6, 6, 32))], w, [torch.zeros((1, 2, 6, 6, 32))], *extra)
    with pytest.raises(ValueError, match="corr2d_patch_multi: 1..4 maps"):
        ops.corr2d_patch_multi([], corr["corr2d_patch_multi"][0], [], 3)
    with pytest.raises(ValueError, match="corr2d_patch_multi: filter shape mismatch"):
        ops.corr2d_patch_multi([m], corr["corr2d_patch_multi"][0], [o], 5)
    with pytest.raises(ValueError, match="corr2d_wino_multi: U must be contiguous"):
        ops.corr2d_wino_multi([m], torch.zeros((36, 16, 32, 8)), [o])
    with pytest.raises(ValueError, match="corr2d_wino43_multi: U43 must be contiguous"):
        ops.corr2d_wino43_multi([m], corr["corr2d_wino43_multi"][0], [o], kblocks=3)
    # a single strided map is fine for the patch kernel (N = 1), not for the Winograd ones
    wide = torch.zeros((1, 1, 6, 6, 64))
    ops.corr2d_patch_multi([wide[..., :32]], corr["corr2d_patch_multi"][0], [torch.zeros((1, 1, 6, 6, 32))], 3)
    with pytest.raises(ValueError, match="corr2d_wino_multi: shape mismatch"):
        ops.corr2d_wino_multi([wide[..., :32]], corr["corr2d_wino_multi"][0], [torch.zeros((1, 1, 6, 6, 32))])
    assert fake.calls[-1][0] == "g6d_corr2d_patch_multi" and len(fake.calls) == 1
    # the 16-bit direct wrappers
    filt = _c16_filters(2, 16, 9, 8)
    h = torch.zeros((1, 4, 4, 8), dtype=torch.float16)
    with pytest.raises(ValueError, match="filters / kd mismatch"):
        ops.conv16_direct_multi([h], filt, None, full="t16", kd=3)
    with pytest.raises(ValueError, match="output types"):
        ops.conv16_direct_multi([h], filt, None, full=torch.float16)
    with pytest.raises(ValueError, match="input 0 must be a dense"):
        ops.conv16_direct_multi([h.float()], filt, None, full="t16")
    with pytest.raises(ValueError, match="input 1 must be a dense"):
        ops.conv16_direct_multi([h, torch.zeros((1, 4, 4, 16), dtype=torch.float16)[..., :8]], filt, None, full="t16")
    with pytest.raises(ValueError, match="out_full must hold"):
        ops.conv16_direct_multi([h], filt, None, full="t16", out_full=[torch.zeros((1, 4, 4, 16))])
    with pytest.raises(ValueError, match="a strided out_full must be an fp32 channel slice"):
        ops.conv16_direct_multi([h], filt, None, full="t16", out_full=[torch.zeros((1, 4, 4, 32), dtype=torch.float16)[..., :16]])
    with pytest.raises(ValueError, match="ranges apply to pairs"):
        ops.conv16_direct_multi([h], filt, None, full="t16", rng=(ops.RangeTable("cpu"), 1))
    table = ops.RangeTable("cpu")
    with pytest.raises(ValueError, match="must all be PairMaps of one slot"):
        ops.conv16_direct_multi([ops.PairMap(h, table, 1), ops.PairMap(h, table, 2)], _c16_filters(3, 16, 9, 8), None, full="t16")
    f2 = _c16_filters(2, 32, 49, 32, k=7)
    g = torch.zeros((1, 4, 4, 32), dtype=torch.float16)
    with pytest.raises(ValueError, match="corr16_multi: dense 16-bit"):
        ops.corr16_multi([g], f2, [torch.zeros((1, 4, 4, 16))])
    with pytest.raises(ValueError, match="corr16_multi: output shape mismatch"):
        ops.corr16_multi([g], f2, [torch.zeros((1, 4, 5, 32))])
    with pytest.raises(ValueError, match="corr16_multi: PairMaps need pair filters"):
        ops.corr16_multi([ops.PairMap(g, table, 1)], f2, [torch.zeros((1, 4, 4, 32))])
    assert len(fake.calls) == 1                                             # none of the refused calls reached the library


# ---- recorded from the wrappers before the refactor (one entry per case of CASE_NAMES) ----------------------------------------------------
EXPECTED = {'wino_multi full=1 pool=1': {'calls': [('g6d_wino_conv3x3_multi',
                                         [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': 'ret[1][0]', 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                           {'in_': 'xs[1]', 'out_full': 'ret[0][1]', 'out_pool': 'ret[1][1]', 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                           {'in_': 'xs[2]', 'out_full': 'ret[0][2]', 'out_pool': 'ret[1][2]', 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                          3, 16, 'U', 'bias', 64, 1, 'ws', 256, 'stream'])],
                              'ret': [[((2, 9, 7, 64), 'float32', (4032, 448, 64, 1), 0), ((1, 8, 8, 64), 'float32', (4096, 512, 64, 1), 8064),
                                       ((3, 5, 13, 64), 'float32', (4160, 832, 64, 1), 12160)],
                                      [((2, 4, 3, 64), 'float32', (768, 192, 64, 1), 0), ((1, 4, 4, 64), 'float32', (1024, 256, 64, 1), 1536),
                                       ((3, 2, 6, 64), 'float32', (768, 384, 64, 1), 2560)]],
                              'log_plain': ['g6d_wino_conv3x3_multi'],
                              'log': ['record', 'g6d_wino_conv3x3_multi', 'record'],
                              'profile': [(3153920.0, 'wino3x3 multi in=2x9x7+1x8x8+3x5x13x16 out=64 full pool', 208192.0)],
                              'hbm': {}},
 'wino_multi full=1 pool=0': {'calls': [('g6d_wino_conv3x3_multi',
                                         [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': None, 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                           {'in_': 'xs[1]', 'out_full': 'ret[0][1]', 'out_pool': None, 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                           {'in_': 'xs[2]', 'out_full': 'ret[0][2]', 'out_pool': None, 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                          3, 16, 'U', 'bias', 64, 1, 'ws', 256, 'stream'])],
                              'ret': [[((2, 9, 7, 64), 'float32', (4032, 448, 64, 1), 0), ((1, 8, 8, 64), 'float32', (4096, 512, 64, 1), 8064),
                                       ((3, 5, 13, 64), 'float32', (4160, 832, 64, 1), 12160)],
                                      None],
                              'log_plain': ['g6d_wino_conv3x3_multi'],
                              'log': ['record', 'g6d_wino_conv3x3_multi', 'record'],
                              'profile': [(3153920.0, 'wino3x3 multi in=2x9x7+1x8x8+3x5x13x16 out=64 full', 188736.0)],
                              'hbm': {}},
 'wino_multi full=0 pool=1': {'calls': [('g6d_wino_conv3x3_multi',
                                         [[{'in_': 'xs[0]', 'out_full': None, 'out_pool': 'ret[1][0]', 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                           {'in_': 'xs[1]', 'out_full': None, 'out_pool': 'ret[1][1]', 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                           {'in_': 'xs[2]', 'out_full': None, 'out_pool': 'ret[1][2]', 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                          3, 16, 'U', 'bias', 64, 1, 'ws', 256, 'stream'])],
                              'ret': [None,
                                      [((2, 4, 3, 64), 'float32', (768, 192, 64, 1), 0), ((1, 4, 4, 64), 'float32', (1024, 256, 64, 1), 1536),
                                       ((3, 2, 6, 64), 'float32', (768, 384, 64, 1), 2560)]],
                              'log_plain': ['g6d_wino_conv3x3_multi'],
                              'log': ['record', 'g6d_wino_conv3x3_multi', 'record'],
                              'profile': [(3153920.0, 'wino3x3 multi in=2x9x7+1x8x8+3x5x13x16 out=64 pool', 109632.0)],
                              'hbm': {}},
 'wino43_multi full=1 pool=1': {'calls': [('g6d_wino43_conv3x3_multi',
                                           [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': 'ret[1][0]', 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                             {'in_': 'xs[1]', 'out_full': 'ret[0][1]', 'out_pool': 'ret[1][1]', 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                             {'in_': 'xs[2]', 'out_full': 'ret[0][2]', 'out_pool': 'ret[1][2]', 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                            3, 16, 'U', 'bias', 64, 0, 'ws', 256, 'stream'])],
                                'ret': [[((2, 9, 7, 64), 'float32', (4032, 448, 64, 1), 0), ((1, 8, 8, 64), 'float32', (4096, 512, 64, 1), 8064),
                                         ((3, 5, 13, 64), 'float32', (4160, 832, 64, 1), 12160)],
                                        [((2, 4, 3, 64), 'float32', (768, 192, 64, 1), 0), ((1, 4, 4, 64), 'float32', (1024, 256, 64, 1), 1536),
                                         ((3, 2, 6, 64), 'float32', (768, 384, 64, 1), 2560)]],
                                'log_plain': ['g6d_wino43_conv3x3_multi'],
                                'log': ['record', 'g6d_wino43_conv3x3_multi', 'record'],
                                'profile': [(1774080.0, 'wino3x3 F43 multi in=2x9x7+1x8x8+3x5x13x16 out=64 full pool', 290112.0, 7096320.0)],
                                'hbm': {}},
 'wino43_multi full=0 pool=1': {'calls': [('g6d_wino43_conv3x3_multi',
                                           [[{'in_': 'xs[0]', 'out_full': None, 'out_pool': 'ret[1][0]', 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                             {'in_': 'xs[1]', 'out_full': None, 'out_pool': 'ret[1][1]', 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                             {'in_': 'xs[2]', 'out_full': None, 'out_pool': 'ret[1][2]', 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                            3, 16, 'U', 'bias', 64, 0, 'ws', 256, 'stream'])],
                                'ret': [None,
                                        [((2, 4, 3, 64), 'float32', (768, 192, 64, 1), 0), ((1, 4, 4, 64), 'float32', (1024, 256, 64, 1), 1536),
                                         ((3, 2, 6, 64), 'float32', (768, 384, 64, 1), 2560)]],
                                'log_plain': ['g6d_wino43_conv3x3_multi'],
                                'log': ['record', 'g6d_wino43_conv3x3_multi', 'record'],
                                'profile': [(1774080.0, 'wino3x3 F43 multi in=2x9x7+1x8x8+3x5x13x16 out=64 pool', 191552.0, 7096320.0)],
                                'hbm': {}},
 'wino16bf_multi full=1 pool=0': {'calls': [('g6d_wino16_conv3x3_multi',
                                             [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': None, 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                               {'in_': 'xs[1]', 'out_full': 'ret[0][1]', 'out_pool': None, 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                               {'in_': 'xs[2]', 'out_full': 'ret[0][2]', 'out_pool': None, 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                              3, 16, 'U', 'bias', 64, 1, 1, 'ws', 256, 'stream'])],
                                  'ret': [[((2, 9, 7, 64), 'float32', (4032, 448, 64, 1), 0), ((1, 8, 8, 64), 'float32', (4096, 512, 64, 1), 8064),
                                           ((3, 5, 13, 64), 'float32', (4160, 832, 64, 1), 12160)],
                                          None],
                                  'log_plain': ['g6d_wino16_conv3x3_multi'],
                                  'log': ['record', 'g6d_wino16_conv3x3_multi', 'record'],
                                  'profile': [(3153920.0, 'wino3x3 bf16 multi in=2x9x7+1x8x8+3x5x13x16 out=64 full', 155968.0)],
                                  'hbm': {}},
 'wino16_multi full=1 pool=1': {'calls': [('g6d_wino16_conv3x3_multi',
                                           [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': 'ret[1][0]', 'N': 2, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                             {'in_': 'xs[1]', 'out_full': 'ret[0][1]', 'out_pool': 'ret[1][1]', 'N': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64},
                                             {'in_': 'xs[2]', 'out_full': 'ret[0][2]', 'out_pool': 'ret[1][2]', 'N': 3, 'H': 5, 'W': 13, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}],
                                            3, 16, 'U', 'bias', 64, 1, 2, 'ws', 256, 'stream'])],
                                'ret': [[((2, 9, 7, 64), 'float32', (4032, 448, 64, 1), 0), ((1, 8, 8, 64), 'float32', (4096, 512, 64, 1), 8064),
                                         ((3, 5, 13, 64), 'float32', (4160, 832, 64, 1), 12160)],
                                        [((2, 4, 3, 64), 'float32', (768, 192, 64, 1), 0), ((1, 4, 4, 64), 'float32', (1024, 256, 64, 1), 1536),
                                         ((3, 2, 6, 64), 'float32', (768, 384, 64, 1), 2560)]],
                                'log_plain': ['g6d_wino16_conv3x3_multi'],
                                'log': ['record', 'g6d_wino16_conv3x3_multi', 'record'],
                                'profile': [(3153920.0, 'wino3x3 fp16 multi in=2x9x7+1x8x8+3x5x13x16 out=64 full pool', 175424.0)],
                                'hbm': {}},
 'wino_multi one segment': {'calls': [('g6d_wino_conv3x3_multi',
                                       [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': None, 'N': 1, 'H': 6, 'W': 5, 'ld_in': 16, 'ld_full': 64, 'ld_pool': 64}], 1, 16, 'U', 'bias',
                                        64, 1, 'ws', 256, 'stream'])],
                            'ret': [[((1, 6, 5, 64), 'float32', (1920, 320, 64, 1), 0)], None],
                            'log_plain': ['g6d_wino_conv3x3_multi'],
                            'log': ['record', 'g6d_wino_conv3x3_multi', 'record'],
                            'profile': [(245760.0, 'wino3x3 multi in=1x6x5x16 out=64 full', 75136.0)],
                            'hbm': {}},
 'corr_patch_multi': {'calls': [('g6d_corr2d_patch_multi',
                                 [[{'in_': 'xs[0]', 'out': 'outs[0]', 'H': 9, 'W': 7, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                   {'in_': 'xs[1]', 'out': 'outs[1]', 'H': 8, 'W': 8, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                   {'in_': 'xs[2]', 'out': 'outs[2]', 'H': 5, 'W': 13, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0}],
                                  3, 32, 'w', 32, 3, 3, 'ws', 256, 0, 'stream'])],
                      'ret': [((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((2, 1, 8, 8, 32), 'float32', (2048, 2048, 256, 32, 1), 4032),
                              ((2, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 8128)],
                      'log_plain': ['g6d_corr2d_patch_multi'],
                      'log': ['record', 'g6d_corr2d_patch_multi', 'record'],
                      'profile': [(7077888.0, 'corr2d_patch multi in=2x9x7+2x8x8+2x5x13x32 out=32 k=3x3', 135168.0)],
                      'hbm': {}},
 'corr_patch_multi N=1 two maps': {'calls': [('g6d_corr2d_patch_multi',
                                              [[{'in_': 'xs[0]', 'out': 'outs[0]', 'H': 9, 'W': 7, 'ld_in': 32, 'ld_out': 32, 'N': 1, 'reserved_': 0},
                                                {'in_': 'xs[1]', 'out': 'outs[1]', 'H': 5, 'W': 13, 'ld_in': 32, 'ld_out': 32, 'N': 1, 'reserved_': 0}],
                                               2, 32, 'w', 32, 3, 3, 'ws', 256, 0, 'stream'])],
                                   'ret': [((1, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((1, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 2016)],
                                   'log_plain': ['g6d_corr2d_patch_multi'],
                                   'log': ['record', 'g6d_corr2d_patch_multi', 'record'],
                                   'profile': [(2359296.0, 'corr2d_patch multi in=9x7+5x13x32 out=32 k=3x3', 69632.0)],
                                   'hbm': {}},
 'corr_wino_multi': {'calls': [('g6d_corr2d_wino_multi',
                                [[{'in_': 'xs[0]', 'out': 'outs[0]', 'H': 9, 'W': 7, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                  {'in_': 'xs[1]', 'out': 'outs[1]', 'H': 8, 'W': 8, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                  {'in_': 'xs[2]', 'out': 'outs[2]', 'H': 5, 'W': 13, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0}],
                                 3, 32, 'U', 32, 5, 'ws', 256, 'stream'])],
                     'ret': [((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((2, 1, 8, 8, 32), 'float32', (2048, 2048, 256, 32, 1), 4032),
                             ((2, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 8128)],
                     'log_plain': ['g6d_corr2d_wino_multi'],
                     'log': ['record', 'g6d_corr2d_wino_multi', 'record'],
                     'profile': [(78643200.0, 'wino3x3 corr multi in=2x9x7+2x8x8+2x5x13x32 out=32 k=15x15 (5x5 blocks of 3x3)', 1736704.0)],
                     'hbm': {}},
 'corr_wino43_multi': {'calls': [('g6d_corr2d_wino43_multi',
                                  [[{'in_': 'xs[0]', 'out': 'outs[0]', 'H': 9, 'W': 7, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                    {'in_': 'xs[1]', 'out': 'outs[1]', 'H': 8, 'W': 8, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                    {'in_': 'xs[2]', 'out': 'outs[2]', 'H': 5, 'W': 13, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0}],
                                   3, 32, 'U', 32, 5, 'ws', 256, 'stream'])],
                       'ret': [((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((2, 1, 8, 8, 32), 'float32', (2048, 2048, 256, 32, 1), 4032),
                               ((2, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 8128)],
                       'log_plain': ['g6d_corr2d_wino43_multi'],
                       'log': ['record', 'g6d_corr2d_wino43_multi', 'record'],
                       'profile': [(44236800.0, 'wino3x3 F43 corr multi in=2x9x7+2x8x8+2x5x13x32 out=32 k=15x15 (5x5 blocks of 3x3)', 3784704.0, 176947200.0)],
                       'hbm': {}},
 'corr_wino43_multi N=1 kblocks=3 k_true=7': {'calls': [('g6d_corr2d_wino43_multi',
                                                         [[{'in_': 'xs[0]', 'out': 'outs[0]', 'H': 9, 'W': 7, 'ld_in': 32, 'ld_out': 32, 'N': 1, 'reserved_': 0},
                                                           {'in_': 'xs[1]', 'out': 'outs[1]', 'H': 8, 'W': 8, 'ld_in': 32, 'ld_out': 32, 'N': 1, 'reserved_': 0},
                                                           {'in_': 'xs[2]', 'out': 'outs[2]', 'H': 5, 'W': 13, 'ld_in': 32, 'ld_out': 32, 'N': 1, 'reserved_': 0}],
                                                          3, 32, 'U', 32, 3, 'ws', 256, 'stream'])],
                                              'ret': [((1, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((1, 1, 8, 8, 32), 'float32', (2048, 2048, 256, 32, 1), 2016),
                                                      ((1, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 4064)],
                                              'log_plain': ['g6d_corr2d_wino43_multi'],
                                              'log': ['record', 'g6d_corr2d_wino43_multi', 'record'],
                                              'profile': [(7962624.0, 'wino3x3 F43 corr multi in=9x7+8x8+5x13x32 out=32 k=7x7 (3x3 blocks of 3x3)', 1376256.0, 19267584.0)],
                                              'hbm': {}},
 'conv16_direct_multi fp16 t16+pool32 stats': {'calls': [('g6d_conv16_direct_multi_ex',
                                                          [[{'in_': 'xs[0]',
                                                             'out_full': 'ret[0][0]',
                                                             'out_pool': 'ret[1][0]',
                                                             'N': 2,
                                                             'D': 1,
                                                             'H': 9,
                                                             'W': 7,
                                                             'ld_in': 8,
                                                             'ld_full': 16,
                                                             'ld_pool': 16},
                                                            {'in_': 'xs[1]',
                                                             'out_full': 'ret[0][1]',
                                                             'out_pool': 'ret[1][1]',
                                                             'N': 1,
                                                             'D': 1,
                                                             'H': 8,
                                                             'W': 8,
                                                             'ld_in': 8,
                                                             'ld_full': 16,
                                                             'ld_pool': 16}],
                                                           2, 8, 'filt', 1, 1.0, 'bias', 16, 1, 0, 1, 2, 2, 'stats', 14, None, 'stream'])],
                                               'ret': [[((2, 9, 7, 16), 'float16', (1008, 112, 16, 1), 0), ((1, 8, 8, 16), 'float16', (1024, 128, 16, 1), None)],
                                                       [((2, 4, 3, 16), 'float32', (192, 48, 16, 1), 0), ((1, 4, 4, 16), 'float32', (256, 64, 16, 1), None)]],
                                               'log_plain': ['g6d_conv16_direct_multi_ex'],
                                               'log': ['record', 'g6d_conv16_direct_multi_ex', 'record'],
                                               'profile': [(437760.0, 'conv16 direct in=2x9x7+1x8x8x8 out=16 k=3x3 full pool stats', 13984.0, 437760.0)],
                                               'hbm': {}},
 'conv16_direct_multi pairs rng': {'calls': [('g6d_conv16_direct_multi_ex',
                                              [[{'in_': 'xs[0]', 'out_full': 'ret[0][0]', 'out_pool': 'ret[1][0]', 'N': 2, 'D': 1, 'H': 9, 'W': 7, 'ld_in': 16, 'ld_full': 32, 'ld_pool': 32},
                                                {'in_': 'xs[1]', 'out_full': 'ret[0][1]', 'out_pool': 'ret[1][1]', 'N': 1, 'D': 1, 'H': 8, 'W': 8, 'ld_in': 16, 'ld_full': 32, 'ld_pool': 32},
                                                {'in_': 'xs[2]',
                                                 'out_full': 'ret[0][2]',
                                                 'out_pool': 'ret[1][2]',
                                                 'N': 3,
                                                 'D': 1,
                                                 'H': 5,
                                                 'W': 13,
                                                 'ld_in': 16,
                                                 'ld_full': 32,
                                                 'ld_pool': 32}],
                                               3, 8, 'filt', 1, 0.25, None, 16, 1, 1, 3, 3, 3, None, 0, {'exps': 'rng.exps', 'rec': 'rng.rec', 'slot_in': 5, 'slot_out': 7}, 'stream'])],
                                   'ret': [[('PairMap', 7, (2, 9, 7, 2, 16), 'float16', (2016, 224, 32, 16, 1), 0), ('PairMap', 7, (1, 8, 8, 2, 16), 'float16', (2048, 256, 32, 16, 1), None),
                                            ('PairMap', 7, (3, 5, 13, 2, 16), 'float16', (2080, 416, 32, 16, 1), None)],
                                           [('PairMap', 7, (2, 4, 3, 2, 16), 'float16', (384, 96, 32, 16, 1), 0), ('PairMap', 7, (1, 4, 4, 2, 16), 'float16', (512, 128, 32, 16, 1), None),
                                            ('PairMap', 7, (3, 2, 6, 2, 16), 'float16', (384, 192, 32, 16, 1), None)]],
                                   'log_plain': ['g6d_conv16_direct_multi_ex'],
                                   'log': ['record', 'g6d_conv16_direct_multi_ex', 'record'],
                                   'profile': [(887040.0, 'conv16x3 direct in=2x9x7+1x8x8+3x5x13x8 out=16 k=3x3 full pool', 46432.0, 887040.0)],
                                   'hbm': {}},
 'conv16_direct_multi 3-D strided out_full': {'calls': [('g6d_conv16_direct_multi_ex',
                                                         [[{'in_': 'xs[0]',
                                                            'out_full': 'wide+32',
                                                            'out_pool': None,
                                                            'N': 2,
                                                            'D': 3,
                                                            'H': 4,
                                                            'W': 5,
                                                            'ld_in': 8,
                                                            'ld_full': 40,
                                                            'ld_pool': 0}],
                                                          1, 8, 'filt', 1, 1.0, None, 16, 3, 1, 2, 0, 1, None, 0, None, 'stream'])],
                                              'ret': [[((2, 3, 4, 5, 16), 'float32', (2400, 800, 200, 40, 1), 0)], [None]],
                                              'log_plain': ['g6d_conv16_direct_multi_ex'],
                                              'log': ['record', 'g6d_conv16_direct_multi_ex', 'record'],
                                              'profile': [(829440.0, 'conv16 direct in=2x3x4x5x8 out=16 k=3x3x3 full', 16512.0, 829440.0)],
                                              'hbm': {}},
 'conv16_direct_multi pairs flat out_full': {'calls': [('g6d_conv16_direct_multi_ex',
                                                        [[{'in_': 'xs[0]',
                                                           'out_full': 'given[0]',
                                                           'out_pool': None,
                                                           'N': 2,
                                                           'D': 1,
                                                           'H': 9,
                                                           'W': 7,
                                                           'ld_in': 16,
                                                           'ld_full': 32,
                                                           'ld_pool': 0},
                                                          {'in_': 'xs[1]',
                                                           'out_full': 'given[1]',
                                                           'out_pool': None,
                                                           'N': 1,
                                                           'D': 1,
                                                           'H': 8,
                                                           'W': 8,
                                                           'ld_in': 16,
                                                           'ld_full': 32,
                                                           'ld_pool': 0}],
                                                         2, 8, 'filt', 1, 0.25, None, 16, 1, 1, 3, 0, 3, None, 0, None, 'stream'])],
                                             'ret': [[((4032,), 'float16', (1,), 0), ((2048,), 'float16', (1,), 4032)], [None, None]],
                                             'log_plain': ['g6d_conv16_direct_multi_ex'],
                                             'log': ['record', 'g6d_conv16_direct_multi_ex', 'record'],
                                             'profile': [(437760.0, 'conv16x3 direct in=2x9x7+1x8x8x8 out=16 k=3x3 full', 22848.0, 437760.0)],
                                             'hbm': {}},
 'corr16_multi fp16': {'calls': [('g6d_corr16_multi_ex',
                                  [[{'in_': 'xs[0]', 'out_full': 'outs[0]', 'out_pool': None, 'N': 2, 'D': 1, 'H': 9, 'W': 7, 'ld_in': 32, 'ld_full': 32, 'ld_pool': 0},
                                    {'in_': 'xs[1]', 'out_full': 'outs[1]', 'out_pool': None, 'N': 1, 'D': 1, 'H': 8, 'W': 8, 'ld_in': 32, 'ld_full': 32, 'ld_pool': 0},
                                    {'in_': 'xs[2]', 'out_full': 'outs[2]', 'out_pool': None, 'N': 3, 'D': 1, 'H': 5, 'W': 13, 'ld_in': 32, 'ld_full': 32, 'ld_pool': 0}],
                                   3, 32, 'filt', 1.0, 32, 7, 2, None, 'stream'])],
                       'ret': [((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((1, 1, 8, 8, 32), 'float32', (2048, 2048, 256, 32, 1), 4032),
                               ((3, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 6080)],
                       'log_plain': ['g6d_corr16_multi_ex'],
                       'log': ['record', 'g6d_corr16_multi_ex', 'record'],
                       'profile': [(38635520.0, 'conv16 corr in=2x9x7+1x8x8+3x5x13x32 out=32 k=7x7', 174272.0, 38635520.0)],
                       'hbm': {}},
 'corr16_multi pairs': {'calls': [('g6d_corr16_multi_ex',
                                   [[{'in_': 'xs[0]', 'out_full': 'outs[0]', 'out_pool': None, 'N': 2, 'D': 1, 'H': 9, 'W': 7, 'ld_in': 64, 'ld_full': 32, 'ld_pool': 0},
                                     {'in_': 'xs[1]', 'out_full': 'outs[1]', 'out_pool': None, 'N': 1, 'D': 1, 'H': 8, 'W': 8, 'ld_in': 64, 'ld_full': 32, 'ld_pool': 0}],
                                    2, 32, 'filt', 0.25, 32, 15, 3, {'exps': 'rng.exps', 'rec': 'rng.rec', 'slot_in': 3, 'slot_out': -1}, 'stream'])],
                        'ret': [((2, 9, 7, 32), 'float32', (2016, 224, 32, 1), 0), ((1, 8, 8, 32), 'float32', (2048, 256, 32, 1), None)],
                        'log_plain': ['g6d_corr16_multi_ex'],
                        'log': ['record', 'g6d_corr16_multi_ex', 'record'],
                        'profile': [(87552000.0, 'conv16x3 corr in=2x9x7+1x8x8x32 out=32 k=15x15', 970240.0, 87552000.0)],
                        'hbm': {}},
 'wino_conv3x3 strided': {'calls': [('g6d_wino_conv3x3', ['wide+16', 2, 9, 7, 16, 24, 'U', 'bias', 64, 0, 'ret[0]', 64, 'ret[1]', 64, 'ws', 256, 'stream'])],
                          'ret': [((2, 9, 7, 64), 'float32', (4032, 448, 64, 1), 0), ((2, 4, 3, 64), 'float32', (768, 192, 64, 1), None)],
                          'log_plain': ['g6d_wino_conv3x3'],
                          'log': ['record', 'g6d_wino_conv3x3', 'record'],
                          'profile': [(1032192.0, 'wino3x3 N=2 in=9x7x16 out=64 full pool', 112000.0)],
                          'hbm': {}},
 'wino_conv3x3 pool only': {'calls': [('g6d_wino_conv3x3', ['x', 1, 8, 8, 16, 16, 'U', 'bias', 64, 1, None, 64, 'ret[1]', 64, 'ws', 256, 'stream'])],
                            'ret': [None, ((1, 4, 4, 64), 'float32', (1024, 256, 64, 1), 0)],
                            'log_plain': ['g6d_wino_conv3x3'],
                            'log': ['record', 'g6d_wino_conv3x3', 'record'],
                            'profile': [(524288.0, 'wino3x3 N=1 in=8x8x16 out=64 pool', 73728.0)],
                            'hbm': {}},
 'corr2d_patch': {'calls': [('g6d_corr2d_patch', ['wide+32', 9, 7, 32, 40, 'w', 20, 5, 5, 'out', 20, 'ws', 256, 0, 'stream'])],
                  'ret': ((1, 1, 9, 7, 20), 'float32', (1260, 1260, 140, 20, 1), None),
                  'log_plain': ['g6d_corr2d_patch'],
                  'log': ['record', 'g6d_corr2d_patch', 'record'],
                  'profile': [(2016000.0, 'corr2d_patch in=9x7x32 out=20 k=5x5', 77104.0)],
                  'hbm': {}},
 'hbm users': {'calls': [('g6d_product_split16_ex', ['ref', 'que', 'sc', 'sc', 'ret[0]', 2, 3, 10, 8, 2, None, 'stream']),
                         ('g6d_affine_split16_ex', ['x', 8, 'sc', 'sc', 1, 1, 1, 2, 6, 4, 8, 'ret[1]', 3, None, 'stream']),
                         ('g6d_selector_scan', ['que', 'ref', 3, 10, 8, 'ret[2][0]', 'ret[2][1]', 'stream'])],
               'ret': [((6, 10, 8), 'float16', (80, 8, 1), None), ((2, 3, 2, 2, 8), 'float16', (96, 32, 16, 8, 1), None), [((3, 10), 'float32', (10, 1), 0), ((3,), 'float32', (1,), None)]],
               'log_plain': ['g6d_product_split16_ex', 'g6d_affine_split16_ex', 'g6d_selector_scan'],
               'log': ['record', 'g6d_product_split16_ex', 'record', 'record', 'g6d_affine_split16_ex', 'record', 'record', 'g6d_selector_scan', 'record'],
               'profile': [],
               'hbm': {'product_split16': [(2560.0,)], 'affine_split16': [(1920.0,)], 'selector_scan': [(1532.0,)]}},
 'corr_patch_multi fp16 -> the 16 entry': {'calls': [('g6d_corr2d_patch16_multi',
                                                      [[{'in_': 'xs[0]', 'out': 'outs[0]', 'H': 9, 'W': 7, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                                        {'in_': 'xs[1]', 'out': 'outs[1]', 'H': 8, 'W': 8, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0},
                                                        {'in_': 'xs[2]', 'out': 'outs[2]', 'H': 5, 'W': 13, 'ld_in': 32, 'ld_out': 32, 'N': 2, 'reserved_': 0}],
                                                       3, 32, 'w16.2', 32, 3, 3, 'ws', 256, 2, 'stream'])],
                                           'ret': [((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), 0), ((2, 1, 8, 8, 32), 'float32', (2048, 2048, 256, 32, 1), 4032),
                                                   ((2, 1, 5, 13, 32), 'float32', (2080, 2080, 416, 32, 1), 8128)],
                                           'log_plain': ['g6d_corr2d_patch16_multi'],
                                           'log': ['record', 'g6d_corr2d_patch16_multi', 'record'],
                                           'profile': [(7077888.0, 'corr2d_patch16 multi in=2x9x7+2x8x8+2x5x13x32 out=32 k=3x3', 135168.0)],
                                           'hbm': {}},
 'conv plan=0': {'calls': [('g6d_conv_igemm',
                            [{'in_': 'x',
                              'mul': 'mul',
                              'in_scale': 'sc',
                              'in_shift': 'sc',
                              'weight': 'w',
                              'bias': None,
                              'out': 'out',
                              'stats': 'stats',
                              'workspace': 'ws',
                              'workspace_bytes': 256,
                              'N': 2,
                              'Di': 1,
                              'Hi': 9,
                              'Wi': 7,
                              'Cin': 16,
                              'ld_in': 24,
                              'Do': 1,
                              'Ho': 9,
                              'Wo': 7,
                              'Cout': 32,
                              'ld_out': 32,
                              'kd': 1,
                              'kh': 3,
                              'kw': 3,
                              'sd': 1,
                              'sh': 1,
                              'sw': 1,
                              'pd': 0,
                              'ph': 1,
                              'pw': 1,
                              'in_relu': 1,
                              'in_affine_per_n': 0,
                              'out_act': 0,
                              'stat_rows_per_group': 63,
                              'split_k': 0,
                              'math_mode': 0,
                              'weight_wino': None,
                              'fin_scale': None,
                              'fin_shift': None,
                              'fin_counter': None,
                              'fin_count': 0.0,
                              'fin_eps': 0.0,
                              'fin_groups': 0,
                              'in_image_mod': 0,
                              'mul_group_images': 0,
                              'reserved_': 0,
                              'weight_wino16': None,
                              'weight_wino43': None},
                             'stream'])],
                 'ret': ((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), None),
                 'log_plain': ['g6d_conv_igemm'],
                 'log': ['record', 'g6d_conv_igemm', 'record', 'g6d_conv_plan'],
                 'profile': [(1161216.0, 'conv N=2 in=1x9x7x16 out=1x9x7x32 k=1x3x3 s=111 mul aff stats', 46656.0, 1161216.0)],
                 'hbm': {}},
 'conv plan=2': {'calls': [('g6d_conv_igemm',
                            [{'in_': 'x',
                              'mul': 'mul',
                              'in_scale': 'sc',
                              'in_shift': 'sc',
                              'weight': 'w',
                              'bias': None,
                              'out': 'out',
                              'stats': 'stats',
                              'workspace': 'ws',
                              'workspace_bytes': 256,
                              'N': 2,
                              'Di': 1,
                              'Hi': 9,
                              'Wi': 7,
                              'Cin': 16,
                              'ld_in': 24,
                              'Do': 1,
                              'Ho': 9,
                              'Wo': 7,
                              'Cout': 32,
                              'ld_out': 32,
                              'kd': 1,
                              'kh': 3,
                              'kw': 3,
                              'sd': 1,
                              'sh': 1,
                              'sw': 1,
                              'pd': 0,
                              'ph': 1,
                              'pw': 1,
                              'in_relu': 1,
                              'in_affine_per_n': 0,
                              'out_act': 0,
                              'stat_rows_per_group': 63,
                              'split_k': 0,
                              'math_mode': 0,
                              'weight_wino': None,
                              'fin_scale': None,
                              'fin_shift': None,
                              'fin_counter': None,
                              'fin_count': 0.0,
                              'fin_eps': 0.0,
                              'fin_groups': 0,
                              'in_image_mod': 0,
                              'mul_group_images': 0,
                              'reserved_': 0,
                              'weight_wino16': None,
                              'weight_wino43': None},
                             'stream'])],
                 'ret': ((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), None),
                 'log_plain': ['g6d_conv_igemm'],
                 'log': ['record', 'g6d_conv_igemm', 'record', 'g6d_conv_plan'],
                 'profile': [(516096.0, 'wino3x3 conv N=2 in=1x9x7x16 out=1x9x7x32 k=1x3x3 s=111 mul aff stats', 46656.0, 1161216.0)],
                 'hbm': {}},
 'conv plan=3': {'calls': [('g6d_conv_igemm',
                            [{'in_': 'x',
                              'mul': 'mul',
                              'in_scale': 'sc',
                              'in_shift': 'sc',
                              'weight': 'w',
                              'bias': None,
                              'out': 'out',
                              'stats': 'stats',
                              'workspace': 'ws',
                              'workspace_bytes': 256,
                              'N': 2,
                              'Di': 1,
                              'Hi': 9,
                              'Wi': 7,
                              'Cin': 16,
                              'ld_in': 24,
                              'Do': 1,
                              'Ho': 9,
                              'Wo': 7,
                              'Cout': 32,
                              'ld_out': 32,
                              'kd': 1,
                              'kh': 3,
                              'kw': 3,
                              'sd': 1,
                              'sh': 1,
                              'sw': 1,
                              'pd': 0,
                              'ph': 1,
                              'pw': 1,
                              'in_relu': 1,
                              'in_affine_per_n': 0,
                              'out_act': 0,
                              'stat_rows_per_group': 63,
                              'split_k': 0,
                              'math_mode': 0,
                              'weight_wino': None,
                              'fin_scale': None,
                              'fin_shift': None,
                              'fin_counter': None,
                              'fin_count': 0.0,
                              'fin_eps': 0.0,
                              'fin_groups': 0,
                              'in_image_mod': 0,
                              'mul_group_images': 0,
                              'reserved_': 0,
                              'weight_wino16': None,
                              'weight_wino43': None},
                             'stream'])],
                 'ret': ((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), None),
                 'log_plain': ['g6d_conv_igemm'],
                 'log': ['record', 'g6d_conv_igemm', 'record', 'g6d_conv_plan'],
                 'profile': [(290304.0, 'wino3x3 F43 conv N=2 in=1x9x7x16 out=1x9x7x32 k=1x3x3 s=111 mul aff stats', 46656.0, 1161216.0)],
                 'hbm': {}},
 'conv plan=4': {'calls': [('g6d_conv_igemm',
                            [{'in_': 'x',
                              'mul': 'mul',
                              'in_scale': 'sc',
                              'in_shift': 'sc',
                              'weight': 'w',
                              'bias': None,
                              'out': 'out',
                              'stats': 'stats',
                              'workspace': 'ws',
                              'workspace_bytes': 256,
                              'N': 2,
                              'Di': 1,
                              'Hi': 9,
                              'Wi': 7,
                              'Cin': 16,
                              'ld_in': 24,
                              'Do': 1,
                              'Ho': 9,
                              'Wo': 7,
                              'Cout': 32,
                              'ld_out': 32,
                              'kd': 1,
                              'kh': 3,
                              'kw': 3,
                              'sd': 1,
                              'sh': 1,
                              'sw': 1,
                              'pd': 0,
                              'ph': 1,
                              'pw': 1,
                              'in_relu': 1,
                              'in_affine_per_n': 0,
                              'out_act': 0,
                              'stat_rows_per_group': 63,
                              'split_k': 0,
                              'math_mode': 0,
                              'weight_wino': None,
                              'fin_scale': None,
                              'fin_shift': None,
                              'fin_counter': None,
                              'fin_count': 0.0,
                              'fin_eps': 0.0,
                              'fin_groups': 0,
                              'in_image_mod': 0,
                              'mul_group_images': 0,
                              'reserved_': 0,
                              'weight_wino16': None,
                              'weight_wino43': None},
                             'stream'])],
                 'ret': ((2, 1, 9, 7, 32), 'float32', (2016, 2016, 224, 32, 1), None),
                 'log_plain': ['g6d_conv_igemm'],
                 'log': ['record', 'g6d_conv_igemm', 'record', 'g6d_conv_plan'],
                 'profile': [],
                 'hbm': {'conv_narrow': [(42624.0,)]}},
 'conv 1x1x1 plain': {'calls': [('g6d_conv_igemm',
                                 [{'in_': 'x',
                                   'mul': None,
                                   'in_scale': None,
                                   'in_shift': None,
                                   'weight': 'w',
                                   'bias': None,
                                   'out': 'out',
                                   'stats': None,
                                   'workspace': 'ws',
                                   'workspace_bytes': 256,
                                   'N': 3,
                                   'Di': 2,
                                   'Hi': 4,
                                   'Wi': 4,
                                   'Cin': 8,
                                   'ld_in': 8,
                                   'Do': 2,
                                   'Ho': 4,
                                   'Wo': 4,
                                   'Cout': 8,
                                   'ld_out': 8,
                                   'kd': 1,
                                   'kh': 1,
                                   'kw': 1,
                                   'sd': 1,
                                   'sh': 1,
                                   'sw': 1,
                                   'pd': 0,
                                   'ph': 0,
                                   'pw': 0,
                                   'in_relu': 0,
                                   'in_affine_per_n': 0,
                                   'out_act': 0,
                                   'stat_rows_per_group': 0,
                                   'split_k': 0,
                                   'math_mode': 0,
                                   'weight_wino': None,
                                   'fin_scale': None,
                                   'fin_shift': None,
                                   'fin_counter': None,
                                   'fin_count': 0.0,
                                   'fin_eps': 0.0,
                                   'fin_groups': 0,
                                   'in_image_mod': 0,
                                   'mul_group_images': 0,
                                   'reserved_': 0,
                                   'weight_wino16': None,
                                   'weight_wino43': None},
                                  'stream'])],
                      'ret': ((3, 2, 4, 4, 8), 'float32', (256, 128, 32, 8, 1), None),
                      'log_plain': ['g6d_conv_igemm'],
                      'log': ['record', 'g6d_conv_igemm', 'record', 'g6d_conv_plan'],
                      'profile': [(12288.0, 'conv N=3 in=2x4x4x8 out=2x4x4x8 k=1x1x1 s=111', 6400.0, 12288.0)],
                      'hbm': {}}}
