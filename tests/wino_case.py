"""Test infrastructure of the Winograd sweep (tests/wino_sweep.py): the operands of a case from its seed, its float64 reference, the
segment table and the calls of its entry point and of g6d_wino_multi_route through gen6d_amd.lib — with explicit row lengths and an
explicit workspace pointer and byte count, on addresses the caller supplies (fake ones on a host without a GPU, tests/launch_contract.py;
the buffers of `Live` on the GPU) — and the grading in the suite's metric: max |error| / max |reference| per segment and output kind."""
import ctypes as C

import torch
import torch.nn.functional as F

import ref_ops
import wino_sweep as S
from gen6d_amd import lib

SENTINEL = -777.0
DT16 = {1: torch.bfloat16, 2: torch.float16}


class knobs:
    """with knobs(case): the case's knobs are set, and reset afterwards."""

    def __init__(self, case):
        self.case = case

    def __enter__(self):
        for k, v in self.case.get("knobs", {}).items():
            lib.set_knob(k, v)

    def __exit__(self, *exc):
        lib.reset_knobs()
        return False


def _rand(g, *shape, scale=1.0):
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def k_of(case):
    """Side of the correlation filter the case's reference runs (kd 9 with k7: the 7x7 filters the launch sees zero-extended)."""
    return 7 if case["k7"] else 3 * case["kb"]


def operands(case):
    """-> dict(xs [N,H,W,Cin] per segment, w ([Cout,Cin,3,3]; correlations [Cout,k*k,Cin]), bias or None), fp32 on the CPU."""
    g = torch.Generator().manual_seed(36_000_000 + case["seed"])
    Cin, Cout = case["Cin"], case["Cout"]
    if case["kb"]:
        k = k_of(case)
        w = _rand(g, Cout, k * k, Cin, scale=(1.0 / (k * k * Cin)) ** 0.5)
    else:
        w = _rand(g, Cout, Cin, 3, 3, scale=(2.0 / (9 * Cin)) ** 0.5 * 1.7)
    bias = _rand(g, Cout, scale=0.3) if case["bias"] else None
    return dict(xs=[_rand(g, N, H, W, Cin) for N, H, W in case["segs"]], w=w, bias=bias)


def filters(case, o):
    """The launch's filter operand, from the package's own host transforms."""
    from gen6d_amd.network import backbone as B
    fam, w = case["fam"], o["w"]
    if fam == "F2":
        return B.winograd_filters(w)
    if fam == "W16":
        return B.winograd_filters16(w, DT16[case["mode"]])
    if fam == "F4":
        return B.winograd43_filters(w)
    if fam == "F2C":
        return B.winograd_corr_filters(w, 15)
    if case["k7"]:
        U, kb = B.winograd43_corr_filters_padded(w, 7)
        assert kb == 3
        return U
    return B.winograd43_corr_filters(w, 3 * case["kb"])


def _conv(case, o, dtype):
    """Per segment (full, pool) in `dtype`, channels-last: F.conv2d + bias (+ ReLU) (+ max_pool2d), or the direct correlation."""
    out = []
    w = o["w"].to(dtype)
    for x in o["xs"]:
        if case["kb"]:
            y = torch.empty((x.shape[0], 1) + tuple(x.shape[1:3]) + (case["Cout"],), dtype=dtype)
            ref_ops.corr2d_patch(x.to(dtype)[:, None], w, y, k_of(case))
            out.append((y[:, 0], None))
            continue
        y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w, o["bias"].to(dtype) if o["bias"] is not None else None, padding=1)
        if case["relu"]:
            y = F.relu(y)
        yp = F.max_pool2d(y, 2, 2).permute(0, 2, 3, 1) if case["pool"] else None
        out.append((y.permute(0, 2, 3, 1) if case["full"] else None, yp))
    return out


def reference(case, o):
    return _conv(case, o, torch.float64)


def fp32_comparator(case, o):
    """torch's own fp32 convolution (the correlations: the fp32 direct correlation): the conditioning yardstick of the fp32 families."""
    return _conv(case, o, torch.float32)


def restatement16(case, o):
    """tests/ref_ops.py wino16_conv3x3_multi: the 16-bit kernel's arithmetic on the host-rounded filters, in float64."""
    bias = (o["bias"] if o["bias"] is not None else torch.zeros(case["Cout"])).double()
    ys, yps = ref_ops.wino16_conv3x3_multi([x.double() for x in o["xs"]], filters(case, o), bias, relu=bool(case["relu"]), full=case["full"], pool=case["pool"])
    return [(ys[i] if ys else None, yps[i] if yps else None) for i in range(len(o["xs"]))]


def where(got, want, tile):
    """Diagnostic: coordinates (n, h, w, c) of the worst element and the error pattern by position modulo the tile."""
    d = (got.double() - want.double()).abs()
    idx = torch.nonzero(d == d.max())[0].tolist()
    pat = d.amax(dim=(0, 3))
    rows = ["%.1e" % pat[i::tile].max().item() if i < pat.shape[0] else "-" for i in range(tile)]
    cols = ["%.1e" % pat[:, j::tile].max().item() if j < pat.shape[1] else "-" for j in range(tile)]
    return f"worst at (n, h, w, c) = {idx}, h % {tile} = {idx[1] % tile}, w % {tile} = {idx[2] % tile}; by row % {tile} {rows}; by col % {tile} {cols}"


def grade(case, ref, got, bar):
    """-> (worst error / bar, failures): every segment and output kind of `got` against `ref` (lists of (full, pool))."""
    worst, fails = 0.0, []
    tile = 4 if case["fam"] in S.F4_FAMS else 8
    for i, (r, g) in enumerate(zip(ref, got)):
        for kind, rr, gg in (("full", r[0], g[0]), ("pool", r[1], g[1])):
            if rr is None:
                assert gg is None
                continue
            rng = rr.abs().max().item()
            e = (gg.double() - rr.double()).abs().max().item() / max(rng, 1e-30)
            worst = max(worst, e / bar)
            if not e <= bar:
                fails.append(f"{case['id']} {kind} segment {i} {tuple(rr.shape)}: {e:.3e} > {bar:.1e}; {where(gg, rr, tile)}")
    return worst, fails


def ranges(ref):
    return [t.abs().max().item() for r in ref for t in r if t is not None]


# ------------------------------------------------------------------------------------------------------------------ tables and calls
def table(case, in_base, full_base, pool_base):
    """The case's segment table on the three buffer addresses (tests/wino_sweep.py layout): G6dCorrSeg rows for the correlations."""
    in_offs, full_offs, pool_offs, _ = S.layout(case)
    ld_in, ldf, ldp = S.ld_in_of(case), case["Cout"] + case["ldf"], case["Cout"] + case["ldp"]
    n = len(case["segs"])
    if case["kb"]:
        t = (lib.G6dCorrSeg * n)()
        for i, (N, H, W) in enumerate(case["segs"]):
            t[i] = lib.G6dCorrSeg(in_=in_base + 4 * (in_offs[i] + case["c_off"]), out=full_base + 4 * full_offs[i], H=H, W=W, ld_in=ld_in, ld_out=ldf, N=N)
        return t
    t = (lib.G6dWinoSeg * n)()
    for i, (N, H, W) in enumerate(case["segs"]):
        t[i] = lib.G6dWinoSeg(in_=in_base + 4 * (in_offs[i] + case["c_off"]), out_full=full_base + 4 * full_offs[i] if case["full"] else None,
                              out_pool=pool_base + 4 * pool_offs[i] if case["pool"] else None, N=N, H=H, W=W, ld_in=ld_in, ld_full=ldf if case["full"] else 0,
                              ld_pool=ldp if case["pool"] else 0)
    return t


def route(case, t, U, ws, ws_bytes):
    """g6d_wino_multi_route for the case's launch -> (rc, lib.G6dWinoRoute).  ws: the workspace address or None."""
    r = lib.G6dWinoRoute()
    rc = lib.load().g6d_wino_multi_route(lib.WINO_ROUTE_ENTRIES[case["entry"]], t, len(case["segs"]), case["Cin"], C.c_void_p(U), case["Cout"], case["kb"], case["mode"],
                                         C.c_void_p(ws), ws_bytes, C.byref(r))
    return rc, r


def routes(case, t, U, ws):
    """-> (rc, the report with the case's workspace bytes, the report with ample room): what classify_case files a case by."""
    rc, r = route(case, t, U, ws if case["ws"] is not None else None, case["ws"] or 0)
    rc2, ra = route(case, t, U, ws, S.AMPLE)
    return rc or rc2, r, ra


def launch(case, t, U, bias, ws, stream):
    """The case's entry point -> rc.  An output kind the case does not ask for and a bias it does not have are passed as NULL."""
    l = lib.load()
    ws_p, ws_b = (C.c_void_p(ws), case["ws"]) if case["ws"] is not None else (None, 0)
    n, Cin, Cout = len(case["segs"]), case["Cin"], case["Cout"]
    U, bias = C.c_void_p(U), C.c_void_p(bias) if case["bias"] else None
    if case["single"]:
        g = t[0]
        return l.g6d_wino_conv3x3(g.in_, g.N, g.H, g.W, Cin, g.ld_in, U, bias, Cout, case["relu"], g.out_full, g.ld_full, g.out_pool, g.ld_pool, ws_p, ws_b, stream)
    if case["fam"] == "F2":
        return l.g6d_wino_conv3x3_multi(t, n, Cin, U, bias, Cout, case["relu"], ws_p, ws_b, stream)
    if case["fam"] == "W16":
        return l.g6d_wino16_conv3x3_multi(t, n, Cin, U, bias, Cout, case["relu"], case["mode"], ws_p, ws_b, stream)
    if case["fam"] == "F4":
        return l.g6d_wino43_conv3x3_multi(t, n, Cin, U, bias, Cout, case["relu"], ws_p, ws_b, stream)
    if case["fam"] == "F2C":
        return l.g6d_corr2d_wino_multi(t, n, Cin, U, Cout, case["kb"], ws_p, ws_b, stream)
    return l.g6d_corr2d_wino43_multi(t, n, Cin, U, Cout, case["kb"], ws_p, ws_b, stream)


class Live:
    """The device buffers of a case: ONE input buffer (NaN wherever no segment's Cin-channel slice lies: row slack, alignment gaps, a
    row of padding at the end) and one buffer per output kind, prefilled with SENTINEL."""

    def __init__(self, case, o, dev):
        self.case = case
        in_offs, full_offs, pool_offs, tot = S.layout(case)
        ld_in, Cin, Cout = S.ld_in_of(case), case["Cin"], case["Cout"]
        self.inbuf = torch.full((tot[0] + ld_in,), float("nan"), dtype=torch.float32, device=dev)
        for (N, H, W), off, x in zip(case["segs"], in_offs, o["xs"]):
            self.inbuf[off:off + N * H * W * ld_in].view(N, H, W, ld_in)[..., case["c_off"]:case["c_off"] + Cin] = x.to(dev)
        self.full = torch.empty((max(tot[1], 4),), dtype=torch.float32, device=dev) if case["full"] else None
        self.pool = torch.empty((max(tot[2], 4),), dtype=torch.float32, device=dev) if case["pool"] else None
        self.U = filters(case, o).to(dev).contiguous()
        self.bias = o["bias"].to(dev) if o["bias"] is not None else None
        self.views = []
        for (N, H, W), fo, po in zip(case["segs"], full_offs, pool_offs):
            ldf, ldp = Cout + case["ldf"], Cout + case["ldp"]
            self.views.append((self.full[fo:fo + N * H * W * ldf].view(N, H, W, ldf) if case["full"] else None,
                               self.pool[po:po + N * (H // 2) * (W // 2) * ldp].view(N, H // 2, W // 2, ldp) if case["pool"] else None))
        self.table = table(case, self.inbuf.data_ptr(), self.full.data_ptr() if case["full"] else 0, self.pool.data_ptr() if case["pool"] else 0)

    def prefill(self):
        for b in (self.full, self.pool):
            if b is not None:
                b.fill_(SENTINEL)

    def maps(self):
        """Per segment (full, pool) on the CPU: the Cout-channel slices of the output rows."""
        Cout = self.case["Cout"]
        return [tuple(v[..., :Cout].cpu() if v is not None else None for v in seg) for seg in self.views]

    def slack_errors(self):
        """What lies outside the maps must still hold SENTINEL, and no map may hold NaN."""
        bad = []
        for name, buf, kind in (("full", self.full, 0), ("pool", self.pool, 1)):
            if buf is None:
                continue
            chk = buf.clone()
            for seg in self.views:
                v = seg[kind]
                lo = v.data_ptr() - buf.data_ptr()
                cv = chk[lo // 4:lo // 4 + v.numel()].view(v.shape)
                if torch.isnan(cv[..., :self.case["Cout"]]).any():
                    bad.append(f"{self.case['id']}: NaN in a {name} map (input slack read into a result)")
                cv[..., :self.case["Cout"]] = SENTINEL
            if not bool((chk == SENTINEL).all()):
                bad.append(f"{self.case['id']}: the {name} buffer was written outside its maps' Cout channels ({int((chk != SENTINEL).sum())} floats)")
        return bad
