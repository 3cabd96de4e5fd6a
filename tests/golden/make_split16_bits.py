"""Records tests/golden/split16_bits.npz: the raw 16-bit outputs (and recorded maxima) of the pair hand-over passes of
gen6d_amd/csrc/split16.hip on small fixed inputs.  Run it ON THE GPU at the commit whose bits are to be pinned:

    python tests/golden/make_split16_bits.py

tests/test_split16_bits_gpu.py imports this module for the cases and replays them against the file.  The inputs are stored beside the
outputs, so the fixture does not depend on a random generator's stream.

Every output lies in a buffer pre-filled with the 16-bit pattern FILL (a NaN in fp16 and in bf16) with GUARD_EL elements before and after the
map and, for the slice producers, GUARD_CH channels at both ends of every row.  The WHOLE buffer is stored and compared: an element outside
the slice that is written differs from the recorded FILL."""
import ctypes as C
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "split16_bits.npz")
FILL = 0x7FFF
GUARD_EL, GUARD_CH = 64, 8
MODES = ((1, None), (2, None), (3, 0), (3, -2))            # (math_mode, slot exponent); bf16, fp16, pairs unscaled and stored as v * 4
KERNELS = ("product", "affine", "affine_to", "upsample", "l2norm")


def mode_tag(mode, exp):
    return f"m{mode}" if exp is None else f"m{mode}e{exp}"


def make_inputs():
    """{name: fp32 array}, CPU.  Values of a few units at most; l2norm rows include one all-zero row (the eps clamp)."""
    g = torch.Generator().manual_seed(20)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(shape, generator=g) * 2 - 1) * scale).numpy()
    d = {
        # product: qn = 2, D = 11 (a run of hypotheses that is no multiple of 8), P = 5, C = 24 (an odd count of 8-channel groups)
        "product.ref": rnd(11, 5, 24), "product.que": rnd(2, 5, 24), "product.scale": rnd(2, 24) * 0.5 + 1.0, "product.shift": rnd(2, 24, scale=0.3),
        # affine: N = 4, H = W = 4, C = 24 inside rows of 40 floats; tables per pair of images
        "affine.x": rnd(4, 4, 4, 40, scale=2.0), "affine.scale": rnd(2, 24) * 0.2 + 0.4, "affine.shift": rnd(2, 24, scale=0.3),
        # upsample: N = 3, C = 24, 4 x 4 (x 2) and 2 x 2 (x 4); tables per image
        "upsample.x4": rnd(3, 4, 4, 24, scale=2.0), "upsample.x2": rnd(3, 2, 2, 24, scale=2.0),
        "upsample.scale": rnd(3, 24) * 0.2 + 0.4, "upsample.shift": rnd(3, 24, scale=0.3),
        "l2norm.x256": rnd(30, 256), "l2norm.x512": rnd(30, 512),
    }
    d["l2norm.x256"][7] = 0.0
    d["l2norm.x512"][7] = 0.0
    return d


class _Buf:
    """pixels rows of ld 16-bit elements (the map's rows begin GUARD_CH elements into a row when guarded) inside GUARD_EL elements."""

    def __init__(self, pixels, ld, row_guard):
        self.t = torch.full((pixels * ld + 2 * GUARD_EL,), FILL, dtype=torch.int16, device="cuda")
        self.ptr = C.c_void_p(self.t.data_ptr() + 2 * (GUARD_EL + (GUARD_CH if row_guard else 0)))
        self.ld = ld


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run(kernel, mode, exp, inputs):
    """The launches of one (kernel, mode) case -> {name: int16 array of a whole output buffer, ..., "rec": uint32 recorded maximum (pairs)}."""
    from gen6d_amd import lib, ops
    l, st = lib.load(), ops._stream()
    x = {k: torch.from_numpy(v).cuda() for k, v in inputs.items() if k.startswith(kernel.split("_")[0] + ".")}
    table = ra = None
    if mode == 3:
        table = ops.RangeTable(torch.device("cuda"))
        table.set_exponents({"map": exp})
        table.clear()
        ra = C.byref(table.arg(-1, table.slot("map")))
    planes = 2 if mode == 3 else 1
    bufs = {}
    if kernel == "product":
        b = bufs["out"] = _Buf(2 * 11 * 5, planes * 24, False)
        lib.check(l.g6d_product_split16_ex(_ptr(x["product.ref"]), _ptr(x["product.que"]), _ptr(x["product.scale"]), _ptr(x["product.shift"]), b.ptr,
                                           2, 11, 5, 24, mode, ra, st), "g6d_product_split16_ex")
    elif kernel in ("affine", "affine_to"):
        xin, sc, sh = x["affine.x"], x["affine.scale"], x["affine.shift"]
        for tables, relu in ((True, 1), (True, 0), (False, 1)):
            s, t, per_n = (sc, sh, 2) if tables else (None, None, 0)
            if kernel == "affine":
                for pool in (0, 1):
                    b = bufs[f"t{int(tables)}r{relu}p{pool}"] = _Buf(4 * (4 >> pool) ** 2, planes * 24, False)
                    lib.check(l.g6d_affine_split16_ex(_ptr(xin), 40, _ptr(s), _ptr(t), per_n, relu, pool, 4, 4, 4, 24, b.ptr, mode, ra, st),
                              "g6d_affine_split16_ex")
            else:                                            # channels [64, 88) of 192-channel rows
                b = bufs[f"t{int(tables)}r{relu}"] = _Buf(4 * 16, planes * 192 + 2 * GUARD_CH, True)
                lib.check(l.g6d_affine_split16_to(_ptr(xin), 40, _ptr(s), _ptr(t), per_n, relu, 0, 4, 4, 4, 24, b.ptr, b.ld, 192, 64, mode, ra, st),
                          "g6d_affine_split16_to")
    elif kernel == "upsample":
        for key, hw, f, tables in (("upsample.x4", 4, 2, True), ("upsample.x2", 2, 4, True), ("upsample.x2", 2, 4, False)):
            s, t, per_n = (x["upsample.scale"], x["upsample.shift"], 1) if tables else (None, None, 0)
            b = bufs[f"f{f}t{int(tables)}"] = _Buf(3 * 64, planes * 192 + 2 * GUARD_CH, True)
            lib.check(l.g6d_upsample_bilinear_split16(_ptr(x[key]), 24, _ptr(s), _ptr(t), per_n, 3, hw, hw, 24, f, b.ptr, b.ld, 192, 128, mode, ra, st),
                      "g6d_upsample_bilinear_split16")
    elif kernel == "l2norm":
        for Cc in (256, 512):
            b = bufs[f"c{Cc}"] = _Buf(30, planes * Cc, False)
            lib.check(l.g6d_l2norm_split16(_ptr(x[f"l2norm.x{Cc}"]), Cc, 30, Cc, b.ptr, mode, ra, st), "g6d_l2norm_split16")
    else:
        raise ValueError(kernel)
    torch.cuda.synchronize()
    out = {k: b.t.cpu().numpy() for k, b in bufs.items()}
    if mode == 3:
        out["rec"] = table.rec.cpu().numpy().view(np.uint32)[table.slot("map")]
    return out


def written(kernel, mode, name, n):
    """Boolean mask over the n elements of output buffer `name`: the elements the case may write."""
    planes = 2 if mode == 3 else 1
    m = np.zeros(n, dtype=bool)
    body = m[GUARD_EL:n - GUARD_EL]
    if kernel in ("affine_to", "upsample"):
        c_off = 64 if kernel == "affine_to" else 128
        rows = body.reshape(-1, planes * 192 + 2 * GUARD_CH)[:, GUARD_CH:-GUARD_CH].reshape(-1, planes, 192)
        rows[:, :, c_off:c_off + 24] = True
    else:
        body[:] = True
    return m


def main():
    inputs = make_inputs()
    d = {"in." + k: v for k, v in inputs.items()}
    for kernel in KERNELS:
        for mode, exp in MODES:
            for name, a in run(kernel, mode, exp, inputs).items():
                key = f"{kernel}.{mode_tag(mode, exp)}.{name}"
                if name != "rec":
                    w = written(kernel, mode, name, a.size)
                    assert (a[~w] == FILL).all(), f"{key}: wrote outside its slice"
                    assert (a[w] != FILL).all(), f"{key}: an element was left unwritten"
                d[key] = a
    np.savez_compressed(PATH, **d)
    print(f"wrote {PATH}: {len(d)} arrays, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    main()
