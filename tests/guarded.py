"""Guarded arenas: an operand of a kernel inside ONE flat allocation, with guard elements before it, after it and in the `ld - C` gap
of every row, at an address that is 16-byte aligned and no more.  Plain torch; works on CPU tensors as well (tests/test_guarded_cpu.py).

    a = arena((N, H, W, C), torch.float32, ld=C + 4, device="cuda")      # lead / tail default to guard_elems(...)
    a.set(values)                # an input: the operand holds `values`, every guard holds the fill
    kernel(a.view, ...)          # a.view: the channels-last view of `shape`, row stride `ld`, data_ptr() % 256 == 16
    assert a.untouched()         # every guard still holds the fill, bit for bit
    assert a.unwritten() == 0    # an output: no operand element still holds the fill

What the guards are for:
  * a value read from a guard and multiplied by a zero weight, a zero transform coefficient or a zero-padded filter tap is invisible
    while the neighbouring memory is finite; a NaN there turns the product to NaN, and with it the output;
  * a store outside the operand changes a guard (`untouched()` compares the bits through an integer view: `isnan` would accept a NaN of
    another payload, which is what a 16-bit store into the middle of a float32 guard leaves);
  * an output arena is filled with NaN in EVERY element, the operand included: an element the kernel never writes stays NaN.

Fills.  Floating-point arenas are filled with a quiet NaN (`float("nan")` converted to the type: 0x7fc00000 / 0x7e00 / 0x7fc0).  An
integer operand has no NaN; its guards hold the LARGEST value of the type (0xff for the byte pixels of the warp kernels, 0x7fffffff for an
int32 index table): under an interpolation weight that is small but not zero it moves the result the furthest, and as an index it points
as far outside any table as the type allows — both far more visible than a mid-range pattern.

Guard sizes.  `guard_elems(shape, ld)` = max(4096, one depth plane H * W * ld + two rows 2 * W * ld + 64) elements on each side: an
overrun by a vector, a row or a plane (conv_igemm's buffer resource starts `pad_a` elements IN FRONT of the map: csrc/conv_igemm.hip, the
`pad_a` of the launcher) lands inside the same allocation.  These arenas never put an operand at the end of an allocation: nothing here
aims to fault.

Where the documented contract lets a kernel read or write more than `[0, C)` of a row, the operand's last axis is the WHOLE documented row
and the guard starts outside it:
  * fp16 hi / lo pair maps (`[pixel][2][C]`: the hi plane, then the lo plane, ld >= 2 C: include/gen6d_hip.h:312-313; as the input of
    conv_igemm's pair variant 5: include/gen6d_hip.h:113-116): the operand row is the `2 * C` elements of both planes; a channel slice
    of a wider pair map (rows of ld_out, `plane`, c_off: include/gen6d_hip.h:400-402, "nothing else of a row is touched") sits in an
    operand of the wider map's row, whose other channels are checked against the values they held;
  * filter packs with padded rows (the unit-major 16-bit correlation filters: rows of 32 channels + 8 zeros and >= 1 KB of padding behind
    the last unit, include/gen6d_hip.h:200; the corr16 / conv16 packs, the F(2x2) / F(4x4) Winograd filter tensors, the spectra B' of
    g6d_corr_fft_gemm): the pack as the host packer returns it is the operand, flat and dense; the guard starts behind its last element;
  * the spectrum and product buffers of the frequency-domain correlation (`[bins][tiles][2][C]`, include/gen6d_hip.h:905): flat
    operands of exactly the plan's size;
  * the split workspace of conv_igemm and the Winograd launchers belongs to the library (ops.workspace): it is not an operand.
"""
import torch

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
MIN_GUARD = 4096


def guard_elems(shape, ld=None):
    """Guard elements on each side of an operand of `shape` with row stride `ld`: at least 4096, and one plane + two rows + 64."""
    shape = tuple(int(s) for s in shape)
    ld = int(ld) if ld is not None else shape[-1]
    W = shape[-2] if len(shape) >= 2 else 1
    H = shape[-3] if len(shape) >= 3 else 1
    return max(MIN_GUARD, H * W * ld + 2 * W * ld + 64)


def fill_value(dtype):
    """The guard value of `dtype`: NaN for the floating-point types, the largest value for the integer ones (module docstring)."""
    return float("nan") if dtype.is_floating_point else torch.iinfo(dtype).max


def _geometry(shape, dtype, ld, base_mod):
    """-> (shape, ld, element size, channels-last strides of row stride ld, elements from the first row to the end of the last one)."""
    shape = tuple(int(s) for s in shape)
    ld = int(ld) if ld is not None else shape[-1]
    if len(shape) >= 2 and ld < shape[-1]:
        raise ValueError("arena: ld below the row length")
    item = torch.empty((), dtype=dtype).element_size()
    if base_mod[0] % item or base_mod[1] % item:
        raise ValueError("arena: base_mod must be a multiple of the element size")
    strides, s = [1] * len(shape), ld
    for i in range(len(shape) - 2, -1, -1):                         # channels-last, dense but for the row stride
        strides[i] = s
        s *= shape[i]
    extent = s if len(shape) >= 2 else shape[0]                     # rows * ld: the gap behind the last row belongs to the map's footprint
    return shape, ld, item, strides, extent


def arena_numel(shape, dtype, *, ld=None, lead=None, tail=None, base_mod=(256, 16)):
    """Elements of the flat buffer an arena of these arguments needs (what `buf=` must hold at least)."""
    shape, ld, item, _, extent = _geometry(shape, dtype, ld, base_mod)
    g = guard_elems(shape, ld)
    return (g if lead is None else int(lead)) + extent + (g if tail is None else int(tail)) + base_mod[0] // item


class Arena:
    def __init__(self, shape, dtype, ld, lead, tail, base_mod, device, buf=None):
        shape, ld, item, strides, extent = _geometry(shape, dtype, ld, base_mod)
        mod, rem = base_mod
        self.fill = fill_value(dtype)
        need = lead + extent + tail + mod // item
        if buf is None:
            self.buf = torch.full((need,), self.fill, dtype=dtype, device=device)
        else:                                                       # a flat region the caller cut from a larger allocation (see arena())
            if buf.dim() != 1 or buf.dtype != dtype or buf.numel() < need or not buf.is_contiguous():
                raise ValueError(f"arena: buf must be a flat contiguous {dtype} tensor of at least {need} elements")
            self.buf = buf
            self.buf.fill_(self.fill)
        addr = self.buf.data_ptr()
        if addr % item:
            raise RuntimeError("arena: the allocator returned an address that is not a multiple of the element size")
        shift = ((rem - addr - lead * item) % mod) // item         # extra lead elements that bring the operand to rem mod `mod`
        if (addr + (lead + shift) * item) % mod != rem:
            raise RuntimeError(f"arena: cannot reach {rem} mod {mod} from base {addr % mod}")
        self.shape, self.dtype, self.ld, self.strides = shape, dtype, ld, tuple(strides)
        self.lead, self.tail, self.offset, self.extent = lead + shift, self.buf.numel() - (lead + shift) - extent, lead + shift, extent
        self.view = self.buf.as_strided(shape, strides, self.buf.storage_offset() + self.offset)      # (as_strided counts from the storage's start)
        self._ibuf = self.buf.view(_INT_VIEW[item])
        self._fill_bits = torch.full((1,), self.fill, dtype=dtype).view(_INT_VIEW[item])[0].item()
        mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        mask.as_strided(shape, strides, self.offset).fill_(True)
        self._operand = mask

    def set(self, values):
        """The operand takes `values` (any device, converted to the arena's type); the guards keep the fill."""
        self.view.copy_(values.to(self.dtype).reshape(self.shape))
        return self.view

    def guards(self):
        """The guard elements as one flat integer tensor (bit patterns), in address order."""
        return self._ibuf[~self._operand]

    def touched(self):
        """Flat buffer indices (relative to the operand's first element) of the guard elements that no longer hold the fill."""
        bad = (~self._operand) & (self._ibuf != self._fill_bits)
        return (bad.nonzero().flatten() - self.offset).tolist()

    def untouched(self):
        return not bool(((~self._operand) & (self._ibuf != self._fill_bits)).any().item())

    def unwritten(self):
        """Operand elements that still hold the fill bit for bit (an output the kernel did not write completely)."""
        return int((self._operand & (self._ibuf == self._fill_bits)).sum().item())

    def describe(self):
        shape = "x".join(str(n) for n in self.shape)
        ld = f", ld {self.ld}" if len(self.shape) >= 2 else ""
        return f"{shape} {str(self.dtype).replace('torch.', '')}, base {self.view.data_ptr() % 256} mod 256{ld}, guards {self.lead} + {self.tail}"


def arena(shape, dtype, *, ld=None, lead=None, tail=None, fill="nan", base_mod=(256, 16), device="cpu", buf=None):
    """`lead` guard elements (at least: the shift to `base_mod` is added to them), the operand `shape` as a channels-last view of row
    stride `ld`, `tail` guard elements, all holding the fill.  lead / tail default to guard_elems(shape, ld).  fill: reserved — "nan" (NaN,
    or the largest value of an integer type) is the one pattern there is, and any other name is refused.
    buf: a flat tensor of at least arena_numel(...) elements to build the arena in, instead of an allocation of its own.  The multi-map
    launchers address all maps of a launch with 32-bit offsets from the lowest one and refuse maps more than 2^29 floats apart
    (csrc/seg_table.h: "allocate them from one buffer"): the arenas of such a launch are cut from one allocation, each with its own guards."""
    if fill != "nan":
        raise ValueError("arena: the guard pattern is NaN (largest value for integer types)")
    g = guard_elems(shape, ld)
    lead = g if lead is None else int(lead)
    tail = g if tail is None else int(tail)
    return Arena(shape, dtype, ld, lead, tail, base_mod, device if buf is None else buf.device, buf)
