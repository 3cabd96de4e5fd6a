"""The hand-over passes of gen6d_amd/csrc/split16.hip (g6d_product_split16, g6d_affine_split16, g6d_affine_split16_to,
g6d_upsample_bilinear_split16, g6d_l2norm_split16) write the BITS recorded in tests/golden/split16_bits.npz, and record the same maximum.

The fixture was recorded on an MI355X by tests/golden/make_split16_bits.py at the commit before these kernels moved out of
conv16_direct.hip and took their store sequence from pair16.h: their device code may change with such an edit, their outputs may not.
Each kernel runs in bf16, fp16 and pair mode, pairs at slot exponents 0 and -2, on the smallest shapes that reach every path (the cases and
what each exercises: make_split16_bits.py).  Every output lies in a buffer filled with a NaN pattern with guards around the map and, for
the slice producers, guard channels at both ends of every row; the whole buffer is compared, so an element written outside the slice fails.

Like the frame-crop equality test this pins a compiler's contraction choices as well as the source: the kernels' fp32 arithmetic (the
bilinear blend, the affine) is written with operators the compiler may fuse, and a toolchain that fuses differently would change last bits
without any fault in the code.  Re-record the fixture then, after checking tests/test_pair_handover_gpu.py (the tolerance test)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_split16_bits", os.path.join(GOLDEN, "make_split16_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def recorded():
    d = dict(np.load(bits.PATH))
    return d, {k[3:]: v for k, v in d.items() if k.startswith("in.")}


@pytest.mark.parametrize("mode,exp", bits.MODES, ids=[bits.mode_tag(m, e) for m, e in bits.MODES])
@pytest.mark.parametrize("kernel", bits.KERNELS)
def test_bits(recorded, kernel, mode, exp):
    gold, inputs = recorded
    prefix = f"{kernel}.{bits.mode_tag(mode, exp)}."
    want = {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}
    got = bits.run(kernel, mode, exp, inputs)
    assert sorted(got) == sorted(want) and len(want) >= (2 if mode == 3 else 1)
    for name, w in want.items():
        if name == "rec":
            assert int(got[name]) == int(w), (prefix + name, "recorded maximum", hex(int(got[name])), hex(int(w)))
            assert int(w) != 0
            continue
        g = got[name]
        inside = bits.written(kernel, mode, name, g.size)
        assert (g[~inside] == np.int16(bits.FILL)).all(), f"{prefix}{name}: wrote outside its slice"
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(w)), \
            f"{prefix}{name}: {int((g != w).sum())} of {int(inside.sum())} elements differ from the recorded bits"
