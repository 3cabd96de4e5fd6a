"""g6d_corr16_multi writes the BITS recorded in tests/golden/corr16_bits.json (a SHA-256 and the largest |value| per output map).

The fixture was recorded on an MI355X by tests/golden/make_corr16_bits.py at the commit before corr16_kernel moved to corr16.hip and took
its index arithmetic from corr16_geom.h: its device code changed with that edit (the loader wave's address set-up compiles differently),
its outputs may not.  The kernel has no atomics and a fixed summation order, so equal arithmetic gives equal bits.  The two cases take every
tile width (K = 7: 32 / 16 / 8 / 4, K = 15: 16 / 8) on ragged maps, in bf16, fp16 and pair mode; the tolerance test of the same cases is
tests/test_conv16_gpu.py::test_corr16_multi."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_corr16_bits", os.path.join(GOLDEN, "make_corr16_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def recorded():
    with open(bits.PATH) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", list(bits.MODES))
@pytest.mark.parametrize("case", list(bits.CASES))
def test_bits(recorded, case, mode):
    want = recorded[f"{case}.{mode}"]
    got = bits.run(case, mode)
    assert len(got) == len(want) == len(bits.CASES[case]["sizes"])
    for size, g, w in zip(bits.CASES[case]["sizes"], got, want):
        assert w["amax"] > 0.1
        assert g["amax"] == w["amax"], (case, mode, size, "largest |value|", g["amax"], w["amax"])
        assert g["sha256"] == w["sha256"], (case, mode, size, "the output map's bits differ from the recorded ones")
