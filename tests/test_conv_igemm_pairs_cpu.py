"""ops.conv(pairs=(RangeTable, slot)) over the recording fake library of test_multi_launch_cpu: the descriptor carries math_mode 3 and
the filter exponent, the launch goes to g6d_conv_igemm_ex with the table's range argument, the Winograd filter packs are not passed, a
reduced-precision MATH_MODE keeps precedence, and the launch is booked under the `conv16x3 igemm` prefix with the usual tuple layout.
And the resource facts of the pair-mode instantiations of conv_igemm_kernel from the compiler's metadata: no scratch, no spilled vector
register, at most 256 vector registers (two blocks per CU)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from gen6d_amd import lib, ops
from test_multi_launch_cpu import STREAM, fake  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _operands(scale=1.0):
    g = torch.Generator().manual_seed(1)
    x = torch.rand((2, 1, 9, 7, 16), generator=g)
    w = (torch.rand((64, 9, 16), generator=g) - 0.5) * scale
    out = torch.empty((2, 1, 9, 7, 64))
    return x, w, out


def _conv(x, w, out, **kw):
    return ops.conv(x, w, None, out, ksize=(1, 3, 3), pad=(0, 1, 1), **kw)


def test_pairs_set_the_descriptor_and_the_range(fake):  # noqa: F811
    x, w, out = _operands(scale=1e-2)
    table = ops.RangeTable(torch.device("cpu"))
    table.slot("other")
    u = torch.zeros((16 // 8, 16, 64, 8))
    _conv(x, w, out, pairs=(table, table.slot("here")), w_wino=u)
    (name, (dref, rref, stream)), = fake.calls
    assert name == "g6d_conv_igemm_ex" and stream.value == STREAM
    d, r = dref._obj, rref._obj
    assert d.math_mode == 3
    assert d.w_exp == d.reserved_ == ops.pair_filter_exponent(w) == 14          # |w| <= 5e-3: the exponent rule of conv16_pack caps at 2^14
    assert d.weight_wino is None and d.weight_wino16 is None and d.weight_wino43 is None
    assert isinstance(r, lib.G6dRange16) and (r.exps, r.rec, r.slot_in, r.slot_out) == (table.exps.data_ptr(), table.rec.data_ptr(), -1, 1)
    assert w.__dict__["_g6d_w_exp"] == 14, "the exponent is cached on the weight tensor"
    w.__dict__["_g6d_w_exp"] = 7                                       # ... and read from there
    _conv(x, w, out, pairs=(table, table.slot("here")))
    assert fake.calls[-1][1][0]._obj.w_exp == 7


def test_without_pairs_nothing_changes(fake):  # noqa: F811
    x, w, out = _operands()
    _conv(x, w, out)
    (name, (dref, stream)), = fake.calls
    assert name == "g6d_conv_igemm" and dref._obj.math_mode == 0 and dref._obj.reserved_ == 0


def test_math_mode_keeps_precedence(fake):  # noqa: F811
    x, w, out = _operands()
    table = ops.RangeTable(torch.device("cpu"))
    with ops.math_mode("fp16"):
        _conv(x, w, out, pairs=(table, table.slot("here")))
    (name, (dref, stream)), = fake.calls
    assert name == "g6d_conv_igemm" and dref._obj.math_mode == 2 and dref._obj.reserved_ == 0
    assert "_g6d_w_exp" not in w.__dict__


def test_profile_name_and_tuple(fake, monkeypatch):  # noqa: F811
    x, w, out = _operands()
    table = ops.RangeTable(torch.device("cpu"))
    fake.plan = 5
    monkeypatch.setattr(ops, "PROFILE", [])
    _conv(x, w, out, pairs=(table, table.slot("here")))
    assert fake.log == ["record", "g6d_conv_igemm_ex", "record", "g6d_conv_plan"]
    (fl, e0, e1, label, nbytes, direct), = ops.PROFILE
    assert label.startswith("conv16x3 igemm conv N=2 in=1x9x7x16 out=1x9x7x64 k=1x3x3")
    assert fl == direct == 2.0 * 2 * 9 * 7 * 64 * 9 * 16              # direct-form FLOPs: bench.py counts the x3 of the split16 family itself
    assert nbytes == 4.0 * (x.numel() + w.numel() + out.numel())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_pair_instantiations_have_no_spills(tmp_path):
    out = tmp_path / "igemm.s"
    src = os.path.join(ROOT, "gen6d_amd", "csrc", "conv_igemm.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"),
                        "-o", str(out), src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"\.name:\s+(\S*conv_igemm_kernel\S*)\n(.*?)\.wavefront_size", out.read_text(), re.S)
    pairs = [(n, b) for n, b in kernels if n.endswith("Li3EEEv7G6dConviiiiiijjjiii")]
    assert len(pairs) == 8, [n for n, _ in pairs]                    # 64x64, 128x64: MODE 0 / 1 / 2; 128x128: MODE 0 / 1
    for name, body in pairs:
        vs = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
        priv = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
        assert vs == 0 and priv == 0, f"{name}: {vs} spilled vector registers, {priv} B of scratch"
        assert vg <= 256, f"{name}: {vg} vector registers (two blocks per CU need <= 256)"
