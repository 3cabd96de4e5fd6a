"""The C-ABI library loads on a machine without a GPU and exports every symbol include/gen6d_hip.h declares
(no compute calls here); the product path refuses to run without the HIP library or on CPU tensors."""
import os
import re

import pytest
import torch

from gen6d_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "gen6d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(g6d_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    l = lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(l, n), f"{n} declared in gen6d_hip.h but not exported by libgen6d_hip.so"
    assert l.g6d_abi_version() == 12
    # every typed binding corresponds to a declared symbol and vice versa
    assert set(lib.SIGNATURES) | {"g6d_abi_version", "g6d_last_error", "g6d_sizeof_conv_desc", "g6d_sizeof_conv_route", "g6d_sizeof_conv16_route", "g6d_sizeof_wino_route", "g6d_set_knob", "g6d_get_knob",
                                  "g6d_reset_knobs"} == set(names)


def test_knobs_have_product_defaults_and_no_environment_reads():
    """The library's launch policy is set through g6d_set_knob only: defaults as documented, unknown names rejected, reset restores, and
    neither the library sources nor the package read A/B switches from the environment."""
    import glob
    assert lib.get_knob("conv_wino") == 1 and lib.get_knob("wino_min_work") == -1 and lib.get_knob("split_target") == 512
    # (round 5's knobs: the name table and the enum of g6d_common.h must stay in the same order)
    assert lib.get_knob("w43_map") == 2 and lib.get_knob("conv_pm") == 1 and lib.get_knob("gemv_mfma") == 1
    assert lib.get_knob("c16_ablate") == 0 and lib.get_knob("conv16_halo") == 1 and lib.get_knob("conv_narrow") == 1      # (round 6)
    lib.set_knob("conv_wino", 0)
    assert lib.get_knob("conv_wino") == 0
    lib.reset_knobs()
    assert lib.get_knob("conv_wino") == 1
    with pytest.raises(RuntimeError):
        lib.set_knob("no_such_knob", 1)
    for f in glob.glob(os.path.join(ROOT, "gen6d_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "gen6d_amd", "csrc", "*.h")):
        assert "getenv" not in open(f, errors="ignore").read(), f
    for f in glob.glob(os.path.join(ROOT, "gen6d_amd", "**", "*.py"), recursive=True):
        src = open(f).read()
        assert "G6D_" not in src.replace("G6D_ERRORS", "").replace("G6D_E", "").replace("G6D_OK", "") or f.endswith("parallel.py"), f


def test_struct_layout_matches_header():
    # 10 pointer-sized fields, 26 int32 (incl. math_mode), then the weight_wino pointer (include/gen6d_hip.h: struct G6dConv)
    import ctypes as C
    # ... 3 fin pointers, 2 doubles, fin_groups + the round-3 batching fields in_image_mod, mul_group_images + reserved_
    # ... weight_wino16, and (ABI v8) weight_wino43
    assert C.sizeof(lib.G6dConv) == 10 * 8 + 26 * 4 + 8 + 3 * 8 + 2 * 8 + 4 * 4 + 8 + 8 == lib.load().g6d_sizeof_conv_desc()
    assert lib.G6dConv.weight_wino43.offset == C.sizeof(lib.G6dConv) - 8
    assert lib.G6dConv.in_image_mod.offset == 80 + 26 * 4 + 8 + 24 + 16 + 4 and C.sizeof(lib.G6dCorrSeg) == 40
    assert lib.G6dConv.fin_scale.offset == 80 + 26 * 4 + 8 and lib.G6dConv.fin_count.offset == 80 + 26 * 4 + 8 + 24
    assert lib.G6dConv.N.offset == 80 and lib.G6dConv.split_k.offset == 80 + 24 * 4
    assert lib.G6dConv.math_mode.offset == 80 + 25 * 4 and lib.G6dConv.weight_wino.offset == 80 + 26 * 4
    # g6d_conv_route's report: eight int32
    assert C.sizeof(lib.G6dConvRoute) == 8 * 4 == lib.load().g6d_sizeof_conv_route()
    # g6d_conv16_direct_route's report: ten int32 for the launch, six for each of four segments
    assert C.sizeof(lib.G6dConv16Route) == (10 + 4 * 6) * 4 == lib.load().g6d_sizeof_conv16_route()
    # g6d_wino_multi_route's report: six int32, the int64 grid2 on its natural alignment, six int32, three for each of four segments
    assert C.sizeof(lib.G6dWinoRoute) == 6 * 4 + 8 + 6 * 4 + 4 * 3 * 4 == lib.load().g6d_sizeof_wino_route()
    assert lib.G6dWinoRoute.grid2.offset == 24 and lib.G6dWinoRoute.blocks.offset == 32 and lib.G6dWinoRoute.seg.offset == 56


def test_null_descriptor_is_rejected_without_gpu():
    assert lib.load().g6d_conv_igemm(None, None) == -1     # G6D_EINVAL before any HIP call


def test_no_cpu_fallback():
    from gen6d_amd import ops
    x = torch.zeros((1, 1, 4, 4, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.conv(x, torch.zeros((8, 1, 8)), None, torch.zeros((1, 1, 4, 4, 8)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.selector_scan(torch.zeros((4, 8)), torch.zeros((2, 4, 8)))


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libgen6d_hip.so")
    with pytest.raises(RuntimeError, match="no fallback"):
        lib.load()


def test_bench_refuses_to_run_without_gpu():
    """bench.py measures the HIP path only: on a box without a GPU it exits with an error instead of timing a fallback."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stderr + r.stdout)
    assert '"metric"' not in r.stdout


def test_bench_self_launches_one_process_per_gpu():
    """`python bench.py --gpus 2` without a launcher environment re-executes itself under torch.distributed.run
    (the driver's N>1 command form).  Without a GPU both ranks must come up and refuse."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, env=env)
    out = r.stderr + r.stdout
    assert r.returncode != 0
    assert "no CPU fallback" in out, out[-2000:]                 # a rank came up under the launcher and refused
    assert "local_rank: 1" in out or "rank      : 1" in out, out[-2000:]    # ... and there were two of them


def test_integration_doc_covers_every_entry_point():
    """INTEGRATION.md's table names the reference code each exported entry point replaces: no symbol may be missing."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [n for n in _declared() if f"`{n}`" not in doc]
    assert not missing, f"INTEGRATION.md does not mention: {missing}"


def test_graft_entry_build_runs_here():
    """The driver's "does it build" check: __graft_entry__.build() compiles (make is up to date in a built tree), loads the library and
    agrees with it on the ABI version (round 5 bumped the library to v10 while build() still asserted 9: caught by running it)."""
    import __graft_entry__ as g
    g.build()
