"""The argument contract of every launcher (tests/launch_contract.py) on a host WITHOUT a GPU: every baseline and boundary call is
accepted (it reaches the launch and fails there with G6D_ELAUNCH, or answers, for the host-only plan functions), every single-fault
violation is refused with G6D_EINVAL / G6D_ENOSPC and a fresh g6d_last_error() — and the table covers every argument of every entry point
of gen6d_amd.lib.SIGNATURES.

Not marked `gpu` and skipped where a GPU is visible: the calls carry FAKE device pointers, and a violation that a launcher failed to
refuse would launch a kernel on them (tests/test_launch_contract_gpu.py is the accept side on real operands)."""
import time

import pytest
import torch

import launch_contract as LC

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="issues calls on fake device pointers: only where no GPU is visible")

CASES = LC.all_cases()


def test_case_ids_are_unique_and_counted():
    ids = [LC.case_id(c) for c in CASES]
    dup = sorted({i for i in ids if ids.count(i) > 1})
    assert not dup, f"duplicate case ids: {dup}"
    per_class = {k: sum(c.cls == k for c in CASES) for k in ("baseline",) + LC.CLASSES}
    print(f"launch contract: {len(CASES)} cases over {len(LC.ENTRIES)} entry points: {per_class}")
    assert all(per_class[k] > 0 for k in per_class)
    assert all(c.cls == "baseline" or c.cls in LC.CLASSES for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=LC.case_id)
def test_launcher_contract(case):
    ok, text = LC.verdict(case)
    assert ok, text


def test_whole_table_is_host_integer_work():
    """Every case once more in one loop: seconds, not minutes (no launch ever happens; the bound is generous for a loaded build host)."""
    t0 = time.time()
    wrong = [text for ok, text in map(LC.verdict, CASES) if not ok]
    dt = time.time() - t0
    print(f"launch contract: {len(CASES)} calls in {dt:.2f} s")
    assert not wrong, wrong[:5]
    assert dt < 60.0


def test_table_covers_every_argument_of_every_entry_point():
    from gen6d_amd import lib
    bad = LC.completeness_errors()
    assert not bad, "\n".join(bad)
    assert set(LC.EXEMPT) <= {"g6d_marker", "g6d_sizeof_frame_desc", "g6d_sizeof_mesh_desc", "g6d_sizeof_sink_desc"}
    assert set(LC.ENTRIES) | set(LC.EXEMPT) == set(lib.SIGNATURES)
    opt, free = LC.declarations()
    assert all(why for _, _, why in opt + free)


def test_completeness_check_sees_a_gap(monkeypatch):
    """The completeness check is not vacuous: an entry point taken out of the table, an integer argument whose violations are taken
    away, and a fifth exemption are each reported."""
    args, hand = LC.ENTRIES["g6d_vps_norm"]
    monkeypatch.setitem(LC.ENTRIES, "g6d_vps_norm", (args, [c for c in hand if "c_off" not in c[3]]))
    assert any("g6d_vps_norm.c_off" in b for b in LC.completeness_errors())
    monkeypatch.delitem(LC.ENTRIES, "g6d_vps_norm")
    assert any(b.startswith("g6d_vps_norm: neither") for b in LC.completeness_errors())
    monkeypatch.setitem(LC.EXEMPT, "g6d_vps_norm", "no reason")
    assert any("only g6d_marker" in b for b in LC.completeness_errors())


def test_helper_refuses_to_run_beside_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(RuntimeError, match="never where a GPU is visible"):
        LC.issue("g6d_layernorm", {})


def test_fake_operands_are_distinct_aligned_and_close():
    """Distinct, non-null, 16-byte aligned, all within 2^29 floats of the fake base (seg_table.h's tightest reach)."""
    for name, (args, _) in LC.ENTRIES.items():
        ptrs = [a.base for a in args if a.kind in ("P", "O")]
        assert len(set(ptrs)) == len(ptrs), name
        assert all(p and p % 16 == 0 and 0 <= p - LC.FAKE_BASE < 4 * (1 << 29) for p in ptrs), name
