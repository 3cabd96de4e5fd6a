"""The guarded-arena helper (tests/guarded.py) catches what it is there to catch — on CPU tensors, with torch fakes in place of kernels —
and the coverage cap: every entry point of gen6d_amd.lib.SIGNATURES is either named by a case of tests/test_guarded_memory_gpu.py or
exempt for one of four reasons."""
import re

import pytest
import torch

from guarded import MIN_GUARD, arena, arena_numel, guard_elems

DTYPES = [torch.float32, torch.float16, torch.bfloat16, torch.uint8]


def _input(dtype=torch.float32, shape=(2, 3, 5, 8), ld=12):
    a = arena(shape, dtype, ld=ld)
    g = torch.Generator().manual_seed(1)
    vals = (torch.rand(shape, generator=g) * 4 + 1)
    a.set(vals.to(dtype))
    return a, vals


@pytest.mark.parametrize("dtype", DTYPES + [torch.float64, torch.int32])
def test_base_congruence_and_layout(dtype):
    """16 mod 256 bytes: 16-byte aligned and not 32-byte aligned; the view has the channels-last strides of row stride ld."""
    for shape, ld in (((2, 3, 5, 8), 12), ((2, 3, 5, 8), None), ((7, 20), 24), ((33,), None)):
        a = arena(shape, dtype, ld=ld)
        p = a.view.data_ptr()
        assert p % 256 == 16 and p % 16 == 0 and p % 32 != 0
        assert tuple(a.view.shape) == shape and a.view.stride(-1) == 1
        if len(shape) >= 2:
            row = ld if ld is not None else shape[-1]
            assert a.view.stride(-2) == row
            assert all(a.view.stride(i) == a.view.stride(i + 1) * shape[i + 1] for i in range(len(shape) - 2))
        g = guard_elems(shape, ld)
        assert a.lead >= g >= MIN_GUARD and a.tail >= g
        assert a.untouched() and a.unwritten() == a.view.numel()
    a = arena((4, 8), dtype, base_mod=(512, 64))
    assert a.view.data_ptr() % 512 == 64


def test_guard_covers_a_plane_two_rows_and_a_vector():
    N, D, H, W, C, ld = 1, 4, 30, 40, 64, 68
    g = guard_elems((N, D, H, W, C), ld)
    assert g == H * W * ld + 2 * W * ld + 64                      # (conv_igemm's pad_a for a 3x3x3 layer: (H + 1) * W * ld + ld)
    assert g >= ((1 * H + 1) * W + 1) * ld
    a = arena((N, D, H, W, C), torch.float32, ld=ld)
    assert a.lead >= g and a.tail >= g
    assert guard_elems((5,), None) == MIN_GUARD


@pytest.mark.parametrize("dtype", DTYPES)
def test_stray_writes_are_seen(dtype):
    """One element written before the operand, after it, and in the ld - C gap of a row in the middle."""
    for where in ("before", "after", "gap", "gap-last-row"):
        a, _ = _input(dtype)
        assert a.untouched()
        flat = a.buf
        C, ld = a.shape[-1], a.ld
        idx = {"before": a.offset - 1, "after": a.offset + a.extent, "gap": a.offset + 7 * ld + C, "gap-last-row": a.offset + a.extent - 1}[where]
        flat[idx] = 3
        assert not a.untouched(), where
        assert a.touched() == [idx - a.offset]
    a, _ = _input(dtype)                                             # far ends of the allocation count as guard too
    a.buf[0] = 1
    assert not a.untouched()
    a, _ = _input(dtype)
    a.buf[-1] = 1
    assert not a.untouched()


def test_nan_of_another_payload_is_a_touched_guard():
    """A 16-bit store into a float32 guard, or a NaN with another payload, leaves a NaN: isnan() would pass it, the bit compare does not."""
    a, _ = _input(torch.float32)
    a.buf.view(torch.int32)[a.offset - 3] = 0x7fc00001
    assert bool(torch.isnan(a.buf[:a.offset]).all()) and not a.untouched()
    for dtype in (torch.float16, torch.bfloat16):
        a, _ = _input(dtype)
        a.buf.view(torch.int16)[a.offset + a.extent + 5] = 0x7e01 if dtype == torch.float16 else 0x7fc1
        assert bool(torch.isnan(a.buf[a.offset + a.extent:]).all()) and not a.untouched()


def test_operand_writes_leave_the_guards_alone():
    a, vals = _input()
    a.view.mul_(2.0)
    assert a.untouched() and torch.equal(a.view, vals * 2)


@pytest.mark.parametrize("where", ["before", "after", "gap"])
def test_read_neutralised_by_a_zero_factor_gives_nan(where):
    """A fake kernel that reads ONE guard element and multiplies it by 0: invisible next to finite memory, NaN next to a NaN guard."""
    a, vals = _input()
    C, ld = a.shape[-1], a.ld
    idx = {"before": a.offset - 1, "after": a.offset + a.extent, "gap": a.offset + 3 * ld + C + 1}[where]

    def fake_kernel(buf):
        return a.view.sum(-1) + 0.0 * buf[idx]                      # the "masked" lane: a product, not a select
    plain = torch.zeros_like(a.buf)
    plain.as_strided(a.shape, a.strides, a.offset).copy_(vals)
    assert bool(torch.isfinite(fake_kernel(plain)).all())           # finite neighbours hide the read
    assert bool(torch.isnan(fake_kernel(a.buf)).all())              # the guard does not
    assert a.untouched()


def test_integer_guards_hold_the_largest_value():
    a = arena((4, 6, 3), torch.uint8, ld=5)
    assert int(a.guards().min()) == 255 and int(a.guards().max()) == 255
    img = torch.full((4, 6, 3), 10, dtype=torch.uint8)
    a.set(img)
    # a bilinear tap that strays one pixel past the row end with weight 1/4 moves the result by (255 - 10) / 4 grey levels
    strayed = 0.75 * a.view[0, 5].float() + 0.25 * a.buf[a.offset + 5 * 5 + 3: a.offset + 5 * 5 + 5].float().mean()
    assert float((strayed - 10.0).abs().max()) > 60
    b = arena((9,), torch.int32)
    assert int(b.guards().min()) == 2 ** 31 - 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_unwritten_output_elements_are_reported(dtype):
    a = arena((2, 4, 6, 8), dtype, ld=16)
    assert a.unwritten() == 2 * 4 * 6 * 8
    a.view.fill_(1.0)
    assert a.unwritten() == 0 and a.untouched()
    a = arena((2, 4, 6, 8), dtype, ld=16)
    a.view.fill_(1.0)
    a.view[1, 3, 5, 7] = float("nan")                                # the fake kernel skipped the last element
    assert a.unwritten() == 1
    assert not bool(torch.isfinite(a.view).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_arenas_cut_from_one_allocation(dtype):
    """Two arenas in one slab (the maps of a multi-map launch): own guards, the same congruence, and a stray write behind the first is
    seen by the first and does not reach the second."""
    item = torch.empty((), dtype=dtype).element_size()
    shapes = [((1, 9, 11, 8), 12), ((2, 5, 6, 8), 16)]
    sizes = [arena_numel(sh, dtype, ld=ld) for sh, ld in shapes]
    starts = [0, (sizes[0] * item + 511) // 512 * 512 // item]
    slab = torch.zeros(starts[1] + sizes[1], dtype=dtype)
    a, b = (arena(sh, dtype, ld=ld, buf=slab[st:st + n]) for (sh, ld), st, n in zip(shapes, starts, sizes))
    for x, (sh, ld) in zip((a, b), shapes):
        assert x.view.data_ptr() % 256 == 16 and x.lead >= guard_elems(sh, ld) and x.tail >= guard_elems(sh, ld)
        assert x.untouched() and x.unwritten() == x.view.numel()
    assert b.view.data_ptr() > a.view.data_ptr() + a.extent * item
    a.buf[a.offset + a.extent + 2] = 1
    assert not a.untouched() and b.untouched()
    with pytest.raises(ValueError):
        arena(shapes[0][0], dtype, ld=12, buf=slab[:sizes[0] - 1])


def test_set_converts_and_checks_shape():
    a = arena((3, 4), torch.float16, ld=8)
    a.set(torch.arange(12, dtype=torch.float64).reshape(3, 4))
    assert a.view.dtype == torch.float16 and float(a.view[2, 3]) == 11.0 and a.untouched()
    with pytest.raises(ValueError):
        arena((3, 8), torch.float32, ld=4)


# ------------------------------------------------------------------------------------------------ the coverage cap
# An entry point of the library is exempt from tests/test_guarded_memory_gpu.py only for one of these reasons.
NO_MAPS = "takes no map pointers"
TABLES = "chain / track kernel: works on tables of a few floats"
FRAMES = "byte-pixel frame kernel: its own tests run unaligned bases and odd pitches"
TWIN = "the _ex form is in the case table"

EXEMPT = {
    "g6d_marker": NO_MAPS, "g6d_zero_bytes": NO_MAPS, "g6d_conv_plan": NO_MAPS, "g6d_conv_route": NO_MAPS, "g6d_conv16_direct_plan": NO_MAPS, "g6d_conv16_direct_route": NO_MAPS, "g6d_wino_multi_route": NO_MAPS, "g6d_corr_fft_plan": NO_MAPS,
    "g6d_stats_finalize": NO_MAPS, "g6d_sizeof_frame_desc": NO_MAPS, "g6d_sizeof_mesh_desc": NO_MAPS, "g6d_sizeof_sink_desc": NO_MAPS,
    "g6d_chain_crop_from_detection": TABLES, "g6d_chain_pose_from_selection": TABLES, "g6d_chain_refine_prepare": TABLES,
    "g6d_chain_refine_update": TABLES, "g6d_track_gather": TABLES, "g6d_track_commit": TABLES, "g6d_track_gate": TABLES,
    "g6d_track_health": TABLES, "g6d_track_verify": TABLES, "g6d_track_corners": TABLES,
    "g6d_frame_ingest": FRAMES, "g6d_frame_ingest_mesh": FRAMES, "g6d_frame_emit": FRAMES, "g6d_frame_emit_source": FRAMES, "g6d_frame_crop": FRAMES,
    "g6d_frame_ingest_area": FRAMES, "g6d_frame_crop_area": FRAMES,
    "g6d_vgg_conv1_pool_nhwc16": TWIN, "g6d_conv16_direct_multi": TWIN, "g6d_corr16_multi": TWIN,
    "g6d_product_split16": TWIN, "g6d_affine_split16": TWIN,
}


def _allowed(name, reason, covered):
    if reason == NO_MAPS:
        return name in ("g6d_marker", "g6d_zero_bytes", "g6d_stats_finalize") or name.endswith(("_plan", "_route")) or name.startswith("g6d_sizeof_") or \
            bool(re.search(r"knob|abi|error", name))
    if reason == TABLES:
        return name.startswith(("g6d_chain_", "g6d_track_"))
    if reason == FRAMES:
        return name.startswith("g6d_frame_")
    if reason == TWIN:
        return not name.endswith("_ex") and name + "_ex" in covered
    return False


def test_every_map_entry_point_has_a_guarded_case():
    from gen6d_amd import lib
    import test_guarded_memory_gpu as G
    covered = G.covered_entries()
    unknown = sorted(covered - set(lib.SIGNATURES))
    assert not unknown, f"cases name entry points the library does not have: {unknown}"
    bad = sorted(n for n, why in EXEMPT.items() if not _allowed(n, why, covered))
    assert not bad, f"exempt for a reason that does not apply: {bad}"
    stale = sorted(n for n in EXEMPT if n not in lib.SIGNATURES)
    assert not stale, f"EXEMPT names entry points the library does not have: {stale}"
    missing = sorted(n for n in lib.SIGNATURES if n not in covered and n not in EXEMPT)
    assert not missing, f"entry points with neither a guarded case nor an exemption: {missing}"
    for c in G.CASES:
        assert c.entries, f"case {c.id} names no entry point"
    assert len({c.id for c in G.CASES}) == len(G.CASES), "case ids must be unique"
