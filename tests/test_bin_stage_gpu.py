"""The binning stage on the device against an exact host reference, list by list (tests/bin_stage_cases.py): integer work,
every comparison is equality.

  bin_kernel<4> / <16> alone, on synthetic rectangles (bgs_selftest_bin): every list entry for entry, the totals, and that
  nothing is written at or past a list's capacity — for both workgroup shapes, every grid size the cases name and list
  capacities below the longest list.
  The lists a real frame built (bgs_debug_frame_lists), at pipeline depth 1 (bin_kernel<16>) and 2 (<4>) and at forced
  supertile levels; and, through the other pipeline, the tile-sorted instances (project_emit_kernel's expansion + the two
  tile-id passes) and the 65 536 tile ranges (tile_ranges_kernel). The reference's input is the host twin's rectangles."""
import copy
import ctypes

import numpy as np
import pytest

import bin_stage_cases as B
import helpers as H
import vertex_stage_cases as VC
from bevy_gaussian_splatting_amd import GaussianSplattingPlugin, _native

pytestmark = pytest.mark.gpu

LEVEL_FLAGS = {0: 0x10000, 1: 0x8000, 3: 0x800000}      # BGS_DEBUG_LEVEL_0 / _1 / _3 (include/bgs_diag.h)
SMALL_LISTS = 0x100000                                   # BGS_DEBUG_SMALL_LISTS


def _entry(e):
    return f"(rank {int(e[0])}, rect 0x{int(e[1]):08x})"


def _assert_lists(what, dev_lists, ref_lists):
    """Entry for entry; prints supertile, position, device entry and reference entry of the first mismatches."""
    msgs = []
    for s, (dev, ref) in enumerate(zip(dev_lists, ref_lists)):
        if dev.shape == ref.shape and np.array_equal(dev, ref):
            continue
        m = min(len(dev), len(ref))
        bad = np.nonzero((dev[:m] != ref[:m]).any(axis=1))[0]
        for pos in bad[:8]:
            msgs.append(f"{what} supertile {s} position {pos}: device {_entry(dev[pos])} reference {_entry(ref[pos])}")
        if len(dev) != len(ref):
            msgs.append(f"{what} supertile {s}: device list holds {len(dev)} entries, the reference {len(ref)}")
    if msgs:
        print(f"{len(msgs)} mismatches ({what}):")
        for line in msgs[:40]:
            print("  " + line)
    assert not msgs, f"{len(msgs)} mismatches ({what}); first: {msgs[0]}"
    assert len(dev_lists) == len(ref_lists)


# ---- bin_kernel alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.BIN_CASE_NAMES)
def test_bin_kernel_builds_the_reference_lists(plugin, name):
    case = B.bin_case(name)
    tx, ty, edge = case.grid
    d = B.built(case)
    lists, lengths = d["lists"], d["lengths"]
    print(f"{name}: {case.num_st} supertiles, {case.num_blocks} blocks, longest list {lengths.max()}, {lengths.sum()} entries")
    for cap in B.capacities(case):
        want = B.expected_buffer(lists, cap)
        for wide in (0, 1):
            for blocks in (case.num_blocks,) + case.blocks:
                what = f"{name} cap {cap} wide {wide} blocks {blocks}"
                out = plugin.selftest_bin(d["rects"], tx, ty, edge, cap, wide, blocks)
                assert out["error"] == 0, f"{what}: Control::error {out['error']}"
                totals = out["totals"].astype(np.int64)
                bad = np.nonzero(totals[:case.num_st] != lengths)[0]
                assert not len(bad), (f"{what}: coarse_total of supertile {bad[0]} is {totals[bad[0]]}, the reference list holds "
                                      f"{lengths[bad[0]]} ({len(bad)} totals differ)")
                assert not totals[case.num_st:].any(), f"{what}: a total past the grid's supertiles"
                kept = np.minimum(lengths, cap)
                _assert_lists(what, [out["lists"][s, :kept[s]] for s in range(case.num_st)], [l[:cap] for l in lists])
                # the whole buffer at once: the slots in [min(total, cap), cap) of every list still hold the fill
                if not np.array_equal(out["lists"], want):
                    s, pos, _ = (int(v[0]) for v in np.nonzero(out["lists"] != want))
                    raise AssertionError(f"{what}: supertile {s} slot {pos} (list of {lengths[s]}, capacity {cap}) holds "
                                         f"{_entry(out['lists'][s, pos])}, not the fill")
                assert (out["guard"] == B.FILL).all(), f"{what}: the guard behind the last list was written: {out['guard'][(out['guard'] != B.FILL).any(axis=1)][:4]}"
    # (every run equals the one expected buffer: the results are identical for wide 0 / 1 and every `blocks`)


# ---- the lists of real frames ----------------------------------------------------------------------------------------
def _upload(plugin, case, d):
    cloud = d["cloud"]
    return plugin.upload(cloud.to_f16()) if case.fmt == "f16" else plugin.upload(cloud, precompute_covariance_3d=(case.fmt == "cov3d"))


def _frame(plugin, case, d, binning, depth, flags=0):
    """One synchronous frame at the pipeline depth; the lists hook's output, the records hook's (depth 1) and the stats."""
    assert d["kept"] is None
    plugin.set_pipeline_depth(depth)
    plugin.set_async(False)
    plugin.set_binning(binning)
    plugin.set_debug_flags(flags)
    handle = _upload(plugin, case, d)
    try:
        plugin.render(handle, d["view"], copy.copy(d["settings"]), download=False)
        out = plugin.debug_frame_lists()
        out["records"] = plugin.debug_frame_records() if depth == 1 else None
        out["stats"] = plugin.stats()
    finally:
        plugin.set_debug_flags(0)
        plugin.set_binning("scan")
        plugin.set_pipeline_depth(1)
        handle.free()
    return out


def _check_scan(what, dev, d, tiles, level, depth):
    rects = d["rects"]
    edge, ran_at = B.supertile_edge(tiles[0], tiles[1], level)
    assert dev["binning"] == "scan" and dev["draw_count"] == len(rects), what
    assert (dev["sup_edge"], dev["level"]) == (edge, ran_at), f"{what}: sup_edge / level {dev['sup_edge']} / {dev['level']}, expected {edge} / {ran_at}"
    assert (dev["sup_x"], dev["sup_y"]) == B.grid_supertiles(tiles[0], tiles[1], edge), what
    assert dev["wide_bin"] == (1 if depth == 1 else 0), f"{what}: wide_bin {dev['wide_bin']} at depth {depth}"
    if dev["records"] is not None:
        assert np.array_equal(dev["records"]["rects"], rects), f"{what}: the device's tile rectangles are not the twin's"
    ref = B.reference_lists(rects, tiles[0], tiles[1], edge)
    lengths = np.array([len(l) for l in ref], np.int64)
    assert np.array_equal(dev["totals"].astype(np.int64), lengths), f"{what}: coarse_total {dev['totals'].tolist()} reference {lengths.tolist()}"
    assert dev["coarse_cap"] >= lengths.max(), f"{what}: the frame ended with lists of {dev['coarse_cap']}, the longest needs {lengths.max()}"
    _assert_lists(what, dev["lists"], ref)
    return lengths


def _check_sort(what, dev, d):
    inst, ranges, present = B.reference_instances(d["rects"])
    assert dev["binning"] == "sort" and dev["draw_count"] == len(d["rects"]), what
    assert dev["instance_count"] == len(inst) == dev["stats"]["instance_count"], f"{what}: instance_count {dev['instance_count']}, reference {len(inst)}"
    bad = np.nonzero((dev["instances"] != inst).any(axis=1))[0]
    for i in bad[:20]:
        print(f"{what} instance {i}: device (tile 0x{int(dev['instances'][i, 0]):04x}, rank {int(dev['instances'][i, 1])}) "
              f"reference (tile 0x{int(inst[i, 0]):04x}, rank {int(inst[i, 1])})")
    assert not len(bad), f"{what}: {len(bad)} of {len(inst)} sorted instances differ, the first at {bad[0]}"
    got = dev["ranges"].astype(np.int64)
    bad = np.nonzero(present & (got != ranges).any(axis=1))[0]
    assert not len(bad), f"{what}: range of tile 0x{bad[0]:04x} is {got[bad[0]].tolist()}, reference {ranges[bad[0]].tolist()} ({len(bad)} differ)"
    bad = np.nonzero(~present & (got[:, 0] != got[:, 1]))[0]
    assert not len(bad), f"{what}: tile 0x{bad[0]:04x} holds no instance but its range is {got[bad[0]].tolist()} ({len(bad)} such)"


@pytest.mark.parametrize("depth", (1, 2))
@pytest.mark.parametrize("name", B.FRAME_CASE_NAMES)
def test_a_frames_lists_equal_the_reference(plugin, name, depth):
    case = B.frame_case(name)
    d = VC.twin_of(case)
    tiles = (-(-int(d["view"].viewport[2]) // 16), -(-int(d["view"].viewport[3]) // 16))
    try:
        for level in (0, 1, 3):
            dev = _frame(plugin, case, d, "scan", depth, LEVEL_FLAGS[level])
            lengths = _check_scan(f"{name} depth {depth} level {level}", dev, d, tiles, level, depth)
            print(f"{name} depth {depth} level {level}: edge {dev['sup_edge']}, {len(lengths)} lists, longest {lengths.max()}, capacity {dev['coarse_cap']}")
        dev = _frame(plugin, case, d, "sort", depth)
        _check_sort(f"{name} depth {depth} sort", dev, d)
        print(f"{name} depth {depth} sort: {dev['instance_count']} instances")
    finally:
        plugin.reset_adaptive_state()    # (the forced levels are not what the session's later frames should start from)


@pytest.mark.parametrize("depth", (1, 2))
def test_lists_that_start_too_small_are_rebuilt_exactly(depth):
    """BGS_DEBUG_SMALL_LISTS: the first run's lists hold 64 entries, the frame is re-run with longer ones."""
    case = B.frame_case("bin_12000_250x130")
    d = VC.twin_of(case)
    with GaussianSplattingPlugin(0) as p:
        dev = _frame(p, case, d, "scan", depth, SMALL_LISTS | LEVEL_FLAGS[1])
        lengths = _check_scan(f"small lists depth {depth}", dev, d, (16, 9), 1, depth)
        counters = p.adaptive_counters()
        print(f"small lists depth {depth}: longest {lengths.max()}, final capacity {dev['coarse_cap']}, stats {dev['stats']['regrow_count']} re-runs, {counters}")
        assert lengths.max() > 64
        assert dev["stats"]["regrow_count"] >= 1 and counters["reruns_lists"] >= 1
        assert dev["coarse_cap"] == dev["stats"]["list_capacity"] >= lengths.max()


def test_a_tile_the_next_frame_leaves_has_an_empty_range():
    """Two BINNING_SORT frames on one context: a cloud over the whole target, then one over its left third. Every tile the
    second frame does not cover has start == end in the second frame's table, whatever the first frame left there."""
    full, left = VC.twin_of(B.STALE_FULL), VC.twin_of(B.STALE_LEFT)
    _, _, covered_full = B.reference_instances(full["rects"])
    _, _, covered_left = B.reference_instances(left["rects"])
    assert (covered_full & ~covered_left).sum() >= 60
    with GaussianSplattingPlugin(0) as p:
        p.set_binning("sort")
        ha, hb = p.upload(full["cloud"]), p.upload(left["cloud"])
        p.render(ha, full["view"], full["settings"], download=False)
        first = p.debug_frame_lists()
        first["stats"] = p.stats()
        _check_sort("full-screen frame", first, full)
        p.render(hb, left["view"], left["settings"], download=False)
        second = p.debug_frame_lists()
        second["stats"] = p.stats()
        _check_sort("left-third frame", second, left)
        got = second["ranges"].astype(np.int64)
        gone = covered_full & ~covered_left
        assert (got[gone, 0] == got[gone, 1]).all()
        ha.free()
        hb.free()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_the_bin_stage_hooks_refuse_what_they_cannot_answer():
    case = VC.by_name("ranks_257")
    d = VC.twin_of(case)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p)
    with GaussianSplattingPlugin(0) as p:
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_lists()
        h = p.upload(d["cloud"])
        p.sort(h, d["view"], d["settings"])
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_lists()
        p.render(h, d["view"], d["settings"])
        out = p.debug_frame_lists()
        assert out["binning"] == "scan" and out["draw_count"] == 257 and len(out["lists"]) == out["sup_x"] * out["sup_y"] == len(out["totals"])
        entries = int(sum(len(l) for l in out["lists"]))
        assert entries > 0
        # too-small host buffers: refused by name, nothing written
        info = _native.BgsFrameListsInfo()
        totals, ents, ranges = np.zeros(256, np.uint32), np.zeros(2 * entries, np.uint32), np.zeros(131072, np.uint32)
        rc = p._lib.bgs_debug_frame_lists(p._ctx, ptr(totals), len(out["lists"]) - 1, ptr(ents), ents.size, ptr(ranges), ranges.size, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_totals holds" in p._lib.bgs_last_error(p._ctx)
        rc = p._lib.bgs_debug_frame_lists(p._ctx, ptr(totals), 256, ptr(ents), ents.size - 1, ptr(ranges), ranges.size, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_entries holds" in p._lib.bgs_last_error(p._ctx)
        assert not totals.any() and not ents.any() and not ranges.any()
        p.radix_sort_pairs(np.arange(10, dtype=np.uint32))        # rewrites the lane's scratch region
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_lists()
        p.set_binning("sort")
        p.render(h, d["view"], d["settings"])
        out = p.debug_frame_lists()
        assert out["binning"] == "sort" and out["instance_count"] == H.twin_instances(d["twin"]) > 0
        ents = np.zeros(2 * out["instance_count"], np.uint32)
        rc = p._lib.bgs_debug_frame_lists(p._ctx, None, 0, ptr(ents), ents.size, ptr(ranges), ranges.size - 1, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_ranges holds" in p._lib.bgs_last_error(p._ctx)
        rc = p._lib.bgs_debug_frame_lists(p._ctx, None, 0, ptr(ents), ents.size - 1, ptr(ranges), ranges.size, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_entries holds" in p._lib.bgs_last_error(p._ctx)
        assert not ents.any() and not ranges.any()
        p.sort(h, d["view"], d["settings"])
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_lists()
        p.set_binning("scan")
        p.render(h, d["view"], d["settings"])
        p.set_pipeline_depth(2)                                   # any depth: the synchronous frame ran on lane 0
        assert p.debug_frame_lists()["draw_count"] == 257
        p.set_async(True)
        for _ in range(2):
            p.render(h, d["view"], d["settings"], download=False)
        with pytest.raises(_native.BgsError, match="frames are in flight|async frame"):
            p.debug_frame_lists()
        p.synchronize()
        with pytest.raises(_native.BgsError, match="async frame"):
            p.debug_frame_lists()
        p.set_async(False)
        # the self-test's arguments: each refusal names the argument
        rects = B.pack([0, 1], [1, 2], [0, 0], [0, 1])
        good = dict(tiles_x=5, tiles_y=3, sup_edge=8, coarse_cap=2, wide=0, blocks=1)
        assert p.selftest_bin(rects, **good)["totals"][0] == 2
        for arg, value, names in (("tiles_x", 0, "tiles_x"), ("tiles_x", 257, "tiles_x"), ("tiles_y", 0, "tiles_y"), ("tiles_y", 257, "tiles_y"),
                                  ("sup_edge", 0, "sup_edge"), ("sup_edge", 33, "sup_edge"), ("wide", 2, "wide"), ("blocks", 0, "blocks"),
                                  ("blocks", 4097, "blocks"), ("coarse_cap", 0, "coarse_cap"), ("coarse_cap", (1 << 25) + 1, "coarse_cap")):
            with pytest.raises(_native.BgsError, match=names + " must"):
                p.selftest_bin(rects, **{**good, arg: value})
        with pytest.raises(_native.BgsError, match="sup_edge 8 gives more than 256 supertiles"):
            p.selftest_bin(rects, **{**good, "tiles_x": 256, "tiles_y": 256})
        with pytest.raises(_native.BgsError, match="sup_edge 4 gives more than 256 supertiles, or more than 32 on an axis"):
            p.selftest_bin(rects, **{**good, "tiles_x": 256, "tiles_y": 4, "sup_edge": 4})
        with pytest.raises(_native.BgsError, match="n must"):
            p.selftest_bin(rects[:0], **good)
        lists, tot, err = np.zeros(2 * (2 + B.GUARD) - 1, np.uint32), np.zeros(256, np.uint32), ctypes.c_uint32(7)
        rc = p._lib.bgs_selftest_bin(p._ctx, ptr(rects), 2, 5, 3, 8, 2, 0, 1, ptr(lists), lists.size, ptr(tot), ctypes.byref(err))
        assert rc == _native.BGS_EINVAL and b"host_lists holds" in p._lib.bgs_last_error(p._ctx)
        assert not lists.any() and not tot.any() and err.value == 7
        h.free()
