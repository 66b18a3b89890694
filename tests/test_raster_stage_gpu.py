"""The tile rasterisers alone on the device (bgs_selftest_raster) against the float64 reference of tests/raster_stage_cases.py
and against each other, case by case:

  1. the scan rasteriser's image equals the sort rasteriser's as uint32 views: equality, undecided pixels included;
  2. both are within TWICE the reference's carried bound on every decided pixel (the worst offenders are printed with their
     tile and pixel);
  3. the 64-pixel guard behind each image still holds the 0xFF bytes it was filled with;
  4. on countable tiles (every keep and saturation verdict decided with margin in float64) the cost word equals the integer
     reference: the work count in mode 0, bit 15 in every mode, and the heavy count, list and flags as a set in modes 1, 2;
  5. Control::error is 0;
  6. every refusal of the hook is checked.
A pixel that misses its bound is traced to the first record of its tile's sequence at which it does (the tile's list cut
after k records, device against reference, by bisection) and printed with tile, pixel and that record.
Every mode a case names is run; strip workgroups (a heavy list) and a reversed workgroup order must leave every bit as it is.
The largest error / bound ratio of every case and mode is printed before it is asserted (profiles/raster_stage.md holds the
figures of the run it was written from)."""
import ctypes

import numpy as np
import pytest

import raster_stage_cases as C
from bevy_gaussian_splatting_amd import _native

pytestmark = pytest.mark.gpu

DESIGNED = C.designed_cases()
_REFERENCES = {}


def reference(case):
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = C.render_reference(case)
    return _REFERENCES[case.name]


def run(plugin, case, mode, heavy=None, order=None):
    out = plugin.selftest_raster(case.width, case.height, case.samples, case.variant, case.records, case.lists, case.totals,
                                 case.sup_edge, case.cap, mode=mode, overlay=case.overlay, clear=case.clear,
                                 color_max_bits=case.color_max_bits, viewport=case.viewport, depth=case.depth, heavy_tiles=heavy, order=order)
    assert out["error"] == 0
    assert (out["scan_guard"] == 0xFFFFFFFF).all() and (out["sort_guard"] == 0xFFFFFFFF).all(), "a rasteriser wrote behind its image"
    return out


def assert_same_bits(what, a, b):
    ua, ub = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    if not np.array_equal(ua, ub):
        bad = np.argwhere((ua != ub).any(axis=2))
        for y, x in bad[:8]:
            print(f"  {what}: tile ({x // 16}, {y // 16}) pixel ({x}, {y}): {a[y, x]} vs {b[y, x]}")
        raise AssertionError(f"{what}: {len(bad)} pixels differ; first at {tuple(bad[0][::-1])}")


def first_diverging_record(plugin, case, mode, x, y):
    """The smallest k such that, with only the first k records of the pixel's tile drawn, the device misses twice the bound at
    the pixel: (k - 1, rank) of the record that broke it. Bisection (an error, once made, is taken to stay)."""
    import copy
    tx, ty = x // 16, y // 16
    pos, ranks = case.tile_entries(tx, ty)
    s = (ty // case.sup_edge) * case.sup_x + tx // case.sup_edge

    def misses(k):
        cut = copy.copy(case)
        cut.lists = case.lists.copy()
        cut.lists[s, pos[k:], 1] = C.RECT_EMPTY
        ref, bound, _ = C.render_reference(cut)
        got = run(plugin, cut, mode)["scan"]
        return bool((np.abs(got[y, x].astype(np.float64) - ref[y, x]) > 2.0 * bound[y, x]).any())
    lo, hi = 0, len(ranks)
    if not misses(hi):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if misses(mid) else (mid, hi)
    return hi - 1, int(ranks[hi - 1])


def assert_within_bound(case, what, got, ref, bound, und, plugin=None, mode=0):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(und[..., None], 0.0, err / bound)
    worst = float(ratio.max())
    print(f"{case.name} {what}: largest error / bound {worst:.3f} (largest error {float(np.where(und[..., None], 0.0, err).max()):.3e}, "
          f"{int(und.sum())} undecided pixels)")
    if worst > 2.0:
        order = np.argsort(ratio.max(axis=2), axis=None)[::-1][:8]
        for flat in order:
            y, x = divmod(int(flat), case.width)
            first = None
            if plugin is not None and ratio[y, x].max() > 2.0:
                try:
                    first = first_diverging_record(plugin, case, mode, x, y)
                except Exception as e:   # (a guard or error assertion inside the trace must not mask the miss itself)
                    print(f"  trace failed at pixel ({x}, {y}): {type(e).__name__}: {e}")
            print(f"  tile ({x // 16}, {y // 16}) strip {(y % 16) // 4} pixel ({x}, {y}): device {got[y, x]} reference {ref[y, x]} bound {bound[y, x]} "
                  f"records of the tile {len(case.tile_entries(x // 16, y // 16)[1])}; first diverging record "
                  f"{'not found by bisection' if first is None else f'number {first[0]} of the tile (rank {first[1]})'}")
    assert np.isfinite(got).all()
    assert worst <= 2.0, f"{case.name} {what}: error / bound {worst:.2f} > 2"
    return worst


_COSTS = {}


def assert_cost_words(case, mode, out):
    """The integer reference (raster_stage_cases.cost_reference) on every countable tile of a plain launch."""
    if case.name not in _COSTS:
        _COSTS[case.name] = C.cost_references(case)
    msgs, heavy = [], []
    for t, want in enumerate(_COSTS[case.name]):
        if not want["countable"]:
            continue
        word = int(out["cost"][t])
        tx, ty = t % case.tiles_x, t // case.tiles_x
        if word >> 15 != int(want["saturated"]):
            msgs.append(f"tile ({tx}, {ty}) mode {mode}: bit 15 is {word >> 15}, the reference says saturated = {want['saturated']}")
        if mode == 0 and word & 0x7FFF != want["work"]:
            msgs.append(f"tile ({tx}, {ty}): work {word & 0x7FFF}, the reference counts {want['work']} ({want['rounds']} rounds)")
        if want["rounds"] >= 2:
            heavy.append(t)
    if mode != 0 and all(w["countable"] for w in _COSTS[case.name]):
        got = sorted(out["heavy_list"].tolist())
        if out["heavy_count"] != len(heavy) or got != heavy or np.nonzero(out["heavy_flags"])[0].tolist() != heavy:
            msgs.append(f"mode {mode}: heavy count {out['heavy_count']} list {got} flags {np.nonzero(out['heavy_flags'])[0].tolist()}, the reference names {heavy}")
    counted = sum(w["countable"] for w in _COSTS[case.name])
    print(f"{case.name} mode {mode}: cost words of {counted} of {len(_COSTS[case.name])} {'surfel ' if case.variant == C.SURFEL else ''}tiles counted"
          + ("" if mode == 0 else f", heavy set {'compared' if counted == len(_COSTS[case.name]) else 'not compared (a tile is not countable)'}"))
    for m in msgs[:12]:
        print(f"  {case.name} {m}")
    assert not msgs, f"{case.name}: {len(msgs)} cost / feedback words differ; first: {msgs[0]}"


def check_case(plugin, case):
    ref, bound, und = reference(case)[:3]
    cap = 0.005 if case.random else 0.0
    assert und.mean() <= cap
    first = None
    for mode in case.modes:
        out = run(plugin, case, mode)
        assert_same_bits(f"{case.name} mode {mode}: scan vs sort", out["scan"], out["sort"])
        assert_within_bound(case, f"mode {mode}", out["scan"], ref, bound, und, plugin, mode)
        assert_cost_words(case, mode, out)
        if first is None:
            first = out["scan"]
        else:
            assert_same_bits(f"{case.name}: mode {mode} vs mode {case.modes[0]}", out["scan"], first)
    return first


@pytest.mark.parametrize("case", DESIGNED, ids=lambda c: c.name)
def test_designed_case_matches_the_reference_and_the_other_rasteriser(plugin, case):
    check_case(plugin, case)


@pytest.mark.parametrize("case", [c for c in DESIGNED if c.notes.get("saturates_after", None) is not None], ids=lambda c: c.name)
def test_saturated_tiles_say_so_in_their_cost_word(plugin, case):
    """Bit 15 of the cost word: the tile ended saturated. In every mode; and a mid-round exit may only lower the work count."""
    works = {}
    for mode in case.modes:
        out = run(plugin, case, mode)
        assert out["cost"][0] >> 15 == 1, (mode, hex(int(out["cost"][0])))
        works[mode] = int(out["cost"][0]) & 0x7FFF
    assert works[1] <= works[0] and works[2] <= works[0], works


@pytest.mark.parametrize("case", [c for c in DESIGNED if "group_hits" in c.notes], ids=lambda c: c.name)
def test_unsaturated_tiles_say_so_in_their_cost_word(plugin, case):
    out = run(plugin, case, 0)
    assert out["cost"][0] >> 15 == 0


@pytest.mark.parametrize("case", [c for c in DESIGNED if c.heavy_tiles], ids=lambda c: c.name)
def test_strip_workgroups_and_a_reversed_order_change_no_bit(plugin, case):
    nblocks = (case.tiles_x * case.tiles_y + 3) // 4
    for mode in case.modes:
        plain = run(plugin, case, mode)
        # the feedback names exactly the tiles that needed more than one staging round
        assert plain["heavy_count"] == len(case.heavy_tiles) and sorted(plain["heavy_list"].tolist()) == sorted(case.heavy_tiles)
        assert np.nonzero(plain["heavy_flags"])[0].tolist() == sorted(case.heavy_tiles)
        strips = run(plugin, case, mode, heavy=np.array(case.heavy_tiles, np.uint16))
        assert_same_bits(f"{case.name} mode {mode}: strip workgroups vs regular waves", strips["scan"], plain["scan"])
        assert sorted(strips["heavy_list"].tolist()) == sorted(case.heavy_tiles)   # the strip waves report the tile heavy again
        rev = np.arange(nblocks, dtype=np.uint16)[::-1]
        for heavy in (None, np.array(case.heavy_tiles, np.uint16)):
            out = run(plugin, case, mode, heavy=heavy, order=rev)
            assert_same_bits(f"{case.name} mode {mode}: reversed order", out["scan"], plain["scan"])
            assert np.array_equal(out["cost"], strips["cost"] if heavy is not None else plain["cost"])


@pytest.mark.parametrize("inst", C.instantiations(), ids=str)
def test_every_instantiation_on_the_mixed_case(plugin, inst):
    check_case(plugin, C.mixed_case(*inst))


@pytest.mark.parametrize("inst", C.tilted_instantiations(), ids=str)
def test_every_surfel_instantiation_on_the_mixed_tilted_case(plugin, inst):
    """Random surfels that do not face the camera (tilts up to 1.3, means off the quad centres) through every surfel instantiation."""
    check_case(plugin, C.mixed_tilted_case(*inst))


@pytest.mark.parametrize("case", C.surfel_grazing_cases(), ids=lambda c: c.name)
def test_grazing_rays_leave_finite_pixels_and_the_screen_space_side(plugin, case):
    """p.z through 0 inside the tile: huge, inf and NaN quotients, of which min(s3, s2) must keep the screen-space side. The two
    rasterisers agree bit for bit and write finite pixels; at the named pixels (an inf quotient, a 0 x inf NaN) the device is
    within twice the reference's bound, which drops the NaN with fmin; elsewhere a pixel is left to the bit comparison alone
    only where the reference's own bound exceeds 2^-10, the whole-frame render tolerance."""
    ref, bound, und = reference(case)[:3]
    assert not und.any()
    out = run(plugin, case, 0)
    assert_same_bits(f"{case.name}: scan vs sort", out["scan"], out["sort"])
    assert np.isfinite(out["scan"]).all() and np.isfinite(out["sort"]).all()
    horizon = bound.max(axis=2) > 2.0 ** -10
    for key in ("inf_pixel", "nan_pixel"):
        if key in case.notes:
            _, x, y = case.notes[key]
            err = np.abs(out["scan"][y, x].astype(np.float64) - ref[y, x])
            print(f"{case.name} {key} ({x}, {y}): device {out['scan'][y, x]} reference {ref[y, x]} error / bound {(err / bound[y, x]).max():.3f}")
            assert not horizon[y, x] and (err <= 2.0 * bound[y, x]).all()
    print(f"{case.name}: {int(horizon.sum())} pixels next to a horizon left to the bit comparison")
    assert_within_bound(case, "grazing", out["scan"], ref, bound, horizon, plugin, 0)
    assert_cost_words(case, 0, out)


def test_a_nan_record_inside_a_list_changes_no_bit(plugin):
    with_nan, without = C.nan_case()
    for mode in with_nan.modes:
        a, b = run(plugin, with_nan, mode), run(plugin, without, mode)
        assert_same_bits(f"NaN record, mode {mode}: scan", a["scan"], b["scan"])
        assert_same_bits(f"NaN record, mode {mode}: sort", a["sort"], b["sort"])
        assert_same_bits(f"NaN record, mode {mode}: scan vs sort", a["scan"], a["sort"])
    check_case(plugin, without)


def test_the_hook_refuses_what_it_cannot_bound(plugin):
    case = C.list_total_cases()[3]
    good = dict(width=16, height=16, sample_count=1, variant=0, records=case.records, lists=case.lists, totals=case.totals, sup_edge=32,
                coarse_cap=case.cap)
    assert plugin.selftest_raster(**good)["error"] == 0
    bad_rank = case.lists.copy()
    bad_rank[0, 5, 0] = len(case.records)
    past_total = case.lists.copy()
    totals_short = case.totals.copy()
    totals_short[0] = 10
    past_total[0, 20, 0] = 1 << 30   # behind the list's total: never read, so not refused
    assert plugin.selftest_raster(**{**good, "lists": past_total, "totals": totals_short})["error"] == 0
    refusals = [("width", {"width": 0}), ("width", {"width": 513}), ("height", {"height": 0}), ("height", {"height": 513}),
                ("sample_count", {"sample_count": 3}), ("sample_count", {"sample_count": 16}), ("variant", {"variant": 3}),
                ("overlay", {"overlay": 2}), ("mode", {"mode": 3}), ("sup_edge", {"sup_edge": 0}), ("sup_edge", {"sup_edge": 33}),
                ("coarse_cap", {"coarse_cap": 0}), ("viewport", {"viewport": (0.0, 16.0)}), ("lists", {"lists": bad_rank}),
                # combinations raster_scan_mode never produces
                ("mode", {"mode": 1, "variant": 2, "records": np.zeros((64, 24), np.float32)}), ("mode", {"mode": 2, "variant": 1}),
                ("mode", {"mode": 1, "sample_count": 2}), ("mode", {"mode": 2, "sample_count": 8}), ("mode", {"mode": 1, "overlay": 1}),
                ("heavy_tiles", {"heavy_tiles": np.array([0], np.uint16)}),                       # mode 0 has no strip workgroups
                ("heavy_tiles", {"mode": 1, "heavy_tiles": np.array([1], np.uint16)}),            # tile id >= tiles
                ("heavy_tiles", {"mode": 1, "heavy_tiles": np.array([0, 0], np.uint16)}),         # twice
                ("heavy_count", {"mode": 2, "heavy_tiles": np.zeros(257, np.uint16)}),
                ("order", {"order": np.array([1], np.uint16)})]
    for word, change in refusals:
        with pytest.raises(_native.BgsError) as e:
            plugin.selftest_raster(**{**good, **change})
        assert e.value.status == _native.BGS_EINVAL and word in str(e.value), (word, change.keys(), str(e.value))
    # more supertiles than the 256-wide scan carries: 32 x 32 tiles in supertiles of 1
    with pytest.raises(_native.BgsError) as e:
        plugin.selftest_raster(512, 512, 1, 0, case.records, np.zeros((1024, 1, 2), np.uint32), np.zeros(1024, np.uint32), 1, 1)
    assert e.value.status == _native.BGS_EINVAL and "sup_edge" in str(e.value)
    # an order that repeats a workgroup (48 x 32: 6 tiles, 2 workgroups)
    big = C.strip_workgroup_cases()[0]
    with pytest.raises(_native.BgsError) as e:
        run(plugin, big, 1, order=np.array([0, 0], np.uint16))
    assert "permutation" in str(e.value)
    # NULL pointers and capacities, through the raw entry point
    arg = _native.BgsRasterSelftest()
    arg.width = arg.height = 16
    arg.sample_count, arg.sup_edge, arg.coarse_cap = 1, 32, 1
    arg.viewport_w = arg.viewport_h = 16.0
    img = np.zeros((16 * 16 + 64) * 4, np.float32)
    fptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    cost, heavy, err = np.zeros(1, np.uint16), np.zeros(641, np.uint8), ctypes.c_uint32()
    lists, totals = np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    arg.lists, arg.totals = lists.ctypes.data, totals.ctypes.data
    call = lambda a, cap_f, cap_h: plugin._lib.bgs_selftest_raster(plugin._ctx, ctypes.byref(a), fptr(img), fptr(img.copy()), cap_f,
                                                                  cost.ctypes.data_as(ctypes.c_void_p), heavy.ctypes.data_as(ctypes.c_void_p), cap_h,
                                                                  ctypes.byref(err))
    assert call(arg, img.size - 1, heavy.size) == _native.BGS_EINVAL
    assert call(arg, img.size, heavy.size - 1) == _native.BGS_EINVAL
    assert plugin._lib.bgs_selftest_raster(plugin._ctx, None, fptr(img), fptr(img), img.size, None, None, 0, None) == _native.BGS_EINVAL
    arg.lists = None
    assert call(arg, img.size, heavy.size) == _native.BGS_EINVAL
    arg.lists = lists.ctypes.data
    assert call(arg, img.size, heavy.size) == _native.BGS_OK and (img[:1024].view(np.uint32) != 0xFFFFFFFF).all()   # an empty frame: the clear colour
