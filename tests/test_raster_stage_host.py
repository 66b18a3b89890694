"""What the rasteriser-stage cases (tests/raster_stage_cases.py) hold, shown on the CPU: each case reaches the edge it is named
for (hits per candidate group, which side of a threshold a record falls on, the record at which a tile saturates), designed
cases hold no undecided pixel and random ones at most 0.5 %, and the float64 reference agrees with helpers.emulate_render's
formulas on a cloud both can draw."""
import os
import re

import numpy as np
import pytest

import raster_stage_cases as C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "render_kernels.hip")

_REFERENCES = {}


_STATES = {}


def reference(case):
    """The float64 reference of a case, computed once."""
    if case.name not in _REFERENCES:
        trace, _STATES[case.name] = {}, {}
        _REFERENCES[case.name] = C.render_reference(case, trace, _STATES[case.name]) + (trace,)
    return _REFERENCES[case.name]


DESIGNED = C.designed_cases()


def test_the_constants_the_reference_restates_are_the_kernels():
    text = open(KERNELS).read()
    assert re.search(r"#define BGS_T_EPS_LOG2 13\b", text) and "T_BUDGET = 1.0f / 2048.0f" in text
    assert "fminf(e * s.a2.z, 0.999f)" in text and "BBOX_EDGE_WIDTH = 0.08f" in text
    assert "constexpr uint32_t FLUSH_AT = 32u;" in text and "const bool fits = qn + hits <= 64u;" in text
    assert "0.9999f * OBB_C" in text and "1.0001f * OBB_C" in text
    device = open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "bgs_device.h")).read()
    assert re.search(r"RECT_EMPTY = 0x000000FFu;", device) and C.RECT_EMPTY == 0xFF
    assert "MS_OX0 = -0.125f, MS_OY0 = -0.375f, MS_OX1 = 0.375f, MS_OY1 = -0.125f" in text
    assert C.SAMPLE_OFFSETS[4] == [(-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375)]
    assert "o8[8] = {0.0625f, -0.0625f, 0.3125f, -0.1875f, -0.3125f, -0.4375f, 0.1875f, 0.4375f}" in text
    assert [o[0] for o in C.SAMPLE_OFFSETS[8]] == [0.0625, -0.0625, 0.3125, -0.1875, -0.3125, -0.4375, 0.1875, 0.4375]
    assert C.t_eps_of(C.float_bits(1.0)) == 2.0 ** -13 and C.t_eps_of(C.float_bits(64.0)) == 2.0 ** -17 and C.t_eps_of(0) == 2.0 ** -13


def test_case_names_are_unique_and_targets_small():
    names = [c.name for c in DESIGNED]
    assert len(names) == len(set(names))
    for c in DESIGNED:
        assert (c.width <= 64 and c.height <= 48) or c.name == "list_17_supertiles_in_a_row", c.name
        for s, total in enumerate(c.totals):   # what the hook checks: every rank below a list's own total names a record
            assert (c.lists[s, :min(int(total), c.cap), 0] < len(c.records)).all(), (c.name, s)


@pytest.mark.parametrize("case", DESIGNED, ids=lambda c: c.name)
def test_designed_cases_hold_no_undecided_pixel(case):
    img, bound, und, _ = reference(case)
    assert not und.any(), np.argwhere(und)[:5]
    assert np.isfinite(img).all() and np.isfinite(bound).all()
    # the bound is a rounding bound: far below what a wrong decision moves a pixel by
    assert bound.max() < 1e-3, bound.max()


@pytest.mark.parametrize("case", [c for c in DESIGNED if "group_hits" in c.notes], ids=lambda c: c.name)
def test_list_and_queue_cases_hold_the_hit_counts_they_name(case):
    assert case.group_hits(0, 0) == case.notes["group_hits"]
    # adjacent records of the tile differ in colour and nothing saturates: every record shows
    _, ranks = case.tile_entries(0, 0)
    cols = case.records[ranks][:, 7:10]
    assert (np.abs(np.diff(cols, axis=0)).sum(axis=1) > 0).all()
    trace = reference(case)[3]
    assert trace[(0, 0)] is None


@pytest.mark.parametrize("case", [c for c in DESIGNED if "never_drawn" in c.notes or "never_adds" in c.notes], ids=lambda c: c.name)
def test_what_must_not_be_drawn_would_show(case):
    """Drawing one of the forbidden records moves the reference by far more than its bound."""
    img, bound, _, _ = reference(case)
    ranks = case.notes.get("never_drawn") or case.notes.get("never_adds")
    if "never_drawn" in case.notes:   # not in any tile's sequence
        for ty in range(case.tiles_y):
            for tx in range(case.tiles_x):
                assert not set(case.tile_entries(tx, ty)[1].tolist()) & set(ranks)
    assert np.abs(case.records[ranks][:, 7:10]).min() >= 4.0
    # nothing of their colour (4 and up) shows: the image stays within the other records' colours and the clear colour
    assert img[..., :3].max() <= 1.0 + 1e-6


@pytest.mark.parametrize("case", [c for c in DESIGNED if "saturates_after" in c.notes], ids=lambda c: c.name)
def test_saturation_cases_saturate_where_they_say_with_a_decade_to_spare(case):
    trace = reference(case)[3]
    assert trace[(0, 0)] == case.notes["saturates_after"]
    t_eps = case.t_eps()
    assert t_eps == case.notes.get("t_eps", 2.0 ** -13)
    at = case.notes["saturates_after"]
    if "above_cutoff_after" in case.notes:   # the first round ends with most pixels between t_eps and 4 t_eps, and the second round shows
        st = _STATES[case.name][(0, 0)][case.notes["above_cutoff_after"]]
        assert not st[0] and st[1] and t_eps < st[3] < 3 * t_eps, st
        costs = C.cost_references(case)[0]
        assert costs["rounds"] == 2 and not costs["saturated"] and costs["countable"]
    if at is not None:
        # the mean transmittances the reference reaches: after the record before the saturating one some pixel is still well
        # above the cut-off, after the saturating one every pixel is well below it (T goes 1 -> 1e-3 -> 1e-6: a factor of 8
        # above and of 120 below 2^-13; against cmax = 64's 2^-17 a factor of 130 above and 7.6 below)
        states = _STATES[case.name][(0, 0)]
        above, below = states[at - 1][3] / t_eps, t_eps / states[at][3]
        assert states[at][0] and states[at][1] and not states[at - 1][0] and states[at - 1][1]
        assert (above > 100 and below > 7) if case.name == "saturate_cmax_64" else (above > 6 and below > 100), (above, below)
        _, ranks = case.tile_entries(0, 0)
        assert (case.records[ranks[at - 1:at + 1], 10] == 1.0).all()
        assert at // 64 == {1: 0, 3: 0, 4: 0, 63: 0, 69: 1, 2: 0}[at]   # the staging round it happens in


@pytest.mark.parametrize("case", [c for c in DESIGNED if "interior" in c.notes], ids=lambda c: c.name)
def test_interior_verdicts_fall_on_the_side_they_name_with_margin(case):
    for (tx, ty), kinds in case.notes["interior"].items():
        _, ranks = case.tile_entries(tx, ty)
        assert len(ranks) == len(kinds)
        for rank, interior in zip(ranks, kinds):
            fig = C.interior_figure(case, case.records[int(rank)], tx, ty)
            # the device evaluates the figure in binary32 (a few 1e-7 relative): 2e-5 is margin enough, and the straddling pair
            # sits within 2e-4 of the threshold
            assert (fig <= 0.9999 - 2e-5) if interior else (fig >= 0.9999 + 2e-5), (case.name, rank, fig)
    if "straddle" in case.name:
        figs = [C.interior_figure(case, r, 0, 0) for r in case.records]
        assert 0.9997 < figs[0] < 0.9999 < figs[1] < 1.0001


@pytest.mark.parametrize("case", [c for c in DESIGNED if "strips" in c.notes], ids=lambda c: c.name)
def test_strip_cases_reach_the_strips_they_name(case):
    for rank, want in case.notes["strips"].items():
        assert C.strip_reach(case, case.records[rank], 0, 0) == want, rank
    for rank, tiles in case.notes["misses_tile"].items():
        for tx, ty in tiles:
            assert rank in case.tile_entries(tx, ty)[1]           # the rectangle holds the tile
            assert not any(C.strip_reach(case, case.records[rank], tx, ty))   # the quad does not
    sub = case.records[4]   # smaller than a pixel: it holds one pixel centre and, at 4 samples, passes between all sample positions
    assert sub[2] > 2 and sub[5] > 2
    ys, xs = np.meshgrid(np.arange(16) + 0.5, np.arange(16) + 0.5, indexing="ij")
    cov = C._record_terms(case, sub, 0, 0, xs, ys)[2]
    assert cov.any(axis=2).sum() == (1 if case.samples == 1 else 0)
    if case.samples == 1:
        assert np.argwhere(cov.any(axis=2)).tolist() == [[9, 5]]


@pytest.mark.parametrize("case", [c for c in DESIGNED if "edge_pixels" in c.notes], ids=lambda c: c.name)
def test_exact_edge_cases_put_a_sample_exactly_on_the_limit(case):
    f = case.records[0].astype(np.float64)
    for x, y in case.notes["edge_pixels"]:
        on = []
        for ox, oy in C.SAMPLE_OFFSETS[case.samples]:
            u, v = f[2] * (x + 0.5 + ox - f[0]), f[3] * (y + 0.5 + oy - f[1])
            on.append(max(abs(u), abs(v)) == 1.0)
        assert any(on), (x, y)
    assert not reference(case)[2].any()   # decided all the same: every binary32 operation on the way is exact


@pytest.mark.parametrize("case", [c for c in DESIGNED if "rounds" in c.notes], ids=lambda c: c.name)
def test_heavy_tiles_need_the_rounds_they_name(case):
    for (tx, ty), rounds in case.notes["rounds"].items():
        pos, ranks = case.tile_entries(tx, ty)
        assert -(-len(ranks) // 64) == rounds and reference(case)[3][(tx, ty)] is None
        assert case.heavy_tiles == (ty * case.tiles_x + tx,)


@pytest.mark.parametrize("case", [c for c in DESIGNED if c.name.startswith("depth_")], ids=lambda c: c.name)
def test_depth_cases_hold_every_relation(case):
    d = case.depth[:, :16]
    z = np.array(case.notes["z"], np.float32)
    assert z[0] > d.max() and z[1] < d.min() and d.min() < z[2] < d.max() and (d == z[3]).any()
    if case.samples > 1:
        assert (d.max(axis=2) > d.min(axis=2)).all()   # the depths differ from sample to sample


MIXED = C.instantiations()


@pytest.mark.parametrize("inst", [i for i in MIXED if i[4] == 0], ids=str)
def test_random_cases_hold_at_most_half_a_percent_undecided_pixels(inst):
    case = C.mixed_case(*inst)
    assert 150 <= len(case.records) <= 250 and case.totals.max() > 64
    und = reference(case)[2]
    assert und.mean() <= 0.005, und.mean()


def test_the_instantiation_table_is_what_the_launcher_dispatches():
    insts = C.instantiations()
    assert len(insts) == len(set(insts)) == 3 * 4 * 2 * 2 + 2 * 2 * 2 + 2 * 2   # every plain one, OBB's two exits, AABB3D's one
    text = open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "frame_params.h")).read()
    assert "if (variant == RV_SURFEL || (samples != 1u && samples != 4u) || overlay ||" in text
    assert "return (level >= 2u || variant == RV_AABB3D) ? 1 : 2;" in text


def test_the_reference_agrees_with_the_emulation_of_whole_frames():
    """helpers.emulate_render composites a cloud's records (from the host build of the vertex stage) per pixel in binary32; fed
    the same records and rectangles, the float64 reference must give the same image to 1e-6: it is no private restatement."""
    import helpers
    from bevy_gaussian_splatting_amd import CloudSettings, View, random_gaussians_3d_seeded
    cloud = random_gaussians_3d_seeded(200, seed=3)
    rng = np.random.default_rng(9)
    for aabb, samples, depth, overlay in ((False, 1, False, False), (False, 4, False, False), (True, 1, False, False), (True, 4, False, False),
                                          (False, 2, True, False), (False, 8, False, True), (True, 8, True, False), (True, 2, False, True),
                                          (False, 4, True, True), (True, 1, True, True),
                                          ("surfel", 1, False, False), ("surfel", 4, False, False), ("surfel", 2, True, False),
                                          ("surfel", 8, False, True), ("surfel", 4, True, True)):
        view = View.headless(64, 48)
        view.msaa_samples = samples
        surfel = aabb == "surfel"
        settings = CloudSettings(aabb=bool(aabb), visualize_bounding_box=overlay)
        if surfel:
            from bevy_gaussian_splatting_amd.settings import GaussianMode
            settings.gaussian_mode = GaussianMode.Gaussian2d
        dplane = rng.uniform(0.0, 1.0, (48, 64, samples)).astype(np.float32) if depth else None
        if depth:
            view.depth_host = dplane
        entries = helpers.device_sorted_entries(cloud, view, settings)
        img = helpers.emulate_render(cloud, view, settings, entries)
        draw, full = helpers.twin_draw_list(cloud, view, settings)
        twin = helpers.twin_project(cloud, view, settings, draw, full_entries=full)
        words, rects, _ = helpers.twin_record_words(twin)
        recs = np.ascontiguousarray(words).view(np.float32).reshape(len(rects), -1)
        cmax = np.nanmax(np.abs(recs[rects != C.RECT_EMPTY][:, 16:19] if surfel else recs[rects != C.RECT_EMPTY][:, 7:10]), initial=0.0)
        lists, totals = C.make_lists([[(i, rc) for i, rc in enumerate(rects)]])
        case = C.Case("emulated", 64, 48, recs, lists, totals, samples=samples, variant=C.SURFEL if surfel else (C.AABB3D if aabb else C.OBB), overlay=int(overlay),
                      depth=dplane, clear=tuple(view.clear_color), color_max_bits=C.float_bits(cmax))
        ref, bound, und = C.render_reference(case)
        err = np.abs(ref - img)[~und]
        scale = max(1.0, float(np.abs(ref).max()))
        if not surfel:
            assert und.mean() < 0.02 and err.max() <= 1e-6 * scale, (aabb, samples, depth, overlay, err.max(), und.mean())
        else:
            # The emulation is itself a binary32 evaluation, and for surfels it intersects the pixel's ray with the plane at
            # full viewport coordinates: p.x = pc.x A.x + pc.y B.x + C.x cancels to a few pixels out of terms of viewport size,
            # exactly the cancellation the reference's bound carries for the kernel (same terms, same magnitudes, a comparable
            # count of roundings). 1e-6 is what two evaluations without that cancellation agree to; here they must agree to
            # 1e-6 plus ONE carried bound (not the two the device is allowed), which a wrong formula misses by orders of magnitude
            # (a sign, a swapped cross product or a missing aspect moves pixels by 1e-2 and more).
            excess = (np.abs(ref - img) - bound)[~und]
            print(f"surfel {samples} samples depth {depth} overlay {overlay}: largest |reference - emulation| {err.max():.2e}, "
                  f"largest excess over the bound {excess.max():.2e}, largest error / bound {(np.abs(ref - img) / bound)[~und].max():.3f}")
            assert und.mean() < 0.02 and excess.max() <= 1e-6 * scale, (samples, depth, overlay, err.max(), excess.max(), und.mean())


def test_the_integer_reference_reads_its_weights_from_the_source_and_the_named_cases_are_countable():
    """WORK_* come from csrc/render_kernels.hip, the heavy buffer's layout from csrc/kernels.h; every designed case's tiles are
    countable (no keep or saturation verdict within its margin), so the cost words of all of them are asserted on the device."""
    from bevy_gaussian_splatting_amd import _native
    assert C.work_constants() == {"blended": 8, "staged": 1, "round": 40, "group": 3}
    text = open(KERNELS).read()
    assert "keep = !(fabsf(uc) - eu > 1.0001f * OBB_C) && !(fabsf(vc) - ev > 1.0001f * OBB_C);" in text and C.KEEP_SLACK == 1.0001
    assert "bool heavy = rounds >= 2u;" in text
    kernels_h = open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "kernels.h")).read()
    assert "constexpr uint32_t HEAVY_CAP = 256u, HEAVY_LIST_OFFSET = 128u, HEAVY_FLAGS_OFFSET = HEAVY_LIST_OFFSET + 2u * HEAVY_CAP;" in kernels_h
    assert (_native.HEAVY_CAP, _native.HEAVY_LIST_OFFSET, _native.HEAVY_FLAGS_OFFSET) == (256, 128, 640)
    for case in DESIGNED:
        if case.variant == C.SURFEL:   # (surfel_negligible_in_tile decides what a surfel tile blends: not restated, not countable)
            assert not any(c["countable"] for c in C.cost_references(case))
            continue
        costs = C.cost_references(case)
        assert all(c["countable"] for c in costs), case.name
        if "rounds" in case.notes:
            for (tx, ty), rounds in case.notes["rounds"].items():
                assert costs[ty * case.tiles_x + tx]["rounds"] == rounds
        if case.notes.get("saturates_after") is not None:
            assert costs[0]["saturated"] and costs[0]["rounds"] == case.notes["saturates_after"] // 64 + 1
    # known answers: one record in a list of one: a group, a round, a staged and a blended record
    assert C.cost_references(C.list_total_cases()[1])[0]["work"] == 3 + 40 + 1 + 8
    # 40 then 40 hits: the second group does not fit, the first is flushed alone, then the second: 2 groups, 2 rounds, 80 records
    assert C.cost_references(C.queue_cases()[4])[0]["work"] == 2 * 3 + 2 * 40 + 80 * (1 + 8)
