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
        # (the negligible cases need 4 x 4 tiles around a 64 x 64 quad: one more tile row than any other case)
        assert (c.width <= 64 and c.height <= (64 if c.name.startswith("surfel_negligible_") else 48)) or c.name == "list_17_supertiles_in_a_row", c.name
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
    assert "return s3 >= limit && s2 >= limit;" in text and "#define BGS_SURFEL_CULL_LOG2 23\n" in text and C.SURFEL_CULL_LOG2 == 23.0
    assert "constexpr float C1 = 0.84932180028801907f;" in text and "constexpr float C2 = 1.2011224087864498f;" in text
    surfel_tiles = 0
    for case in DESIGNED:
        costs = C.cost_references(case)
        # surfel tiles are countable too: surfel_negligible_in_tile is restated (negligible_figure), every verdict with margin
        assert all(c["countable"] for c in costs), case.name
        surfel_tiles += len(costs) if case.variant == C.SURFEL else 0
        if "rounds" in case.notes:
            for (tx, ty), rounds in case.notes["rounds"].items():
                assert costs[ty * case.tiles_x + tx]["rounds"] == rounds
        if case.notes.get("saturates_after") is not None:
            assert costs[0]["saturated"] and costs[0]["rounds"] == case.notes["saturates_after"] // 64 + 1
    # known answers: one record in a list of one: a group, a round, a staged and a blended record
    assert C.cost_references(C.list_total_cases()[1])[0]["work"] == 3 + 40 + 1 + 8
    # 40 then 40 hits: the second group does not fit, the first is flushed alone, then the second: 2 groups, 2 rounds, 80 records
    assert C.cost_references(C.queue_cases()[4])[0]["work"] == 2 * 3 + 2 * 40 + 80 * (1 + 8)
    print(f"surfel tiles counted: {surfel_tiles}")
    assert surfel_tiles >= 100
    # a surfel's known answer: tile (0, 0) of the negligible case stages two records and blends neither; tile (1, 1) blends both
    neg = C.cost_references(C.surfel_negligible_cases()[0])
    assert neg[0]["work"] == 3 + 40 + 2 and neg[5]["work"] == 3 + 40 + 2 + 2 * 8


def test_a_tilt_of_zero_reproduces_surfel_record_bit_for_bit():
    for args in ((9.1, 7.3, 40, 14, 11), (5.3, 5.1, 4.3, 1.5, 1.2), (16.0, 16.0, 0.3, 0.2, 0.2)):
        a = C.surfel_record(*args, rgb=C.PRIMARIES[1], a=0.3, z=0.25)
        for focal in (64.0, 256.0):
            b = C.tilted_surfel_record(*args, tilt=0.0, spin=0.0, mean_offset=(0.0, 0.0), focal=focal, rgb=C.PRIMARIES[1], a=0.3, z=0.25)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # and a tilt is what the docstring derives: A.z = -sx sy sin tilt cos spin / focal, B.z = -sx sy sin tilt sin spin / focal, C.z = sx sy cos tilt
    r = C.tilted_surfel_record(9.0, 7.0, 40, 14.0, 11.0, 1.2, 2.2, (3.0, -2.0), focal=256.0).astype(np.float64)
    want = (-14 * 11 * np.sin(1.2) * np.cos(2.2) / 256, -14 * 11 * np.sin(1.2) * np.sin(2.2) / 256, 14 * 11 * np.cos(1.2))
    assert np.allclose((r[9], r[12], r[15]), want, rtol=1e-6, atol=0.0) and (r[5], r[6]) == (12.0, 5.0)
    # the surfel's own centre is seen at (s, t) = (0, 0): p.xy = 0 at pc = mean
    p = [r[7 + i] * r[5] + r[10 + i] * r[6] + r[13 + i] for i in range(3)]
    assert abs(p[0]) < 1e-3 and abs(p[1]) < 1e-3 and abs(p[2] - (want[2] + 12.0 * want[0] + 5.0 * want[1])) < 1e-4 * want[2] and p[2] > 0


TILTED = [c for c in DESIGNED if "tilted" in c.notes]
SURFEL_CASES = [c for c in DESIGNED if c.variant == C.SURFEL]


@pytest.mark.parametrize("case", TILTED, ids=lambda c: c.name)
def test_tilted_records_carry_a_depth_gradient(case):
    """|A.z| and |B.z| above 1e-3 in every tilted record (p.z = C.z + A.z pc.x + B.z pc.y varies over the tile by far more than
    rounding), p.z positive over the whole target (no ray grazes), and in the interior case every pair of signs."""
    recs = case.records[case.notes["tilted"]].astype(np.float64)
    assert (np.abs(recs[:, 9]) > 1e-3).all() and (np.abs(recs[:, 12]) > 1e-3).all()
    for r in case.records[case.notes["tilted"]]:
        for ty in range(case.tiles_y):
            for tx in range(case.tiles_x):
                pz = C.surfel_sides(case, r, tx, ty)[0][2]
                assert pz.min() > 0.3 * float(r[15]) and pz.max() - pz.min() > 1e-3 * float(r[15])
    if case.name.startswith("surfel_tilt_interior"):
        assert {(np.sign(a), np.sign(b)) for a, b in recs[:, [9, 12]]} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
        assert len({round(abs(a / b), 2) for a, b in recs[:, [9, 12]]}) == 4
        assert (np.abs(recs[:, 5:7] - recs[:, 0:2]).max(axis=1) >= 1.5).all()   # means a few pixels off the quad centres
    if "aspect" in case.name:
        assert case.viewport in ((48.0, 32.0), (32.0, 48.0)) and (case.width, case.height) == (32, 32)


@pytest.mark.parametrize("case", [c for c in DESIGNED if "crossover_tile" in c.notes], ids=lambda c: c.name)
def test_the_filter_crossover_case_lets_either_side_win(case):
    tx, ty = case.notes["crossover_tile"]
    for r in case.records:
        _, s3, s2 = C.surfel_sides(case, r, tx, ty)
        assert int((s3 < s2).sum()) >= 16 and int((s2 < s3).sum()) >= 16, ((s3 < s2).sum(), (s2 < s3).sum())
        # and where it shows: within 2 px of the quad centre both sides win at a pixel whose alpha is above 1e-2
        vis = np.minimum(s3, s2) < 2.0 * np.log(r[19] / 1e-2)
        assert (vis & (s3 < s2)).any() and (vis & (s2 < s3)).any()

@pytest.mark.parametrize("case", [c for c in DESIGNED if "blended" in c.notes], ids=lambda c: c.name)
def test_negligible_cases_drop_what_they_name_with_margin(case):
    for (tx, ty), want in case.notes["blended"].items():
        _, ranks = case.tile_entries(tx, ty)
        assert len(ranks) == len(want)
        for rank, w in zip(ranks, want):
            r = case.records[int(rank)]
            assert C.keep_figure(case, r, tx, ty) <= C.KEEP_SLACK - C.KEEP_MARGIN
            fig = C.negligible_figure(case, r, tx, ty)
            assert case.overlay or ((fig < -0.25) if w else (fig > 0.25)), (case.name, tx, ty, rank, fig)   # a quarter of a power of two: 1e-2 relative
            assert C.negligible_decided(case, r, tx, ty)
    costs = C.cost_references(case)
    for (tx, ty), want in case.notes["blended"].items():
        assert costs[ty * case.tiles_x + tx]["work"] == 3 + 40 + 2 + 8 * sum(want)
    if "flips" in case.notes:
        low = [c for c in DESIGNED if c.name == "surfel_negligible_cmax_1_s1"][0]
        assert np.array_equal(low.records, case.records) and low.color_max_bits == C.float_bits(1.0) and case.color_max_bits == C.float_bits(6.0)
        flips = [(rank, tx, ty) for (tx, ty), want in sorted(case.notes["blended"].items()) for rank in range(2)
                 if want[rank] and not low.notes["blended"][(tx, ty)][rank]]
        assert sorted(flips) == sorted(case.notes["flips"]) and len(flips) >= 1
        for rank, tx, ty in flips:   # the limit moved by log2(6) and nothing else did
            a, b = C.negligible_terms(low, low.records[rank], tx, ty), C.negligible_terms(case, case.records[rank], tx, ty)
            assert a[:2] == b[:2] and abs(b[2] - a[2] - np.log2(6.0)) < 1e-12 and a[2] == 23.0
    if case.overlay:
        assert all(all(w) for w in case.notes["blended"].values())


def _all_surfel_cases():
    return SURFEL_CASES + C.surfel_grazing_cases() + [C.mixed_case(C.SURFEL, 1, False, 0, 0), C.mixed_tilted_case(1, False, 0)]


def test_what_the_negligible_verdict_drops_is_negligible_at_every_pixel():
    """Soundness of negligible_figure's (the kernel's) interval bound against the exact per-pixel expression: at every pixel
    centre of a tile a record is dropped from, alpha <= a 2^-23 / max(1, cmax). No tolerance: the bound is conservative."""
    dropped = checked = 0
    for case in _all_surfel_cases():
        if case.overlay:
            continue
        cmax = max(1.0, float(np.uint32(case.color_max_bits).view(np.float32)))
        plain = C.Case(case.name, case.width, case.height, case.records, case.lists, case.totals, sup_edge=case.sup_edge, samples=1,
                       variant=C.SURFEL, color_max_bits=case.color_max_bits, viewport=case.viewport)
        for ty in range(case.tiles_y):
            for tx in range(case.tiles_x):
                ys, xs = np.meshgrid(ty * 16 + np.arange(16) + 0.5, tx * 16 + np.arange(16) + 0.5, indexing="ij")
                for rank in case.tile_entries(tx, ty)[1]:
                    r = case.records[int(rank)]
                    checked += 1
                    if C.negligible_figure(case, r, tx, ty) >= 0.0:
                        dropped += 1
                        alpha = C._record_terms(plain, r, tx, ty, xs, ys)[0]
                        assert alpha.max() <= float(r[19]) * 2.0 ** -23 / cmax, (case.name, tx, ty, int(rank), alpha.max())
    print(f"{dropped} of {checked} (record, tile) pairs dropped, every one below 2^-23 / cmax of its opacity at every pixel")
    assert dropped >= 100


GRAZING = C.surfel_grazing_cases()


@pytest.mark.parametrize("case", GRAZING, ids=lambda c: c.name)
def test_grazing_cases_graze_and_the_reference_copes(case):
    img, bound, und, _ = reference(case)
    assert np.isfinite(img).all() and np.isfinite(bound).all() and not und.any()
    covered = np.zeros((16, 16), bool)
    ys, xs = np.meshgrid(np.arange(16) + 0.5, np.arange(16) + 0.5, indexing="ij")
    for r in case.records:
        covered |= C._record_terms(case, r, 0, 0, xs, ys)[2].any(axis=2)
    horizon = bound.max(axis=2) > 2.0 ** -10
    print(f"{case.name}: {int(horizon.sum())} of {int(covered.sum())} covered pixels left to the bit comparison alone")
    assert horizon.sum() <= 0.10 * covered.sum() and not (horizon & ~covered).any()
    for (tx, ty), kinds in case.notes["interior"].items():
        assert [C.interior_figure(case, r, tx, ty) <= 0.9999 - 2e-5 for r in case.records] == kinds
    if "inf_pixel" not in case.notes:
        for r in case.records:   # the horizon crosses the tile: p.z takes both signs, and misses every pixel centre
            pz = C.surfel_sides(case, r, 0, 0)[0][2]
            assert (pz > 0).sum() >= 32 and (pz < 0).sum() >= 32 and np.abs(pz).min() > 0
        assert horizon.any()   # and next to it the bound does grow
        return
    assert not horizon.any()
    for key in ("inf_pixel", "nan_pixel"):
        rank, x, y = case.notes[key]
        r = case.records[rank]
        st = C.stage_surfel32(case, r, 0, 0)
        f = r.astype(np.float64)
        # every operation on the way to the staged words is exact in binary32: the float64 evaluation gives the same numbers
        U0, V0 = f[2] * (0.5 - f[0]), f[3] * (0.5 - f[1])
        bx, by = U0 * f[4] + f[5], V0 * f[4] + f[6]
        inner = [f[7 + i] * bx + f[10 + i] * by + f[13 + i] for i in range(3)]
        assert C._exact32((np.float64(U0), st["U0"]), (np.float64(V0), st["V0"]), (np.float64(bx), st["bx"]), (np.float64(by), st["by"]),
                          (np.float64(f[2] * f[4]), st["ax"]), (np.float64(f[3] * f[4]), st["ay"]), (np.float64(1.0), st["ax"]), (np.float64(1.0), st["ay"]),
                          *[(np.float64(inner[i]), st["inner"][i]) for i in range(3)], (np.float64(f[9]), st["Px"][2]), (np.float64(f[12]), st["Py"][2]))
        p = C.pixel_p32(st, x, y)
        p64, s3, s2 = C.surfel_sides(case, r, 0, 0)
        assert float(p[2]) == 0.0 == p64[2][y, x]
        if key == "inf_pixel":
            assert float(p[0]) != 0.0 and np.isposinf(s3[y, x])
            assert (p64[2][:, x] == 0.0).all() and (np.abs(p64[2][:, [x - 1, x + 1]]) >= 0.5).all()   # the column, and only it
        else:
            assert float(p[0]) == 0.0 == float(p[1]) and p64[0][y, x] == 0.0 == p64[1][y, x] and np.isnan(s3[y, x])
            # the constant C1 scales a power of two: exact as well
            c1 = np.float32(C.STAGE_C1)
            assert C._exact32((np.float64(c1) * inner[0], st["P0"][0]), (np.float64(c1) * inner[1], st["P0"][1]),
                              (np.float64(c1) * f[7], st["Px"][0]), (np.float64(c1) * f[8], st["Px"][1]))
        # the pixel is decided, shows the record, and the reference took the screen-space side
        assert bound[y, x].max() < 1e-5 and s2[y, x] <= 2.0
        without = C.Case("w", 16, 16, np.delete(case.records, rank, axis=0), *C.make_lists([[(0, C.rect(0, 0, 0, 0))]]), samples=case.samples, variant=C.SURFEL)
        assert np.abs(C.render_reference(without)[0][y, x] - img[y, x]).max() > 0.05


TILTED_INSTS = C.tilted_instantiations()


@pytest.mark.parametrize("inst", TILTED_INSTS, ids=str)
def test_random_tilted_cases_stay_under_the_cap_of_undecided_pixels(inst):
    assert len(TILTED_INSTS) == 16 == len([i for i in MIXED if i[0] == C.SURFEL])
    case = C.mixed_tilted_case(*inst)
    assert len(case.records) == 200 and case.totals.max() > 64
    tilts = np.arctan2(np.hypot(case.records[:, 9], case.records[:, 12]) * 512.0, case.records[:, 15])   # tan tilt = |(A.z, B.z)| focal / C.z
    assert tilts.min() >= 0.0 and tilts.max() <= 1.3 + 1e-6 and (tilts > 0.6).mean() > 0.4
    assert np.abs(case.records[:, 5:7] - case.records[:, 0:2]).max() <= 2.0 + 1e-5
    img, bound, und, _ = reference(case)
    assert np.isfinite(img).all() and und.mean() <= 0.005, und.mean()
