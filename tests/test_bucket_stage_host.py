"""What the cases of tests/bucket_stage_cases.py hold, shown on the CPU with the host replicas: the device comparison
(tests/test_bucket_stage_gpu.py) is only as good as the inputs it steers to where bucket_sort_kernel and keygen's
bucket_of decide things."""
import numpy as np
import pytest

import bucket_stage_cases as C
from bevy_gaussian_splatting_amd import _native
from bevy_gaussian_splatting_amd.settings import SortMode


def _case(wide, name):
    tag = "wide" if wide else "narrow"
    found = [c for c in C.sort_cases(wide) if c.name == (name if name.startswith("wide") else f"{tag} {name}")]
    assert len(found) == 1, name
    return found[0]


def _only_bucket(case):
    (at,) = np.nonzero(case.counts)[0]
    return int(at), case.pairs


def test_constants_are_the_headers_and_the_bindings():
    assert (C.BUCKET_COUNT, C.BUCKET_CAP, C.BUCKET_FINE, C.BUCKET_FINE_MAX) == (256, 4096, 2048, 1024)
    assert (C.BUCKET_CAP_WIDE, C.BUCKET_FINE_WIDE, C.BUCKET_SUB_MAX, C.BUCKET_SUB_KERNARG) == (16384, 8192, 16, 3)
    assert _native.SELFTEST_BUCKET_GUARD == 64
    header = open(C.os.path.join(C.ROOT, "include", "bgs_diag.h")).read()
    assert "#define BGS_SELFTEST_BUCKET_GUARD 64u" in header


@pytest.mark.parametrize("wide", (0, 1))
def test_fine_of_is_monotone_and_stays_below_nf_at_every_span_edge(wide):
    nf = C.nf_of(wide)
    for span in (0, 1, nf - 1, nf, nf + 1, 2 * nf - 1, 1 << 31, C.M32 - 1, C.M32):
        for kmn in {0, C.M32 - span}:
            keys = sorted({kmn, kmn + span, kmn + span // 2, kmn + min(span, 1), kmn + max(span - 1, 0)})
            f = [C.fine_of(k, kmn, kmn + span, nf) for k in keys]
            assert f == sorted(f) and f[0] == 0 and f[-1] <= nf - 1, (span, f)
            if span >= nf - 1:
                assert f[-1] >= nf - 2, (span, f)   # (the last or the last but one range is in use: the scale is a floor)


@pytest.mark.parametrize("wide", (0, 1))
def test_every_span_case_has_the_span_it_is_named_for_with_pairs_at_both_ends(wide):
    nf = C.nf_of(wide)
    for s in C.SPANS:
        _, pairs = _only_bucket(_case(wide, f"span={s}"))
        keys = pairs[:, 0].astype(np.int64)
        assert keys.max() - keys.min() == C.span_value(s, nf), s
        assert (keys == keys.min()).sum() >= 3 and (keys == keys.max()).sum() >= 3
        if C.span_value(s, nf):
            assert ((keys > keys.min()) & (keys < keys.max())).any()
        assert keys.max() >= 1 << 31


@pytest.mark.parametrize("wide", (0, 1))
def test_the_give_up_boundary_cases_sit_on_it(wide):
    nf, fmax = C.nf_of(wide), C.BUCKET_FINE_MAX
    # 1024 equal pairs: no range over the limit; 1025: one range with 1025
    assert max(C.fine_histogram(_only_bucket(_case(wide, f"{fmax} equal"))[1][:, 0], nf).values()) == fmax
    assert max(C.fine_histogram(_only_bucket(_case(wide, f"{fmax + 1} equal"))[1][:, 0], nf).values()) == fmax + 1
    hist = C.fine_histogram(_only_bucket(_case(wide, f"{fmax} equal + other ranges"))[1][:, 0], nf)
    assert max(hist.values()) == fmax and len(hist) > 100
    # two distinct keys in one range: 1025 pairs there, no key value repeated more than 1024 times — and its twin with 1024
    for total, verdict in ((fmax + 1, 2), (fmax, 0)):
        case = _case(wide, f"two keys in one fine range, {total}")
        keys = _only_bucket(case)[1][:, 0]
        hist = C.fine_histogram(keys, nf)
        assert sorted(hist.values())[-1] == total and sorted(hist.values())[-2] <= 1
        assert np.unique(keys, return_counts=True)[1].max() < fmax and case.verdict == verdict
    groups = np.unique(_only_bucket(_case(wide, "tie groups"))[1][:, 0], return_counts=True)[1]
    assert sorted(groups) == [2, 3, 64, 65, 500, fmax]
    assert sorted(C.fine_histogram(_only_bucket(_case(wide, "tie groups"))[1][:, 0], nf).values()) == sorted(groups)


def test_the_wide_case_fills_both_halves_of_a_word_and_the_first_and_last_range():
    nf = C.BUCKET_FINE_WIDE
    hist = C.fine_histogram(_only_bucket(_case(1, "wide heavy neighbour ranges, first and last range"))[1][:, 0], nf)
    assert hist[3000] == 1000 and hist[3001] == C.BUCKET_FINE_MAX          # ranges 2j and 2j + 1: one packed word
    assert hist[0] == 1 and hist[1] == 800 and hist[nf - 2] == 900 and hist[nf - 1] == 1
    assert max(hist.values()) <= C.BUCKET_FINE_MAX
    full = _case(1, "m=16384")
    assert full.counts.max() == 16384 == C.BUCKET_CAP_WIDE == len(full.pairs)


@pytest.mark.parametrize("wide", (0, 1))
def test_the_predicted_verdicts_are_the_ones_the_cases_are_built_for(wide):
    cap = C.cap_of(wide)
    names = [c.name for c in C.sort_cases(wide)]
    assert len(set(names)) == len(names)
    seen = set()
    for case in C.sort_cases(wide):
        want = C.expected_sort(wide, 0, case.counts, case.pairs)
        assert want["sort_overflow"] == case.verdict, case.name
        assert (case.counts.max() > cap) == (case.verdict == 1), case.name
        assert len(case.pairs) == np.minimum(case.counts.astype(np.int64), cap).sum()
        assert len(case.counts) == C.BUCKET_COUNT * case.sub
        if len(case.pairs) > 1:
            assert case.pairs[:, 1].max() >= 1 << 31 and case.pairs[:, 1].min() < 1 << 31, case.name
            assert len(np.unique(case.pairs[:, 1])) == len(case.pairs)
        if case.verdict == 2:      # the bucket that gives up is the launch's last: one thread orders the two draw_count stores
            assert np.nonzero(case.counts)[0].tolist() == [len(case.counts) - 1]
        if case.verdict == 0 and len(case.pairs):
            out = want["out"]
            assert want["draw_count"] == len(case.pairs) and not (out == C.FILL).all(axis=1).any()
        seen.add(case.verdict)
    assert seen == {0, 1, 2}
    sizes = {int(c.counts.max()) for c in C.sort_cases(wide) if np.count_nonzero(c.counts) == 1}
    assert {1, 2, 63, 64, 65, 255, 256, 257, cap - 1, cap, cap + 1} <= sizes
    subs = {c.sub for c in C.sort_cases(wide)}
    assert subs == {1, 2, 3, 4, 16}
    for sub in (1, 2, 3, 4, 16):
        forms = [c for c in C.sort_cases(wide) if c.sub == sub and "sub=" in c.name]
        assert any(c.counts[0] == 0 and c.counts[1:].any() for c in forms)
        assert any(c.counts[-1] == 0 and c.counts[:-1].any() for c in forms)
        assert any(c.counts[-1] and not c.counts[:-1].any() for c in forms)
        assert any((c.counts == 1).all() for c in forms)


def test_expected_sort_orders_by_key_then_index_as_unsigned_numbers():
    pairs = np.array([[0x80000000, 5], [0x7FFFFFFF, 9], [0x80000000, 0x80000001], [0x80000000, 3], [0, 0xFFFFFFFE]], np.uint32)
    counts = np.zeros(256, np.uint32)
    counts[7] = 5
    want = C.expected_sort(0, C.M32, counts, pairs)
    assert want["out"][:, 1].tolist() == [0xFFFFFFFE, 9, 3, 5, 0x80000001]
    assert want["out"][:, 0].tolist() == [C.M32, 0x80000000, 0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF]


def test_every_sub_reaches_the_lookup_form_and_table_source_it_is_meant_to():
    assert [C.lookup_form(s) for s in C.SUBS] == [("256", "kernel arguments"), ("512", "kernel arguments"), ("1024", "kernel arguments"),
                                                  ("1024", "device table"), ("general", "device table"), ("general", "device table")]
    assert C.tile_shape(6000, 0) == C.tile_shape(6000, 1) == (256, 8)
    assert C.tile_shape(C.BIG, 0) == (256, 16) and C.tile_shape(C.BIG, 1) == (1024, 4)
    assert C.BIG % 4096 == 1 and C.BIG // 4096 >= 1      # full tiles and a ragged last one


def test_bucket_of_counts_the_splitters_at_or_below_the_key():
    tab = np.array([5, 5, 9, C.M32, C.M32], np.uint32)       # (six buckets)
    assert C.bucket_of([0, 4, 5, 6, 9, 10, C.M32 - 1, C.M32], tab).tolist() == [0, 0, 2, 2, 3, 3, 3, 5]
    assert C.bucket_of([0, C.M32], np.zeros(255, np.uint32)).tolist() == [255, 255]
    assert C.bucket_of([0, C.M32 - 1, C.M32], np.full(255, C.M32, np.uint32)).tolist() == [0, 0, 255]


@pytest.mark.parametrize("n", C.SIZES)
def test_placement_scenes_hold_what_they_are_for(oracle, n):
    for mode in C.MODES:
        cloud, view, settings = C.placement_scene(n, mode)
        entries, kk, drawable, d = C.keygen_space(oracle, cloud, view, settings)
        assert len(kk) == n
        if mode == "rayon":
            assert settings.sort_mode == SortMode.Rayon and d == n
            assert kk[n // 2] == C.M32                        # the splat at the camera: key ~0 in keygen's space
            assert entries["key"][-1] == 0 and (n == 1 or (kk != C.M32).any())
        else:
            assert 0 < d < n or (n == 1 and d == 1)           # the camera culls part of the cloud
            assert (entries["key"][d:] == C.M32).all() and (np.diff(entries["index"][d:].astype(np.int64)) > 0).all()
        kd = np.sort(kk[drawable])
        _, kk2, dr2, _ = C.keygen_space(oracle, cloud, C.placement_view(other=True), settings)
        kd_other = np.sort(kk2[dr2])
        for sub in C.SUBS:
            nb = 256 * sub
            for kind in C.TABLES:
                tab = C.table(kind, sub, kd, kd_other)
                assert tab.dtype == np.uint32 and tab.shape == (nb - 1,) and (np.diff(tab.astype(np.int64)) >= 0).all(), (kind, sub)
                counts = C.expected_counts(kk, drawable, tab)
                assert counts.sum() == d and len(counts) == nb
                if kind == "zeros":
                    assert counts[-1] == d
                if kind == "ones":
                    assert counts[0] == d - int((kk[drawable] == C.M32).sum())
                if kind == "quantiles" and d:
                    assert np.isin(tab, kd).all()
                if kind == "below occurring keys" and d:
                    assert np.isin(tab + np.uint32(1), kd).all() or (tab == 0).any()
        # the one-bucket tables overflow a narrow region with 6000 drawable splats, and nothing else does
        over = C.expected_counts(kk, drawable, np.zeros(255, np.uint32)).max() > C.BUCKET_CAP
        assert over == (n == 6000 and mode == "rayon")
        assert C.expected_counts(kk, drawable, C.table("quantiles", 1, kd, kd_other)).max() <= C.BUCKET_CAP
