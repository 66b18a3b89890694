"""The bucket sort path on the device against exact host references, bucket by bucket (tests/bucket_stage_cases.py):
integer work, every comparison is equality.

  bucket_sort_kernel alone (bgs_selftest_bucket_sort), narrow and wide: the verdict, draw_count, bucket_max, every entry of
  the list and the guard behind it, with key_xor 0 and ~0, on buckets built for the fine-range scale's edges, the give-up
  rule, the packed half-word counts, 64-bit ranking with keys and indices past 2^31, and the offsets over 256 .. 4096 buckets.
  keygen's bucket placement alone (bgs_selftest_keygen_buckets): every count, every bucket's slots as a multiset, every
  slot past the count untouched — for the three code paths, the three tile shapes, both table sources and tables that are
  exact, degenerate, stale or from another camera.
  Both together: the placement's counts and slots, handed to the sort, give oracle.sort's entries."""
import numpy as np
import pytest

import bucket_stage_cases as C
from bevy_gaussian_splatting_amd import _native

pytestmark = pytest.mark.gpu


def _pair(e):
    return f"(key 0x{int(e[0]):08x}, index {int(e[1])})"


def _check_sort(plugin, case, key_xor):
    what = f"{case.name} key_xor 0x{key_xor:08x}"
    want = C.expected_sort(case.wide, key_xor, case.counts, case.pairs)
    out = plugin.selftest_bucket_sort(case.sub, case.wide, key_xor, case.counts, case.pairs)
    print(f"{what}: sort_overflow {out['sort_overflow']} draw_count {out['draw_count']} bucket_max {out['bucket_max']}")
    assert out["sort_overflow"] == want["sort_overflow"], f"{what}: sort_overflow {out['sort_overflow']}, the reference {want['sort_overflow']}"
    assert out["draw_count"] == want["draw_count"], f"{what}: draw_count {out['draw_count']}, the reference {want['draw_count']}"
    assert out["bucket_max"] == want["bucket_max"], f"{what}: bucket_max {out['bucket_max']}, the reference {want['bucket_max']}"
    if not np.array_equal(out["out"], want["out"]):
        bad = np.nonzero((out["out"] != want["out"]).any(axis=1))[0]
        ends = np.cumsum(np.minimum(case.counts.astype(np.int64), C.cap_of(case.wide)))
        lines = []
        for pos in bad[:8]:
            b = int(np.searchsorted(ends, pos, side="right"))
            word = "key" if out["out"][pos, 0] != want["out"][pos, 0] else "index"
            lines.append(f"bucket {b} entry {pos - (ends[b - 1] if b else 0)} (list position {pos}), {word}: device {_pair(out['out'][pos])} "
                         f"reference {_pair(want['out'][pos])}")
        print("\n".join(lines))
        raise AssertionError(f"{what}: {len(bad)} entries differ; first: {lines[0]}")
    assert (out["guard"] == C.FILL).all(), f"{what}: the guard behind the list was written: {out['guard'][(out['guard'] != C.FILL).any(axis=1)][:4]}"


# ---- bucket_sort_kernel alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", (0, 1))
@pytest.mark.parametrize("group", ("one bucket", "sub=1 ", "sub=2 ", "sub=3 ", "sub=4 ", "sub=16 "))
def test_bucket_sort_kernel_orders_every_bucket_as_the_reference(plugin, wide, group):
    cases = [c for c in C.sort_cases(wide) if (group in c.name if group != "one bucket" else "sub=" not in c.name)]
    assert cases
    for case in cases:
        for key_xor in (0, C.M32):
            _check_sort(plugin, case, key_xor)


# ---- keygen's placement alone ----------------------------------------------------------------------------------------
def _tables(oracle, n, mode):
    cloud, view, settings = C.placement_scene(n, mode)
    entries, kk, drawable, d = C.keygen_space(oracle, cloud, view, settings)
    _, kk2, dr2, _ = C.keygen_space(oracle, cloud, C.placement_view(other=True), settings)
    return cloud, view, settings, entries, kk, drawable, d, np.sort(kk[drawable]), np.sort(kk2[dr2])


def _check_run(plugin, handle, scene, what, tab, sub, wide, ordered, alone, blocks=None):
    """`blocks`: the workgroups the launch must have had (default: one per tile; tests/test_grid_cap_gpu.py runs it capped)."""
    cloud, view, settings, entries, kk, drawable, d = scene[:7]
    n = len(kk)
    out = plugin.selftest_keygen_buckets(handle, view, settings, tab, sub, wide, ordered, alone)
    assert out["error"] == 0, f"{what}: Control::error {out['error']}"
    threads, items = C.tile_shape(n, alone)
    assert (out["threads"], out["blocks"]) == (threads, -(-n // (threads * items)) if blocks is None else blocks), \
        f"{what}: the launch ran {out['blocks']} workgroups of {out['threads']} threads, not one per {threads} x {items} tile"
    msgs = C.check_placement(what, out, kk, drawable, tab, C.cap_of(wide))
    assert out["splat_count"] == n, f"{what}: splat_count {out['splat_count']}"
    if ordered:
        # the words keygen publishes with the chain, and the culled tail: oracle.sort's entries behind the drawable ones
        assert out["draw_count"] == d, f"{what}: draw_count {out['draw_count']}, the reference {d}"
        tail = np.stack([entries["key"][d:] ^ np.uint32(C.key_xor_of(settings)), entries["index"][d:]], axis=1)
        if not np.array_equal(out["culled"][:n - d], tail):
            pos = int(np.nonzero((out["culled"][:n - d] != tail).any(axis=1))[0][0])
            msgs.append(f"{what}: culled entry {pos}: device {_pair(out['culled'][pos])} reference {_pair(tail[pos])}")
        if not (out["culled"][n - d:] == C.FILL).all():
            msgs.append(f"{what}: the culled list was written past its {n - d} entries")
    else:
        assert out["draw_count"] == 0 and out["culled"] is None      # (left to bucket_sort_kernel)
    if msgs:
        print("\n".join(msgs))
    assert not msgs, f"{len(msgs)} mismatches; first: {msgs[0]}"
    return out


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("n", C.SIZES)
def test_keygen_places_every_drawable_pair_in_its_bucket(plugin, oracle, n, mode):
    scene = _tables(oracle, n, mode)
    kd, kd_other = scene[7], scene[8]
    handle = plugin.upload(scene[0])
    try:
        runs = 0
        for ordered in (0, 1):
            for t, kind in enumerate(C.TABLES):
                # every table with two of the forms of the look-up: (1, 4), (2, 5), (3, 1), ... over the seven tables both
                # instantiations meet every sub of 1 .. 5; sub = 16 and the wide regions below
                for sub in ((1, 2, 3, 4, 5)[(t + ordered) % 5], (4, 5, 1, 2, 3)[(t + ordered) % 5]):
                    tab = C.table(kind, sub, kd, kd_other)
                    _check_run(plugin, handle, scene, f"n {n} {mode} ordered {ordered} table '{kind}' sub {sub}", tab, sub, 0, ordered, 0)
                    runs += 1
        for ordered, kind, sub, wide in ((0, "quantiles", 16, 0), (1, "runs", 16, 0), (0, "zeros", 1, 1), (1, "quantiles", 4, 1),
                                         (0, "another camera", 2, 1), (1, "ones", 1, 1)):
            tab = C.table(kind, sub, kd, kd_other)
            out = _check_run(plugin, handle, scene, f"n {n} {mode} ordered {ordered} table '{kind}' sub {sub} wide {wide}", tab, sub, wide, ordered, 0)
            if n == 6000 and mode == "rayon" and kind == "zeros":
                assert out["counts"][-1] == 6000            # fits a wide region
        if n == 6000 and mode == "rayon":
            # one-bucket tables overflow a narrow region: the count runs on, 4096 slots are written, the rest is untouched
            for ordered in (0, 1):
                out = _check_run(plugin, handle, scene, f"n 6000 rayon ordered {ordered} overflow", np.zeros(255, np.uint32), 1, 0, ordered, 0)
                assert out["counts"][255] == 6000 and (out["slots"][255] != C.FILL).any(axis=1).all() and (out["slots"][:255] == C.FILL).all()   # (a KEY may be ~0)
        print(f"n {n} {mode}: {runs} runs")
    finally:
        handle.free()


@pytest.fixture(scope="module")
def big(plugin, oracle):
    """The 2^19 + 1 cloud, uploaded once per sort mode for the module."""
    scenes = {mode: _tables(oracle, C.BIG, mode) for mode in C.MODES}
    handles = {mode: plugin.upload(scenes[mode][0]) for mode in C.MODES}
    yield scenes, handles
    for h in handles.values():
        h.free()


@pytest.mark.parametrize("alone", (0, 1))
@pytest.mark.parametrize("mode", C.MODES)
def test_keygen_places_the_long_tiles_as_the_short_ones(plugin, big, mode, alone):
    """4096-splat tiles: 256 x 16, and 1024 x 4 when alone on the chip; 128 full tiles and a last tile of one splat."""
    scenes, handles = big
    scene = scenes[mode]
    kd, kd_other = scene[7], scene[8]
    for ordered in (0, 1):
        for kind, sub in (("quantiles", 1), ("another camera", 3), ("runs", 5), ("one occurring key", 2)):
            tab = C.table(kind, sub, kd, kd_other)
            _check_run(plugin, handles[mode], scene, f"n 2^19+1 {mode} ordered {ordered} alone {alone} table '{kind}' sub {sub}", tab, sub, 0,
                       ordered, alone)


# ---- both together ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mode,sub,wide", ((6000, "radix", 1, 0), (2049, "rayon", 4, 0), (6000, "rayon", 2, 1)))
def test_placement_then_sort_gives_the_oracles_entries(plugin, oracle, n, mode, sub, wide):
    scene = _tables(oracle, n, mode)
    cloud, view, settings, entries, kk, drawable, d, kd, kd_other = scene
    handle = plugin.upload(cloud)
    try:
        tab = C.table("quantiles", sub, kd, kd_other)
        placed = _check_run(plugin, handle, scene, f"n {n} {mode} sub {sub} wide {wide}", tab, sub, wide, 0, 0)
    finally:
        handle.free()
    counts = placed["counts"]
    assert counts.max() <= C.cap_of(wide)
    pairs = np.concatenate([placed["slots"][b, :c] for b, c in enumerate(counts)])
    out = plugin.selftest_bucket_sort(sub, wide, C.key_xor_of(settings), counts, pairs)
    assert (out["sort_overflow"], out["draw_count"], out["bucket_max"]) == (0, d, int(counts.max()))
    want = np.stack([entries["key"][:d], entries["index"][:d]], axis=1)
    if not np.array_equal(out["out"], want):
        pos = int(np.nonzero((out["out"] != want).any(axis=1))[0][0])
        raise AssertionError(f"list position {pos}: device {_pair(out['out'][pos])} oracle {_pair(want[pos])}")
    assert (out["guard"] == C.FILL).all()


# ---- the refusals ----------------------------------------------------------------------------------------------------
def test_the_hooks_refuse_what_the_kernels_cannot_index(plugin, oracle):
    import ctypes
    counts = np.zeros(256, np.uint32)
    counts[3] = 2
    pairs = np.array([[5, 1], [4, 2]], np.uint32)
    assert plugin.selftest_bucket_sort(1, 0, 0, counts, pairs)["out"].tolist() == [[4, 2], [5, 1]]
    for sub in (0, 17):
        with pytest.raises(_native.BgsError, match="sub must"):
            plugin.selftest_bucket_sort(sub, 0, 0, counts, pairs)
    with pytest.raises(_native.BgsError, match="wide must"):
        plugin.selftest_bucket_sort(1, 2, 0, counts, pairs)
    with pytest.raises(_native.BgsError, match="pair_count is 1, host_counts asks for 2"):
        plugin.selftest_bucket_sort(1, 0, 0, counts, pairs[:1])
    over = counts.copy()
    over[3] = C.BUCKET_CAP + 5          # (asks for the capacity's 4096 pairs, not for the count's)
    with pytest.raises(_native.BgsError, match="pair_count is 2, host_counts asks for 4096"):
        plugin.selftest_bucket_sort(1, 0, 0, over, pairs)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p)
    out, info = np.zeros(2 * (2 + _native.SELFTEST_BUCKET_GUARD) - 1, np.uint32), np.zeros(3, np.uint32)
    rc = plugin._lib.bgs_selftest_bucket_sort(plugin._ctx, 1, 0, 0, ptr(counts), ptr(pairs), 2, ptr(out), out.size, ptr(info))
    assert rc == _native.BGS_EINVAL and b"host_out holds" in plugin._lib.bgs_last_error(plugin._ctx)
    assert not out.any() and not info.any()

    scene = _tables(oracle, 2049, "radix")
    cloud, view, settings = scene[:3]
    handle = plugin.upload(cloud)
    try:
        tab = C.table("quantiles", 1, scene[7], scene[8])
        good = dict(sub=1, wide_buckets=0, ordered=0, alone=0)
        for arg, value in (("sub", 0), ("sub", 17), ("wide_buckets", 2), ("ordered", 2), ("alone", 2)):
            with pytest.raises(_native.BgsError, match=arg + " must"):
                plugin.selftest_keygen_buckets(handle, view, settings, tab, **{**good, arg: value})
        bad = tab.copy()
        assert bad[100] > 0
        bad[101] = bad[100] - 1
        with pytest.raises(_native.BgsError, match="host_splitters must ascend, entry 101 is below entry 100"):
            plugin.selftest_keygen_buckets(handle, view, settings, bad, **good)
        v, s = view.to_native(), settings.to_native()
        cnt, slots, info = np.zeros(256, np.uint32), np.zeros(256 * C.BUCKET_CAP * 2 - 1, np.uint32), np.zeros(5, np.uint32)
        rc = plugin._lib.bgs_selftest_keygen_buckets(plugin._ctx, handle._ptr, ctypes.byref(v), ctypes.byref(s), ptr(tab), 1, 0, 0, 0, ptr(cnt),
                                                     ptr(slots), slots.size, None, 0, ptr(info))
        assert rc == _native.BGS_EINVAL and b"host_slots holds" in plugin._lib.bgs_last_error(plugin._ctx)
        slots = np.zeros(256 * C.BUCKET_CAP * 2, np.uint32)
        rc = plugin._lib.bgs_selftest_keygen_buckets(plugin._ctx, handle._ptr, ctypes.byref(v), ctypes.byref(s), ptr(tab), 1, 0, 1, 0, ptr(cnt),
                                                     ptr(slots), slots.size, None, 0, ptr(info))
        assert rc == _native.BGS_EINVAL and b"host_culled must hold" in plugin._lib.bgs_last_error(plugin._ctx)
        assert not cnt.any() and not slots.any() and not info.any()
    finally:
        handle.free()
