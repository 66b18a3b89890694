"""Sparse-splat selection on the device (libbgs_sparse.so): every comparison is BITWISE against the numpy twin
`neighbor_counts_reference`, which counts all pairs (tests/test_sparse_select_host.py ties the twin to the compiled
arithmetic and to geometry). A grid that loses or doubles a pair fails here. The selection reaches the draw only through a
kept chunk, whose frames are compared bitwise too."""
import numpy as np
import pytest

import sparse_select_cases as C
from bevy_gaussian_splatting_amd import (
    CloudSettings, SortMode, SparseGrid, SparseSelect, View, _native_sparse, neighbor_counts_reference, random_gaussians_3d_seeded,
    select_reference)
from bevy_gaussian_splatting_amd.sparse_select import CULLED_KEY, keep_reference, selected_indices
from bevy_gaussian_splatting_amd.plugin import SORT_ENTRY_DTYPE

pytestmark = pytest.mark.gpu

W = HT = 128
GARBAGE = 0xDEADBEEF


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class DevicePoints:
    """float4 points and a counts plane in device memory of the plugin's context (`bgs_device_alloc` / `bgs_upload`); the
    plane is garbage before every count."""

    def __init__(self, plugin, points):
        self.plugin = plugin
        p = C.float4(points)
        self.n = p.shape[0]
        self.points = plugin.device_alloc(max(p.nbytes, 16))
        self.counts = plugin.device_alloc(4 * self.n + 16)
        if p.nbytes:
            plugin.upload_bytes(self.points, p)

    def count(self, grid, radius=C.RADIUS, cap=0, n=None):
        """The whole plane after counting the first n points: one word more than there are points, to see what is written."""
        n = self.n if n is None else n
        self.plugin.upload_bytes(self.counts, np.full(self.n + 1, GARBAGE, np.uint32))
        grid.neighbor_counts(self.plugin.stream_handle(), self.points, n, radius, self.counts, cap=cap)
        self.plugin.synchronize()
        return self.plugin.download(self.counts, np.empty(self.n + 1, np.uint32))

    def free(self):
        self.plugin.device_free(self.points)
        self.plugin.device_free(self.counts)


@pytest.fixture()
def quiet(plugin):
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)
    plugin.set_binning("scan")
    plugin.reset_adaptive_state()
    yield plugin
    plugin.set_async(False)
    plugin.set_pipeline_depth(1)


@pytest.fixture(scope="module")
def grid(plugin):
    with SparseGrid(20_000, plugin.device) as g:
        assert g.capacity == 20_000
        yield g


# ---- 6. device against twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_counts_equal_the_twin(quiet, grid, case, n):
    grid.set_table_bits(0)
    dp = DevicePoints(quiet, C.points(case, 5000))
    try:
        got = dp.count(grid, n=n)
    finally:
        dp.free()
    assert same_bits(got[:n], C.reference(case, n)), (case, n)
    assert (got[n:] == GARBAGE).all()   # nothing is written past n


@pytest.mark.parametrize("cap", [0, 3, 5000])
def test_one_heavy_cell_and_the_cap(quiet, grid, cap):
    grid.set_table_bits(0)
    dp = DevicePoints(quiet, C.coincident())
    try:
        got = dp.count(grid, cap=cap)
    finally:
        dp.free()
    assert same_bits(got[:5000], np.full(5000, cap if cap == 3 else 5000, np.uint32)) and got[5000] == GARBAGE


def test_the_cap_clamps_and_changes_nothing_else(quiet, grid):
    grid.set_table_bits(0)
    want = C.reference("clustered", 5000)
    dp = DevicePoints(quiet, C.points("clustered", 5000))
    try:
        for cap in (1, 3, 50):
            assert same_bits(dp.count(grid, cap=cap)[:5000], np.minimum(want, np.uint32(cap))), cap
    finally:
        dp.free()
    assert want.max() > 50 and want.min() < 3


# ---- 7. collisions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 5000])
def test_the_counts_do_not_depend_on_the_table(quiet, grid, n):
    """2, 4 and 16 slots for thousands of cells: every slot holds many cells, and the 27 cells round a point share
    slots. Each pair is still counted once."""
    want = C.reference("clustered", n)
    dp = DevicePoints(quiet, C.points("clustered", 5000))
    try:
        for bits in (1, 2, 4, 0, 40):   # 0 = automatic; 40 is clamped to what the grid allocated
            grid.set_table_bits(bits)
            assert same_bits(dp.count(grid, n=n)[:n], want), bits
    finally:
        grid.set_table_bits(0)
        dp.free()


# ---- 8. one grid, call after call ------------------------------------------------------------------------------------------------
def test_one_grid_serves_call_after_call(quiet, grid):
    """A large n, then a small one, then another radius, then the first again: nothing of a call is left for the next."""
    grid.set_table_bits(0)
    big = DevicePoints(quiet, C.points("uniform", 5000))
    small = DevicePoints(quiet, C.points("lattice", 65))
    try:
        first = big.count(grid)[:5000]
        assert same_bits(first, C.reference("uniform", 5000))
        assert same_bits(small.count(grid)[:65], C.reference("lattice", 65))
        wide = neighbor_counts_reference(C.points("uniform", 5000), 0.11)
        assert same_bits(big.count(grid, radius=0.11)[:5000], wide) and wide.mean() > 5 * first.mean()
        assert same_bits(big.count(grid)[:5000], first)
    finally:
        big.free()
        small.free()


# ---- 9. the keep kernel -------------------------------------------------------------------------------------------------------------
def _cloud_and_select():
    """20 000 splats uniform in [-20, 20]^3; within 1.5 a splat has 4.4 splats on average, so threshold 3 splits them."""
    return random_gaussians_3d_seeded(20_000, 21), SparseSelect(radius=1.5, neighbor_threshold=3)


@pytest.fixture(scope="module")
def cloud_counts():
    cloud, select = _cloud_and_select()
    counts = neighbor_counts_reference(cloud.position_visibility, select.radius)
    counts.setflags(write=False)
    return counts


@pytest.mark.parametrize("dense", [False, True])
def test_entries_keep_equals_the_reference(quiet, grid, cloud_counts, dense):
    """A sorted chunk that already holds culled keys, and a plane shorter than the cloud: entries with index >= n stay."""
    plugin = quiet
    cloud, select = _cloud_and_select()
    n_plane = 12_000
    counts = np.ascontiguousarray(cloud_counts[:n_plane])
    v, s = View.headless(W, HT), CloudSettings(sort_mode=SortMode.Radix)
    h = plugin.upload(cloud)
    dse = plugin.device_sorted_entries(1, h)
    plane = plugin.device_alloc(4 * n_plane)
    try:
        entries = plugin.sort(h, v, s, into=dse.chunk(0))
        live = entries["key"] != CULLED_KEY
        assert 100 < int((~live).sum()) and int((live & (entries["index"] >= n_plane)).sum()) > 100
        plugin.upload_bytes(plane, counts)
        grid.entries_keep(plugin.stream_handle(), dse.chunk(0).ptr, dse.chunk(0).count, plane, n_plane, select.neighbor_threshold, dense=dense)
        got = dse.download(0)
        want = keep_reference(entries, counts, select.neighbor_threshold, dense=dense)
        assert same_bits(got, want) and same_bits(got["index"], entries["index"])
        # Exactly the live entries that name a point of the plane and fail the predicate change, and both kinds occur. (Some
        # 8 % of these splats are sparse and the camera sees under a tenth of the cloud, so with `dense` only tens of keys
        # change: the sets are compared, not their sizes.)
        changed = got["key"] != entries["key"]
        named = live & (entries["index"] < n_plane)
        sparse = np.zeros(entries.shape[0], bool)
        sparse[named] = counts[entries["index"][named]] < select.neighbor_threshold
        fails = named & (sparse == dense)
        assert np.array_equal(changed, fails) and fails.any() and (named & ~fails).any()
        assert (got["key"][changed] == CULLED_KEY).all()
        assert same_bits(got[~live], entries[~live])
    finally:
        plugin.device_free(plane)
        dse.free()
        h.free()


# ---- 10. end to end through the plugin -------------------------------------------------------------------------------------------
def test_keep_sparse_chunk_and_the_frame_it_draws(quiet, grid, cloud_counts):
    plugin = quiet
    cloud, select = _cloud_and_select()
    n = len(cloud)
    v, s = View.headless(W, HT, msaa_samples=4), CloudSettings(sort_mode=SortMode.Radix)
    h = plugin.upload(cloud)
    dse = plugin.device_sorted_entries(2, h)
    points = plugin.device_alloc(cloud.position_visibility.nbytes)
    plugin.upload_bytes(points, cloud.position_visibility)
    try:
        entries = plugin.sort(h, v, s, into=dse.chunk(0))
        all_frame = plugin.render(h, v, s, entries=dse.chunk(0))
        plugin.keep_sparse(dse.chunk(0), points, grid, select, dense=True)       # the floaters go
        got = dse.download(0)
        want = keep_reference(entries, cloud_counts, select.neighbor_threshold, dense=True)
        assert same_bits(got, want)
        live = entries["key"] != CULLED_KEY
        dropped = (got["key"] == CULLED_KEY) & live
        floaters = live & (cloud_counts[entries["index"]] < select.neighbor_threshold)
        assert np.array_equal(dropped, floaters) and floaters.any() and (live & ~floaters).any()
        frame = plugin.render(h, v, s, entries=dse.chunk(0))
        dse.upload(1, want)
        host_frame = plugin.render(h, v, s, entries=dse.chunk(1))
        assert same_bits(frame, host_frame)
        assert not np.array_equal(frame, all_frame) and np.abs(frame[..., :3]).max() > 0.05
        # the reference's own selection, and its complement on the live entries
        plugin.sort(h, v, s, download=False, into=dse.chunk(1))
        plugin.keep_sparse(dse.chunk(1), points, grid, select)
        got_sparse = dse.download(1)
        assert same_bits(got_sparse, keep_reference(entries, cloud_counts, select.neighbor_threshold))
        assert ((got["key"] == CULLED_KEY) ^ (got_sparse["key"] == CULLED_KEY))[live].all()
        selected = plugin.sparse_select(points, n, grid, select)
        assert same_bits(selected, selected_indices(cloud_counts, select.neighbor_threshold)) and 1000 < len(selected) < n - 1000
        # ... and against select_reference itself on a plane of the first 5000 points (the twin counts them among themselves)
        few = plugin.sparse_select(points, 5000, grid, SparseSelect(radius=2.0, neighbor_threshold=3))
        assert same_bits(few, select_reference(cloud.position_visibility[:5000], 2.0, 3)) and 100 < len(few) < 4900
    finally:
        plugin.device_free(points)
        dse.free()
        h.free()


# ---- errors on a live device ---------------------------------------------------------------------------------------------------
def test_errors_name_the_argument(quiet, grid):
    stream = quiet.stream_handle()
    with pytest.raises(_native_sparse.BgsSparseError, match="n 20001 is above the grid's capacity 20000") as ei:
        grid.neighbor_counts(stream, 16, 20_001, C.RADIUS, 16)
    assert ei.value.status == _native_sparse.BGSS_EINVAL
    with pytest.raises(_native_sparse.BgsSparseError, match="points_device_ptr"):
        grid.neighbor_counts(stream, 8, 4, C.RADIUS, 16)
    with pytest.raises(_native_sparse.BgsSparseError, match="radius 0 must be finite and positive"):
        grid.neighbor_counts(stream, 16, 4, 0.0, 16)
    grid.neighbor_counts(stream, 0, 0, C.RADIUS, 0)          # n == 0: nothing is enqueued, nothing is looked at
    grid.entries_keep(stream, 0, 0, 0, 0, 3)
    with SparseGrid(0, quiet.device) as empty:
        assert empty.capacity == 0
        empty.neighbor_counts(stream, 0, 0, C.RADIUS, 0)
    with pytest.raises(_native_sparse.BgsSparseError, match="no usable HIP device 99"):
        SparseGrid(16, 99)
    assert SORT_ENTRY_DTYPE.itemsize == 8
