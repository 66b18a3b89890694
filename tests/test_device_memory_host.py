"""The host side's memory bookkeeping, checked without a GPU through the host shim: the lane's scratch layout
(frame_params.h: scratch_layout) and the owning buffer (device_buffer.h: Buffer, reserve_group) over a memory policy that
counts its calls and can be told to fail one."""
import ctypes

import pytest

from helpers import ScratchLayoutC, scratch_layout, shim

NS = (0, 1, 2048, 2049, 1_000_000, 5_000_000, (1 << 30) - 1)
CAPS = (0, 1 << 22, 1 << 30)

# (n, inst_cap): (bytes, the seven offsets in address order, depth_tiles, inst_tiles, pass_stride) — evaluated once with
# the arithmetic ensure_scratch had before scratch_layout existed (its seven offsets were Lane fields then), not with
# the function under test
LAYOUTS = {
    (0, 0): (616448, 42240, 46336, 46592, 48640, 572928, 573952, 574208, 1, 1, 256),
    (0, 4194304): (2713600, 42240, 46336, 46592, 2145792, 2670080, 2671104, 2671360, 1, 1025, 256),
    (0, 1073741824): (537487360, 42240, 46336, 46592, 536919552, 537443840, 537444864, 537445120, 1, 262145, 256),
    (1, 0): (621568, 42240, 50432, 50688, 52736, 577024, 579072, 579328, 2, 1, 512),
    (1, 4194304): (2718720, 42240, 50432, 50688, 2149888, 2674176, 2676224, 2676480, 2, 1025, 512),
    (1, 1073741824): (537492480, 42240, 50432, 50688, 536923648, 537447936, 537449984, 537450240, 2, 262145, 512),
    (2048, 0): (628736, 42240, 50432, 50688, 52736, 577024, 586240, 586496, 2, 1, 512),
    (2048, 4194304): (2725888, 42240, 50432, 50688, 2149888, 2674176, 2683392, 2683648, 2, 1025, 512),
    (2048, 1073741824): (537499648, 42240, 50432, 50688, 536923648, 537447936, 537457152, 537457408, 2, 262145, 512),
    (2049, 0): (633856, 42240, 54528, 54784, 56832, 581120, 591360, 591616, 3, 1, 768),
    (2049, 4194304): (2731008, 42240, 54528, 54784, 2153984, 2678272, 2688512, 2688768, 3, 1025, 768),
    (2049, 1073741824): (537504768, 42240, 54528, 54784, 536927744, 537452032, 537462272, 537462528, 3, 262145, 768),
    (1000000, 0): (6653184, 42240, 2049280, 2080768, 2082816, 2607104, 6608896, 6610944, 490, 1, 125440),
    (1000000, 4194304): (8750336, 42240, 2049280, 2080768, 4179968, 4704256, 8706048, 8708096, 490, 1025, 125440),
    (1000000, 1073741824): (543524096, 42240, 2049280, 2080768, 538953728, 539478016, 543479808, 543481856, 490, 262145, 125440),
    (5000000, 0): (30785536, 42240, 10048768, 10205184, 10207232, 10731520, 30733312, 30743296, 2443, 1, 625408),
    (5000000, 4194304): (32882688, 42240, 10048768, 10205184, 12304384, 12828672, 32830464, 32840448, 2443, 1025, 625408),
    (5000000, 1073741824): (567656448, 42240, 10048768, 10205184, 547078144, 547602432, 567604224, 567614208, 2443, 262145, 625408),
    (1073741823, 0): (6478718976, 42240, 2147529984, 2181084672, 2181086720, 2181611008, 6476579328, 6478676736, 524289, 1, 134217984),
    (1073741823, 4194304): (6480816128, 42240, 2147529984, 2181084672, 2183183872, 2183708160, 6478676480, 6480773888, 524289, 1025, 134217984),
    (1073741823, 1073741824): (7015589888, 42240, 2147529984, 2181084672, 2717957632, 2718481920, 7013450240, 7015547648, 524289, 262145, 134217984),
}
CONTROL_BYTES = 42240   # sizeof(Control) rounded up to 256: where the first region starts, and the size of the last one


def _offsets(lay):
    return [getattr(lay, r) for r in ScratchLayoutC.REGIONS]


def _sizes(lay):
    """Bytes of the eight regions in address order (the first Control block, the seven behind it)."""
    bounds = [0] + _offsets(lay) + [lay.bytes]
    return [b - a for a, b in zip(bounds, bounds[1:])]


def test_scratch_layout_literals():
    assert set(LAYOUTS) == {(n, c) for n in NS for c in CAPS}
    for (n, cap), want in LAYOUTS.items():
        lay = scratch_layout(n, cap)
        got = (lay.bytes, *_offsets(lay), lay.depth_tiles, lay.inst_tiles, lay.pass_stride)
        assert got == want, (n, cap)
        assert (lay.n, lay.inst_cap) == (n, cap)


def test_scratch_layout_regions_are_aligned_ordered_and_disjoint():
    for n in NS + (255, 256, 257, 4095, 4096, 4097, 123_457):
        for cap in CAPS + (1, 4096, 4097):
            lay = scratch_layout(n, cap)
            offs = _offsets(lay)
            assert all(o % 256 == 0 for o in offs) and lay.bytes % 256 == 0
            # the documented order, each region non-empty and starting where the one before it ends (so: no overlap), the
            # total the end of the last
            assert offs[0] == CONTROL_BYTES and offs == sorted(offs) and all(s > 0 for s in _sizes(lay))
            assert lay.bytes == lay.off_ctl1 + CONTROL_BYTES
            # what the kernels index: four depth passes and two tile passes of look-back words, one spare tile each
            assert lay.depth_tiles == -(-n // 2048) + 1 and lay.inst_tiles == -(-cap // 4096) + 1
            assert lay.pass_stride == lay.depth_tiles * 256
            assert lay.off_scan_status - lay.off_depth_status >= 4 * lay.pass_stride * 4
            assert lay.off_ranges - lay.off_tile_status >= 2 * lay.inst_tiles * 256 * 4
            assert lay.off_ctl1 - lay.off_part_status >= (-(-n // 2048) + 1) * 4


def test_scratch_layout_never_shrinks_a_region_when_a_capacity_grows():
    ns = sorted(NS + (255, 256, 257, 4095, 4096, 4097, 123_457))
    caps = sorted(CAPS + (1, 4096, 4097))
    for cap in caps:
        for n0, n1 in zip(ns, ns[1:]):
            assert all(a <= b for a, b in zip(_sizes(scratch_layout(n0, cap)), _sizes(scratch_layout(n1, cap))))
    for n in ns:
        for c0, c1 in zip(caps, caps[1:]):
            assert all(a <= b for a, b in zip(_sizes(scratch_layout(n, c0)), _sizes(scratch_layout(n, c1))))


# ---- Buffer ----------------------------------------------------------------------------------------------------------

class Mem:
    """The shim's counting memory policy."""

    def __init__(self, fail_at=0):
        shim().shim_mem_reset(fail_at)

    @staticmethod
    def counters():
        out = (ctypes.c_int64 * 5)()
        shim().shim_mem_counters(out)
        return dict(zip(("live", "peak", "allocs", "frees", "last_bytes"), out))


class Buf:
    """One Buffer<uint64_t, CountingMem> of the shim."""

    def __init__(self, handle=None):
        self.h = handle if handle is not None else shim().shim_buf_new()

    def reserve(self, count, min_bytes=-1):
        return bool(shim().shim_buf_reserve(self.h, count, min_bytes))

    def state(self):
        out = (ctypes.c_uint64 * 2)()
        shim().shim_buf_state(self.h, out)
        return int(out[0]), int(out[1])

    def delete(self):
        shim().shim_buf_delete(self.h)


@pytest.fixture
def live_before():
    live = Mem.counters()["live"] if shim() else 0
    yield live
    assert Mem.counters()["live"] == live   # nothing is live after destruction, whatever the test did


def test_buffer_reserve_keeps_grows_and_fails(live_before):
    Mem()
    b = Buf()
    assert b.state() == (0, 0)
    assert b.reserve(100) and Mem.counters()["last_bytes"] == 800
    ptr, cap = b.state()
    assert ptr != 0 and cap == 100 and Mem.counters()["allocs"] == 1
    # within capacity: no allocation, the same pointer
    for count in (100, 99, 1, 0):
        assert b.reserve(count) and b.state() == (ptr, 100)
    assert Mem.counters()["allocs"] == 1 and Mem.counters()["frees"] == 0
    # growth frees BEFORE it allocates: never two allocations at once
    Mem()
    assert b.reserve(101) and b.state()[1] == 101
    c = Mem.counters()
    assert (c["allocs"], c["frees"], c["peak"] - live_before, c["live"] - live_before) == (1, 1, 1, 1)
    # a failed reserve leaves {null, 0} and nothing live; the next one allocates again
    Mem(fail_at=1)
    assert not b.reserve(1000) and b.state() == (0, 0)
    c = Mem.counters()
    assert (c["allocs"], c["frees"], c["live"] - live_before) == (1, 1, 0)
    assert b.reserve(1000) and b.state()[1] == 1000
    b.delete()


def test_buffer_minimum_sizes(live_before):
    Mem()
    b = Buf()
    # a zero-length request still allocates: one element by default, min_bytes where the caller gives one
    assert b.reserve(0) and b.state()[0] != 0 and b.state()[1] == 0 and Mem.counters()["last_bytes"] == 8
    assert b.reserve(0) and Mem.counters()["allocs"] == 1
    shim().shim_buf_reset(b.h)
    assert b.state() == (0, 0)
    assert b.reserve(3, 256) and b.state()[1] == 3 and Mem.counters()["last_bytes"] == 256
    assert b.reserve(33, 256) and b.state()[1] == 33 and Mem.counters()["last_bytes"] == 264
    b.delete()


def test_buffer_move_leaves_the_source_empty(live_before):
    Mem()
    a, b = Buf(), Buf()
    assert a.reserve(10) and b.reserve(20)
    pa = a.state()[0]
    shim().shim_buf_move_assign(b.h, a.h)   # frees what b held
    assert a.state() == (0, 0) and b.state() == (pa, 10)
    assert Mem.counters()["frees"] == 1 and Mem.counters()["live"] - live_before == 1
    c = Buf(shim().shim_buf_move_new(b.h))
    assert b.state() == (0, 0) and c.state() == (pa, 10) and Mem.counters()["allocs"] == 2
    shim().shim_buf_move_assign(c.h, c.h)   # self-move: a no-op
    assert c.state() == (pa, 10)
    for x in (a, b):
        x.delete()
    assert Mem.counters()["live"] - live_before == 1
    c.delete()   # the destructor frees
    assert Mem.counters()["live"] - live_before == 0 and Mem.counters()["frees"] == 2
    d = Buf()
    assert d.reserve(5)
    shim().shim_buf_release_and_free(d.h)   # release() hands the allocation over: the buffer forgets it
    assert d.state() == (0, 0)
    d.delete()


@pytest.mark.parametrize("failing", (1, 2, 3))
def test_buffer_group_is_all_or_nothing(live_before, failing):
    """The regression test for the sort lists' allocation: when the second or third of the three failed, the first stayed live
    beside a stale capacity, the next call took the group for complete and the frame launched with a null list."""
    Mem()
    g = [Buf(), Buf(), Buf()]
    group = lambda count: shim().shim_buf_reserve_group(g[0].h, g[1].h, g[2].h, count)
    assert group(64) == -1 and all(b.state()[1] == 64 for b in g)
    Mem(fail_at=failing)
    assert group(1000) == failing - 1   # which member could not be had
    assert all(b.state() == (0, 0) for b in g) and Mem.counters()["live"] - live_before == 0
    # ... and a later request allocates all three anew — one the capacity from before the failure would have covered (the
    # stale "it is all there already") as much as the same one again
    Mem()
    assert group(64) == -1 and Mem.counters()["allocs"] == 3 and all(b.state()[0] != 0 and b.state()[1] == 64 for b in g)
    Mem()
    assert group(1000) == -1
    assert Mem.counters()["allocs"] == 3 and all(b.state()[0] != 0 and b.state()[1] == 1000 for b in g)
    # complete and large enough: nothing happens
    Mem()
    assert group(1000) == -1 and group(7) == -1 and Mem.counters()["allocs"] == 0 and Mem.counters()["frees"] == 0
    # one member missing: the group is not complete, all of it is made anew, freed first
    shim().shim_buf_reset(g[1].h)
    Mem()
    assert group(1000) == -1
    c = Mem.counters()
    assert (c["allocs"], c["frees"], c["peak"] - live_before) == (3, 2, 3)
    for b in g:
        b.delete()
