"""The context's learnt state and the rules that write it (csrc/adaptive_state.h), driven through the host shim: no GPU, no
frames, counts instead of clouds. Every expected value is worked out here from the rule as it is documented; nothing is
read back from the library and called expected."""
import ctypes
import math

import numpy as np
import pytest

from bevy_gaussian_splatting_amd.camera import BgsView
from bevy_gaussian_splatting_amd.settings import BgsSettings
import helpers

U32_MAX = 0xFFFFFFFF
SLOTS = 16
SORT_RADIX, SORT_RAYON = 1, 2     # include/bgs.h (0: none, 3: std)
CLOUD_A, CLOUD_B = 0x1000, 0x2000   # a cloud is an identity and a length
EDGES_1080P = (6, 8, 16, 32)


class State:
    """An AdaptiveState behind the shim's opaque handle."""

    def __init__(self):
        self.lib = helpers.shim()
        self.h = self.lib.shim_state_new()

    def __del__(self):
        self.lib.shim_state_delete(self.h)

    def get(self) -> dict:
        out = (ctypes.c_uint64 * len(helpers.STATE_FIELDS))()
        self.lib.shim_state_get(self.h, out)
        return dict(zip(helpers.STATE_FIELDS, (int(v) for v in out)))

    def slot(self, i: int, nkeys: int = 0) -> dict:
        out, reach, keys = (ctypes.c_uint64 * 5)(), ctypes.c_float(0), (ctypes.c_uint32 * max(nkeys, 1))()
        self.lib.shim_state_slot(self.h, i, out, ctypes.byref(reach), keys, nkeys)
        return {"epoch": int(out[0]), "last_used": int(out[1]), "sub": int(out[2]), "n": int(out[3]), "cloud": int(out[4]),
                "reach": float(reach.value), "keys": list(keys)[:nkeys]}

    def epochs(self):
        return [self.slot(i)["epoch"] for i in range(SLOTS)]

    def kind(self, kind: int):
        """None if the kind is not settled, else (level, midround)."""
        level, mid = ctypes.c_uint32(0), ctypes.c_int(0)
        if not self.lib.shim_state_kind(self.h, kind, ctypes.byref(level), ctypes.byref(mid)):
            return None
        return int(level.value), bool(mid.value)

    def find(self, cloud, n, view, settings) -> int:
        return self.lib.shim_state_find_splitter_slot(self.h, cloud, n, ctypes.byref(view), ctypes.byref(settings))

    def store(self, keys, view, settings, *, cloud=CLOUD_A, n=100_000, sub=1, places=4, draw_count=50_000, seq=0):
        arr = (ctypes.c_uint32 * len(keys))(*keys)
        self.lib.shim_state_store_splitters(self.h, arr, sub, places, draw_count, cloud, n, ctypes.byref(view), ctypes.byref(settings), seq)

    def learn_level(self, kind, lv, edges, instances, visible, longest):
        verdict = self.lib.shim_state_learn_level(self.h, kind, lv, (ctypes.c_uint32 * 4)(*edges), instances, visible, longest)
        return bool(verdict & 1), bool(verdict & 2)   # moved, changed

    def __getattr__(self, name):   # every other rule: the shim's export of that name, on this state
        fn = getattr(self.lib, "shim_state_" + name)
        return lambda *args: fn(self.h, *args)


def make_view(pos=(0.0, 0.0, 0.0), angle=0.0, width=640, height=360, fov_scale=1.0, samples=0, depth_ptr=0) -> BgsView:
    """A camera at `pos` looking down -Z turned by `angle` (radians) about Y."""
    v = BgsView()
    m = np.eye(4, dtype=np.float32)
    m[:3, 0] = [math.cos(angle), 0.0, -math.sin(angle)]
    m[:3, 2] = [math.sin(angle), 0.0, math.cos(angle)]   # the view frame's +Z: the camera looks down its negative
    m[:3, 3] = pos
    v.world_from_view[:] = m.T.reshape(-1).tolist()      # column-major
    v.clip_from_view[:] = [fov_scale, 0, 0, 0, 0, fov_scale * 16 / 9, 0, 0, 0, 0, 0, -1, 0, 0, 0.1, 0]
    v.viewport[:] = [0.0, 0.0, float(width), float(height)]
    v.sample_count = samples
    v.depth_device_ptr = depth_ptr
    return v


def make_settings(sort_mode=SORT_RADIX, scale=1.0, translate=0.0, **fields) -> BgsSettings:
    s = BgsSettings()
    s.transform[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, translate, 0, 0, 1]
    s.global_opacity, s.global_scale = 1.0, scale
    s.gaussian_mode, s.opacity_adaptive_radius, s.radix_depth_bits, s.sort_mode = 1, 1, 32, sort_mode
    for k, val in fields.items():
        setattr(s, k, val)
    return s


def table(median_d2=100.0, sub=1, mid_bits=None):
    """256 * sub - 1 ascending keys whose median key says the median drawable splat lies sqrt(median_d2) away: keys are
    0xFFFFFFFF - bits(distance^2)."""
    if mid_bits is None:
        mid_bits = int(np.float32(median_d2).view(np.uint32))
    mid = 256 * sub // 2 - 1
    mid_key = U32_MAX - mid_bits
    assert mid_key >= mid
    return [min(i, mid_key) if i < mid else mid_key for i in range(256 * sub - 1)]


def pow2_ceil(v: int) -> int:
    p = 1
    while p < v:
        p <<= 1
    return min(p, 1 << 31)


# ---- draw hint -------------------------------------------------------------------------------------------------------------

def test_draw_hint_goes_up_at_once_and_down_after_64_frames_in_a_row():
    st = State()
    assert st.get()["draw_hint_valid"] == 0
    st.learn_draw_count(1000)
    assert (st.get()["draw_hint_valid"], st.get()["draw_hint"]) == (1, 1000 + 1000 // 8 + 1024)
    st.learn_draw_count(5000)
    hint = 5000 + 5000 // 8 + 1024
    assert st.get()["draw_hint"] == hint
    low, between = 100, 2000
    assert 4 * low < hint and 4 * between >= hint and between <= hint
    for _ in range(63):
        st.learn_draw_count(low)
        assert st.get()["draw_hint"] == hint
    st.learn_draw_count(between)          # one frame in between restarts the 64
    for _ in range(63):
        st.learn_draw_count(low)
        assert st.get()["draw_hint"] == hint
    st.learn_draw_count(low)              # the 64th in a row
    assert st.get()["draw_hint"] == 2 * low + 1024
    st.learn_draw_count(U32_MAX)
    assert st.get()["draw_hint"] == U32_MAX


# ---- list capacity ---------------------------------------------------------------------------------------------------------

def list_want(longest: int) -> int:
    return max(pow2_ceil(longest + longest // 4), 4096)


def test_list_capacity_goes_up_at_once_and_down_after_64_frames_in_a_row():
    st = State()
    roomy = 1 << 30
    assert st.get()["sup_level"] == 1
    assert st.learn_list_capacity(10_000, 1, roomy) == 0
    assert st.get()["coarse_cap_hint"] == list_want(10_000) == 16384
    assert st.learn_list_capacity(100_000, 1, roomy) == 0
    hint = list_want(100_000)
    assert st.get()["coarse_cap_hint"] == hint == 131072
    short, between = 1000, 20_000
    assert 8 * list_want(short) <= hint and 8 * list_want(between) > hint and list_want(between) <= hint
    for _ in range(63):
        st.learn_list_capacity(short, 1, roomy)
    st.learn_list_capacity(between, 1, roomy)      # not in a row: starts over
    for _ in range(63):
        st.learn_list_capacity(short, 1, roomy)
        assert st.get()["coarse_cap_hint"] == hint
    # a frame that ran at another level than the one the context is on has no vote
    assert st.learn_list_capacity(short, 2, roomy) == 0
    assert st.get()["coarse_cap_hint"] == hint
    assert st.learn_list_capacity(400_000, 2, roomy) == 0
    assert st.get()["coarse_cap_hint"] == hint
    st.learn_list_capacity(between, 1, roomy)
    for _ in range(63):
        st.learn_list_capacity(short, 1, roomy)
        assert st.get()["coarse_cap_hint"] == hint
    st.learn_list_capacity(short, 1, roomy)        # the 64th
    assert st.get()["coarse_cap_hint"] == 2 * list_want(short) == 8192


@pytest.mark.parametrize("level", [1, 3])
def test_a_frame_that_dropped_list_entries_is_rerun_with_room_for_them(level):
    st = State()
    st.learn_list_capacity(1000, 1, 1 << 30)
    assert st.get()["coarse_cap_hint"] == 4096
    assert st.learn_list_capacity(50_000, level, 4096) == 1           # longest > the capacity it was given
    assert st.get()["coarse_cap_hint"] >= list_want(50_000) == 65536
    assert st.learn_list_capacity(4096, level, 4096) == 0             # exactly full is not dropped


def test_first_list_capacity_is_a_guess_from_the_cloud_size():
    st = State()
    assert st.list_capacity(1_000_000, 0) == max(pow2_ceil(1_000_000 // 64), 4096) == 16384
    assert st.get()["coarse_cap_hint"] == 16384
    assert st.list_capacity(5000, 0) == 5000          # never more than n: a list holds each rank at most once
    assert State().list_capacity(1000, 0) == 1000 and State().list_capacity(0, 0) == 1
    small = State()
    assert small.list_capacity(1_000_000, 1) == 64 and small.get()["coarse_cap_hint"] == 64


# ---- tile-instance capacity (BINNING_SORT) ---------------------------------------------------------------------------------

MIN_INSTANCES, MAX_INSTANCES = 1 << 22, 1 << 30


def instance_want(need: int):
    """The growth rule as check_capacities documents it: refused (None) past 2^30, else the next power of two from 2^22
    that holds the need and a quarter of it (integer division), never more than 2^30."""
    if need > MAX_INSTANCES:
        return None
    return min(next(1 << k for k in range(22, 64) if (1 << k) >= need + need // 4), MAX_INSTANCES)


def instance_capacity_for(need: int):
    limits = (ctypes.c_uint64 * 2)()
    cap = int(helpers.shim().shim_instance_capacity_for(need, limits))
    assert (int(limits[0]), int(limits[1])) == (MIN_INSTANCES, MAX_INSTANCES)
    return cap or None


def test_instance_capacity_grows_to_a_power_of_two_with_a_quarter_of_head_room_and_refuses_past_2_pow_30():
    def fits(k):   # the largest need a capacity of 2^k serves: need + need // 4 <= 2^k, 2^k / 1.25 rounded as the rule rounds
        need = (1 << k) * 4 // 5
        while need + 1 + (need + 1) // 4 <= 1 << k:
            need += 1
        assert need + need // 4 <= 1 << k < need + 1 + (need + 1) // 4 and abs(need - (1 << k) / 1.25) <= 1
        return need
    fits_22, fits_23, fits_30 = fits(22), fits(23), fits(30)
    expected = {
        0: 1 << 22, 1: 1 << 22,
        fits_22: 1 << 22, fits_22 + 1: 1 << 23,                 # 1.25 x need across 2^22, both ways
        (1 << 22) - 1: 1 << 23, 1 << 22: 1 << 23, (1 << 22) + 1: 1 << 23,
        (1 << 22) * 5 // 4: 1 << 23,                                     # a need of 1.25 x 2^22
        fits_23: 1 << 23, fits_23 + 1: 1 << 24,                          # 1.25 x need across 2^23, both ways
        (1 << 23) + 1: 1 << 24, (1 << 23) * 5 // 4: 1 << 24, (1 << 23) * 5 // 4 + 1: 1 << 24,
        fits_30 - 1: 1 << 30, fits_30: 1 << 30,
        fits_30 + 1: 1 << 30,                                            # 2^31 by the rule, held to the limit: the need still fits
        (1 << 30) - 1: 1 << 30, 1 << 30: 1 << 30,
        (1 << 30) + 1: None, (1 << 30) + 65536: None, (1 << 32) + 65536: None, (1 << 64) - 1: None,
    }
    for need, want in expected.items():
        assert instance_want(need) == want, need          # the transcription says what the table says
        assert instance_capacity_for(need) == want, f"need {need}: {instance_capacity_for(need)}, expected {want}"
    # the head-room is there: without it these needs would keep the smaller power of two
    for need in (fits_22 + 1, fits_23 + 1, 1 << 23):
        assert instance_capacity_for(need) >= 2 * next(1 << k for k in range(22, 31) if (1 << k) >= need)
    rng = np.random.default_rng(22)
    for need in (int(v) for v in rng.integers(0, (1 << 30) + (1 << 20), 2000)):
        cap = instance_capacity_for(need)
        assert cap == instance_want(need), need
        if cap is not None:
            assert cap >= need and cap & (cap - 1) == 0 and MIN_INSTANCES <= cap <= MAX_INSTANCES


# ---- bucket back-off -------------------------------------------------------------------------------------------------------

def test_bucket_overflow_backs_off_by_tables_that_failed_in_a_row():
    st = State()
    assert st.learn_bucket_sort(2, -1, 1) == 1 and st.get()["bucket_block"] == 256    # one key far too often
    st = State()
    assert st.learn_bucket_sort(3, -1, 1) == 1 and st.get()["bucket_block"] == 256
    st = State()
    blocks = []
    for epoch in range(1, 11):   # successively newer tables, each over capacity on its first use
        assert st.learn_bucket_sort(1, -1, epoch) == 1
        blocks.append(st.get()["bucket_block"])
        assert st.get()["split_failed_epoch"] == epoch
    assert blocks == [0, 0, 7, 15, 31, 63, 127, 255, 255, 255]
    assert st.get()["bucket_fail_streak"] == 8


def test_bucket_overflow_of_a_table_not_newer_than_the_last_failed_one_adds_nothing():
    st = State()
    st.learn_bucket_sort(1, -1, 5)
    st.learn_bucket_sort(1, -1, 6)
    for epoch in (6, 5, 1, 0):   # frames that were in flight with the same stale table, or an older one
        assert st.learn_bucket_sort(1, -1, epoch) == 1    # (the frame is re-run all the same)
        assert (st.get()["bucket_fail_streak"], st.get()["bucket_block"], st.get()["split_failed_epoch"]) == (2, 0, 6)
    st.learn_bucket_sort(1, -1, 7)
    assert (st.get()["bucket_fail_streak"], st.get()["bucket_block"]) == (3, 7)
    assert st.learn_bucket_sort(0, -1, 8) == 0            # a bucket frame that ran clean
    assert (st.get()["bucket_fail_streak"], st.get()["bucket_block"]) == (0, 7)
    st.learn_bucket_sort(1, -1, 9)
    assert (st.get()["bucket_fail_streak"], st.get()["bucket_block"]) == (1, 7)


def test_bucket_block_counts_down_on_frames_with_four_digit_places_only():
    st = State()
    for epoch in (1, 2, 3):
        st.learn_bucket_sort(1, -1, epoch)
    assert st.get()["bucket_block"] == 7
    for places in (0, 2, 3):
        st.frame_enqueued(places, -1, 1)
        assert st.get()["bucket_block"] == 7
    for left in (6, 5, 4, 3, 2, 1, 0, 0):
        st.frame_enqueued(4, -1, 1)
        assert st.get()["bucket_block"] == left


def test_failed_table_is_dropped_only_if_its_slot_still_holds_it():
    st, view, settings = State(), make_view(), make_settings()
    st.store(table(), view, settings, seq=1)
    st.store(table(), view, settings, seq=2)      # the same view: the same slot, a newer table
    assert st.epochs() == [2] + [0] * 15
    assert st.learn_bucket_sort(1, 0, 1) == 1     # a frame that sorted with the older table
    assert st.epochs() == [2] + [0] * 15
    assert st.learn_bucket_sort(1, 0, 2) == 1
    assert st.epochs() == [0] * 16
    st.store(table(), view, settings, seq=3)
    assert st.learn_bucket_sort(2, 0, 3) == 1     # ... on either kind of overflow
    assert st.epochs() == [0] * 16


# ---- splitter slots --------------------------------------------------------------------------------------------------------

REACH = 10.0                                          # of table(): sqrt(100)
NEAR = float(np.float32(0.05) * np.float32(REACH))    # the rule's bound on the camera's distance, in its own arithmetic


def test_table_fits_a_camera_near_the_pose_it_was_measured_at():
    st, settings = State(), make_settings()
    st.store(table(), make_view(), settings, seq=1)
    assert st.slot(0)["reach"] == REACH
    assert st.find(CLOUD_A, 100_000, make_view(), settings) == 0
    assert NEAR == 0.5
    assert st.find(CLOUD_A, 100_000, make_view(pos=(NEAR, 0, 0)), settings) == 0
    assert st.find(CLOUD_A, 100_000, make_view(pos=(0, 0, -NEAR)), settings) == 0
    assert st.find(CLOUD_A, 100_000, make_view(pos=(float(np.nextafter(np.float32(NEAR), np.float32(1))), 0, 0)), settings) == -1
    assert st.find(CLOUD_A, 100_000, make_view(pos=(0.4, 0.4, 0)), settings) == -1
    assert st.find(CLOUD_A, 100_000, make_view(angle=math.acos(0.9849)), settings) == 0
    assert st.find(CLOUD_A, 100_000, make_view(angle=-math.acos(0.9849)), settings) == 0
    assert st.find(CLOUD_A, 100_000, make_view(angle=math.acos(0.9847)), settings) == -1
    assert st.find(CLOUD_A, 100_000, make_view(angle=math.pi), settings) == -1


@pytest.mark.parametrize("sort_mode", [SORT_RADIX, SORT_RAYON])
def test_table_is_refused_for_another_cloud_transform_sort_mode_or_projection(sort_mode):
    st, view, settings = State(), make_view(), make_settings(sort_mode)
    st.store(table(), view, settings, seq=1)
    assert st.find(CLOUD_A, 100_000, view, settings) == 0
    assert st.find(CLOUD_B, 100_000, view, settings) == -1
    assert st.find(CLOUD_A, 100_001, view, settings) == -1
    assert st.find(CLOUD_A, 100_000, view, make_settings(sort_mode, translate=0.25)) == -1
    assert st.find(CLOUD_A, 100_000, view, make_settings(SORT_RAYON if sort_mode == SORT_RADIX else SORT_RADIX)) == -1
    # SORT_RADIX keys only what the frustum keeps: the projection and the viewport belong to its key; the others keep every splat
    other_view = 0 if sort_mode != SORT_RADIX else -1
    assert st.find(CLOUD_A, 100_000, make_view(fov_scale=1.5), settings) == other_view
    assert st.find(CLOUD_A, 100_000, make_view(width=641), settings) == other_view
    assert st.find(CLOUD_A, 100_000, make_view(height=361), settings) == other_view


def test_of_two_fitting_tables_the_nearer_one_wins():
    st, settings = State(), make_settings()
    st.store(table(), make_view(pos=(0, 0, 0)), settings, seq=1)
    st.store(table(), make_view(pos=(0.8, 0, 0)), settings, seq=2)      # too far from the first: a slot of its own
    assert st.epochs()[:3] == [1, 2, 0]
    # both fit (0.35 and 0.45 away, same direction): the lower distance / reach + (1 - cos) wins
    assert st.find(CLOUD_A, 100_000, make_view(pos=(0.35, 0, 0)), settings) == 0
    assert st.find(CLOUD_A, 100_000, make_view(pos=(0.45, 0, 0)), settings) == 1
    # at the same distance from both, the one it looks along: (1 - cos) of 5 degrees against 0
    turned = 5 * math.pi / 180
    st2 = State()
    st2.store(table(), make_view(pos=(0, 0, 0)), settings, seq=1)
    st2.store(table(), make_view(pos=(0.8, 0, 0), angle=turned), settings, seq=2)
    assert st2.find(CLOUD_A, 100_000, make_view(pos=(0.4, 0, 0), angle=turned), settings) == 1
    assert st2.find(CLOUD_A, 100_000, make_view(pos=(0.4, 0, 0)), settings) == 0


def test_seventeen_views_evict_the_least_recently_used_table_and_an_empty_slot_goes_first():
    st, settings = State(), make_settings()
    for i in range(SLOTS):
        st.store(table(), make_view(pos=(10.0 * i, 0, 0)), settings, seq=i + 1)
    assert st.epochs() == list(range(1, 17))
    st.frame_enqueued(4, 0, 100)                  # a frame sorts with slot 0's table: slot 1's is the oldest now
    st.store(table(), make_view(pos=(500.0, 0, 0)), settings, seq=101)
    assert st.epochs() == [1, 17] + list(range(3, 17))
    assert st.learn_bucket_sort(1, 9, 10) == 1    # slot 9 is emptied
    st.store(table(), make_view(pos=(600.0, 0, 0)), settings, seq=102)
    assert st.epochs() == [1, 17] + list(range(3, 10)) + [18] + list(range(11, 17))   # not slot 2, the least recently used
    st.store(table(), make_view(pos=(700.0, 0, 0)), settings, seq=103)
    assert st.epochs()[2] == 19
    assert st.get()["split_epoch"] == 19


def test_nothing_is_stored_for_a_list_that_cannot_serve_as_a_table():
    st, view, settings = State(), make_view(), make_settings()
    for places in (0, 2, 3):
        st.store(table(), view, settings, places=places)
    st.store(table(), view, settings, draw_count=255)
    descending = table()
    descending[40], descending[41] = descending[41], descending[40]
    st.store(descending, view, settings)
    st.store(table(), view, settings, cloud=None)
    assert st.epochs() == [0] * 16 and st.get()["split_epoch"] == 0
    st.store(table(), view, settings, draw_count=256, seq=7)
    assert st.epochs() == [1] + [0] * 15
    assert st.slot(0, 255) == {"epoch": 1, "last_used": 7, "sub": 1, "n": 100_000, "cloud": CLOUD_A, "reach": REACH, "keys": table()}


def test_reach_is_the_median_key_s_distance():
    view, settings = make_view(), make_settings()
    for d2 in (0.25, 2.0, 1.0e6):
        st = State()
        st.store(table(d2), view, settings)
        assert st.slot(0)["reach"] == float(np.sqrt(np.float32(d2)))
    st = State()
    st.store(table(400.0, sub=3), view, settings, sub=3)     # 767 keys: the median is key 383
    assert (st.slot(0)["sub"], st.slot(0)["reach"]) == (3, 20.0)
    assert st.slot(0, 767)["keys"] == table(400.0, sub=3)
    huge = int(np.float32(3.2e38).view(np.uint32))
    for bits in (0, 0x80000000 | int(np.float32(4.0).view(np.uint32)), huge, 0x7F800000, 0x7FC00000):   # 0, -4, > 3e38, inf, NaN
        st = State()
        st.store(table(mid_bits=bits), view, settings)
        assert st.epochs()[0] == 1 and st.slot(0)["reach"] == 1.0


def test_forget_cloud_empties_that_cloud_s_tables_only():
    st, settings = State(), make_settings()
    for i, cloud in enumerate((CLOUD_A, CLOUD_B, CLOUD_A, CLOUD_B)):
        st.store(table(), make_view(pos=(10.0 * i, 0, 0)), settings, cloud=cloud, seq=i + 1)
    before = st.get()
    st.forget_cloud(CLOUD_A)
    assert st.epochs()[:5] == [0, 2, 0, 4, 0]
    assert st.get() == before
    assert st.find(CLOUD_B, 100_000, make_view(pos=(10.0, 0, 0)), settings) == 1
    assert st.find(CLOUD_A, 100_000, make_view(pos=(0.0, 0, 0)), settings) == -1


# ---- kinds -----------------------------------------------------------------------------------------------------------------

def kind_of(n=100_000, fmt=0, view=None, settings=None) -> int:
    view, settings = view or make_view(), settings or make_settings()
    return helpers.shim().shim_frame_kind(n, fmt, ctypes.byref(view), ctypes.byref(settings))


def test_frame_kind_follows_what_the_capacities_depend_on_and_nothing_else():
    base = kind_of()
    # poses do not count; a cloud enters by its size and format alone (its address is not even an input)
    assert kind_of(view=make_view(pos=(3, 4, 5), angle=1.0)) == base
    assert kind_of(settings=make_settings(translate=2.0)) == base
    # the global scale to half an octave: the nearest integer of 2 * log2(scale)
    assert kind_of(settings=make_settings(scale=2.0 ** 0.24)) == kind_of(settings=make_settings(scale=2.0 ** -0.24)) == base
    assert kind_of(settings=make_settings(scale=2.0 ** 0.26)) != base
    assert kind_of(settings=make_settings(scale=2.0 ** 0.26)) == kind_of(settings=make_settings(scale=2.0 ** 0.74))
    assert kind_of(settings=make_settings(scale=2.0 ** 0.76)) != kind_of(settings=make_settings(scale=2.0 ** 0.74))
    assert kind_of(view=make_view(samples=4)) == base      # 0 = not set = 4 samples
    different = [kind_of(n=100_001), kind_of(fmt=1), kind_of(view=make_view(width=641)), kind_of(view=make_view(height=361)),
                 kind_of(view=make_view(samples=1)), kind_of(view=make_view(depth_ptr=0x7000)),
                 kind_of(settings=make_settings(rasterize_mode=1)), kind_of(settings=make_settings(gaussian_mode=0)),
                 kind_of(settings=make_settings(aabb=1)), kind_of(settings=make_settings(draw_mode=1)),
                 kind_of(settings=make_settings(visualize_bounding_box=1)), kind_of(settings=make_settings(scale=0.0)),
                 kind_of(settings=make_settings(scale=float("nan")))]
    assert len(set(different + [base])) == len(different)   # (scale 0 and NaN: one kind, "no scale step")
    assert different[-1] == different[-2]
    assert all(k != 0 for k in different + [base])
    rng = np.random.default_rng(5)
    for n, w, h in rng.integers(1, 4096, size=(200, 3)):
        assert kind_of(n=int(n), view=make_view(width=int(w), height=int(h))) != 0


def test_a_clean_frame_settles_its_kind_at_the_level_it_ran():
    st = State()
    assert st.kind(77) is None
    st.settle(77, 2)
    assert st.kind(77) == (2, False) and st.get()["kinds"] == 1
    assert st.get()["sup_level"] == 1               # the context moves when it switches to the kind, not before
    st.switch_kind(77)
    assert (st.get()["sup_level"], st.get()["cur_kind"]) == (2, 77)
    st.switch_kind(78)                              # a kind with no level of its own: the context stays where it is
    assert (st.get()["sup_level"], st.get()["cur_kind"]) == (2, 78)


def test_a_kind_that_never_runs_clean_is_settled_after_three_early_frames_in_total():
    st = State()
    for done in (1, 2):
        st.completed_early(5)
        assert st.kind(5) is None and st.get()["learning"] == 1
    st.completed_early(5)
    assert st.kind(5) == (1, False) and st.get()["learning"] == 0
    # two such kinds that alternate: three of EACH, not three in a row
    st = State()
    st.learn_level(0, 1, EDGES_1080P, 900, 100, 10)     # (the context is on level 2 by now: what they are settled at)
    assert st.get()["sup_level"] == 2
    for done in (1, 2):
        st.completed_early(5)
        st.completed_early(6)
        assert st.kind(5) is None and st.kind(6) is None and st.get()["learning"] == 2
    st.completed_early(5)
    assert st.kind(5) == (2, False) and st.kind(6) is None
    st.completed_early(6)
    assert st.kind(6) == (2, False) and st.get()["learning"] == 0
    # a frame completed early that did run clean (settle) just ends the count
    st = State()
    st.completed_early(9)
    st.settle(9, 3)
    st.completed_early(9)
    assert st.kind(9) == (3, False) and st.get()["learning"] == 0


def test_forty_kinds_are_kept_each_with_its_own_level():
    st = State()
    for k in range(1, 41):
        st.settle(k, k % 4)
    assert st.get()["kinds"] == 40
    for k in range(1, 41):
        assert st.kind(k) == (k % 4, False)
        st.switch_kind(k)
        assert st.get()["sup_level"] == k % 4


def next_level(ratio, lv, edges):
    """frame_params.h next_supertile_level as documented there -> (target, by how much the longest list grows)."""
    if not (ratio > 4.0 and lv < 3) and not (ratio < 1.6 and lv > 0):
        return lv, 1.0
    extent = max(math.sqrt(ratio) - 1.0, 0.0) * edges[lv]
    target = next((k for k in range(4) if edges[k] >= extent), 3)
    target = max(target, lv + 1) if ratio > 4.0 else min(target, lv - 1)
    longer = 1.0
    if target > lv:
        longer = max(((extent / edges[target] + 1.0) ** 2 / ratio) * (edges[target] / edges[lv]) ** 2, 1.0)
    return target, longer


def test_learn_level_moves_the_context_and_predicts_the_new_lists():
    for lv, instances, visible, longest in ((1, 900, 100, 10_000), (2, 120, 100, 10_000), (0, 2500, 100, 3000), (1, 900, 100, U32_MAX)):
        target, longer = next_level(instances / visible, lv, EDGES_1080P)
        assert target != lv
        st = State()
        st.learn_level(0, 1, EDGES_1080P, *((900, 100, 1) if lv == 2 else (100, 100, 1) if lv == 0 else (200, 100, 1)))
        assert st.get()["sup_level"] == lv
        st.learn_list_capacity(100_000, lv, 1 << 30)
        for _ in range(5):
            st.learn_list_capacity(10, lv, 1 << 30)
        assert st.get()["list_shrink_votes"] == 5
        assert st.learn_level(0, lv, EDGES_1080P, instances, visible, longest) == (True, True)
        want = max(pow2_ceil(int(min(longest * (longer if target > lv else 1.0) * 1.25, 1.0e9))), 4096)
        got = st.get()
        assert (got["sup_level"], got["coarse_cap_hint"], got["list_shrink_votes"]) == (target, want, 0)
    # inside the band, or without room to move: no verdict
    st = State()
    for ratio_x100 in (160, 250, 400):
        assert st.learn_level(0, 1, EDGES_1080P, ratio_x100, 100, 10_000) == (False, False)
    assert st.get()["sup_level"] == 1 and st.get()["coarse_cap_hint"] == 0


def test_learn_level_of_a_frame_of_another_kind_belongs_to_that_kind():
    st = State()
    st.settle(11, 1)
    st.settle(12, 1)
    st.switch_kind(11)
    st.learn_list_capacity(100_000, 1, 1 << 30)
    st.learn_list_capacity(10, 1, 1 << 30)
    before = st.get()
    assert before["list_shrink_votes"] == 1
    target, _ = next_level(9.0, 1, EDGES_1080P)
    assert st.learn_level(12, 1, EDGES_1080P, 900, 100, 50_000) == (True, False)   # it asks for a move; the context does not make it
    assert st.kind(12) == (target, False) and st.kind(11) == (1, False)
    assert st.get() == before
    # ... and of the kind the context is on: the kind's level and the context's
    assert st.learn_level(11, 1, EDGES_1080P, 900, 100, 50_000) == (True, True)
    assert st.kind(11) == (target, False) and st.get()["sup_level"] == target
    # a frame that ran before the context moved (frames in flight) and asks for where it already is: no second change
    hint = st.get()["coarse_cap_hint"]
    assert st.learn_level(11, 1, EDGES_1080P, 900, 100, 400_000) == (True, False)
    assert st.get()["coarse_cap_hint"] == hint


def test_levels_whose_edges_coincide_are_one_level():
    edges = (24, 32, 32, 32)     # a target of ~4096 px: levels 2 and 3 are level 1
    target, _ = next_level(9.0, 1, edges)
    assert target > 1
    st = State()
    st.settle(3, 1)
    st.switch_kind(3)
    st.learn_list_capacity(100_000, 1, 1 << 30)
    before = st.get()
    assert st.learn_level(3, 1, edges, 900, 100, 50_000) == (False, False)
    assert st.get() == before and st.kind(3) == (1, False)


# ---- mid-round hysteresis --------------------------------------------------------------------------------------------------

def test_midround_choice_has_hysteresis():
    full = 0x7FFF
    on, below_on = math.ceil(0.30 * full), math.ceil(0.30 * full) - 1
    off, above_off = math.floor(0.15 * full), math.floor(0.15 * full) + 1
    assert on / full >= 0.30 > below_on / full and off / full <= 0.15 < above_off / full
    st = State()
    st.settle(21, 1)
    for share, expect in ((below_on, False), (above_off, False), (on, True), (below_on, True), (above_off, True), (U32_MAX, True),
                          (off, False), (U32_MAX, False), (above_off, False), (full, True), (0, False)):
        st.learn_saturation(21, share)       # 0xFFFFFFFF: the frame had no report
        assert st.kind(21) == (1, expect), share
    st.learn_saturation(22, full)            # a kind that is not settled is left alone (and not created)
    st.learn_saturation(0, full)
    assert st.kind(22) is None and st.get()["kinds"] == 1


# ---- reset() and distrust() ------------------------------------------------------------------------------------------------

def drive(st: State, stale_epoch: int):
    """A mixed sequence of rules; returns everything it can see, epochs relative to the ones handed out before it."""
    seen, settings = [], make_settings()
    base = st.get()["split_epoch"]

    def look():
        got = st.get()
        got["split_epoch"] -= base
        got["split_failed_epoch"] -= base
        seen.append(got)
        seen.append([(e - base if e else 0) for e in st.epochs()])

    for c in (3000, 70_000, 100):
        st.learn_draw_count(c)
        look()
    seen.append(st.list_capacity(200_000, 0))
    st.switch_kind(31)
    seen.append(st.learn_list_capacity(30_000, 1, 4096))
    seen.append(st.learn_level(31, 1, EDGES_1080P, 900, 100, 30_000))
    st.completed_early(31)
    look()
    for i in range(3):
        st.store(table(), make_view(pos=(10.0 * i, 0, 0)), settings, seq=i + 1)
    look()
    seen.append(st.find(CLOUD_A, 100_000, make_view(pos=(10.0, 0, 0)), settings))
    # a frame that was planned with a table from before: not newer than anything, and no slot holds it
    seen.append(st.learn_bucket_sort(1, 1, stale_epoch))
    look()
    for i in range(3):
        seen.append(st.learn_bucket_sort(1, i, base + i + 1))
        st.frame_enqueued(4, -1, 10 + i)
    look()
    st.settle(31, 2)
    st.learn_saturation(31, 0x7FFF)
    seen.append([st.kind(k) for k in (31, 32)])
    for _ in range(2):
        st.completed_early(32)
    look()
    return seen


def test_reset_leaves_a_state_that_answers_like_a_new_one():
    used, settings = State(), make_settings()
    drive(used, 0)
    for i in range(SLOTS + 2):     # every slot taken, in an order of use that is not the order of the slots
        used.store(table(), make_view(pos=(0, 10.0 * i, 0)), settings, cloud=CLOUD_B, seq=1000 - i)
    for _ in range(40):
        used.learn_draw_count(10)
        used.learn_list_capacity(10, used.get()["sup_level"], 1 << 30)
    used.learn_bucket_sort(2, -1, 1)
    before = used.get()
    # (41: the last count of drive() was under a quarter of the hint too)
    assert before["draw_shrink_votes"] == 41 and before["list_shrink_votes"] == 40 and before["bucket_block"] == 256
    assert all(used.epochs())
    used.reset()
    after = used.get()
    assert after["split_epoch"] == before["split_epoch"] == after["split_failed_epoch"]     # epochs stay monotonic
    assert drive(used, before["split_epoch"]) == drive(State(), 0)
    # epochs handed out after the reset exceed those handed out before: drive() stored three tables, this is the fourth
    assert used.epochs() == [0] * 16
    used.store(table(), make_view(), settings, seq=2000)
    assert used.epochs() == [before["split_epoch"] + 4] + [0] * 15


def test_distrust_invalidates_the_draw_hint_and_every_table_and_nothing_else():
    st = State()
    drive(st, 0)
    st.store(table(), make_view(), make_settings(), seq=50)
    before, kinds = st.get(), [st.kind(k) for k in (31, 32)]
    assert before["draw_hint_valid"] == 1 and any(st.epochs())
    st.distrust()
    assert st.epochs() == [0] * 16
    assert st.get() == {**before, "draw_hint_valid": 0}
    assert [st.kind(k) for k in (31, 32)] == kinds
