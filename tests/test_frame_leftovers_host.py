"""What a frame leaves behind, the part that needs no GPU (tests/frame_leftover_cases.py): the clean-up's bounds cover what
the kernels' tile geometry can publish, both fit the lane's scratch layout, and the quantile reference is a usable table."""
import ctypes

import numpy as np
import pytest

import frame_leftover_cases as L
import helpers as H


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_the_clean_up_covers_what_the_frame_may_publish(name):
    case = L.by_name(name)
    info = L.planned_info(case)
    lay = H.scratch_layout(case.n, 0)
    for d in L.draw_counts(case):
        for tail in (0, 1):
            used, zeroed = L.words_used(dict(info, culled_tail=tail), d), L.words_zeroed(info, d)
            what = f"{name} D {d} culled_tail {tail}"
            assert used["passes"] <= zeroed["passes"] or used["depth"] == 0, what
            for region in L.CHAIN_REGIONS:
                assert used[region] <= zeroed[region], f"{what}: {region} publishes {used[region]} words, the clean-up zeroes {zeroed[region]}"
                for p in range(4 if region == "depth" else 1):
                    first, words = L.region_words(lay, region, p)
                    assert zeroed[region] <= words, f"{what}: the clean-up zeroes {zeroed[region]} {region} words, the region holds {words}"
                    assert (first + words) * 4 <= lay.bytes
    # the four depth arrays end where the next region starts
    assert L.region_words(lay, "depth", 3)[0] + lay.pass_stride <= lay.off_scan_status // 4


def test_the_layout_the_references_index_is_the_binding_s():
    from bevy_gaussian_splatting_amd import _native
    assert [f[0] for f in _native.BgsScratchLayout._fields_] == [f[0] for f in H.ScratchLayoutC._fields_]
    assert ctypes.sizeof(_native.BgsScratchLayout) == ctypes.sizeof(H.ScratchLayoutC) == H.shim().shim_scratch_layout_size()
    off = H.control_offsets()
    assert off["header_words"] == 12 and off["strip_tiles"] == 10 and off["saturated_tiles_prev"] == 11
    assert off["splitters"] == off["coarse_total"] + 256 and off["bucket_count"] == off["splitters"] + off["bucket_max_keys"]
    assert off["words"] == off["bucket_count"] + off["bucket_max_keys"] and off["bucket_max_keys"] == 4096


def _ascends(keys):
    return H.shim().shim_splitters_ascending(keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), keys.size) == 1


def test_quantile_keys_on_hand_made_lists():
    q = L.quantile_keys
    # D = 1: every quantile is the one key
    assert q(np.array([7], np.uint32), 1, 256, 0).tolist() == [7] * 255 + [0xFFFFFFFF]
    # D == nbk: key t + 1 of the list
    keys = np.arange(100, 356, dtype=np.uint32)
    assert q(keys, 256, 256, 0).tolist() == list(range(101, 356)) + [0xFFFFFFFF]
    # D < nbk: floor((t + 1) * D / nbk), every key 256 / D times over (the first one time short)
    got = q(np.array([10, 20, 30, 40], np.uint32), 4, 256, 0)
    assert got.tolist() == [10] * 63 + [20] * 64 + [30] * 64 + [40] * 64 + [0xFFFFFFFF]
    # the entries behind D are not read
    assert np.array_equal(q(np.array([10, 20, 30, 40, 1, 2, 3], np.uint32), 4, 256, 0), got)
    # D > nbk, sub 2
    keys = np.arange(0, 5120, 5, dtype=np.uint32)   # 1024 keys
    got = q(keys, 1024, 512, 0)
    assert got[0] == keys[2] and got[510] == keys[1022] and got[511] == 0xFFFFFFFF and got.size == 512
    # descending-key modes: the list descends in the sorted key, key ^ ~0 ascends
    desc = np.array([900, 700, 700, 300, 5], np.uint32)
    got = q(desc, 5, 256, 0xFFFFFFFF)
    assert got[0] == 900 ^ 0xFFFFFFFF and got[254] == 5 ^ 0xFFFFFFFF and _ascends(got)
    # duplicates, an empty list, structured entries
    assert q(np.full(1000, 42, np.uint32), 1000, 256, 0).tolist() == [42] * 255 + [0xFFFFFFFF]
    assert (q(np.zeros(0, np.uint32), 0, 768, 0) == 0xFFFFFFFF).all()
    ents = np.zeros(300, np.dtype([("key", np.uint32), ("index", np.uint32)]))
    ents["key"] = np.arange(300) * 3
    assert np.array_equal(q(ents, 300, 256, 0), q(ents["key"], 300, 256, 0))


@pytest.mark.parametrize("seed", range(6))
def test_quantile_keys_always_ascend(seed):
    rng = np.random.default_rng(seed)
    for d in (0, 1, 2, 255, 256, 257, 4095, 20000):
        keys = np.sort(rng.integers(0, 1 << 32, d, dtype=np.uint64).astype(np.uint32))
        if seed % 2:
            keys = np.sort(rng.integers(0, 16, d).astype(np.uint32))   # heavy ties
        for sub in (1, 2, 16):
            for xor in (0, 0xFFFFFFFF):
                # the list a frame leaves: sorted ascending in keygen's key, which Rayon / Std store complemented (it descends)
                left = keys ^ np.uint32(xor)
                got = L.quantile_keys(left, d, 256 * sub, xor)
                assert got.size == 256 * sub and got[-1] == 0xFFFFFFFF
                assert (np.diff(got.astype(np.int64)) >= 0).all() and _ascends(got), (d, sub, xor)
