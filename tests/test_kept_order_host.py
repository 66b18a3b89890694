"""The kept sort order, the part that needs no GPU: the seam's struct keeps its layout, the device-resident entries' chunk
arithmetic, `render_with_trigger` against the reference's trigger policy under an injected clock, and the compaction's
index arithmetic (csrc/entries_math.h, what the HIP kernel runs) as a g++ program against numpy."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
from bevy_gaussian_splatting_amd import (
    CloudSettings, DeviceEntriesChunk, DeviceSortedEntries, GaussianSplattingPlugin, SortConfig, SortTrigger, View, _native,
    update_sort_trigger)
from bevy_gaussian_splatting_amd.camera import BgsView
from bevy_gaussian_splatting_amd.plugin import SORT_ENTRY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
TOOL = os.path.join(HERE, "cpp", "entries_tool")
CULLED = 0xFFFFFFFF


def test_view_struct_keeps_its_size_and_offsets():
    """bgs_view of ABI 0.4: the two fields took the place of reserved ones."""
    base = (16 * 4 + 8 + 16) * 4   # the matrices, viewport, clear colour and previous_clip_from_world
    assert ctypes.sizeof(BgsView) == base + 4 * 4 + 16 == 384   # (what tests/test_abi.py pins)
    offsets = {name: getattr(BgsView, name).offset for name, _ in BgsView._fields_}
    assert offsets["delta_time"] == base and offsets["sample_count"] == base + 4
    assert offsets["entry_count"] == base + 8 and offsets["reserved"] == base + 12      # was reserved[0], reserved[1]
    assert offsets["depth_device_ptr"] == base + 16 and offsets["entries_device_ptr"] == base + 24   # was reserved_ptr
    assert BgsView.entry_count.size == 4 and BgsView.reserved.size == 4 and BgsView.entries_device_ptr.size == 8
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    struct = header[header.index("typedef struct bgs_view {"):header.index("} bgs_view;")]
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = re.findall(r"\b(?:float|uint32_t|uint64_t)\s+(\w+)", struct)
    assert fields == [name for name, _ in BgsView._fields_]
    assert "reserved_ptr" not in header
    lib = _native.load()
    assert lib.bgs_version() == H.header_version() == _native.ABI_VERSION
    # zero in both fields is what the helpers hand out
    v = View.headless(64, 64).to_native()
    assert v.entries_device_ptr == 0 and v.entry_count == 0
    out = BgsView()
    out.entries_device_ptr, out.entry_count = 0xDEAD, 7
    lib.bgs_view_perspective(v.world_from_view, ctypes.c_float(0.7), ctypes.c_float(0.1), 64, 64, ctypes.byref(out))
    assert out.entries_device_ptr == 0 and out.entry_count == 0 and list(out.reserved) == [0]
    w = View.headless(64, 64)
    w.entries = DeviceEntriesChunk(0x1000, 5)
    n = w.to_native()
    assert n.entries_device_ptr == 0x1000 and n.entry_count == 5


class FakePlugin(GaussianSplattingPlugin):
    """The plugin's host logic over stubbed device calls: a bump allocator and a log."""

    def __init__(self):   # (no library, no context)
        self._ctx = "stub"
        self.calls = []
        self._next = 0x10000
        self.uploads = {}

    def device_alloc(self, nbytes):
        p = self._next
        self._next += (int(nbytes) + 255) // 256 * 256
        self.calls.append(("alloc", int(nbytes)))
        return p

    def device_free(self, ptr):
        self.calls.append(("free", ptr))

    def upload_bytes(self, ptr, host):
        self.uploads[ptr] = np.array(host, copy=True)

    def sort(self, handle, view, settings, download=True, into=None):
        self.calls.append(("sort", into.ptr, into.count))

    def render(self, handle, view, settings=None, download=True, entries=None):
        self.calls.append(("render", entries.ptr, entries.count))
        return "frame"

    def close(self):
        pass


def test_device_sorted_entries_chunk_arithmetic():
    p = FakePlugin()
    dse = DeviceSortedEntries(p, 3, 5000)
    assert p.calls == [("alloc", 3 * 5000 * 8)] and dse.nbytes == 120000
    assert [DeviceSortedEntries.chunk_offset(c, 5000) for c in range(4)] == [0, 40000, 80000, 120000]
    chunks = [dse.chunk(c) for c in range(3)]
    assert [c.ptr - dse.ptr for c in chunks] == [0, 40000, 80000] and all(c.count == 5000 and c.ptr % 8 == 0 for c in chunks)
    # an odd cloud length still leaves every chunk aligned to one entry, and the chunks tile the block exactly
    odd = DeviceSortedEntries(p, 4, 4097)
    assert [odd.chunk(c).ptr - odd.ptr for c in range(4)] == [c * 4097 * 8 for c in range(4)]
    assert odd.chunk(3).ptr + 4097 * 8 == odd.ptr + odd.nbytes
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            dse.chunk(bad)
    # the asset's initial content: key 1, identity order, in every chunk (src/sort/mod.rs:347-354)
    init = p.uploads[dse.ptr]
    assert init.dtype == SORT_ENTRY_DTYPE and init.shape == (15000,)
    assert (init["key"] == 1).all() and np.array_equal(init["index"], np.tile(np.arange(5000, dtype=np.uint32), 3))
    dse.upload(1, np.zeros(5000, SORT_ENTRY_DTYPE))
    assert dse.chunk(1).ptr in p.uploads
    with pytest.raises(ValueError):
        dse.upload(1, np.zeros(4999, SORT_ENTRY_DTYPE))
    dse.free()
    assert p.calls[-1] == ("free", chunks[0].ptr) and dse.ptr is None
    dse.free()   # idempotent
    assert p.calls.count(("free", chunks[0].ptr)) == 1
    with pytest.raises(ValueError):
        dse.chunk(0)
    with pytest.raises(ValueError):
        DeviceSortedEntries(p, 0, 10)
    empty = DeviceSortedEntries(p, 2, 0)   # an empty cloud: a block all the same, no upload
    assert empty.chunk(1).count == 0 and empty.ptr not in p.uploads


def test_render_with_trigger_sorts_exactly_when_the_policy_says_so():
    """update_sort_trigger (src/sort/mod.rs:164-193) under an injected clock: the first frame sorts; inside the period
    nothing does, moved camera or not; past it a moved camera does, a resting one does not."""
    p = FakePlugin()
    chunk = DeviceEntriesChunk(0x4000, 100)
    cfg, trig, s = SortConfig(period_ms=1000), SortTrigger(), CloudSettings()
    clock = {"t": 10.0}
    script = [  # (time, camera x, sorts?)
        (10.0, 0.0, True),     # first frame
        (10.2, 0.0, False),    # inside the period
        (10.5, 1.0, False),    # moved, still inside the period: drawn from the stale chunk
        (11.1, 1.0, True),     # period over, position differs from the last sorted one
        (11.2, 2.0, False),    # the period restarted with that sort
        (12.3, 1.0, False),    # period over, camera back where it was sorted last
        (12.4, 3.0, True),
    ]
    for t, x, sorts in script:
        clock["t"] = t
        v = View.headless(32, 32)
        v.world_from_view[0, 3] = x
        update_sort_trigger(trig, v.world_position, v.camera.order, cfg, now=lambda: clock["t"])
        before = len(p.calls)
        assert trig.needs_sort == sorts, (t, x)
        out = p.render_with_trigger(None, v, s, trig, chunk)
        made = p.calls[before:]
        assert out == "frame" and trig.needs_sort is False
        assert made == ([("sort", 0x4000, 100)] if sorts else []) + [("render", 0x4000, 100)], (t, x, made)


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", TOOL, os.path.join(HERE, "cpp", "entries_tool.cpp")],
                   check=True, capture_output=True)
    return TOOL


def test_compaction_arithmetic_constants_and_selftest(tool):
    threads, items, tile, rows, grid_max, sweep = (int(x) for x in subprocess.run([tool, "constants"], capture_output=True, text=True,
                                                                                   check=True).stdout.split())
    assert (threads, items, tile, rows) == (256, 8, 2048, 32) and sweep == grid_max * tile == 524288
    # a tile is a chain word of keygen's: the rasteriser's clean-up zeroes ceil(n / KEYGEN_TILE) of them
    dev = open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "bgs_device.h")).read()
    assert int(re.search(r"KEYGEN_TILE\s*=\s*(\d+)", dev).group(1)) == tile
    assert subprocess.run([tool, "selftest"], capture_output=True, text=True, check=True).stdout.strip() == "ok"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2048, 2049, 4097, 70001])
def test_compaction_arithmetic_against_numpy(tool, tmp_path, n):
    rng = np.random.default_rng(n)
    for pattern in range(4):
        e = np.empty(n, SORT_ENTRY_DTYPE)
        e["key"] = rng.integers(0, CULLED, n, dtype=np.uint32)
        e["index"] = rng.permutation(n)
        if pattern == 1:
            e["key"][0::4] = CULLED
            e["index"][2::4] = n + 3
        elif pattern == 2:
            e["key"][:-1] = CULLED
        elif pattern == 3:
            e["key"][:] = CULLED
        src, out, tail = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "tail.bin"
        e.tofile(src)
        d, tiles, blocks = (int(x) for x in subprocess.run([tool, "compact", str(src), str(n), str(out), str(tail)], capture_output=True,
                                                           text=True, check=True).stdout.split())
        keep = (e["key"] != CULLED) & (e["index"] < n)
        want, want_tail = e[keep], e[~keep].copy()
        want_tail["index"] = np.minimum(want_tail["index"], n - 1)
        assert d == len(want) and tiles == -(-n // 2048) and blocks == min(tiles, 256)
        assert np.fromfile(out, SORT_ENTRY_DTYPE).tobytes() == want.tobytes()
        assert np.fromfile(tail, SORT_ENTRY_DTYPE).tobytes() == want_tail.tobytes()
