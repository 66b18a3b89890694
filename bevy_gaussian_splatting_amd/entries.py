"""The sorted entries (src/sort/mod.rs:331-393): the (key, index) record, `SortedEntries` on the host, and
`DeviceSortedEntries` with its `DeviceEntriesChunk`s kept in device memory. `plugin.sort` fills them and `plugin.render`
draws from them; `bevy_gaussian_splatting_amd.plugin` still exports every name here."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .device_memory import DeviceBlock

SORT_ENTRY_DTYPE = np.dtype([("key", np.uint32), ("index", np.uint32)])


def initial_entries(camera_count: int, count: int) -> np.ndarray:
    """What the asset holds before any sort (src/sort/mod.rs:347-354): `camera_count` chunks of `count` entries, key 1 and
    index i in every chunk."""
    s = np.empty(camera_count * count, dtype=SORT_ENTRY_DTYPE)
    s["key"] = 1
    s["index"] = np.tile(np.arange(count, dtype=np.uint32), camera_count)
    return s


@dataclass
class SortedEntries:
    """src/sort/mod.rs:331-393: `camera_count * entry_count` (key, index) pairs, where the creator
    passes `entry_count = cloud.len_sqrt_ceil()**2` (src/sort/mod.rs:259-262). Camera `c` owns the
    chunk `sorted[c * gaussians : (c + 1) * gaussians]` with `gaussians = cloud.len()` — the stride is
    the CLOUD length, not entry_count, both where the sort writes (`chunks_mut(gaussians).nth(
    camera_index)`, src/sort/rayon.rs:82-84) and where the draw binds (dynamic offset
    `camera_index * 8 * cloud.len()`, src/render/mod.rs:1548-1554); the square-padding tail is unused."""

    camera_count: int
    entry_count: int
    sorted: np.ndarray  # structured SORT_ENTRY_DTYPE

    @staticmethod
    def new(camera_count: int, entry_count: int) -> "SortedEntries":
        return SortedEntries(camera_count, entry_count, initial_entries(camera_count, entry_count))

    @staticmethod
    def for_cloud(camera_count: int, cloud_len: int) -> "SortedEntries":
        """`auto_insert_sorted_entries` (src/sort/mod.rs:218-268)."""
        side = int(np.ceil(np.sqrt(np.float32(cloud_len))))
        return SortedEntries.new(camera_count, side * side)

    def chunk(self, camera_index: int, gaussians: Optional[int] = None) -> np.ndarray:
        g = self.entry_count if gaussians is None else int(gaussians)
        if camera_index < 0 or (camera_index + 1) * g > self.sorted.shape[0]:
            raise IndexError("camera chunk out of range")  # `.nth(camera_index).unwrap()` panics
        return self.sorted[camera_index * g : (camera_index + 1) * g]

    def resized(self, camera_count: int) -> "SortedEntries":
        """`update_sorted_entries_sizes` (src/sort/mod.rs:270-296): a camera-count change re-creates
        the asset (all chunks back to key 1 / identity order)."""
        return self if camera_count == self.camera_count else SortedEntries.new(camera_count, self.entry_count)


@dataclass
class DeviceEntriesChunk:
    """One camera's chunk of a `DeviceSortedEntries`: `count` (key, index) records at the device address `ptr`
    (`bgs_view.entries_device_ptr` / `entry_count`)."""

    ptr: int
    count: int


class DeviceSortedEntries:
    """`SortedEntries` resident on the device: `camera_count` chunks of `gaussians` = cloud.len() entries each in ONE
    `bgs_device_alloc` block, camera `c` at byte offset `c * 8 * gaussians` — the dynamic offset the reference's draw binds
    (src/render/mod.rs:1548-1554). `sort(..., into=chunk)` fills a chunk, `render(..., entries=chunk)` draws it as it is.
    New chunks hold the asset's initial content (`initial_entries`). The caller orders a sort into a chunk against frames
    in flight that read it (`bgs_sort` completes the frames in flight first)."""

    ENTRY_BYTES = 8

    def __init__(self, plugin: "GaussianSplattingPlugin", camera_count: int, gaussians: int):
        if camera_count < 1 or gaussians < 0:
            raise ValueError("camera_count must be >= 1 and gaussians >= 0")
        self._plugin = plugin
        self.camera_count = int(camera_count)
        self.gaussians = int(gaussians)
        self._block = DeviceBlock.allocate(plugin, max(self.nbytes, self.ENTRY_BYTES), initial_entries(self.camera_count, self.gaussians))

    @property
    def ptr(self) -> Optional[int]:     # the block's address; None once it is freed
        return self._block.ptr or None

    @staticmethod
    def chunk_offset(camera_index: int, gaussians: int) -> int:
        """Byte offset of camera `camera_index`'s chunk: `camera_index * 8 * gaussians` (always a multiple of 8)."""
        return int(camera_index) * DeviceSortedEntries.ENTRY_BYTES * int(gaussians)

    @property
    def nbytes(self) -> int:
        return self.chunk_offset(self.camera_count, self.gaussians)

    def chunk(self, camera_index: int) -> DeviceEntriesChunk:
        if self.ptr is None:
            raise ValueError("the entries have been freed")
        if camera_index < 0 or camera_index >= self.camera_count:
            raise IndexError("camera chunk out of range")  # `.nth(camera_index).unwrap()` panics
        return DeviceEntriesChunk(self.ptr + self.chunk_offset(camera_index, self.gaussians), self.gaussians)

    def upload(self, camera_index: int, entries: np.ndarray) -> None:
        """Overwrite a chunk with host entries (hand-built orders; blocking)."""
        e = np.ascontiguousarray(entries, dtype=SORT_ENTRY_DTYPE)
        if e.shape != (self.gaussians,):
            raise ValueError("a chunk holds exactly cloud.len() entries")
        if e.nbytes:
            self._plugin.upload_bytes(self.chunk(camera_index).ptr, e)

    def download(self, camera_index: int) -> np.ndarray:
        """A chunk's entries (completes the frames in flight first; blocking)."""
        out = np.empty(self.gaussians, dtype=SORT_ENTRY_DTYPE)
        self._plugin.synchronize()
        if out.nbytes:
            self._plugin.download(self.chunk(camera_index).ptr, out)
        return out

    def free(self) -> None:
        self._block.free()
