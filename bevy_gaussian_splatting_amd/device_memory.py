"""`DeviceBlock`: the one owner, on the Python side, of a block from `bgs_device_alloc`. Whatever keeps such a block (the
device entries, the particle behaviours, the resident producers, the selections' scratch) frees through one, so "free
once, and not after the plugin is closed" is written here only. `device_alloc` / `device_free` remain the raw pair."""
from __future__ import annotations


class DeviceBlock:
    """`nbytes` of device memory at `ptr`, owned: `free()` releases it once, and makes no library call once the plugin
    is closed (`bgs_destroy` has released the context's memory). `ptr` is 0 afterwards. As a context manager it frees on
    exit. `plugin` is anything with `_ctx`, `device_alloc`, `device_free` and `upload_bytes`."""

    def __init__(self, plugin, ptr: int, nbytes: int):
        self._plugin, self.ptr, self.nbytes = plugin, int(ptr), int(nbytes)

    @classmethod
    def allocate(cls, plugin, nbytes: int, init=None) -> "DeviceBlock":
        """A new block, holding `init` (a contiguous array; blocking upload) if one is given and it is not empty. If the
        upload raises, the block is freed and the exception goes on."""
        block = cls(plugin, plugin.device_alloc(nbytes), nbytes)
        if init is not None and init.nbytes:
            try:
                plugin.upload_bytes(block.ptr, init)
            except BaseException:
                block.free()
                raise
        return block

    def release(self) -> int:
        """Hand the block over to the caller, who frees the address with `device_free`: the owner forgets it."""
        ptr, self.ptr = self.ptr, 0
        return ptr

    def free(self) -> None:
        ptr = self.release()
        if ptr and self._plugin._ctx is not None:
            self._plugin.device_free(ptr)   # (completes the frames in flight first)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
