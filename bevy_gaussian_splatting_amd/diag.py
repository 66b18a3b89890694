"""The wrappers of include/bgs_diag.h: test hooks, probes, counters and experiment switches of libbgs.so, kept apart from the
plugin surface that `plugin.GaussianSplattingPlugin` mirrors. The plugin inherits `DiagHooks`, so the tests, `bench.py` and
the scripts call them as `plugin.<name>`; nothing here is needed to sort or render."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native
from .camera import View
from .entries import SORT_ENTRY_DTYPE
from .settings import CloudSettings


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _uptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class DiagHooks:
    """What `GaussianSplattingPlugin` inherits: it provides `_lib`, `_ctx` and `_check`."""

    def _sizes_then_data(self, name: str, sizes: tuple, data, frame) -> None:
        """The two calls of a read-back of the last frame: `name(ctx, *sizes)` for the sizes only, then `name(ctx, *data())`
        with buffers `data` makes of those sizes. `frame()` reads, from the hook's info struct, what names the frame: it must
        be the same after either call."""
        call = getattr(self._lib, name)
        self._check(call(self._ctx, *sizes))
        seen = frame()
        self._check(call(self._ctx, *data()))
        if frame() != seen:
            raise RuntimeError(f"the frame changed between the two calls of {name}")

    def radix_sort_pairs(self, keys: np.ndarray, passes: int = 4) -> np.ndarray:
        """Run the device Onesweep kernel on arbitrary (key, index=i) pairs (test hook)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        e = np.empty(keys.shape[0], dtype=SORT_ENTRY_DTYPE)
        e["key"] = keys
        e["index"] = np.arange(keys.shape[0], dtype=np.uint32)
        self._check(
            self._lib.bgs_radix_sort_pairs(
                self._ctx, e.ctypes.data_as(ctypes.POINTER(_native.BgsSortEntry)),
                keys.shape[0], int(passes)))
        return e

    def hbm_probe(self, nbytes: int = 1 << 29, iters: int = 20):
        """Measured HBM ceiling: (DtoD-copy GB/s counting read+write, triad GB/s) — for the roofline."""
        c, t = ctypes.c_float(), ctypes.c_float()
        self._check(self._lib.bgs_hbm_probe(self._ctx, int(nbytes), int(iters), ctypes.byref(c), ctypes.byref(t)))
        return float(c.value), float(t.value)

    def selftest_ln(self, first_bits: int, count: int, download: Optional[bool] = None):
        """`bgs_selftest_ln_f32`: the correctly rounded ln of the adaptive cutoff evaluated ON THE DEVICE for the
        binary32 bit patterns first_bits .. first_bits + count - 1. Returns (results or None, checksum); the results
        are downloaded for count <= 2^24 unless `download` says otherwise."""
        if download is None:
            download = count <= (1 << 24)
        out = np.empty(count, np.float32) if download else None
        chk = ctypes.c_uint64()
        self._check(self._lib.bgs_selftest_ln_f32(
            self._ctx, int(first_bits), int(count),
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if download else None, ctypes.byref(chk)))
        return out, int(chk.value)

    def selftest_pack(self, fmt: str, device_in: int, pixels: int, device_out: int) -> None:
        """`bgs_selftest_pack`: the packed outputs' conversion (encode_srgb8_kernel) of `pixels` RGBA f32 pixels at the
        device address `device_in` into `device_out` (4 bytes per pixel for fmt "srgb8", 8 for "rgba16f"; an int is
        passed as the bgs_pack_format as it is). The caller's writes to the input must be complete (e.g.
        torch.cuda.synchronize()); returns once the output is written."""
        code = fmt if isinstance(fmt, int) else {"srgb8": 1, "rgba16f": 2}[fmt]   # BGS_PACK_SRGB8 / BGS_PACK_RGBA16F
        self._check(self._lib.bgs_selftest_pack(self._ctx, code, device_in or None, int(pixels), device_out or None))

    def debug_frame_records(self) -> dict:
        """`bgs_debug_frame_records`: what the vertex stage of the last synchronous `render` left on the device, as it is:
        `records` uint32[draw_count, stride / 4] (12 words: Record, 24: RecordSurfel; front-to-back rank order), `rects`
        uint32[draw_count] (scan binning; None otherwise), and `draw_count`, `record_stride`, `visible_count`,
        `color_max_bits`. Test hook; raises when there is no such frame (see include/bgs_diag.h)."""
        info, out = _native.BgsFrameRecordsInfo(), {}

        def data():
            count = int(info.draw_count)
            out.update(records=np.zeros((count, int(info.record_stride) // 4), np.uint32), rects=np.zeros(count, np.uint32))
            return out["records"].ctypes.data_as(ctypes.c_void_p), out["records"].nbytes, _uptr(out["rects"]), count, ctypes.byref(info)

        self._sizes_then_data("bgs_debug_frame_records", (None, 0, None, 0, ctypes.byref(info)), data, lambda: int(info.draw_count))
        return {"draw_count": int(info.draw_count), "record_stride": int(info.record_stride), "records": out["records"],
                "rects": out["rects"] if info.has_rects else None, "visible_count": int(info.visible_count),
                "color_max_bits": int(info.color_max_bits)}

    def selftest_bin(self, rects: np.ndarray, tiles_x: int, tiles_y: int, sup_edge: int, coarse_cap: int, wide: int, blocks: int) -> dict:
        """`bgs_selftest_bin`: bin_kernel alone on packed tile rectangles (uint32[n]). `lists` uint32[supertiles, coarse_cap,
        2] (rank, rectangle; what the kernel did not write holds 0xFFFFFFFF), `guard` uint32[64, 2] (the entries behind the
        last list), `totals` uint32[256] and `error` (Control::error). Test hook (see include/bgs_diag.h)."""
        r = np.ascontiguousarray(rects, dtype=np.uint32)
        num_st = max(-(-int(tiles_x) // max(int(sup_edge), 1)) * -(-int(tiles_y) // max(int(sup_edge), 1)), 0)
        entries = num_st * max(int(coarse_cap), 0) + _native.SELFTEST_BIN_GUARD
        lists = np.zeros((entries, 2), np.uint32)
        totals = np.zeros(256, np.uint32)
        err = ctypes.c_uint32()
        self._check(self._lib.bgs_selftest_bin(self._ctx, _uptr(r), r.size, int(tiles_x), int(tiles_y), int(sup_edge), int(coarse_cap),
                                               int(wide), int(blocks), _uptr(lists), lists.size, _uptr(totals), ctypes.byref(err)))
        body = entries - _native.SELFTEST_BIN_GUARD
        return {"lists": lists[:body].reshape(num_st, int(coarse_cap), 2), "guard": lists[body:], "totals": totals, "error": int(err.value)}

    def debug_frame_lists(self) -> dict:
        """`bgs_debug_frame_lists`: what the binning stage of the last synchronous `render` left on the device, at any
        pipeline depth. Scan binning: `sup_edge`, `sup_x`, `sup_y`, `level`, `coarse_cap`, `wide_bin`, `totals`
        uint32[supertiles] and `lists`, one uint32[min(total, coarse_cap), 2] (rank, rectangle) per supertile. Sort
        binning: `instance_count`, `instances` uint32[instance_count, 2] (tile id, rank) and `ranges` uint32[65536, 2].
        Both: `binning` ("scan" / "sort") and `draw_count`. Test hook; raises when there is no such frame."""
        info, bufs = _native.BgsFrameListsInfo(), {}
        ranges = np.zeros((65536, 2), np.uint32)

        def data():
            count, num_st = int(info.entry_count), int(info.sup_x) * int(info.sup_y)
            bufs.update(totals=np.zeros(max(num_st, 1), np.uint32), entries=np.zeros((max(count, 1), 2), np.uint32))
            return (_uptr(bufs["totals"]), num_st if int(info.binning) == 0 else 0, _uptr(bufs["entries"]), 2 * count, _uptr(ranges), ranges.size,
                    ctypes.byref(info))

        self._sizes_then_data("bgs_debug_frame_lists", (None, 0, None, 0, None, 0, ctypes.byref(info)), data, lambda: int(info.entry_count))
        count, scan, num_st = int(info.entry_count), int(info.binning) == 0, int(info.sup_x) * int(info.sup_y)
        totals, entries = bufs["totals"], bufs["entries"]
        out = {"binning": "scan" if scan else "sort", "draw_count": int(info.draw_count)}
        if scan:
            cap = int(info.coarse_cap)
            totals = totals[:num_st]
            ends = np.cumsum(np.minimum(totals, cap).astype(np.int64))
            out.update(sup_edge=int(info.sup_edge), sup_x=int(info.sup_x), sup_y=int(info.sup_y), level=int(info.level), coarse_cap=cap,
                       wide_bin=int(info.wide_bin), totals=totals,
                       lists=[entries[int(e) - int(min(t, cap)):int(e)] for e, t in zip(ends, totals)])
        else:
            out.update(instance_count=int(info.instance_count), instances=entries[:count], ranges=ranges)
        return out

    def debug_frame_leftovers(self) -> dict:
        """`bgs_debug_frame_leftovers`: what lane 0's last completed `render` left for the frame behind it, at any pipeline
        depth. `scratch` uint32[layout.bytes / 4] (the lane's whole scratch region), `layout` (a BgsScratchLayout),
        `control` uint32[control_bytes / 4] (the lane's pinned host Control) and every field of bgs_frame_leftovers_info by
        its name (`dirty_words`, `ctl_block`, `scratch_clean`, ...). A read-back that finds dirty words under a clean flag
        takes the flag back (`scratch_reset`). Test hook; raises when there is no such frame (see include/bgs_diag.h)."""
        info, layout, first, out = _native.BgsFrameLeftoversInfo(), _native.BgsScratchLayout(), {}, {}

        def data():
            # (the first call is the one that saw the lane's flag as the frame left it: it may have taken it back)
            first.update({name: int(getattr(info, name)) for name, _ in info._fields_})
            out.update(scratch=np.zeros(int(layout.bytes) // 4, np.uint32), control=np.zeros(int(info.control_bytes) // 4, np.uint32))
            return (out["scratch"].ctypes.data_as(ctypes.c_void_p), out["scratch"].nbytes, out["control"].ctypes.data_as(ctypes.c_void_p),
                    out["control"].nbytes, ctypes.byref(layout), ctypes.byref(info))

        self._sizes_then_data("bgs_debug_frame_leftovers", (None, 0, None, 0, ctypes.byref(layout), ctypes.byref(info)), data,
                              lambda: (int(layout.bytes), int(info.dirty_words)))
        return dict(first, scratch=out["scratch"], layout=layout, control=out["control"])

    def selftest_bucket_sort(self, sub: int, wide: int, key_xor: int, counts: np.ndarray, pairs: np.ndarray) -> dict:
        """`bgs_selftest_bucket_sort`: bucket_sort_kernel alone on `counts` uint32[256 * sub] (Control::bucket_count) and
        `pairs` uint32[n, 2] (key, index; bucket after bucket, min(count, capacity) of each, in arrival order). `out`
        uint32[n, 2] (key ^ key_xor, index; what the kernel did not write holds 0xFFFFFFFF), `guard` uint32[64, 2] (the
        entries behind the list), `draw_count`, `sort_overflow`, `bucket_max`. Test hook (see include/bgs_diag.h)."""
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        p = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        n = p.shape[0]
        out = np.zeros((n + _native.SELFTEST_BUCKET_GUARD, 2), np.uint32)
        info = np.zeros(3, np.uint32)
        if 1 <= int(sub) <= 16 and c.size != 256 * int(sub):   # (any other sub is the library's to refuse)
            raise ValueError("counts holds one word per bucket: 256 * sub")
        self._check(self._lib.bgs_selftest_bucket_sort(self._ctx, int(sub), int(wide), int(key_xor) & 0xFFFFFFFF, _uptr(c), _uptr(p), n,
                                                       _uptr(out), out.size, _uptr(info)))
        return {"out": out[:n], "guard": out[n:], "draw_count": int(info[0]), "sort_overflow": int(info[1]), "bucket_max": int(info[2])}

    def selftest_keygen_buckets(self, handle: PlanarGaussian3dHandle, view: View, settings: CloudSettings, splitters: np.ndarray,
                                sub: int, wide_buckets: int = 0, ordered: int = 0, alone: int = 0) -> dict:
        """`bgs_selftest_keygen_buckets`: keygen's bucket placement alone with the table `splitters` uint32[256 * sub - 1]
        (keygen's key space, ascending). `counts` uint32[256 * sub], `slots` uint32[256 * sub, capacity, 2] (key, index;
        unwritten slots hold 0xFFFFFFFF), `culled` uint32[n, 2] (ordered only, else None), `draw_count`, `splat_count`,
        `error`, `threads`, `blocks`. Test hook (see include/bgs_diag.h)."""
        t = np.ascontiguousarray(splitters, dtype=np.uint32)
        nb = 256 * min(max(int(sub), 1), 16)   # (a sub outside 1 .. 16 is the library's to refuse)
        if 1 <= int(sub) <= 16 and t.size != nb - 1:
            raise ValueError("splitters holds 256 * sub - 1 keys")
        cap = 16384 if int(wide_buckets) == 1 else 4096
        counts = np.zeros(nb, np.uint32)
        slots = np.zeros((nb, cap, 2), np.uint32)
        culled = np.zeros((handle.n, 2), np.uint32) if int(ordered) == 1 else None
        info = np.zeros(5, np.uint32)
        v, s = view.to_native(), settings.to_native()
        self._check(self._lib.bgs_selftest_keygen_buckets(self._ctx, handle._ptr, ctypes.byref(v), ctypes.byref(s), _uptr(t), int(sub),
                                                          int(wide_buckets), int(ordered), int(alone), _uptr(counts), _uptr(slots), slots.size,
                                                          _uptr(culled) if culled is not None else None,
                                                          culled.size if culled is not None else 0, _uptr(info)))
        return {"counts": counts, "slots": slots, "culled": culled, "draw_count": int(info[0]), "splat_count": int(info[1]),
                "error": int(info[2]), "threads": int(info[3]), "blocks": int(info[4])}

    def selftest_raster(self, width: int, height: int, sample_count: int, variant: int, records: np.ndarray, lists: np.ndarray,
                        totals: np.ndarray, sup_edge: int, coarse_cap: int, mode: int = 0, overlay: int = 0,
                        clear=(0.0, 0.0, 0.0, 0.0), color_max_bits: int = 0, viewport=None, depth: Optional[np.ndarray] = None,
                        heavy_tiles: Optional[np.ndarray] = None, order: Optional[np.ndarray] = None) -> dict:
        """`bgs_selftest_raster`: both tile rasterisers alone on `records` uint32 / float32 [n, 12] (variant 0 OBB, 1 AABB3D)
        or [n, 24] (2 surfel), the supertile `lists` uint32[supertiles, coarse_cap, 2] (rank, packed rectangle) and `totals`
        uint32[supertiles]; `depth` float32[height, width, sample_count], `heavy_tiles` and `order` uint16 or None. `scan` and
        `sort` float32[height, width, 4] (the two images), `scan_guard` / `sort_guard` uint32[64, 4] (the pixels behind each,
        filled with 0xFF bytes before the launch), `cost` uint16[tiles], `heavy_count`, `heavy_list`, `heavy_flags` (the
        scan rasteriser's heavy_out) and `error` (Control::error). Test hook (see include/bgs_diag.h)."""
        w, h, ms = int(width), int(height), int(sample_count)
        rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 24 if int(variant) == 2 else 12)
        li = np.ascontiguousarray(lists, dtype=np.uint32)
        to = np.ascontiguousarray(totals, dtype=np.uint32)
        tiles = max(-(-w // 16) * -(-h // 16), 0)
        edge = max(int(sup_edge), 1)
        num_st = -(-(-(-w // 16)) // edge) * -(-(-(-h // 16)) // edge)
        if 1 <= w <= 512 and 1 <= h <= 512 and 1 <= int(sup_edge) <= 32 and int(coarse_cap) >= 1:   # (anything else is the library's to refuse)
            if li.size != num_st * int(coarse_cap) * 2 or to.size != num_st:
                raise ValueError("lists holds supertiles x coarse_cap entries of two words, totals one word per supertile")
        arg = _native.BgsRasterSelftest()
        arg.width, arg.height, arg.sample_count, arg.variant, arg.overlay, arg.mode = w, h, ms, int(variant), int(overlay), int(mode)
        arg.sup_edge, arg.coarse_cap, arg.color_max_bits, arg.record_count = int(sup_edge), int(coarse_cap), int(color_max_bits) & 0xFFFFFFFF, rec.shape[0]
        vw, vh = viewport if viewport is not None else (float(w), float(h))
        arg.viewport_w, arg.viewport_h = float(vw), float(vh)
        arg.clear[:] = [float(c) for c in clear]
        keep = [rec, li, to]
        arg.records, arg.lists, arg.totals = rec.ctypes.data, li.ctypes.data, to.ctypes.data
        if depth is not None:
            d = np.ascontiguousarray(depth, dtype=np.float32)
            if d.size != w * h * ms:
                raise ValueError("depth holds width x height x sample_count floats")
            keep.append(d)
            arg.depth = d.ctypes.data
        if heavy_tiles is not None:
            hv = np.ascontiguousarray(heavy_tiles, dtype=np.uint16)
            keep.append(hv)
            arg.heavy_tiles, arg.heavy_count = hv.ctypes.data, hv.size
        if order is not None:
            od = np.ascontiguousarray(order, dtype=np.uint16)
            if od.size != (tiles + 3) // 4:
                raise ValueError("order holds one entry per raster workgroup: (tiles + 3) // 4")
            keep.append(od)
            arg.order = od.ctypes.data
        pixels = max(w * h, 0)
        scan = np.zeros((pixels + _native.SELFTEST_RASTER_GUARD, 4), np.float32)
        sort = np.zeros_like(scan)
        cost = np.zeros(max(tiles, 1), np.uint16)
        heavy = np.zeros(_native.HEAVY_FLAGS_OFFSET + tiles, np.uint8)
        err = ctypes.c_uint32()
        self._check(self._lib.bgs_selftest_raster(self._ctx, ctypes.byref(arg), scan.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                  sort.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), scan.size,
                                                  cost.ctypes.data_as(ctypes.c_void_p), heavy.ctypes.data_as(ctypes.c_void_p), heavy.size,
                                                  ctypes.byref(err)))
        count = int(heavy[:4].view(np.uint32)[0])
        return {"scan": scan[:pixels].reshape(h, w, 4), "sort": sort[:pixels].reshape(h, w, 4),
                "scan_guard": scan[pixels:].view(np.uint32), "sort_guard": sort[pixels:].view(np.uint32), "cost": cost[:tiles],
                "heavy_count": count,
                "heavy_list": heavy[_native.HEAVY_LIST_OFFSET:_native.HEAVY_FLAGS_OFFSET].view(np.uint16)[:min(count, _native.HEAVY_CAP)].copy(),
                "heavy_flags": heavy[_native.HEAVY_FLAGS_OFFSET:],
                "error": int(err.value)}

    def graph_counters(self) -> tuple:
        """(frames captured into a graph, frames replayed from one) since the plugin was created."""
        c, r = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.bgs_graph_counters(self._ctx, ctypes.byref(c), ctypes.byref(r)))
        return int(c.value), int(r.value)

    def tile_order_counters(self) -> tuple:
        """(frames that left per-tile costs, frames whose raster workgroups ran in cost order, times that order was made
        anew) since the plugin was created."""
        c, r, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.bgs_tile_order_counters(self._ctx, ctypes.byref(c), ctypes.byref(r), ctypes.byref(n)))
        return int(c.value), int(r.value), int(n.value)

    def selftest_tile_order(self, cost: np.ndarray, runs: int = 1, sums: bool = False):
        """`bgs_selftest_tile_order`: the raster workgroups' order tile_order_kernel makes of per-tile costs (uint16,
        one per tile): uint16[(tiles + 3) // 4] — with `sums` also (work of all tiles, work of the tiles with bit 15 set)."""
        c = np.ascontiguousarray(cost, dtype=np.uint16)
        out = np.empty((c.size + 3) // 4, np.uint16)
        two = np.zeros(2, np.uint32)
        self._check(self._lib.bgs_selftest_tile_order(self._ctx, c.ctypes.data_as(ctypes.c_void_p), c.size, runs,
                                                      out.ctypes.data_as(ctypes.c_void_p), two.ctypes.data_as(ctypes.c_void_p)))
        return (out, (int(two[0]), int(two[1]))) if sums else out

    def set_debug_flags(self, flags: int) -> None:
        """Kernel-ablation switches for experiments only (non-zero => wrong images)."""
        self._check(self._lib.bgs_set_debug_flags(self._ctx, int(flags)))

    def set_grid_cap(self, blocks: int) -> None:
        """`bgs_set_grid_cap`: every persistent launch of the context with at most `blocks` workgroups (1 .. 4096), so that
        a small frame walks the kernels' tile loops several times; 0 (default) = the grids as they are. Test hook."""
        self._check(self._lib.bgs_set_grid_cap(self._ctx, int(blocks)))

    def debug_frame_grids(self) -> dict:
        """`bgs_debug_frame_grids`: per persistent kernel of the last completed frame (or of a `radix_sort_pairs` since)
        `(workgroups launched, tiles of work)` under "front", "depth", "project", "bin", "tile_sort" — `(0, 0)` for a kernel
        the frame did not launch —, the `cap` the launches ran under, `front_chainless` (the keygen that is never capped), and
        `tail_ptr` / `tail_count`: the device list of culled / skipped entries the front kernel left (0, 0: none)."""
        out = np.zeros(_native.FRAME_GRIDS_WORDS, np.uint32)
        self._check(self._lib.bgs_debug_frame_grids(self._ctx, _uptr(out), out.size))
        grids = {name: (int(out[2 * k]), int(out[2 * k + 1])) for k, name in enumerate(_native.GRID_KERNELS)}
        grids.update(cap=int(out[10]), front_chainless=bool(out[11]), tail_ptr=int(out[12]) | (int(out[13]) << 32), tail_count=int(out[14]))
        return grids

    def set_tile_trace(self, device_ptr: Optional[int]) -> None:
        """`bgs_set_tile_trace`: per-tile timing / placement trace of the rasteriser into a caller-owned device buffer
        (tiles_x * tiles_y * 32 bytes); None switches it off."""
        self._check(self._lib.bgs_set_tile_trace(self._ctx, ctypes.c_void_p(device_ptr or 0)))

    def adaptive_counters(self) -> dict:
        """Cumulative counters of the adaptive machinery (bgs_adaptive_counters)."""
        out = (ctypes.c_uint64 * 8)()
        self._check(self._lib.bgs_adaptive_counters(self._ctx, out))
        names = ("bucket_frames", "onesweep_frames", "reruns_sort", "reruns_lists", "reruns_instances",
                 "level_changes", "supertile_level", "list_capacity_hint")
        return {k: int(v) for k, v in zip(names, out)}

    def learning_counters(self) -> dict:
        """Async frames completed inside their render call because their kind of frame was new to the context, and the
        kinds it has settled on (bgs_learning_counters)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.bgs_learning_counters(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return {"early_frames": a.value, "kinds_settled": b.value}
