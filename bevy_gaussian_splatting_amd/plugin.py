"""Host-side mirror of the reference's plugin surface for the sort + rasterize path.

Reference call sites this stands behind:
  - cloud upload: RenderAsset upload of the planar cloud (src/lib.rs:65-68,
    src/render/mod.rs:279-313)                               -> `upload`
  - sort: `run_radix_sort` (src/sort/radix.rs:616-756) / `rayon_sort`
    (src/sort/rayon.rs:27-130), output `SortedEntries` (src/sort/mod.rs:331-393) -> `sort`
  - draw: `DrawGaussianInstanced::render` (src/render/mod.rs:1513-1569)   -> `render`

All compute happens in libbgs.so (hand-written HIP for gfx950). This module only marshals
arguments; it has no CPU implementation of any stage. The sorted entries are `entries.py`, the owner of a
`bgs_device_alloc` block is `device_memory.py`, `MorphPair` and `ResidentCloud4d` are `resident.py`; their names are exported here too.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from . import _native
from .camera import View, color_attachment_offset
from .device_memory import DeviceBlock
from .diag import DiagHooks, _fptr
from .entries import SORT_ENTRY_DTYPE, DeviceEntriesChunk, DeviceSortedEntries, SortedEntries  # noqa: F401
from .gaussian import PlanarGaussian3d, PlanarGaussian3dF16, PlanarGaussian4d
from .interpolate import covariance_planes
from .particles import PARTICLE_BEHAVIOR_DTYPE, ParticleBehaviors, ParticleBehaviorsHandle
from .resident import MorphPair, ResidentCloud4d
from .settings import CloudSettings
from .sparse_select import SparseSelect, selected_indices


def _with_entries(v, chunk):
    """A copy of the native view `v` that names `chunk` (the caller's struct — a PreparedView's — stays as it is)."""
    if chunk is None:
        return v
    v = type(v).from_buffer_copy(v)
    v.entries_device_ptr = int(chunk.ptr)
    v.entry_count = int(chunk.count)
    return v


@dataclass
class PreparedView:
    """C-struct images of one (View, CloudSettings) pair (GaussianSplattingPlugin.prepare)."""

    view: object
    settings: object
    width: int
    height: int


class PlanarGaussian3dHandle:
    """Device-resident cloud (the reference's `PlanarGaussian3dHandle` +
    `GpuPlanarStorage` rolled into one opaque handle)."""

    def __init__(self, plugin: "GaussianSplattingPlugin", ptr, n: int, fmt: str, nbytes: int):
        self._plugin = plugin
        self._ptr = ptr
        self.n = n
        self.format = fmt
        self.nbytes = nbytes

    def __len__(self) -> int:
        return self.n

    def free(self) -> None:
        if self._ptr is not None and self._plugin._ctx is not None:
            self._plugin._lib.bgs_cloud_free(self._plugin._ctx, self._ptr)
        self._ptr = None


# The three cloud uploads by format: the C entry point, its planes in the order of its arguments, and the bytes of a splat.
DEVICE_PLANE_FORMATS = {
    "f32": ("bgs_cloud_upload_f32", ("position_visibility", "spherical_harmonic", "rotation", "scale_opacity"), 16 + 192 + 16 + 16),
    "f16": ("bgs_cloud_upload_f16", ("position_visibility", "spherical_harmonic_h2", "rotation_scale_opacity"), 16 + 96 + 16),
    "cov3d": ("bgs_cloud_upload_cov3d_f32", ("position_visibility", "spherical_harmonic", "covariance_3d_opacity"), 16 + 192 + 32),
}
# ... and the type of each plane's argument, by plane: float rows, but for the two planes of packed halves (uint32 words)
PLANE_POINTER_TYPES = {name: ctypes.POINTER(ctypes.c_uint32 if name in ("spherical_harmonic_h2", "rotation_scale_opacity") else
                                            ctypes.c_float) for _, names, _ in DEVICE_PLANE_FORMATS.values() for name in names}


class GaussianSplattingPlugin(DiagHooks):
    """One instance = one HIP device + one stream (`bgs_ctx`). Not re-entrant, like a Bevy
    render world. Use one instance per GPU / per process rank. The wrappers of include/bgs_diag.h's test hooks, probes and
    counters are inherited (`diag.DiagHooks`): they are not part of the plugin surface this class mirrors."""

    def __init__(self, device: int = 0):
        self._lib = _native.load()
        ctx = ctypes.c_void_p()
        _native.check(self._lib, None, self._lib.bgs_create(int(device), ctypes.byref(ctx)))
        self._ctx = ctx
        self.device = device

    # -- lifecycle -------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None:
            self._lib.bgs_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status: int) -> None:
        _native.check(self._lib, self._ctx, status)

    # -- cloud upload ----------------------------------------------------------------
    def upload(self, cloud: Union[PlanarGaussian3d, PlanarGaussian3dF16], precompute_covariance_3d: bool = False) -> PlanarGaussian3dHandle:
        """Make the cloud resident in HBM (the reference's asset upload). `precompute_covariance_3d`: store
        the `Covariance3dOpacity` plane (src/gaussian/f32.rs:218-251) instead of rotation and scale, as the
        reference's feature of that name does; the vertex stage then skips compute_cov3d."""
        if precompute_covariance_3d:
            if not isinstance(cloud, PlanarGaussian3d):
                raise TypeError("precompute_covariance_3d needs an f32 PlanarGaussian3d")
            fmt, planes = "cov3d", covariance_planes(cloud)
        elif isinstance(cloud, PlanarGaussian3dF16):
            fmt, planes = "f16", (cloud.position_visibility, cloud.spherical_harmonic, cloud.rotation_scale_opacity)
        elif isinstance(cloud, PlanarGaussian3d):
            fmt, planes = "f32", (cloud.position_visibility, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity)
        else:
            raise TypeError("cloud must be PlanarGaussian3d or PlanarGaussian3dF16")
        return self._upload_host_planes(fmt, len(cloud), planes)

    def _upload_cloud(self, fmt: str, n: int, args) -> PlanarGaussian3dHandle:
        """The one call of a cloud upload: `fmt`'s entry point over `args`, its planes as ctypes pointers in the order of
        `DEVICE_PLANE_FORMATS`; the handle carries the format and the bytes of `n` splats in it."""
        entry, _, splat_bytes = DEVICE_PLANE_FORMATS[fmt]
        out = ctypes.c_void_p()
        self._check(getattr(self._lib, entry)(self._ctx, n, *args, ctypes.byref(out)))
        return PlanarGaussian3dHandle(self, out, n, fmt, n * splat_bytes)

    def _upload_host_planes(self, fmt: str, n: int, planes) -> PlanarGaussian3dHandle:
        """`_upload_cloud` of contiguous host arrays (`planes` keeps them alive across the call)."""
        names = DEVICE_PLANE_FORMATS[fmt][1]
        return self._upload_cloud(fmt, n, [a.ctypes.data_as(PLANE_POINTER_TYPES[name]) for a, name in zip(planes, names)])

    def upload_covariance_planes(self, position_visibility, spherical_harmonic, covariance_3d_opacity) -> PlanarGaussian3dHandle:
        """The sibling of `upload(..., precompute_covariance_3d=True)` for a covariance plane that is already made:
        [n, 4], [n, 48] and [n, 8] float32 (`Covariance3dOpacity`: xx, xy, xz, yy, yz, zz, opacity, pad) go up as they
        are (`bgs_cloud_upload_cov3d_f32`). Returns a handle of format "cov3d"."""
        pv, sh, cov = (np.ascontiguousarray(a, np.float32) for a in (position_visibility, spherical_harmonic, covariance_3d_opacity))
        n = pv.shape[0]
        if pv.shape != (n, 4) or sh.shape != (n, 48) or cov.shape != (n, 8):
            raise ValueError("expected planes of shape [n, 4], [n, 48] and [n, 8]")
        return self._upload_host_planes("cov3d", n, (pv, sh, cov))

    def upload_device_planes(self, fmt: str, n: int, pointers) -> PlanarGaussian3dHandle:
        """A resident cloud of `n` splats from planes that are in device memory already (include/bgs.h "DEVICE PLANES"):
        `fmt` is "f32", "f16" or "cov3d", `pointers` the planes' addresses as integers in the order of that format's C
        entry point (`DEVICE_PLANE_FORMATS`). Each is device memory of this plugin's device, 16-byte aligned; the work
        that writes it is complete or was enqueued on `stream_handle()` before this call, and no `synchronize()` is
        needed in between. Returns once the cloud is complete: the planes are the caller's again, and unchanged. The
        entry points take host addresses as well, plane by plane, so the planes may be mixed."""
        if fmt not in DEVICE_PLANE_FORMATS:
            raise ValueError(f"fmt must be one of {sorted(DEVICE_PLANE_FORMATS)}, not {fmt!r}")
        entry, names, _ = DEVICE_PLANE_FORMATS[fmt]
        pointers = [int(p or 0) for p in pointers]
        if len(pointers) != len(names):
            raise ValueError(f"{entry} takes {len(names)} planes ({', '.join(names)}), got {len(pointers)} pointers")
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        return self._upload_cloud(fmt, n, [ctypes.cast(ctypes.c_void_p(p), PLANE_POINTER_TYPES[name]) for p, name in zip(pointers, names)])

    # -- 4D clouds (src/render/gaussian_4d.wgsl; libbgs_slice.so) ----------------------
    def resident_4d(self, cloud4d: PlanarGaussian4d, slicer=None) -> "ResidentCloud4d":
        """The five planes of a 4D cloud made resident once, with room for its slice: a `ResidentCloud4d` whose
        `.at(settings)` does only the slice and the upload from the slice's device planes. A host that plays the cloud
        uploads it once and calls `playback_update` then `.at` per frame. Free it (`.free()`, or use it as a context
        manager) when the playback ends."""
        return ResidentCloud4d(self, cloud4d, slicer)

    def slice_4d(self, cloud4d: PlanarGaussian4d, settings: CloudSettings, slicer=None, return_planes: bool = False):
        """The 4D cloud at `settings.time` as a resident 3D cloud of format "cov3d", in one shot: the five planes go
        into device memory, `bgst_slice` runs on `bgs_stream` (`time_slice.TimeSlicer`; global_scale, time_start and
        time_stop are read too), and `bgs_cloud_upload_cov3d_f32` packs the cloud from the three device planes of the
        slice (include/bgs_slice.h "ORDERING"). For more than one `time` keep the cloud
        resident (`resident_4d`). Sort and render the handle with any settings of the precomputed-covariance path, which
        reads neither `time` nor `global_scale`; free it before the next time's slice replaces it. With `return_planes`
        also the three planes on the host."""
        with self.resident_4d(cloud4d, slicer) as resident:
            return resident.at(settings, return_planes=return_planes)

    # -- morph between two clouds (src/morph/interpolate.wgsl; libbgs_morph.so) ---------
    def morph_pair(self, lhs: PlanarGaussian3d, rhs: PlanarGaussian3d, precompute_covariance_3d: bool = False,
                   interpolator=None) -> "MorphPair":
        """Both sides of a `GaussianInterpolate` made resident once: a `MorphPair` whose `.at(settings)` does only the
        kernel and the upload from the output's device planes. A host that scrubs `time` uploads each side once. Free it (`.free()`, or
        use it as a context manager) when the morph ends."""
        return MorphPair(self, lhs, rhs, precompute_covariance_3d, interpolator)

    def interpolate(self, lhs: PlanarGaussian3d, rhs: PlanarGaussian3d, settings: CloudSettings,
                    precompute_covariance_3d: bool = False, interpolator=None, return_planes: bool = False):
        """The blend of two clouds of equal length at `settings.time` between `time_start` and `time_stop` as a resident
        cloud (the reference's `GaussianInterpolate { lhs, rhs }`), in one shot: both sides' planes go into device memory,
        `bgsm_interpolate_f32` runs on `bgs_stream` (`interpolate.GaussianInterpolator`), and `bgs_cloud_upload_f32` packs
        the cloud from the output's device planes. With `precompute_covariance_3d` the two clouds' `Covariance3dOpacity`
        planes are blended instead of rotation and scale (`bgsm_interpolate_cov3d_f32`) and the handle is of format
        "cov3d" (include/bgs_morph.h "ORDERING"). For more than one `time` keep the pair
        resident (`morph_pair`). Free the handle before the next time's morph replaces it. With `return_planes` also the
        output's planes on the host."""
        with self.morph_pair(lhs, rhs, precompute_covariance_3d, interpolator) as pair:
            return pair.at(settings, return_planes=return_planes)

    # -- particle behaviours (src/morph/particle.rs) -----------------------------------
    def upload_particle_behaviors(self, behaviors) -> ParticleBehaviorsHandle:
        """Put a behaviours buffer into device memory (`bgs_device_alloc` + `bgs_upload`). `behaviors` is a
        `ParticleBehaviors` (validated against its cloud when it was built) or a bare array of PARTICLE_BEHAVIOR_DTYPE,
        which goes up as it is: the C ABI's precondition (distinct indices of active records) is then the caller's."""
        rec = behaviors.records if isinstance(behaviors, ParticleBehaviors) else np.ascontiguousarray(behaviors)
        if rec.dtype != PARTICLE_BEHAVIOR_DTYPE or rec.ndim != 1:
            raise TypeError("behaviors must be ParticleBehaviors or a 1-D array of PARTICLE_BEHAVIOR_DTYPE")
        return ParticleBehaviorsHandle(self, self.device_block(max(rec.nbytes, 64), rec).release(), rec.shape[0])

    def apply_particle_behaviors(self, handle: PlanarGaussian3dHandle, behaviors: ParticleBehaviorsHandle, dt: float) -> None:
        """One step of the behaviours on the resident cloud (`bgs_cloud_apply_particle_behaviors`): positions (and
        visibility) of the named splats move, velocity and acceleration of the records advance, on the device. Call it
        before the frame's `render`, as the reference runs `run_particle_behaviors` before the prepass. Completes the
        frames in flight (they keep their place in the ring), then only enqueues the step."""
        self._check(self._lib.bgs_cloud_apply_particle_behaviors(
            self._ctx, handle._ptr, ctypes.c_void_p(behaviors.ptr or 0), int(behaviors.count), ctypes.c_float(dt)))

    def download_particle_behaviors(self, behaviors: ParticleBehaviorsHandle) -> np.ndarray:
        """The records as the steps so far left them (`bgs_synchronize`, which completes the frames in flight, then
        `bgs_download`)."""
        out = np.empty(behaviors.count, PARTICLE_BEHAVIOR_DTYPE)
        self.synchronize()
        if out.nbytes:
            self.download(behaviors.ptr, out)
        return out

    # -- point-in-mesh selection (src/query/raycast.rs; libbgs_query.so) ----------------
    def keep_inside_mesh(self, chunk: DeviceEntriesChunk, points_ptr: int, mesh, matrix=None, outside: bool = False,
                         n: Optional[int] = None) -> None:
        """Cull from a kept chunk every entry whose splat lies outside `mesh` (a `mesh_query.MeshQuery`; with `outside`,
        inside it): its key becomes 0xFFFFFFFF, which `render(..., entries=chunk)` skips wherever it stands. `points_ptr`
        is the device address of the cloud's `position_visibility` plane in caller-owned memory (`n` points, default
        `chunk.count`), `matrix` the 4x4 `mesh_query.mesh_from_points` (None = identity). Applies the ordering rule of
        include/bgs_query.h: completes the frames in flight (they may read the chunk), enqueues the two query launches
        on `bgs_stream`, and completes them before it returns."""
        n = int(chunk.count if n is None else n)
        self.synchronize()
        if n == 0 or chunk.count == 0:
            return
        with self.device_block(4 * n) as scratch:
            stream = self.stream_handle()
            mesh.crossings(stream, points_ptr, n, matrix, scratch.ptr)
            mesh.entries_keep(stream, chunk.ptr, chunk.count, scratch.ptr, n, outside=outside)
            self.synchronize()

    # -- sparse-splat selection (src/query/sparse.rs; libbgs_sparse.so) ------------------
    def keep_sparse(self, chunk: DeviceEntriesChunk, points_ptr: int, grid, select: SparseSelect = SparseSelect(),
                    dense: bool = False, n: Optional[int] = None) -> None:
        """Cull from a kept chunk every entry whose splat is not sparse under `select` (fewer than `neighbor_threshold`
        splats within `radius`, itself included); with `dense`, every entry whose splat is: the floaters go. `grid` is a
        `sparse_select.SparseGrid` of capacity >= n, `points_ptr` the device address of the cloud's `position_visibility`
        plane in caller-owned memory (`n` points, default `chunk.count`). The counting stops at `neighbor_threshold`
        neighbours a point, which the predicate cannot tell from more. Applies the ordering rule of include/bgs_sparse.h:
        completes the frames in flight (they may read the chunk), enqueues the launches on `bgs_stream`, and completes
        them before it returns."""
        n = int(chunk.count if n is None else n)
        self.synchronize()
        if n == 0 or chunk.count == 0:
            return
        with self.device_block(4 * n) as scratch:
            stream = self.stream_handle()
            grid.neighbor_counts(stream, points_ptr, n, select.radius, scratch.ptr, cap=select.neighbor_threshold)
            grid.entries_keep(stream, chunk.ptr, chunk.count, scratch.ptr, n, select.neighbor_threshold, dense=dense)
            self.synchronize()

    def sparse_select(self, points_ptr: int, n: int, grid, select: SparseSelect = SparseSelect()) -> np.ndarray:
        """The ascending indices of the sparse splats among the `n` points at `points_ptr` (the reference's
        `Select.indicies` after `SparseSelect::select`), from counts taken on the device and downloaded."""
        n = int(n)
        self.synchronize()
        if n == 0:
            return np.zeros(0, np.uint32)
        with self.device_block(4 * n) as scratch:
            grid.neighbor_counts(self.stream_handle(), points_ptr, n, select.radius, scratch.ptr, cap=select.neighbor_threshold)
            self.synchronize()
            counts = self.download(scratch.ptr, np.empty(n, np.uint32))
        return selected_indices(counts, select.neighbor_threshold)

    # -- hot path --------------------------------------------------------------------
    def sort(self, handle: PlanarGaussian3dHandle, view: View, settings: CloudSettings,
             download: bool = True, into: Optional[DeviceEntriesChunk] = None) -> Optional[np.ndarray]:
        """Depth sort for one camera. Returns the (key, index) entries of this camera's
        chunk in draw order (structured array), or None if `download` is False. `into` (default: `view.entries`): a chunk
        of a `DeviceSortedEntries` that receives the same entries on the device."""
        v, s = _with_entries(view.to_native(), into), settings.to_native()
        if download:
            out = np.empty(handle.n, dtype=SORT_ENTRY_DTYPE)
            ptr = out.ctypes.data_as(ctypes.POINTER(_native.BgsSortEntry))
        else:
            out, ptr = None, None
        self._check(self._lib.bgs_sort(self._ctx, handle._ptr, ctypes.byref(v), ctypes.byref(s), ptr))
        return out

    def sort_cameras(self, handle: PlanarGaussian3dHandle, views, settings: CloudSettings,
                     sorted_entries: Optional[SortedEntries] = None, camera_indices=None) -> SortedEntries:
        """Multi-camera entry layout (src/sort/mod.rs:331-393): depth-sort the cloud for each view and
        store the result in that camera's chunk of one `SortedEntries`. `views[i]` belongs to camera
        index `camera_indices[i]` (default i = `Camera.order`, src/sort/mod.rs:171-176). Unlike the
        reference's GPU radix path, which only ever sorts into chunk 0 (TODO at src/sort/mod.rs:427),
        every camera gets its own order here. Cameras whose trigger does not ask for a sort are simply
        left out of `views`; their chunks keep their previous content."""
        views = list(views)
        idx = list(range(len(views))) if camera_indices is None else [int(i) for i in camera_indices]
        if len(idx) != len(views):
            raise ValueError("camera_indices must match views")
        count = (max(idx) + 1) if idx else 0
        if sorted_entries is None:
            sorted_entries = SortedEntries.for_cloud(count, handle.n)
        if count > sorted_entries.camera_count:
            raise ValueError("sorted_entries has fewer camera chunks than the camera indices need")
        for view, ci in zip(views, idx):
            chunk = sorted_entries.chunk(ci, handle.n)
            chunk[:] = self.sort(handle, view, settings)
        return sorted_entries

    def prepare(self, view: View, settings: CloudSettings) -> "PreparedView":
        """Marshal a (view, settings) pair once (the per-call conversion to the C structs costs ~20 us
        of host time, a fifth of a pipelined frame). Pass the result as `view` with `settings=None`."""
        return PreparedView(view.to_native(), settings.to_native(), view.width, view.height)

    def render(self, handle: PlanarGaussian3dHandle, view, settings: Optional[CloudSettings] = None,
               download: bool = True, entries: Optional[DeviceEntriesChunk] = None) -> Optional[np.ndarray]:
        """Sort + project + bin + rasterize one view. Returns [H, W, 4] float32
        (premultiplied linear RGBA, unclamped, row 0 = top) or None if not downloaded.
        `view` is a View (with `settings`) or a PreparedView from `prepare()`. `entries` (default: `view.entries`): draw
        this chunk of a `DeviceSortedEntries` as it is instead of sorting — the reference's frames between two sorts."""
        if isinstance(view, PreparedView):
            v, s = view.view, view.settings
        else:
            v, s = view.to_native(), settings.to_native()
        v = _with_entries(v, entries)
        if download:
            out = np.empty((view.height, view.width, 4), dtype=np.float32)
            ptr = _fptr(out)
        else:
            out, ptr = None, None
        self._check(self._lib.bgs_render(self._ctx, handle._ptr, ctypes.byref(v), ctypes.byref(s), ptr))
        return out

    def device_sorted_entries(self, camera_count: int, handle: PlanarGaussian3dHandle) -> DeviceSortedEntries:
        """`SortedEntries` for `camera_count` cameras of this cloud, kept on the device."""
        return DeviceSortedEntries(self, camera_count, handle.n)

    def render_with_trigger(self, handle: PlanarGaussian3dHandle, view: View, settings: CloudSettings, trigger,
                            chunk: DeviceEntriesChunk, download: bool = True) -> Optional[np.ndarray]:
        """One frame the way the reference draws it: sort into the camera's chunk iff `trigger.needs_sort`
        (`sort_policy.update_sort_trigger` raised it; it is cleared, as the sort systems do), then draw from the chunk —
        freshly sorted or as the last sort left it."""
        if trigger.needs_sort:
            self.sort(handle, view, settings, download=False, into=chunk)
            trigger.needs_sort = False
        return self.render(handle, view, settings, download=download, entries=chunk)

    def set_pipeline_streams(self, streams: int) -> None:
        """HIP streams the lanes are multiplexed onto (0 = one per lane); see bgs_set_pipeline_streams."""
        self._check(self._lib.bgs_set_pipeline_streams(self._ctx, int(streams)))

    def set_graphs(self, enabled: bool) -> None:
        """Replay steady-state async frames from a captured hipGraph (default off; opt-in for CPU-bound hosts; bgs_set_graphs)."""
        self._check(self._lib.bgs_set_graphs(self._ctx, 1 if enabled else 0))

    # -- interop / introspection -----------------------------------------------------
    def synchronize(self) -> None:
        self._check(self._lib.bgs_synchronize(self._ctx))

    def set_profiling(self, level: int) -> None:
        """0 = no HIP events, 1 = frame start/end only, 2 = every stage (default)."""
        self._check(self._lib.bgs_set_profiling(self._ctx, int(level)))

    def set_profiling_stride(self, every_nth_frame: int) -> None:
        """Record HIP events only on every Nth frame (each record costs ~4 us of GPU timeline)."""
        self._check(self._lib.bgs_set_profiling_stride(self._ctx, int(every_nth_frame)))

    def set_pipeline_depth(self, lanes: int) -> None:
        """Frames in flight (1..8 lanes = per-frame buffer sets, multiplexed onto set_pipeline_streams() HIP
        streams); see bgs_set_pipeline_depth."""
        self._check(self._lib.bgs_set_pipeline_depth(self._ctx, int(lanes)))

    def set_output_srgb8(self, enabled: bool) -> None:
        """Also produce every frame as Rgba8UnormSrgb (the reference's target format)."""
        self._check(self._lib.bgs_set_output_srgb8(self._ctx, 1 if enabled else 0))

    def set_srgb8_target(self, device_ptr: Optional[int]) -> None:
        """The next `render` writes its Rgba8UnormSrgb image to this device address (one-shot)."""
        self._check(self._lib.bgs_set_srgb8_target(self._ctx, ctypes.c_void_p(device_ptr or 0)))

    def set_output_rgba16f(self, enabled: bool) -> None:
        """Also produce every frame as Rgba16Float (the reference's hdr colour attachment); exclusive with sRGB8."""
        self._check(self._lib.bgs_set_output_rgba16f(self._ctx, 1 if enabled else 0))

    def set_packed_only(self, enabled: bool) -> None:
        """Frames that write a packed image (sRGB8 / Rgba16Float) skip the f32 target."""
        self._check(self._lib.bgs_set_packed_only(self._ctx, 1 if enabled else 0))

    def _framebuffer(self, getter):
        """(address, bytes) of one of the last frame's images, from its `bgs_framebuffer_*device_ptr`."""
        p, nbytes = ctypes.c_void_p(), ctypes.c_uint64()
        self._check(getter(self._ctx, ctypes.byref(p), ctypes.byref(nbytes)))
        return p.value, nbytes.value

    def framebuffer_device_ptr(self):
        return self._framebuffer(self._lib.bgs_framebuffer_device_ptr)

    def framebuffer_rgba16f_device_ptr(self):
        return self._framebuffer(self._lib.bgs_framebuffer_rgba16f_device_ptr)

    def framebuffer_srgb8_device_ptr(self):
        return self._framebuffer(self._lib.bgs_framebuffer_srgb8_device_ptr)

    def pipeline_pop(self):
        """Complete the oldest frame in flight; returns (f32 framebuffer ptr, srgb8 ptr or None)."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.bgs_pipeline_pop(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def frames_in_flight(self) -> int:
        c = ctypes.c_uint32()
        self._check(self._lib.bgs_frames_in_flight(self._ctx, ctypes.byref(c)))
        return int(c.value)

    def set_async(self, enabled: bool) -> None:
        """Async frames: render(download=False) only enqueues (scan binning); see bgs_set_async."""
        self._check(self._lib.bgs_set_async(self._ctx, 1 if enabled else 0))

    def set_binning(self, mode: str) -> None:
        """'scan' (default): ordered coarse lists + lazy per-tile scan; 'sort': (tile, splat)
        instances + stable radix sort on the tile id. Images are bit-identical."""
        self._check(self._lib.bgs_set_binning(self._ctx, {"scan": 0, "sort": 1}[mode]))

    def draw_list(self) -> np.ndarray:
        """The sorted entries the last call left on the device (`bgs_sorted_entries_device_ptr` + `bgs_download`): after
        `sort` all n entries, after `render` the drawable prefix (what reaches the vertex stage, back to front)."""
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        self._check(self._lib.bgs_sorted_entries_device_ptr(self._ctx, ctypes.byref(p), ctypes.byref(n)))
        out = np.empty(n.value, dtype=SORT_ENTRY_DTYPE)
        if n.value:
            self._check(self._lib.bgs_download(self._ctx, p, out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    def device_alloc(self, nbytes: int) -> int:
        """`bgs_device_alloc`: device memory for what the caller hands over by device pointer (a depth buffer, a packed
        image target). Returns the address."""
        p = ctypes.c_void_p()
        self._check(self._lib.bgs_device_alloc(self._ctx, int(nbytes), ctypes.byref(p)))
        return int(p.value or 0)

    def device_free(self, device_ptr: int) -> None:
        self._check(self._lib.bgs_device_free(self._ctx, ctypes.c_void_p(device_ptr)))

    def device_block(self, nbytes: int, init: Optional[np.ndarray] = None) -> DeviceBlock:
        """`device_alloc` with an owner (`device_memory.DeviceBlock`: `free()` once, or `with`), holding `init` if one is
        given and it is not empty. If that upload raises, the block is freed."""
        return DeviceBlock.allocate(self, nbytes, init)

    def upload_bytes(self, device_ptr: int, host: np.ndarray) -> None:
        """`bgs_upload`: blocking host-to-device copy of a contiguous array."""
        a = np.ascontiguousarray(host)
        self._check(self._lib.bgs_upload(self._ctx, ctypes.c_void_p(device_ptr), a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    def download(self, device_ptr: int, host_out: np.ndarray) -> np.ndarray:
        """`bgs_download`: blocking device-to-host copy into a contiguous array (of a COMPLETED frame's memory)."""
        if not host_out.flags["C_CONTIGUOUS"] or not host_out.flags["WRITEABLE"]:
            raise ValueError("host_out must be a writeable C-contiguous array")
        self._check(self._lib.bgs_download(self._ctx, ctypes.c_void_p(device_ptr), host_out.ctypes.data_as(ctypes.c_void_p),
                                           host_out.nbytes))
        return host_out

    def upload_depth(self, depth: np.ndarray) -> int:
        """Put a view's scene depth on the device: `depth` is [height, width, samples] float32 (reverse-Z, what Bevy's
        opaque passes left in the view's Depth32Float attachment; src/render/mod.rs:959-974). Returns the device
        address for `View.depth_device_ptr`; release it with `device_free` once the frames that use it are complete."""
        return self.upload_attachments(depth)[0]

    def upload_attachments(self, depth: np.ndarray, color: Optional[np.ndarray] = None):
        """Put a view's attachment pair on the device in ONE allocation (include/bgs.h BGS_VIEW_ATTACH_COLOR): `depth`
        [height, width, samples] float32 as for `upload_depth`, and behind it, at `color_attachment_offset`, `color`
        [height, width, samples, 4] float32 — linear, premultiplied, unclamped RGBA, what the engine's opaque passes left in
        the colour attachment. Returns (address, holder): the address for `View.depth_device_ptr` (with
        `View.color_attachment = True` when `color` was given), and the allocation to `device_free` once the frames that
        use it are complete — the same value today; hold on to it rather than to the view's field. Without `color` this is
        `upload_depth` in an allocation whose start is 16-byte aligned."""
        d = np.ascontiguousarray(depth, dtype=np.float32)
        if d.ndim != 3 or d.shape[2] not in (1, 2, 4, 8):
            raise ValueError("depth must be [height, width, samples] with 1, 2, 4 or 8 samples")
        if color is None:
            return (self.device_block(d.nbytes, d).release(),) * 2
        c = np.ascontiguousarray(color, dtype=np.float32)
        if c.shape != d.shape + (4,):
            raise ValueError(f"color must be [height, width, samples, 4] = {d.shape + (4,)}, got {c.shape}")
        h, w, s = d.shape
        off = color_attachment_offset(w, h, s)
        with self.device_block(off + c.nbytes) as block:        # (the caller's once both halves are up)
            if block.ptr % 16:
                raise RuntimeError("device_alloc returned memory that is not 16-byte aligned")
            self.upload_bytes(block.ptr, d)
            self.upload_bytes(block.ptr + off, c)
            p = block.release()
        return p, p

    def build_id(self) -> str:
        """`bgs_build_id()`: SHA-256 of the kernel sources the loaded library was compiled from."""
        return self._lib.bgs_build_id().decode()

    # -- the multi-GPU frame gather (bgs_comm_*: RCCL behind the C ABI) ---------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128 bytes rank 0 ships to every rank (by any means) before `comm_create`."""
        buf = ctypes.create_string_buffer(_native.COMM_ID_BYTES)
        lib = _native.load()
        _native.check(lib, None, lib.bgs_comm_unique_id(buf))
        return buf.raw

    def comm_create(self, unique_id: bytes, world_size: int, rank: int) -> int:
        """Collective: returns the communicator handle once every rank has called it."""
        if len(unique_id) != _native.COMM_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        out = ctypes.c_void_p()
        self._check(self._lib.bgs_comm_create(self._ctx, unique_id, int(world_size), int(rank), ctypes.byref(out)))
        return out.value

    def comm_gather(self, comm: int, root: int, send_ptr: int, nbytes: int, recv_ptr: Optional[int]) -> int:
        """Enqueue one gather of `nbytes` per rank (device pointers; `recv_ptr` on the root only). Returns its ticket."""
        ticket = ctypes.c_uint64()
        self._check(self._lib.bgs_comm_gather(self._ctx, comm, int(root), ctypes.c_void_p(send_ptr), int(nbytes),
                                              ctypes.c_void_p(recv_ptr or 0), ctypes.byref(ticket)))
        return ticket.value

    def comm_gather_after(self, comm: int, root: int, send_ptr: int, nbytes: int, recv_ptr: Optional[int],
                          hip_stream: Optional[int] = None) -> int:
        """`bgs_comm_gather_after`: the gather ordered ON THE DEVICE behind everything enqueued so far on `hip_stream` (None:
        behind every frame this context still has in flight) — no pop / synchronise before the batch goes out. Returns the
        ticket. A frame re-run later (adaptive_counters: reruns_*) went out in the state of its first attempt."""
        t = ctypes.c_uint64(0)
        self._check(self._lib.bgs_comm_gather_after(self._ctx, comm, int(root), ctypes.c_void_p(send_ptr), int(nbytes),
                                                    ctypes.c_void_p(recv_ptr or 0), ctypes.c_void_p(hip_stream or 0), ctypes.byref(t)))
        return int(t.value)

    def comm_wait(self, comm: int, ticket: int = 0) -> None:
        """Block until the gather with `ticket` (and every earlier one) has completed; 0 = all of them."""
        self._check(self._lib.bgs_comm_wait(self._ctx, comm, int(ticket)))

    def comm_destroy(self, comm: int) -> None:
        self._lib.bgs_comm_destroy(self._ctx, comm)

    def reset_adaptive_state(self) -> None:
        """Forget the hints completed frames left in the context (draw count, key range, list capacity,
        supertile rule): the next frames behave like the first frames of a fresh context."""
        self._check(self._lib.bgs_reset_adaptive_state(self._ctx))

    def stream_handle(self) -> int:
        p = ctypes.c_void_p()
        self._check(self._lib.bgs_stream(self._ctx, ctypes.byref(p)))
        return p.value or 0

    def stats(self) -> dict:
        st = _native.BgsStats()
        self._check(self._lib.bgs_get_stats(self._ctx, ctypes.byref(st)))
        return {
            "total_ms": float(st.total_ms),
            "splat_count": int(st.splat_count),
            "visible_count": int(st.visible_count),
            "draw_count": int(st.draw_count),
            "instance_count": int(st.instance_count),
            "instance_capacity": int(st.instance_capacity),
            "list_entries_allocated": int(st.list_entries_allocated),
            "strip_tiles": int(st.strip_tiles),
            "tile_saturation": {"known": bool((int(st.tile_saturation) >> 16) & 1), "work_share": (int(st.tile_saturation) & 0x7FFF) / 0x7FFF,
                                "midround_exit": bool(int(st.tile_saturation) >> 31)},
            "tiles": (int(st.tiles_x), int(st.tiles_y)),
            "depth_passes": int(st.depth_passes),
            "tile_passes": int(st.tile_passes),
            "algorithmic_bytes": int(st.algorithmic_bytes),
            "regrow_count": int(st.regrow_count),
            "sort_path": ("onesweep", "bucket", "kept")[int(st.sort_path)],
            "list_capacity": int(st.list_capacity),
            "binning": "sort" if st.binning_mode else "scan",
            "frames_averaged": int(st.frames_averaged),
            "stage_ms": {n: float(st.stage_ms[i]) for i, n in enumerate(_native.STAGE_NAMES)},
        }
