"""`MorphPair` (the two sides of a `GaussianInterpolate`, libbgs_morph.so) and `ResidentCloud4d` (a playing 4D asset,
libbgs_slice.so), made by `GaussianSplattingPlugin.morph_pair` / `resident_4d`. Both are a `ResidentProducer`: input planes
that go up once, output planes, and `at(settings)`, which enqueues the producer on `bgs_stream` and hands the output's device
planes to the cloud upload, which packs them where they lie (include/bgs.h "DEVICE PLANES"): nothing crosses the host."""
from __future__ import annotations

import numpy as np

from .device_memory import DeviceBlock
from .gaussian import PlanarGaussian3d, PlanarGaussian4d
from .interpolate import COV3D_WIDTHS, F32_WIDTHS, GaussianInterpolator, covariance_planes, planes_of
from .settings import CloudSettings
from .time_slice import TimeSlicer


class ResidentProducer:
    """`n` splats' input planes and output planes, one `DeviceBlock` each, inputs first. A subclass states the input planes
    (host arrays, uploaded here), the output planes' widths in floats, the cloud format of the output
    (`plugin.DEVICE_PLANE_FORMATS`), and `enqueue`. A construction that fails part-way frees what it had."""

    def __init__(self, plugin: "GaussianSplattingPlugin", n: int, in_planes, out_widths, fmt: str):
        self._plugin = plugin
        self.n = int(n)
        self._inputs, self._out_widths, self._format = len(in_planes), tuple(out_widths), fmt
        self._blocks = []
        if self.n:
            try:
                for plane in in_planes:
                    self._blocks.append(DeviceBlock.allocate(plugin, plane.nbytes, plane))
                for w in self._out_widths:
                    self._blocks.append(DeviceBlock.allocate(plugin, self.n * w * 4))
            except BaseException:
                self.free()
                raise

    def __len__(self) -> int:
        return self.n

    @property
    def in_ptrs(self) -> list:     # the input planes' device addresses, in the producer's order ([] once freed, or empty)
        return [b.ptr for b in self._blocks[:self._inputs]]

    @property
    def out_ptrs(self) -> list:    # the output planes' device addresses, in the order of the format's C entry point
        return [b.ptr for b in self._blocks[self._inputs:]]

    def enqueue(self, stream: int, settings: CloudSettings) -> None:
        """Enqueue the producer on `stream`: `in_ptrs` at `settings.time` into `out_ptrs`. Nothing is waited for."""
        raise NotImplementedError

    def at(self, settings: CloudSettings, return_planes: bool = False):
        """The output cloud at `settings.time` (see the producer for what else it reads) as a resident handle. The producer
        is enqueued on `bgs_stream` and the upload follows it with no synchronisation in between: the upload orders itself
        behind that stream and returns once the cloud is complete, so the next `at` may overwrite the output planes. Free
        the handle before the next time's replaces it. With `return_planes` also the output's planes, downloaded."""
        plugin, widths = self._plugin, self._out_widths
        outs = [np.zeros((self.n, w), np.float32) for w in widths] if return_planes else None
        if self.n and not self._blocks:
            raise RuntimeError(f"this {type(self).__name__} was freed")
        if self.n:
            self.enqueue(plugin.stream_handle(), settings)
        out_ptrs = self.out_ptrs if self.n else [0] * len(widths)
        handle = plugin.upload_device_planes(self._format, self.n, out_ptrs)
        if return_planes and self.n:
            for ptr, plane in zip(out_ptrs, outs):     # (the upload has synchronised: the planes are complete)
                plugin.download(ptr, plane)
        return (handle, tuple(outs)) if return_planes else handle

    def free(self) -> None:
        blocks, self._blocks = self._blocks, []
        for block in blocks:
            block.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class MorphPair(ResidentProducer):
    """The two sides of a morph (`GaussianInterpolate { lhs, rhs }`) and the output's planes. `at(settings)` runs the blend
    (`interpolate.GaussianInterpolator`; time_start and time_stop are read as well); the handle is of format "cov3d" for a
    pair made with `precompute_covariance_3d`, which blends the `Covariance3dOpacity` planes instead of rotation and scale."""

    def __init__(self, plugin: "GaussianSplattingPlugin", lhs: PlanarGaussian3d, rhs: PlanarGaussian3d,
                 precompute_covariance_3d: bool = False, interpolator=None):
        if not isinstance(lhs, PlanarGaussian3d) or not isinstance(rhs, PlanarGaussian3d):
            raise TypeError("lhs and rhs must be f32 PlanarGaussian3d")
        if len(lhs) != len(rhs):
            raise ValueError(f"lhs has {len(lhs)} splats, rhs {len(rhs)}: a morph needs two clouds of equal length")
        self.interpolator = interpolator or GaussianInterpolator(plugin.device)
        self.precompute_covariance_3d = bool(precompute_covariance_3d)
        sides = [planes_of(covariance_planes(c) if precompute_covariance_3d else c) for c in (lhs, rhs)]
        super().__init__(plugin, len(lhs), sides[0] + sides[1], COV3D_WIDTHS if precompute_covariance_3d else F32_WIDTHS,
                         "cov3d" if precompute_covariance_3d else "f32")

    def enqueue(self, stream: int, settings: CloudSettings) -> None:
        ins, k = self.in_ptrs, len(self._out_widths)       # the lhs's planes, then the rhs's: as many a side as the output's
        self.interpolator.interpolate(stream, self.n, ins[:k], ins[k:], self.out_ptrs, settings)


class ResidentCloud4d(ResidentProducer):
    """A 4D cloud's five planes and the three planes of its slice: the analogue of `MorphPair` for a playing 4D asset.
    `at(settings)` runs the slice (`time_slice.TimeSlicer`; global_scale, time_start and time_stop are read too); the handle is
    of format "cov3d": sort and render it with any settings of that path, which reads neither `time` nor `global_scale`."""

    WIDTHS = (4, 48, 8)

    def __init__(self, plugin: "GaussianSplattingPlugin", cloud4d: PlanarGaussian4d, slicer=None):
        if not isinstance(cloud4d, PlanarGaussian4d):
            raise TypeError("cloud4d must be a PlanarGaussian4d")
        self.slicer = slicer or TimeSlicer(plugin.device)
        super().__init__(plugin, len(cloud4d), cloud4d.planes(), self.WIDTHS, "cov3d")

    def enqueue(self, stream: int, settings: CloudSettings) -> None:
        self.slicer.slice(stream, self.n, self.in_ptrs, self.out_ptrs, settings)
