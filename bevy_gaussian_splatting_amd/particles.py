"""Particle behaviours (src/morph/particle.rs, src/morph/particle.wgsl): per-splat velocity / acceleration / jerk that a
compute pass integrates into the cloud's positions before the draw.

The step itself runs on the device (`bgs_cloud_apply_particle_behaviors`, csrc/particle_kernels.hip) on records that live
in device memory; this module holds the record layout, the host-side validation, the seeded generator and
`step_reference`, a numpy twin of the step's arithmetic contract that the tests compare the device with bit for bit.
"""
from __future__ import annotations

import numpy as np

from .device_memory import DeviceBlock

# ParticleBehavior (src/morph/particle.rs:349-358, #[repr(C)] Pod): 64 bytes, fields at 0 / 16 / 32 / 48.
# `indicies` is the reference's spelling; [0] is the splat index, read as int32 (negative = inactive).
PARTICLE_BEHAVIOR_DTYPE = np.dtype([
    ("indicies", np.uint32, (4,)),
    ("velocity", np.float32, (4,)),
    ("acceleration", np.float32, (4,)),
    ("jerk", np.float32, (4,)),
])
assert PARTICLE_BEHAVIOR_DTYPE.itemsize == 64

_C6 = np.float32(1.0 / 6.0)   # 0x3E2AAAAB
_HALF = np.float32(0.5)


def splat_indices(records: np.ndarray) -> np.ndarray:
    """`indicies[0]` of every record as the kernel reads it: int32."""
    return np.ascontiguousarray(records["indicies"][:, 0]).view(np.int32)


def validate(records: np.ndarray, n: int) -> None:
    """What the C ABI states as its precondition, checked on the host: every active record (index >= 0 as int32) names a
    splat of the cloud (index < n; the device would skip such a record, a host that builds one has a bug) and no two
    active records name the same splat (on the device that is a data race)."""
    idx = splat_indices(records)
    active = idx[idx >= 0]
    if active.size and int(active.max()) >= int(n):
        raise ValueError(f"particle behaviour names splat {int(active.max())}, the cloud has {int(n)}")
    if np.unique(active).size != active.size:
        raise ValueError("two active particle behaviours name the same splat")


class ParticleBehaviors:
    """Host image of a behaviours buffer for a cloud of `n` splats: a structured array of PARTICLE_BEHAVIOR_DTYPE,
    validated (`validate`). `GaussianSplattingPlugin.upload_particle_behaviors` puts it on the device."""

    def __init__(self, records: np.ndarray, n: int):
        records = np.ascontiguousarray(records)
        if records.dtype != PARTICLE_BEHAVIOR_DTYPE or records.ndim != 1:
            raise TypeError("records must be a 1-D array of PARTICLE_BEHAVIOR_DTYPE")
        validate(records, n)
        self.records = records.copy()
        self.n = int(n)

    def __len__(self) -> int:
        return int(self.records.shape[0])


class ParticleBehaviorsHandle(DeviceBlock):
    """Behaviours resident in device memory the caller owns (`bgs_device_alloc`): a `DeviceBlock` (`ptr`, 0 once freed;
    `free()`) of `count` records, never shorter than 64 bytes."""

    def __init__(self, plugin, ptr: int, count: int):
        super().__init__(plugin, ptr, max(int(count) * PARTICLE_BEHAVIOR_DTYPE.itemsize, 64))
        self.count = int(count)

    def __len__(self) -> int:
        return self.count


def random_particle_behaviors(n: int, seed: int) -> ParticleBehaviors:
    """`random_particle_behaviors` (src/morph/particle.rs:374-410) for splats 0 .. n-1: velocity ~ U(-1, 1), acceleration
    ~ U(-0.01, 0.01), jerk ~ U(-1e-4, 1e-4) on all four lanes, indicies = (i, 0, 0, 0). The reference draws from the
    thread RNG; this is seeded (numpy's PCG64)."""
    rng = np.random.default_rng(seed)
    r = np.zeros(int(n), PARTICLE_BEHAVIOR_DTYPE)
    r["indicies"][:, 0] = np.arange(int(n), dtype=np.uint32)
    r["velocity"] = rng.uniform(-1.0, 1.0, (int(n), 4)).astype(np.float32)
    r["acceleration"] = rng.uniform(-0.01, 0.01, (int(n), 4)).astype(np.float32)
    r["jerk"] = rng.uniform(-1e-4, 1e-4, (int(n), 4)).astype(np.float32)
    return ParticleBehaviors(r, n)


def step_reference(position_visibility: np.ndarray, behaviors: np.ndarray, dt: float):
    """One step as the device computes it (csrc/particle_math.h), op by op in float32, every operation rounded once:

        dp = ((v*dt) + (((0.5*a)*dt)*dt)) + ((((c6*j)*dt)*dt)*dt)
        dv = (a*dt) + (((0.5*j)*dt)*dt)
        da = j*dt

    Records whose index is negative (int32) or >= n are skipped entirely; indices of active records must be distinct.
    Returns (new position_visibility [n, 4], new records); the inputs are left unchanged."""
    pv = np.array(position_visibility, dtype=np.float32, copy=True)
    rec = np.array(behaviors, dtype=PARTICLE_BEHAVIOR_DTYPE, copy=True)
    dt = np.float32(dt)
    idx = splat_indices(rec)
    act = np.flatnonzero((idx >= 0) & (idx < pv.shape[0]))
    i = idx[act]
    v, a, j = rec["velocity"][act], rec["acceleration"][act], rec["jerk"][act]
    dp = ((v * dt) + (((_HALF * a) * dt) * dt)) + ((((_C6 * j) * dt) * dt) * dt)
    dv = (a * dt) + (((_HALF * j) * dt) * dt)
    da = j * dt
    assert dp.dtype == dv.dtype == da.dtype == np.float32
    pv[i] = pv[i] + dp
    rec["velocity"][act] = v + dv
    rec["acceleration"][act] = a + da
    return pv, rec
