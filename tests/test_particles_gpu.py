"""Particle behaviours on the device (bgs_cloud_apply_particle_behaviors). Every comparison is bitwise: the step's
arithmetic is a contract that numpy reproduces exactly (`particles.step_reference`, checked against the compiled
arithmetic in test_particles_host.py), so the expected value of everything below is computed on the host.

There is no position read-back in the C ABI. The two device copies of the position are pinned through what the library
exposes: a cloud stepped on the device must sort (the position plane) and render (word 0 of the packed records) exactly
like a fresh upload of the stepped positions."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from bevy_gaussian_splatting_amd import (
    PARTICLE_BEHAVIOR_DTYPE, CloudSettings, DrawMode, PlanarGaussian3d, SortMode, View, _native,
    random_gaussians_3d_seeded, random_particle_behaviors, step_reference)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5000
W = H = 128
DT60 = float(np.float32(1.0) / np.float32(60.0))
_CLOUD = None


def base_cloud() -> PlanarGaussian3d:
    """The 5000-splat cloud every test starts from (made once, never modified)."""
    global _CLOUD
    if _CLOUD is None:
        _CLOUD = random_gaussians_3d_seeded(N, 21)
        _CLOUD.position_visibility.setflags(write=False)
    return _CLOUD


def with_positions(cloud: PlanarGaussian3d, pv: np.ndarray) -> PlanarGaussian3d:
    return PlanarGaussian3d(pv, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity)


def upload(plugin, cloud, fmt):
    if fmt == "f16":
        return plugin.upload(cloud.to_f16())
    return plugin.upload(cloud, precompute_covariance_3d=(fmt == "cov3d"))


def indices(pattern: str, count: int, seed: int) -> np.ndarray:
    """`count` record indices; every pattern but the one-record identity names the last splat N - 1."""
    rng = np.random.default_rng(seed)
    if pattern == "identity":
        return np.arange(count, dtype=np.uint32)
    idx = np.append(rng.permutation(N - 1)[:count - 1], N - 1).astype(np.uint32)
    if pattern == "sparse":   # inactive and out-of-range records mixed in
        idx[::5] = 0xFFFFFFFF
        idx[1::7] = N
        idx[2::11] = N + 7
        idx[3::13] = 0x80000000
    idx[-1] = N - 1
    return idx


def records(idx: np.ndarray, seed: int) -> np.ndarray:
    r = random_particle_behaviors(len(idx), seed).records
    r["indicies"][:, 0] = idx
    return r


def views(samples: int = 4):
    return [View.headless(W, H, yaw=0.0, msaa_samples=samples), View.headless(W, H, yaw=2.0, msaa_samples=samples)]


def sort_blocking(plugin, handle, view, mode):
    plugin.reset_adaptive_state()
    return plugin.sort(handle, view, CloudSettings(sort_mode=mode))


def render_blocking(plugin, handle, view, settings=None):
    plugin.reset_adaptive_state()
    return plugin.render(handle, view, settings or CloudSettings())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_cloud(plugin, a, b, samples=4, settings=None, what=""):
    """Cloud handles a and b sort and render identically: the plane (Rayon: a key for every splat), the cull decisions
    (Radix), the record copy and its agreement with the plane (the frame)."""
    for k, v in enumerate(views(samples)):
        for mode in (SortMode.Rayon, SortMode.Radix):
            ea, eb = sort_blocking(plugin, a, v, mode), sort_blocking(plugin, b, v, mode)
            assert same_bits(ea, eb), f"{what}: {mode.name} entries differ, camera {k}"
    fa, fb = render_blocking(plugin, a, views(samples)[0], settings), render_blocking(plugin, b, views(samples)[0], settings)
    assert np.array_equal(fa, fb), f"{what}: frames differ"
    return fa


# ---- 1. the behaviours buffer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [DT60, 0.25], ids=["dt60", "dt025"])
def test_records_advance_like_the_numpy_twin_and_skipped_records_stay(plugin, dt):
    cloud = base_cloud()
    idx = indices("sparse", 1000, 5)
    idx[:3] = (0xFFFFFFFF, N, N + 7)
    rec0 = records(idx, 6)
    h = plugin.upload(cloud)
    b = plugin.upload_particle_behaviors(rec0)
    try:
        pv, rec = cloud.position_visibility, rec0
        for step in range(3):
            plugin.apply_particle_behaviors(h, b, dt)
            pv, rec = step_reference(pv, rec, dt)
            if step in (0, 2):   # after one step and after three
                got = plugin.download_particle_behaviors(b)
                assert same_bits(got, rec), f"records after step {step + 1}"
                assert same_bits(got["jerk"], rec0["jerk"]) and same_bits(got["indicies"], rec0["indicies"])
                skipped = (idx.view(np.int32) < 0) | (idx >= N)
                assert skipped[:3].all() and skipped.sum() > 300
                assert same_bits(got[skipped], rec0[skipped])
                assert not same_bits(got[~skipped]["velocity"], rec0[~skipped]["velocity"])
    finally:
        b.free()
        h.free()


# ---- 2. both position copies, via equivalence with a fresh upload ---------------------------------------------------
FORMATS, COUNTS, PATTERNS = ("f32", "f16", "cov3d"), (1, 255, 256, 257, 5000), ("identity", "permutation", "sparse")
CASES = [(FORMATS[i % 3], COUNTS[i % 5], PATTERNS[(i + 2 * (i // 5)) % 3], ("scan", "sort")[i % 2], (1, 4)[(i // 2) % 2],
          (DT60, 0.25)[(i // 3) % 2]) for i in range(15)]


@pytest.mark.parametrize("fmt,count,pattern,binning,samples,dt", CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-s{c[4]}-{'dt60' if c[5] == DT60 else 'dt025'}" for c in CASES])
def test_a_stepped_cloud_is_a_fresh_upload_of_the_stepped_positions(plugin, fmt, count, pattern, binning, samples, dt):
    cloud = base_cloud()
    rec0 = records(indices(pattern, count, 100 + count), 200 + count)
    pv1, rec1 = step_reference(cloud.position_visibility, rec0, dt)
    pv2, _ = step_reference(pv1, rec1, dt)
    plugin.set_binning(binning)
    a = upload(plugin, cloud, fmt)
    b = plugin.upload_particle_behaviors(rec0)
    fresh = []
    try:
        before = sort_blocking(plugin, a, views()[0], SortMode.Rayon)
        for step, pv in enumerate((pv1, pv2)):   # one step, then a second one on the stepped cloud
            plugin.apply_particle_behaviors(a, b, dt)
            fresh.append(upload(plugin, with_positions(cloud, pv), fmt))
            assert_same_cloud(plugin, a, fresh[-1], samples, what=f"step {step + 1}")
        if count >= 255:   # (the stepped cloud is not the old one)
            assert not same_bits(sort_blocking(plugin, a, views()[0], SortMode.Rayon), before)
    finally:
        plugin.set_binning("scan")
        b.free()
        a.free()
        for h in fresh:
            h.free()


# ---- 3. the w lane --------------------------------------------------------------------------------------------------
def test_visibility_moves_with_the_w_lane(plugin):
    """velocity.w = +-40 at dt = 1/60 moves visibility by 2/3: across the 0.5 of DrawMode::Selected, both ways."""
    cloud = base_cloud()
    pv0 = cloud.position_visibility.copy()
    pv0[:, 3] = (np.arange(N) % 2).astype(np.float32)            # odd splats selected
    start = with_positions(cloud, pv0)
    rec0 = np.zeros(N, PARTICLE_BEHAVIOR_DTYPE)
    rec0["indicies"][:, 0] = np.arange(N, dtype=np.uint32)
    rec0["velocity"][:, 3] = np.where(np.arange(N) % 2 == 1, -40.0, 40.0)   # ... and every splat changes sides
    pv1, _ = step_reference(pv0, rec0, DT60)
    assert ((pv1[:, 3] > 0.5) == (pv0[:, 3] < 0.5)).all() and same_bits(pv1[:, :3], pv0[:, :3])
    selected = CloudSettings(draw_mode=DrawMode.Selected)
    a, fresh = plugin.upload(start), plugin.upload(with_positions(cloud, pv1))
    b = plugin.upload_particle_behaviors(rec0)
    try:
        unstepped = render_blocking(plugin, a, views()[0], selected)
        plugin.apply_particle_behaviors(a, b, DT60)
        stepped = assert_same_cloud(plugin, a, fresh, settings=selected, what="w lane")
        assert not np.array_equal(stepped, unstepped)
    finally:
        b.free()
        a.free()
        fresh.free()


# ---- 4. dt = 0 ------------------------------------------------------------------------------------------------------
def test_a_step_of_zero_seconds_changes_nothing(plugin):
    cloud = base_cloud()
    rec0 = records(indices("permutation", 5000, 9), 10)
    a, same = plugin.upload(cloud), plugin.upload(cloud)
    b = plugin.upload_particle_behaviors(rec0)
    try:
        plugin.apply_particle_behaviors(a, b, 0.0)
        assert_same_cloud(plugin, a, same, what="dt 0")
        assert same_bits(plugin.download_particle_behaviors(b), rec0)
    finally:
        b.free()
        a.free()
        same.free()


# ---- 5. the step is a pipeline barrier ------------------------------------------------------------------------------
def _popped_frame(plugin):
    f32, _ = plugin.pipeline_pop()
    return plugin.download(f32, np.empty((H, W, 4), np.float32))


def test_frames_in_flight_keep_the_old_positions_and_later_frames_see_the_new(plugin):
    cloud = base_cloud()
    rec0 = records(indices("permutation", 5000, 31), 32)
    pv1, _ = step_reference(cloud.position_visibility, rec0, 0.25)
    v, s = views()[0], CloudSettings()
    a, fresh = plugin.upload(cloud), plugin.upload(with_positions(cloud, pv1))
    b = plugin.upload_particle_behaviors(rec0)
    try:
        old, new = render_blocking(plugin, a, v), render_blocking(plugin, fresh, v)
        assert not np.array_equal(old, new)
        plugin.set_pipeline_depth(4)
        plugin.set_async(True)
        for _ in range(4):   # settle the kind of frame, so that F0 below is really in flight when the step arrives
            plugin.render(a, v, s, download=False)
        for _ in range(4):
            assert np.array_equal(_popped_frame(plugin), old)
        plugin.render(a, v, s, download=False)               # F0
        plugin.apply_particle_behaviors(a, b, 0.25)
        assert plugin.frames_in_flight() == 1                # completed by the step, still in the ring
        plugin.render(a, v, s, download=False)               # F1
        assert plugin.frames_in_flight() == 2
        assert np.array_equal(_popped_frame(plugin), old), "F0 was enqueued before the step"
        assert np.array_equal(_popped_frame(plugin), new), "F1 was enqueued after the step"
        assert plugin.frames_in_flight() == 0
    finally:
        plugin.set_async(False)
        plugin.set_pipeline_depth(1)
        b.free()
        a.free()
        fresh.free()


def test_a_replayed_frame_graph_draws_the_stepped_cloud(plugin):
    cloud = base_cloud()
    rec0 = records(indices("permutation", 5000, 41), 42)
    pv1, _ = step_reference(cloud.position_visibility, rec0, 0.25)
    v, s = views()[0], CloudSettings()
    a, fresh = plugin.upload(cloud), plugin.upload(with_positions(cloud, pv1))
    b = plugin.upload_particle_behaviors(rec0)

    def frame():
        plugin.render(a, v, s, download=False)
        plugin.synchronize()
        ptr, _ = plugin.framebuffer_device_ptr()
        return plugin.download(ptr, np.empty((H, W, 4), np.float32))
    try:
        old, new = render_blocking(plugin, a, v), render_blocking(plugin, fresh, v)
        plugin.set_profiling(0)   # (timed frames are launched directly)
        plugin.set_pipeline_depth(2)
        plugin.set_async(True)
        plugin.set_graphs(True)
        _, r0 = plugin.graph_counters()
        for _ in range(12):
            assert np.array_equal(frame(), old)
        _, r1 = plugin.graph_counters()
        assert r1 > r0, "no frame was replayed from a graph before the step"
        plugin.apply_particle_behaviors(a, b, 0.25)
        replayed = 0
        for _ in range(6):
            _, before = plugin.graph_counters()
            got = frame()
            replayed += plugin.graph_counters()[1] - before
            assert np.array_equal(got, new)
        assert replayed >= 1, "no frame behind the step was replayed from a graph"
    finally:
        plugin.set_graphs(False)
        plugin.set_async(False)
        plugin.set_pipeline_depth(1)
        plugin.set_profiling(2)
        b.free()
        a.free()
        fresh.free()


# ---- 6. errors ------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_einval_with_a_message(plugin):
    lib, ctx = plugin._lib, plugin._ctx
    a = plugin.upload(base_cloud())
    b = plugin.upload_particle_behaviors(records(indices("identity", 16, 1), 2))
    call = lib.bgs_cloud_apply_particle_behaviors
    f = ctypes.c_float
    try:
        assert call(None, a._ptr, ctypes.c_void_p(b.ptr), 16, f(0.1)) == _native.BGS_EINVAL
        assert b"ctx is NULL" in lib.bgs_last_error(None)
        assert call(ctx, None, ctypes.c_void_p(b.ptr), 16, f(0.1)) == _native.BGS_EINVAL
        assert b"cloud is NULL" in lib.bgs_last_error(ctx)
        assert call(ctx, a._ptr, None, 16, f(0.1)) == _native.BGS_EINVAL
        assert b"behaviors_device_ptr is NULL" in lib.bgs_last_error(ctx)
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert call(ctx, a._ptr, ctypes.c_void_p(b.ptr), 16, f(bad)) == _native.BGS_EINVAL
            assert b"delta_time" in lib.bgs_last_error(ctx)
        assert call(ctx, a._ptr, None, 0, f(0.1)) == _native.BGS_OK            # count == 0: nothing happens
        assert call(ctx, a._ptr, ctypes.c_void_p(b.ptr), 0, f(0.1)) == _native.BGS_OK
        same = plugin.upload(base_cloud())
        assert_same_cloud(plugin, a, same, what="after the refused calls")       # ... and nothing did
        same.free()
    finally:
        b.free()
        a.free()


# ---- 7. the example's flag ------------------------------------------------------------------------------------------
def test_headless_particle_count_matches_the_python_plugin(plugin, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "headless"], check=True, capture_output=True)
    cloud = base_cloud()
    planes = tmp_path / "cloud.bin"
    with open(planes, "wb") as f:
        f.write(struct.pack("<I", len(cloud)))
        for plane in (cloud.position_visibility, cloud.spherical_harmonic, cloud.rotation, cloud.scale_opacity):
            f.write(np.ascontiguousarray(plane, np.float32).tobytes())
    r = subprocess.run([os.path.join(ROOT, "examples", "headless"), "--cloud", str(planes), "--width", str(W), "--height", str(H),
                        "--frames", "3", "--depth", "2", "--particle-count", "1000", "--output-dir", str(tmp_path),
                        "--dump-f32", str(tmp_path / "frame.f32"), "--dump-particle-behaviors", str(tmp_path / "behaviors.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "frame.f32", np.float32).reshape(H, W, 4)
    rec0 = np.fromfile(tmp_path / "behaviors.bin", PARTICLE_BEHAVIOR_DTYPE)
    assert rec0.shape == (1000,) and np.array_equal(rec0["indicies"][:, 0], np.arange(1000, dtype=np.uint32))
    a = plugin.upload(cloud)
    b = plugin.upload_particle_behaviors(rec0)
    try:
        unstepped = render_blocking(plugin, a, View.headless(W, H))
        for _ in range(3):   # --particle-dt defaults to 1/60
            plugin.apply_particle_behaviors(a, b, DT60)
        want = render_blocking(plugin, a, View.headless(W, H))
        assert np.array_equal(got, want) and not np.array_equal(got, unstepped)
    finally:
        b.free()
        a.free()
