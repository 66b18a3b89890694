"""The twelve traced instantiations of raster_scan_kernel (RasterInst::exists with trace, csrc/frame_params.h: no depth buffer,
no overlay, 1 or 4 samples; OBB modes 0 / 1 / 2, AABB3D 0 / 1, surfel 0), which no stage test launches: each one through a
whole frame with a per-tile trace buffer set (bgs_set_tile_trace), its mode forced by the debug flags.

  The image is bit-equal to the same frame without the trace: the instrumentation touches no pixel.
  The frame ran the mode that was asked for (bgs_debug_frame_leftovers: raster_mode).
  Every tile's two trace words were written over the 0xFF bytes the buffer held."""
import numpy as np
import pytest

from bevy_gaussian_splatting_amd import CloudSettings, GaussianMode, GaussianSplattingPlugin, View, random_gaussians_3d_seeded

pytestmark = pytest.mark.gpu

W, H = 64, 48
TILES = (W // 16) * (H // 16)
OBB, AABB3D, SURFEL = 0, 1, 2
# include/bgs_diag.h
LEVEL = {0: 0x10000, 1: 0x8000, 2: 0x400000, 3: 0x800000}
MIDROUND_ALWAYS, NO_MIDROUND = 0x20000, 0x1000000

# (variant, samples, mode, flags): level >= 2 gives the dense frames' exit (1); below it MIDROUND_ALWAYS gives OBB the sparse
# frames' exit (2) and AABB3D its only one (1); surfels have none whatever is asked
CASES = [(OBB, 1, 0, LEVEL[0] | NO_MIDROUND), (OBB, 4, 0, LEVEL[3] | NO_MIDROUND),
         (OBB, 1, 1, LEVEL[2]), (OBB, 4, 1, LEVEL[3]),
         (OBB, 1, 2, LEVEL[0] | MIDROUND_ALWAYS), (OBB, 4, 2, LEVEL[1] | MIDROUND_ALWAYS),
         (AABB3D, 1, 0, LEVEL[1] | NO_MIDROUND), (AABB3D, 4, 0, LEVEL[2] | NO_MIDROUND),
         (AABB3D, 1, 1, LEVEL[1] | MIDROUND_ALWAYS), (AABB3D, 4, 1, LEVEL[2]),
         (SURFEL, 1, 0, LEVEL[0]), (SURFEL, 4, 0, LEVEL[3] | MIDROUND_ALWAYS)]


def test_the_cases_are_the_twelve_traced_instantiations():
    assert sorted({c[:3] for c in CASES}) == sorted((v, s, m) for v, modes in ((OBB, (0, 1, 2)), (AABB3D, (0, 1)), (SURFEL, (0,)))
                                                    for s in (1, 4) for m in modes)
    assert len(CASES) == 12 and {lv for lv in LEVEL if any(c[3] & LEVEL[lv] for c in CASES)} == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def ctx():
    """A context of its own (the session's plugin keeps its trace pointer and flags), the cloud resident, a trace buffer."""
    p = GaussianSplattingPlugin(0)
    cloud = random_gaussians_3d_seeded(200, 3)
    cloud.position_visibility[:, :3] *= 0.1   # all 200 in front of the headless camera, scales up to 1: they overlap
    p.cloud = p.upload(cloud)
    p.trace = p.device_alloc(TILES * 32)
    yield p
    p.set_tile_trace(None)
    p.device_free(p.trace)
    p.cloud.free()
    p.close()


def _settings(variant):
    s = CloudSettings(aabb=variant != OBB)
    if variant == SURFEL:
        s.gaussian_mode = GaussianMode.Gaussian2d
    return s


@pytest.mark.parametrize("variant,samples,mode,flags", CASES, ids=[f"v{v}_s{s}_m{m}_flags{f:#x}" for v, s, m, f in CASES])
def test_a_traced_frame_draws_the_untraced_image_in_the_mode_asked_for(ctx, variant, samples, mode, flags):
    p = ctx
    view, settings = View.headless(W, H, msaa_samples=samples), _settings(variant)
    try:
        p.set_debug_flags(flags)
        p.reset_adaptive_state()
        plain = p.render(p.cloud, view, settings)
        assert p.debug_frame_leftovers()["raster_mode"] == mode
        assert p.stats()["visible_count"] >= 100 and (plain != plain[0, 0]).any()
        p.upload_bytes(p.trace, np.full(TILES * 32, 0xFF, np.uint8))
        p.set_tile_trace(p.trace)
        p.reset_adaptive_state()
        traced = p.render(p.cloud, view, settings)
        assert p.debug_frame_leftovers()["raster_mode"] == mode
        words = p.download(p.trace, np.empty((TILES, 2, 4), np.uint32))
    finally:
        p.set_tile_trace(None)
        p.set_debug_flags(0)
    assert np.array_equal(plain.view(np.uint32), traced.view(np.uint32))
    # word 0: s_memtime at the wave's start and end; word 1: HW_ID, XCC_ID, candidates scanned, blended | staged << 16
    start = words[:, 0, 0].astype(np.uint64) | (words[:, 0, 1].astype(np.uint64) << np.uint64(32))
    end = words[:, 0, 2].astype(np.uint64) | (words[:, 0, 3].astype(np.uint64) << np.uint64(32))
    assert (words[:, 0] != 0xFFFFFFFF).any(axis=1).all() and (end >= start).all()
    assert (words[:, 1] != 0xFFFFFFFF).any(axis=1).all()
    assert (words[:, 1, 2] > 0).all() and (words[:, 1, 2] != 0xFFFFFFFF).all()   # every tile had candidates to scan
