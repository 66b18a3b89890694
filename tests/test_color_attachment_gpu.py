"""The view's colour attachment on the device (bgs_view.reserved[0] = BGS_VIEW_ATTACH_COLOR, include/bgs.h): a frame blends
over what the engine's opaque passes left in the colour attachment, sample by sample, instead of over a constant clear
colour. The case (viewport, cloud, depth plane, colour plane) is color_attachment_cases.py's; expected values come from the
oracle, which knows nothing of colour attachments: it takes a depth buffer and a sample count, and that is enough to
recover every sample's transmittance (test 4)."""
import contextlib

import numpy as np
import pytest

import color_attachment_cases as K
import helpers as H
import packed_exact as P
from bevy_gaussian_splatting_amd import GaussianMode, PlanarGaussian3d, composite_reference

pytestmark = pytest.mark.gpu

VARIANTS = {"obb3d": {}, "aabb3d": {"aabb": True}, "obb2d": {"gaussian_mode": GaussianMode.Gaussian2d},
            "surfel": {"gaussian_mode": GaussianMode.Gaussian2d, "aabb": True}}
_ORACLE = {}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def restore(plugin):
    plugin.set_debug_flags(0)
    plugin.set_packed_only(False)
    plugin.set_async(False)
    plugin.set_graphs(False)
    plugin.set_profiling(2)
    plugin.set_pipeline_depth(1)
    plugin.set_output_srgb8(False)
    plugin.set_output_rgba16f(False)
    plugin.set_binning("scan")


@pytest.fixture()
def ctx(plugin):
    """The session's context with every switch these tests touch at its default, before and after."""
    restore(plugin)
    yield plugin
    restore(plugin)


@pytest.fixture(params=["scan", "sort"])
def binning(request, ctx):
    ctx.set_binning(request.param)
    return request.param


@contextlib.contextmanager
def attached(plugin, view, depth, color, flag=True):
    """`view` with the attachment pair (depth, color) on the device for the frames inside; freed afterwards."""
    ptr, holder = plugin.upload_attachments(depth, color)
    view.depth_device_ptr, view.color_attachment = ptr, bool(flag and color is not None)
    try:
        yield view
    finally:
        view.depth_device_ptr, view.color_attachment = 0, False
        plugin.device_free(holder)


def oracle_frame(oracle, samples, variant="obb3d", bbox=False, seed=K.SEED):
    """The oracle's frame of the case over a TRANSPARENT clear, with the case's depth plane: (C, amb, entries). C.a =
    1 - mean_s(T_s). Computed once per configuration."""
    key = (samples, variant, bbox, seed)
    if key not in _ORACLE:
        c, v = K.cloud(seed), K.view(samples)
        s = K.settings(visualize_bounding_box=bbox, **VARIANTS[variant])
        e = oracle.sort(c, v, s)
        ref, amb = oracle.render(c, e, v, s, with_ambiguity=True, depth=K.depth_plane(samples))
        for a in (ref, amb, e):
            a.setflags(write=False)
        _ORACLE[key] = (ref, amb, e)
    return _ORACLE[key]


def only_through_amb(ref, got, amb):
    """(every value within 1e-3 + 1e-4 |ref| + amb, share of PIXELS that need the amb term, largest error)"""
    ok, err = H.tolerance_mask(ref, got, amb)
    strict, _ = H.tolerance_mask(ref, got, None)
    return bool(ok.all()), float((~strict).any(axis=2).mean()), float(err.max())


# ---- 1. refusals (on the parent commit these frames render) -----------------------------------------------------------------
def test_invalid_flags_and_addresses_are_refused(ctx):
    c, s = K.cloud(), K.settings()
    h = ctx.upload(c)
    ptr, holder = ctx.upload_attachments(K.depth_plane(2), K.color_plane(2))
    try:
        # reserved[0] > 1 (a View cannot say that: through the marshalled struct)
        v = K.view(2)
        v.depth_device_ptr = ptr
        pv = ctx.prepare(v, s)
        pv.view.reserved[0] = 2
        with pytest.raises(Exception) as ei:
            ctx.render(h, pv)
        assert "reserved" in str(ei.value)
        # the colour flag without an address
        v = K.view(2)
        v.color_attachment = True
        with pytest.raises(Exception) as ei:
            ctx.render(h, v, s)
        assert "reserved" in str(ei.value) and "depth_device_ptr" in str(ei.value)
        # ... and with one that a depth plane alone could have (a multiple of 4 * sample_count) but a pair cannot
        for samples, off in ((1, 4), (2, 8), (1, 12)):
            v = K.view(samples)
            v.depth_device_ptr, v.color_attachment = ptr + off, True
            with pytest.raises(Exception) as ei:
                ctx.render(h, v, s)
            assert "reserved" in str(ei.value) and "16" in str(ei.value), (samples, off)
            v.color_attachment = False
            ctx.render(h, v, s)    # the same address as a depth plane alone is fine
        # the context is as usable as before
        v = K.view(2)
        v.depth_device_ptr, v.color_attachment = ptr, True
        assert np.isfinite(ctx.render(h, v, s)).all()
    finally:
        ctx.device_free(holder)
        h.free()


# ---- 2. pixels no fragment reaches are exact ---------------------------------------------------------------------------------
def _packed_of(oracle, f32, fmt):
    """packed_exact.py's conversion of an f32 image: uint16 [h, w, 4] binary16 bits from its f16_bits; uint8 [h, w, 4] sRGB8
    codes through the oracle's srgb8_codes, which test_packed_exact_host.py pins to packed_exact.py's thresholds at every
    code boundary (building the 510 thresholds from rationals takes ten seconds; the oracle searches the same boundaries)."""
    f32 = np.ascontiguousarray(f32, np.float32)
    if fmt == "srgb8":
        return oracle.srgb8_codes(f32)
    import torch   # (f16_bits is written in torch; the session's first import of it is the ten seconds of a run of this file alone)
    return P.f16_bits(torch.from_numpy(f32.view(np.int32).copy())).numpy().astype(np.uint16)


@pytest.mark.parametrize("fmt", ["f32", "srgb8", "rgba16f"])
@pytest.mark.parametrize("samples", [1, 2, 4, 8])
def test_untouched_pixels_are_exact(ctx, oracle, binning, samples, fmt):
    """Every pixel no fragment reaches in the oracle's frame — empty, or behind the occluder in every sample — has C = 0 and
    T_s = 1 and comes out as the twin says, bit for bit: the left-to-right f32 sum of its S samples times 1/S. That pins the
    colour plane's offset, the [y][x][sample] order and the partial tiles at the right and bottom edges; the packed outputs
    are packed_exact.py's conversions of the same value."""
    c, s, v = K.cloud(), K.settings(), K.view(samples, clear=(0.3, 0.6, 0.9, 1.0))   # (the clear colour is ignored)
    depth, color = K.depth_plane(samples), K.color_plane(samples)
    ref, amb, _ = oracle_frame(oracle, samples)
    untouched = (ref == 0.0).all(axis=2) & (amb == 0.0)
    assert untouched.mean() > 1.0 / 3.0 and untouched[16:].any() and untouched[:, 32:].any() and untouched[16:, 32:].any()
    assert (untouched[:, :K.W // 3]).any(), "empty pixels the depth plane leaves open"
    assert ((ref[..., 3] > 0.999) & (amb == 0.0)).any() and not untouched.all(), "saturated pixels exist too"
    twin = composite_reference(np.zeros((K.H, K.W, 4), np.float32), np.ones((K.H, K.W, samples), np.float32), color)
    h = ctx.upload(c)
    if fmt == "srgb8":
        ctx.set_output_srgb8(True)
    elif fmt == "rgba16f":
        ctx.set_output_rgba16f(True)
    try:
        with attached(ctx, v, depth, color) as va:
            got = ctx.render(h, va, s)
            packed = None
            if fmt != "f32":
                ptr = (ctx.framebuffer_srgb8_device_ptr() if fmt == "srgb8" else ctx.framebuffer_rgba16f_device_ptr())[0]
                packed = ctx.download(ptr, np.empty((K.H, K.W, 4), np.uint8 if fmt == "srgb8" else np.uint16))
                if binning == "scan":     # packed-only frames: the same bytes, no f32 target
                    ctx.set_packed_only(True)
                    ctx.render(h, va, s, download=False)
                    ctx.synchronize()
                    ptr = (ctx.framebuffer_srgb8_device_ptr() if fmt == "srgb8" else ctx.framebuffer_rgba16f_device_ptr())[0]
                    only = ctx.download(ptr, np.empty((K.H, K.W, 4), np.uint8 if fmt == "srgb8" else np.uint16))
                    ctx.set_packed_only(False)
                    assert same_bits(only, packed)
    finally:
        h.free()
    bad = (got.view(np.uint32) != twin.view(np.uint32)).any(axis=2) & untouched
    assert not bad.any(), f"{int(bad.sum())} untouched pixels differ from the twin, first at (y, x) = {np.argwhere(bad)[0].tolist()}"
    assert not same_bits(got, twin)           # (the splats are there)
    if packed is not None:
        want = _packed_of(oracle, got, fmt)           # the whole frame: a conversion of the final pixel
        assert same_bits(packed, want.astype(packed.dtype))
        want_twin = _packed_of(oracle, twin, fmt)
        assert np.array_equal(packed[untouched], want_twin.astype(packed.dtype)[untouched])


# ---- 3. a constant attachment is a clear colour; a depth-only frame does not look at the colour plane ----------------------
@pytest.mark.parametrize("samples", [1, 2, 4, 8])
def test_a_constant_attachment_is_a_clear_colour(ctx, binning, samples):
    """Colour plane = k everywhere against the frame with clear_color = k and the same depth plane: C + mean_s(T_s k) against
    C + k mean_s(T_s), each (S + 2) half-ulps of |C| + |k| from the exact value at the most (the twin's rounding model, where
    the clear-colour frame has fewer roundings still)."""
    k = 0.7
    c, s = K.cloud(), K.settings()
    depth = K.depth_plane(samples)
    h = ctx.upload(c)
    try:
        with attached(ctx, K.view(samples), depth, np.full((K.H, K.W, samples, 4), k, np.float32)) as va:
            over = ctx.render(h, va, s)
        with attached(ctx, K.view(samples, clear=(k, k, k, k)), depth, None) as vd:
            clear = ctx.render(h, vd, s)
        with attached(ctx, K.view(samples), depth, None) as vd:
            C = ctx.render(h, vd, s)      # transparent clear: the splats' own contribution, alpha = 1 - mean T
        # reserved[0] = 0 with the pair's address: the depth plane alone, whatever lies behind it
        plain = []
        for seed in (7, 8):
            with attached(ctx, K.view(samples, clear=(k, k, k, k)), depth, K.color_plane(samples, seed), flag=False) as vp:
                plain.append(ctx.render(h, vp, s))
                plain.append(ctx.render(h, vp, s))
    finally:
        h.free()
    assert all(same_bits(p, clear) for p in plain)
    bound = (samples + 2) * K.HALF_ULP * (np.abs(C.astype(np.float64)) + k)
    err = np.abs(over.astype(np.float64) - clear.astype(np.float64))
    print(f"[constant attachment x{samples} {binning}] largest |over - clear| / bound: {(err / bound).max():.3f}, "
          f"values that differ: {(err > 0).mean():.2%}")
    assert (err <= bound).all(), float((err / bound).max())
    assert np.abs(over - C).max() > 0.1       # (k shows)


# ---- 4. per-sample transmittance against the oracle --------------------------------------------------------------------------
_T4 = ([(v, sm, False) for v in sorted(VARIANTS) for sm in (1, 4)] + [("obb3d", 2, False), ("obb3d", 8, False), ("obb3d", 4, True)])


@pytest.mark.parametrize("variant,samples,bbox", _T4, ids=[f"{v}-x{sm}{'-bbox' if b else ''}" for v, sm, b in _T4])
def test_per_sample_transmittance_against_the_oracle(ctx, oracle, binning, variant, samples, bbox):
    """expected = C + sum_s T_s d_s / S with everything from the oracle: C from its frame over a transparent clear, and T_s
    from a frame whose depth plane is the case's at sample s and occluding at every other sample — occluded samples keep
    T = 1, so that frame's alpha is (1 - T_s) / S. Compared as every image is, 1e-3 + 1e-4 |ref| + amb, with amb = amb_C +
    sum_s |d_s| amb_s / S (amb_s: the bound on T_s, S times the bound on that frame's alpha). The share of pixels that pass
    only through amb stays within the share the plain depth-attached frame of the same case needs."""
    S = samples
    c, v = K.cloud(), K.view(S)
    s = K.settings(visualize_bounding_box=bbox, **VARIANTS[variant])
    depth, color = K.depth_plane(S), K.color_plane(S)
    C, amb_C, e = oracle_frame(oracle, S, variant, bbox)
    T = np.empty((K.H, K.W, S), np.float64)
    amb = amb_C.astype(np.float64).copy()
    for k in range(S):
        dk = np.full((K.H, K.W, S), K.OCCLUDING, np.float32)
        dk[..., k] = depth[..., k]
        rk, ak = oracle.render(c, e, v, s, with_ambiguity=True, depth=dk)
        T[..., k] = 1.0 - S * rk[..., 3].astype(np.float64)
        amb += np.abs(color[:, :, k, :]).max(axis=2) * (S * ak.astype(np.float64)) / S
    assert T.min() > -1e-5 and T.max() <= 1.0
    mixed = K.mixed_pixels(S)
    if S > 1:
        assert (np.ptp(T[mixed], axis=1) > 0.05).any(), "pixels whose samples see different transmittances"
    expected = K.composite_float64(C, T, color)
    if S > 1:
        assert np.abs(expected - (C.astype(np.float64) + (1.0 - C[..., 3:4]) * color.mean(axis=2))).max() > 1e-2, \
            "the case tells mean_s(T_s d_s) from mean_s(T_s) mean_s(d_s)"
    h = ctx.upload(c)
    try:
        with attached(ctx, v, depth, color) as va:
            got = ctx.render(h, va, s)
            st = ctx.stats()
        with attached(ctx, K.view(S), depth, None) as vd:
            plain = ctx.render(h, vd, s)
            st_plain = ctx.stats()
    finally:
        h.free()
    assert st["algorithmic_bytes"] - st_plain["algorithmic_bytes"] == K.W * K.H * S * 16
    ok, share, worst = only_through_amb(expected, got, amb)
    ok_p, share_p, worst_p = only_through_amb(C, plain, amb_C)
    print(f"[attachment {variant} x{S} bbox={bbox} {binning}] pixels through amb only: {share:.4f} (plain depth-attached frame: "
          f"{share_p:.4f}); largest error {worst:.2e} (plain {worst_p:.2e})")
    assert np.isfinite(got).all() and ok_p and ok, (worst, worst_p)
    assert share <= share_p, (share, share_p)


# ---- 5. a second cloud over a first ------------------------------------------------------------------------------------------
def test_a_second_cloud_over_a_first(ctx, oracle, binning):
    """S = 1, nothing occludes: cloud A over a transparent clear, its f32 frame handed on as the colour plane (at one sample
    per pixel the layouts coincide), cloud B over it — against the oracle's draw of both clouds as one, A's entries in A's
    order, then B's in B's (indices offset by len(A)): the reference's two-entity draw order."""
    a, b = K.cloud(K.SEED), K.cloud(K.SEED + 1)
    s, v = K.settings(), K.view(1)
    both = PlanarGaussian3d(*(np.concatenate([getattr(a, f), getattr(b, f)]) for f in
                              ("position_visibility", "spherical_harmonic", "rotation", "scale_opacity")))
    ea, eb = oracle.sort(a, v, s), oracle.sort(b, v, s).copy()
    eb["index"] += len(a)
    ref, amb = oracle.render(both, np.concatenate([ea, eb]), v, s, with_ambiguity=True)
    depth = np.zeros((K.H, K.W, 1), np.float32)
    ha, hb = ctx.upload(a), ctx.upload(b)
    try:
        first = ctx.render(ha, v, s)
        alone = ctx.render(hb, v, s)
        with attached(ctx, K.view(1), depth, first.reshape(K.H, K.W, 1, 4)) as va:
            got = ctx.render(hb, va, s)
    finally:
        ha.free()
        hb.free()
    ok, share, worst = only_through_amb(ref, got, amb)
    print(f"[second cloud over a first, {binning}] pixels through amb only: {share:.4f}, largest error {worst:.2e}")
    assert ok, worst
    assert np.abs(got - first).max() > 0.1      # B shows
    assert np.abs(got - alone).max() > 0.1      # ... and so does A under it


# ---- 6. in flight and replayed -----------------------------------------------------------------------------------------------
def test_frames_in_flight_and_replayed_graphs_each_see_their_own_planes(ctx):
    """Three frames with three colour planes on three lanes, then the same from captured graphs: flag and address travel with
    the frame as the depth address does, so every frame equals its blocking twin bit for bit and a replay needs no new
    capture for another plane."""
    S = 4
    c, s = K.cloud(), K.settings()
    depth = K.depth_plane(S)
    h = ctx.upload(c)
    pairs, views, want = [], [], []
    try:
        for k in range(3):
            ptr, holder = ctx.upload_attachments(depth, K.color_plane(S, 7 + k))
            pairs.append(holder)
            v = K.view(S)
            v.depth_device_ptr, v.color_attachment = ptr, True
            views.append(v)
            want.append(ctx.render(h, v, s))
        assert not same_bits(want[0], want[1]) and not same_bits(want[1], want[2])

        def round_of(order):
            for k in order:
                ctx.render(h, views[k], s, download=False)
            for k in order:
                f32, _ = ctx.pipeline_pop()
                got = ctx.download(f32, np.empty((K.H, K.W, 4), np.float32))
                assert same_bits(got, want[k]), (order, k)

        ctx.set_profiling(0)
        ctx.set_async(True)
        ctx.set_pipeline_depth(3)
        round_of((0, 1, 2))
        round_of((2, 0, 1))
        ctx.set_graphs(True)
        c0, r0 = ctx.graph_counters()
        for order in ((0, 1, 2), (0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 1, 2)):   # every lane's graphs see every plane
            round_of(order)
        c1, r1 = ctx.graph_counters()
        print(f"[colour attachment under graphs] captures +{c1 - c0}, replays +{r1 - r0}")
        assert r1 - r0 >= 6 and (c1 - c0) + (r1 - r0) == 15 and c1 - c0 <= 6     # a capture per (lane, parity) at the most
    finally:
        restore(ctx)
        for p in pairs:
            ctx.device_free(p)
        h.free()
