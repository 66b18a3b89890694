"""The DEVICE build of the vertex stage (project_kernel / project_emit_kernel -> project_rank -> project_splat) against
its host twin, record by record: what enforces csrc/splat_math.h's arithmetic contract on the device. For every case of
tests/vertex_stage_cases.py one synchronous frame per binning mode is rendered at pipeline depth 1, its records, tile
rectangles, visible_count and color_max_bits are read back (bgs_debug_frame_records) and compared with the g++ build of
the same header (helpers.twin_project) — bit for bit, as uint32, every field but one:

  the 2.4 power of srgb_to_linear1. The device forms it as v_exp_f32(2.4f * v_log_f32(b)), the host build calls powf, so
  neither is the other's reference: the device's value is compared with b ** 2.4 in float64, b = (c + 0.055f) * (1 /
  1.055f) formed in float32 from the LinRec709Display frame's colour c (itself pinned bit for bit). With L = log2 b, a
  1-ulp v_log_f32, the rounded product by 2.4f and a 1-ulp v_exp_f32 allow about 2^-23 (1 + 2 ln2 max(1, |2.4 L|))
  relative; TWICE that is asserted. (The 1-ulp figures are those of AMD's instruction-set documentation; the measured
  ratio to the bound is in profiles/vertex_stage.md.) Below the 0.04045 knee there is no power: bit for bit.

A NaN lane (inputs are finite, but a scale of 7e4 overflows the AABB conic to inf - inf) must be a NaN on both sides;
its sign and payload are the platform's (x86 and gfx950 differ, cf. sort_key_kind) and are not compared."""
import copy
import math

import numpy as np
import pytest

import helpers as H
import vertex_stage_cases as VC
from bevy_gaussian_splatting_amd import GaussianSplattingPlugin, _native

pytestmark = pytest.mark.gpu

SRGB_WORST = {"ratio": 0.0}   # the largest |device - b^2.4| / bound seen in this run, and its input (printed per case)


def _frame(plugin, case, d, binning, color_space=None):
    """One synchronous frame of the case; returns bgs_debug_frame_records' output plus the frame's instance count."""
    settings = copy.copy(d["settings"])
    if color_space is not None:
        settings.color_space = color_space
    cloud = d["cloud"]
    plugin.set_pipeline_depth(1)
    plugin.set_async(False)
    plugin.set_binning(binning)
    handle = plugin.upload(cloud.to_f16()) if case.fmt == "f16" else plugin.upload(cloud, precompute_covariance_3d=(case.fmt == "cov3d"))
    entries = None
    try:
        chunk = None
        if d["kept"] is not None:
            entries = plugin.device_sorted_entries(1, handle)
            entries.upload(0, d["kept"])
            chunk = entries.chunk(0)
        plugin.render(handle, d["view"], settings, download=False, entries=chunk)
        out = plugin.debug_frame_records()
        out["instance_count"] = plugin.stats()["instance_count"]
    finally:
        plugin.set_binning("scan")
        if entries is not None:
            entries.free()
        handle.free()
    return out


def _same(dev: np.ndarray, twin: np.ndarray) -> np.ndarray:
    """uint32 lanes equal bit for bit, or both a NaN."""
    fd, ft = dev.view(np.float32), twin.view(np.float32)
    return (dev == twin) | (np.isnan(fd) & np.isnan(ft))


def _mismatches(name, what, dev, d, twin_records, drawn, skip=()):
    """Every (rank, field) whose device word is not the twin's, on the ranks the twin draws, as messages naming the splat."""
    names = {12: H.RECORD_FIELDS, 24: H.SURFEL_FIELDS}[twin_records.shape[1]]
    cols = [i for i, f in enumerate(names) if f not in skip]
    bad = ~_same(dev[:, cols], twin_records[:, cols]) & drawn[:, None]
    count = len(drawn)
    msgs = []
    for j, ci in zip(*np.nonzero(bad)):
        i = cols[ci]
        splat = int(d["draw_list"][count - 1 - j]["index"])
        msgs.append(f"{name} [{what}] rank {j} splat {splat} field {names[i]}: device 0x{int(dev[j, i]):08x} "
                    f"({dev[j, i:i + 1].view(np.float32)[0]!r}) twin 0x{int(twin_records[j, i]):08x} ({twin_records[j, i:i + 1].view(np.float32)[0]!r})")
    return msgs


def _assert_none(msgs, what):
    if msgs:
        print(f"{len(msgs)} mismatching fields ({what}):")
        for m in msgs[:40]:
            print("  " + m)
    assert not msgs, f"{len(msgs)} mismatching fields ({what}); first: {msgs[0]}"


def _color_max_bits(records, drawn) -> int:
    names = {12: H.RECORD_FIELDS, 24: H.SURFEL_FIELDS}[records.shape[1]]
    cols = [names.index(f) for f in H.COLOR_FIELDS]
    mags = np.abs(records[drawn][:, cols].view(np.float32))
    mags = mags[~np.isnan(mags)]                       # fmaxf drops a NaN
    return int(np.float32(mags.max()).view(np.uint32)) if mags.size else 0


def _check_frame(case, d, dev, what, scan, skip=()):
    tw, twin_records, twin_rects, drawn = d["twin"], d["records"], d["rects"], d["drawn"]
    count = tw["count"]
    assert dev["draw_count"] == count, f"{case.name} [{what}]: draw_count {dev['draw_count']}, the twin's list has {count}"
    assert dev["record_stride"] == 4 * twin_records.shape[1]
    assert dev["records"].shape == twin_records.shape
    if scan:
        assert dev["rects"] is not None
        bad = np.nonzero(dev["rects"] != twin_rects)[0]
        msgs = [f"{case.name} [{what}] rank {j} splat {int(d['draw_list'][count - 1 - j]['index'])} rect: device 0x{int(dev['rects'][j]):08x} "
                f"twin 0x{int(twin_rects[j]):08x}" for j in bad]
        _assert_none(msgs, f"{case.name} {what} rects")
    else:
        assert dev["rects"] is None
        assert dev["instance_count"] == H.twin_instances(tw), f"{case.name} [{what}]: instance_count"
    _assert_none(_mismatches(case.name, what, dev["records"], d, twin_records, drawn, skip), f"{case.name} {what} records")
    assert dev["visible_count"] == int(tw["visible"].sum()), f"{case.name} [{what}]: visible_count"
    own = (dev["rects"] != H.RECT_EMPTY) if scan else drawn        # the device's own drawn records
    assert dev["color_max_bits"] == _color_max_bits(dev["records"], own), f"{case.name} [{what}]: color_max_bits"


def _check_srgb(case, lin, dev, drawn):
    """The one tolerance (module docstring). `lin`: the LinRec709Display frame's records (pinned), `dev`: the sRGB frame's."""
    names = {12: H.RECORD_FIELDS, 24: H.SURFEL_FIELDS}[lin.shape[1]]
    cols = [names.index(f) for f in H.COLOR_FIELDS]
    c = np.ascontiguousarray(lin[drawn][:, cols]).view(np.float32)
    got = np.ascontiguousarray(dev[drawn][:, cols]).view(np.float32)
    below = c <= np.float32(0.04045)
    assert below.any() and (~below).any() and (np.abs(c) > 5).any()
    linear = c * (np.float32(1.0) / np.float32(12.92))
    # the knee is a compare on a bit-exact value: below it the device took the linear branch, bit for bit
    assert np.array_equal(got[below].view(np.uint32), linear[below].view(np.uint32)), f"{case.name}: colours below the sRGB knee"
    b = ((c + np.float32(0.055)) * (np.float32(1.0) / np.float32(1.055)))[~below]
    assert b.dtype == np.float32
    ref = b.astype(np.float64) ** 2.4
    bound = 2.0 * 2.0 ** -23 * (1.0 + 2.0 * math.log(2.0) * np.maximum(1.0, np.abs(2.4 * np.log2(b.astype(np.float64)))))
    ratio = np.abs(got[~below].astype(np.float64) - ref) / (bound * ref)
    k = int(np.argmax(ratio))
    print(f"sRGB {case.name}: {ratio.size} powers, max |device - b^2.4| / bound = {ratio[k]:.4f} at b = {b[k]!r} (c = {c[~below][k]!r}, "
          f"device {got[~below][k]!r}, float64 {ref[k]!r}, bound {bound[k] / 2.0 ** -23:.2f} x 2^-23 relative); largest c {np.abs(c).max()!r}")
    if ratio[k] > SRGB_WORST["ratio"]:
        SRGB_WORST.update(ratio=float(ratio[k]), b=float(b[k]), c=float(c[~below][k]), case=case.name)
    assert ratio[k] <= 1.0, f"{case.name}: the power at b = {b[k]!r} is {ratio[k]:.3f} x the derived bound off"
    # above the knee nothing took the linear branch (it would be off by far more than the bound unless b is near 1: then compare bits)
    assert not np.array_equal(got[~below].view(np.uint32), linear[~below].view(np.uint32))


@pytest.mark.parametrize("name", VC.CASE_NAMES)
def test_device_vertex_stage_equals_its_host_twin(plugin, name):
    case = VC.by_name(name)
    d = VC.twin_of(case)
    drawn = d["drawn"]
    scan = _frame(plugin, case, d, "scan")
    print(f"{name}: {d['twin']['count']} ranks, {int(drawn.sum())} drawn, {int(d['twin']['visible'].sum())} visible")
    _check_frame(case, d, scan, "scan", True)
    sort = _frame(plugin, case, d, "sort")
    _check_frame(case, d, sort, "sort", False)
    assert np.array_equal(scan["records"][drawn], sort["records"][drawn]), f"{name}: project_emit_kernel's records differ from project_kernel's"
    if case.srgb:
        ds = VC.twin_of(case, VC.SRGB)
        assert np.array_equal(ds["drawn"], drawn) and np.array_equal(ds["rects"], d["rects"])
        for binning, is_scan in (("scan", True), ("sort", False)):
            dev = _frame(plugin, case, ds, binning, VC.SRGB)
            # geometry, rects and counts as before; the colour against float64 below
            tw = ds["twin"]
            assert dev["draw_count"] == tw["count"] and dev["visible_count"] == int(tw["visible"].sum())
            if is_scan:
                assert np.array_equal(dev["rects"], ds["rects"])
            else:
                assert dev["instance_count"] == H.twin_instances(tw)
            _assert_none(_mismatches(name, f"sRGB {binning}", dev["records"], ds, ds["records"], drawn, skip=H.COLOR_FIELDS), f"{name} sRGB {binning} geometry")
            _check_srgb(case, scan["records"], dev["records"], drawn)
            assert dev["color_max_bits"] == _color_max_bits(dev["records"], drawn)


def test_frame_records_hook_refuses_what_it_cannot_answer():
    case = VC.by_name("ranks_257")
    d = VC.twin_of(case)
    with GaussianSplattingPlugin(0) as p:
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_records()
        h = p.upload(d["cloud"])
        p.sort(h, d["view"], d["settings"])
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_records()
        p.render(h, d["view"], d["settings"])
        out = p.debug_frame_records()
        assert out["draw_count"] == 257 and out["record_stride"] == 48 and out["rects"].shape == (257,)
        import ctypes
        info = _native.BgsFrameRecordsInfo()
        small = np.zeros(257 * 12 - 1, np.uint32)
        rects = np.zeros(257, np.uint32)
        rc = p._lib.bgs_debug_frame_records(p._ctx, small.ctypes.data_as(ctypes.c_void_p), small.nbytes,
                                            rects.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 257, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_records holds" in p._lib.bgs_last_error(p._ctx) and not small.any()
        full = np.zeros(257 * 12, np.uint32)
        rc = p._lib.bgs_debug_frame_records(p._ctx, full.ctypes.data_as(ctypes.c_void_p), full.nbytes,
                                            rects.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 256, ctypes.byref(info))
        assert rc == _native.BGS_EINVAL and b"host_rects holds" in p._lib.bgs_last_error(p._ctx)
        p.radix_sort_pairs(np.arange(10, dtype=np.uint32))        # rewrites the lane's scratch region
        with pytest.raises(_native.BgsError, match="no frame has been rendered"):
            p.debug_frame_records()
        p.render(h, d["view"], d["settings"])
        p.set_pipeline_depth(2)
        with pytest.raises(_native.BgsError, match="pipeline depth"):
            p.debug_frame_records()
        p.set_async(True)
        p.render(h, d["view"], d["settings"], download=False)
        with pytest.raises(_native.BgsError):
            p.debug_frame_records()
        p.synchronize()
        h.free()
