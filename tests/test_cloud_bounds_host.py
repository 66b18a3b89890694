"""The cloud's own bounds (BGS_BOUNDS_CLOUD, bgs_settings.reserved[0]), the part that needs no GPU: the arithmetic of
csrc/bounds_math.h — the operations the HIP kernel and the host's decode run — built with g++ and compared bit for bit with
the numpy twin `bounds_reference`; the same header as a stand-alone program under the address and undefined-behaviour
sanitizers; the twin against float64; the order-preserving encoding; the struct, the defaults and the C++ layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bevy_gaussian_splatting_amd import CloudSettings, bounds_reference
from bevy_gaussian_splatting_amd.bounds import (
    BOUNDS_CALLER, BOUNDS_CLOUD, bounds_grid, bounds_key, bounds_key_bits, bounds_single_sweep_reach)
from bevy_gaussian_splatting_amd.settings import BgsSettings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")
SHIM_SRC = os.path.join(HERE, "host_shim", "bounds_shim.cpp")
SHIM_LIB = os.path.join(HERE, "host_shim", "libbounds_shim.so")
GXX_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror"]
PARTS = (1, 3, 64, 256, 1000)   # how many interleaved partial results stand in for the device's lanes and workgroups


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def inputs():
    """name -> [n, 4] float32 positions (w: a visibility the reduction must not read)."""
    rng = np.random.default_rng(77)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    random5000 = np.concatenate([rng.normal(0, 7, (5000, 3)), rng.uniform(0, 1, (5000, 1))], axis=1).astype(np.float32)
    special = np.array([
        [nan, 1.0, -2.0, 1.0],
        [0.5, nan, -inf, 0.0],
        [-0.0, 0.0, 3.0, nan],
        [0.0, -0.0, nan, -inf],
        [inf, -3.5, 1e-45, inf],
        [-1e-45, 1e-39, -1e-39, 1.0],
        [2.0, -inf, 4.0, 0.5],
    ], np.float32)
    special[0, 0] = _f32(0xFFC00001)      # a negative quiet NaN with a payload
    special[1, 1] = _f32(0x7F800001)      # a signalling NaN
    zeros = np.array([[-0.0, 0.0, -0.0, 1.0], [0.0, -0.0, -0.0, 1.0]], np.float32)
    all_nan_axis = random5000[:300].copy()
    all_nan_axis[:, 1] = nan
    w_poison = random5000[:257].copy()
    w_poison[:, 3] = np.where(np.arange(257) % 2, nan, -inf)
    return {"random5000": random5000, "special": special, "zeros": zeros, "all_nan_axis": all_nan_axis,
            "single": np.array([[0.3, 1.2, -4.0, 1.0]], np.float32), "w_poison": w_poison}


@pytest.fixture(scope="module")
def shim():
    deps = [SHIM_SRC, os.path.join(CSRC, "bounds_math.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(["g++", *GXX_FLAGS, "-shared", "-fPIC", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    lib = ctypes.CDLL(SHIM_LIB)
    lib.shim_bounds_reference.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    lib.shim_bounds_reference.restype = None
    lib.shim_bounds_device_order.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.shim_bounds_device_order.restype = None
    lib.shim_bounds_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_bounds_decode.restype = None
    for name in ("shim_bounds_key", "shim_bounds_key_bits"):
        getattr(lib, name).argtypes = [ctypes.c_uint32]
        getattr(lib, name).restype = ctypes.c_uint32
    lib.shim_bounds_grid.argtypes = [ctypes.c_uint32] * 3
    lib.shim_bounds_grid.restype = ctypes.c_uint32
    return lib


def twin_bits(pv):
    lo, hi = bounds_reference(pv)
    assert lo.dtype == hi.dtype == np.float32 and lo.shape == hi.shape == (3,)
    return np.concatenate([lo, hi]).view(np.uint32)


def shim_bits(lib, pv, parts=None):
    pv = np.ascontiguousarray(pv, np.float32)
    out = np.zeros(6, np.float32)
    if parts is None:
        lib.shim_bounds_reference(pv.ctypes.data_as(ctypes.c_void_p), pv.shape[0], out.ctypes.data_as(ctypes.c_void_p))
    else:
        lib.shim_bounds_device_order(pv.ctypes.data_as(ctypes.c_void_p), pv.shape[0], parts, out.ctypes.data_as(ctypes.c_void_p))
    return out.view(np.uint32)


# ---- 1. twin vs compiled header --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(inputs()))
def test_the_compiled_header_equals_the_numpy_twin_bit_for_bit(shim, name):
    """Both routes of the header: the fold as the reference writes it (offset per splat, one splat after the other) and the
    device's (raw coordinates in interleaved partial results, merged as integer keys, offset once) — the monotonicity
    argument of bounds_math.h, on every input."""
    pv = inputs()[name]
    want = twin_bits(pv)
    assert np.array_equal(shim_bits(shim, pv), want), name
    for parts in PARTS:
        assert np.array_equal(shim_bits(shim, pv, parts), want), (name, parts)
    # the visiting order does not matter either
    rng = np.random.default_rng(5)
    shuffled = pv[rng.permutation(pv.shape[0])]
    assert np.array_equal(twin_bits(shuffled), want)
    assert np.array_equal(shim_bits(shim, shuffled, 64), want)


def test_what_the_special_inputs_must_give():
    inf = np.float32(np.inf)
    f = np.float32
    lo, hi = bounds_reference(inputs()["all_nan_axis"])
    assert lo[1] == inf and hi[1] == -inf and np.isfinite(lo[[0, 2]]).all() and np.isfinite(hi[[0, 2]]).all()
    lo, hi = bounds_reference(inputs()["special"])
    assert lo[0] == f(-1e-45) - f(0.1) and hi[0] == inf                   # NaN skipped, +inf propagates
    assert lo[1] == -inf and hi[1] == f(1.0) + f(0.1)
    assert lo[2] == -inf and hi[2] == f(4.0) + f(0.1)
    lo, hi = bounds_reference(inputs()["zeros"])                           # a zero -+ 0.1 is never a zero: no sign to carry
    assert lo.view(np.uint32).tolist() == [int(f(-0.1).view(np.uint32))] * 3
    assert hi.view(np.uint32).tolist() == [int(f(0.1).view(np.uint32))] * 3
    lo, hi = bounds_reference(inputs()["single"])
    assert lo.tolist() == [float(f(0.3) - f(0.1)), float(f(1.2) - f(0.1)), float(f(-4.0) - f(0.1))]
    assert hi.tolist() == [float(f(0.3) + f(0.1)), float(f(1.2) + f(0.1)), float(f(-4.0) + f(0.1))]
    # the visibility lane is not read, and a bare [n, 3] plane is the same cloud
    pv = inputs()["w_poison"]
    assert np.array_equal(twin_bits(pv), twin_bits(pv[:, :3]))
    assert bounds_reference(np.zeros((0, 4), np.float32)) is None


def test_the_header_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """bounds_shim.cpp with its own main, built with -fsanitize=address,undefined and run on the same inputs: clean exit,
    nothing on stderr, and the twin's bits on stdout for both routes."""
    exe = tmp_path / "bounds_shim_san"
    subprocess.run(["g++", *GXX_FLAGS, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBOUNDS_SHIM_MAIN",
                    SHIM_SRC, "-o", str(exe)], check=True, capture_output=True)
    for name, pv in inputs().items():
        path = tmp_path / (name + ".bin")
        np.ascontiguousarray(pv, np.float32).tofile(path)
        want = twin_bits(pv).tolist()
        for parts in (1, 64, 1000):
            r = subprocess.run([str(exe), str(path), str(parts)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and r.stderr == "", (name, parts, r.stderr)
            got = [int(w, 16) for w in r.stdout.split()]
            assert got == want + want, (name, parts)


# ---- 2. twin vs float64 ----------------------------------------------------------------------------------------------
def test_the_twin_is_within_one_ulp_of_float64():
    pv = inputs()["random5000"]
    lo, hi = bounds_reference(pv)
    xyz = pv[:, :3].astype(np.float64)
    for got, exact in ((lo, xyz.min(axis=0) - 0.1), (hi, xyz.max(axis=0) + 0.1)):
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - exact) <= ulp).all(), (got, exact)


# ---- 3. the encoding -------------------------------------------------------------------------------------------------
def test_the_encoding_round_trips_and_is_monotone(shim):
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                     0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3DCCCCCD, 0xBDCCCCCD], np.uint32)
    bits = np.concatenate([bits, edge])
    keys = bounds_key(bits)
    assert np.array_equal(bounds_key_bits(keys), bits)
    for b in edge.tolist() + bits[:200].tolist():
        assert shim.shim_bounds_key(b) == int(bounds_key(np.uint32(b))) and shim.shim_bounds_key_bits(shim.shim_bounds_key(b)) == b
    values = bits.view(np.float32)
    ordered = bits[~np.isnan(values)]
    # the order of the floats, -0 below +0: sort by (value, sign clear)
    v = ordered.view(np.float32)
    ordered = ordered[np.lexsort((~(ordered >> 31).astype(bool), v))]
    k = bounds_key(ordered).astype(np.int64)
    assert (np.diff(k) >= 0).all()
    v = ordered.view(np.float32)
    strictly = np.diff(v.astype(np.float64)) > 0
    assert (np.diff(k)[strictly] > 0).all()
    assert int(bounds_key(np.uint32(0x80000000))) + 1 == int(bounds_key(np.uint32(0)))          # -0 right below +0
    assert int(bounds_key(np.uint32(0xFF800000))) == 0x007FFFFF and int(bounds_key(np.uint32(0x7F800000))) == 0xFF800000
    # every non-NaN key beats the presets of the device words (all-ones for a min, zero for a max)
    assert 0 < k.min() and k.max() < 0xFFFFFFFF
    # words still at their presets decode to an empty axis: +inf / -inf (the offset leaves them there)
    words = np.array([0xFFFFFFFF] * 3 + [0] * 3, np.uint32)
    out = np.zeros(6, np.float32)
    shim.shim_bounds_decode(words.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert out.tolist() == [np.inf] * 3 + [-np.inf] * 3


def test_the_grid_arithmetic_is_the_headers(shim):
    for n in (1, 255, 256, 257, 5000, 131072, 131073, 5_000_000):
        for cus in (1, 104, 256, 304):
            for cap in (0, 1, 2, 7, 100000):
                assert bounds_grid(n, cus, cap) == shim.shim_bounds_grid(n, cus, cap) >= 1, (n, cus, cap)
    assert bounds_grid(5_000_000, 256) == 512 and bounds_single_sweep_reach(256) == 131072    # two workgroups on every CU
    assert bounds_single_sweep_reach(256, 2) == 512


# ---- 4. struct and defaults ------------------------------------------------------------------------------------------
def test_the_struct_is_unchanged_and_the_flag_is_the_reserved_word():
    assert ctypes.sizeof(BgsSettings) == (16 + 2 + 8 + 1 + 1 + 2 + 8) * 4
    assert BgsSettings.reserved.offset == (16 + 2 + 11) * 4 and BgsSettings.reserved.size == 4
    assert BgsSettings.visualize_bounding_box.offset == BgsSettings.reserved.offset - 4
    assert BgsSettings.position_min.offset == BgsSettings.reserved.offset + 4
    assert BgsSettings.position_max.offset == BgsSettings.position_min.offset + 16
    assert CloudSettings().bounds_from_cloud is False
    assert CloudSettings().to_native().reserved[0] == 0 == BOUNDS_CALLER
    flagged = CloudSettings(bounds_from_cloud=True, position_min=(1, 2, 3), position_max=(4, 5, 6)).to_native()
    assert flagged.reserved[0] == 1 == BOUNDS_CLOUD
    assert list(flagged.position_min) == [1.0, 2.0, 3.0, 1.0] and list(flagged.position_max) == [4.0, 5.0, 6.0, 1.0]
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    assert re.search(r"#define\s+BGS_BOUNDS_CALLER\s+0u\b", header) and re.search(r"#define\s+BGS_BOUNDS_CLOUD\s+1u\b", header)
    assert re.search(r"#define BGS_VERSION_MINOR 9\b", header)
    body = header[header.index("typedef struct bgs_settings"):header.index("} bgs_settings;")]
    assert "uint32_t reserved[1];" in re.sub(r"/\*.*?\*/", "", body, flags=re.S)


def test_settings_default_still_writes_zero():
    from bevy_gaussian_splatting_amd import _native
    s = BgsSettings()
    s.reserved[0] = 7
    _native.load().bgs_settings_default(ctypes.byref(s))
    assert s.reserved[0] == 0


# ---- 5. the C++ layer ------------------------------------------------------------------------------------------------
def test_the_cpp_layer_toggles_the_word(tmp_path):
    src = tmp_path / "bounds.cpp"
    src.write_text('#include "bgs.hpp"\n'
                   "int main() { bgs::CloudSettings s; if (s.bounds_from_cloud() || s.to_native().reserved[0] != BGS_BOUNDS_CALLER) return 1;\n"
                   "  s.set_bounds_from_cloud(true); if (!s.bounds_from_cloud() || s.to_native().reserved[0] != BGS_BOUNDS_CLOUD) return 2;\n"
                   "  s.set_bounds_from_cloud(false); return s.to_native().reserved[0] == BGS_BOUNDS_CALLER ? 0 : 3; }\n")
    exe = tmp_path / "bounds_cpp"
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, capture_output=True)
    subprocess.run(["g++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L" + CSRC, "-lbgs", "-Wl,-rpath," + CSRC], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
