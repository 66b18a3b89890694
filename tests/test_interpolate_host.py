"""The morph between two clouds, the part that needs no GPU: the arithmetic — the g++ build of csrc_morph/morph_math.h (the
operations the HIP kernels run) against the numpy twin `interpolate_reference`, bit for bit; the factor's known answers;
the twin against float64; the end points; the same header under the sanitizers as a program of its own; the fifth
library's ABI, its headers and its host-side validation; and that the other four libraries did not move."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import interpolate_cases as C
from bevy_gaussian_splatting_amd import (
    CloudSettings, GaussianInterpolator, _build_id, _native, _native_morph, _native_query, _native_slice, _native_sparse,
    interpolate_reference, interpolation_factor, random_gaussians_3d_seeded)
from bevy_gaussian_splatting_amd import interpolate as I
from test_native_binding import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "bevy_gaussian_splatting_amd")
CSRC_MORPH = os.path.join(PKG, "csrc_morph")
SHIM_SRC = os.path.join(HERE, "host_shim", "morph_math_shim.cpp")
SHIM_LIB = os.path.join(HERE, "host_shim", "libmorph_math_shim.so")
TOOL_SRC = os.path.join(HERE, "cpp", "morph_math_tool.cpp")
WIDTHS = {"f32": (4, 48, 4, 4), "cov3d": (4, 48, 8)}

same_bits, same_values, same_numbers = C.same_bits, C.same_values, C.same_numbers


@pytest.fixture(scope="module")
def shim():
    """g++ build of morph_math.h, with the flags of helpers.shim()."""
    deps = [SHIM_SRC, os.path.join(CSRC_MORPH, "morph_math.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                        "-Wno-unknown-pragmas", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    lib = ctypes.CDLL(SHIM_LIB)
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    lib.shim_factor.argtypes = [f32, f32, f32, vp, vp]
    lib.shim_interpolate_f32.argtypes = [u32] + [vp] * 8 + [f32] * 3 + [vp] * 4
    lib.shim_interpolate_cov3d_f32.argtypes = [u32] + [vp] * 6 + [f32] * 3 + [vp] * 3
    for fn in (lib.shim_factor, lib.shim_interpolate_f32, lib.shim_interpolate_cov3d_f32):
        fn.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def shim_factor(lib, time, start, stop):
    t, u = np.zeros(1, np.float32), np.zeros(1, np.float32)
    lib.shim_factor(time, start, stop, _ptr(t), _ptr(u))
    return t[0], u[0]


def shim_interpolate(lib, layout, lhs, rhs, settings):
    n = lhs[0].shape[0]
    outs = [np.full((n, w), np.float32(-77.0)) for w in WIDTHS[layout]]
    fn = lib.shim_interpolate_f32 if layout == "f32" else lib.shim_interpolate_cov3d_f32
    fn(n, *(_ptr(p) for p in lhs), *(_ptr(p) for p in rhs), settings.time, settings.time_start, settings.time_stop, *(_ptr(o) for o in outs))
    return outs


# ---- 1. the compiled arithmetic against the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("case", C.CASES)
def test_shim_equals_the_twin(shim, case, layout):
    """5000 splats a case, every setting, both layouts: the bit patterns where the value is not NaN, NaN-ness where it is."""
    lhs, rhs = C.sides(case, layout)
    for name in C.SETTINGS:
        got = shim_interpolate(shim, layout, lhs, rhs, C.settings(name))
        want = C.reference(case, layout, name)
        assert len(got) == len(want) == len(WIDTHS[layout])
        for k, (g, w) in enumerate(zip(got, want)):
            assert same_values(g, w), f"{case} {layout} {name}: plane {k}"
        t, u = shim_factor(shim, *C.SETTINGS[name][0])
        assert same_bits(np.float32([t, u]), np.float32([C.factor(name), np.float32(1.0) - C.factor(name)])), name
    if case == "edge":
        # the case does what it says: NaNs come out, and not everywhere
        nan = np.isnan(C.reference(case, layout, "inside")[2])
        assert 50 < nan.any(axis=1).sum() < 0.5 * C.N


# ---- 2. the factor ---------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_factor(shim):
    """interpolate.wgsl:51-57: the clamped quotient, backwards over a reversed interval, the step where |duration| < 1e-6
    (time >= time_stop gives 1), and that threshold from both sides. The header's function and the twin's, to the bit."""
    factor = lambda time, start, stop: interpolation_factor(CloudSettings(time=time, time_start=start, time_stop=stop))
    assert factor(0.25, 0.0, 1.0) == 0.25 and factor(0.25, 1.0, 0.0) == 0.75
    assert factor(-2.0, 0.0, 1.0) == 0.0 and factor(5.0, 0.0, 1.0) == 1.0
    assert factor(2.0, 1.0, 0.0) == 0.0 and factor(-1.0, 1.0, 0.0) == 1.0
    assert factor(0.4, 0.5, 0.5) == 0.0 and factor(0.5, 0.5, 0.5) == 1.0 and factor(0.6, 0.5, 0.5) == 1.0
    assert float(np.float32(C.JUST_UNDER)) < float(np.float32(1e-6))
    assert factor(5e-7, 0.0, 1e-6) == 0.5 and factor(5e-7, 0.0, C.JUST_UNDER) == 0.0 and factor(C.JUST_UNDER, 0.0, C.JUST_UNDER) == 1.0
    for name, (times, want) in C.SETTINGS.items():
        t = factor(*times)
        assert t.dtype == np.float32 and (0.0 < t < 1.0 if want is None else same_bits(t, np.float32(want))), name
        assert same_bits(np.float32(shim_factor(shim, *times)), np.float32([t, np.float32(1.0) - t])), name
    for times, want in C.FACTOR_CORNERS:
        t = factor(*times)
        assert same_bits(t, np.float32(want)), times                       # a clamped -0 is +0: bits, not numbers
        assert same_bits(np.float32(shim_factor(shim, *times)), np.float32([t, np.float32(1.0) - t])), times
    for bad in ("time", "time_start", "time_stop"):
        with pytest.raises(ValueError, match=f"{bad} (nan|inf) must be finite"):
            interpolation_factor(CloudSettings(**{bad: float("nan") if bad == "time" else float("inf")}))


# ---- 3. the twin against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_twin_against_float64(layout):
    """Every mixed lane is within 4 * 2^-23 * max(|a|, |b|) of the float64 blend: four roundings (u = 1 - t, the two
    products, the sum) of at most half an ulp each of a quantity no larger than that maximum, doubled for slack.
    Normalised rotations have float64 norm within 4 * 2^-23 of 1."""
    lhs, rhs = C.sides("random", layout)
    for name in ("inside", "offset", "reversed", "half"):
        twin, f64 = C.reference("random", layout, name), C.float64("random", layout, name)
        mixed = [0, 1, 3] if layout == "f32" else [0, 1, 2]
        worst = 0.0
        for k in mixed:
            lanes = slice(0, 7) if (layout, k) == ("cov3d", 2) else slice(None)
            scale = np.maximum(np.abs(lhs[k]), np.abs(rhs[k])).astype(np.float64)[:, lanes]
            err = np.abs(twin[k].astype(np.float64) - f64[k])[:, lanes]
            assert (err <= 4 * 2.0 ** -23 * scale).all(), (name, k)
            worst = max(worst, float((err / np.where(scale > 0, scale, 1.0)).max()))
        line = f"random {layout} {name}: largest error of a mixed lane {worst / 2.0 ** -23:.3f} x 2^-23 of max(|a|, |b|) (bound 4)"
        if layout == "f32":
            norm = np.sqrt((twin[2].astype(np.float64) ** 2).sum(axis=1))
            assert (np.abs(norm - 1.0) <= 4 * 2.0 ** -23).all()
            line += f"; largest | |q| - 1 | {np.abs(norm - 1.0).max() / 2.0 ** -23:.3f} x 2^-23 (bound 4)"
        print(line)


# ---- 4. end points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_end_points(case):
    """t = 0 gives the lhs and t = 1 the rhs as numbers (a -0 may come out +0) wherever BOTH sides' lanes are finite: the
    other side's inf or NaN times 0 is NaN, as in the shader. The rotation is the twin's normalisation of that side's."""
    for name, side in (("zero", 0), ("before", 0), ("step_before", 0), ("one", 1), ("after", 1), ("step_at", 1)):
        planes, other = C.sides(case, "f32")[side], C.sides(case, "f32")[1 - side]
        got = C.reference(case, "f32", name)
        for k in (0, 1, 3):
            finite = np.isfinite(other[k])
            assert same_numbers(got[k][finite], planes[k][finite]), (name, k)
            assert np.isnan(got[k][~finite]).all()
        finite = np.isfinite(other[2]).all(axis=1)
        assert same_numbers(got[2][finite], I.normalize_quaternion_reference(np.ascontiguousarray(planes[2][finite])))
        assert np.isnan(got[2][~finite]).all()
        cov, cov_other = C.sides(case, "cov3d")[side], C.sides(case, "cov3d")[1 - side]
        got = C.reference(case, "cov3d", name)
        finite = np.isfinite(cov_other[2][:, :7])
        assert same_numbers(got[2][:, :7][finite], cov[2][:, :7][finite])
    if case == "random":
        assert same_numbers(C.reference(case, "f32", "zero")[0], C.sides(case, "f32")[0][0])          # no lane left out there
        assert same_numbers(C.reference(case, "f32", "one")[1], C.sides(case, "f32")[1][1])


def test_the_antipodal_fallback_and_the_pad_lane():
    """rhs.rotation = -lhs.rotation at t = 0.5: the mixed quaternion is exactly 0 on every splat and every stored row
    becomes (0, 0, 0, 1) — z = 1 in this project's [w, x, y, z], as the reference has it. At 0.25 it is 0.5 * lhs,
    normalised. In the covariance layout lane 7 is +0 whatever stood there in the inputs."""
    lhs, rhs = C.sides("antipodal", "f32")
    assert same_bits(rhs[2], -lhs[2]) and (np.abs(np.log2(np.abs(lhs[2]))) <= 3).all()
    half = C.reference("antipodal", "f32", "half")
    assert same_bits(half[2], np.tile(np.float32([0, 0, 0, 1]), (C.N, 1)))
    quarter = C.reference("antipodal", "f32", "quarter")
    assert same_bits(quarter[2], I.normalize_quaternion_reference(np.float32(0.5) * lhs[2]))
    assert not np.isnan(quarter[2]).any()
    for case in C.CASES:
        l, r = C.sides(case, "cov3d")
        assert (l[2][:, 7] == 3.25).all() and np.isnan(r[2][::7, 7]).all() and (r[2][1::7, 7] == -1).all()
        for name in ("inside", "zero", "one", "reversed"):
            assert (C.reference(case, "cov3d", name)[2][:, 7].view(np.uint32) == 0).all(), (case, name)
    # the zero quaternions of the edge case: on both sides the fallback at every t; on one side the other's direction
    l, r = C.sides("edge", "f32")
    both = (l[2] == 0).all(axis=1) & (r[2] == 0).all(axis=1)
    inside = C.reference("edge", "f32", "inside")[2]
    assert both.sum() > 50 and same_bits(inside[both], np.tile(np.float32([0, 0, 0, 1]), (int(both.sum()), 1)))
    one_side = (l[2] == 0).all(axis=1) & ~both & np.isfinite(r[2]).all(axis=1)
    assert one_side.sum() > 50
    # (0 * u + r * t, normalised, against r normalised: one rounding of the product and some three of each normalisation,
    # 2^-24 each on lanes of at most 1: 8 * 2^-24)
    assert np.abs(inside[one_side] - I.normalize_quaternion_reference(np.ascontiguousarray(r[2][one_side]))).max() <= 8 * 2.0 ** -24
    tiny = (np.abs(l[2]) <= 1e-25).all(axis=1) & (np.abs(r[2]) <= 1e-25).all(axis=1) & ~both      # len2 underflows to 0
    assert tiny.sum() > 50 and same_bits(inside[tiny], np.tile(np.float32([0, 0, 0, 1]), (int(tiny.sum()), 1)))


def test_the_twin_refuses_what_is_no_pair():
    a, b = random_gaussians_3d_seeded(8, 1), random_gaussians_3d_seeded(9, 2)
    with pytest.raises(ValueError, match="equal length"):
        interpolate_reference(a, b, CloudSettings())
    with pytest.raises(ValueError, match="different layouts"):
        interpolate_reference(a, I.covariance_planes(a), CloudSettings())
    with pytest.raises(ValueError, match="four planes"):
        interpolate_reference(I.planes_of(a)[:2], I.planes_of(a)[:2], CloudSettings())
    with pytest.raises(ValueError, match="four planes"):
        GaussianInterpolator(0).interpolate(0, 0, [0] * 4, [0] * 4, [0] * 3, CloudSettings())


# ---- 5. the header under the sanitizers, as a program of its own ------------------------------------------------------------------
def _tool_run(exe, tmp_path, tag, layout, lhs, rhs, triples):
    n = lhs[0].shape[0]
    src, dst = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    with open(src, "wb") as f:
        f.write(struct.pack("<3I", n, len(lhs), len(triples)))
        f.write(np.float32(triples).tobytes())
        for p in tuple(lhs) + tuple(rhs):
            f.write(np.ascontiguousarray(p, np.float32).tobytes())
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    data = np.fromfile(dst, np.float32)
    per = 2 + n * sum(WIDTHS[layout])
    assert data.size == per * len(triples)
    out = []
    for k in range(len(triples)):
        rec, at, planes = data[k * per:(k + 1) * per], 2, []
        for w in WIDTHS[layout]:
            planes.append(rec[at:at + n * w].reshape(n, w))
            at += n * w
        out.append((rec[0], rec[1], planes))
    return out


def test_the_header_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/morph_math_tool.cpp: g++ -fsanitize=address,undefined -fno-sanitize-recover, a main of its own, no Python
    in the process. It blends the edge case in both layouts and takes the factor's corner values; what it writes is the
    twin's, and it ends clean."""
    exe = tmp_path / "morph_math_tool"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover", "-Wall", "-Werror", "-Wno-unknown-pragmas", TOOL_SRC, "-o", str(exe)],
                   check=True, capture_output=True)
    names = ("inside", "zero", "one", "reversed", "step_at", "tiny_before")
    triples = [C.SETTINGS[name][0] for name in names]
    for layout in C.LAYOUTS:
        lhs, rhs = C.sides("edge", layout)
        for name, (t, u, planes) in zip(names, _tool_run(exe, tmp_path, layout, layout, lhs, rhs, triples)):
            want = C.reference("edge", layout, name)
            assert same_bits(np.float32([t, u]), np.float32([C.factor(name), np.float32(1.0) - C.factor(name)]))
            assert all(same_values(np.ascontiguousarray(g), w) for g, w in zip(planes, want)), (layout, name)
    corners = [times for times, _ in C.FACTOR_CORNERS]
    empty = tuple(np.zeros((0, w), np.float32) for w in WIDTHS["f32"])
    got = _tool_run(exe, tmp_path, "corners", "f32", empty, empty, corners)
    for (times, want), (t, u, _) in zip(C.FACTOR_CORNERS, got):
        assert same_bits(np.float32([t, u]), np.float32([want, np.float32(1.0) - np.float32(want)])), times


# ---- 6. ABI and build ----------------------------------------------------------------------------------------------------------------
NAMES = ["bgsm_version", "bgsm_last_error", "bgsm_interpolate_f32", "bgsm_interpolate_cov3d_f32"]


def test_the_library_exports_exactly_what_its_header_declares():
    lib = _native_morph.load()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _native_morph.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert defined == set(_native_morph.EXPORTED_SYMBOLS) == set(NAMES), sorted(defined ^ set(NAMES))
    assert len(defined) == 4 and all(hasattr(lib, n) for n in defined)
    assert lib.bgsm_version() == (0 << 16) | 1 == _native_morph.ABI_VERSION
    readelf = shutil.which("readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    needed = subprocess.run([readelf, "-d", _native_morph.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libbgs" not in needed


def test_prototype_table_agrees_with_the_header():
    """What is this header's own; the table against the header, function by function, is tests/test_native_binding.py's."""
    declared = declarations(("bgs_morph.h",), "bgsm_")
    assert [name for name, _, _ in declared] == NAMES
    header = open(os.path.join(ROOT, "include", "bgs_morph.h")).read()
    assert declared[2] == ("bgsm_interpolate_f32", "int", 18) and declared[3] == ("bgsm_interpolate_cov3d_f32", "int", 15)
    assert (_native_morph.BGSM_OK, _native_morph.BGSM_EINVAL, _native_morph.BGSM_ENOMEM, _native_morph.BGSM_EHIP) == (0, -1, -2, -3)
    for name, value in (("BGSM_VERSION_MAJOR", "0"), ("BGSM_VERSION_MINOR", "1"), ("BGSM_EINVAL", r"\(-1\)"), ("BGSM_ENOMEM", r"\(-2\)"),
                        ("BGSM_EHIP", r"\(-3\)")):
        assert re.search(r"#define %s %s" % (name, value), header)
    assert "ORDERING" in header and "bgs_cloud_upload_f32" in header and "bgs_cloud_upload_cov3d_f32" in header


def test_the_build_id_is_the_source_hash_and_the_other_four_did_not_move():
    """The library's directory holds these files and no other source (what the small libraries share lives in small_lib/),
    and the built library carries its own id and nobody else's marker. The recipe of the hash, the table of libraries
    and the compiler flags are tests/test_native_binding.py's, for all five."""
    spec = _build_id.LIBBGS_MORPH
    _native_morph.load()
    assert _build_id.library_build_id(_native_morph.LIB_PATH, spec) == _build_id.source_sha256(spec)
    assert sorted(n for n in os.listdir(CSRC_MORPH) if n.endswith((".hip", ".h", ".map")) or n == "Makefile") == [
        "Makefile", "bgs_morph_api.hip", "libbgs_morph.map", "morph_kernels.h", "morph_kernels.hip", "morph_math.h"]
    data = open(_native_morph.LIB_PATH, "rb").read()
    for marker in (b"BGS_BUILD_ID=", b"BGSQ_BUILD_ID=", b"BGSS_BUILD_ID=", b"BGST_BUILD_ID="):
        assert marker not in data


def test_the_other_libraries_and_headers_do_not_know_of_this_one():
    for d in ("csrc", "csrc_query", "csrc_sparse", "csrc_slice"):
        for name in sorted(os.listdir(os.path.join(PKG, d))):
            path = os.path.join(PKG, d, name)
            if os.path.isfile(path) and (name.endswith((".hip", ".h", ".map", ".inc")) or name == "Makefile"):
                assert b"bgsm_" not in open(path, "rb").read() and b"BGSM_" not in open(path, "rb").read(), path
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name not in ("bgs_morph.h", "bgs_morph.hpp"):
            text = open(os.path.join(ROOT, "include", name)).read()
            assert "bgsm_" not in text and "BGSM_" not in text, name
    others = _native.EXPORTED_SYMBOLS + _native_query.EXPORTED_SYMBOLS + _native_sparse.EXPORTED_SYMBOLS + _native_slice.EXPORTED_SYMBOLS
    assert not any(n.startswith("bgsm") for n in others)
    other = ("bgs" + "s_", "bgs" + "q_", "bgs" + "t_")       # the other three small libraries' prefixes
    new_files = [os.path.join(CSRC_MORPH, n) for n in os.listdir(CSRC_MORPH) if n.endswith((".hip", ".h", ".map")) or n == "Makefile"]
    new_files += [os.path.join(ROOT, "include", "bgs_morph.h"), os.path.join(ROOT, "include", "bgs_morph.hpp"),
                  os.path.join(PKG, "_native_morph.py"), os.path.join(PKG, "interpolate.py"), SHIM_SRC, TOOL_SRC]
    for path in new_files:
        text = open(path).read()
        assert not any(p in text or p.upper() in text for p in other) and '"../csrc' not in text and '"bgs.h"' not in text, path


def test_header_is_plain_c_and_the_cpp_layer_is_standard_cpp17(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "bgs_morph.h"\nint main(void) { return (int)bgsm_version() == BGSM_EINVAL '
                 "|| bgsm_interpolate_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.0f, 1.0f) != BGSM_OK "
                 "|| bgsm_interpolate_cov3d_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.5f, 0.0f, 1.0f) != BGSM_OK; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)
    cpp = tmp_path / "host.cpp"
    cpp.write_text('#include "bgs_morph.hpp"\nint main() { const bgs::morph::TimeSettings s; bgs::morph::PlanesF32<const void*> p; '
                   "return s.time == 0.0f && s.time_start == 0.0f && s.time_stop == 1.0f && !p.rotation ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(cpp), "-o", str(tmp_path / "host.o")], check=True)


def test_cpp_layer_carries_the_c_abis_errors(tmp_path):
    """bgs_morph.hpp linked against the library: a refusal of the C ABI that needs no device arrives as
    bgs::morph::Error with the status and the offender named; n == 0 is no error, nor is time_stop == time_start."""
    _native_morph.load()
    src = tmp_path / "tool.cpp"
    src.write_text(r'''
#include <cstdio>
#include <limits>
#include "bgs_morph.hpp"
int main() {
    namespace m = bgs::morph;
    m::PlanesF32<const void*> lhs, rhs; m::PlanesF32<void*> out; m::TimeSettings t;
    m::PlanesCov3d<const void*> clhs, crhs; m::PlanesCov3d<void*> cout;
    t.time_start = std::numeric_limits<float>::infinity();
    try { m::interpolate(0, nullptr, 4, lhs, rhs, out, t); std::printf("no error\n"); }
    catch (const m::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    t.time_start = t.time_stop;
    try { m::interpolate(0, nullptr, 4, lhs, rhs, out, t); std::printf("no error\n"); }
    catch (const m::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    try { m::interpolate(0, nullptr, 4, clhs, crhs, cout, t); std::printf("no error\n"); }
    catch (const m::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    try { m::interpolate(0, nullptr, 0, lhs, rhs, out, t); m::interpolate(0, nullptr, 0, clhs, crhs, cout, t); std::printf("ok\n"); }
    catch (const m::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    return 0;
}
''')
    exe = tmp_path / "tool"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + CSRC_MORPH, "-lbgs_morph", "-Wl,-rpath," + CSRC_MORPH], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[0] == "-1 bgsm_interpolate_f32: time_start inf must be finite"
    assert lines[1] == "-1 bgsm_interpolate_f32: lhs_position_visibility_device_ptr is NULL"
    assert lines[2] == "-1 bgsm_interpolate_cov3d_f32: lhs_position_visibility_device_ptr is NULL"
    assert lines[3] == "ok"


# ---- 7. validation without a device --------------------------------------------------------------------------------------------------
PLANES = {"f32": ["position_visibility", "spherical_harmonic", "rotation", "scale_opacity"],
          "cov3d": ["position_visibility", "spherical_harmonic", "covariance_3d_opacity"]}


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_validation_names_the_offender(layout):
    """Every BGSM_EINVAL path by its message. hip_device is -1 throughout: a call that got past the validation would say
    so (that check is the last before a device is touched), so no device was."""
    lib = _native_morph.load()
    EINVAL, OK = _native_morph.BGSM_EINVAL, _native_morph.BGSM_OK
    f = ctypes.c_float
    fn_name = "bgsm_interpolate_f32" if layout == "f32" else "bgsm_interpolate_cov3d_f32"
    fn, tag = getattr(lib, fn_name), fn_name.encode()
    per = len(PLANES[layout])
    names = [f"{side}_{plane}".encode() for side in ("lhs", "rhs", "out") for plane in PLANES[layout]]
    count = len(names)
    good = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(count)]
    times = (f(0.5), f(0.0), f(1.0))

    def call(ptrs, n=4, t=times, device=-1):
        return fn(device, None, n, *ptrs, *t)

    for k, name in enumerate(names):
        assert call(good[:k] + [None] + good[k + 1:]) == EINVAL
        assert lib.bgsm_last_error() == b"%s: %s_device_ptr is NULL" % (tag, name)
        assert call(good[:k] + [ctypes.c_void_p(good[k].value + 8)] + good[k + 1:]) == EINVAL
        assert lib.bgsm_last_error() == b"%s: %s_device_ptr must be a 16-byte aligned device address" % (tag, name)
    for o in range(2 * per, count):
        for k in range(o):
            assert call(good[:o] + [good[k]] + good[o + 1:]) == EINVAL
            assert lib.bgsm_last_error() == b"%s: %s_device_ptr is %s_device_ptr as well" % (tag, names[o], names[k])
    for k, name in enumerate((b"time", b"time_start", b"time_stop")):
        for bad, shown in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf")):
            t = list(times)
            t[k] = f(bad)
            assert call(good, t=t) == EINVAL and lib.bgsm_last_error() == b"%s: %s %s must be finite" % (tag, name, shown)
            assert call([None] * count, n=0, t=t) == EINVAL                                 # the times are looked at first
    # what is NOT an error reaches the last check, the device's number: the validation let it through, and nothing was touched
    past = b"%s: hip_device -1" % tag
    assert call(good) == EINVAL and lib.bgsm_last_error() == past
    assert call(good, t=(f(0.5), f(0.25), f(0.25))) == EINVAL and lib.bgsm_last_error() == past          # time_stop == time_start: the step
    assert call(good, t=(f(0.5), f(1.0), f(0.0))) == EINVAL and lib.bgsm_last_error() == past            # a reversed interval
    assert call(good[:per] + good[:per] + good[2 * per:]) == EINVAL and lib.bgsm_last_error() == past    # a side given twice
    assert call([None] * count, n=0) == OK and lib.bgsm_last_error() == b""                 # n == 0: no pointer is looked at
    assert call([None] * count, n=0, device=-1) == OK


def test_no_cpu_fallback_without_a_usable_device():
    import torch
    device = 99 if torch.cuda.is_available() else 0
    for per in (4, 3):
        ptrs = [[0x1000 * (per * s + k + 1) for k in range(per)] for s in range(3)]
        with pytest.raises(_native_morph.BgsMorphError) as ei:
            GaussianInterpolator(device).interpolate(0, 4, *ptrs, CloudSettings())
        assert ei.value.status == _native_morph.BGSM_EHIP and f"no usable HIP device {device}" in str(ei.value)


def test_the_package_exports_the_surface():
    import bevy_gaussian_splatting_amd as pkg
    for name in ("GaussianInterpolator", "interpolate_reference", "interpolation_factor"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert all(hasattr(pkg.GaussianSplattingPlugin, m) for m in ("interpolate", "morph_pair"))
