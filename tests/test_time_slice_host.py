"""The time slice of a 4D cloud, the part that needs no GPU: the arithmetic — the g++ build of csrc_slice/slice_math.h (the
operations the HIP kernels run) against the numpy twin `slice_reference`, bit for bit; the twin against float64 linear
algebra; the colour fold against the reference's own formula; the fourth library's ABI, its headers and its host-side
validation; and that the other three libraries did not move."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import time_slice_cases as C
from bevy_gaussian_splatting_amd import (
    CloudSettings, PlanarGaussian4d, TimeSlicer, _build_id, _native, _native_query, _native_slice, _native_sparse,
    compute_covariance_3d, random_gaussians_4d_seeded, slice_float64, slice_reference)
from bevy_gaussian_splatting_amd import time_slice as TS
from test_native_binding import declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "bevy_gaussian_splatting_amd")
CSRC_SLICE = os.path.join(PKG, "csrc_slice")
SHIM_SRC = os.path.join(HERE, "host_shim", "slice_math_shim.cpp")
SHIM_LIB = os.path.join(HERE, "host_shim", "libslice_math_shim.so")
IMAGE_TOLERANCE = 1e-3          # the project's bar on an image value (tests/test_gpu_parity.py, helpers.tolerance_mask)


same_bits, same_values = C.same_bits, C.same_values


@pytest.fixture(scope="module")
def shim():
    """g++ build of slice_math.h, with the flags of helpers.shim()."""
    deps = [SHIM_SRC, os.path.join(CSRC_SLICE, "slice_math.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                        "-Wno-unknown-pragmas", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    lib = ctypes.CDLL(SHIM_LIB)
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    lib.shim_slice.argtypes = [u32] + [vp] * 5 + [f32] * 4 + [vp] * 5
    lib.shim_slice.restype = None
    for fn in (lib.shim_expf, lib.shim_cosf):
        fn.argtypes = [vp, u32, vp]
        fn.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _elementwise(fn):
    def call(a):
        a = np.ascontiguousarray(a, np.float32)
        out = np.empty_like(a)
        fn(_ptr(a), a.size, _ptr(out))
        return out
    return call


def shim_slice(lib, cloud, settings):
    n = len(cloud)
    outs = [np.full((n, w), np.float32(-77.0)) for w in (4, 48, 8, 1, 2)]
    lib.shim_slice(n, *(_ptr(p) for p in cloud.planes()), settings.global_scale, settings.time, settings.time_start, settings.time_stop,
                   *(_ptr(o) for o in outs))
    return outs


# ---- 1. the compiled arithmetic against the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(C.CASES))
def test_shim_equals_the_twin(shim, case):
    """5000 splats a case: the reference's random cloud; time_scale 0 and negative, zero quaternions, NaN / inf lanes and
    dt = 0; the probe cloud. With this host's expf and cosf handed to the twin EVERY lane is bit for bit; with the twin's
    own (float64, rounded) the arguments of exp and cos, and every lane of every splat that does not pass through them, are."""
    cloud = C.CASES[case]()
    pv, sh, cov, exponent, args = shim_slice(shim, cloud, C.SETTINGS)
    twin = slice_reference(cloud, C.SETTINGS, exp=_elementwise(shim.shim_expf), cos=_elementwise(shim.shim_cosf))
    assert same_bits(pv, twin.position_visibility) and same_bits(cov, twin.covariance_3d_opacity)
    assert same_values(sh, twin.spherical_harmonic)
    ref = C.reference(case)
    assert same_values(exponent[:, 0], ref.exponent) and same_values(args, ref.cosine_arguments)
    agree = (ref.mask == twin.mask) & ~C.near_the_mask(case)
    assert agree.mean() > 0.995
    lanes = [0, 1, 2, 3, 4, 5, 7]                                         # all but the opacity
    assert same_bits(cov[agree][:, lanes], ref.covariance_3d_opacity[agree][:, lanes])
    assert same_bits(pv[agree], ref.position_visibility[agree])
    masked = ~twin.mask
    assert same_bits(cov[masked], np.zeros((int(masked.sum()), 8), np.float32))                     # eight +0, not -0
    assert same_bits(pv[masked], np.ascontiguousarray(cloud.position_visibility[masked]))           # copied, NaNs and all
    assert same_bits(pv[:, 3], np.ascontiguousarray(cloud.position_visibility[:, 3]))
    assert (cov[:, 7].view(np.uint32) == 0).all()
    assert 0.02 < masked.mean() < 0.9
    if case == "edge":
        tt, t = cloud.timestamp_timescale, np.float32(C.SETTINGS.time)
        assert masked[tt[:, 1] == 0].all() and (tt[:, 1] == 0).sum() > 100            # cov_t = 0: -inf or NaN, masked
        assert ((tt[:, 1] == 0) & (tt[:, 0] == t)).sum() > 50
        zero_q = (cloud.isotropic_rotations[:, :4] == 0).all(axis=1)
        assert zero_q.sum() > 100 and masked[zero_q].all()
        still = (tt[:, 0] == t) & (tt[:, 1] != 0) & ~zero_q & np.isfinite(cloud.isotropic_rotations).all(axis=1) & np.isfinite(tt).all(axis=1)
        assert still.sum() > 50 and (ref.marginal[still] == 1).all() and not masked[still].any()    # dt = 0: exp(-0) = 1
        assert same_bits(pv[still], np.ascontiguousarray(cloud.position_visibility[still]))         # delta = c * 0
        assert np.isnan(ref.marginal).sum() > 100 and (tt[:, 1] < 0).sum() > 1000
    if case == "probe":
        assert same_bits(cov[~masked, 6], twin.marginal[~masked])                                   # 1 * m = m
        assert same_bits(sh[:, 0], twin.cosines[:, 0]) and same_bits(sh[:, 1], twin.cosines[:, 1])
        assert same_bits(sh[:, 2:], np.ascontiguousarray(cloud.spherindrical_harmonic[:, 2:48]))


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_few_splats_sit_at_the_mask(case):
    """The seeds of the cases: a splat whose float64 marginal lies within the math library's error of 0.05 may fall on
    either side on a device; such splats are left out there, and may be at most 0.5 % of a case."""
    near = C.near_the_mask(case)
    print(f"{case}: {int(near.sum())} of {near.size} splats within {C.EXP_ULP} ulp of the mask threshold")
    for n in C.SIZES[1:]:
        assert near[:n].sum() <= 0.005 * n, n


# ---- 2. the twin against float64 ------------------------------------------------------------------------------------------------
def _six(m):
    return np.stack([m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 1], m[:, 1, 2], m[:, 2, 2]], axis=1)


def test_twin_is_the_schur_complement():
    """The twin's covariance, mean offset and marginal against float64 linear algebra on the random case, the Schur
    complement taken by a solve rather than by the shader's division; and it is positive semidefinite.

    Bound: every entry of Sigma is a sum of four products of entries of M, themselves sums of four products: some 12
    roundings of 2^-24 on terms of size |q|^2 |q_r|^2 S_i S_j, and the division by cov_t brings the residue of cov12
    back to that size. 64 * 2^-24 of the entry's scale is taken; the scale is the float64 diagonal's."""
    cloud, ref, f = C.random(), C.reference("random"), C.float64("random")
    sigma = f.sigma
    solved = sigma[:, :3, :3] - sigma[:, :3, 3:] @ np.linalg.solve(sigma[:, 3:, 3:], sigma[:, 3:, :3])
    assert np.allclose(solved, f.covariance, rtol=1e-12, atol=1e-15)
    m = ref.mask
    scale = np.sqrt(np.einsum("nii->ni", sigma)[:, :3])
    bound = 64 * 2.0 ** -24 * _six(scale[:, :, None] * scale[:, None, :])
    err = np.abs(ref.covariance_3d_opacity[:, :6].astype(np.float64) - _six(f.covariance))
    assert m.sum() > 3000 and (err[m] <= bound[m]).all(), (err[m] / bound[m]).max()
    eig = np.linalg.eigvalsh(f.covariance[m])
    assert (eig >= -1e-12 * np.abs(eig).max(axis=1, keepdims=True)).all()
    assert np.allclose(ref.marginal[m], f.marginal[m], rtol=1e-5)
    delta = ref.position_visibility[:, :3].astype(np.float64) - cloud.position_visibility[:, :3]
    assert np.abs(delta[m] - f.delta_mean[m]).max() < 1e-4            # both are rounding residue (below), under an ulp of 20


def test_the_rotation_pair_scales_and_does_not_turn():
    """What the reference's formula is (slice_math.h): Sigma = M^T M = S (R^T R) S and R^T R = |q|^2 |q_r|^2 I for EVERY
    pair, so in float64 Sigma is diagonal, cov12 and delta_mean vanish, and the conditional covariance is
    |q|^2 |q_r|^2 diag((g s)^2) — for the reference's random pairs as much as for unit ones."""
    cloud, f = C.random(), C.float64("random")
    rot, so = cloud.isotropic_rotations.astype(np.float64), cloud.scale_opacity.astype(np.float64)
    norms = (rot[:, :4] ** 2).sum(axis=1) * (rot[:, 4:] ** 2).sum(axis=1)
    s = np.concatenate([C.SETTINGS.global_scale * so[:, :3], cloud.timestamp_timescale[:, 1:2].astype(np.float64)], axis=1)
    want = norms[:, None, None] * (s[:, :, None] * s[:, None, :]) * np.eye(4)
    assert np.abs(f.sigma - want).max() < 1e-14 * max(1.0, np.abs(want).max())
    assert np.abs(f.delta_mean).max() < 1e-11


def test_identity_rotations_and_a_pure_spatial_rotation():
    """Identity rotations give diag((g s)^2) and delta_mean = 0, exactly, in the twin. A pair (q, q_r) with
    q_r = (w, x, y, -z) of a unit q makes R = M_r M_l a rotation of space that leaves time alone (its last row and
    column are e_4), so cov12 = 0 and cov_t = time_scale^2: the slice is a known 3D cloud — by the paragraph above one
    with the scales g s and NO rotation: it equals compute_covariance_3d of the identity, and of the spatial rotation
    itself exactly where that cannot matter, on splats whose three scales are equal."""
    n = 600
    base = random_gaussians_4d_seeded(n, 7)
    rot = np.zeros((n, 8), np.float32)
    rot[:, 0] = rot[:, 4] = 1.0
    settings = CloudSettings(global_scale=0.5, time=0.3)
    ident = PlanarGaussian4d(base.position_visibility, base.spherindrical_harmonic, rot, base.scale_opacity, base.timestamp_timescale)
    r = slice_reference(ident, settings)
    gs = np.float32(0.5) * base.scale_opacity[:, :3]
    want = np.zeros((n, 6), np.float32)
    want[:, 0], want[:, 3], want[:, 5] = gs[:, 0] * gs[:, 0], gs[:, 1] * gs[:, 1], gs[:, 2] * gs[:, 2]
    m = r.mask
    assert m.sum() > 300 and same_bits(r.covariance_3d_opacity[m][:, :6], want[m])
    assert same_bits(r.position_visibility, base.position_visibility)                       # delta_mean = 0 exactly
    assert same_bits(want, compute_covariance_3d(np.tile(np.float32([1, 0, 0, 0]), (n, 1)), gs))

    cloud, q3 = spatial_rotation_cloud(n, 9)
    f = slice_float64(cloud, settings)
    R = pair_matrix(cloud.isotropic_rotations.astype(np.float64))
    assert np.abs(R[:, 3, :3]).max() < 1e-7 and np.abs(R[:, :3, 3]).max() < 1e-7 and np.abs(R[:, 3, 3] - 1).max() < 1e-7
    assert np.abs(np.linalg.det(R[:, :3, :3]) - 1).max() < 1e-6 and np.abs(R[:, :3, :3] - np.eye(3)).max() > 0.5   # a real turn
    gs = np.float32(0.5) * cloud.scale_opacity[:, :3]
    ident3 = compute_covariance_3d(np.tile(np.float32([1, 0, 0, 0]), (n, 1)), gs).astype(np.float64)
    assert np.abs(_six(f.covariance) - ident3).max() < 1e-6 and np.abs(f.sigma[:, :3, 3]).max() < 1e-7
    assert np.allclose(f.sigma[:, 3, 3], cloud.timestamp_timescale[:, 1].astype(np.float64) ** 2, rtol=1e-6)
    equal = np.arange(n) % 3 == 0                                                            # these have sx = sy = sz
    turned = compute_covariance_3d(q3, gs).astype(np.float64)
    assert np.abs(_six(f.covariance)[equal] - turned[equal]).max() < 1e-6
    assert np.abs(_six(f.covariance)[~equal] - turned[~equal]).max() > 1e-2                  # ... and only there


def pair_matrix(rot):
    ml, mr = TS._rotation_rows(rot)
    return np.stack([np.stack(row, axis=1) for row in mr], axis=1) @ np.stack([np.stack(row, axis=1) for row in ml], axis=1)


def spatial_rotation_cloud(n, seed, time_scale=(0.3, 1.0)):
    """A 4D cloud whose pairs are pure spatial rotations: unit q, q_r = (w, x, y, -z) (derived from the WGSL's M_l and
    M_r: the (3, 3) entry of M_r M_l is wr w + xr x + yr y - zr z, which is 1 only for that q_r, and the rest of the last
    row and column then vanish). Every third splat has three equal scales. Returns the cloud and its q [n, 4].

    The q are the sixteen unit quaternions (+-1/2, +-1/2, +-1/2, +-1/2), turns by 120 degrees about a diagonal: every
    product and sum of the contract is then exact but the squares of the scales, so the twin's covariance is
    diag((g s)^2) to the BIT and delta_mean is +-0. A renderer is not continuous in its input (a coverage decision flips
    on the last bit of a covariance), so the end-to-end test needs a slice whose equivalent 3D cloud is the same bits."""
    c = random_gaussians_4d_seeded(n, seed)
    pv, sh, rot, so, tt = (np.array(p) for p in c.planes())
    rot[:, :4] = np.where(rot[:, :4] < 0, np.float32(-0.5), np.float32(0.5))
    rot[:, 4:] = rot[:, :4] * np.float32([1, 1, 1, -1])
    so[::3, 1] = so[::3, 2] = so[::3, 0]
    tt[:, 1] = time_scale[0] + (time_scale[1] - time_scale[0]) * np.abs(tt[:, 1])
    return PlanarGaussian4d(pv, sh, rot, so, tt), np.ascontiguousarray(rot[:, :4])


# ---- 3. the colour fold ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "probe"])
def test_the_colour_fold(case):
    """Stated deviation 1: the colour evaluated from the twin's 48 folded float32 coefficients (float64 evaluation of
    spherical_harmonics_lookup) against the float64 evaluation of the reference's own spherindrical formula on the 144,
    for a random unit direction a splat. Bounded by the project's image tolerance."""
    cloud, ref, f = C.CASES[case](), C.reference(case), C.float64(case)
    d = np.random.default_rng(5).normal(size=(len(cloud), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    want = TS.color_4d_float64(cloud.spherindrical_harmonic, d, f.cosines)
    got = TS.color_3d_float64(ref.spherical_harmonic, d)
    err = np.abs(got - want)
    print(f"{case}: largest colour difference of the fold {err.max():.3e} (colours up to {np.abs(want).max():.2f})")
    assert want.shape == (len(cloud), 3) and np.abs(want).max() > 1.0 and err.max() <= IMAGE_TOLERANCE


# ---- 4. ABI and build ----------------------------------------------------------------------------------------------------------------
def test_the_library_exports_exactly_what_its_header_declares():
    lib = _native_slice.load()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _native_slice.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert defined == set(_native_slice.EXPORTED_SYMBOLS), sorted(defined ^ set(_native_slice.EXPORTED_SYMBOLS))
    assert len(defined) == 3 and all(hasattr(lib, n) for n in defined)
    assert lib.bgst_version() == (0 << 16) | 1 == _native_slice.ABI_VERSION
    readelf = shutil.which("readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    needed = subprocess.run([readelf, "-d", _native_slice.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libbgs" not in needed


def test_prototype_table_agrees_with_the_header():
    """What is this header's own; the table against the header, function by function, is tests/test_native_binding.py's."""
    declared = declarations(("bgs_slice.h",), "bgst_")
    assert [name for name, _, _ in declared] == ["bgst_version", "bgst_last_error", "bgst_slice"]
    header = open(os.path.join(ROOT, "include", "bgs_slice.h")).read()
    assert declared[2] == ("bgst_slice", "int", 15)
    assert (_native_slice.BGST_OK, _native_slice.BGST_EINVAL, _native_slice.BGST_ENOMEM, _native_slice.BGST_EHIP) == (0, -1, -2, -3)
    for name, value in (("BGST_VERSION_MAJOR", "0"), ("BGST_VERSION_MINOR", "1"), ("BGST_EINVAL", r"\(-1\)"), ("BGST_EHIP", r"\(-3\)")):
        assert re.search(r"#define %s %s" % (name, value), header)


def test_the_build_id_is_the_source_hash_and_the_other_three_did_not_move():
    """The built library carries its own id and nobody else's marker. The recipe of the hash and the table of libraries
    are tests/test_native_binding.py's, for all five."""
    spec = _build_id.LIBBGS_SLICE
    _native_slice.load()
    assert _build_id.library_build_id(_native_slice.LIB_PATH, spec) == _build_id.source_sha256(spec)
    data = open(_native_slice.LIB_PATH, "rb").read()
    assert b"BGS_BUILD_ID=" not in data and b"BGSQ_BUILD_ID=" not in data and b"BGSS_BUILD_ID=" not in data


def test_the_other_libraries_and_headers_do_not_know_of_this_one():
    for d in ("csrc", "csrc_query", "csrc_sparse"):
        for name in sorted(os.listdir(os.path.join(PKG, d))):
            path = os.path.join(PKG, d, name)
            if os.path.isfile(path) and (name.endswith((".hip", ".h", ".map", ".inc")) or name == "Makefile"):
                assert b"bgst_" not in open(path, "rb").read() and b"BGST_" not in open(path, "rb").read(), path
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name not in ("bgs_slice.h", "bgs_slice.hpp"):
            assert "bgst_" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert not any(n.startswith("bgst") for n in _native.EXPORTED_SYMBOLS + _native_query.EXPORTED_SYMBOLS + _native_sparse.EXPORTED_SYMBOLS)
    other = ("bgs" + "s_", "bgs" + "q_")       # the other two small libraries' prefixes
    new_files = [os.path.join(CSRC_SLICE, n) for n in os.listdir(CSRC_SLICE) if n.endswith((".hip", ".h", ".map")) or n == "Makefile"]
    new_files += [os.path.join(ROOT, "include", "bgs_slice.h"), os.path.join(ROOT, "include", "bgs_slice.hpp"),
                  os.path.join(PKG, "_native_slice.py"), os.path.join(PKG, "time_slice.py"), SHIM_SRC]
    for path in new_files:
        text = open(path).read()
        assert not any(p in text for p in other) and '"../csrc' not in text and '"bgs.h"' not in text, path


def test_header_is_plain_c_and_the_cpp_layer_is_standard_cpp17(tmp_path):
    c = tmp_path / "abi.c"
    c.write_text('#include "bgs_slice.h"\nint main(void) { return (int)bgst_version() == BGST_EINVAL '
                 "|| bgst_slice(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0.0f, 0.0f, 1.0f) != BGST_OK; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(c), "-o", str(tmp_path / "abi.o")], check=True)
    cpp = tmp_path / "host.cpp"
    cpp.write_text('#include "bgs_slice.hpp"\nint main() { const bgs::slice::TimeSettings s; '
                   "return s.global_scale == 1.0f && s.time == 0.0f && s.time_start == 0.0f && s.time_stop == 1.0f ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Wshadow", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(cpp), "-o", str(tmp_path / "host.o")], check=True)


def test_cpp_layer_carries_the_c_abis_errors(tmp_path):
    """bgs_slice.hpp linked against the library: a refusal of the C ABI that needs no device arrives as
    bgs::slice::Error with the status and the offender named; n == 0 is no error."""
    _native_slice.load()
    src = tmp_path / "tool.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bgs_slice.hpp"
int main() {
    namespace s = bgs::slice;
    s::Planes4d in; s::Planes3d out; s::TimeSettings t;
    t.time_stop = t.time_start;
    try { s::slice(0, nullptr, 4, in, out, t); std::printf("no error\n"); }
    catch (const s::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    t.time_stop = 2.0f;
    try { s::slice(0, nullptr, 4, in, out, t); std::printf("no error\n"); }
    catch (const s::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    try { s::slice(0, nullptr, 0, in, out, t); std::printf("ok\n"); }
    catch (const s::Error& e) { std::printf("%d %s\n", e.status(), e.what()); }
    return 0;
}
''')
    exe = tmp_path / "tool"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + CSRC_SLICE, "-lbgs_slice", "-Wl,-rpath," + CSRC_SLICE], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[0].startswith("-1 ") and "time_stop == time_start" in lines[0]
    assert lines[1].startswith("-1 ") and "position_visibility_device_ptr is NULL" in lines[1]
    assert lines[2] == "ok"


# ---- 5. validation without a device --------------------------------------------------------------------------------------------------
def test_validation_names_the_offender():
    lib = _native_slice.load()
    EINVAL, OK = _native_slice.BGST_EINVAL, _native_slice.BGST_OK
    f = ctypes.c_float
    names = ["position_visibility", "spherindrical_harmonic", "isotropic_rotations", "scale_opacity", "timestamp_timescale",
             "out_position_visibility", "out_spherical_harmonic", "out_covariance_3d_opacity"]
    good = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(8)]
    times = (f(1.0), f(0.5), f(0.0), f(1.0))

    def call(ptrs, n=4, t=times):
        return lib.bgst_slice(0, None, n, *ptrs, *t)

    for k, name in enumerate(names):
        assert call(good[:k] + [None] + good[k + 1:]) == EINVAL
        assert lib.bgst_last_error() == b"bgst_slice: %s_device_ptr is NULL" % name.encode()
        assert call(good[:k] + [ctypes.c_void_p(good[k].value + 8)] + good[k + 1:]) == EINVAL
        assert lib.bgst_last_error() == b"bgst_slice: %s_device_ptr must be a 16-byte aligned device address" % name.encode()
    for o in (5, 6, 7):
        for k in range(o):
            assert call(good[:o] + [good[k]] + good[o + 1:]) == EINVAL
            assert lib.bgst_last_error() == b"bgst_slice: %s_device_ptr is %s_device_ptr as well" % (names[o].encode(), names[k].encode())
    for k, name in enumerate(("global_scale", "time", "time_start", "time_stop")):
        for bad, shown in ((float("nan"), b"nan"), (float("inf"), b"inf"), (float("-inf"), b"-inf")):
            t = list(times)
            t[k] = f(bad)
            assert call(good, t=t) == EINVAL and lib.bgst_last_error() == b"bgst_slice: %s %s must be finite" % (name.encode(), shown)
            assert call([None] * 8, n=0, t=t) == EINVAL                                     # the settings are looked at first
    assert call(good, t=(f(1.0), f(0.5), f(0.25), f(0.25))) == EINVAL
    assert lib.bgst_last_error() == b"bgst_slice: time_stop == time_start (0.25): the duration is 0"
    assert call([None] * 8, n=0) == OK and lib.bgst_last_error() == b""                     # n == 0: no pointer is looked at
    assert lib.bgst_slice(-1, None, 4, *good, *times) == EINVAL and b"hip_device -1" in lib.bgst_last_error()
    # the twin refuses the same settings in the same words
    cloud = random_gaussians_4d_seeded(4, 1)
    with pytest.raises(ValueError, match="time_stop == time_start"):
        slice_reference(cloud, CloudSettings(time_start=0.25, time_stop=0.25))
    with pytest.raises(ValueError, match="time nan must be finite"):
        slice_reference(cloud, CloudSettings(time=float("nan")))
    with pytest.raises(ValueError, match="five planes"):
        TimeSlicer(0).slice(0, 0, [0] * 4, [0] * 3, CloudSettings())


def test_no_cpu_fallback_without_a_usable_device():
    import torch
    device = 99 if torch.cuda.is_available() else 0
    with pytest.raises(_native_slice.BgsSliceError) as ei:
        TimeSlicer(device).slice(0, 4, [0x1000 * (k + 1) for k in range(5)], [0x1000 * (k + 6) for k in range(3)], CloudSettings())
    assert ei.value.status == _native_slice.BGST_EHIP and f"no usable HIP device {device}" in str(ei.value)


def test_the_cloud_model():
    c = random_gaussians_4d_seeded(100, 3)
    assert [p.shape[1] for p in c.planes()] == [4, 144, 8, 4, 4] and c.nbytes() == 100 * 656 and len(c.slice(10, 30)) == 20
    assert all(p.dtype == np.float32 for p in c.planes())
    tt, so = c.timestamp_timescale, c.scale_opacity
    assert (tt[:, 2:] == 0).all() and tt[:, 0].min() >= 0 and tt[:, 0].max() <= 1 and tt[:, 1].min() < -0.5 < 0.5 < tt[:, 1].max()
    assert (c.position_visibility[:, 3] == 1).all() and np.abs(c.position_visibility[:, :3]).max() <= 20 and so[:, 3].max() <= 0.8
    assert same_bits(random_gaussians_4d_seeded(100, 3).spherindrical_harmonic, c.spherindrical_harmonic)
    with pytest.raises(ValueError):
        PlanarGaussian4d(c.position_visibility, c.spherindrical_harmonic[:, :48], c.isotropic_rotations, so, tt)
