"""Particle behaviours, the part that needs no GPU: the record layout, the seeded generators, the host-side validation of
both layers, and the step's arithmetic — the g++ build of csrc/particle_math.h (the operations the HIP kernel runs)
against the numpy twin `step_reference`, bit for bit, and against literals worked out by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
from bevy_gaussian_splatting_amd import (
    PARTICLE_BEHAVIOR_DTYPE, ParticleBehaviors, _native, random_particle_behaviors, step_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc")
SHIM_SRC = os.path.join(HERE, "host_shim", "particle_math_shim.cpp")
SHIM_LIB = os.path.join(HERE, "host_shim", "libparticle_math_shim.so")
TOOL = os.path.join(HERE, "cpp", "particle_tool")
SYMBOL = "bgs_cloud_apply_particle_behaviors"
DTS = (0.0, 1.0 / 60.0, 0.25)


@pytest.fixture(scope="module")
def shim():
    """g++ build of particle_math.h, with the flags of helpers.shim()."""
    deps = [SHIM_SRC, os.path.join(CSRC, "particle_math.h")]
    if not os.path.exists(SHIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_LIB) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared", "-fPIC",
                        "-Wno-unknown-pragmas", SHIM_SRC, "-o", SHIM_LIB], check=True, capture_output=True)
    lib = ctypes.CDLL(SHIM_LIB)
    lib.shim_particle_step.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float]
    lib.shim_particle_step.restype = None
    lib.shim_particle_c6_bits.argtypes = []
    lib.shim_particle_c6_bits.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, capture_output=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", TOOL, os.path.join(HERE, "cpp", "particle_tool.cpp"),
                    "-L" + CSRC, "-lbgs", "-Wl,-rpath," + CSRC], check=True)
    return TOOL


def shim_step(lib, pv, rec, dt):
    pv, rec = np.array(pv, np.float32, copy=True), np.array(rec, copy=True)
    lib.shim_particle_step(pv.ctypes.data_as(ctypes.c_void_p), pv.shape[0], rec.ctypes.data_as(ctypes.c_void_p), rec.shape[0],
                           ctypes.c_float(dt))
    return pv, rec


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_entry_point_is_declared_bound_and_documented():
    """(tests/test_abi.py enforces the sets; this names the symbol so that a failure reads clearly)"""
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", header)
    assert "typedef struct bgs_particle_behavior" in header
    assert SYMBOL in _native.EXPORTED_SYMBOLS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index('extern "C" {'):]
    assert f"pub fn {SYMBOL}(" in block[:block.index("\n}")]
    assert hasattr(_native.load(), SYMBOL)
    assert _native.load().bgs_version() == H.header_version() == _native.ABI_VERSION


def test_record_layout_is_the_references_64_bytes(tool):
    d = PARTICLE_BEHAVIOR_DTYPE
    assert d.itemsize == 64
    assert [d.fields[k][1] for k in ("indicies", "velocity", "acceleration", "jerk")] == [0, 16, 32, 48]
    assert d.fields["indicies"][0].base == np.uint32 and d.fields["velocity"][0].base == np.float32
    lines = subprocess.run([tool, "layout"], capture_output=True, text=True, check=True).stdout.split("\n")
    assert lines[0].split() == lines[1].split() == ["64", "0", "16", "32", "48"]   # bgs::ParticleBehavior, bgs_particle_behavior


def _in_reference_ranges(r, n):
    assert r.shape == (n,)
    assert np.array_equal(r["indicies"][:, 0], np.arange(n, dtype=np.uint32)) and not r["indicies"][:, 1:].any()
    for field, lim in (("velocity", 1.0), ("acceleration", 0.01), ("jerk", 1e-4)):
        x = r[field]
        assert np.isfinite(x).all() and (np.abs(x) <= np.float32(lim)).all(), field
        # ... and it is that range, not a narrower one: a uniform draw of 4 n values reaches beyond 90 % of the limit
        assert x.max() > 0.9 * lim and x.min() < -0.9 * lim, field
        assert abs(float(x.mean())) < 0.05 * lim, field


def test_python_generator_is_seeded_and_within_the_references_ranges():
    a, b, c = random_particle_behaviors(2000, 7), random_particle_behaviors(2000, 7), random_particle_behaviors(2000, 8)
    assert isinstance(a, ParticleBehaviors) and len(a) == 2000 and a.n == 2000
    assert same_bits(a.records, b.records) and not same_bits(a.records, c.records)
    _in_reference_ranges(a.records, 2000)


def test_cpp_generator_is_seeded_and_within_the_references_ranges(tool, tmp_path):
    out = []
    for name, seed in (("a", 7), ("b", 7), ("c", 8)):
        subprocess.run([tool, "random", "2000", str(seed), str(tmp_path / name)], check=True)
        out.append(np.fromfile(tmp_path / name, PARTICLE_BEHAVIOR_DTYPE))
    assert same_bits(out[0], out[1]) and not same_bits(out[0], out[2])
    _in_reference_ranges(out[0], 2000)


def _records(indices):
    r = np.zeros(len(indices), PARTICLE_BEHAVIOR_DTYPE)
    r["indicies"][:, 0] = np.asarray(indices, np.int64).astype(np.uint32)
    return r


def test_python_validation_refuses_an_index_out_of_range_and_a_duplicate():
    ParticleBehaviors(_records([0, 5, 99, 0xFFFFFFFF, 0xFFFFFFFF]), 100)   # distinct, in range; inactive ones may repeat
    with pytest.raises(ValueError, match="names splat 100"):
        ParticleBehaviors(_records([0, 100]), 100)
    with pytest.raises(ValueError, match="same splat"):
        ParticleBehaviors(_records([3, 7, 3]), 100)
    with pytest.raises(TypeError):
        ParticleBehaviors(np.zeros((4, 16), np.float32), 100)


def test_cpp_validation_refuses_an_index_out_of_range_and_a_duplicate(tool, tmp_path):
    def run(indices, n):
        _records(indices).tofile(tmp_path / "r.bin")
        return subprocess.run([tool, "validate", str(tmp_path / "r.bin"), str(n)], capture_output=True, text=True)
    ok = run([0, 5, 99, 0xFFFFFFFF, 0xFFFFFFFF], 100)
    assert ok.returncode == 0 and ok.stdout.strip() == "ok"
    bad = run([0, 100], 100)
    assert bad.returncode == 1 and "names splat 100" in bad.stderr
    dup = run([3, 7, 3], 100)
    assert dup.returncode == 1 and "same splat" in dup.stderr


def test_the_compiled_arithmetic_equals_the_numpy_twin_bit_for_bit(shim):
    """4096 random records (the generator's ranges) on a 5000-splat plane, indices a random permutation with inactive
    (negative as int32) and out-of-range records mixed in, for dt = 0, 1/60 and 0.25, three steps in a row."""
    n, count = 5000, 4096
    rng = np.random.default_rng(11)
    rec = random_particle_behaviors(count, 3).records
    idx = rng.permutation(n)[:count].astype(np.uint32)
    idx[::97] = 0xFFFFFFFF
    idx[5::131] = n
    idx[7::149] = n + 7
    idx[11::151] = 0x80000000
    rec["indicies"][:, 0] = idx
    pv0 = np.concatenate([rng.uniform(-20, 20, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
    assert shim.shim_particle_c6_bits() == 0x3E2AAAAB == int(np.float32(1.0 / 6.0).view(np.uint32))
    for dt in DTS:
        pv_a, rec_a, pv_b, rec_b = pv0, rec, pv0, rec
        for _ in range(3):
            pv_a, rec_a = shim_step(shim, pv_a, rec_a, dt)
            pv_b, rec_b = step_reference(pv_b, rec_b, dt)
            assert same_bits(pv_a, pv_b) and same_bits(rec_a, rec_b), dt
        skipped = (idx.view(np.int32) < 0) | (idx >= n)
        assert skipped.sum() > 100 and same_bits(rec_b[skipped], rec[skipped])
        assert same_bits(rec_b["jerk"], rec["jerk"]) and same_bits(rec_b["indicies"], rec["indicies"])
        moved = np.zeros(n, bool)
        moved[idx[~skipped]] = True
        assert same_bits(pv_b[~moved], pv0[~moved])
        assert (dt == 0.0) == same_bits(pv_b, pv0)
    # the inputs are left unchanged
    assert same_bits(rec["indicies"][:, 0], idx)


def test_one_record_worked_out_by_hand(shim):
    """dt = 1/4, every product and sum exact in binary32 (c6 * 6 = 1.00000003 rounds to 1):
        lane x: p 10, v 1, a 2, j 6:      dp = 1/4 + (1 * 1/4 * 1/4) + (1 * 1/64) = 0.328125; dv = 1/2 + 3/16 = 0.6875; da = 1.5
        lane y: the same with every sign flipped
        lane z: p -3, v 0, a 0, j 0:      nothing moves
        lane w: p 0.75 (visibility), v -2, a 0, j 0:   dp = -1/2"""
    rec = np.zeros(2, PARTICLE_BEHAVIOR_DTYPE)
    rec["indicies"][:, 0] = (2, 0xFFFFFFFF)
    rec["velocity"][:] = (1, -1, 0, -2)
    rec["acceleration"][:] = (2, -2, 0, 0)
    rec["jerk"][:] = (6, -6, 0, 0)
    pv = np.zeros((4, 4), np.float32)
    pv[2] = (10, -10, -3, 0.75)
    pv[3] = (1, 2, 3, 4)
    for step in (lambda: shim_step(shim, pv, rec, 0.25), lambda: step_reference(pv, rec, 0.25)):
        p, r = step()
        assert p[2].tolist() == [10.328125, -10.328125, -3.0, 0.25]
        assert r["velocity"][0].tolist() == [1.6875, -1.6875, 0.0, -2.0]
        assert r["acceleration"][0].tolist() == [3.5, -3.5, 0.0, 0.0]
        assert r["jerk"][0].tolist() == [6.0, -6.0, 0.0, 0.0] and r["indicies"][0].tolist() == [2, 0, 0, 0]
        assert same_bits(r[1], rec[1])                                  # the inactive record: untouched
        assert same_bits(p[[0, 1, 3]], pv[[0, 1, 3]])                   # the splats nobody named: untouched
