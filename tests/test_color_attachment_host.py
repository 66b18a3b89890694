"""The view's colour attachment (bgs_view.reserved[0] = BGS_VIEW_ATTACH_COLOR), the parts that need no GPU: the seam's two
constants, the Python view's marshalling, the colour plane's offset in Python and in include/bgs.hpp, and the numpy twin of
the resolve against a float64 evaluation."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import color_attachment_cases as K
from bevy_gaussian_splatting_amd import View, color_attachment_offset, composite_reference
from bevy_gaussian_splatting_amd import camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_the_header_names_the_two_values():
    text = open(os.path.join(ROOT, "include", "bgs.h")).read()
    for name, value in (("BGS_VIEW_ATTACH_DEPTH_ONLY", 0), ("BGS_VIEW_ATTACH_COLOR", 1)):
        m = re.findall(rf"^#define\s+{name}\s+(\d+)u\s*$", text, re.M)
        assert m == [str(value)], (name, m)
    assert (camera.VIEW_ATTACH_DEPTH_ONLY, camera.VIEW_ATTACH_COLOR) == (0, 1)
    # the word keeps its name and place: one uint32 between entry_count and depth_device_ptr
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"uint32_t\s+entry_count;\s*uint32_t\s+reserved\[1\];", code)
    fields = [f[0] for f in camera.BgsView._fields_]
    assert fields[fields.index("entry_count") + 1] == "reserved" and fields[fields.index("reserved") + 1] == "depth_device_ptr"
    assert camera.BgsView.reserved.size == 4


def test_to_native_writes_the_flag():
    v = View.headless(K.W, K.H)
    assert v.color_attachment is False
    assert v.to_native().reserved[0] == 0          # what every existing caller passes
    v.depth_device_ptr = 0x7F0000001000
    assert v.to_native().reserved[0] == 0          # a depth plane alone
    v.color_attachment = True
    n = v.to_native()
    assert n.reserved[0] == 1 and n.depth_device_ptr == 0x7F0000001000
    assert ctypes.sizeof(n) == ctypes.sizeof(View.headless(8, 8).to_native())


@pytest.mark.parametrize("whs", [(1, 1, 1), (3, 1, 1), (5, 3, 1), (7, 5, 2), (K.W, K.H, 1), (K.W, K.H, 8), (41, 23, 1),
                                 (1920, 1080, 4), (4095, 4093, 1), (4096, 4096, 8)])
def test_the_offset_is_the_next_multiple_of_16_behind_the_depth_plane(whs):
    w, h, s = whs
    off = color_attachment_offset(w, h, s)
    assert off % 16 == 0 and 0 <= off - w * h * s * 4 < 16


def test_python_and_cpp_agree_on_the_offset(tmp_path):
    """g++ build of include/bgs.hpp (no HIP on the include path): bgs::color_attachment_offset for odd w * h * S, and the
    flag through bgs::View."""
    cases = [(1, 1, 1), (3, 1, 1), (5, 3, 1), (7, 5, 1), (41, 23, 1), (4095, 4093, 1), (K.W, K.H, 4), (4096, 4096, 8), (333, 77, 1)]
    src = tmp_path / "offset.cpp"
    calls = "\n".join(f'    std::printf("%llu\\n", (unsigned long long)bgs::color_attachment_offset({w}, {h}, {s}));' for w, h, s in cases)
    src.write_text('#include <cstdio>\n#include "bgs.hpp"\n'
                   "static_assert(bgs::color_attachment_offset(3, 1, 1) == 16, \"constexpr\");\n"
                   "int main() {\n" + calls + "\n"
                   "    bgs::View v;\n"
                   '    std::printf("%u ", v.native.reserved[0]);\n'
                   "    v.set_color_attachment(true);\n"
                   '    std::printf("%u %d ", v.native.reserved[0], (int)v.color_attachment());\n'
                   "    v.set_color_attachment(false);\n"
                   '    std::printf("%u\\n", v.native.reserved[0]);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "offset"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [int(x) for x in out[:len(cases)]] == [color_attachment_offset(*c) for c in cases]
    assert any((w * h * s) % 2 == 1 for w, h, s in cases)
    assert out[len(cases)].split() == ["0", "1", "1", "0"]


@pytest.mark.parametrize("samples", [1, 2, 4, 8])
def test_the_twin_against_float64(samples):
    """composite_reference against C + mean_s(T_s d_s) in float64, within the twin's own rounding model: (S + 2) half-ulps
    of the largest magnitude a term or partial sum reaches (color_attachment_cases.twin_bound). Largest observed share of
    that bound, 200 000 pixels per sample count (T in [0, 1], d in [0, 2), C in [-1, 3)): 0.498 / 0.296 / 0.158 / 0.082 at
    S = 1 / 2 / 4 / 8."""
    rng = np.random.default_rng(100 + samples)
    n = 200_000
    T = rng.random((n, samples), dtype=np.float32)
    T[: n // 8] = 1.0                                   # pixels nothing reached
    T[n // 8: n // 4, ::2] = 0.0                        # samples a saturated fragment covers
    dst = (2.0 * rng.random((n, samples, 4), dtype=np.float32)).astype(np.float32)
    C = (4.0 * rng.random((n, 4), dtype=np.float32) - 1.0).astype(np.float32)
    C[: n // 8] = 0.0
    got = composite_reference(C, T, dst)
    assert got.dtype == np.float32 and got.shape == (n, 4)
    want = K.composite_float64(C, T, dst)
    err = np.abs(got.astype(np.float64) - want)
    bound = K.twin_bound(C, T, dst)
    share = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[twin vs float64, S = {samples}] largest error / bound: {share:.3f}")
    assert (err <= bound).all(), share
    # a pixel nothing reached is the left-to-right f32 sum of its samples times 1/S, bit for bit
    acc = dst[: n // 8, 0, :].copy()
    for s in range(1, samples):
        acc = acc + dst[: n // 8, s, :]
    assert acc.dtype == np.float32
    assert np.array_equal(got[: n // 8], acc * np.float32(1.0 / samples))


def test_the_twin_refuses_shapes_that_do_not_belong_together():
    with pytest.raises(ValueError):
        composite_reference(np.zeros((3, 4), np.float32), np.ones((3, 4), np.float32), np.zeros((3, 2, 4), np.float32))
