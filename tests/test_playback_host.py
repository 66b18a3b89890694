"""How a playing cloud's time advances: `settings.playback_update` against cases worked by hand (the reference's
`playback_update`, src/gaussian/settings.rs:145-191, in f32 in the order it is written), its Sin mode against a float64
evaluation within a bound derived below, and the C++ twin of include/bgs_host.hpp against the Python on the same cases.
No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

from bevy_gaussian_splatting_amd import CloudSettings, PlaybackMode, playback_update

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
U = 2.0 ** -24          # the unit roundoff of binary32: a rounded result r of an operation is exact * (1 + d), |d| <= U


def run(mode, time, scale=1.0, start=0.0, stop=1.0, delta=0.0, elapsed=0.0, steps=1):
    s = CloudSettings(playback_mode=mode, time=time, time_scale=scale, time_start=start, time_stop=stop)
    for _ in range(steps):
        playback_update(s, delta, elapsed)
    return s.time


# ---- the modes and the defaults ---------------------------------------------------------------------------------------------------
def test_the_modes_are_the_references_and_still_is_the_default():
    assert [m.name for m in PlaybackMode] == ["Loop", "Once", "Sin", "Still"] and [int(m) for m in PlaybackMode] == [0, 1, 2, 3]
    s = CloudSettings()
    assert s.playback_mode == PlaybackMode.Still and s.time_scale == 1.0 and (s.time, s.time_start, s.time_stop) == (0.0, 0.0, 1.0)


# ---- cases worked by hand: every number below is a dyadic rational with few bits, so the f32 sums are exact ------------------
def test_still_and_a_zero_time_scale_change_nothing():
    for mode in PlaybackMode:
        assert run(mode, 0.375, scale=0.0, delta=0.25, elapsed=0.3) == 0.375            # time_scale == 0: every mode
        assert run(mode, 0.375, scale=-0.0, delta=0.25, elapsed=0.3) == 0.375           # -0.0 == 0.0
    assert run(PlaybackMode.Still, 0.375, delta=0.25, elapsed=0.3) == 0.375
    assert run(PlaybackMode.Still, 7.0, delta=0.25) == 7.0                              # not even when it is past time_stop


def test_once_stops_at_time_stop_and_does_not_reset():
    assert run(PlaybackMode.Once, 0.5, delta=0.25) == 0.75
    assert run(PlaybackMode.Once, 0.75, delta=0.25) == 1.0                              # arrives at time_stop exactly
    assert run(PlaybackMode.Once, 0.75, delta=0.25, steps=5) == 1.0                     # time >= time_stop: it stays
    assert run(PlaybackMode.Once, 0.875, delta=0.25) == 1.125                           # the last step is not clamped ...
    assert run(PlaybackMode.Once, 0.875, delta=0.25, steps=5) == 1.125                  # ... and nothing resets it
    assert run(PlaybackMode.Once, 0.5, scale=0.5, delta=0.5) == 0.75                    # delta_secs * time_scale
    assert run(PlaybackMode.Once, 0.5, scale=-1.0, delta=0.75, start=0.25) == -0.25     # backwards, below time_start: no rule stops it


def test_loop_wraps_only_when_strictly_past_time_stop():
    assert run(PlaybackMode.Loop, 0.5, delta=0.25, start=0.125) == 0.75
    assert run(PlaybackMode.Loop, 0.75, delta=0.25, start=0.125) == 1.0                 # == time_stop: not past it
    assert run(PlaybackMode.Loop, 0.75, delta=0.25, start=0.125, steps=2) == 0.125      # 1.25 > 1: back to time_start
    assert run(PlaybackMode.Loop, 0.75, delta=0.25, start=0.125, steps=3) == 0.375
    assert run(PlaybackMode.Loop, 1.0, delta=2.0 ** -23, start=0.125) == 0.125          # one ulp past time_stop is past it
    assert run(PlaybackMode.Loop, 0.25, scale=-1.0, delta=0.5) == -0.25                 # backwards: only `> time_stop` resets
    assert run(PlaybackMode.Loop, 3.0, delta=0.0) == 0.0                                # already past: reset even by a zero step


def test_the_linear_modes_are_f32():
    """1 + 2^-25 is a quarter of an ulp above 1 and rounds to 1 in f32: Loop with time_stop = 1 stays at 1. In float64
    the sum is past 1 and the cloud would jump back to time_start."""
    assert run(PlaybackMode.Loop, 1.0, delta=2.0 ** -25, start=0.5) == 1.0
    assert run(PlaybackMode.Once, 1.0, delta=2.0 ** -25, stop=2.0) == 1.0
    # 0.1f = 13421773 * 2^-27. Times 3 is 40265319 * 2^-27, which needs 26 bits: rounded to even 40265320 * 2^-27. The
    # sum 53687093 * 2^-27 needs 26 bits too: 53687092 * 2^-27 = 13421773 * 2^-25, which is 0.4f.
    assert np.float32(run(PlaybackMode.Once, float(np.float32(0.1)), scale=3.0, delta=float(np.float32(0.1)))) == np.float32(0.4)
    # (the significand 13421773 carries the implicit bit 2^23: biased exponents 123 and 125)
    assert int(np.float32(0.1).view(np.uint32)) == 13421773 + (122 << 23) and int(np.float32(0.4).view(np.uint32)) == 13421773 + (124 << 23)


# ---- Sin against float64 ----------------------------------------------------------------------------------------------------------
def sin_bound(scale, elapsed, start, stop, sine_ulps=2.0):
    """|f32 result - exact| for time_start + ((time_stop - time_start) * (sin(x) + 1)) / 2, x = 2 pi time_scale elapsed_secs,
    with the inputs exact f32 numbers. Every f32 operation is exact * (1 + d), |d| <= U:
      the argument  b = fl(fl(fl(scale * elapsed) * 2) * fl(pi)): three relative errors (the first product, the rounding of pi
                    to f32, which is below U, and the last product; the doubling is exact), so |b - x| <= |x| ((1 + U)^3 - 1).
                    With time_scale * elapsed_secs <= 20 that is at most 40 pi * 3.0000004 U = 2.25e-5.
      the sine      |sin b - sin x| <= |b - x| (the derivative is at most 1). The f32 sine itself is taken to be within
                    `sine_ulps` = 2 ulp of sin b (glibc documents 1 ulp for sinf, numpy's f32 loops stay below 2), and an
                    ulp of a value of magnitude at most 1 is at most 2^-23 = 2 U: e_sin = sine_ulps * 2 U.
      operation 1   s = fl(y + 1) lies in [0, 2]: its rounding adds at most 2 U. So |s - (sin x + 1)| <= e_s = e_arg + e_sin + 2 U.
      the span      d = fl(time_stop - time_start): one relative error.
      operation 2   p = fl(d * s): one more; the halving is exact. |p / 2 - D (sin x + 1) / 2| <= |D| / 2 * (e_s + (2 + e_s) ((1 + U)^2 - 1)) = e_h
      operation 3   t = fl(time_start + p / 2): a relative error U of a result whose magnitude is at most S + e_h, where
                    S = max(|time_start|, |time_stop|), because the exact value lies between the two.
    The float64 evaluation it is compared with has its own error, below 2^-50 (|x| + S + |D|), which is added."""
    x = abs(2.0 * math.pi * scale * elapsed)
    span, s_max = abs(stop - start), max(abs(start), abs(stop))
    e_arg = x * ((1.0 + U) ** 3 - 1.0)
    e_s = e_arg + sine_ulps * 2.0 * U + 2.0 * U
    e_h = span / 2.0 * (e_s + (2.0 + e_s) * ((1.0 + U) ** 2 - 1.0))
    return e_h * (1.0 + U) + U * (s_max + e_h) + 2.0 ** -50 * (x + s_max + span)


def sin_float64(scale, elapsed, start, stop):
    return start + (stop - start) * (math.sin(2.0 * math.pi * scale * elapsed) + 1.0) / 2.0


def sin_cases():
    rng = np.random.default_rng(20)
    cases = [(1.0, 0.0, 0.0, 1.0), (1.0, 0.25, 0.0, 1.0), (1.0, 0.75, 0.0, 1.0), (0.5, 40.0, 0.0, 1.0), (20.0, 1.0, -3.0, 5.0),
             (-1.0, 0.125, 0.25, 0.75), (2.0, 10.0, 1.0, 0.0), (1.0, 0.5, 2.0, 2.0)]
    for _ in range(400):
        scale = float(np.float32(rng.uniform(-4.0, 4.0)))
        elapsed = float(np.float32(rng.uniform(0.0, 20.0 / max(abs(scale), 1.0))))
        start, stop = (float(np.float32(v)) for v in rng.uniform(-2.0, 2.0, 2))
        cases.append((scale, elapsed, start, stop))
    assert all(abs(s * e) <= 20.0 for s, e, _, _ in cases)
    return cases


def test_sin_is_within_the_derived_bound_of_float64():
    worst = 0.0
    for scale, elapsed, start, stop in sin_cases():
        got = run(PlaybackMode.Sin, 123.0, scale=scale, start=start, stop=stop, delta=0.7, elapsed=elapsed)   # time and delta are not read
        bound = sin_bound(scale, elapsed, start, stop)
        err = abs(got - sin_float64(scale, elapsed, start, stop))
        worst = max(worst, err / bound)
        assert err <= bound, (scale, elapsed, start, stop, got, err, bound)
        assert got == float(np.float32(got))                                    # an f32 value
    print(f"Sin: worst error {worst:.3f} of the bound")
    assert sin_bound(1.0, 20.0, 0.0, 1.0) < 1.2e-5                              # the bound is small where it is largest
    # known answers: sin(0) = 0 gives the middle, a quarter period the stop's end, three quarters the start's
    assert run(PlaybackMode.Sin, 9.0, elapsed=0.0) == 0.5
    assert abs(run(PlaybackMode.Sin, 9.0, elapsed=0.25) - 1.0) <= sin_bound(1.0, 0.25, 0.0, 1.0)
    assert abs(run(PlaybackMode.Sin, 9.0, elapsed=0.75) - 0.0) <= sin_bound(1.0, 0.75, 0.0, 1.0)
    assert run(PlaybackMode.Sin, 9.0, scale=0.0, elapsed=0.25) == 9.0           # time_scale == 0 comes first


# ---- the C++ twin -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def playback_tool(tmp_path_factory):
    """include/bgs_host.hpp's playback_update in a small g++ program (tests/cpp/playback_tool.cpp). -ffp-contract=off: the
    comparison of the linear modes is bit for bit, and a fused multiply-add would round once where the reference rounds
    twice."""
    exe = tmp_path_factory.mktemp("playback") / "playback_tool"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "playback_tool.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def bits(value):
    return int(np.float32(value).view(np.uint32))


def cpp_times(tool, cases):
    """cases: (mode, time, scale, start, stop, delta, elapsed) -> the C++ twin's time after one update, as f32."""
    text = "".join("%d %08x %08x %08x %08x %08x %08x\n" % ((int(c[0]),) + tuple(bits(v) for v in c[1:])) for c in cases)
    out = subprocess.run([tool], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(cases)
    return np.array([int(w, 16) for w in out], np.uint32).view(np.float32)


def test_the_cpp_twin_agrees_on_the_linear_modes_bit_for_bit(playback_tool):
    rng = np.random.default_rng(21)
    hand = [(PlaybackMode.Loop, 0.75, 1.0, 0.125, 1.0, 0.25, 0.0), (PlaybackMode.Loop, 1.0, 1.0, 0.125, 1.0, 0.25, 0.0),
            (PlaybackMode.Loop, 1.0, 1.0, 0.5, 1.0, 2.0 ** -25, 0.0), (PlaybackMode.Loop, 1.0, 1.0, 0.125, 1.0, 2.0 ** -23, 0.0),
            (PlaybackMode.Once, 0.75, 1.0, 0.0, 1.0, 0.25, 0.0), (PlaybackMode.Once, 1.0, 1.0, 0.0, 1.0, 0.25, 0.0),
            (PlaybackMode.Once, 0.875, 1.0, 0.0, 1.0, 0.25, 0.0), (PlaybackMode.Once, 0.1, 3.0, 0.0, 1.0, 0.1, 0.0),
            (PlaybackMode.Still, 0.375, 1.0, 0.0, 1.0, 0.25, 0.3), (PlaybackMode.Loop, 0.375, 0.0, 0.0, 1.0, 0.25, 0.3),
            (PlaybackMode.Once, 0.375, -0.0, 0.0, 1.0, 0.25, 0.3), (PlaybackMode.Sin, 0.375, 0.0, 0.0, 1.0, 0.25, 0.3)]
    cases = [tuple(float(np.float32(v)) if k else v for k, v in enumerate(c)) for c in hand]
    for _ in range(2000):
        mode = (PlaybackMode.Loop, PlaybackMode.Once, PlaybackMode.Still)[int(rng.integers(3))]
        start, stop = sorted(float(np.float32(v)) for v in rng.uniform(-2.0, 2.0, 2))
        time = float(np.float32(rng.uniform(start - 0.1, stop + 0.1)))
        scale = float(np.float32(rng.choice([0.0, 1.0, rng.uniform(-3.0, 3.0)])))
        delta = float(np.float32(rng.uniform(0.0, 0.3)))
        cases.append((mode, time, scale, start, stop, delta, float(np.float32(rng.uniform(0.0, 5.0)))))
    got = cpp_times(playback_tool, cases)
    want = np.array([run(c[0], c[1], scale=c[2], start=c[3], stop=c[4], delta=c[5], elapsed=c[6]) for c in cases], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    moved = sum(1 for c, w in zip(cases, want) if np.float32(c[1]) != w)
    wrapped = sum(1 for c, w in zip(cases, want) if c[0] == PlaybackMode.Loop and np.float32(c[1]) != w and w == np.float32(c[3]))
    assert moved > 500 and wrapped > 20                                          # the cases exercise the steps and the wrap


def test_the_cpp_twin_agrees_on_sin_within_the_bound(playback_tool):
    """Both twins against the float64 evaluation within the bound of `sin_bound` (the two sine functions may differ)."""
    cases = [(PlaybackMode.Sin, 123.0, scale, start, stop, 0.7, elapsed) for scale, elapsed, start, stop in sin_cases()]
    got = cpp_times(playback_tool, cases)
    for c, g in zip(cases, got):
        truth, bound = sin_float64(c[2], c[6], c[3], c[4]), sin_bound(c[2], c[6], c[3], c[4])
        python = run(c[0], c[1], scale=c[2], start=c[3], stop=c[4], delta=c[5], elapsed=c[6])
        assert abs(float(g) - truth) <= bound and abs(python - truth) <= bound, (c, float(g), python, truth, bound)


def test_the_package_exports_the_playback_surface():
    import bevy_gaussian_splatting_amd as pkg
    for name in ("PlaybackMode", "playback_update", "MorphPair", "ResidentCloud4d"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert all(hasattr(pkg.GaussianSplattingPlugin, m) for m in ("resident_4d", "upload_device_planes", "slice_4d", "morph_pair"))
