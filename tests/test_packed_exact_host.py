"""The exact references of the packed outputs (tests/packed_exact.py) checked on the host: the sRGB8 thresholds against
the oracle at every code boundary, the binary16 reference against numpy, and the committed pack_tables.h against the
thresholds (scripts/gen_pack_tables.py)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import packed_exact as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def thresholds():
    return P.colour_thresholds(), P.alpha_thresholds()


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_thresholds_are_the_least_f32_at_or_above_each_midpoint(thresholds):
    from fractions import Fraction
    colour, alpha = thresholds
    assert (np.diff(colour.astype(np.int64)) > 0).all() and (np.diff(alpha.astype(np.int64)) > 0).all()
    assert colour[-1] < 0x3F800000 and alpha[-1] < 0x3F800000 and colour[0] > 0 and alpha[0] > 0
    for k in range(1, 256):   # alpha: straight from the definition, t >= (2k - 1) / 510 > t - 1 ulp
        y = Fraction(2 * k - 1, 510)
        assert P.f32_value(int(alpha[k - 1])) >= y > P.f32_value(int(alpha[k - 1]) - 1)
    assert alpha[127] == 0x3F000000   # 0.5 = 127.5 / 255 exactly: the one tie, rounded up like the oracle


def test_srgb8_code_boundaries_through_the_oracle(oracle, thresholds):
    """At every one of the 255 boundaries of every channel, the f32 just below the threshold gives code k - 1 and the
    threshold itself code k, in the oracle and in the torch reference the device tests use."""
    colour, alpha = thresholds
    k = np.arange(1, 256)
    below = np.stack([colour - 1] * 3 + [alpha - 1], axis=1)
    at = np.stack([colour] * 3 + [alpha], axis=1)
    px = _f32(np.concatenate([below, at]))
    want = np.concatenate([np.repeat(k - 1, 4).reshape(-1, 4), np.repeat(k, 4).reshape(-1, 4)]).astype(np.uint8)
    assert np.array_equal(oracle.srgb8_codes(px), want)
    bits = torch.from_numpy(px.view(np.int32))
    ref = torch.cat([P.srgb8_codes_from_bits(bits[:, :3].contiguous(), torch.from_numpy(colour.view(np.int32))),
                     P.srgb8_codes_from_bits(bits[:, 3:].contiguous(), torch.from_numpy(alpha.view(np.int32)))], dim=1)
    assert np.array_equal(ref.numpy(), want)


def test_srgb8_special_values(oracle, thresholds):
    colour, alpha = thresholds
    cases = {0x00000000: 0, 0x80000000: 0, 0x00000001: 0, 0x80000001: 0, 0xBF800000: 0, 0xFF800000: 0,
             0x7FC00000: 0, 0xFFC00000: 0, 0x7F800001: 0, 0x7FFFFFFF: 0, 0xFFFFFFFF: 0,
             0x3F800000: 255, 0x3F800001: 255, 0x40000000: 255, 0x7F7FFFFF: 255, 0x7F800000: 255}
    bits = np.array(list(cases), np.uint32)
    want = np.repeat(np.array(list(cases.values()), np.uint8), 4).reshape(-1, 4)
    px = np.repeat(bits, 4).reshape(-1, 4).view(np.float32)
    assert np.array_equal(oracle.srgb8_codes(px), want)
    t = torch.from_numpy(px.view(np.int32))
    ref = torch.cat([P.srgb8_codes_from_bits(t[:, :3].contiguous(), torch.from_numpy(colour.view(np.int32))),
                     P.srgb8_codes_from_bits(t[:, 3:].contiguous(), torch.from_numpy(alpha.view(np.int32)))], dim=1)
    assert np.array_equal(ref.numpy(), want)


def test_srgb8_torch_reference_matches_the_oracle_on_random_patterns(oracle, thresholds):
    colour, alpha = thresholds
    rng = np.random.default_rng(11)
    b = np.concatenate([rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32),
                        rng.integers(0, 0x3F800001, 3 << 20, dtype=np.uint64).astype(np.uint32)])   # mostly [0, 1]
    px = b.view(np.float32).reshape(-1, 4)
    t = torch.from_numpy(px.view(np.int32))
    ref = torch.cat([P.srgb8_codes_from_bits(t[:, :3].contiguous(), torch.from_numpy(colour.view(np.int32))),
                     P.srgb8_codes_from_bits(t[:, 3:].contiguous(), torch.from_numpy(alpha.view(np.int32)))], dim=1)
    assert np.array_equal(ref.numpy(), oracle.srgb8_codes(px))


def _f16_check(bits: np.ndarray):
    with np.errstate(over="ignore"):
        want = bits.view(np.float32).astype(np.float16).view(np.uint16).astype(np.int32)
    got = P.f16_bits(torch.from_numpy(bits.view(np.int32))).numpy()
    assert ((got >= 0) & (got <= 0xFFFF)).all()
    miss = P.f16_mismatch(torch.from_numpy(got), torch.from_numpy(want)).numpy()
    assert not miss.any(), [(hex(int(b)), hex(int(g)), hex(int(w))) for b, g, w in
                            zip(bits[miss][:20], got[miss][:20], want[miss][:20])]
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    assert ((got[nan] & 0x7FFF) > 0x7C00).all() and (got[~nan] == want[~nan]).all()


def test_f16_reference_every_exponent_and_the_mantissas_that_matter():
    """Every binary32 exponent (both signs) crossed with the mantissa patterns where rounding decides: every single bit,
    a bit +-1 and a bit - 1 (the tie, next to it and just under an ulp at every shift a subnormal result takes), the
    binary16 tie 0x1000 and its neighbours, all ones, and the named edges 65504, 65519, 65520, inf, NaN payloads, -0."""
    mant = {0, 0x7FFFFF, 0x1000, 0x0FFF, 0x1001, 0x1FFF, 0x2000, 0x3000, 0x2FFF, 0x3001, 0x7FF000, 0x7FEFFF, 0x7FF001}
    for j in range(23):
        for d in (-1, 0, 1):
            mant.add(((1 << j) + d) & 0x7FFFFF)
            mant.add(((3 << j) + d) & 0x7FFFFF)
            mant.add((0x7FFFFF - (1 << j) + d) & 0x7FFFFF)
    mant = np.array(sorted(mant), np.uint32)
    exps = np.arange(256, dtype=np.uint32)
    bits = ((exps[:, None] << 23) | mant[None, :]).ravel()
    named = np.array([65504.0, 65519.0, 65520.0, 65536.0, 6.1035156e-05, 5.9604645e-08, 2.9802322e-08],
                     np.float32).view(np.uint32)
    extra = np.array([0x477FEFFF, 0x477FF000, 0x477FF001, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF,
                      0x7F801000, 0x7FA00000, 0x33000000, 0x33000001, 0x32FFFFFF, 0x38800000, 0x387FFFFF, 0x387FF000], np.uint32)
    bits = np.concatenate([bits, named, extra])
    bits = np.concatenate([bits, bits | 0x80000000])
    _f16_check(bits)
    assert P.f16_bits(torch.tensor([struct.unpack("<i", struct.pack("<f", 65520.0))[0]], dtype=torch.int32)).item() == 0x7C00
    assert P.f16_bits(torch.tensor([struct.unpack("<i", struct.pack("<f", 65519.0))[0]], dtype=torch.int32)).item() == 0x7BFF


def test_f16_reference_random_patterns():
    rng = np.random.default_rng(7)
    for _ in range(4):
        _f16_check(rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32))


def test_pack_tables_header_is_what_the_script_writes(thresholds):
    """csrc/pack_tables.h (the device's colour thresholds) == the exact thresholds above, via the committed script."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_pack_tables.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    import re
    with open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "pack_tables.h")) as f:
        pairs = re.findall(r"\{0x([0-9a-f]{8}), 0x([0-9a-f]{8})\}", f.read())
    table = np.array([[int(a, 16), int(b, 16)] for a, b in pairs], np.uint32)
    colour, _ = thresholds
    assert table.shape == (256, 2)
    assert table[0, 0] == 0 and table[255, 1] == 0x7FFFFFFF
    assert np.array_equal(table[1:, 0], colour) and np.array_equal(table[:-1, 1], colour)
