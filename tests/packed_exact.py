"""Exact references of the packed outputs' conversion (include/bgs.h "packed outputs"), shared by the CPU tests, the
device tests and scripts/gen_pack_tables.py:

- Rgba8UnormSrgb colour: the code of x is the number of thresholds eotf((2k - 1) / 510), k = 1..255, that x reaches
  (round to nearest of the exact sRGB OETF); alpha: the same with the thresholds (2k - 1) / 510. As binary32 inputs, a
  threshold is the least f32 at or above it, found with exact rational arithmetic (no float rounding anywhere).
- Rgba16Float: binary32 -> binary16 round to nearest even, overflow to inf, NaN to NaN, in integer operations only
  (torch, so that the same function runs on the host and on the device)."""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

# sRGB EOTF (IEC 61966-2-1, the reference's Rgba8UnormSrgb attachment): v <= 0.04045 -> v / 12.92,
# else ((v + 0.055) / 1.055) ** 2.4
_LIN_CUT = Fraction(4045, 100000)
_LIN_DIV = Fraction(1292, 100)
_A = Fraction(55, 1000)
_A1 = Fraction(1055, 1000)


def f32_value(bits: int) -> Fraction:
    return Fraction(struct.unpack("<f", struct.pack("<I", bits))[0])


def _f32_bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _least_f32_at_or_above(reaches, estimate: float) -> int:
    """Bit pattern of the least positive finite f32 t with reaches(t) (a monotone predicate on exact values)."""
    b = _f32_bits(estimate)
    while not reaches(f32_value(b)):
        b += 1
    while b > 0 and reaches(f32_value(b - 1)):
        b -= 1
    return b


def colour_thresholds() -> np.ndarray:
    """uint32[255]: entry k - 1 = the least f32 (bits) at or above eotf((2k - 1) / 510), the least input of code k."""
    out = []
    for k in range(1, 256):
        v = Fraction(2 * k - 1, 510)
        if v <= _LIN_CUT:
            y = v / _LIN_DIV
            reaches = lambda t, y=y: t >= y   # noqa: E731
            est = float(y)
        else:
            r = (v + _A) / _A1   # eotf = r ** (12 / 5): t >= eotf <=> t ** 5 >= r ** 12 (both sides positive)
            r12 = r ** 12
            reaches = lambda t, r12=r12: t ** 5 >= r12   # noqa: E731
            est = float(r) ** 2.4
        out.append(_least_f32_at_or_above(reaches, est))
    return np.array(out, np.uint32)


def alpha_thresholds() -> np.ndarray:
    """uint32[255]: entry k - 1 = the least f32 (bits) at or above (2k - 1) / 510, the least alpha of code k."""
    out = []
    for k in range(1, 256):
        y = Fraction(2 * k - 1, 510)
        out.append(_least_f32_at_or_above(lambda t, y=y: t >= y, float(y)))
    return np.array(out, np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# torch references (int32 bit patterns in, codes out; run wherever the tensors live)
# ---------------------------------------------------------------------------------------------------------------------
def srgb8_codes_from_bits(bits, thresholds):
    """Codes of f32 bit patterns (int32 tensor) against a threshold table (int32 tensor [255], ascending): the number
    of thresholds the value reaches. Negative patterns (sign bit set: -0, negatives, -inf, negative NaNs) come first as
    int32 and reach none; +inf and everything above 1 reach all 255; positive NaNs are set to 0."""
    import torch
    code = torch.searchsorted(thresholds, bits, right=True)
    return torch.where(bits > 0x7F800000, 0, code).to(torch.uint8)


def f16_bits(bits):
    """binary32 bit patterns (int32 tensor) -> binary16 bit patterns (int32 tensor, 0..0xFFFF): round to nearest even,
    overflow to inf, NaN to the quiet NaN 0x7E00 (with the input's sign). Integer operations only."""
    import torch
    i32 = torch.int32
    sign = (bits >> 16) & 0x8000
    a = bits & 0x7FFFFFFF
    # normal binary16 range, a >= 2^-14: re-bias the exponent, round the 13 dropped bits (a carry into the exponent is
    # the right result, up to and including inf from 65520 on)
    rem = a & 0x1FFF
    h = (a >> 13) - ((127 - 15) << 10)
    h = h + ((rem > 0x1000) | ((rem == 0x1000) & ((h & 1) == 1))).to(i32)
    # subnormal range: the significand with its implicit bit, shifted to units of 2^-24 (shift 25 leaves 0 for every
    # value below 2^-25, binary32 subnormals included)
    e = a >> 23
    m = (a & 0x7FFFFF) | 0x800000
    s = (126 - e).clamp(1, 25)
    q = m >> s
    r = m & (torch.bitwise_left_shift(torch.ones_like(s), s) - 1)
    half = torch.bitwise_left_shift(torch.ones_like(s), s - 1)
    q = q + ((r > half) | ((r == half) & ((q & 1) == 1))).to(i32)
    out = torch.where(a < 0x38800000, q, h)
    out = torch.where(a >= 0x47800000, 0x7C00, out)
    out = torch.where(a > 0x7F800000, 0x7E00, out)
    return out | sign


def f16_mismatch(got, want):
    """Element-wise: device binary16 bits `got` differ from the reference `want` (int32 tensors). A NaN must map to
    some NaN; everything else must match bit for bit."""
    want_nan = (want & 0x7FFF) > 0x7C00
    got_nan = (got & 0x7FFF) > 0x7C00
    return (want_nan & ~got_nan) | (~want_nan & (got != want))


# ---------------------------------------------------------------------------------------------------------------------
# exhaustive device run
# ---------------------------------------------------------------------------------------------------------------------
def exhaustive_pack(plugin, fmt: str, chunk_floats: int = 1 << 24, max_report: int = 20):
    """Every one of the 2^32 binary32 bit patterns through bgs_selftest_pack in every channel: four passes, pass r
    feeding pattern 4 i + (c + r) % 4 to channel c of pixel i, in chunks of `chunk_floats` patterns. Expected values
    are computed on the device with the functions above. Returns (mismatches per output channel [4], first `max_report`
    as (bits, channel, device code, expected code), patterns checked); channel 3 is alpha."""
    import torch
    dev = "cuda:0"
    assert (1 << 32) % chunk_floats == 0 and chunk_floats % 4 == 0
    pixels = chunk_floats // 4
    colour = torch.from_numpy(colour_thresholds().astype(np.int32)).to(dev)
    alpha = torch.from_numpy(alpha_thresholds().astype(np.int32)).to(dev)
    idx = torch.arange(chunk_floats, dtype=torch.int32, device=dev)
    out = torch.empty(pixels * (4 if fmt == "srgb8" else 8), dtype=torch.uint8, device=dev)
    bad, report, checked = [0, 0, 0, 0], [], 0
    for r in range(4):
        for base in range(0, 1 << 32, chunk_floats):
            b32 = base - (1 << 32) if base >= (1 << 31) else base    # chunks never straddle 2^31: int32 arithmetic
            x = (idx + b32).view(pixels, 4).roll(-r, dims=1).contiguous()
            torch.cuda.synchronize()
            plugin.selftest_pack(fmt, x.data_ptr(), pixels, out.data_ptr())
            if fmt == "srgb8":
                got = out.view(pixels, 4)
                want = torch.cat([srgb8_codes_from_bits(x[:, :3].contiguous(), colour),
                                  srgb8_codes_from_bits(x[:, 3:].contiguous(), alpha)], dim=1)
                miss = got != want
            else:
                got = out.view(torch.int16).view(pixels, 4).to(torch.int32) & 0xFFFF
                want = f16_bits(x)
                miss = f16_mismatch(got, want)
            per_channel = miss.sum(dim=0).tolist()
            checked += chunk_floats
            if sum(per_channel):
                bad = [a + b for a, b in zip(bad, per_channel)]
                if len(report) < max_report:
                    where = miss.nonzero()[: max_report - len(report)].cpu().numpy()
                    xs, gs, ws = x.cpu().numpy(), got.cpu().numpy(), want.cpu().numpy()
                    for i, c in where:
                        report.append((int(xs[i, c]) & 0xFFFFFFFF, int(c), int(gs[i, c]), int(ws[i, c])))
    return bad, report, checked


def format_report(fmt: str, bad, report) -> str:
    lines = [f"{fmt}: {sum(bad)} of 2^34 (pattern, channel) pairs differ from the exact conversion (per channel R, G, B, "
             f"A: {bad}); first {len(report)}:"]
    for bits, c, g, w in report:
        lines.append(f"  0x{bits:08x} ({struct.unpack('<f', struct.pack('<I', bits))[0]!r}) channel {c}: "
                     f"device {g:#x}, expected {w:#x}")
    return "\n".join(lines)
