"""References and cases for the bucket sort path (tests/test_bucket_stage_host.py, tests/test_bucket_stage_gpu.py).

Two kernels are pinned, each run alone through a diagnostic of include/bgs_diag.h:

  bucket_sort_kernel (bgs_selftest_bucket_sort) on caller-supplied bucket contents. The reference is `expected_sort`: the
  verdict (a count over the capacity; else a fine range of more than BUCKET_FINE_MAX pairs; else sorted) and, bucket by
  bucket, the pairs ordered by (key, index) with key ^ key_xor written.
  keygen's bucket placement (bgs_selftest_keygen_buckets) on a resident cloud with a caller-supplied splitter table. The
  reference is `bucket_of` = min(searchsorted(table, key, side="right"), nb - 1) over the drawable keys of oracle.sort.

Integer work: every comparison is equality. The constants are the values of csrc/bgs_device.h, read from the header."""
import dataclasses
import functools
import os
import re

import numpy as np

from bevy_gaussian_splatting_amd import CloudSettings, View, random_gaussians_3d_seeded
from bevy_gaussian_splatting_amd.settings import SortMode

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_HEADER = open(os.path.join(ROOT, "bevy_gaussian_splatting_amd", "csrc", "bgs_device.h")).read()


def _const(name):
    m = re.search(rf"(?:constexpr uint32_t|#define) {name}(?: =)? (\d+)", _HEADER)
    assert m, f"csrc/bgs_device.h does not define {name}"
    return int(m.group(1))


BUCKET_COUNT = _const("BUCKET_COUNT")
BUCKET_CAP = _const("BUCKET_CAP")
BUCKET_FINE = _const("BUCKET_FINE")
BUCKET_FINE_MAX = _const("BUCKET_FINE_MAX")
BUCKET_SUB_MAX = _const("BUCKET_SUB_MAX")
BUCKET_SUB_KERNARG = _const("BUCKET_SUB_KERNARG")
BUCKET_CAP_WIDE = _const("BUCKET_CAP_WIDE")
BUCKET_FINE_WIDE = _const("BGS_BUCKET_FINE_WIDE")
FILL = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def cap_of(wide):
    return BUCKET_CAP_WIDE if wide else BUCKET_CAP


def nf_of(wide):
    return BUCKET_FINE_WIDE if wide else BUCKET_FINE


# ---- the references --------------------------------------------------------------------------------------------------
def bucket_of(keys, table):
    """Bucket of every key for the ascending table of nb - 1 splitters: the number of splitters <= key."""
    table = np.asarray(table, np.uint32)
    return np.minimum(np.searchsorted(table, np.asarray(keys, np.uint32), side="right"), len(table)).astype(np.int64)


def fine_of(key, kmn, kmx, nf):
    """bucket_sort_kernel's fine range of a key in a bucket whose keys span [kmn, kmx], in Python integers:
    __umulhi(key - kmn, floor(2^32 nf / (span + 1))), or the difference itself when span < nf."""
    span = int(kmx) - int(kmn)
    d = int(key) - int(kmn)
    if span < nf:
        return d
    scale = (nf << 32) // (span + 1)
    assert scale < (1 << 32)
    return (d * scale) >> 32


def fine_histogram(keys, nf):
    """Pairs per fine range of one bucket's keys (a dict range -> pairs)."""
    keys = np.asarray(keys, np.uint32)
    if not len(keys):
        return {}
    kmn, kmx = int(keys.min()), int(keys.max())
    vals, cnt = np.unique(keys, return_counts=True)
    hist = {}
    for v, c in zip(vals.tolist(), cnt.tolist()):
        f = fine_of(v, kmn, kmx, nf)
        hist[f] = hist.get(f, 0) + c
    return hist


def split_buckets(counts, pairs, cap):
    """The pairs of every bucket: min(count, cap) of each, in the caller's order."""
    kept = np.minimum(np.asarray(counts, np.int64), cap)
    ends = np.cumsum(kept)
    return [pairs[int(e - k):int(e)] for e, k in zip(ends, kept)]


def sort_bucket(pairs):
    """One bucket ordered by (key, index)."""
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def expected_sort(wide, key_xor, counts, pairs):
    """What bgs_selftest_bucket_sort returns: `sort_overflow`, `draw_count`, `bucket_max` (None: not stated) and `out`, the
    list of n entries — a bucket that gives up, and every bucket of a launch with a count over the capacity, leaves its
    stretch of the list as it was (the fill)."""
    cap, nf = cap_of(wide), nf_of(wide)
    counts = np.asarray(counts, np.int64)
    n = int(np.minimum(counts, cap).sum())
    out = np.full((n, 2), FILL, np.uint32)
    if (counts > cap).any():
        return {"sort_overflow": 1, "draw_count": 0, "bucket_max": int(counts.max()), "out": out}
    flag, at = 0, 0
    for b in split_buckets(counts, pairs, cap):
        if len(b):
            if max(fine_histogram(b[:, 0], nf).values()) > BUCKET_FINE_MAX:
                flag = 2
            else:
                s = sort_bucket(b)
                out[at:at + len(b), 0] = s[:, 0] ^ np.uint32(key_xor)
                out[at:at + len(b), 1] = s[:, 1]
        at += len(b)
    return {"sort_overflow": flag, "draw_count": 0 if flag else n, "bucket_max": int(counts.max()), "out": out}


# ---- cases for the kernel alone ---------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class SortCase:
    name: str
    sub: int
    wide: int
    counts: np.ndarray          # uint32[256 * sub]
    pairs: np.ndarray           # uint32[n, 2], bucket after bucket, arrival order shuffled
    verdict: int                # the sort_overflow the case is built for


def _indices(rng, m):
    """m distinct indices over the whole 32-bit range, half of them >= 2^31 (m >= 2), in random order."""
    lo = rng.choice(1 << 31, size=(m + 1) // 2, replace=False).astype(np.uint64)
    hi = rng.choice(1 << 31, size=m // 2, replace=False).astype(np.uint64) + (1 << 31)
    idx = np.concatenate([lo, hi]).astype(np.uint32)
    rng.shuffle(idx)
    return idx


def _bucket(rng, keys):
    """(key, index) pairs of one bucket in a shuffled arrival order."""
    keys = np.asarray(keys, np.uint64).astype(np.uint32)
    p = np.stack([keys, _indices(rng, len(keys))], axis=1)
    rng.shuffle(p, axis=0)
    return p


def _one_bucket(name, wide, bucket, count=None, at=None, sub=1, verdict=0):
    """A launch whose only non-empty bucket is `at` (default: a middle one; the last one for a bucket that gives up: the
    same thread then publishes draw_count and voids it, in program order — with two workgroups the order of the two stores
    is open, and what the kernels behind it read is the flag)."""
    nb = BUCKET_COUNT * sub
    if at is None:
        at = nb - 1 if verdict == 2 else nb // 3
    counts = np.zeros(nb, np.uint32)
    counts[at] = len(bucket) if count is None else count
    return SortCase(name, sub, wide, counts, bucket, verdict)


def _random_keys(rng, m):
    """m keys over the whole 32-bit range (both halves), a few of them repeated."""
    keys = rng.integers(0, 1 << 32, size=m, dtype=np.uint64)
    if m >= 8:
        keys[rng.choice(m, size=min(m // 8, 300), replace=False)] = keys[0]
    return keys


def _span_keys(rng, kmn, span, m=200):
    """Three pairs at kmn, three at kmx = kmn + span, the rest in between."""
    if span == 0:
        return np.full(m, kmn, np.uint64)
    mid = kmn + rng.integers(0, span + 1, size=m - 6, dtype=np.uint64)
    return np.concatenate([np.full(3, kmn, np.uint64), np.full(3, kmn + span, np.uint64), mid])


def two_keys_one_range(nf, span=1 << 20):
    """Two distinct keys with the same fine range, neither kmn nor kmx of a bucket spanning [kmn, kmn + span]."""
    kmn = 0x7FF00000
    a = kmn + 5 * ((span + 1) // nf) + 3
    assert fine_of(a, kmn, kmn + span, nf) == fine_of(a + 1, kmn, kmn + span, nf)
    return kmn, a, a + 1


SPANS = ("0", "NF-1", "NF", "NF+1", "2^31", "0xFFFFFFFF")


def span_value(name, nf):
    return {"0": 0, "NF-1": nf - 1, "NF": nf, "NF+1": nf + 1, "2^31": 1 << 31, "0xFFFFFFFF": M32}[name]


def span_kmn(name, nf):
    """The smallest key of a span case: spans below 2^31 straddle 2^31, the two long ones start at 2^31 - 7 and at 0."""
    span = span_value(name, nf)
    return 0 if span == M32 else ((1 << 31) - 7 if span == 1 << 31 else (1 << 31) - span // 2)


@functools.lru_cache(maxsize=None)
def sort_cases(wide):
    rng = np.random.Generator(np.random.PCG64(20 + wide))
    cap, nf = cap_of(wide), nf_of(wide)
    tag = "wide" if wide else "narrow"
    cases = []
    for m in (1, 2, 63, 64, 65, 255, 256, 257, cap - 1, cap):
        cases.append(_one_bucket(f"{tag} m={m}", wide, _bucket(rng, _random_keys(rng, m))))
    cases.append(_one_bucket(f"{tag} m=cap+1", wide, _bucket(rng, _random_keys(rng, cap)), count=cap + 1, verdict=1))
    for s in SPANS:
        cases.append(_one_bucket(f"{tag} span={s}", wide, _bucket(rng, _span_keys(rng, span_kmn(s, nf), span_value(s, nf)))))
    for m in (BUCKET_FINE_MAX, BUCKET_FINE_MAX + 1):
        cases.append(_one_bucket(f"{tag} {m} equal", wide, _bucket(rng, np.full(m, 0x80000123, np.uint64)),
                                 verdict=2 if m > BUCKET_FINE_MAX else 0))
    others = 0x9000_0000 + 977 * np.arange(1, 301, dtype=np.uint64)
    cases.append(_one_bucket(f"{tag} {BUCKET_FINE_MAX} equal + other ranges", wide,
                             _bucket(rng, np.concatenate([np.full(BUCKET_FINE_MAX, 0x9000_0000, np.uint64), others]))))
    kmn, a, b = two_keys_one_range(nf)
    for total in (BUCKET_FINE_MAX, BUCKET_FINE_MAX + 1):
        keys = np.concatenate([[kmn, kmn + (1 << 20)], np.full(600, a, np.uint64), np.full(total - 600, b, np.uint64)])
        cases.append(_one_bucket(f"{tag} two keys in one fine range, {total}", wide, _bucket(rng, keys), verdict=2 if total > BUCKET_FINE_MAX else 0))
    groups = (2, 3, 64, 65, 500, BUCKET_FINE_MAX)        # tie groups, one fine range each (span < NF: every key its own range)
    keys = np.concatenate([np.full(g, 0xFFFF_F000 + 11 * i, np.uint64) for i, g in enumerate(groups)])
    cases.append(_one_bucket(f"{tag} tie groups", wide, _bucket(rng, keys)))
    if wide:
        k0, j = 0x7FFF_F000, 1500                        # (span = NF - 1: the fine range of a key is key - k0)
        keys = np.concatenate([[k0, k0 + nf - 1], np.full(1000, k0 + 2 * j, np.uint64), np.full(1024, k0 + 2 * j + 1, np.uint64),
                               np.full(900, k0 + nf - 2, np.uint64), np.full(800, k0 + 1, np.uint64)])
        cases.append(_one_bucket("wide heavy neighbour ranges, first and last range", wide, _bucket(rng, keys)))
    # several buckets: every bucket draws its keys by itself (the kernel never compares two buckets), counts 0 .. 40
    for sub in (1, 2, 3, 4, 16):
        nb = BUCKET_COUNT * sub
        for form in ("first empty", "last empty", "only the last", "one pair each", "a full bucket and its neighbours"):
            counts = rng.integers(0, 41, size=nb).astype(np.uint32)
            if form == "first empty":
                counts[0] = 0
            elif form == "last empty":
                counts[-1] = 0
            elif form == "only the last":
                counts[:-1] = 0
                counts[-1] = 37
            elif form == "one pair each":
                counts[:] = 1
            else:
                if sub not in (1, 16):
                    continue
                counts[nb // 2 - 1:nb // 2 + 2] = (cap - 1, cap, 1)
            n = int(counts.sum())
            idx = _indices(rng, n)
            keys = np.concatenate([_random_keys(rng, int(c)) for c in counts if c]).astype(np.uint32)
            cases.append(SortCase(f"{tag} sub={sub} {form}", sub, wide, counts, np.stack([keys, idx], axis=1), 0))
    return tuple(cases)


# ---- cases for the placement -----------------------------------------------------------------------------------------
SIZES = (1, 2047, 2048, 2049, 6000)
BIG = (1 << 19) + 1
MODES = ("radix", "rayon")
TABLES = ("quantiles", "zeros", "ones", "one occurring key", "runs", "below occurring keys", "another camera")
SUBS = (1, 2, 3, 4, 5, 16)


def lookup_form(sub):
    """(the unrolled form of keygen's bucket_of, where the table travels) for a table of 256 * sub buckets."""
    p2 = 256
    while p2 < BUCKET_COUNT * sub:
        p2 <<= 1
    form = "256" if sub == 1 else ("512" if p2 == 512 else ("1024" if p2 == 1024 else "general"))
    return form, ("kernel arguments" if sub <= BUCKET_SUB_KERNARG else "device table")


def tile_shape(n, alone):
    """(threads, splats per thread) of keygen's tile for a bucket frame of n splats."""
    if n >= 1 << 19:
        return (1024, 4) if alone else (256, 16)
    return (256, 8)


def placement_view(other=False):
    return View.headless(320, 180, yaw=0.6 if other else 0.0)


@functools.lru_cache(maxsize=None)
def placement_scene(n, mode):
    """The cloud, view and settings of a placement case. `radix`: the camera culls most of the cloud; `rayon`: every splat
    is drawable and splat n // 2 lies exactly at the camera position (its key is ~0 in keygen's key space)."""
    cloud = random_gaussians_3d_seeded(n, 40 + (n % 97))
    view = placement_view()
    settings = CloudSettings()
    if mode == "rayon":
        settings.sort_mode = SortMode.Rayon
        cloud.position_visibility[n // 2, :3] = view.world_position.astype(np.float32)
    else:
        settings.sort_mode = SortMode.Radix
        if n == 1:
            cloud.position_visibility[0, :3] = (0.25, 1.5, -3.0)   # (in front of the camera: one drawable splat)
    return cloud, view, settings


def key_xor_of(settings):
    return M32 if settings.sort_mode in (SortMode.Rayon, SortMode.Std) else 0


def keygen_space(oracle, cloud, view, settings):
    """From oracle.sort: the sorted entries, and in keygen's key space (key ^ key_xor) the key of every splat, the drawable
    mask and the number of drawable splats."""
    entries = oracle.sort(cloud, view, settings)
    n = len(entries)
    kk = np.empty(n, np.uint32)
    kk[entries["index"]] = entries["key"] ^ np.uint32(key_xor_of(settings))
    if settings.sort_mode == SortMode.Radix:
        drawable = kk != np.uint32(M32 >> (32 - settings.radix_sort_depth_bits))
    else:
        drawable = np.ones(n, bool)
    return entries, kk, drawable, int(drawable.sum())


def quantile_table(sorted_keys, sub):
    """splitter_kernel's table: the keys at the 1 / (256 sub)-quantiles of the ascending drawable keys (~0 for an empty list)."""
    nb, d = BUCKET_COUNT * sub, len(sorted_keys)
    if d == 0:
        return np.full(nb - 1, FILL, np.uint32)
    return np.asarray(sorted_keys, np.uint32)[(np.arange(1, nb, dtype=np.int64) * d) // nb]


def table(kind, sub, kd, kd_other):
    """A splitter table of 256 * sub - 1 keys; kd: this camera's drawable keys, ascending; kd_other: another camera's."""
    nb = BUCKET_COUNT * sub
    q = quantile_table(kd, sub)
    if kind == "quantiles":
        return q
    if kind == "zeros":
        return np.zeros(nb - 1, np.uint32)
    if kind == "ones":
        return np.full(nb - 1, FILL, np.uint32)
    if kind == "one occurring key":
        return np.full(nb - 1, kd[len(kd) // 2] if len(kd) else 7, np.uint32)
    if kind == "runs":
        return q[(np.arange(nb - 1) // 64) * 64]
    if kind == "below occurring keys":
        return np.where(q > 0, q - np.uint32(1), q).astype(np.uint32)
    if kind == "another camera":
        return quantile_table(kd_other, sub)
    raise KeyError(kind)


def expected_counts(kk, drawable, tab):
    nb = len(tab) + 1
    return np.bincount(bucket_of(kk[drawable], tab), minlength=nb).astype(np.int64)


def check_placement(what, out, kk, drawable, tab, cap):
    """Holds a placement run to the reference: every count; per bucket the written slots as a multiset (a sub-multiset of
    `cap` pairs where the bucket overflows); every slot past min(count, cap) untouched. Returns the messages of what differs."""
    msgs = []
    nb = len(tab) + 1
    want = expected_counts(kk, drawable, tab)
    got = out["counts"].astype(np.int64)
    for b in np.nonzero(got != want)[0][:8]:
        msgs.append(f"{what}: bucket {b} counts {got[b]} pairs, the reference {want[b]}")
    if msgs:
        return msgs
    slots = out["slots"]
    assert slots.shape == (nb, cap, 2)
    kept = np.minimum(want, cap)
    written = np.arange(cap)[None, :] < kept[:, None]
    bad = np.nonzero(~written & (slots != FILL).any(axis=2))
    for b, s in list(zip(*bad))[:8]:
        msgs.append(f"{what}: bucket {b} slot {s} (count {want[b]}) was written: key 0x{slots[b, s, 0]:08x} index {slots[b, s, 1]}")
    dev_b = np.nonzero(written)[0]
    dev = (slots[written][:, 0].astype(np.uint64) << np.uint64(32)) | slots[written][:, 1].astype(np.uint64)
    idx = np.nonzero(drawable)[0]
    ref_b = bucket_of(kk[idx], tab)
    ref = (kk[idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    # every written pair is a drawable splat with its own key ...
    di = slots[written][:, 1].astype(np.int64)
    ok = (di < len(kk))
    ok[ok] &= drawable[di[ok]] & (kk[di[ok]] == slots[written][:, 0][ok])
    # ... in its own bucket, once
    ok[ok] &= bucket_of(slots[written][:, 0][ok], tab) == dev_b[ok]
    for j in np.nonzero(~ok)[0][:8]:
        msgs.append(f"{what}: bucket {dev_b[j]} holds key 0x{int(dev[j]) >> 32:08x} index {int(dev[j]) & M32}, which the reference does not place there")
    if len(np.unique(dev)) != len(dev):
        msgs.append(f"{what}: {len(dev) - len(np.unique(dev))} pairs were written twice")
    fits = want <= cap
    a = np.sort(dev[fits[dev_b]])
    r = np.sort(ref[fits[ref_b]])
    if not np.array_equal(a, r):
        msgs.append(f"{what}: the buckets that fit hold {len(a)} pairs, the reference {len(r)}; as multisets they differ")
    return msgs
