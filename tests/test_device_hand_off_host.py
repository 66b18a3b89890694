"""The device hand-off's host side: what `upload_device_planes` refuses before any library call, and what the documents
and include/bgs.h must say about device planes. No GPU."""
import os
import re

import pytest

from bevy_gaussian_splatting_amd import GaussianSplattingPlugin
from bevy_gaussian_splatting_amd.plugin import DEVICE_PLANE_FORMATS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


class NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


@pytest.fixture()
def bare_plugin():
    """A plugin object without a context or a library: what is validated on the host needs neither."""
    p = object.__new__(GaussianSplattingPlugin)
    p._lib, p._ctx, p.device = NoLibrary(), None, 0
    return p


def test_upload_device_planes_rejects_a_wrong_format_on_the_host(bare_plugin):
    for fmt in ("f64", "", "F32", "cov3d_f32", None, 3):
        with pytest.raises(ValueError, match="fmt must be one of"):
            bare_plugin.upload_device_planes(fmt, 4, [0x1000, 0x2000, 0x3000])


def test_upload_device_planes_rejects_a_wrong_pointer_count_on_the_host(bare_plugin):
    assert {k: len(v[1]) for k, v in DEVICE_PLANE_FORMATS.items()} == {"f32": 4, "f16": 3, "cov3d": 3}
    for fmt, (entry, names, _) in DEVICE_PLANE_FORMATS.items():
        for count in (0, len(names) - 1, len(names) + 1):
            with pytest.raises(ValueError, match=f"{entry} takes {len(names)} planes") as ei:
                bare_plugin.upload_device_planes(fmt, 4, [0x1000 * (k + 1) for k in range(count)])
            assert all(name in str(ei.value) for name in names)             # the message lists the planes in order
    with pytest.raises(ValueError, match="n must be >= 0"):
        bare_plugin.upload_device_planes("f32", -1, [0x1000, 0x2000, 0x3000, 0x4000])


def test_the_formats_name_the_c_entry_points_in_argument_order():
    """The order of `pointers` is the order of the C declaration's plane arguments."""
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    for entry, names, splat_bytes in DEVICE_PLANE_FORMATS.values():
        decl = re.search(r"int %s\(bgs_ctx\* ctx, uint32_t n,([^;]*)bgs_cloud\*\* out\);" % entry, header).group(1)
        assert re.findall(r"\*\s*(\w+)\s*,", decl) == list(names), entry
    assert [v[2] for v in DEVICE_PLANE_FORMATS.values()] == [240, 128, 240]


def section(doc, number):
    start = doc.index(f"## {number}. ")
    return doc[start:doc.index("\n## ", start + 1)]


def test_the_integration_sections_give_the_device_order():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for number, producer, upload in (("2d", "bgst_slice", "bgs_cloud_upload_cov3d_f32"), ("2e", "bgsm_interpolate_f32", "bgs_cloud_upload_f32")):
        text = " ".join(section(doc, number).split())          # (line breaks are not content)
        assert "goes through the host" not in text and "through the host" not in text, number
        assert "stays on the device" in text
        # the device order: produce, upload from the output planes, sort and render, free before the next
        at = [text.index(s) for s in (f"produce: `{producer}", f"`{upload}(ctx, n", "OUTPUT", "`bgs_sort` / `bgs_render`", "`bgs_cloud_free`")]
        assert at == sorted(at), number
        # ... the host order kept as the alternative, and whose the bounds are
        assert "alternative" in text and "`bgs_download`" in text and "`bgs_synchronize(ctx)` after step" in text
        assert re.search(r"`position_min` /\s+`position_max`[^.]*remain the caller's, as with the particle step", text), number
        assert "bgs_stream(ctx)" in text
    assert "playback_update" in section(doc, "2d") and "PlaybackMode" in section(doc, "2d")


def test_bgs_h_states_the_device_plane_contract():
    header = open(os.path.join(ROOT, "include", "bgs.h")).read()
    start = header.index("DEVICE PLANES")
    comment = " ".join(header[start:header.index("int bgs_cloud_upload_f32", start)].replace(" * ", " ").split())
    for phrase in ("either host memory or device memory of the context's device", "may be mixed", "16-byte aligned",
                   "BGS_EINVAL, naming the plane", "device memory of another device",
                   "enqueued on the stream bgs_stream(ctx) names BEFORE the call", "never writes a plane of the caller's",
                   "synchronises its own stream", "n == 0 is BGS_OK"):
        assert phrase in comment, phrase
    for name in ("bgs_slice.h", "bgs_morph.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        ordering = text[text.index("ORDERING"):text.index("#ifndef")]
        assert "no entry point that takes planes by device address" not in ordering and "through the host" not in ordering
        assert "DEVICE PLANES" in ordering and "no synchronisation after it" in ordering
    for doc, gone in (("SURVEY.md", "device-side hand-off stay out of scope"), ("README.md", "through the host for now")):
        assert gone not in open(os.path.join(ROOT, doc)).read()
