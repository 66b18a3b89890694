"""The Python bindings of the two native libraries against what they bind. Each binding's prototype table agrees with the
C headers function by function (name, parameter count, return type): ctypes itself reports nothing when a header gains
a parameter the table does not pass, the library then reads a garbage argument. Each library's source hash is the recipe
written out here. And a stale or missing library is refused, with both ids named. No device, nothing is loaded."""
import ctypes
import hashlib
import os
import re

import pytest

from bevy_gaussian_splatting_amd import _build_id, _loader, _native, _native_query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bevy_gaussian_splatting_amd")
BINDINGS = {"libbgs": (_native, ("bgs.h", "bgs_diag.h"), "bgs_", 61),
            "libbgs_query": (_native_query, ("bgs_query.h",), "bgsq_", 8)}
RESTYPES = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "const char*": ctypes.c_char_p, "void": None}


def declarations(headers, prefix):
    """[(name, return type, parameter count)] of the functions the headers declare, in their order. Comments go first,
    then preprocessor lines: a #define directly above a declaration would otherwise read as part of its return type."""
    found = []
    for hname in headers:
        text = open(os.path.join(ROOT, "include", hname)).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        assert not re.search(r"^\s*#.*\\$", text, flags=re.M), f"{hname}: a continued preprocessor line"
        text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
        # a declaration starts where a statement or a block ended, or one opened (extern "C" {)
        for ret, name, params in re.findall(r"(?<=[;{}])\s*([A-Za-z_][\w\s*]*?)\b(%s[a-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefix, text):
            ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
            params = " ".join(params.split())
            found.append((name, ret, 0 if params == "void" else params.count(",") + 1))
    return found


@pytest.mark.parametrize("library", sorted(BINDINGS))
def test_prototype_table_agrees_with_the_headers(library):
    module, headers, prefix, count = BINDINGS[library]
    declared = declarations(headers, prefix)
    names = [name for name, _, _ in declared]
    assert len(names) == len(set(names)) == count
    # every name the headers call (the looser scan of test_abi / test_mesh_query_host) is a declaration found here
    loose = set()
    for hname in headers:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hname)).read(), flags=re.S)
        loose |= set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, text))
    assert loose == set(names)
    table = {name: (restype, argtypes) for name, restype, argtypes in module.PROTOTYPES}
    assert len(table) == len(module.PROTOTYPES), "a function is stated twice"
    assert set(table) == set(names), sorted(set(table) ^ set(names))
    assert [name for name, _, _ in module.PROTOTYPES] == names, "the table is in the headers' order"
    assert module.EXPORTED_SYMBOLS == tuple(names)
    for name, ret, nparams in declared:
        restype, argtypes = table[name]
        assert len(argtypes) == nparams, f"{name}: the header declares {nparams} parameters, the table passes {len(argtypes)}"
        assert ret in RESTYPES, f"{name}: return type {ret!r}"
        assert restype is RESTYPES[ret], f"{name}: the header returns {ret}, the table says {restype}"


def test_declare_applies_the_table():
    class Function:
        restype, argtypes = "unset", "unset"

    class Library:
        bgsq_version, bgsq_mesh_free = Function(), Function()

    lib = Library()
    rows = [r for r in _native_query.PROTOTYPES if r[0] in ("bgsq_version", "bgsq_mesh_free")]
    _loader.declare(lib, rows)
    assert lib.bgsq_version.restype is ctypes.c_uint32 and lib.bgsq_version.argtypes == []
    assert lib.bgsq_mesh_free.restype is None and lib.bgsq_mesh_free.argtypes == [ctypes.c_void_p]
    with pytest.raises(AttributeError):
        _loader.declare(lib, _native_query.PROTOTYPES)   # a row the library does not export


def test_both_source_hashes_are_the_recipes_written_out():
    """The recipes are part of the ids (a library built under another recipe is stale), so they are restated here by
    hand and not imported. libbgs: csrc/'s *.hip, *.h and Makefile in sorted order, name then bytes — not its map file,
    not include/. libbgs_query: the same over csrc_query/ with *.map as well, then include/bgs_query.h under its label."""
    csrc = os.path.join(PKG, "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".hip") or name.endswith(".h") or name == "Makefile":
            h.update(name.encode())
            h.update(open(os.path.join(csrc, name), "rb").read())
    assert _build_id.source_sha256(_build_id.LIBBGS) == _build_id.kernel_source_sha256() == h.hexdigest()
    csrc_query = os.path.join(PKG, "csrc_query")
    q = hashlib.sha256()
    for name in sorted(os.listdir(csrc_query)):
        if name.endswith(".hip") or name.endswith(".h") or name.endswith(".map") or name == "Makefile":
            q.update(name.encode())
            q.update(open(os.path.join(csrc_query, name), "rb").read())
    q.update(b"bgs_query.h")
    q.update(open(os.path.join(ROOT, "include", "bgs_query.h"), "rb").read())
    assert _build_id.source_sha256(_build_id.LIBBGS_QUERY) == q.hexdigest() != h.hexdigest()
    assert _build_id.MARKER == b"BGS_BUILD_ID=" and _build_id.LIBBGS_QUERY.marker == b"BGSQ_BUILD_ID="
    assert _native.LIB_PATH == os.path.join(csrc, "libbgs.so") and _native_query.LIB_PATH == os.path.join(csrc_query, "libbgs_query.so")


def test_the_script_prints_each_librarys_hash():
    import subprocess
    import sys
    script = os.path.join(PKG, "_build_id.py")
    run = lambda *args: subprocess.run([sys.executable, script, *args], check=True, capture_output=True, text=True).stdout.strip()
    assert run() == run("libbgs") == _build_id.kernel_source_sha256()
    assert run("libbgs_query") == _build_id.source_sha256(_build_id.LIBBGS_QUERY)


@pytest.mark.parametrize("library", sorted(_build_id.LIBRARIES))
def test_a_stale_or_missing_library_is_refused(library, tmp_path, monkeypatch):
    """File bytes only: a copy of the built library with the id's bytes replaced by zeros, and no file at all. With
    auto-build off the loader refuses both, each in its own words; the stale one with both 12-character prefixes."""
    spec = _build_id.LIBRARIES[library]
    want = _loader.ensure_current(spec, spec.path)   # (builds it if need be; does not load it)
    assert want == _build_id.source_sha256(spec) == _build_id.library_build_id(spec.path, spec) and len(want) == 64
    other = [s for s in _build_id.LIBRARIES.values() if s is not spec][0]
    assert _build_id.library_build_id(spec.path, other) is None   # each marker finds its own library's id only
    stale, missing = tmp_path / f"{library}_stale.so", tmp_path / "missing.so"
    stale.write_bytes(open(spec.path, "rb").read().replace(want.encode(), b"0" * 64))
    assert _build_id.library_build_id(str(stale), spec) == "0" * 64
    assert _build_id.library_build_id(str(missing), spec) is None
    monkeypatch.setenv("BGS_NO_AUTOBUILD", "1")
    with pytest.raises(ImportError) as ei:
        _loader.ensure_current(spec, str(stale))
    assert "000000000000" in str(ei.value) and want[:12] in str(ei.value) and str(stale) in str(ei.value)
    with pytest.raises(ImportError) as ei:
        _loader.ensure_current(spec, str(missing))
    assert "not found" in str(ei.value) and str(missing) in str(ei.value) and "000000000000" not in str(ei.value)
    assert not missing.exists()
    assert _loader.ensure_current(spec, spec.path) == want
