"""The Python bindings of the five native libraries against what they bind, and the one table that names the libraries.
Each binding's prototype table agrees with the C headers function by function (name, parameter count, return type):
ctypes itself reports nothing when a header gains a parameter the table does not pass, the library then reads a garbage
argument. Each library's source hash is the recipe written out here. A stale or missing library is refused, with both
ids named. The four small libraries are built by one recipe with libbgs's flags, and the host code their C ABI files
share runs clean under the sanitizers as a program of its own. No device; only that program and `make -n` are run."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest

from bevy_gaussian_splatting_amd import _build_id, _loader, _native, _native_morph, _native_query, _native_slice, _native_sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bevy_gaussian_splatting_amd")
SMALL_LIB = os.path.join(PKG, "small_lib")
# in build order: the binding, the headers it binds, the prefix of their functions and how many they declare
BINDINGS = {"libbgs": (_native, ("bgs.h", "bgs_diag.h"), "bgs_", 69),
            "libbgs_query": (_native_query, ("bgs_query.h",), "bgsq_", 8),
            "libbgs_sparse": (_native_sparse, ("bgs_sparse.h",), "bgss_", 8),
            "libbgs_slice": (_native_slice, ("bgs_slice.h",), "bgst_", 3),
            "libbgs_morph": (_native_morph, ("bgs_morph.h",), "bgsm_", 4)}
SMALL = [name for name in BINDINGS if name != "libbgs"]
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


def test_the_table_of_libraries_is_the_five_in_build_order():
    names = ["libbgs", "libbgs_query", "libbgs_sparse", "libbgs_slice", "libbgs_morph"]
    constants = [_build_id.LIBBGS, _build_id.LIBBGS_QUERY, _build_id.LIBBGS_SPARSE, _build_id.LIBBGS_SLICE, _build_id.LIBBGS_MORPH]
    assert list(_build_id.LIBRARIES) == names == list(BINDINGS)
    for name, constant in zip(names, constants):
        assert _build_id.LIBRARIES[name] is constant is BINDINGS[name][0].SPEC and constant.name == name
    assert len({spec.marker for spec in constants}) == 5 and len({_build_id.source_sha256(spec) for spec in constants}) == 5
    assert _build_id.MARKER == _build_id.LIBBGS.marker == b"BGS_BUILD_ID="
    assert not hasattr(_build_id, "BY_NAME")                 # one table: the script's argument indexes LIBRARIES


def test_source_hash_is_the_recipe_written_out():
    """The recipes are part of the ids (a library built under another recipe is stale), so they are restated here by
    hand and not imported. libbgs: csrc/'s *.hip, *.h and Makefile in sorted order, name then bytes — not its map file,
    not include/. A small library: the same over its own directory with *.map as well, then its public header, then
    small_lib/'s two support headers and library.mk, each of the four under its file name."""
    for library, (module, headers, prefix, _) in BINDINGS.items():
        small = library != "libbgs"
        directory = os.path.join(PKG, "csrc_" + library[len("libbgs_"):] if small else "csrc")
        h = hashlib.sha256()
        for name in sorted(os.listdir(directory)):
            if name.endswith(".hip") or name.endswith(".h") or (small and name.endswith(".map")) or name == "Makefile":
                h.update(name.encode())
                h.update(open(os.path.join(directory, name), "rb").read())
        if small:
            (header,) = headers
            h.update(header.encode())
            h.update(open(os.path.join(ROOT, "include", header), "rb").read())
            for name in ("api_support.h", "api_support_hip.h", "library.mk"):
                h.update(name.encode())
                h.update(open(os.path.join(SMALL_LIB, name), "rb").read())
        else:
            assert _build_id.kernel_source_sha256() == h.hexdigest()
        spec = _build_id.LIBRARIES[library]
        assert _build_id.source_sha256(spec) == h.hexdigest(), library
        assert spec.marker == prefix[:-1].upper().encode() + b"_BUILD_ID=", library
        assert module.LIB_PATH == spec.path == os.path.join(directory, library + ".so"), library


def test_the_script_prints_each_librarys_hash():
    script = os.path.join(PKG, "_build_id.py")
    run = lambda *args: subprocess.run([sys.executable, script, *args], check=True, capture_output=True, text=True).stdout.strip()
    assert run() == _build_id.kernel_source_sha256()
    for library, spec in _build_id.LIBRARIES.items():
        assert run(library) == _build_id.source_sha256(spec), library
    assert subprocess.run([sys.executable, script, "libbgs_none"], capture_output=True).returncode != 0


@pytest.mark.parametrize("library", sorted(_build_id.LIBRARIES))
def test_a_stale_or_missing_library_is_refused(library, tmp_path, monkeypatch):
    """File bytes only: a copy of the built library with the id's bytes replaced by zeros, and no file at all. With
    auto-build off the loader refuses both, each in its own words; the stale one with both 12-character prefixes."""
    spec = _build_id.LIBRARIES[library]
    want = _loader.ensure_current(spec, spec.path)   # (builds it if need be; does not load it)
    assert want == _build_id.source_sha256(spec) == _build_id.library_build_id(spec.path, spec) and len(want) == 64
    for other in _build_id.LIBRARIES.values():                    # each marker finds its own library's id only
        assert other is spec or _build_id.library_build_id(spec.path, other) is None
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


# ---- the small libraries' one build recipe and shared host code ---------------------------------------------------------------
def test_the_small_libraries_are_built_with_libbgs_flags():
    """The bit-exact contracts of the small libraries hold under the flags of csrc/Makefile. They are stated once more,
    in small_lib/library.mk, as the same line; no small library's Makefile sets them; and each one's hipcc line has them."""
    flags = lambda path: re.findall(r"^HIPFLAGS\b.*$", open(path).read(), flags=re.M)
    (line,) = flags(os.path.join(PKG, "csrc", "Makefile"))
    assert flags(os.path.join(SMALL_LIB, "library.mk")) == [line] and line.startswith("HIPFLAGS ?= --offload-arch=$(ARCH) -O3 ")
    assert "-ffp-contract=off" in line and "fast" not in line
    expanded = line[len("HIPFLAGS ?= "):].replace("$(ARCH)", "gfx950")
    for library in SMALL:
        directory = os.path.dirname(_build_id.LIBRARIES[library].path)
        makefile = open(os.path.join(directory, "Makefile")).read()
        assert "HIPFLAGS" not in makefile and "include ../small_lib/library.mk\n" in makefile, library
        dry = subprocess.run(["make", "-n", "-B", "-C", directory, "ARCH=gfx950"], check=True, capture_output=True, text=True).stdout
        compiles = [row for row in dry.splitlines() if "hipcc" in row]
        assert len(compiles) == 1 and f"hipcc {expanded} -shared -Wl,--version-script={library}.map -o {library}.so " in compiles[0], dry


def test_the_shared_files_know_no_library():
    assert sorted(os.listdir(SMALL_LIB)) == ["api_support.h", "api_support_hip.h", "library.mk"]
    for name in os.listdir(SMALL_LIB):
        text = open(os.path.join(SMALL_LIB, name)).read()
        for _, _, prefix, _ in BINDINGS.values():
            assert prefix == "bgs_" or (prefix not in text.lower()), (name, prefix)
        assert "csrc/" not in text.replace("../csrc/Makefile", "") and "bgs.h" not in text and "include/" not in text, name
    assert not re.search(r"\bhip[A-Z_/]", open(os.path.join(SMALL_LIB, "api_support.h")).read())   # no HIP in the first one
    for library in SMALL:                                    # the C ABI file takes them; the kernels and the arithmetic do not
        directory = os.path.dirname(_build_id.LIBRARIES[library].path)
        takes = sorted(n for n in os.listdir(directory) if n.endswith((".hip", ".h")) and "small_lib/" in open(os.path.join(directory, n)).read())
        assert takes == ["bgs_%s_api.hip" % library[len("libbgs_"):]]


def test_the_shared_api_support_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/api_support_tool.cpp: g++ -fsanitize=address,undefined -fno-sanitize-recover, a main of its own, no Python
    in the process. It holds every answer against the expected one itself and ends clean; the lines it prints are read
    once more here: the cut message, the replaced one, and the three refusals in the words the libraries' tests expect."""
    exe = tmp_path / "api_support_tool"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "api_support_tool.cpp"), "-o", str(exe)], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout.splitlines() == [
        "-3 fn: " + "x" * 507,
        "-2 second 2",
        "0 ",
        "-1 fn: in_a is NULL",
        "-1 fn: in_c is NULL",
        "-1 fn: out_b is NULL",
        "-1 fn: in_b must be a 16-byte aligned device address",
        "-1 fn: out_a must be a 16-byte aligned device address",
        "-1 fn: in_b must be a 16-byte aligned device address",
        "-1 fn: out_a is in_b as well",
        "-1 fn: out_b is out_a as well",
        "0 ",
        "0 "]
