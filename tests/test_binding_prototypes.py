"""The binding's statement of the ABI (spectrogram_midi_amd/_abi.py) held against include/aegis_hip.h: every prototype
argument by argument, every structure's layout through the host C compiler, and that nothing else in the package binds a
function.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import pytest

from spectrogram_midi_amd import _abi, events_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aegis_hip.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double,
           "float": C.c_float}


def _declarations():
    """name -> (return type, [argument types]) of every `ret aegis_x(args);` of the header, as C text without the
    argument names: "const aegis_config *", "int32_t", ..."""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    src = re.sub(r"(?m)^\s*#.*$", " ", src)
    out = {}
    for chunk in src.split(";"):
        if "(" not in chunk:
            continue
        m = re.fullmatch(r"\s*(.*?)\b(aegis_\w+)\s*\((.*)\)\s*", chunk, re.S)
        assert m, chunk
        args = [] if m.group(3).strip() == "void" else [re.sub(r"\w+\s*$", "", a.strip()) for a in m.group(3).split(",")]
        out[m.group(2)] = (" ".join(m.group(1).split()), [" ".join(a.split()) for a in args])
    return out


DECLS = _declarations()


def _agrees(ctype, ctext):
    """Does the table's type stand for the header's?  Scalars by exact type; anything with a `*` by a pointer type, whose
    target is checked where the table names one."""
    base = ctext.replace("const", "").replace("*", "").strip()
    depth = ctext.count("*")
    if depth == 0:
        return ctype is (None if base == "void" else SCALARS[base])
    if ctype is C.c_void_p:
        return True
    if ctype is C.c_char_p:
        return depth == 1 and base in ("char", "uint8_t")
    if not (isinstance(ctype, type) and issubclass(ctype, C._Pointer)):
        return False
    if depth == 2:
        return ctype._type_ is C.c_void_p
    return ctype._type_ is {**SCALARS, **_abi.STRUCTS, "uint8_t": C.c_uint8, "int16_t": C.c_int16}.get(base, "no typed pointer")


def test_the_parser_reads_the_header():
    assert len(DECLS) > 40
    assert DECLS["aegis_abi_version"] == ("int", [])
    assert DECLS["aegis_last_error"] == ("const char *", ["const aegis_handle *"])
    assert DECLS["aegis_create"] == ("int", ["const aegis_config *", "aegis_handle **"])
    assert DECLS["aegis_analyze_batch"][1][1:4] == ["const float *const *", "const int64_t *", "int32_t"]
    # the comparison itself tells widths and targets apart
    assert _agrees(C.c_int64, "int64_t") and not _agrees(C.c_int32, "int64_t") and not _agrees(C.c_int64, "const int64_t *")
    assert _agrees(C.POINTER(_abi.Config), "const aegis_config *") and not _agrees(C.POINTER(_abi.Outputs), "const aegis_config *")
    assert _agrees(C.POINTER(C.c_int64), "int64_t *") and not _agrees(C.POINTER(C.c_int32), "int64_t *")
    assert not _agrees(C.c_char_p, "const double *") and not _agrees(C.c_double, "float")


def test_every_declared_function_has_a_prototype_and_no_other():
    assert set(DECLS) == set(_abi.PROTOTYPES)
    assert _abi.EXPORTS == tuple(_abi.PROTOTYPES)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_prototype_matches_the_header(name):
    ret, args = DECLS[name]
    restype, argtypes = _abi.PROTOTYPES[name]
    assert _agrees(restype, ret), (restype, ret)
    assert len(argtypes) == len(args), (len(argtypes), args)
    for i, (t, a) in enumerate(zip(argtypes, args)):
        assert _agrees(t, a), (i, t, a)


def _layout(kind):
    """[(field, offset, size)] of a ctypes Structure or of a NumPy record dtype."""
    if isinstance(kind, type):
        return C.sizeof(kind), [(f[0], getattr(kind, f[0]).offset, getattr(kind, f[0]).size) for f in kind._fields_]
    return kind.itemsize, [(n, kind.fields[n][1], kind.fields[n][0].itemsize) for n in kind.names]


def test_structures_have_the_headers_layout(tmp_path):
    """A C program that includes the header prints sizeof and, per field, offsetof and the field's size; a field name the
    header lacks fails the compile.  The record dtypes that cross the boundary as arrays of structs are held to it too."""
    mirrors = [(n, c) for n, c in _abi.STRUCTS.items()]
    mirrors += [("aegis_synth_note", _abi.SYNTH_NOTE_DTYPE), ("aegis_synth_wheel", _abi.SYNTH_WHEEL_DTYPE),
                ("aegis_event", events_native.EVENT_DTYPE), ("aegis_run_fit", events_native.FIT_DTYPE)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "aegis_hip.h"', "int main(void) {"]
    want = []
    for k, (name, kind) in enumerate(mirrors):
        size, fields = _layout(kind)
        lines.append(f'    printf("{k} - %zu 0\\n", sizeof({name}));')
        want.append(f"{k} - {size} 0")
        for field, off, fsize in fields:
            lines.append(f'    printf("{k} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name} *)0)->{field}));')
            want.append(f"{k} {field} {off} {fsize}")
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(want) > 80
    for g, w in zip(got, want):
        assert g == w, (mirrors[int(w.split()[0])][0], "header: " + g, "binding: " + w)
    assert len(got) == len(want)


def test_load_applies_the_table():
    lib = _abi.load()
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        fn = getattr(lib, name)        # the built library has every entry (test_header_symbols_are_exported)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_a_library_that_lacks_entries_loads_without_them(tmp_path, monkeypatch):
    """load()'s one rule for a missing symbol (an older build behind AEGIS_HIP_LIB): skipped, AttributeError on use; the
    entries it has are bound; another ABI version is refused before anything is bound."""
    def stub(version):
        src, so = tmp_path / f"stub{version}.c", tmp_path / f"libstub{version}.so"
        src.write_text(f"int aegis_abi_version(void) {{ return {version}; }}\n"
                       "long long aegis_frames_for(const void *h, long long n) { return n + 1; }\n")
        subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True, capture_output=True)
        return str(so)

    monkeypatch.setattr(_abi, "_loaded", None)
    monkeypatch.setattr(_abi, "LIB_PATH", stub(_abi.ABI_VERSION))
    lib = _abi.load()
    assert lib.aegis_frames_for.restype is C.c_int64 and lib.aegis_frames_for(None, 1 << 40) == (1 << 40) + 1
    with pytest.raises(AttributeError):
        lib.aegis_salience
    monkeypatch.setattr(_abi, "_loaded", None)
    monkeypatch.setattr(_abi, "LIB_PATH", stub(_abi.ABI_VERSION + 1))
    with pytest.raises(ImportError, match="ABI version"):
        _abi.load()


def test_nothing_else_binds_a_function():
    """No argtypes or restype assignment in the package's own sources but the two of load()'s loop."""
    pkg = os.path.dirname(os.path.abspath(_abi.__file__))
    hits = []
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            for line in open(os.path.join(pkg, fn)):
                if re.search(r"\b(argtypes|restype)\s*=(?!=)", line):
                    hits.append((fn, line.strip()))
    assert hits == [("_abi.py", "fn.restype = restype"), ("_abi.py", "fn.argtypes = argtypes")]
