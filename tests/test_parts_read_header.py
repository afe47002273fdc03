"""include/chunky_ec_parts_read.h (the ragged read with a packed return and the ragged read
pipeline) against the Rust crate's `sys::parts_read` extern block and the library, by the rules
tests/test_parts_header.py applies to include/chunky_ec_parts.h: the same functions on both sides,
the same arity, every parameter and return type matching in kind; every `sys::parts_read::cec_*`
call of the crate declared and every declared function used; every declared function exported by
the library and bound with a signature by the Python binding; chunky_ec.h brings the header
along; and the header is part of the build provenance."""
import os
import re

import pytest

import chunky_ec as ce
import test_rust_conformance as conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chunky_ec_parts_read.h")
EXPECTED = {"cec_read_ragged_packed_async", "cec_parts_reader_new", "cec_parts_reader_free",
            "cec_parts_reader_depth", "cec_parts_reader_acquire", "cec_parts_reader_submit",
            "cec_parts_reader_submit_from", "cec_parts_reader_wait", "cec_parts_reader_scatter",
            "cec_parts_reader_query", "cec_parts_reader_drain", "cec_parts_reader_stats"}


def _header_functions(monkeypatch):
    # the conformance module's parser, on this header, with the one handle type this header adds
    monkeypatch.setitem(conf.C_BASE, "cec_parts_reader", "cec_parts_reader")
    monkeypatch.setattr(conf, "HEADER", HEADER)
    return conf.header_functions()


def _rust_functions():
    src = open(conf.RUST).read()
    mod = re.search(r'pub mod parts_read \{(.*?)\n    \}', src, flags=re.S).group(1)
    block = re.search(r'extern "C"\s*\{(.*?)\n        \}', mod, flags=re.S).group(1)
    block = re.sub(r"//[^\n]*", "", block)
    out = {}
    for m in re.finditer(r"pub fn (cec_[a-z0-9_]+)\s*\((.*?)\)\s*(->\s*([^;]+))?;", block,
                         flags=re.S):
        name, params, ret = m.group(1), m.group(2), m.group(4)
        ps = [p.strip() for p in params.split(",") if p.strip()]
        out[name] = (conf.rust_type(ret) if ret else "c_void",
                     [conf.rust_type(p.split(":", 1)[1]) for p in ps])
    return out


def test_rust_block_declares_the_header_with_matching_types(monkeypatch):
    h, r = _header_functions(monkeypatch), _rust_functions()
    assert set(h) == EXPECTED
    assert sorted(h) == sorted(r), (sorted(set(h) - set(r)), sorted(set(r) - set(h)))
    for name in h:
        hret, hps = h[name]
        rret, rps = r[name]
        assert len(hps) == len(rps), name
        assert hret == rret, (name, hret, rret)
        for i, (a, b) in enumerate(zip(hps, rps)):
            assert a == b, (name, i, a, b)
    assert len(h["cec_read_ragged_packed_async"][1]) == 14
    # the handle is an opaque struct of the crate's sys module
    assert re.search(r"pub struct cec_parts_reader \{\s*_private: \[u8; 0\],\s*\}",
                     open(conf.RUST).read())


def test_every_ffi_use_is_declared_and_every_declaration_used():
    declared = set(_rust_functions())
    used = set()
    for name, src in conf._crate_sources().items():
        used |= set(re.findall(r"sys::parts_read::(cec_[a-z0-9_]+)\s*\(", src))
        # no call reaches the reader past its block
        assert not re.findall(r"sys::(cec_parts_reader_[a-z_]+)\s*\(", src), name
        assert not re.findall(r"sys::(cec_read_ragged_packed_async)\s*\(", src), name
    assert used == declared, (sorted(used - declared), sorted(declared - used))
    lib = open(conf.RUST).read()
    for s in ("pub struct PartsReader", "pub struct PartsReadResult",
              "pub unsafe fn read_ragged_packed_async("):
        assert s in lib, s


def test_main_header_brings_the_header_and_declares_nothing_of_it():
    main = conf._strip_c_comments(open(os.path.join(ROOT, "include", "chunky_ec.h")).read())
    assert '#include "chunky_ec_parts_read.h"' in main
    assert "cec_parts_reader" not in main and "cec_read_ragged_packed_async" not in main
    parts = conf._strip_c_comments(open(os.path.join(ROOT, "include", "chunky_ec_parts.h")).read())
    assert "cec_parts_reader" not in parts  # the write pipeline's header keeps its function set
    own = conf._strip_c_comments(open(HEADER).read())
    assert '#include "chunky_ec.h"' in own
    assert "typedef struct cec_parts_reader cec_parts_reader;" in own


def test_library_exports_and_python_binds_every_function(monkeypatch):
    for name in _header_functions(monkeypatch):
        fn = getattr(ce._lib, name)  # AttributeError: not exported
        assert fn.argtypes is not None, name  # bound with a signature in chunky_ec/__init__.py
    h = _header_functions(monkeypatch)
    for name, (ret, params) in h.items():
        assert len(getattr(ce._lib, name).argtypes) == len(params), name
    assert callable(ce.read_ragged_packed_async) and isinstance(ce.PartsReader, type)


@pytest.mark.parametrize("compiler,std,lang", [("gcc", "c99", "c"), ("gcc", "c11", "c"),
                                               ("g++", "c++17", "cpp")])
def test_header_compiles_on_its_own(tmp_path, compiler, std, lang):
    """Included first and alone, it gives the whole ABI: a reader call, a write pipeline call and a
    chunky_ec.h call in one translation unit, warnings as errors."""
    from test_headers import _compile
    src = ('#include "chunky_ec_parts_read.h"\n'
           'int main(void) {\n'
           '    cec_parts_reader* rd = 0;\n'
           '    cec_parts_pipeline* pl = 0;\n'
           '    return (int)cec_parts_reader_depth(rd) + (int)cec_parts_pipeline_depth(pl) +\n'
           '           (int)cec_ragged_stride(0);\n'
           '}\n')
    _compile(compiler, std, lang, src, tmp_path)


def test_header_and_sources_are_part_of_the_build_provenance():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "chunky-bits_amd", "csrc"))
    try:
        import source_hash as sh
    finally:
        sys.path.pop(0)
    files = sh.source_files()
    for rel in ("include/chunky_ec_parts_read.h", "chunky-bits_amd/csrc/ragged_read_pipeline.cpp",
                "chunky-bits_amd/csrc/return_plan.hpp"):
        assert rel in files, rel
    assert ce.BUILD_MATCHES_SOURCE
    mk = open(os.path.join(ROOT, "chunky-bits_amd", "csrc", "Makefile")).read()
    assert "ragged_read_pipeline.o" in mk and "return_plan.hpp" in mk
