"""include/chunky_ec_parts.h (the ragged write pipeline's part of the C-ABI) against the Rust
crate's `sys::parts` extern block and the library, by the rules tests/test_rust_conformance.py and
tests/test_capi.py apply to include/chunky_ec.h: the same functions on both sides, the same arity,
every parameter and return type matching in kind; every `sys::parts::cec_*` call of the crate
declared; every declared function exported by the library; and chunky_ec.h brings the header
along, so the two are one ABI."""
import os
import re

import pytest

import chunky_ec as ce
import test_rust_conformance as conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS_HEADER = os.path.join(ROOT, "include", "chunky_ec_parts.h")
EXPECTED = {"cec_parts_pipeline_new", "cec_parts_pipeline_free", "cec_parts_pipeline_depth",
            "cec_parts_pipeline_acquire", "cec_parts_pipeline_submit",
            "cec_parts_pipeline_submit_from", "cec_parts_pipeline_wait",
            "cec_parts_pipeline_query", "cec_parts_pipeline_drain"}


def _header_functions(monkeypatch):
    # the conformance module's parser, on this header, with the one handle type this header adds
    monkeypatch.setitem(conf.C_BASE, "cec_parts_pipeline", "cec_parts_pipeline")
    monkeypatch.setattr(conf, "HEADER", PARTS_HEADER)
    return conf.header_functions()


def _rust_parts_functions():
    src = open(conf.RUST).read()
    mod = re.search(r'pub mod parts \{(.*?)\n    \}', src, flags=re.S).group(1)
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


def test_rust_parts_block_declares_the_header_with_matching_types(monkeypatch):
    h, r = _header_functions(monkeypatch), _rust_parts_functions()
    assert set(h) == EXPECTED
    assert sorted(h) == sorted(r), (sorted(set(h) - set(r)), sorted(set(r) - set(h)))
    for name in h:
        hret, hps = h[name]
        rret, rps = r[name]
        assert len(hps) == len(rps), name
        assert hret == rret, (name, hret, rret)
        for i, (a, b) in enumerate(zip(hps, rps)):
            assert a == b, (name, i, a, b)
    # the handle is the opaque struct of the crate's sys module
    assert re.search(r"pub struct cec_parts_pipeline \{\s*_private: \[u8; 0\],\s*\}",
                     open(conf.RUST).read())


def test_every_parts_ffi_use_is_declared():
    declared = set(_rust_parts_functions())
    used = set()
    for name, src in conf._crate_sources().items():
        used |= set(re.findall(r"sys::parts::(cec_[a-z0-9_]+)\s*\(", src))
        # no call reaches the pipeline past the parts block
        assert not re.findall(r"sys::(cec_parts_pipeline_[a-z_]+)\s*\(", src), name
    assert used == declared, (sorted(used - declared), sorted(declared - used))


def test_main_header_brings_the_parts_header_and_keeps_the_split_calls():
    main = conf._strip_c_comments(open(os.path.join(ROOT, "include", "chunky_ec.h")).read())
    assert '#include "chunky_ec_parts.h"' in main
    assert "cec_parts_pipeline" not in main  # declared once, in its own header
    for name in ("cec_split_layout", "cec_encode_hash_split"):
        assert re.search(rf"\bint {name}\s*\(", main), name
    parts = conf._strip_c_comments(open(PARTS_HEADER).read())
    assert '#include "chunky_ec.h"' in parts
    assert "typedef struct cec_parts_pipeline cec_parts_pipeline;" in parts


def test_library_exports_and_python_binds_every_parts_function(monkeypatch):
    for name in _header_functions(monkeypatch):
        fn = getattr(ce._lib, name)  # AttributeError: not exported
        assert fn.argtypes is not None, name  # bound with a signature in chunky_ec/__init__.py


@pytest.mark.parametrize("compiler,std,lang", [("gcc", "c99", "c"), ("gcc", "c11", "c"),
                                               ("g++", "c++17", "cpp")])
def test_parts_header_compiles_on_its_own(tmp_path, compiler, std, lang):
    """Included first and alone, it gives the whole ABI (it includes chunky_ec.h, which includes
    it): a pipeline call and a chunky_ec.h call in one translation unit, warnings as errors."""
    from test_headers import _compile
    src = ('#include "chunky_ec_parts.h"\n'
           'int main(void) {\n'
           '    cec_parts_pipeline* pl = 0;\n'
           '    return (int)cec_parts_pipeline_depth(pl) + (int)cec_ragged_stride(0);\n'
           '}\n')
    _compile(compiler, std, lang, src, tmp_path)


def test_parts_header_is_part_of_the_build_provenance():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "chunky-bits_amd", "csrc"))
    try:
        import source_hash as sh
    finally:
        sys.path.pop(0)
    assert "include/chunky_ec_parts.h" in sh.source_files()
    assert ce.BUILD_MATCHES_SOURCE
