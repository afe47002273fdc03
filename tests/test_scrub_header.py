"""include/chunky_ec_scrub.h (the segmented scrub and the scrub pipeline) against the Rust crate's
`sys::scrub` extern block and the library, by the rules tests/test_segments_header.py applies to
include/chunky_ec_segments.h: the same functions on both sides, the same arity, every parameter
and return type matching in kind; every declared function exported by the library and bound with a
signature by the Python binding; chunky_ec.h brings the header along and declares nothing of it; it
compiles on its own as C99, C11 and C++17; and the header and the new sources are part of the
build provenance."""
import os
import re

import pytest

import chunky_ec as ce
import test_rust_conformance as conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chunky_ec_scrub.h")
EXPECTED = {"cec_verify_segments", "cec_scrub_pipeline_new", "cec_scrub_pipeline_free",
            "cec_scrub_pipeline_depth", "cec_scrub_pipeline_acquire",
            "cec_scrub_pipeline_submit_from", "cec_scrub_pipeline_wait",
            "cec_scrub_pipeline_query", "cec_scrub_pipeline_drain",
            "cec_scrub_pipeline_open_count", "cec_scrub_pipeline_abandon"}


def _header_functions(monkeypatch):
    # the conformance module's parser, on this header, with the types this header adds
    monkeypatch.setitem(conf.C_BASE, "cec_scrub_pipeline", "cec_scrub_pipeline")
    monkeypatch.setitem(conf.C_BASE, "uint32_t", "u32")
    monkeypatch.setattr(conf, "HEADER", HEADER)
    return conf.header_functions()


def _rust_functions():
    src = open(conf.RUST).read()
    mod = re.search(r'pub mod scrub \{(.*?)\n    \}', src, flags=re.S).group(1)
    block = re.search(r'extern "C"\s*\{(.*?)\n        \}', mod, flags=re.S).group(1)
    block = re.sub(r"//[^\n]*", "", block)
    out = {}
    for m in re.finditer(r"pub fn (cec_[a-z0-9_]+)\s*\((.*?)\)\s*(->\s*([^;]+))?;", block,
                         flags=re.S):
        name, params, ret = m.group(1), m.group(2), m.group(4)
        ps = [p.strip() for p in params.split(",") if p.strip()]
        out[name] = (conf.rust_type(ret) if ret else "c_void",
                     [conf.rust_type(p.split(":", 1)[1]) for p in ps])
    return mod, out


def test_rust_block_declares_the_header_with_matching_types(monkeypatch):
    h = _header_functions(monkeypatch)
    mod, r = _rust_functions()
    assert set(h) == EXPECTED
    assert sorted(h) == sorted(r), (sorted(set(h) - set(r)), sorted(set(r) - set(h)))
    for name in h:
        hret, hps = h[name]
        rret, rps = r[name]
        assert len(hps) == len(rps), name
        assert hret == rret, (name, hret, rret)
        for i, (a, b) in enumerate(zip(hps, rps)):
            assert a == b, (name, i, a, b)
    assert len(h["cec_verify_segments"][1]) == 11
    assert len(h["cec_scrub_pipeline_new"][1]) == 5
    assert len(h["cec_scrub_pipeline_submit_from"][1]) == 9
    assert len(h["cec_scrub_pipeline_wait"][1]) == 4
    # the handle is an opaque struct of the crate's sys module
    assert re.search(r"pub struct cec_scrub_pipeline \{\s*_private: \[u8; 0\],\s*\}",
                     open(conf.RUST).read())
    # the flags are the segments header's, which this header brings: one definition, the same
    # values in the crate's segments block and in the Python binding
    assert "#define CEC_SEG_" not in open(HEADER).read()
    seg = open(os.path.join(ROOT, "include", "chunky_ec_segments.h")).read()
    rust = open(conf.RUST).read()
    for const, py in (("CEC_SEG_FIRST", ce.SEG_FIRST), ("CEC_SEG_LAST", ce.SEG_LAST)):
        cv = int(re.search(rf"#define {const}\s+(\d+)u", seg).group(1))
        rv = int(re.search(rf"pub const {const}:[^=]+=\s*(\d+);", rust).group(1))
        assert cv == rv == py, const
    assert "pub const" not in mod  # and no second copy of them in the scrub block


def test_the_crate_declares_and_adds_no_loop():
    for name, src in conf._crate_sources().items():
        # no call reaches the scrub calls past their block
        assert not re.findall(r"sys::(?:scrub::)?(cec_scrub_pipeline_[a-z_]+)\s*\(", src), name
        assert not re.findall(r"sys::(?:scrub::)?(cec_verify_segments)\s*\(", src), name


def test_main_header_brings_the_header_and_declares_nothing_of_it():
    main = conf._strip_c_comments(open(os.path.join(ROOT, "include", "chunky_ec.h")).read())
    assert '#include "chunky_ec_scrub.h"' in main
    assert "cec_scrub_pipeline" not in main and "cec_verify_segments" not in main
    for other in ("chunky_ec_parts.h", "chunky_ec_parts_read.h", "chunky_ec_segments.h"):
        src = conf._strip_c_comments(open(os.path.join(ROOT, "include", other)).read())
        assert "cec_scrub" not in src and "cec_verify_segments" not in src, other
    own = conf._strip_c_comments(open(HEADER).read())
    assert '#include "chunky_ec.h"' in own
    assert "typedef struct cec_scrub_pipeline cec_scrub_pipeline;" in own


def test_library_exports_and_python_binds_every_function(monkeypatch):
    h = _header_functions(monkeypatch)
    for name, (ret, params) in h.items():
        fn = getattr(ce._lib, name)  # AttributeError: not exported
        assert fn.argtypes is not None, name  # bound with a signature in chunky_ec/__init__.py
        assert len(fn.argtypes) == len(params), name
    assert callable(ce.verify_segments) and isinstance(ce.ScrubPipeline, type)
    for method in ("acquire", "submit_from", "wait", "query", "drain", "open_count", "abandon"):
        assert callable(getattr(ce.ScrubPipeline, method)), method
        assert callable(getattr(ce.SegmentPipeline, method)), method  # the same shape


@pytest.mark.parametrize("compiler,std,lang", [("gcc", "c99", "c"), ("gcc", "c11", "c"),
                                               ("g++", "c++17", "cpp")])
def test_header_compiles_on_its_own(tmp_path, compiler, std, lang):
    """Included first and alone, it gives the whole ABI: a scrub call, a segment pipeline call and
    a chunky_ec.h call in one translation unit, warnings as errors."""
    from test_headers import _compile
    src = ('#include "chunky_ec_scrub.h"\n'
           'int main(void) {\n'
           '    cec_scrub_pipeline* sc = 0;\n'
           '    cec_segment_pipeline* sp = 0;\n'
           '    unsigned whole = CEC_SEG_FIRST | CEC_SEG_LAST;\n'
           '    return (int)cec_scrub_pipeline_depth(sc) + (int)cec_segment_pipeline_depth(sp) +\n'
           '           (int)cec_scrub_pipeline_open_count(sc) + (int)cec_ragged_stride(0) +\n'
           '           (int)cec_sha_midstate_bytes() + (int)whole;\n'
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
    for rel in ("include/chunky_ec_scrub.h", "chunky-bits_amd/csrc/scrub_pipeline.cpp",
                "chunky-bits_amd/csrc/scrub_words.hpp",
                "chunky-bits_amd/csrc/sha256_resume_kernels.hip"):
        assert rel in files, rel
    assert ce.BUILD_MATCHES_SOURCE
    mk = open(os.path.join(ROOT, "chunky-bits_amd", "csrc", "Makefile")).read()
    assert "scrub_pipeline.o" in mk and "scrub_words.hpp" in mk
    assert "scrub_words_test" in mk and "verify_many_stream_test" in mk
