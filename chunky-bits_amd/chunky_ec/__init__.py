"""chunky_ec — Python host binding of the MI355X erasure-coding + chunk-hashing engine.

Thin ctypes layer over ``libchunky_ec.so`` (C-ABI declared in ``include/chunky_ec.h``), shaped
like the Rust API the reference calls on its hot path so that tests read like the reference's:

* :class:`ReedSolomon` — ``reed_solomon_erasure::ReedSolomon<galois_8::Field>``
  (``new`` / ``encode_sep`` / ``reconstruct`` / ``reconstruct_data``; call sites
  src/file/file_part.rs:77,128,161-165,302-304).
* :class:`Sha256Hash` / :class:`AnyHash` — src/file/hash/{sha256,any}.rs (``from_buf``,
  ``verify``, ``sha256-<hex>`` display).
* :class:`Error` — ``reed_solomon_erasure::Error`` variants (wrapped by
  ``FileWriteError::Erasure`` / ``FileReadError::Erasure``, src/error.rs:44,55).
* :func:`part_encode` and the ``*_batch`` functions — the part layer's compute
  (``FilePart::write_with_encoder`` / ``read_with_context`` / ``resilver`` / ``verify``,
  src/file/file_part.rs:73-390), batched over parts resident in HBM.

Host loops built on these (submodules): :mod:`chunky_ec.readstream` (FileReadBuilder's part
loop over a ReadPipeline with read_with_context's retry rule), :mod:`chunky_ec.batchwriter` /
:mod:`chunky_ec.batchreader` (the batched FileWriteBuilder / FileReadBuilder loops over the
multi-GPU scheduler: twins of the Rust crate's ``batch`` module), :mod:`chunky_ec.sharding`
(part ranges and the bench's cross-rank helpers).

All computation runs in the HIP library on the GPU; there is no CPU fallback.  If the
library is missing this module raises on import.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, MutableSequence, Optional, Sequence

try:  # torch ships its own libamdhip64.so.7: load it first so one HIP runtime serves both.
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the host-buffer API
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# CEC_LIBRARY loads another build of the library (the host-sanitizer build, `make -C
# chunky-bits_amd/csrc asan`); everything else loads the library next to this file.
LIB_PATH = os.environ.get("CEC_LIBRARY") or os.path.join(_HERE, "libchunky_ec.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"chunky_ec: HIP library not built ({LIB_PATH}); run `make -C chunky-bits_amd/csrc` "
        "or __graft_entry__.build()")

_lib = ctypes.CDLL(LIB_PATH)

_u8p = ctypes.POINTER(ctypes.c_uint8)
_szp = ctypes.POINTER(ctypes.c_size_t)
_vp = ctypes.c_void_p


class PartBatchStruct(ctypes.Structure):
    _fields_ = [
        ("base", ctypes.c_void_p),
        ("part_stride", ctypes.c_size_t),
        ("chunk_stride", ctypes.c_size_t),
        ("n_parts", ctypes.c_size_t),
        ("chunk_len", ctypes.c_size_t),
    ]


def _sig(name, argtypes, restype=ctypes.c_int):
    fn = getattr(_lib, name)
    fn.argtypes = argtypes
    fn.restype = restype
    return fn


_sig("cec_abi_version", [])
# the include/chunky_ec.h this binding mirrors (2: CEC_PRESENT_VERIFIED = 0x80)
ABI_VERSION = 3
if _lib.cec_abi_version() != ABI_VERSION:
    raise ImportError(f"chunky_ec: {LIB_PATH} has ABI {_lib.cec_abi_version()}, this binding "
                      f"needs {ABI_VERSION}; rebuild with `make -C chunky-bits_amd/csrc`")
if not hasattr(_lib, "cec_build_id"):
    raise ImportError(f"chunky_ec: {LIB_PATH} predates cec_build_id; rebuild with "
                      "`make -C chunky-bits_amd/csrc`")
_sig("cec_build_id", [], ctypes.c_char_p)


def _shipped_source_hash() -> Optional[str]:
    """Hash of the library sources shipped beside this package (csrc/source_hash.py), or None
    when they are not (an installed copy)."""
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    script = os.path.join(csrc, "source_hash.py")
    if not os.path.exists(script):
        return None
    import importlib.util
    spec = importlib.util.spec_from_file_location("_cec_source_hash", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.source_hash()


BUILD_ID = _lib.cec_build_id().decode()
SOURCE_HASH = _shipped_source_hash()
# Build provenance: a library built from other sources than the ones shipped with it (a stale
# build, or objects carried over from another tree) is refused, so what runs on a GPU box is what
# the tree says.  CEC_ALLOW_STALE_BUILD=1 lets a developer load it anyway.
BUILD_MATCHES_SOURCE = SOURCE_HASH is None or SOURCE_HASH == BUILD_ID
if not BUILD_MATCHES_SOURCE and os.environ.get("CEC_ALLOW_STALE_BUILD") != "1":
    raise ImportError(f"chunky_ec: {LIB_PATH} was built from sources {BUILD_ID}, the shipped "
                      f"sources hash to {SOURCE_HASH}; rebuild with `make -C chunky-bits_amd/csrc`")
_sig("cec_status_name", [ctypes.c_int], ctypes.c_char_p)
_sig("cec_last_error", [], ctypes.c_char_p)
_sig("cec_device_count", [])
_sig("cec_build_info", [], ctypes.c_char_p)
_sig("cec_reload_knobs", [], None)
_sig("cec_release_cached", [ctypes.c_int], ctypes.c_size_t)
_sig("cec_codec_cached_patterns", [_vp], ctypes.c_size_t)
_sig("cec_codec_new", [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp)])
_sig("cec_codec_free", [_vp], None)
_sig("cec_codec_data_shards", [_vp], ctypes.c_size_t)
_sig("cec_codec_parity_shards", [_vp], ctypes.c_size_t)
_sig("cec_codec_total_shards", [_vp], ctypes.c_size_t)
_sig("cec_codec_matrix", [_vp, _u8p, ctypes.c_size_t])
_sig("cec_encode_sep", [_vp, ctypes.POINTER(_u8p), _szp, ctypes.c_size_t,
                        ctypes.POINTER(_u8p), _szp, ctypes.c_size_t])
_sig("cec_reconstruct", [_vp, ctypes.POINTER(_u8p), _szp, _u8p, ctypes.c_size_t])
_sig("cec_reconstruct_data", [_vp, ctypes.POINTER(_u8p), _szp, _u8p, ctypes.c_size_t])
_sig("cec_sha256", [_u8p, ctypes.c_size_t, _u8p])
_sig("cec_sha256_many", [ctypes.POINTER(_u8p), _szp, ctypes.c_size_t, _u8p])
_sig("cec_part_encode", [_vp, _u8p, ctypes.c_size_t, _u8p, _u8p, _szp])
_sig("cec_parts_encode", [_vp, ctypes.POINTER(_u8p), _szp, ctypes.c_size_t, ctypes.POINTER(_u8p),
                          _u8p, _szp])
_sig("cec_ragged_stride", [ctypes.c_size_t], ctypes.c_size_t)
_sig("cec_ragged_layout", [ctypes.c_size_t, _szp, ctypes.c_size_t, _szp, _szp])
_sig("cec_encode_hash_ragged", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _vp, _vp])
_sig("cec_split_layout", [ctypes.c_size_t, ctypes.c_size_t, _szp, ctypes.c_size_t, _szp, _szp,
                          _szp, _szp])
_sig("cec_encode_hash_split", [_vp, _vp, _szp, _vp, _szp, _szp, ctypes.c_size_t, _vp, _vp])
_sig("cec_parts_pipeline_new", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                ctypes.POINTER(_vp)])
_sig("cec_parts_pipeline_free", [_vp], None)
_sig("cec_parts_pipeline_depth", [_vp], ctypes.c_size_t)
_sig("cec_parts_pipeline_acquire", [_vp, _szp, ctypes.POINTER(_u8p)])
_sig("cec_parts_pipeline_submit", [_vp, ctypes.c_size_t, _szp, ctypes.c_size_t])
_sig("cec_parts_pipeline_submit_from", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), _szp,
                                        ctypes.c_size_t, _szp])
_sig("cec_parts_pipeline_wait", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), ctypes.POINTER(_u8p),
                                 _szp])
_sig("cec_parts_pipeline_query", [_vp, ctypes.c_size_t])
_sig("cec_parts_pipeline_drain", [_vp])
_u32p = ctypes.POINTER(ctypes.c_uint32)
_sig("cec_sha_midstate_bytes", [], ctypes.c_size_t)
_sig("cec_encode_hash_segments", [_vp, _vp, _szp, _vp, _szp, _szp, ctypes.c_size_t, _u32p, _u8p,
                                  _vp, ctypes.c_size_t, _vp, _vp])
_sig("cec_segment_pipeline_new", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                  ctypes.c_size_t, ctypes.POINTER(_vp)])
_sig("cec_segment_pipeline_free", [_vp], None)
_sig("cec_segment_pipeline_depth", [_vp], ctypes.c_size_t)
_sig("cec_segment_pipeline_acquire", [_vp, _szp])
_sig("cec_segment_pipeline_submit_from", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), _szp, _szp,
                                          _szp, _u32p, ctypes.c_size_t, _szp])
_sig("cec_segment_pipeline_wait", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p),
                                   ctypes.POINTER(_u8p), _szp])
_sig("cec_segment_pipeline_query", [_vp, ctypes.c_size_t])
_sig("cec_segment_pipeline_drain", [_vp])
_sig("cec_segment_pipeline_open_count", [_vp], ctypes.c_size_t)
_sig("cec_segment_pipeline_abandon", [_vp, ctypes.c_uint32])
_sig("cec_verify_segments", [_vp, _szp, _szp, ctypes.c_size_t, _u32p, _u8p, _vp, ctypes.c_size_t,
                             _vp, _vp, _vp])
_sig("cec_scrub_pipeline_new", [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                ctypes.POINTER(_vp)])
_sig("cec_scrub_pipeline_free", [_vp], None)
_sig("cec_scrub_pipeline_depth", [_vp], ctypes.c_size_t)
_sig("cec_scrub_pipeline_acquire", [_vp, _szp])
_sig("cec_scrub_pipeline_submit_from", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), _szp, _szp,
                                        _szp, _u32p, _u8p, ctypes.c_size_t])
_sig("cec_scrub_pipeline_wait", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), _szp])
_sig("cec_scrub_pipeline_query", [_vp, ctypes.c_size_t])
_sig("cec_scrub_pipeline_drain", [_vp])
_sig("cec_scrub_pipeline_open_count", [_vp], ctypes.c_size_t)
_sig("cec_scrub_pipeline_abandon", [_vp, ctypes.c_uint32])
_sig("cec_reconstruct_ragged", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _u8p, ctypes.c_int, _vp])
_sig("cec_read_ragged", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _u8p, _vp, _u8p,
                         ctypes.POINTER(ctypes.c_int), _vp])
_sig("cec_resilver_ragged", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _u8p, _vp, _u8p,
                             ctypes.POINTER(ctypes.c_int), _vp])
_sig("cec_read_ragged_async", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _u8p, _vp, _u8p,
                               ctypes.POINTER(ctypes.c_int), _vp])
_sig("cec_resilver_ragged_async", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _u8p, _vp, _u8p,
                                   ctypes.POINTER(ctypes.c_int), _vp])
_sig("cec_read_ragged_packed_async", [_vp, _vp, _szp, _szp, ctypes.c_size_t, _u8p, _vp, ctypes.c_int,
                                      _u8p, ctypes.POINTER(ctypes.c_int), _vp, ctypes.c_size_t,
                                      _szp, _vp])
_sig("cec_parts_reader_new", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                              ctypes.POINTER(_vp)])
_sig("cec_parts_reader_free", [_vp], None)
_sig("cec_parts_reader_depth", [_vp], ctypes.c_size_t)
_sig("cec_parts_reader_acquire", [_vp, _szp, ctypes.POINTER(_u8p)])
_sig("cec_parts_reader_submit", [_vp, ctypes.c_size_t, _szp, ctypes.c_size_t, _u8p, _u8p])
_sig("cec_parts_reader_submit_from", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), _szp,
                                      ctypes.c_size_t, _u8p, _u8p])
_sig("cec_parts_reader_wait", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p),
                               ctypes.POINTER(ctypes.POINTER(ctypes.c_int)), ctypes.POINTER(_u8p),
                               ctypes.POINTER(_szp), _szp])
_sig("cec_parts_reader_scatter", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p)])
_sig("cec_parts_reader_query", [_vp, ctypes.c_size_t])
_sig("cec_parts_reader_drain", [_vp])
_sig("cec_parts_reader_stats", [_vp, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
     None)
_sig("cec_ragged_read_stats", [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
     None)
_sig("cec_parts_read", [_vp, ctypes.POINTER(_u8p), _szp, ctypes.c_size_t, _u8p, _u8p, ctypes.c_int,
                        _u8p, ctypes.POINTER(ctypes.c_int)])
_sig("cec_part_read", [_vp, ctypes.POINTER(_u8p), ctypes.c_size_t, _u8p, _u8p, ctypes.c_int, _u8p])
_sig("cec_coalesce_detail", [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                             ctypes.POINTER(ctypes.c_uint64)], None)
_sig("cec_verify_ragged", [ctypes.c_size_t, _vp, _szp, _szp, ctypes.c_size_t, _u8p, _vp, _u8p, _vp])
_sig("cec_parts_verify", [ctypes.POINTER(_u8p), _szp, ctypes.c_size_t, _u8p, _u8p])
_sig("cec_coalesce_stats", [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
     None)
_sig("cec_ragged_stats", [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)],
     None)
_sig("cec_encode_batch", [_vp, ctypes.POINTER(PartBatchStruct), _vp])
_sig("cec_encode_hash_batch", [_vp, ctypes.POINTER(PartBatchStruct), _vp, _vp])
_sig("cec_sha256_batch", [ctypes.POINTER(PartBatchStruct), ctypes.c_size_t, ctypes.c_size_t,
                          _vp, _vp])
_sig("cec_reconstruct_batch", [_vp, ctypes.POINTER(PartBatchStruct), _u8p, ctypes.c_int, _vp])
_sig("cec_fill_synthetic", [ctypes.POINTER(PartBatchStruct), ctypes.c_size_t, ctypes.c_uint64,
                            _vp])
_sig("cec_verify_batch", [ctypes.POINTER(PartBatchStruct), ctypes.c_size_t, ctypes.c_size_t,
                          _vp, _vp, _vp, _vp])
_sig("cec_read_batch", [_vp, ctypes.POINTER(PartBatchStruct), _u8p, _vp, _u8p,
                        ctypes.POINTER(ctypes.c_int), _vp])
_sig("cec_resilver_batch", [_vp, ctypes.POINTER(PartBatchStruct), _u8p, _vp, _u8p,
                            ctypes.POINTER(ctypes.c_int), _vp])
_sig("cec_pipeline_new", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                          ctypes.POINTER(_vp)])
_sig("cec_pipeline_free", [_vp], None)
_sig("cec_pipeline_depth", [_vp], ctypes.c_size_t)
_sig("cec_pipeline_acquire", [_vp, _szp, ctypes.POINTER(_u8p)])
_sig("cec_pipeline_submit", [_vp, ctypes.c_size_t, ctypes.c_size_t])
_sig("cec_pipeline_wait", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), ctypes.POINTER(_u8p),
                           _szp])
_sig("cec_pipeline_drain", [_vp])
_sig("cec_pipeline_query", [_vp, ctypes.c_size_t])
_sig("cec_read_pipeline_query", [_vp, ctypes.c_size_t])
_sig("cec_pipeline_last_error", [], ctypes.c_char_p)
_sig("cec_read_pipeline_new", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                               ctypes.POINTER(_vp)])
_sig("cec_read_pipeline_free", [_vp], None)
_sig("cec_read_pipeline_depth", [_vp], ctypes.c_size_t)
_sig("cec_read_pipeline_acquire", [_vp, _szp, ctypes.POINTER(_u8p), ctypes.POINTER(_u8p),
                                   ctypes.POINTER(_u8p)])
_sig("cec_read_pipeline_submit", [_vp, ctypes.c_size_t, ctypes.c_size_t])
_sig("cec_read_pipeline_acquire_idle", [_vp, _szp, ctypes.POINTER(_u8p), ctypes.POINTER(_u8p),
                                        ctypes.POINTER(_u8p)])
_sig("cec_read_pipeline_wait", [_vp, ctypes.c_size_t, ctypes.POINTER(_u8p), ctypes.POINTER(_u8p),
                                ctypes.POINTER(ctypes.POINTER(ctypes.c_int)), _szp])
_sig("cec_read_pipeline_drain", [_vp])
_sig("cec_read_pipeline_new_ex", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                  ctypes.c_uint, ctypes.POINTER(_vp)])
_sig("cec_read_pipeline_data_chunks", [_vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                                       ctypes.c_size_t])
_sig("cec_synth_byte", [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64],
     ctypes.c_uint8)
_sig("cec_current_device", [ctypes.POINTER(ctypes.c_int)])
_sig("cec_set_device", [ctypes.c_int])
_sig("cec_device_numa_node", [ctypes.c_int])
_sig("cec_host_alloc", [ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_vp)])
_sig("cec_host_free", [_vp], None)
_sig("cec_host_is_pinned", [_vp, ctypes.c_size_t])
_sig("cec_host_numa_node", [_vp])
_sig("cec_bind_thread_to_device_node", [ctypes.c_int])
_sig("cec_pipeline_new_ex", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint,
                             ctypes.POINTER(_vp)])
_sig("cec_pipeline_submit_from", [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp, _vp])
_sig("cec_read_pipeline_submit_from", [_vp, ctypes.c_size_t, _vp, _vp, _vp, ctypes.c_size_t, _vp])
_sig("cec_read_pipeline_submit_packed", [_vp, ctypes.c_size_t, _vp, _vp, _vp, ctypes.c_size_t, _vp])
_sig("cec_read_pipeline_carry_ids", [_vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32),
                                     ctypes.c_size_t])
_sig("cec_read_pipeline_submit_carried", [_vp, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_int32)])
_sig("cec_read_pipeline_carry_release", [_vp, ctypes.c_int32])
_sig("cec_read_pipeline_carry_held", [_vp], ctypes.c_size_t)


class ReadSubmitStruct(ctypes.Structure):
    """cec_read_submit (include/chunky_ec.h)."""
    _fields_ = [("chunks", ctypes.c_void_p), ("present", ctypes.c_void_p),
                ("expected", ctypes.c_void_p), ("n_parts", ctypes.c_size_t),
                ("data_out", ctypes.c_void_p), ("carry_ids", ctypes.c_void_p),
                ("flags", ctypes.c_uint)]


class MultiStatsStruct(ctypes.Structure):
    """cec_multi_stats (include/chunky_ec.h)."""
    _fields_ = [("device", ctypes.c_int), ("numa_node", ctypes.c_int),
                ("parts", ctypes.c_uint64), ("pipelines_made", ctypes.c_uint64),
                ("chunks_uploaded", ctypes.c_uint64), ("chunks_carried", ctypes.c_uint64),
                ("carry_held", ctypes.c_uint64)]


_sig("cec_read_pipeline_submit_ex", [_vp, ctypes.c_size_t, ctypes.POINTER(ReadSubmitStruct)])
_sig("cec_pipelines_made", [], ctypes.c_uint64)
_sig("cec_multi_new_ex", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                          ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.c_uint,
                          ctypes.POINTER(_vp)])
_sig("cec_multi_read_carry", [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp,
                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p),
                              ctypes.c_uint, ctypes.POINTER(ctypes.c_int32),
                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)])
_sig("cec_multi_carry_release", [_vp, ctypes.c_int32])
_sig("cec_multi_shard_stats", [_vp, ctypes.c_size_t, ctypes.POINTER(MultiStatsStruct)])
_sig("cec_multi_new", [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                       ctypes.POINTER(ctypes.c_int), ctypes.c_size_t, ctypes.POINTER(_vp)])
_sig("cec_multi_free", [_vp], None)
_sig("cec_multi_shards", [_vp], ctypes.c_size_t)
_sig("cec_multi_shard_info", [_vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)])
_sig("cec_multi_encode_hash", [_vp, _vp, ctypes.c_size_t, _vp, _vp,
                               ctypes.POINTER(ctypes.c_uint64)])
_sig("cec_multi_read", [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp,
                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint,
                        ctypes.POINTER(ctypes.c_uint64)])
_sig("cec_multi_resilver", [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp,
                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p),
                            ctypes.POINTER(ctypes.c_uint64)])
_sig("cec_multi_verify", [_vp, _vp, _vp, _vp, ctypes.c_size_t, _vp,
                          ctypes.POINTER(ctypes.c_uint64)])
_sig("cec_multi_wait", [_vp, ctypes.c_uint64])
_sig("cec_multi_query", [_vp, ctypes.c_uint64])
_sig("cec_multi_last_error", [], ctypes.c_char_p)

# Status codes (include/chunky_ec.h).
OK = 0
TOO_FEW_SHARDS = 1
TOO_MANY_SHARDS = 2
TOO_FEW_DATA_SHARDS = 3
TOO_MANY_DATA_SHARDS = 4
TOO_FEW_PARITY_SHARDS = 5
TOO_MANY_PARITY_SHARDS = 6
TOO_FEW_BUFFER_SHARDS = 7
TOO_MANY_BUFFER_SHARDS = 8
INCORRECT_SHARD_SIZE = 9
TOO_FEW_SHARDS_PRESENT = 10
EMPTY_SHARD = 11
INVALID_SHARD_FLAGS = 12
INVALID_INDEX = 13
ERR_INVALID_ARGUMENT = 101
ERR_HIP = 102
ERR_NO_DEVICE = 103
ERR_OUT_OF_MEMORY = 104


class Error(Exception):
    """reed_solomon_erasure::Error (codes 1..13) or an engine error (>= 100)."""

    def __init__(self, code: int):
        self.code = code
        self.name = _lib.cec_status_name(code).decode()
        detail = _lib.cec_last_error().decode() if code >= 100 else ""
        super().__init__(f"{self.name}" + (f": {detail}" if detail else ""))


def _check(code: int) -> None:
    if code != OK:
        raise Error(code)


def abi_version() -> int:
    return _lib.cec_abi_version()


def device_count() -> int:
    return _lib.cec_device_count()


def build_info() -> str:
    return _lib.cec_build_info().decode()


def reload_knobs() -> None:
    """Re-read the CEC_* environment knobs (test-only: the library reads them once per
    process, cec_reload_knobs)."""
    _lib.cec_reload_knobs()


def release_cached(device: int = -1) -> int:
    """Free the idle per-call staging on `device` (every device when < 0); returns the device
    bytes released (cec_release_cached)."""
    return _lib.cec_release_cached(device)


def status_name(code: int) -> str:
    return _lib.cec_status_name(code).decode()


def _buf_ptr(b, keep: list) -> "ctypes._Pointer":
    """Pointer to the first byte of a bytes-like object (valid while `b` / `keep` live)."""
    if isinstance(b, bytes):
        return ctypes.cast(ctypes.c_char_p(b), _u8p)
    mv = memoryview(b)
    if mv.nbytes == 0:
        return _u8p()
    if mv.readonly or not mv.c_contiguous:
        tmp = mv.tobytes()
        keep.append(tmp)
        return ctypes.cast(ctypes.c_char_p(tmp), _u8p)
    return ctypes.cast((ctypes.c_char * mv.nbytes).from_buffer(mv.cast("B")), _u8p)


def _nbytes(b) -> int:
    return memoryview(b).nbytes


class ReedSolomon:
    """reed_solomon_erasure::ReedSolomon<galois_8::Field> backed by the gfx950 kernels."""

    def __init__(self, data_shards: int, parity_shards: int):
        h = _vp()
        _check(_lib.cec_codec_new(data_shards, parity_shards, ctypes.byref(h)))
        self._h = h

    def __del__(self, _free=_lib.cec_codec_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def data_shard_count(self) -> int:
        return _lib.cec_codec_data_shards(self._h)

    def parity_shard_count(self) -> int:
        return _lib.cec_codec_parity_shards(self._h)

    def total_shard_count(self) -> int:
        return _lib.cec_codec_total_shards(self._h)

    def cached_patterns(self) -> int:
        """Decode matrices cached in the codec (bounded LRU)."""
        return _lib.cec_codec_cached_patterns(self._h)

    def matrix(self) -> List[List[int]]:
        d, t = self.data_shard_count(), self.total_shard_count()
        out = (ctypes.c_uint8 * (d * t))()
        _check(_lib.cec_codec_matrix(self._h, out, d * t))
        return [list(out[r * d:(r + 1) * d]) for r in range(t)]

    def encode_sep(self, data: Sequence, parity: MutableSequence) -> None:
        """Overwrites each writable parity buffer with the parity of `data` (crate semantics)."""
        keep: list = []
        dp = (_u8p * max(len(data), 1))(*[_buf_ptr(x, keep) for x in data])
        dl = (ctypes.c_size_t * max(len(data), 1))(*[_nbytes(x) for x in data])
        pp = (_u8p * max(len(parity), 1))(*[_buf_ptr(x, keep) for x in parity])
        pl = (ctypes.c_size_t * max(len(parity), 1))(*[_nbytes(x) for x in parity])
        _check(_lib.cec_encode_sep(self._h, dp, dl, len(data), pp, pl, len(parity)))

    def _reconstruct(self, shards: MutableSequence[Optional[bytearray]], data_only: bool):
        n = len(shards)
        present = (ctypes.c_uint8 * max(n, 1))(*[0 if s is None else 1 for s in shards])
        slen = next((_nbytes(s) for s in shards if s is not None and _nbytes(s) > 0), 0)
        bufs = []
        for s in shards:
            bufs.append(bytearray(slen) if s is None else s)
        keep: list = []
        ptrs = (_u8p * max(n, 1))(*[_buf_ptr(b, keep) for b in bufs])
        lens = (ctypes.c_size_t * max(n, 1))(*[_nbytes(b) for b in bufs])
        code = (_lib.cec_reconstruct_data if data_only else _lib.cec_reconstruct)(
            self._h, ptrs, lens, present, n)
        _check(code)
        for i in range(n):
            if shards[i] is None and present[i]:
                shards[i] = bufs[i]

    def reconstruct(self, shards: MutableSequence[Optional[bytearray]]) -> None:
        """Fills every None slot (data and parity), like ReedSolomon::reconstruct."""
        self._reconstruct(shards, False)

    def reconstruct_data(self, shards: MutableSequence[Optional[bytearray]]) -> None:
        """Fills missing data slots only, like ReedSolomon::reconstruct_data."""
        self._reconstruct(shards, True)


class Sha256Hash:
    """src/file/hash/sha256.rs: Sha256Hash([u8; 32]) with hex display."""

    __slots__ = ("digest",)

    def __init__(self, digest: bytes):
        assert len(digest) == 32
        self.digest = bytes(digest)

    @classmethod
    def from_buf(cls, buf) -> "Sha256Hash":
        out = (ctypes.c_uint8 * 32)()
        keep: list = []
        _check(_lib.cec_sha256(_buf_ptr(buf, keep), _nbytes(buf), out))
        return cls(bytes(out))

    @classmethod
    def from_bufs(cls, bufs: Sequence) -> List["Sha256Hash"]:
        """Batched DataHasher::from_buf over many buffers (one launch)."""
        n = len(bufs)
        if n == 0:
            return []
        out = (ctypes.c_uint8 * (32 * n))()
        keep: list = []
        ptrs = (_u8p * n)(*[_buf_ptr(b, keep) for b in bufs])
        lens = (ctypes.c_size_t * n)(*[_nbytes(b) for b in bufs])
        _check(_lib.cec_sha256_many(ptrs, lens, n, out))
        raw = bytes(out)
        return [cls(raw[32 * i:32 * (i + 1)]) for i in range(n)]

    @classmethod
    def from_str(cls, s: str) -> "Sha256Hash":
        return cls(bytes.fromhex(s))

    def verify(self, buf) -> bool:
        return Sha256Hash.from_buf(buf) == self

    def __eq__(self, other) -> bool:
        return isinstance(other, Sha256Hash) and other.digest == self.digest

    def __hash__(self) -> int:
        return hash(self.digest)

    def __str__(self) -> str:
        return self.digest.hex()

    __repr__ = __str__


class AnyHash:
    """src/file/hash/any.rs: AnyHash::Sha256, displayed as ``sha256-<hex>``."""

    def __init__(self, h: Sha256Hash):
        self.sha256 = h

    def __str__(self) -> str:
        return f"sha256-{self.sha256}"

    @classmethod
    def from_str(cls, s: str) -> "AnyHash":
        kind, _, hexs = s.partition("-")
        if not _:
            raise ValueError("Invalid hash format")
        if kind != "sha256":
            raise ValueError(f"Unknown Hash Format: {kind}")
        return cls(Sha256Hash.from_str(hexs))

    def verify(self, buf) -> bool:
        return self.sha256.verify(buf)

    def __eq__(self, other) -> bool:
        return isinstance(other, AnyHash) and other.sha256 == self.sha256


@dataclass
class EncodedPart:
    """Compute result of FilePart::write_with_encoder: chunksize, parity chunks, digests."""

    chunksize: int
    parity: List[bytes]
    hashes: List[Sha256Hash]  # d data then p parity, in order


def part_encode(codec: ReedSolomon, data_buf, length: int) -> EncodedPart:
    """FilePart::write_with_encoder's compute (file_part.rs:150-185) for one part."""
    d, p = codec.data_shard_count(), codec.parity_shard_count()
    if length > _nbytes(data_buf):  # file_part.rs:150 asserts length <= data_buf.len()
        raise ValueError(f"length {length} > data_buf length {_nbytes(data_buf)}")
    L = (length + d - 1) // d if length else 0
    buf = bytearray(d * L)
    src = memoryview(data_buf)[:length]
    buf[:length] = src
    par = (ctypes.c_uint8 * max(p * L, 1))()
    dig = (ctypes.c_uint8 * (32 * (d + p)))()
    cs = ctypes.c_size_t(0)
    keep: list = []
    _check(_lib.cec_part_encode(codec.handle, _buf_ptr(buf, keep) if L else _u8p(), length, par,
                                dig, ctypes.byref(cs)))
    raw = bytes(par)
    draw = bytes(dig)
    return EncodedPart(
        chunksize=cs.value,
        parity=[raw[i * L:(i + 1) * L] for i in range(p)],
        hashes=[Sha256Hash(draw[32 * i:32 * (i + 1)]) for i in range(d + p)],
    )


def parts_encode(codec: ReedSolomon, bufs: Sequence) -> List[EncodedPart]:
    """:func:`part_encode` for parts of unrelated lengths in ONE engine call
    (``cec_parts_encode``): part k is the whole of ``bufs[k]``, read as it is -- the engine pads
    to ``d * chunksize`` with zeros in its own staging.  Results equal ``part_encode(codec,
    bufs[k], len(bufs[k]))`` part by part."""
    d, p = codec.data_shard_count(), codec.parity_shard_count()
    n = len(bufs)
    if n == 0:
        return []
    keep: list = []
    lens = [_nbytes(b) for b in bufs]
    Ls = [(ln + d - 1) // d for ln in lens]
    ptrs = (_u8p * n)(*[_buf_ptr(b, keep) for b in bufs])
    c_lens = (ctypes.c_size_t * n)(*lens)
    pars = [(ctypes.c_uint8 * max(p * L, 1))() for L in Ls]
    par_ptrs = (_u8p * n)(*[ctypes.cast(x, _u8p) for x in pars])
    dig = (ctypes.c_uint8 * (32 * (d + p) * n))()
    cs = (ctypes.c_size_t * n)()
    _check(_lib.cec_parts_encode(codec.handle, ptrs, c_lens, n, par_ptrs, dig, cs))
    draw = bytes(dig)
    out = []
    for k in range(n):
        raw, L, d0 = bytes(pars[k]), Ls[k], 32 * (d + p) * k
        out.append(EncodedPart(
            chunksize=cs[k],
            parity=[raw[i * L:(i + 1) * L] for i in range(p)],
            hashes=[Sha256Hash(draw[d0 + 32 * i:d0 + 32 * (i + 1)]) for i in range(d + p)]))
    return out


# ---------------------------------------------------------------------------------------------
# Device-resident batches
# ---------------------------------------------------------------------------------------------


@dataclass
class PartBatch:
    """Part k's chunk i at base + k*part_stride + i*chunk_stride, chunk_len bytes (device)."""

    base: int
    part_stride: int
    chunk_stride: int
    n_parts: int
    chunk_len: int

    def struct(self) -> PartBatchStruct:
        return PartBatchStruct(self.base, self.part_stride, self.chunk_stride, self.n_parts,
                               self.chunk_len)

    @classmethod
    def from_tensor(cls, t, chunk_len: Optional[int] = None) -> "PartBatch":
        """t: contiguous uint8 device tensor shaped (n_parts, n_chunks, chunk_stride)."""
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.is_contiguous()
        n_parts, n_chunks, cstride = t.shape
        return cls(t.data_ptr(), n_chunks * cstride, cstride, n_parts,
                   cstride if chunk_len is None else chunk_len)


def _stream_ptr(stream) -> int:
    if stream is None:
        if torch is not None and torch.cuda.is_available():
            return torch.cuda.current_stream().cuda_stream
        return 0
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream
    return int(stream)


def encode_batch(codec: ReedSolomon, batch: PartBatch, stream=None) -> None:
    s = batch.struct()
    _check(_lib.cec_encode_batch(codec.handle, ctypes.byref(s), _stream_ptr(stream)))


def encode_hash_batch(codec: ReedSolomon, batch: PartBatch, digests_ptr: int,
                      stream=None) -> None:
    s = batch.struct()
    _check(_lib.cec_encode_hash_batch(codec.handle, ctypes.byref(s), digests_ptr,
                                      _stream_ptr(stream)))


def ragged_stride(chunk_len: int) -> int:
    """Chunk stride of a ragged batch: ``chunk_len`` rounded up to 16."""
    return _lib.cec_ragged_stride(chunk_len)


def ragged_layout(total_shards: int, chunk_lens: Sequence[int]):
    """The packed ragged layout of parts with these chunk lengths: ``(part_offsets,
    total_bytes)``; part k's chunk i is at ``part_offsets[k] + i * ragged_stride(chunk_lens[k])``."""
    n = len(chunk_lens)
    lens = (ctypes.c_size_t * max(n, 1))(*chunk_lens)
    offs = (ctypes.c_size_t * max(n, 1))()
    total = ctypes.c_size_t(0)
    _check(_lib.cec_ragged_layout(total_shards, lens, n, offs, ctypes.byref(total)))
    return list(offs[:n]), total.value


def encode_hash_ragged(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                       chunk_lens: Sequence[int], digests_ptr: int, stream=None) -> None:
    """encode_sep + SHA-256 of all d+p chunks of parts of different chunk lengths, one launch
    sequence (``cec_encode_hash_ragged``): device memory at ``base_ptr`` in the layout of
    :func:`ragged_layout`, digests ``[n][d+p][32]`` at ``digests_ptr``."""
    n = len(chunk_lens)
    if len(part_offsets) != n:
        raise ValueError("part_offsets and chunk_lens differ in length")
    offs = (ctypes.c_size_t * max(n, 1))(*part_offsets)
    lens = (ctypes.c_size_t * max(n, 1))(*chunk_lens)
    _check(_lib.cec_encode_hash_ragged(codec.handle, base_ptr, offs, lens, n, digests_ptr,
                                       _stream_ptr(stream)))


def split_layout(data_shards: int, parity_shards: int, chunk_lens: Sequence[int]):
    """The packed split ragged layout (``cec_split_layout``): ``(data_offsets, parity_offsets,
    data_bytes, parity_bytes)``.  Part k's data chunk j is at ``data_offsets[k] + j * stride`` of
    the data region, its parity chunk i at ``parity_offsets[k] + i * stride`` of the parity
    region, ``stride = ragged_stride(chunk_lens[k])``."""
    n = len(chunk_lens)
    lens = (ctypes.c_size_t * max(n, 1))(*chunk_lens)
    doffs = (ctypes.c_size_t * max(n, 1))()
    poffs = (ctypes.c_size_t * max(n, 1))()
    db, pb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(_lib.cec_split_layout(data_shards, parity_shards, lens, n, doffs, poffs,
                                 ctypes.byref(db), ctypes.byref(pb)))
    return list(doffs[:n]), list(poffs[:n]), db.value, pb.value


def encode_hash_split(codec: ReedSolomon, data_ptr: int, data_offsets: Sequence[int],
                      parity_ptr: int, parity_offsets: Sequence[int], chunk_lens: Sequence[int],
                      digests_ptr: int, stream=None) -> None:
    """:func:`encode_hash_ragged` over the split layout (``cec_encode_hash_split``): the data
    chunks are read from the device region at ``data_ptr``, the parity chunks written to the one
    at ``parity_ptr``, digests ``[n][d+p][32]`` at ``digests_ptr``."""
    n = len(chunk_lens)
    if len(data_offsets) != n or len(parity_offsets) != n:
        raise ValueError("offsets and chunk_lens differ in length")
    doffs = (ctypes.c_size_t * max(n, 1))(*data_offsets)
    poffs = (ctypes.c_size_t * max(n, 1))(*parity_offsets)
    lens = (ctypes.c_size_t * max(n, 1))(*chunk_lens)
    _check(_lib.cec_encode_hash_split(codec.handle, data_ptr, doffs, parity_ptr, poffs, lens, n,
                                      digests_ptr, _stream_ptr(stream)))


SEG_FIRST, SEG_LAST = 1, 2
MIDSTATE_BYTES = _lib.cec_sha_midstate_bytes()


def encode_hash_segments(codec: ReedSolomon, data_ptr: int, data_offsets: Sequence[int],
                         parity_ptr: int, parity_offsets: Sequence[int], seg_lens: Sequence[int],
                         state_slots: Sequence[int], flags: Sequence[int], midstates_ptr: int,
                         n_state_slots: int, digests_ptr: int, stream=None) -> None:
    """:func:`encode_hash_split` over column segments (``cec_encode_hash_segments``): entry k is
    ``seg_lens[k]`` columns of one part in the split layout over ``seg_lens``.  Its parity pieces
    are written, and the SHA-256 chain of each of its d + p chunks starts (``SEG_FIRST``), resumes
    from the records of state slot ``state_slots[k]`` in the device pool at ``midstates_ptr``
    (``n_state_slots * (d + p)`` records of ``MIDSTATE_BYTES``), and with ``SEG_LAST`` ends: only
    then is the entry's digest row written.  Successive segments of a part go in order on one
    stream."""
    n = len(seg_lens)
    arr = lambda v: (ctypes.c_size_t * max(n, 1))(*v)  # noqa: E731
    _check(_lib.cec_encode_hash_segments(
        codec.handle, data_ptr, arr(data_offsets), parity_ptr, arr(parity_offsets), arr(seg_lens),
        n, (ctypes.c_uint32 * max(n, 1))(*state_slots), (ctypes.c_uint8 * max(n, 1))(*flags),
        midstates_ptr, n_state_slots, digests_ptr, _stream_ptr(stream)))


def verify_segments(base_ptr: int, offsets: Sequence[int], seg_lens: Sequence[int],
                    state_slots: Sequence[int], flags: Sequence[int], midstates_ptr: int,
                    n_state_slots: int, expected_ptr: int, ok_ptr: int, stream=None) -> None:
    """:func:`verify_ragged` of single copies over segments (``cec_verify_segments``), queued on
    the stream with no wait: entry k is ``seg_lens[k]`` bytes at ``base_ptr + offsets[k]``, the
    layout of :func:`ragged_layout` with one chunk per part.  The SHA-256 chain of its copy starts
    (``SEG_FIRST``), resumes from the record of state slot ``state_slots[k]`` in the device pool at
    ``midstates_ptr`` (``n_state_slots`` records of ``MIDSTATE_BYTES``), and with ``SEG_LAST``
    ends: only then is row k of the device rows ``[n][32]`` at ``expected_ptr`` read and byte k of
    the device bytes at ``ok_ptr`` written, 1 if the whole copy has that digest, else 0.
    Successive segments of a copy go in order on one stream."""
    n = len(seg_lens)
    arr = lambda v: (ctypes.c_size_t * max(n, 1))(*v)  # noqa: E731
    _check(_lib.cec_verify_segments(
        base_ptr, arr(offsets), arr(seg_lens), n, (ctypes.c_uint32 * max(n, 1))(*state_slots),
        (ctypes.c_uint8 * max(n, 1))(*flags), midstates_ptr, n_state_slots, expected_ptr, ok_ptr,
        _stream_ptr(stream)))


def sha256_batch(batch: PartBatch, first_chunk: int, n_chunks: int, digests_ptr: int,
                 stream=None) -> None:
    s = batch.struct()
    _check(_lib.cec_sha256_batch(ctypes.byref(s), first_chunk, n_chunks, digests_ptr,
                                 _stream_ptr(stream)))


def reconstruct_batch(codec: ReedSolomon, batch: PartBatch, present, data_only: bool,
                      stream=None) -> None:
    """present: host bytes-like of n_parts*(d+p) flags (part-major)."""
    s = batch.struct()
    pres = bytes(present)
    _check(_lib.cec_reconstruct_batch(codec.handle, ctypes.byref(s),
                                      ctypes.cast(ctypes.c_char_p(pres), _u8p),
                                      1 if data_only else 0, _stream_ptr(stream)))


def verify_batch(batch: PartBatch, first_chunk: int, n_chunks: int, expected_ptr: int,
                 ok_ptr: int, present_ptr: int = 0, stream=None) -> None:
    """DataVerifier::verify over a batch (device pointers; present_ptr 0 = all present)."""
    s = batch.struct()
    _check(_lib.cec_verify_batch(ctypes.byref(s), first_chunk, n_chunks, present_ptr or None,
                                 expected_ptr, ok_ptr, _stream_ptr(stream)))


def _verify_rebuild(fn, codec, batch, present, expected_ptr, stream):
    t = codec.total_shard_count()
    n = batch.n_parts * t
    pres = bytes(present)
    assert len(pres) == n
    verified = (ctypes.c_uint8 * max(n, 1))()
    status = (ctypes.c_int * max(batch.n_parts, 1))()
    s = batch.struct()
    _check(fn(codec.handle, ctypes.byref(s), ctypes.cast(ctypes.c_char_p(pres), _u8p),
              expected_ptr, verified, status, _stream_ptr(stream)))
    return bytes(verified)[:n], list(status)[:batch.n_parts]


def read_batch(codec: ReedSolomon, batch: PartBatch, present, expected_ptr: int, stream=None):
    """FilePart::read_with_context compute: verify loaded chunks, reconstruct_data.
    Returns (verified flags, per-part status)."""
    return _verify_rebuild(_lib.cec_read_batch, codec, batch, present, expected_ptr, stream)


def resilver_batch(codec: ReedSolomon, batch: PartBatch, present, expected_ptr: int,
                   stream=None):
    """FilePart::resilver compute: verify all chunks, rebuild missing data and parity."""
    return _verify_rebuild(_lib.cec_resilver_batch, codec, batch, present, expected_ptr, stream)


def _ragged_args(part_offsets, chunk_lens):
    n = len(chunk_lens)
    if len(part_offsets) != n:
        raise ValueError("part_offsets and chunk_lens differ in length")
    return ((ctypes.c_size_t * max(n, 1))(*part_offsets),
            (ctypes.c_size_t * max(n, 1))(*chunk_lens), n)


def reconstruct_ragged(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                       chunk_lens: Sequence[int], present, data_only: bool, stream=None) -> None:
    """:func:`reconstruct_batch` over parts of different chunk lengths
    (``cec_reconstruct_ragged``): device memory at ``base_ptr`` in the layout of
    :func:`ragged_layout`, ``present`` host flags ``n*(d+p)``."""
    offs, lens, n = _ragged_args(part_offsets, chunk_lens)
    pres = bytes(present)
    assert len(pres) == n * codec.total_shard_count()
    _check(_lib.cec_reconstruct_ragged(codec.handle, base_ptr, offs, lens, n,
                                       ctypes.cast(ctypes.c_char_p(pres), _u8p),
                                       1 if data_only else 0, _stream_ptr(stream)))


def _verify_rebuild_ragged(fn, codec, base_ptr, part_offsets, chunk_lens, present, expected_ptr,
                           stream):
    offs, lens, n = _ragged_args(part_offsets, chunk_lens)
    items = n * codec.total_shard_count()
    pres = bytes(present)
    assert len(pres) == items
    verified = (ctypes.c_uint8 * max(items, 1))()
    status = (ctypes.c_int * max(n, 1))()
    _check(fn(codec.handle, base_ptr, offs, lens, n, ctypes.cast(ctypes.c_char_p(pres), _u8p),
              expected_ptr, verified, status, _stream_ptr(stream)))
    return bytes(verified)[:items], list(status)[:n]


def read_ragged(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                chunk_lens: Sequence[int], present, expected_ptr: int, stream=None):
    """:func:`read_batch` over parts of different chunk lengths (``cec_read_ragged``).
    Returns (verified flags, per-part status)."""
    return _verify_rebuild_ragged(_lib.cec_read_ragged, codec, base_ptr, part_offsets,
                                  chunk_lens, present, expected_ptr, stream)


def resilver_ragged(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                    chunk_lens: Sequence[int], present, expected_ptr: int, stream=None):
    """:func:`resilver_batch` over parts of different chunk lengths (``cec_resilver_ragged``)."""
    return _verify_rebuild_ragged(_lib.cec_resilver_ragged, codec, base_ptr, part_offsets,
                                  chunk_lens, present, expected_ptr, stream)


def _verify_rebuild_ragged_async(fn, codec, base_ptr, part_offsets, chunk_lens, present,
                                 expected_ptr, verified, part_status, stream):
    offs, lens, n = _ragged_args(part_offsets, chunk_lens)
    items = n * codec.total_shard_count()
    pres = bytes(present)
    assert len(pres) == items
    if n and (_out_nbytes(verified) < items or
              _out_nbytes(part_status) < n * ctypes.sizeof(ctypes.c_int)):
        raise ValueError("verified needs n*(d+p) bytes and part_status n C ints")
    ver = ctypes.cast(_addr(verified), _u8p) if n else _u8p()
    st = ctypes.cast(_addr(part_status), ctypes.POINTER(ctypes.c_int)) if n else None
    _check(fn(codec.handle, base_ptr, offs, lens, n, ctypes.cast(ctypes.c_char_p(pres), _u8p),
              expected_ptr, ver, st, _stream_ptr(stream)))


def _out_nbytes(buf) -> int:
    return buf.nbytes if hasattr(buf, "nbytes") else _nbytes(buf)


def read_ragged_async(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                      chunk_lens: Sequence[int], present, expected_ptr: int, verified,
                      part_status, stream=None) -> None:
    """:func:`read_ragged` without the wait (``cec_read_ragged_async``): the decode is planned
    on the device, so the call only queues work on ``stream``.  ``verified`` (``n*(d+p)`` bytes)
    and ``part_status`` (``n`` C ints) are host buffers (a :class:`HostBuffer`, a numpy array or
    any writable buffer) that copies queued on the stream fill: valid once the stream's work is
    done, and to be kept alive until then.  Only page-locked buffers (:class:`HostBuffer`) keep
    the call from blocking."""
    _verify_rebuild_ragged_async(_lib.cec_read_ragged_async, codec, base_ptr, part_offsets,
                                 chunk_lens, present, expected_ptr, verified, part_status, stream)


def resilver_ragged_async(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                          chunk_lens: Sequence[int], present, expected_ptr: int, verified,
                          part_status, stream=None) -> None:
    """:func:`resilver_ragged` without the wait (``cec_resilver_ragged_async``); outputs as
    :func:`read_ragged_async`."""
    _verify_rebuild_ragged_async(_lib.cec_resilver_ragged_async, codec, base_ptr, part_offsets,
                                 chunk_lens, present, expected_ptr, verified, part_status, stream)


def read_ragged_packed_async(codec: ReedSolomon, base_ptr: int, part_offsets: Sequence[int],
                             chunk_lens: Sequence[int], present, expected_ptr: int, data_only: bool,
                             verified, part_status, rebuilt_ptr: int, rebuilt_cap: int,
                             rebuilt_offsets, stream=None) -> None:
    """:func:`read_ragged_async` (``data_only``) / :func:`resilver_ragged_async` with a packed
    return (``cec_read_ragged_packed_async``): every rebuilt chunk also lands in the device region
    at ``rebuilt_ptr`` (``rebuilt_cap`` bytes), dense and in part order, and ``rebuilt_offsets``
    (a host buffer of ``n+1`` ``size_t``) receives the parts' byte offsets into it through a copy
    queued on the stream, like ``verified`` and ``part_status``.  The r-th rebuilt chunk of part k
    is ``L_k`` bytes at ``rebuilt_offsets[k] + r * ragged_stride(L_k)``."""
    offs, lens, n = _ragged_args(part_offsets, chunk_lens)
    items = n * codec.total_shard_count()
    pres = bytes(present)
    assert len(pres) == items
    if n and (_out_nbytes(verified) < items or
              _out_nbytes(part_status) < n * ctypes.sizeof(ctypes.c_int) or
              _out_nbytes(rebuilt_offsets) < (n + 1) * ctypes.sizeof(ctypes.c_size_t)):
        raise ValueError("verified needs n*(d+p) bytes, part_status n C ints and rebuilt_offsets "
                         "n+1 size_t")
    ver = ctypes.cast(_addr(verified), _u8p) if n else _u8p()
    st = ctypes.cast(_addr(part_status), ctypes.POINTER(ctypes.c_int)) if n else None
    ro = ctypes.cast(_addr(rebuilt_offsets), _szp)
    _check(_lib.cec_read_ragged_packed_async(
        codec.handle, base_ptr, offs, lens, n, ctypes.cast(ctypes.c_char_p(pres), _u8p),
        expected_ptr, 1 if data_only else 0, ver, st, rebuilt_ptr, rebuilt_cap, ro,
        _stream_ptr(stream)))


def ragged_read_stats():
    """(device_planned, host_planned): ``*_ragged_async`` calls since load by who planned the
    decode (cec_ragged_read_stats); host_planned counts the shapes outside the device planner's
    scope (d > 32 or p > 8), which take the synchronous path inside the call."""
    dev, host = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.cec_ragged_read_stats(ctypes.byref(dev), ctypes.byref(host))
    return dev.value, host.value


def parts_read(codec: ReedSolomon, parts: Sequence[Sequence], expected: Sequence,
               data_only: bool = True):
    """The read counterpart of :func:`parts_encode` (``cec_parts_read``): verify and rebuild
    parts of unrelated chunk lengths in ONE engine call.  ``parts[k]`` lists the d+p chunks of
    part k: bytes-like for a loaded chunk, a ``(bytes-like, PRESENT_VERIFIED)`` pair for one an
    earlier pass verified, ``None`` for a missing one; every loaded chunk of a part has the
    part's chunk length.  ``expected[k]`` is the part's d+p digests (32 bytes each).  Returns
    ``(chunks, verified, status)``: ``chunks[k][i]`` is the loaded chunk as given when it
    verified, the rebuilt chunk as ``bytes``, or ``None`` where there is neither (missing parity
    under ``data_only``, what did not verify in a part whose status is
    ``TOO_FEW_SHARDS_PRESENT``); ``verified`` the flags ``n*(d+p)``; ``status`` per part."""
    d, t = codec.data_shard_count(), codec.total_shard_count()
    n = len(parts)
    if n == 0:
        return [], b"", []
    lens, pres, exp, slots, ptrs = _parts_read_args(d, t, parts, expected, data_only)
    verified = (ctypes.c_uint8 * (n * t))()
    status = (ctypes.c_int * n)()
    _check(_lib.cec_parts_read(codec.handle, ptrs, (ctypes.c_size_t * n)(*lens), n,
                               ctypes.cast(ctypes.c_char_p(pres), _u8p),
                               ctypes.cast(ctypes.c_char_p(exp), _u8p), 1 if data_only else 0,
                               verified, status))
    return _parts_read_result(d, t, parts, lens, slots, verified, status, data_only)


def part_read(codec: ReedSolomon, shards: Sequence, expected: Sequence, data_only: bool = True):
    """:func:`parts_read` for ONE part, coalesced (``cec_part_read``): the per-part call of the
    read side, ``read_with_context``'s (``data_only``) or ``resilver``'s compute in one call per
    FilePart task.  Concurrent calls with one codec and one mode share a launch whatever their
    chunk lengths.  ``shards`` lists the part's d+p chunks and ``expected`` its d+p digests as
    ``parts[k]`` / ``expected[k]`` of :func:`parts_read`.  Returns ``(chunks, verified, status)``
    for the part: ``status`` is ``OK`` or ``TOO_FEW_SHARDS_PRESENT`` (``verified`` is filled in
    both cases; nothing is rebuilt in the second)."""
    d, t = codec.data_shard_count(), codec.total_shard_count()
    lens, pres, exp, slots, ptrs = _parts_read_args(d, t, [shards], [expected], data_only)
    verified = (ctypes.c_uint8 * t)()
    code = _lib.cec_part_read(codec.handle, ptrs, lens[0],
                              ctypes.cast(ctypes.c_char_p(pres), _u8p),
                              ctypes.cast(ctypes.c_char_p(exp), _u8p), 1 if data_only else 0,
                              verified)
    if code not in (OK, TOO_FEW_SHARDS_PRESENT):
        raise Error(code)
    out, ver, _ = _parts_read_result(d, t, [shards], lens, slots, verified, [code], data_only)
    return out[0], ver, code


def coalesce_detail():
    """(part_mixed_batches, read_calls, read_launches) of the per-call coalescing path
    (cec_coalesce_detail): the ``part_encode`` batches of two or more chunk lengths, and the
    ``part_read`` calls made and launches issued."""
    mixed, calls, launches = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.cec_coalesce_detail(ctypes.byref(mixed), ctypes.byref(calls), ctypes.byref(launches))
    return mixed.value, calls.value, launches.value


def _parts_read_args(d, t, parts, expected, data_only):
    """:func:`parts_read`'s arguments in the C call's form: (chunk lengths, loaded flags, digest
    bytes, the engine's chunk slots by (k, i), their pointer array)."""
    n = len(parts)
    lens, flags, ptrs, slots = [], bytearray(n * t), [], {}
    for k, chunks in enumerate(parts):
        if len(chunks) != t:
            raise ValueError(f"part {k}: {len(chunks)} chunks, the codec has {t}")
        loaded = [c[0] if isinstance(c, tuple) else c for c in chunks]
        sizes = {_nbytes(c) for c in loaded if c is not None}
        if len(sizes) != 1:
            raise ValueError(f"part {k}: loaded chunks of sizes {sorted(sizes)}")
        L = sizes.pop()
        lens.append(L)
        for i, c in enumerate(chunks):
            if c is None and i >= d and data_only:
                ptrs.append(_u8p())  # never filled
                continue
            # the engine's own copy: a loaded chunk that fails verification is rebuilt in place
            slot = (ctypes.c_uint8 * max(L, 1))()
            if c is not None:
                flags[k * t + i] = c[1] if isinstance(c, tuple) else 1
                ctypes.memmove(slot, bytes(loaded[i]), L)
            slots[(k, i)] = slot
            ptrs.append(ctypes.cast(slot, _u8p))
    exp = b"".join(bytes(h) for part in expected for h in part)
    if len(exp) != n * t * 32:
        raise ValueError("expected: d+p digests of 32 bytes per part")
    return lens, bytes(flags), exp, slots, (_u8p * max(n * t, 1))(*ptrs)


def _parts_read_result(d, t, parts, lens, slots, verified, status, data_only):
    """:func:`parts_read`'s result from the flags, the statuses and the filled chunk slots."""
    out = []
    for k, chunks in enumerate(parts):
        row = []
        for i, c in enumerate(chunks):
            fillable = i < d or not data_only
            if verified[k * t + i]:
                row.append(c[0] if isinstance(c, tuple) else c)
            elif status[k] == OK and fillable:
                row.append(bytes(slots[(k, i)])[:lens[k]])
            else:
                row.append(None)
        out.append(row)
    return out, bytes(verified), [int(x) for x in status]


def verify_ragged(total_shards: int, base_ptr: int, part_offsets: Sequence[int],
                  chunk_lens: Sequence[int], present, expected_ptr: int, stream=None) -> bytes:
    """The verification half of :func:`read_ragged` alone (``cec_verify_ragged``):
    FilePart::verify's compute over device memory at ``base_ptr`` in the layout of
    :func:`ragged_layout` with ``total_shards`` chunks per part; nothing is rebuilt or written.
    ``present``: host flags ``n*total_shards`` or ``None`` (every chunk present);
    ``expected_ptr``: device digests ``[n][total_shards][32]``.  Returns the verified flags."""
    offs, lens, n = _ragged_args(part_offsets, chunk_lens)
    items = n * total_shards
    pres, c_pres = None, None  # NULL: every chunk present
    if present is not None:
        pres = bytes(present)
        assert len(pres) == items
        c_pres = ctypes.cast(ctypes.c_char_p(pres), _u8p)
    verified = (ctypes.c_uint8 * max(items, 1))()
    _check(_lib.cec_verify_ragged(total_shards, base_ptr, offs, lens, n, c_pres, expected_ptr,
                                  verified, _stream_ptr(stream)))
    return bytes(verified)[:items]


def parts_verify(copies: Sequence, expected: Sequence) -> bytes:
    """FilePart::verify's compute for a flat list of chunk copies of unrelated lengths in ONE
    engine call (``cec_parts_verify``): flag i of the result is 1 iff
    ``SHA-256(copies[i]) == expected[i]`` (32 bytes each).  An entry is a copy, not a chunk: a
    chunk with three locations is three entries with the same digest."""
    n = len(copies)
    if len(expected) != n:
        raise ValueError("copies and expected differ in length")
    if n == 0:
        return b""
    keep: list = []
    ptrs = (_u8p * n)(*[_buf_ptr(b, keep) for b in copies])
    lens = (ctypes.c_size_t * n)(*[_nbytes(b) for b in copies])
    exp = b"".join(bytes(h) for h in expected)
    if len(exp) != n * 32:
        raise ValueError("expected: one digest of 32 bytes per copy")
    ok = (ctypes.c_uint8 * n)()
    _check(_lib.cec_parts_verify(ptrs, lens, n, ctypes.cast(ctypes.c_char_p(exp), _u8p), ok))
    return bytes(ok)


def fill_synthetic(batch: PartBatch, n_chunks: int, seed: int, stream=None) -> None:
    s = batch.struct()
    _check(_lib.cec_fill_synthetic(ctypes.byref(s), n_chunks, seed, _stream_ptr(stream)))


def coalesce_stats():
    """(calls, launches) made through the per-call coalescing path (cec_coalesce_stats)."""
    calls, launches = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.cec_coalesce_stats(ctypes.byref(calls), ctypes.byref(launches))
    return calls.value, launches.value


def ragged_stats():
    """(fused, two_pass): ragged encode launch sequences queued by each path since load
    (cec_ragged_stats)."""
    fused, two_pass = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.cec_ragged_stats(ctypes.byref(fused), ctypes.byref(two_pass))
    return fused.value, two_pass.value


def synth_byte(seed: int, part: int, chunk: int, offset: int) -> int:
    return _lib.cec_synth_byte(seed, part, chunk, offset)


# ---------------------------------------------------------------------------------------------
# Host-staged write pipeline (FileWriteBuilder::write's part loop, batched)
# ---------------------------------------------------------------------------------------------


class Pipeline:
    """cec_pipeline: pinned host slots -> H2D -> fused encode+hash -> D2H, `depth` in flight.

    Usage per batch: ``slot, data = pl.acquire()`` (a writable numpy view of the pinned
    [parts][d][L] buffer), fill it, ``pl.submit(slot, n_parts)``, later
    ``parity, digests = pl.wait(slot)`` (numpy views valid until the slot is re-acquired).
    """

    def __init__(self, codec: ReedSolomon, chunk_len: int, parts_per_batch: int, depth: int = 4,
                 flags: int = 0):
        h = _vp()
        code = _lib.cec_pipeline_new_ex(codec.handle, chunk_len, parts_per_batch, depth, flags,
                                        ctypes.byref(h))
        if code != OK:
            raise Error(code)
        self._h = h
        self.codec = codec  # keep the codec alive
        self.d, self.p = codec.data_shard_count(), codec.parity_shard_count()
        self.L = chunk_len
        self.parts = parts_per_batch
        self.depth = depth

    def __del__(self, _free=_lib.cec_pipeline_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def acquire(self):
        import numpy as np
        slot = ctypes.c_size_t(0)
        ptr = _u8p()
        _check(_lib.cec_pipeline_acquire(self._h, ctypes.byref(slot), ctypes.byref(ptr)))
        if not ptr:  # PIPE_EXTERNAL: no slot buffer, batches come through submit_from
            return slot.value, None
        n = self.parts * self.d * self.L
        arr = np.ctypeslib.as_array(ptr, shape=(n,)).reshape(self.parts, self.d, self.L)
        return slot.value, arr

    def submit(self, slot: int, n_parts: int) -> None:
        _check(_lib.cec_pipeline_submit(self._h, slot, n_parts))

    def submit_from(self, slot: int, data, n_parts: int, parity=None, digests=None) -> None:
        """Batch from the caller's buffers (page-locked ones are DMA'd directly)."""
        _check(_lib.cec_pipeline_submit_from(self._h, slot, _addr(data), n_parts,
                                             _addr(parity) if parity is not None else None,
                                             _addr(digests) if digests is not None else None))

    def wait(self, slot: int):
        import numpy as np
        par, dig = _u8p(), _u8p()
        n = ctypes.c_size_t(0)
        _check(_lib.cec_pipeline_wait(self._h, slot, ctypes.byref(par), ctypes.byref(dig),
                                      ctypes.byref(n)))
        k = n.value
        parity = np.ctypeslib.as_array(par, shape=(max(k * self.p * self.L, 1),))[
            : k * self.p * self.L].reshape(k, self.p, self.L)
        digests = np.ctypeslib.as_array(dig, shape=(max(k * (self.d + self.p) * 32, 1),))[
            : k * (self.d + self.p) * 32].reshape(k, self.d + self.p, 32)
        return parity, digests

    def query(self, slot: int) -> bool:
        """True when the slot's batch is complete (never blocks)."""
        r = _lib.cec_pipeline_query(self._h, slot)
        if r < 0 or r > 1:
            raise Error(r)
        return bool(r)

    def drain(self) -> None:
        _check(_lib.cec_pipeline_drain(self._h))


class PartsPipeline:
    """cec_parts_pipeline: :func:`parts_encode` with `depth` slots in flight, for parts whose
    chunk lengths differ, in the split ragged layout (:func:`split_layout`).

    Per batch: ``slot, data = pl.acquire()`` (a writable numpy view of the slot's pinned data
    region), then either fill it in the packed split layout and ``pl.submit(slot, chunk_lens)``,
    or ``pl.submit_from(slot, bufs)`` (the engine packs; returns the chunk sizes); later
    ``parity, digests = pl.wait(slot)``: a numpy view of the slot's pinned parity region (part k's
    parity chunk i at ``parity_offsets[k] + i * ragged_stride(L_k)``) and ``[n][d+p][32]``
    digests, valid until the slot is acquired again.
    """

    def __init__(self, codec: ReedSolomon, slot_data_bytes: int, max_parts: int, depth: int = 3):
        h = _vp()
        _check(_lib.cec_parts_pipeline_new(codec.handle, slot_data_bytes, max_parts, depth,
                                           ctypes.byref(h)))
        self._h = h
        self.codec = codec  # keep the codec alive
        self.d, self.p = codec.data_shard_count(), codec.parity_shard_count()
        self.slot_data_bytes = slot_data_bytes
        self.max_parts = max_parts
        self.depth = depth
        self._parity_bytes = [0] * depth

    def __del__(self, _free=_lib.cec_parts_pipeline_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def acquire(self):
        import numpy as np
        slot = ctypes.c_size_t(0)
        ptr = _u8p()
        _check(_lib.cec_parts_pipeline_acquire(self._h, ctypes.byref(slot), ctypes.byref(ptr)))
        return slot.value, np.ctypeslib.as_array(ptr, shape=(self.slot_data_bytes,))

    def _submitted(self, slot: int, chunk_lens) -> None:
        self._parity_bytes[slot] = sum(self.p * ragged_stride(L) for L in chunk_lens)

    def submit(self, slot: int, chunk_lens: Sequence[int]) -> None:
        n = len(chunk_lens)
        lens = (ctypes.c_size_t * max(n, 1))(*chunk_lens)
        _check(_lib.cec_parts_pipeline_submit(self._h, slot, lens, n))
        self._submitted(slot, chunk_lens)

    def submit_from(self, slot: int, bufs: Sequence) -> List[int]:
        """Part k is the whole of ``bufs[k]``; returns the parts' chunk sizes."""
        n = len(bufs)
        keep: list = []
        ptrs = (_u8p * max(n, 1))(*[_buf_ptr(b, keep) for b in bufs])
        lens = (ctypes.c_size_t * max(n, 1))(*[_nbytes(b) for b in bufs])
        cs = (ctypes.c_size_t * max(n, 1))()
        _check(_lib.cec_parts_pipeline_submit_from(self._h, slot, ptrs, lens, n, cs))
        out = list(cs[:n])
        self._submitted(slot, out)
        return out

    def wait(self, slot: int):
        import numpy as np
        par, dig = _u8p(), _u8p()
        n = ctypes.c_size_t(0)
        _check(_lib.cec_parts_pipeline_wait(self._h, slot, ctypes.byref(par), ctypes.byref(dig),
                                            ctypes.byref(n)))
        k, t = n.value, self.d + self.p
        nb = self._parity_bytes[slot] if k else 0
        parity = np.ctypeslib.as_array(par, shape=(max(nb, 1),))[:nb]
        digests = np.ctypeslib.as_array(dig, shape=(max(k * t * 32, 1),))[: k * t * 32].reshape(
            k, t, 32)
        return parity, digests

    def query(self, slot: int) -> bool:
        """True when the slot's batch is complete (never blocks)."""
        r = _lib.cec_parts_pipeline_query(self._h, slot)
        if r < 0 or r > 1:
            raise Error(r)
        return bool(r)

    def drain(self) -> None:
        _check(_lib.cec_parts_pipeline_drain(self._h))


class SegmentPipeline:
    """cec_segment_pipeline: :class:`PartsPipeline` whose batches carry column segments of parts,
    so that a part with long chunks passes through in pieces and no batch waits for a long SHA-256
    chain.  The midstates of the parts under way ("open", each holding an id below `max_open`
    from its first to its last segment) stay on the device between batches.

    Per batch: ``slot = pl.acquire()``, ``pl.submit_from(slot, entries)`` with entries
    ``(buf, seg_offset, seg_len, open_id)`` (columns ``[seg_offset, seg_offset + seg_len)`` of each
    of the part's chunks; the id of a whole part is ignored), later ``parity, digests =
    pl.wait(slot)``: the parity pieces in the split layout of the batch's segment lengths and
    ``[n][d+p][32]`` digests, whose rows are valid for the entries that ended their part.
    """

    def __init__(self, codec: ReedSolomon, slot_data_bytes: int, max_parts: int, depth: int = 3,
                 max_open: int = 0):
        h = _vp()
        _check(_lib.cec_segment_pipeline_new(codec.handle, slot_data_bytes, max_parts, depth,
                                             max_open, ctypes.byref(h)))
        self._h = h
        self.codec = codec  # keep the codec alive
        self.d, self.p = codec.data_shard_count(), codec.parity_shard_count()
        self.slot_data_bytes = slot_data_bytes
        self.max_parts = max_parts
        self.depth = depth
        self.max_open = max_open
        self._parity_bytes = [0] * depth

    def __del__(self, _free=_lib.cec_segment_pipeline_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def acquire(self) -> int:
        slot = ctypes.c_size_t(0)
        _check(_lib.cec_segment_pipeline_acquire(self._h, ctypes.byref(slot)))
        return slot.value

    def submit_from(self, slot: int, entries: Sequence) -> List[int]:
        """``entries[k] = (buf, seg_offset, seg_len, open_id)``; returns the parts' chunk sizes."""
        n = len(entries)
        keep: list = []
        m = max(n, 1)
        ptrs = (_u8p * m)(*[_buf_ptr(e[0], keep) for e in entries])
        lens = (ctypes.c_size_t * m)(*[_nbytes(e[0]) for e in entries])
        offs = (ctypes.c_size_t * m)(*[e[1] for e in entries])
        segs = (ctypes.c_size_t * m)(*[e[2] for e in entries])
        ids = (ctypes.c_uint32 * m)(*[e[3] for e in entries])
        cs = (ctypes.c_size_t * m)()
        _check(_lib.cec_segment_pipeline_submit_from(self._h, slot, ptrs, lens, offs, segs, ids, n,
                                                     cs))
        self._parity_bytes[slot] = sum(self.p * ragged_stride(e[2]) for e in entries)
        return list(cs[:n])

    def wait(self, slot: int):
        import numpy as np
        par, dig = _u8p(), _u8p()
        n = ctypes.c_size_t(0)
        _check(_lib.cec_segment_pipeline_wait(self._h, slot, ctypes.byref(par), ctypes.byref(dig),
                                              ctypes.byref(n)))
        k, t = n.value, self.d + self.p
        nb = self._parity_bytes[slot] if k else 0
        parity = np.ctypeslib.as_array(par, shape=(max(nb, 1),))[:nb]
        digests = np.ctypeslib.as_array(dig, shape=(max(k * t * 32, 1),))[: k * t * 32].reshape(
            k, t, 32)
        return parity, digests

    def query(self, slot: int) -> bool:
        """True when the slot's batch is complete (never blocks)."""
        r = _lib.cec_segment_pipeline_query(self._h, slot)
        if r < 0 or r > 1:
            raise Error(r)
        return bool(r)

    def drain(self) -> None:
        _check(_lib.cec_segment_pipeline_drain(self._h))

    def open_count(self) -> int:
        return _lib.cec_segment_pipeline_open_count(self._h)

    def abandon(self, open_id: int) -> None:
        """Closes an open id whose part will not be finished."""
        _check(_lib.cec_segment_pipeline_abandon(self._h, open_id))


class ScrubPipeline:
    """cec_scrub_pipeline: :func:`parts_verify` with `depth` slots in flight, whose batches carry
    segments of stored copies, so that a long copy passes through in pieces and no batch waits for
    a long SHA-256 chain.  The midstates of the copies under way ("open", each holding an id below
    `max_open` from its first to its last segment) stay on the device between batches.  It runs on
    the current device; there is no codec.

    Per batch: ``slot = pl.acquire()``, ``pl.submit_from(slot, entries)`` with entries
    ``(buf, seg_offset, seg_len, open_id, expected)`` (bytes ``[seg_offset, seg_offset + seg_len)``
    of the copy ``buf``; the id of a whole copy is ignored; ``expected`` is the copy's 32-byte
    digest, read only for the entry that ends the copy, else it may be None), later ``ok =
    pl.wait(slot)``: one flag per entry, valid for the entries that ended their copy.
    """

    def __init__(self, slot_bytes: int, max_entries: int, depth: int = 3, max_open: int = 0):
        h = _vp()
        _check(_lib.cec_scrub_pipeline_new(slot_bytes, max_entries, depth, max_open,
                                           ctypes.byref(h)))
        self._h = h
        self.slot_bytes = slot_bytes
        self.max_entries = max_entries
        self.depth = depth
        self.max_open = max_open

    def __del__(self, _free=_lib.cec_scrub_pipeline_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def acquire(self) -> int:
        slot = ctypes.c_size_t(0)
        _check(_lib.cec_scrub_pipeline_acquire(self._h, ctypes.byref(slot)))
        return slot.value

    def submit_from(self, slot: int, entries: Sequence) -> None:
        """``entries[k] = (buf, seg_offset, seg_len, open_id, expected)``."""
        n = len(entries)
        keep: list = []
        m = max(n, 1)
        ptrs = (_u8p * m)(*[_buf_ptr(e[0], keep) for e in entries])
        lens = (ctypes.c_size_t * m)(*[_nbytes(e[0]) for e in entries])
        offs = (ctypes.c_size_t * m)(*[e[1] for e in entries])
        segs = (ctypes.c_size_t * m)(*[e[2] for e in entries])
        ids = (ctypes.c_uint32 * m)(*[e[3] for e in entries])
        rows = b"".join(bytes(e[4]) if e[4] is not None else bytes(32) for e in entries)
        if len(rows) != 32 * n:
            raise ValueError("an expected digest is not 32 bytes")
        exp = (ctypes.c_uint8 * (32 * m)).from_buffer_copy(rows.ljust(32 * m, b"\0"))
        _check(_lib.cec_scrub_pipeline_submit_from(self._h, slot, ptrs, lens, offs, segs, ids, exp,
                                                   n))

    def wait(self, slot: int):
        import numpy as np
        ok = _u8p()
        n = ctypes.c_size_t(0)
        _check(_lib.cec_scrub_pipeline_wait(self._h, slot, ctypes.byref(ok), ctypes.byref(n)))
        k = n.value
        if not k:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(ok, shape=(k,))

    def query(self, slot: int) -> bool:
        """True when the slot's batch is complete (never blocks)."""
        r = _lib.cec_scrub_pipeline_query(self._h, slot)
        if r < 0 or r > 1:
            raise Error(r)
        return bool(r)

    def drain(self) -> None:
        _check(_lib.cec_scrub_pipeline_drain(self._h))

    def open_count(self) -> int:
        return _lib.cec_scrub_pipeline_open_count(self._h)

    def abandon(self, open_id: int) -> None:
        """Closes an open id whose copy will not be finished."""
        _check(_lib.cec_scrub_pipeline_abandon(self._h, open_id))


class PartsReader:
    """cec_parts_reader: :func:`parts_read` with `depth` slots in flight, only the rebuilt chunks
    coming back, packed.

    Per batch: ``slot, stage = rd.acquire()`` (a writable numpy view of the slot's pinned staging
    region), then either place the loaded chunks at the :func:`ragged_layout` ``(d+p, chunk_lens)``
    offsets and ``rd.submit(slot, chunk_lens, present, expected)``, or
    ``rd.submit_from(slot, parts, expected)`` with ``parts`` in :func:`parts_read`'s form (the
    engine packs); later ``verified, status, rebuilt, offsets = rd.wait(slot)``: numpy views of
    pinned memory, valid until the slot is acquired again, the r-th rebuilt chunk of part k at
    ``rebuilt[offsets[k] + r * ragged_stride(L_k):][:L_k]``; or ``rd.collect(slot)``, which gives
    :func:`parts_read`'s result through ``cec_parts_reader_scatter``.
    """

    def __init__(self, codec: ReedSolomon, slot_bytes: int, max_parts: int, depth: int = 2,
                 data_only: bool = True):
        h = _vp()
        _check(_lib.cec_parts_reader_new(codec.handle, slot_bytes, max_parts, depth,
                                         1 if data_only else 0, ctypes.byref(h)))
        self._h = h
        self.codec = codec  # keep the codec alive
        self.d, self.p = codec.data_shard_count(), codec.parity_shard_count()
        self.slot_bytes = slot_bytes
        self.max_parts = max_parts
        self.depth = depth
        self.data_only = data_only
        self._batch = [None] * depth  # submit_from's (parts, lens, slots, pointer array)

    def __del__(self, _free=_lib.cec_parts_reader_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def acquire(self):
        import numpy as np
        slot = ctypes.c_size_t(0)
        ptr = _u8p()
        _check(_lib.cec_parts_reader_acquire(self._h, ctypes.byref(slot), ctypes.byref(ptr)))
        self._batch[slot.value] = None
        return slot.value, np.ctypeslib.as_array(ptr, shape=(self.slot_bytes,))

    def submit(self, slot: int, chunk_lens: Sequence[int], present, expected) -> None:
        """``present``: the ``n*(d+p)`` loaded flags; ``expected``: ``n*(d+p)*32`` digest bytes."""
        n = len(chunk_lens)
        lens = (ctypes.c_size_t * max(n, 1))(*chunk_lens)
        pres, exp = bytes(present), bytes(expected)
        if len(pres) != n * (self.d + self.p) or len(exp) != len(pres) * 32:
            raise ValueError("present needs n*(d+p) flags and expected 32 bytes for each")
        _check(_lib.cec_parts_reader_submit(self._h, slot, lens, n,
                                            ctypes.cast(ctypes.c_char_p(pres), _u8p),
                                            ctypes.cast(ctypes.c_char_p(exp), _u8p)))

    def submit_from(self, slot: int, parts: Sequence[Sequence], expected: Sequence) -> None:
        """``parts`` and ``expected`` as in :func:`parts_read`."""
        n = len(parts)
        lens, pres, exp, slots, arr = _parts_read_args(self.d, self.d + self.p, parts, expected,
                                                       self.data_only)
        _check(_lib.cec_parts_reader_submit_from(
            self._h, slot, arr, (ctypes.c_size_t * max(n, 1))(*lens), n,
            ctypes.cast(ctypes.c_char_p(pres), _u8p), ctypes.cast(ctypes.c_char_p(exp), _u8p)))
        self._batch[slot] = (parts, lens, slots, arr)

    def wait(self, slot: int):
        import numpy as np
        ver, reb = _u8p(), _u8p()
        st = ctypes.POINTER(ctypes.c_int)()
        off = _szp()
        n = ctypes.c_size_t(0)
        _check(_lib.cec_parts_reader_wait(self._h, slot, ctypes.byref(ver), ctypes.byref(st),
                                          ctypes.byref(reb), ctypes.byref(off), ctypes.byref(n)))
        k, t = n.value, self.d + self.p
        verified = np.ctypeslib.as_array(ver, shape=(max(k * t, 1),))[: k * t]
        status = np.ctypeslib.as_array(st, shape=(max(k, 1),))[:k]
        offsets = np.ctypeslib.as_array(off, shape=(k + 1,))
        total = int(offsets[k])
        rebuilt = np.ctypeslib.as_array(reb, shape=(max(total, 1),))[:total]
        return verified, status, rebuilt, offsets

    def collect(self, slot: int):
        """After :meth:`submit_from`: waits, scatters the rebuilt chunks into the batch's chunk
        slots (``cec_parts_reader_scatter``) and returns what :func:`parts_read` returns."""
        if self._batch[slot] is None:
            raise ValueError("collect needs a batch queued with submit_from on this slot")
        parts, lens, slots, arr = self._batch[slot]
        verified, status, _, _ = self.wait(slot)
        _check(_lib.cec_parts_reader_scatter(self._h, slot, arr))
        return _parts_read_result(self.d, self.d + self.p, parts, lens, slots, verified, status,
                                  self.data_only)

    def query(self, slot: int) -> bool:
        """True when the slot's batch is complete (never blocks)."""
        r = _lib.cec_parts_reader_query(self._h, slot)
        if r < 0 or r > 1:
            raise Error(r)
        return bool(r)

    def drain(self) -> None:
        _check(_lib.cec_parts_reader_drain(self._h))

    def stats(self):
        """(bytes_up, bytes_down, tail_copies) since the reader was made."""
        up, down, tails = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.cec_parts_reader_stats(self._h, ctypes.byref(up), ctypes.byref(down),
                                    ctypes.byref(tails))
        return up.value, down.value, tails.value


class ReadPipeline:
    """cec_read_pipeline: FileReadBuilder's part loop batched over pinned slots.

    ``slot, chunks, present, expected = rp.acquire()`` gives writable numpy views of the pinned
    [parts][d+p][L] chunk buffer, [parts][d+p] loaded flags and [parts][d+p][32] metadata
    digests; fill them, ``rp.submit(slot, n_parts)``; later
    ``data, verified, status = rp.wait(slot)`` -> [parts][d][L] part bytes (read_with_context's
    output), [parts][d+p] verification flags, [parts] status codes (views valid until the slot
    is re-acquired).
    """

    REBUILT_ONLY = 1  # CEC_READ_REBUILT_ONLY
    CARRY = 16  # CEC_READ_CARRY: retries' verified chunks kept on the device
    SUBMIT_PACKED = 32  # CEC_SUBMIT_PACKED (submit_ex)

    def __init__(self, codec: ReedSolomon, chunk_len: int, parts_per_batch: int, depth: int = 4,
                 flags: int = 0):
        h = _vp()
        code = _lib.cec_read_pipeline_new_ex(codec.handle, chunk_len, parts_per_batch, depth,
                                             flags, ctypes.byref(h))
        if code != OK:
            raise Error(code)
        self._h = h
        self.codec = codec
        self.d, self.p = codec.data_shard_count(), codec.parity_shard_count()
        self.t = self.d + self.p
        self.L = chunk_len
        self.parts = parts_per_batch
        self.depth = depth
        self.carry = bool(flags & self.CARRY)

    def __del__(self, _free=_lib.cec_read_pipeline_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def acquire(self):
        import numpy as np
        slot = ctypes.c_size_t(0)
        ch, pr, ex = _u8p(), _u8p(), _u8p()
        _check(_lib.cec_read_pipeline_acquire(self._h, ctypes.byref(slot), ctypes.byref(ch),
                                              ctypes.byref(pr), ctypes.byref(ex)))
        P, t, L = self.parts, self.t, self.L
        chunks = (np.ctypeslib.as_array(ch, shape=(P * t * L,)).reshape(P, t, L) if ch
                  else None)  # PIPE_EXTERNAL: chunks come through submit_from
        present = np.ctypeslib.as_array(pr, shape=(P * t,)).reshape(P, t)
        expected = np.ctypeslib.as_array(ex, shape=(P * t * 32,)).reshape(P, t, 32)
        return slot.value, chunks, present, expected

    def submit(self, slot: int, n_parts: int) -> None:
        _check(_lib.cec_read_pipeline_submit(self._h, slot, n_parts))

    def carry_ids(self, slot: int, n_parts: int):
        """[n_parts] int32: each part's carry entry after wait (-1: none; CARRY pipelines); the
        caller now holds the entries (submit them with a retry, or carry_release them)."""
        import numpy as np
        ids = np.full(self.parts, -1, np.int32)  # room for the largest batch a slot can hold
        _check(_lib.cec_read_pipeline_carry_ids(
            self._h, slot, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(ids)))
        return ids[:n_parts]

    def carry_held(self) -> int:
        """Carry entries the caller holds (taken with carry_ids, not yet used or released)."""
        return _lib.cec_read_pipeline_carry_held(self._h)

    def submit_ex(self, slot: int, n_parts: int, chunks=None, present=None, expected=None,
                  data=None, carry_ids=None, mode: int = 0, packed: bool = False) -> None:
        """cec_read_pipeline_submit_ex: any mode (0 read, REBUILT_ONLY, READ_RESILVER,
        READ_VERIFY_ONLY) on this pipeline, the caller's or the slot's buffers (None), carry ids
        (CARRY pipelines) and a packed upload."""
        import numpy as np
        ids = None
        if carry_ids is not None:
            ids = np.ascontiguousarray(carry_ids, dtype=np.int32)
            assert len(ids) >= n_parts
        a = ReadSubmitStruct(
            _addr(chunks) if chunks is not None else None,
            _addr(present) if present is not None else None,
            _addr(expected) if expected is not None else None, n_parts,
            _addr(data) if data is not None else None,
            ids.ctypes.data if ids is not None else None,
            mode | (self.SUBMIT_PACKED if packed else 0))
        code = _lib.cec_read_pipeline_submit_ex(self._h, slot, ctypes.byref(a))
        if code != OK:
            raise Error(code)

    def submit_carried(self, slot: int, n_parts: int, carry_ids) -> None:
        """submit, with carry_ids[n_parts] (-1 = none): those parts' CEC_PRESENT_VERIFIED chunks
        come from the carry pool (the slot need not hold them)."""
        import numpy as np
        ids = np.ascontiguousarray(carry_ids, dtype=np.int32)
        assert len(ids) >= n_parts
        code = _lib.cec_read_pipeline_submit_carried(
            self._h, slot, n_parts, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if code != OK:
            raise Error(code)

    def carry_release(self, carry_id: int) -> None:
        _check(_lib.cec_read_pipeline_carry_release(self._h, int(carry_id)))

    def submit_from(self, slot: int, chunks, present, expected, n_parts: int, data=None) -> None:
        """Batch from the caller's buffers (page-locked ones are DMA'd directly)."""
        _check(_lib.cec_read_pipeline_submit_from(
            self._h, slot, _addr(chunks), _addr(present), _addr(expected), n_parts,
            _addr(data) if data is not None else None))

    def submit_packed(self, slot: int, chunks, present, expected, n_parts: int,
                      data=None) -> None:
        """Batch whose loaded chunks are packed back to back in (part, chunk index) order
        (cec_read_pipeline_submit_packed): one upload per batch."""
        _check(_lib.cec_read_pipeline_submit_packed(
            self._h, slot, _addr(chunks), _addr(present), _addr(expected), n_parts,
            _addr(data) if data is not None else None))

    def wait(self, slot: int):
        import numpy as np
        data, ok = _u8p(), _u8p()
        status = ctypes.POINTER(ctypes.c_int)()
        n = ctypes.c_size_t(0)
        _check(_lib.cec_read_pipeline_wait(self._h, slot, ctypes.byref(data), ctypes.byref(ok),
                                           ctypes.byref(status), ctypes.byref(n)))
        k, t, d, L = n.value, self.t, self.d, self.L
        out = None  # a verify batch of a pipeline without its own output has none
        if data:
            out = np.ctypeslib.as_array(data, shape=(max(k * d * L, 1),))[: k * d * L].reshape(k, d, L)
        ver = np.ctypeslib.as_array(ok, shape=(max(k * t, 1),))[: k * t].reshape(k, t)
        st = np.ctypeslib.as_array(status, shape=(max(k, 1),))[:k]
        return out, ver, st

    def data_chunks(self, slot: int, n_parts: int, out_chunks: Optional[int] = None):
        """[n_parts][out] addresses of the output chunks (cec_read_pipeline_data_chunks; out = d,
        or d+p after a resilver batch)."""
        import numpy as np
        w = out_chunks or self.d
        ptrs = (ctypes.c_void_p * (self.parts * self.t))()  # room for any batch of the slot
        _check(_lib.cec_read_pipeline_data_chunks(self._h, slot, ptrs, len(ptrs)))
        return np.array([p or 0 for p in ptrs[: n_parts * w]],
                        dtype=np.uint64).reshape(n_parts, w)

    def part_bytes(self, slot: int, n_parts: int, k: int) -> bytes:
        """Part k's d data chunks concatenated (read_with_context's output), via data_chunks."""
        return b"".join(ctypes.string_at(int(a), self.L) for a in self.data_chunks(slot, n_parts)[k])

    def query(self, slot: int) -> bool:
        """True when the slot's batch is complete (never blocks)."""
        r = _lib.cec_read_pipeline_query(self._h, slot)
        if r < 0 or r > 1:
            raise Error(r)
        return bool(r)

    def drain(self) -> None:
        _check(_lib.cec_read_pipeline_drain(self._h))


# ---------------------------------------------------------------------------------------------
# Page-locked host memory (cec_host_alloc): buffers the engine DMAs directly
# ---------------------------------------------------------------------------------------------


def _addr(buf) -> int:
    """Address of a host buffer: a HostBuffer, a numpy array, or any writable bytes-like."""
    if isinstance(buf, HostBuffer):
        return buf.ptr
    if hasattr(buf, "__array_interface__"):
        return buf.__array_interface__["data"][0]
    mv = memoryview(buf)
    return ctypes.addressof((ctypes.c_char * mv.nbytes).from_buffer(mv.cast("B")))


class HostBuffer:
    """Page-locked, portable host memory from cec_host_alloc (pages on `device`'s NUMA node).
    ``.array`` is a writable numpy uint8 view.  Every view holds a reference to the HostBuffer
    (through its base buffer), so the memory is freed only once the object AND all views of it
    are gone: ``HostBuffer(n).view(a, b)`` is safe to keep."""

    def __init__(self, nbytes: int, device: int = -1):
        h = _vp()
        _check(_lib.cec_host_alloc(nbytes, device, ctypes.byref(h)))
        self.ptr = h.value
        self.nbytes = nbytes

    @property
    def array(self):
        import numpy as np
        if not self.ptr:
            raise ValueError("HostBuffer already freed")
        raw = (ctypes.c_uint8 * self.nbytes).from_address(self.ptr)
        raw._owner = self  # the numpy view's base is `raw`: it keeps this buffer alive
        return np.frombuffer(raw, dtype=np.uint8)

    def view(self, *shape):
        return self.array.reshape(*shape)

    def __del__(self, _free=_lib.cec_host_free):
        p = getattr(self, "ptr", None)
        if p:
            _free(p)
            self.ptr = None


def host_is_pinned(buf, nbytes: Optional[int] = None) -> bool:
    n = nbytes if nbytes is not None else (buf.nbytes if hasattr(buf, "nbytes") else _nbytes(buf))
    return bool(_lib.cec_host_is_pinned(_addr(buf), n))


def host_numa_node(buf) -> int:
    return _lib.cec_host_numa_node(_addr(buf))


def device_numa_node(device: int) -> int:
    return _lib.cec_device_numa_node(device)


def bind_thread_to_device_node(device: int) -> bool:
    """Restrict the calling thread to the CPUs of the device's NUMA node (False if impossible)."""
    return bool(_lib.cec_bind_thread_to_device_node(device))


def current_device() -> int:
    d = ctypes.c_int(0)
    _check(_lib.cec_current_device(ctypes.byref(d)))
    return d.value


def set_device(device: int) -> None:
    _check(_lib.cec_set_device(device))


# ---------------------------------------------------------------------------------------------
# Multi-GPU part scheduler (cec_multi_*): one process, contiguous part ranges per shard
# ---------------------------------------------------------------------------------------------

PIPE_EXTERNAL = 2  # CEC_PIPE_EXTERNAL
PRESENT_VERIFIED = 0x80  # CEC_PRESENT_VERIFIED: read-retry flag (loaded, verified by an earlier pass)
MULTI_AHEAD = 64  # CEC_MULTI_AHEAD: a read job queued ahead of the jobs not yet started
READ_RESILVER = 4  # CEC_READ_RESILVER: read-pipeline flag, FilePart::resilver's compute
READ_VERIFY_ONLY = 8  # CEC_READ_VERIFY_ONLY: read-pipeline flag, FilePart::verify's compute
READ_CARRY = 16  # CEC_READ_CARRY: read-pipeline flag, retries' verified chunks kept on the device


class MultiError(Error):
    def __init__(self, code: int):
        Exception.__init__(self, f"{_lib.cec_status_name(code).decode()}: "
                                 f"{_lib.cec_multi_last_error().decode()}")
        self.code = code
        self.name = _lib.cec_status_name(code).decode()


class Multi:
    """cec_multi: FileWriteBuilder::write / FileReadBuilder over several GPUs in one process.

    ``devices`` lists one device ordinal per shard (repeats allowed).  ``encode_hash`` /
    ``read`` take host buffers (numpy arrays or HostBuffer views; page-locked ones are DMA'd
    directly) and return a job id for ``wait``; the blocking forms ``encode_hash_sync`` /
    ``read_sync`` do both.  Shard g owns parts [g*n/G, (g+1)*n/G) of every job."""

    WRITE = 1  # CEC_MULTI_WRITE
    READ = 2  # CEC_MULTI_READ

    def __init__(self, codec: ReedSolomon, chunk_len: int, parts_per_batch: int, depth: int,
                 devices: Sequence[int], kinds: int = WRITE | READ):
        """``kinds``: the job kinds (WRITE, READ) whose pipelines every shard makes here, once."""
        h = _vp()
        devs = (ctypes.c_int * max(len(devices), 1))(*devices)
        code = _lib.cec_multi_new_ex(codec.handle, chunk_len, parts_per_batch, depth, devs,
                                     len(devices), kinds, ctypes.byref(h))
        if code != OK:
            raise MultiError(code)
        self._h = h
        self.codec = codec
        self.d, self.p = codec.data_shard_count(), codec.parity_shard_count()
        self.t = self.d + self.p
        self.L = chunk_len
        self._keep = {}

    def __del__(self, _free=_lib.cec_multi_free):
        h = getattr(self, "_h", None)
        if h:
            _free(h)
            self._h = None

    def shards(self) -> int:
        return _lib.cec_multi_shards(self._h)

    def shard_info(self, g: int):
        dev, numa, parts = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint64(0)
        _check(_lib.cec_multi_shard_info(self._h, g, ctypes.byref(dev), ctypes.byref(numa),
                                         ctypes.byref(parts)))
        return dev.value, numa.value, parts.value

    def stats(self, g: int) -> dict:
        """Shard g's counters (cec_multi_shard_stats)."""
        st = MultiStatsStruct()
        _check(_lib.cec_multi_shard_stats(self._h, g, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in MultiStatsStruct._fields_}

    def carry_release(self, carry_id: int) -> None:
        """Gives back a carry id this caller will not use (cec_multi_carry_release)."""
        code = _lib.cec_multi_carry_release(self._h, int(carry_id))
        if code != OK:
            raise MultiError(code)

    def encode_hash(self, data, n_parts: int, parity, digests) -> int:
        job = ctypes.c_uint64(0)
        code = _lib.cec_multi_encode_hash(self._h, _addr(data), n_parts, _addr(parity),
                                          _addr(digests), ctypes.byref(job))
        if code != OK:
            raise MultiError(code)
        self._keep[job.value] = (data, parity, digests)
        return job.value

    def read(self, chunks, present, expected, n_parts: int, data, verified, status,
             rebuilt_only: bool = False, carry_in=None, carry_out=None, ahead: bool = False):
        """Returns (job, data_ptrs) where data_ptrs ([n*d] c_void_p) is filled at wait().
        carry_out ([n] int32 numpy, nullable) receives, at wait(), a carry id for each part
        reported TOO_FEW_SHARDS_PRESENT whose verified chunks stay on its GPU (-1: none);
        carry_in ([n] int32, nullable) hands such ids to a retry: those parts' PRESENT_VERIFIED
        chunks are taken from the GPU, not from `chunks` (cec_multi_read_carry).  ahead
        (CEC_MULTI_AHEAD): the job goes ahead of the queued jobs not yet started (a reader's retry
        round, which the window being emitted waits for)."""
        import numpy as np
        job = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * max(n_parts * self.d, 1))()
        i32 = ctypes.POINTER(ctypes.c_int32)
        cin = None
        if carry_in is not None:
            cin = np.ascontiguousarray(carry_in, dtype=np.int32)
            assert len(cin) >= n_parts
        if carry_out is not None:
            assert carry_out.dtype == np.int32 and carry_out.flags.c_contiguous
            assert len(carry_out) >= n_parts
        code = _lib.cec_multi_read_carry(
            self._h, _addr(chunks), _addr(present), _addr(expected), n_parts, _addr(data),
            _addr(verified), ctypes.cast(_addr(status), ctypes.POINTER(ctypes.c_int)), ptrs,
            (1 if rebuilt_only else 0) | (MULTI_AHEAD if ahead else 0),
            cin.ctypes.data_as(i32) if cin is not None else None,
            carry_out.ctypes.data_as(i32) if carry_out is not None else None, ctypes.byref(job))
        if code != OK:
            raise MultiError(code)
        self._keep[job.value] = (chunks, present, expected, data, verified, status, ptrs, cin,
                                 carry_out)
        return job.value, ptrs

    def resilver(self, chunks, present, expected, n_parts: int, rebuilt, verified, status):
        """FilePart::resilver's compute; returns (job, chunk_ptrs [n*(d+p)] filled at wait())."""
        job = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * max(n_parts * self.t, 1))()
        code = _lib.cec_multi_resilver(self._h, _addr(chunks), _addr(present), _addr(expected),
                                       n_parts, _addr(rebuilt), _addr(verified),
                                       ctypes.cast(_addr(status), ctypes.POINTER(ctypes.c_int)),
                                       ptrs, ctypes.byref(job))
        if code != OK:
            raise MultiError(code)
        self._keep[job.value] = (chunks, present, expected, rebuilt, verified, status, ptrs)
        return job.value, ptrs

    def resilver_sync(self, chunks, present, expected, n_parts: int, rebuilt, verified, status):
        job, ptrs = self.resilver(chunks, present, expected, n_parts, rebuilt, verified, status)
        keep = self._keep[job]
        self.wait(job)
        del keep
        return [p or 0 for p in ptrs[: n_parts * self.t]]

    def verify(self, chunks, present, expected, n_parts: int, verified) -> int:
        """FilePart::verify's compute: verified[n][d+p] for every loaded chunk; returns the job."""
        job = ctypes.c_uint64(0)
        code = _lib.cec_multi_verify(self._h, _addr(chunks), _addr(present), _addr(expected),
                                     n_parts, _addr(verified), ctypes.byref(job))
        if code != OK:
            raise MultiError(code)
        self._keep[job.value] = (chunks, present, expected, verified)
        return job.value

    def verify_sync(self, chunks, present, expected, n_parts: int, verified) -> None:
        self.wait(self.verify(chunks, present, expected, n_parts, verified))

    def wait(self, job: int) -> None:
        code = _lib.cec_multi_wait(self._h, job)
        self._keep.pop(job, None)
        if code != OK:
            raise MultiError(code)

    def query(self, job: int) -> bool:
        """True when the job is done (wait() then returns at once); never blocks
        (cec_multi_query)."""
        code = _lib.cec_multi_query(self._h, job)
        if code not in (0, 1):
            raise MultiError(code)
        return code == 1

    def encode_hash_sync(self, data, n_parts: int, parity, digests) -> None:
        self.wait(self.encode_hash(data, n_parts, parity, digests))

    def read_sync(self, chunks, present, expected, n_parts: int, data, verified, status,
                  rebuilt_only: bool = False):
        job, ptrs = self.read(chunks, present, expected, n_parts, data, verified, status,
                              rebuilt_only)
        keep = self._keep[job]
        self.wait(job)
        del keep
        return [p or 0 for p in ptrs[: n_parts * self.d]]
