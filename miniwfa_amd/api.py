"""Python mirror of the miniwfa interface over the C ABI of libmwf_hip.so (include/miniwfa.h).

Names, argument meaning and error behaviour follow the reference API (miniwfa.h:36-89):
``opt_init()`` -> mwf_opt_init, ``wfa_exact`` -> mwf_wfa_exact, ``wfa_auto`` -> mwf_wfa_auto,
``cigar2score`` -> mwf_cigar2score.  ``Engine``/``Batch`` wrap the device-resident part of the ABI.

This module only marshals arguments.  All alignment work happens in the HIP kernels behind the
C ABI; if the shared library is missing or no GPU can be opened, calls raise — there is no
Python or CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Iterable, Sequence

import numpy as np

from . import build as _build

MWF_F_CIGAR = 0x1
MWF_F_NO_KALLOC = 0x2
MWF_F_DEBUG = 0x10000
CIGAR_CHARS = "MIDNSHP=XBid"  # reference main.c:78
# the six text products of a CIGAR (include/miniwfa.h): CIGAR string, SAM M-form, cs tag, MD tag, gapped target row, gapped query row
MWF_TXT_CIGAR, MWF_TXT_SAM, MWF_TXT_CS, MWF_TXT_MD, MWF_TXT_ROW_T, MWF_TXT_ROW_Q, MWF_TXT_KINDS = 0, 1, 2, 3, 4, 5, 6


class MwfOpt(C.Structure):
    """mwf_opt_t (reference miniwfa.h:36-44), 56 bytes."""
    _fields_ = [("flag", C.c_int32), ("x", C.c_int32), ("o1", C.c_int32), ("e1", C.c_int32),
                ("o2", C.c_int32), ("e2", C.c_int32), ("step", C.c_int32), ("max_s", C.c_int32),
                ("max_iter", C.c_int64), ("max_occ", C.c_int32), ("kmer", C.c_int32), ("min_len", C.c_int32)]


class MwfRst(C.Structure):
    """mwf_rst_t (reference miniwfa.h:46-51), 24 bytes."""
    _fields_ = [("s", C.c_int32), ("n_cigar", C.c_int32), ("n_iter", C.c_int64), ("cigar", C.POINTER(C.c_uint32))]


class MwfEnds(C.Structure):
    """mwf_ends_t (include/miniwfa.h), 16 bytes: the bases that may stay unaligned, free of charge, at the begin / end of target and query."""
    _fields_ = [("t_beg", C.c_int32), ("t_end", C.c_int32), ("q_beg", C.c_int32), ("q_end", C.c_int32)]


ENDS_FREE = 0x7fffffff  # an allowance that covers any sequence


class MwfExt(C.Structure):
    """mwf_ext_t (include/miniwfa.h), 8 bytes: the match score A of an extension alignment and its drop Z (-1: no drop rule)."""
    _fields_ = [("match", C.c_int32), ("zdrop", C.c_int32)]


MWF_EXT_END, MWF_EXT_DROP = 0, 1  # info[2] of an extension: why its pass ended


class MwfBand(C.Structure):
    """mwf_band_t (include/miniwfa.h), 8 bytes: the inclusive range of diagonals (query index - target index) an alignment must stay on."""
    _fields_ = [("d_lo", C.c_int32), ("d_hi", C.c_int32)]


def _ends_array(ends, n: int) -> np.ndarray:
    """(4,) or (n, 4) allowances as a C-contiguous int32 array of shape (1, 4) or (n, 4)."""
    a = np.ascontiguousarray(np.asarray(ends, dtype=np.int64))
    if a.shape == (4,):
        a = a.reshape(1, 4)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] not in (1, n):
        raise ValueError(f"ends must have shape (4,) or ({n}, 4), not {a.shape}")
    return np.ascontiguousarray(np.clip(a, -0x80000000, 0x7fffffff).astype(np.int32))


def _band_array(band, n: int):
    """(n, 2) bands as a C-contiguous int32 array, or None."""
    if band is None:
        return None
    a = np.asarray(band, dtype=np.int64)
    if n == 0 and a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape != (n, 2):
        raise ValueError(f"band must have shape ({n}, 2), not {a.shape}")
    return np.ascontiguousarray(np.clip(a, -0x80000000, 0x7fffffff).astype(np.int32))


class GpuStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("cells", C.c_int64), ("cells_pass1", C.c_int64), ("n_launches", C.c_int32),
                ("n_retries", C.c_int32), ("grid", C.c_int32), ("block", C.c_int32), ("kernel_kind", C.c_int32),
                ("dev_bytes", C.c_int64), ("dev_bytes_peak", C.c_int64), ("packed", C.c_int32), ("lowmem_two_pass", C.c_int32)]


class AlnSummary(C.Structure):
    """mwf_aln_summary_t (include/miniwfa.h), 48 bytes: what a CIGAR says about its pair and whether it aligns THESE sequences."""
    _fields_ = [("score", C.c_int32), ("t_len", C.c_int32), ("q_len", C.c_int32), ("n_eq", C.c_int32), ("n_x", C.c_int32),
                ("n_ins", C.c_int32), ("n_del", C.c_int32), ("n_ins_runs", C.c_int32), ("n_del_runs", C.c_int32),
                ("n_words", C.c_int32), ("first_bad", C.c_int32), ("flags", C.c_int32)]


# the same record as a numpy structured dtype: Batch.summary() returns an array of it
SUMMARY_DTYPE = np.dtype([(name, "<i4") for name, _ in AlnSummary._fields_])


class DevArray:
    """A device buffer owned by the library (or anyone) as a __cuda_array_interface__ object: torch.as_tensor(DevArray(ptr, n, "<i4"),
    device=...) is a zero-copy tensor over it.  typestr as in numpy ("<i4", "<i8", "<u4", "|u1"); the buffer must outlive the tensor."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr or 0), False), "version": 2}


class KmStat(C.Structure):
    _fields_ = [("capacity", C.c_size_t), ("available", C.c_size_t), ("n_blocks", C.c_size_t),
                ("n_cores", C.c_size_t), ("largest", C.c_size_t)]


# every symbol include/miniwfa.h and include/kalloc.h declare
ABI_SYMBOLS = (
    "mwf_opt_init", "mwf_wfa_exact", "mwf_wfa_auto", "mwf_wfa_chain", "mwf_cigar2score", "mwf_assert_cigar",
    "mwf_wfa_batch", "mwf_wfa_batch_multi", "mwf_wfa_chain_batch", "mwf_wfa_auto_batch", "mwf_wfa_submit", "mwf_wfa_wait", "mwf_wfa_async_stats", "mwf_gpu_batch_dev_status", "mwf_gpu_batch_fetch_cigars", "mwf_gpu_device_count", "mwf_gpu_create", "mwf_gpu_destroy", "mwf_gpu_last_error",
    "mwf_gpu_batch_upload", "mwf_gpu_batch_wrap", "mwf_gpu_batch_free", "mwf_gpu_batch_align", "mwf_gpu_batch_results",
    "mwf_gpu_batch_dev_scores", "mwf_gpu_batch_dev_iters", "mwf_gpu_batch_cigar", "mwf_gpu_get_stats", "mwf_gpu_set",
    "mwf_gpu_debug_band",
    "mwf_cigar_summary", "mwf_gpu_batch_dev_cigars", "mwf_gpu_batch_summarize", "mwf_gpu_batch_dev_summary", "mwf_gpu_batch_summary",
    "mwf_gpu_batch_map", "mwf_gpu_batch_dev_map", "mwf_gpu_batch_map_fetch",
    "mwf_cigar_text", "mwf_gpu_batch_text", "mwf_gpu_batch_dev_text", "mwf_gpu_batch_text_fetch",
    "mwf_alphabet_class", "mwf_alphabet_class16", "mwf_gpu_batch_alphabet",
    "mwf_gpu_batch_align_ends", "mwf_gpu_batch_ranges", "mwf_gpu_batch_dev_ranges", "mwf_wfa_ends", "mwf_wfa_ends_batch",
    "mwf_gpu_batch_align_ext", "mwf_gpu_batch_ext_info", "mwf_gpu_batch_dev_ext_info", "mwf_wfa_ext", "mwf_wfa_ext_batch",
    "mwf_gpu_batch_align_ends_pp", "mwf_gpu_batch_align_ext_band", "mwf_wfa_ends_pp_batch", "mwf_wfa_ext_band_batch",
    "kmalloc", "kcalloc", "krealloc", "krelocate", "kfree", "km_init", "km_init2", "km_destroy", "km_stat", "km_stat_print",
)

_lib = None


def lib() -> C.CDLL:
    """The C-ABI library (built on demand by hipcc; raises if that is impossible)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MWF_HIP_LIB")   # experiments only (e.g. an instrumented build); default: the in-tree library
    if not path:
        path = _build.LIB
        if not os.path.exists(path) or _build.stale():
            path = _build.build()
    L = C.CDLL(path)
    P = C.POINTER
    sig = [C.c_void_p, P(MwfOpt), C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, P(MwfRst)]
    for name in ("mwf_wfa_exact", "mwf_wfa_auto", "mwf_wfa_chain"):
        getattr(L, name).argtypes = sig
        getattr(L, name).restype = None
    L.mwf_opt_init.argtypes = [P(MwfOpt)]
    L.mwf_opt_init.restype = None
    L.mwf_cigar2score.argtypes = [P(MwfOpt), C.c_int32, P(C.c_uint32), P(C.c_int32), P(C.c_int32)]
    L.mwf_cigar2score.restype = C.c_int32
    L.mwf_assert_cigar.argtypes = [P(MwfOpt), C.c_int32, P(C.c_uint32), C.c_int32, C.c_int32, C.c_int32]
    L.mwf_assert_cigar.restype = None
    L.mwf_wfa_batch.argtypes = [C.c_void_p, P(MwfOpt), C.c_int32, P(C.c_int32), P(C.c_char_p), P(C.c_int32), P(C.c_char_p), P(MwfRst)]
    L.mwf_wfa_batch.restype = None
    L.mwf_wfa_batch_multi.argtypes = L.mwf_wfa_batch.argtypes + [C.c_int32, P(C.c_int32)]
    L.mwf_wfa_batch_multi.restype = None
    L.mwf_wfa_chain_batch.argtypes = L.mwf_wfa_batch.argtypes
    L.mwf_wfa_chain_batch.restype = None
    L.mwf_wfa_auto_batch.argtypes = L.mwf_wfa_batch.argtypes
    L.mwf_wfa_auto_batch.restype = None
    L.mwf_wfa_submit.argtypes = [P(MwfOpt), C.c_int32, C.c_char_p, C.c_int32, C.c_char_p]
    L.mwf_wfa_submit.restype = C.c_void_p
    L.mwf_wfa_wait.argtypes = [C.c_void_p, C.c_void_p, P(MwfRst)]
    L.mwf_wfa_wait.restype = None
    L.mwf_wfa_async_stats.argtypes = [P(C.c_int64), P(C.c_int64)]
    L.mwf_wfa_async_stats.restype = None
    L.mwf_gpu_batch_dev_status.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_dev_status.restype = C.c_void_p
    L.mwf_gpu_batch_fetch_cigars.argtypes = [C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_fetch_cigars.restype = C.c_int
    L.mwf_gpu_device_count.restype = C.c_int
    L.mwf_gpu_create.argtypes = [C.c_int, C.c_void_p]
    L.mwf_gpu_create.restype = C.c_void_p
    L.mwf_gpu_destroy.argtypes = [C.c_void_p]
    L.mwf_gpu_destroy.restype = None
    L.mwf_gpu_last_error.argtypes = [C.c_void_p]
    L.mwf_gpu_last_error.restype = C.c_char_p
    L.mwf_gpu_batch_upload.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_upload.restype = C.c_void_p
    L.mwf_gpu_batch_wrap.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_wrap.restype = C.c_void_p
    L.mwf_gpu_batch_free.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_free.restype = None
    L.mwf_gpu_batch_align.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt)]
    L.mwf_gpu_batch_align.restype = C.c_int
    L.mwf_gpu_batch_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_results.restype = C.c_int
    L.mwf_gpu_batch_dev_scores.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_dev_scores.restype = C.c_void_p
    L.mwf_gpu_batch_dev_iters.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_dev_iters.restype = C.c_void_p
    L.mwf_gpu_batch_cigar.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    L.mwf_gpu_batch_cigar.restype = C.c_int32
    L.mwf_gpu_get_stats.argtypes = [C.c_void_p, P(GpuStats)]
    L.mwf_gpu_get_stats.restype = None
    L.mwf_gpu_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.mwf_gpu_set.restype = C.c_int
    L.mwf_gpu_test_hook.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.mwf_gpu_test_hook.restype = C.c_int
    L.mwf_gpu_test_pair_sketch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_test_pair_sketch.restype = C.c_int
    L.mwf_gpu_debug_band.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt), C.c_int32, C.c_void_p, C.c_int32]
    L.mwf_gpu_debug_band.restype = C.c_int32
    L.mwf_cigar_summary.argtypes = [P(MwfOpt), C.c_int32, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, P(AlnSummary)]
    L.mwf_cigar_summary.restype = None
    L.mwf_gpu_batch_dev_cigars.argtypes = [C.c_void_p, C.c_void_p, P(C.c_void_p), P(C.c_void_p), P(C.c_void_p), P(C.c_int64)]
    L.mwf_gpu_batch_dev_cigars.restype = C.c_int
    L.mwf_gpu_batch_summarize.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_summarize.restype = C.c_int
    L.mwf_gpu_batch_dev_summary.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_dev_summary.restype = C.c_void_p
    L.mwf_gpu_batch_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_summary.restype = C.c_int
    L.mwf_gpu_batch_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.mwf_gpu_batch_map.restype = C.c_int
    L.mwf_gpu_batch_dev_map.argtypes = [C.c_void_p, C.c_int32]
    L.mwf_gpu_batch_dev_map.restype = C.c_void_p
    L.mwf_gpu_batch_map_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_map_fetch.restype = C.c_int
    L.mwf_cigar_text.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_int64]
    L.mwf_cigar_text.restype = C.c_int64
    L.mwf_gpu_batch_text.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_text.restype = C.c_int
    L.mwf_gpu_batch_dev_text.argtypes = [C.c_void_p, C.c_int32, P(C.c_void_p), P(C.c_int64)]
    L.mwf_gpu_batch_dev_text.restype = C.c_void_p
    L.mwf_gpu_batch_text_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_text_fetch.restype = C.c_int
    L.mwf_alphabet_class.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_void_p]
    L.mwf_alphabet_class.restype = C.c_int32
    L.mwf_alphabet_class16.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_void_p]
    L.mwf_alphabet_class16.restype = C.c_int32
    L.mwf_gpu_batch_alphabet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_alphabet.restype = C.c_int
    L.mwf_gpu_batch_align_ends.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt), P(MwfEnds)]
    L.mwf_gpu_batch_align_ends.restype = C.c_int
    L.mwf_gpu_batch_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_ranges.restype = C.c_int
    L.mwf_gpu_batch_dev_ranges.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_dev_ranges.restype = C.c_void_p
    L.mwf_wfa_ends.argtypes = [C.c_void_p, P(MwfOpt), P(MwfEnds), C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, P(MwfRst), C.c_void_p]
    L.mwf_wfa_ends.restype = None
    L.mwf_wfa_ends_batch.argtypes = [C.c_void_p, P(MwfOpt), P(MwfEnds), C.c_int32, P(C.c_int32), P(C.c_char_p), P(C.c_int32), P(C.c_char_p), P(MwfRst), C.c_void_p]
    L.mwf_wfa_ends_batch.restype = None
    L.mwf_gpu_batch_align_ext.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt), P(MwfExt)]
    L.mwf_gpu_batch_align_ext.restype = C.c_int
    L.mwf_gpu_batch_ext_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mwf_gpu_batch_ext_info.restype = C.c_int
    L.mwf_gpu_batch_dev_ext_info.argtypes = [C.c_void_p]
    L.mwf_gpu_batch_dev_ext_info.restype = C.c_void_p
    L.mwf_wfa_ext.argtypes = [C.c_void_p, P(MwfOpt), P(MwfExt), C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, P(MwfRst), C.c_void_p, C.c_void_p]
    L.mwf_wfa_ext.restype = None
    L.mwf_wfa_ext_batch.argtypes = [C.c_void_p, P(MwfOpt), P(MwfExt), C.c_int32, P(C.c_int32), P(C.c_char_p), P(C.c_int32), P(C.c_char_p), P(MwfRst), C.c_void_p, C.c_void_p]
    L.mwf_wfa_ext_batch.restype = None
    L.mwf_gpu_batch_align_ends_pp.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt), C.c_void_p, C.c_int32, C.c_void_p]
    L.mwf_gpu_batch_align_ends_pp.restype = C.c_int
    L.mwf_gpu_batch_align_ext_band.argtypes = [C.c_void_p, C.c_void_p, P(MwfOpt), P(MwfExt), C.c_void_p]
    L.mwf_gpu_batch_align_ext_band.restype = C.c_int
    L.mwf_wfa_ends_pp_batch.argtypes = [C.c_void_p, P(MwfOpt), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_char_p), P(C.c_int32), P(C.c_char_p), P(MwfRst), C.c_void_p]
    L.mwf_wfa_ends_pp_batch.restype = None
    L.mwf_wfa_ext_band_batch.argtypes = [C.c_void_p, P(MwfOpt), P(MwfExt), C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_char_p), P(C.c_int32), P(C.c_char_p), P(MwfRst), C.c_void_p, C.c_void_p]
    L.mwf_wfa_ext_band_batch.restype = None
    L.mwf_gpu_test_alpha_ms.argtypes = [C.c_void_p, P(C.c_double)]
    L.mwf_gpu_test_alpha_ms.restype = C.c_int
    for name, res, args in (("kmalloc", C.c_void_p, [C.c_void_p, C.c_size_t]), ("kcalloc", C.c_void_p, [C.c_void_p, C.c_size_t, C.c_size_t]),
                            ("krealloc", C.c_void_p, [C.c_void_p, C.c_void_p, C.c_size_t]), ("krelocate", C.c_void_p, [C.c_void_p, C.c_void_p, C.c_size_t]),
                            ("kfree", None, [C.c_void_p, C.c_void_p]), ("km_init", C.c_void_p, []), ("km_init2", C.c_void_p, [C.c_void_p, C.c_size_t]),
                            ("km_destroy", None, [C.c_void_p]), ("km_stat", None, [C.c_void_p, P(KmStat)]), ("km_stat_print", None, [C.c_void_p])):
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    _lib = L
    return L


def opt_init(**overrides) -> MwfOpt:
    """mwf_opt_init() (reference miniwfa.c:11-18) plus keyword overrides of individual fields."""
    o = MwfOpt()
    lib().mwf_opt_init(C.byref(o))
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


def cigar_str(words: Iterable[int]) -> str:
    """CIGAR words (len<<4|op) as text, the way reference main.c:76-79 prints them."""
    return "".join(f"{int(w) >> 4}{CIGAR_CHARS[int(w) & 0xf]}" for w in words)


def _take(r: MwfRst, km):
    cig = None
    if r.cigar:
        cig = [r.cigar[i] for i in range(r.n_cigar)]
        lib().kfree(km, C.cast(r.cigar, C.c_void_p))
    return r.s, r.n_iter, cig


def wfa_exact(t: bytes, q: bytes, opt: MwfOpt, km=None):
    """mwf_wfa_exact (reference miniwfa.c:603-615) -> (s, n_iter, cigar words or None)."""
    r = MwfRst()
    lib().mwf_wfa_exact(km, C.byref(opt), len(t), t, len(q), q, C.byref(r))
    return _take(r, km)


def wfa_auto(t: bytes, q: bytes, opt: MwfOpt, km=None):
    """mwf_wfa_auto (reference miniwfa.c:898-908)."""
    r = MwfRst()
    lib().mwf_wfa_auto(km, C.byref(opt), len(t), t, len(q), q, C.byref(r))
    return _take(r, km)


def wfa_chain(t: bytes, q: bytes, opt: MwfOpt, km=None):
    """mwf_wfa_chain (reference miniwfa.c:850-896)."""
    r = MwfRst()
    lib().mwf_wfa_chain(km, C.byref(opt), len(t), t, len(q), q, C.byref(r))
    return _take(r, km)


def wfa_chain_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, km=None):
    """mwf_wfa_chain_batch: mwf_wfa_chain of every pair, their gap fills in one device batch -> list of (s, n_iter, cigar)."""
    n = len(pairs)
    if n == 0:
        return []
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    lib().mwf_wfa_chain_batch(km, C.byref(opt), n, tl, ts, ql, qs, r)
    return [_take(r[i], km) for i in range(n)]


def wfa_auto_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, km=None):
    """mwf_wfa_auto_batch: mwf_wfa_auto of every pair (exact branch as one batch, chain mode for what it gives up on) -> list of (s, n_iter, cigar)."""
    n = len(pairs)
    if n == 0:
        return []
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    lib().mwf_wfa_auto_batch(km, C.byref(opt), n, tl, ts, ql, qs, r)
    return [_take(r[i], km) for i in range(n)]


class Job:
    """A pair submitted with mwf_wfa_submit; keeps the buffers it borrows alive until wait()."""

    def __init__(self, t: bytes, q: bytes, opt: MwfOpt):
        self._keep = (t, q, opt)
        self.h = lib().mwf_wfa_submit(C.byref(opt), len(t), t, len(q), q)
        if not self.h:
            raise ValueError("mwf_wfa_submit refused the pair")

    def wait(self, km=None):
        """mwf_wfa_wait -> (s, n_iter, cigar words or None), exactly what wfa_exact returns for the pair."""
        r = MwfRst()
        lib().mwf_wfa_wait(km, self.h, C.byref(r))
        self.h = None
        return _take(r, km)


def wfa_submit(t: bytes, q: bytes, opt: MwfOpt) -> Job:
    """mwf_wfa_submit: queue one pair for the dispatcher (include/miniwfa.h part 2); job.wait() collects it."""
    return Job(t, q, opt)


def async_stats():
    """(batches the dispatcher has run, pairs in them)."""
    a, b = C.c_int64(), C.c_int64()
    lib().mwf_wfa_async_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def wfa_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, km=None):
    """mwf_wfa_batch over host buffers -> list of (s, n_iter, cigar)."""
    n = len(pairs)
    if n == 0:
        return []
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    lib().mwf_wfa_batch(km, C.byref(opt), n, tl, ts, ql, qs, r)
    return [_take(r[i], km) for i in range(n)]


def wfa_batch_multi(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, devices: Sequence[int] | None = None, n_dev: int = 0, km=None):
    """mwf_wfa_batch_multi: the batch dealt over several devices (an ordinal may repeat) -> list of (s, n_iter, cigar)."""
    n = len(pairs)
    if n == 0:
        return []
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    dv = (C.c_int32 * len(devices))(*devices) if devices else None
    lib().mwf_wfa_batch_multi(km, C.byref(opt), n, tl, ts, ql, qs, r, len(devices) if devices else n_dev, dv)
    return [_take(r[i], km) for i in range(n)]


def wfa_ends_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, t_beg: int = 0, t_end: int = 0, q_beg: int = 0, q_end: int = 0, km=None):
    """mwf_wfa_ends_batch: ends-free alignment of host buffers -> list of (s, n_iter, cigar, (tb, te, qb, qe))."""
    n = len(pairs)
    if n == 0:
        return []
    ends = MwfEnds(t_beg, t_end, q_beg, q_end)
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    rng = np.zeros((n, 4), dtype=np.int32)
    lib().mwf_wfa_ends_batch(km, C.byref(opt), C.byref(ends), n, tl, ts, ql, qs, r, rng.ctypes.data)
    return [_take(r[i], km) + (tuple(int(v) for v in rng[i]),) for i in range(n)]


def wfa_ends(t: bytes, q: bytes, opt: MwfOpt, t_beg: int = 0, t_end: int = 0, q_beg: int = 0, q_end: int = 0, km=None):
    """mwf_wfa_ends: one ends-free alignment -> (s, n_iter, cigar words or None, (tb, te, qb, qe))."""
    ends = MwfEnds(t_beg, t_end, q_beg, q_end)
    r = MwfRst()
    rng = np.zeros(4, dtype=np.int32)
    lib().mwf_wfa_ends(km, C.byref(opt), C.byref(ends), len(t), t, len(q), q, C.byref(r), rng.ctypes.data)
    return _take(r, km) + (tuple(int(v) for v in rng),)


def wfa_ext_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, match: int = 1, zdrop: int = -1, km=None):
    """mwf_wfa_ext_batch: extension alignment of host buffers -> list of (s, n_iter, cigar, (tb, te, qb, qe), (V, s_stop, why, F))."""
    n = len(pairs)
    if n == 0:
        return []
    ext = MwfExt(match, zdrop)
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    rng = np.zeros((n, 4), dtype=np.int32)
    info = np.zeros((n, 4), dtype=np.int32)
    lib().mwf_wfa_ext_batch(km, C.byref(opt), C.byref(ext), n, tl, ts, ql, qs, r, rng.ctypes.data, info.ctypes.data)
    return [_take(r[i], km) + (tuple(int(v) for v in rng[i]), tuple(int(v) for v in info[i])) for i in range(n)]


def wfa_ends_pp_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, ends, band=None, km=None):
    """mwf_wfa_ends_pp_batch: ends-free alignment of host buffers under per-pair allowances (ends: (4,) or (n, 4)) and bands (band: (n, 2) or None)
    -> list of (s, n_iter, cigar, (tb, te, qb, qe))."""
    n = len(pairs)
    if n == 0:
        return []
    e, bd = _ends_array(ends, n), _band_array(band, n)
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    rng = np.zeros((n, 4), dtype=np.int32)
    lib().mwf_wfa_ends_pp_batch(km, C.byref(opt), e.ctypes.data, e.shape[0], None if bd is None else bd.ctypes.data, n, tl, ts, ql, qs, r, rng.ctypes.data)
    return [_take(r[i], km) + (tuple(int(v) for v in rng[i]),) for i in range(n)]


def wfa_ext_band_batch(pairs: Sequence[tuple[bytes, bytes]], opt: MwfOpt, band, match: int = 1, zdrop: int = -1, km=None):
    """mwf_wfa_ext_band_batch: extension alignment of host buffers under per-pair bands (band: (n, 2))
    -> list of (s, n_iter, cigar, (tb, te, qb, qe), (V, s_stop, why, F))."""
    n = len(pairs)
    if n == 0:
        return []
    ext, bd = MwfExt(match, zdrop), _band_array(band, n)
    if bd is None:
        raise ValueError("band must not be None")
    tl = (C.c_int32 * n)(*[len(t) for t, _ in pairs])
    ql = (C.c_int32 * n)(*[len(q) for _, q in pairs])
    ts = (C.c_char_p * n)(*[t for t, _ in pairs])
    qs = (C.c_char_p * n)(*[q for _, q in pairs])
    r = (MwfRst * n)()
    rng = np.zeros((n, 4), dtype=np.int32)
    info = np.zeros((n, 4), dtype=np.int32)
    lib().mwf_wfa_ext_band_batch(km, C.byref(opt), C.byref(ext), bd.ctypes.data, n, tl, ts, ql, qs, r, rng.ctypes.data, info.ctypes.data)
    return [_take(r[i], km) + (tuple(int(v) for v in rng[i]), tuple(int(v) for v in info[i])) for i in range(n)]


def wfa_ext(t: bytes, q: bytes, opt: MwfOpt, match: int = 1, zdrop: int = -1, km=None):
    """mwf_wfa_ext: one extension alignment -> (s, n_iter, cigar words or None, (tb, te, qb, qe), (V, s_stop, why, F))."""
    ext = MwfExt(match, zdrop)
    r = MwfRst()
    rng = np.zeros(4, dtype=np.int32)
    info = np.zeros(4, dtype=np.int32)
    lib().mwf_wfa_ext(km, C.byref(opt), C.byref(ext), len(t), t, len(q), q, C.byref(r), rng.ctypes.data, info.ctypes.data)
    return _take(r, km) + (tuple(int(v) for v in rng), tuple(int(v) for v in info))


def cigar2score(opt: MwfOpt, cigar: Sequence[int]):
    """mwf_cigar2score (reference mwf-dbg.c:6-22) -> (score, target length, query length)."""
    arr = (C.c_uint32 * max(1, len(cigar)))(*cigar)
    tl, ql = C.c_int32(), C.c_int32()
    s = lib().mwf_cigar2score(C.byref(opt), len(cigar), arr, C.byref(tl), C.byref(ql))
    return s, tl.value, ql.value


def cigar_summary(t: bytes, q: bytes, opt: MwfOpt, cigar: Sequence[int]) -> np.void:
    """mwf_cigar_summary, the host twin of Batch.summary(): one SUMMARY_DTYPE record for `cigar` (words len<<4|op) against (t, q).  Needs no device."""
    words = np.ascontiguousarray(np.asarray(cigar, dtype=np.uint32))
    out = AlnSummary()
    lib().mwf_cigar_summary(C.byref(opt), len(words), words.ctypes.data if len(words) else None, len(t), t, len(q), q, C.byref(out))
    return np.frombuffer(bytes(out), dtype=SUMMARY_DTYPE)[0]


def cigar_text(kind: int, t: bytes, q: bytes, cigar: Sequence[int]) -> bytes | None:
    """mwf_cigar_text, the host twin of Batch.texts(): text `kind` (MWF_TXT_*) of `cigar` (words len<<4|op) against (t, q); None when the words are
    not renderable for the pair or kind is out of range.  Needs no device."""
    words = np.ascontiguousarray(np.asarray(cigar, dtype=np.uint32))
    wp = words.ctypes.data if len(words) else None
    n = lib().mwf_cigar_text(kind, len(words), wp, len(t), t, len(q), q, None, 0)
    if n < 0:
        return None
    buf = C.create_string_buffer(max(1, n))
    lib().mwf_cigar_text(kind, len(words), wp, len(t), t, len(q), q, buf, n)
    return buf.raw[:n]


def alphabet_class(t: bytes, q: bytes):
    """mwf_alphabet_class -> (class, map): 0 every byte of the pair is one of A C G T, 1 at most four distinct bytes (and not class 0), 2 five or
    more.  map: 256 bytes; for class 1 the letter (A, C, G, T by ascending byte value) of every byte that occurs and 0 elsewhere, else all 0 —
    bytes(t).translate(map) is the pair as "alpha_remap" aligns it.  Needs no device."""
    m = (C.c_uint8 * 256)()
    cls = lib().mwf_alphabet_class(len(t), t, len(q), q, m)
    return int(cls), bytes(m)


ALPHA16_TAG = 0x40  # MWF_ALPHA16_TAG: the high nibble of a class-3 image byte


def alphabet_class16(t: bytes, q: bytes):
    """mwf_alphabet_class16 -> (class, map): the classes an engine reports under "alpha16" 1 — 0 and 1 as alphabet_class, 3 five to sixteen distinct
    bytes, 2 seventeen or more.  map: for class 1 as alphabet_class gives it; for class 3 ALPHA16_TAG | code (codes 0 ... 15 by ascending byte value)
    for every byte that occurs and 0 elsewhere; else all 0 — bytes(t).translate(map) is the pair as "alpha16" aligns it.  Needs no device."""
    m = (C.c_uint8 * 256)()
    cls = lib().mwf_alphabet_class16(len(t), t, len(q), q, m)
    return int(cls), bytes(m)


class Engine:
    """mwf_gpu_t: one device, one stream, one workspace pool."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = lib()
        if L.mwf_gpu_device_count() <= 0:
            raise RuntimeError("libmwf_hip: no HIP device visible; the library has no CPU path")
        self.h = L.mwf_gpu_create(device, stream)
        if not self.h:
            raise RuntimeError(f"libmwf_hip: cannot open device {device}")
        self.device = device
        self._batches = weakref.WeakSet()

    def close(self):
        if self.h:
            for b in list(self._batches):  # a batch must not outlive its engine
                b.free()
            lib().mwf_gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self) -> str:
        return lib().mwf_gpu_last_error(self.h).decode()

    def set(self, name: str, value: int):
        """A user tunable (mwf_gpu_set, include/miniwfa.h) or — for tests and profiling scripts — one of the library's test hooks
        (mwf_gpu_test_hook: forced kernels / geometries / failure paths; exported, not part of the public header)."""
        if lib().mwf_gpu_set(self.h, name.encode(), int(value)) != 0 and lib().mwf_gpu_test_hook(self.h, name.encode(), int(value)) != 0:
            raise ValueError(f"bad tunable {name}={value}")

    def alpha_ms(self):
        """(classification ms, copy ms) of the mwf_alphabet.hip launches of the engine's last align, from HIP events (test hook; 0.0: not launched)."""
        ms = (C.c_double * 2)()
        if lib().mwf_gpu_test_alpha_ms(self.h, ms) != 0:
            raise RuntimeError("alpha_ms failed: " + self.error())
        return float(ms[0]), float(ms[1])

    def stats(self) -> GpuStats:
        st = GpuStats()
        lib().mwf_gpu_get_stats(self.h, C.byref(st))
        return st

    def upload(self, packed) -> "Batch":
        """Batch from a miniwfa_amd.synth.PackedBatch living in host memory."""
        h = lib().mwf_gpu_batch_upload(self.h, packed.n, packed.seqs.ctypes.data, packed.total, packed.t_off.ctypes.data,
                                       packed.tl.ctypes.data, packed.q_off.ctypes.data, packed.ql.ctypes.data)
        if not h:
            raise RuntimeError("upload failed: " + self.error())
        return Batch(self, h, packed.n, keep=(packed,))

    def wrap(self, n, d_seqs_ptr, seq_bytes, d_t_off_ptr, d_tl_ptr, d_q_off_ptr, d_ql_ptr, h_tl: np.ndarray, h_ql: np.ndarray, keep=()) -> "Batch":
        """Batch over buffers that already live in this device's HBM (e.g. torch tensors' data_ptr())."""
        h_tl = np.ascontiguousarray(h_tl, dtype=np.int32)
        h_ql = np.ascontiguousarray(h_ql, dtype=np.int32)
        h = lib().mwf_gpu_batch_wrap(self.h, n, d_seqs_ptr, seq_bytes, d_t_off_ptr, d_tl_ptr, d_q_off_ptr, d_ql_ptr,
                                     h_tl.ctypes.data, h_ql.ctypes.data)
        if not h:
            raise RuntimeError("wrap failed: " + self.error())
        return Batch(self, h, n, keep=tuple(keep))

    def wrap_packed(self, packed, torch_device) -> "Batch":
        """A miniwfa_amd.synth.PackedBatch copied into torch tensors on `torch_device` and wrapped zero-copy: the device-resident path a
        torch program uses — the library never sees the bytes on the host."""
        import torch
        t = [torch.from_numpy(np.array(a, copy=True)).to(torch_device) for a in (packed.seqs, packed.t_off, packed.tl, packed.q_off, packed.ql)]
        torch.cuda.synchronize(torch_device)
        return self.wrap(packed.n, t[0].data_ptr(), packed.total, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                         packed.tl, packed.ql, keep=tuple(t))


class Batch:
    """mwf_gpu_batch_t."""

    def __init__(self, eng: Engine, handle, n: int, keep=()):
        self.eng, self.h, self.n, self._keep = eng, handle, n, keep
        eng._batches.add(self)

    def free(self):
        if self.h and self.eng.h:
            lib().mwf_gpu_batch_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def align(self, opt: MwfOpt):
        """Enqueue the alignment kernels on the engine's stream."""
        rc = lib().mwf_gpu_batch_align(self.eng.h, self.h, C.byref(opt))
        if rc != 0:
            raise RuntimeError(f"align failed ({rc}): " + self.eng.error())

    def align_ends(self, opt: MwfOpt, t_beg: int = 0, t_end: int = 0, q_beg: int = 0, q_end: int = 0):
        """Enqueue an ends-free alignment (mwf_gpu_batch_align_ends): up to t_beg / q_beg bases in front of and t_end / q_end bases behind the aligned
        ranges are free (ENDS_FREE: any number).  results(), cigar(), summary() and texts() work as after align(); ranges() gives what was aligned."""
        ends = MwfEnds(t_beg, t_end, q_beg, q_end)
        rc = lib().mwf_gpu_batch_align_ends(self.eng.h, self.h, C.byref(opt), C.byref(ends))
        if rc != 0:
            raise RuntimeError(f"align_ends failed ({rc}): " + self.eng.error())

    def align_ends_pp(self, opt: MwfOpt, ends, band=None):
        """Enqueue an ends-free alignment under per-pair parameters (mwf_gpu_batch_align_ends_pp): ends is array-like of shape (4,) — one set of
        (t_beg, t_end, q_beg, q_end) for every pair — or (n, 4); band is None or array-like of shape (n, 2), the inclusive diagonals (d_lo, d_hi),
        d = query index - target index, pair i's alignment must stay on (include/miniwfa.h, mwf_band_t).  A pair whose band admits no alignment
        comes back with s == -1 and n_iter == 0.  Afterwards as after align_ends()."""
        e, bd = _ends_array(ends, self.n), _band_array(band, self.n)
        rc = lib().mwf_gpu_batch_align_ends_pp(self.eng.h, self.h, C.byref(opt), e.ctypes.data, e.shape[0], None if bd is None else bd.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"align_ends_pp failed ({rc}): " + self.eng.error())

    def align_ext(self, opt: MwfOpt, match: int = 1, zdrop: int = -1, band=None):
        """Enqueue an extension alignment (mwf_gpu_batch_align_ext): from the origin outwards, the prefix pair that scores best under match +`match`
        (include/miniwfa.h, mwf_ext_t); the pass stops at an edge of the matrix or, with zdrop >= 0, once the best score leads by more than zdrop.
        band: None, or array-like of shape (n, 2): the diagonals (d_lo, d_hi) pair i's extension must stay on (mwf_gpu_batch_align_ext_band).
        Afterwards as after align_ends(); ext_info() says what the pass found and why it stopped."""
        ext = MwfExt(match, zdrop)
        bd = _band_array(band, self.n)
        if bd is not None:
            rc = lib().mwf_gpu_batch_align_ext_band(self.eng.h, self.h, C.byref(opt), C.byref(ext), bd.ctypes.data)
            if rc != 0:
                raise RuntimeError(f"align_ext failed ({rc}): " + self.eng.error())
            return
        rc = lib().mwf_gpu_batch_align_ext(self.eng.h, self.h, C.byref(opt), C.byref(ext))
        if rc != 0:
            raise RuntimeError(f"align_ext failed ({rc}): " + self.eng.error())

    def ext_info(self) -> np.ndarray:
        """int32[n, 4]: (V, s_stop, why, F) of every pair of the last align_ext(); waits for the stream.  Raises after any other align."""
        out = np.zeros((max(1, self.n), 4), dtype=np.int32)
        rc = lib().mwf_gpu_batch_ext_info(self.eng.h, self.h, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"ext_info failed ({rc}): " + self.eng.error())
        return out[:self.n]

    def dev_ext_info_ptr(self) -> int | None:
        """Device pointer to the n x 4 int32 info of the last align_ext(); None after any other align."""
        return lib().mwf_gpu_batch_dev_ext_info(self.h)

    def ranges(self) -> np.ndarray:
        """int32[n, 4]: (tb, te, qb, qe) of every pair of the last align_ends(), half-open; waits for the stream.  Raises after a plain align()."""
        out = np.zeros((max(1, self.n), 4), dtype=np.int32)
        rc = lib().mwf_gpu_batch_ranges(self.eng.h, self.h, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"ranges failed ({rc}): " + self.eng.error())
        return out[:self.n]

    def dev_ranges_ptr(self) -> int | None:
        """Device pointer to the n x 4 int32 ranges of the last align_ends(); None after a plain align()."""
        return lib().mwf_gpu_batch_dev_ranges(self.h)

    def results(self):
        """(s[int32], n_iter[int64], n_cigar[int32]) as numpy arrays; waits for the stream."""
        s = np.zeros(self.n, dtype=np.int32)
        it = np.zeros(self.n, dtype=np.int64)
        nc = np.zeros(self.n, dtype=np.int32)
        rc = lib().mwf_gpu_batch_results(self.eng.h, self.h, s.ctypes.data, it.ctypes.data, nc.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"results failed ({rc}): " + self.eng.error())
        return s, it, nc

    def cigar(self, i: int, n_cigar: int) -> np.ndarray:
        out = np.zeros(max(1, n_cigar), dtype=np.uint32)
        rc = lib().mwf_gpu_batch_cigar(self.eng.h, self.h, i, out.ctypes.data, n_cigar)
        if rc < 0:
            raise RuntimeError(f"cigar download failed ({rc}): " + self.eng.error())
        return out[:rc]

    def alphabet(self) -> np.ndarray:
        """Per-pair alphabet class (int8: 0, 1, 2 as alphabet_class; with "alpha16" 1: 0, 1, 2, 3 as alphabet_class16) of the last align under "alpha_remap" 1; raises before the first align and
        when that align ran with the tunable off (mwf_gpu_batch_alphabet)."""
        out = np.zeros(max(1, self.n), dtype=np.int8)
        rc = lib().mwf_gpu_batch_alphabet(self.eng.h, self.h, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"alphabet failed ({rc}): " + self.eng.error())
        return out[:self.n]

    def dev_scores_ptr(self) -> int:
        return lib().mwf_gpu_batch_dev_scores(self.h)

    def dev_iters_ptr(self) -> int:
        return lib().mwf_gpu_batch_dev_iters(self.h)

    def dev_status_ptr(self) -> int:
        return lib().mwf_gpu_batch_dev_status(self.h)

    def fetch_cigars(self):
        """Bring every CIGAR of the batch to the host in one copy (cigar() then serves from it)."""
        rc = lib().mwf_gpu_batch_fetch_cigars(self.eng.h, self.h)
        if rc != 0:
            raise RuntimeError(f"CIGAR download failed ({rc}): " + self.eng.error())

    def dev_cigars(self):
        """(pool_ptr, off_ptr, n_words_ptr, pool_words): the device arrays of the last CIGAR-mode align, zero-copy (mwf_gpu_batch_dev_cigars).
        Pair i's words are pool[off[i] : off[i] + n_words[i]] (uint32 / int64 / int32); valid until the next align or free of the batch."""
        pool, off, nw, used = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = lib().mwf_gpu_batch_dev_cigars(self.eng.h, self.h, C.byref(pool), C.byref(off), C.byref(nw), C.byref(used))
        if rc != 0:
            raise RuntimeError(f"dev_cigars failed ({rc}): " + self.eng.error())
        return pool.value or 0, off.value or 0, nw.value or 0, used.value

    def summarize(self, opt: MwfOpt | None = None, cigars=None):
        """Enqueue the summary kernel (mwf_gpu_batch_summarize) and return; dev_summary_ptr() then points at the n records.  cigars: None for
        the batch's own CIGARs, or (words_ptr, off_ptr, n_words_ptr) device arrays of foreign ones (uint32 / int64 / int32)."""
        w, o, c = cigars if cigars is not None else (None, None, None)
        rc = lib().mwf_gpu_batch_summarize(self.eng.h, self.h, C.byref(opt) if opt is not None else None, w, o, c)
        if rc != 0:
            raise RuntimeError(f"summarize failed ({rc}): " + self.eng.error())

    def summary(self, opt: MwfOpt | None = None, cigars=None) -> np.ndarray:
        """summarize() + wait + copy: a structured array (SUMMARY_DTYPE) of n records."""
        self.summarize(opt, cigars)
        out = np.zeros(self.n, dtype=SUMMARY_DTYPE)
        rc = lib().mwf_gpu_batch_summary(self.eng.h, self.h, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"summary download failed ({rc}): " + self.eng.error())
        return out

    def dev_summary_ptr(self) -> int | None:
        """Device pointer to the records of the last summarize(); None before the first one and after a newer align."""
        return lib().mwf_gpu_batch_dev_summary(self.h)

    def map(self, which: int):
        """Enqueue the coordinate-map kernel (mwf_gpu_batch_map; which 0: query -> target, 1: target -> query) and return."""
        rc = lib().mwf_gpu_batch_map(self.eng.h, self.h, which)
        if rc != 0:
            raise RuntimeError(f"map failed ({rc}): " + self.eng.error())

    def coord_map(self, which: int):
        """map() + wait + copy -> (values[int32], offsets[int64, n + 1]): pair i's slice is values[offsets[i]:offsets[i + 1]] (include/miniwfa.h)."""
        self.map(which)
        off = np.zeros(self.n + 1, dtype=np.int64)
        rc = lib().mwf_gpu_batch_map_fetch(self.eng.h, self.h, which, None, off.ctypes.data)
        vals = np.zeros(int(off[-1]), dtype=np.int32)
        if rc == 0 and len(vals):
            rc = lib().mwf_gpu_batch_map_fetch(self.eng.h, self.h, which, vals.ctypes.data, None)
        if rc != 0:
            raise RuntimeError(f"map download failed ({rc}): " + self.eng.error())
        return vals, off

    def dev_map_ptr(self, which: int) -> int | None:
        """Device pointer to the map of the last map(which); None before the first one and after a newer align."""
        return lib().mwf_gpu_batch_dev_map(self.h, which)

    def text(self, kind: int, cigars=None):
        """Enqueue the text kernels (mwf_gpu_batch_text; kind: MWF_TXT_*) and return; dev_text(kind) then points at the text.  cigars: None for the
        batch's own CIGARs, or (words_ptr, off_ptr, n_words_ptr) device arrays of foreign ones, as in summarize()."""
        w, o, c = cigars if cigars is not None else (None, None, None)
        rc = lib().mwf_gpu_batch_text(self.eng.h, self.h, kind, w, o, c)
        if rc != 0:
            raise RuntimeError(f"text failed ({rc}): " + self.eng.error())

    def text_fetch(self, kind: int):
        """Wait for the last text(kind) and copy it -> (text[bytes], offsets[int64, n + 1]): pair i's text is text[offsets[i]:offsets[i + 1]]."""
        off = np.zeros(self.n + 1, dtype=np.int64)
        rc = lib().mwf_gpu_batch_text_fetch(self.eng.h, self.h, kind, None, off.ctypes.data)
        buf = np.zeros(max(1, int(off[-1])), dtype=np.uint8)
        if rc == 0 and off[-1] > 0:
            rc = lib().mwf_gpu_batch_text_fetch(self.eng.h, self.h, kind, buf.ctypes.data, None)
        if rc != 0:
            raise RuntimeError(f"text download failed ({rc}): " + self.eng.error())
        return buf.tobytes()[:int(off[-1])], off

    def texts(self, kind: int, cigars=None) -> list[bytes]:
        """text() + wait + copy: one bytes object per pair (empty for a pair without a CIGAR or with unrenderable words)."""
        self.text(kind, cigars)
        raw, off = self.text_fetch(kind)
        return [raw[off[i]:off[i + 1]] for i in range(self.n)]

    def dev_text(self, kind: int):
        """(text_ptr, off_ptr, total) of the last text(kind): pair i's text is the bytes [off[i], off[i + 1]) from text_ptr on, off int64[n + 1] on the
        device, total = off[n]; None before the first text(kind) and after a newer align."""
        off, total = C.c_void_p(), C.c_int64()
        p = lib().mwf_gpu_batch_dev_text(self.h, kind, C.byref(off), C.byref(total))
        return (p, off.value or 0, total.value) if p else None

    def work_sketch(self) -> np.ndarray:
        """hits[i]: 8-mers of pair i's query that occur in its target — the per-pair work estimate the band classes are dealt by (test hook)."""
        out = np.zeros(max(1, self.n), dtype=np.int32)
        if lib().mwf_gpu_test_pair_sketch(self.eng.h, self.h, out.ctypes.data) != 0:
            raise RuntimeError("pair sketch failed: " + self.eng.error())
        return out[:self.n]

    def debug_band(self, opt: MwfOpt, pair: int, cap: int = 1 << 20):
        """[(lo, hi)] in DIAGONAL coordinates of every slice the core pass opened for `pair` (diagnostics)."""
        buf = np.zeros(2 * cap, dtype=np.int32)
        n = lib().mwf_gpu_debug_band(self.eng.h, self.h, C.byref(opt), pair, buf.ctypes.data, cap)
        if n < 0:
            raise RuntimeError(f"debug_band failed ({n}): " + self.eng.error())
        return buf[:2 * n].reshape(-1, 2)
