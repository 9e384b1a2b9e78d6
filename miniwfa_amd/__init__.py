"""miniwfa_amd — MI355X (gfx950) implementation of lh3/miniwfa's exact WFA score-and-CIGAR path.

The product is the C-ABI shared library ``miniwfa_amd/csrc/libmwf_hip.so`` (headers in
``include/``); this package is the thin Python host side over it (``miniwfa_amd.api``) plus the
synthetic-pair generator the tests and the benchmark share (``miniwfa_amd.synth``).
"""
from .api import (MWF_F_CIGAR, MWF_F_DEBUG, MWF_F_NO_KALLOC, Batch, Engine, MwfOpt, MwfRst, cigar2score, cigar_str,
                  lib, opt_init, wfa_auto, wfa_batch, wfa_batch_multi, wfa_chain, wfa_chain_batch, wfa_auto_batch, wfa_exact, wfa_submit, async_stats, Job,
                  AlnSummary, SUMMARY_DTYPE, DevArray, cigar_summary, alphabet_class, alphabet_class16, cigar_text,
                  MWF_TXT_CIGAR, MWF_TXT_SAM, MWF_TXT_CS, MWF_TXT_MD, MWF_TXT_ROW_T, MWF_TXT_ROW_Q, MWF_TXT_KINDS,
                  MwfEnds, ENDS_FREE, wfa_ends, wfa_ends_batch,
                  MwfExt, MWF_EXT_END, MWF_EXT_DROP, wfa_ext, wfa_ext_batch,
                  MwfBand, wfa_ends_pp_batch, wfa_ext_band_batch)

__all__ = ["MWF_F_CIGAR", "MWF_F_DEBUG", "MWF_F_NO_KALLOC", "Batch", "Engine", "MwfOpt", "MwfRst", "cigar2score",
           "cigar_str", "lib", "opt_init", "wfa_auto", "wfa_batch", "wfa_batch_multi", "wfa_chain", "wfa_chain_batch", "wfa_auto_batch", "wfa_exact", "wfa_submit", "async_stats", "Job",
           "AlnSummary", "SUMMARY_DTYPE", "DevArray", "cigar_summary", "alphabet_class", "alphabet_class16", "cigar_text",
           "MWF_TXT_CIGAR", "MWF_TXT_SAM", "MWF_TXT_CS", "MWF_TXT_MD", "MWF_TXT_ROW_T", "MWF_TXT_ROW_Q", "MWF_TXT_KINDS",
           "MwfEnds", "ENDS_FREE", "wfa_ends", "wfa_ends_batch",
           "MwfExt", "MWF_EXT_END", "MWF_EXT_DROP", "wfa_ext", "wfa_ext_batch",
           "MwfBand", "wfa_ends_pp_batch", "wfa_ext_band_batch"]
