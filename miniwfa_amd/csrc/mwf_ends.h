// mwf_ends.h — what the host side (mwf_plan.cpp) and the ends-free kernel (mwf_ends.hip) share: the kernel's argument block and its launch
// wrappers.  The semantics of an ends-free alignment are stated in include/miniwfa.h (mwf_ends_t); nothing here is part of the public ABI.
#pragma once
#include <stdint.h>
#include "mwf_internal.h"

namespace mwf {

// wfa_ends_kernel<T, EXT> takes the generic kernel's arguments as they are (workspace, options, per-pair outputs: one workgroup per pair on
// the engine's ring pool and traceback arena) plus the allowances and the outputs only an ends-free alignment has.
struct EndsArgs {
	BatchArgs b;               // first: the device helpers of mwf_device.h read it as the generic kernel's (b.step is 0: no low-memory mode here)
	int32_t t_beg, t_end, q_beg, q_end; // mwf_ends_t, each >= 0; clamped to the pair's lengths on the device
	int32_t *out_range;        // [pair][4] = {tb, te, qb, qe}, half-open; -1 where not known (stopped pair: all four; score-only: tb and qb)
	// the aligned sub-ranges as a batch geometry of their own (what mwf_cigar_ops.hip / mwf_cigar_text.hip read after an ends-free CIGAR align)
	int64_t *sub_t_off, *sub_q_off; // [pair] t_off + tb, q_off + qb
	int32_t *sub_tl, *sub_ql;       // [pair] te - tb, qe - qb
	// extension alignment (mwf_ext_t): the EXT form of the kernel; the allowances are then {0, INT32_MAX, 0, INT32_MAX}
	int32_t ext;               // 0: ends-free, 1: extension
	int32_t match, zdrop;      // mwf_ext_t: A >= 1; Z >= 0, or -1 for no drop rule
	int32_t *out_info;         // [pair][4] = {V, s_stop, why, F}; all -1 for a stopped pair
	// per-pair parameters (mwf_gpu_batch_align_ends_pp / _ext_band), both null for the calls that have one set per batch
	const int32_t *pp_ends;    // [pair][4] = {t_beg, t_end, q_beg, q_end}, each >= 0: read instead of the four scalars above
	const int32_t *pp_band;    // [pair][2] = {d_lo, d_hi}, mwf_band_t: the pass stays on these diagonals; null: no band
};

// launch wrappers implemented in mwf_ends.hip; block: 256 or 512
int launch_ends(const EndsArgs &a, int grid, int block, void *stream);
int ends_kernel_occupancy(int block, bool ext); // resident workgroups per CU

} // namespace mwf
