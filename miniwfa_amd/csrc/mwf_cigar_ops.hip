// mwf_cigar_ops.hip — what a caller derives from the CIGARs of a batch, on the device (gfx950, wave64): the per-pair summary
// and self-check (mwf_aln_summary_t, include/miniwfa.h: counters, score, first_bad) and the dense coordinate maps
// (query -> target, target -> query).  Off the align path: nothing here runs unless mwf_gpu_batch_summarize / _map is called.
//
// One launch per product, one workgroup per pair, no global atomics.  The workgroup walks the pair's words in passes of one word per
// thread (a coalesced load):
//   1. the (target, query) lengths the words consume are prefix-summed in 64 bits — shuffles inside a wave, the waves' totals through
//      LDS — on top of a 64-bit carry from the previous pass: every word knows where it starts, (ti, qj);
//   2. rules (a) and (b) of first_bad (unknown op, a word that runs past a sequence) are per-word tests on those positions; the per-op
//      counters and the score are per-thread sums (modulo 2^32: what truncating the 64-bit sums on store gives), reduced once per pair;
//   3. the bases are spread over the LANES, not over the words: the in-range bases of the pass's words are prefix-summed too, the
//      starts go to LDS, and consecutive threads take consecutive bases of that numbering and find their word by binary search in
//      LDS.  `5000=` is 5000 units of work like 1000 words of 5 bases are, and the byte loads from t / q (rule (c)) and the int32
//      stores to a map are consecutive across a wave inside a word.  A unit exists only for a base INSIDE its sequence, so whatever
//      the words claim, no access leaves [t_off, t_off + tl) / [q_off, q_off + ql) or the pair's slice of the map.
// first_bad is an LDS atomicMin over the workgroup.
// Geometry: the host picks the workgroup size for the launch from the longest pair of the batch (launch_cigar_ops below): one wave
// per pair for reads, 256 threads for pairs of kilobases, 1024 for a pair the whole-device kernel aligned.  One size per launch: a
// batch of reads with a single long pair in it runs every read at the long pair's size (DESIGN.md states the cost).
#include <hip/hip_runtime.h>
#include "mwf_internal.h"

namespace mwf {
namespace {

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ int64_t wave_scan64(int64_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int64_t o = __shfl_up((long long)v, d, 64);
		if (lane >= d) v += o;
	}
	return v;
}

__device__ __forceinline__ int32_t wave_scan32(int32_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int32_t o = __shfl_up(v, d, 64);
		if (lane >= d) v += o;
	}
	return v;
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int32_t)v, d, 64);
	return v;
}

// MODE 0: summary; 1: map query -> target; 2: map target -> query.  B threads, one pair.
template <int B, int MODE>
__global__ __launch_bounds__(B) void cigar_ops_kernel(CigarOpsArgs A)
{
	constexpr int NW = B / 64;
	__shared__ int32_t s_cstart[B]; // units (bases this pass works on) before word k of the pass
	// where word k starts, low 32 bits.  Exact on a sequence the word has a unit on (the unit lies inside it).  The OTHER sequence's start —
	// the partner index wt + off of a map entry, the t_next / q_next of an I / D code — is exact only while that start fits 32 bits too: true
	// for a valid CIGAR of the pair (both starts <= tl, ql), which the batch's own are and which is all the map modes are given.  Foreign
	// words (summary mode only) never use the other sequence's value; wiring them into a map needs 64-bit starts or a clamp here first.
	__shared__ int32_t s_ti[B], s_qj[B];
	__shared__ uint32_t s_word[B];
	__shared__ int64_t s_wt[NW], s_wq[NW];
	__shared__ int32_t s_wc[NW];
	__shared__ int32_t s_bad;
	__shared__ uint32_t s_acc[7];

	const int32_t pair = (int32_t)blockIdx.x;
	const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int32_t tl = A.tl[pair], ql = A.ql[pair];
	int32_t nw = A.n_words[pair];
	// the batch's own CIGARs: a pair has one when the align finished it; foreign ones: when it has words
	const bool has = A.status ? A.status[pair] == ST_OK : nw > 0;
	if (nw < 0) nw = 0;
	if (!has) {
		if (MODE == 0) {
			if (tid < 12) A.summary[(int64_t)pair * 12 + tid] = tid == 10 ? -1 : 0;
		} else {
			const int32_t span = MODE == 1 ? ql : tl;
			int32_t *m = A.map + A.map_off[pair];
			for (int32_t j = tid; j < span; j += B) m[j] = INT32_MIN;
		}
		return;
	}
	const uint8_t *t = A.seqs + A.t_off[pair], *q = A.seqs + A.q_off[pair];
	const uint32_t *words = A.words + A.word_off[pair];
	int32_t *map = MODE == 0 ? nullptr : A.map + A.map_off[pair];
	int64_t ct = 0, cq = 0; // carry: bases consumed by the passes so far (the same in every thread)
	uint32_t acc[7] = {0, 0, 0, 0, 0, 0, 0}; // score, n_eq, n_x, n_ins, n_del, n_ins_runs, n_del_runs
	if (tid == 0) s_bad = INT32_MAX;
	if (tid < 7) s_acc[tid] = 0;
	__syncthreads();

	for (int32_t base = 0; base < nw; base += B) {
		const int32_t w = base + tid;
		const bool in = w < nw;
		const uint32_t word = in ? words[w] : 0u;
		const int op = (int)(word & 0xfu);
		const int64_t len = (int64_t)(word >> 4);
		const bool both = in && (op == 7 || op == 8);
		const bool on_t = both || (in && op == 2), on_q = both || (in && op == 1);
		const int64_t dt = on_t ? len : 0, dq = on_q ? len : 0;
		if (MODE == 0 && in) {
			if (op == 1 || op == 2) {
				const int64_t p1 = A.o1 + len * A.e1, p2 = A.o2 + len * A.e2;
				acc[0] += (uint32_t)(p1 < p2 ? p1 : p2);
				acc[3] += op == 1 ? (uint32_t)len : 0u, acc[4] += op == 2 ? (uint32_t)len : 0u;
				acc[5] += op == 1 ? 1u : 0u, acc[6] += op == 2 ? 1u : 0u;
			} else if (op == 8) acc[0] += (uint32_t)(len * A.x), acc[2] += (uint32_t)len;
			else if (op == 7) acc[1] += (uint32_t)len;
		}
		// 1. start positions
		const int64_t it = wave_scan64(dt, lane), iq = wave_scan64(dq, lane);
		if (lane == 63) s_wt[wave] = it, s_wq[wave] = iq;
		__syncthreads();
		int64_t ti = ct + it - dt, qj = cq + iq - dq;
#pragma unroll
		for (int v = 0; v < NW; ++v) {
			const int64_t a = s_wt[v], b = s_wq[v];
			if (v < wave) ti += a, qj += b;
			ct += a, cq += b;
		}
		// 2. rules (a) and (b)
		if (MODE == 0 && in && (!(on_t || on_q) || (on_t && ti + len > tl) || (on_q && qj + len > ql))) atomicMin(&s_bad, w);
		// 3. the bases of this pass that lie inside their sequence(s), numbered across the words
		const int64_t room_t = ti < tl ? tl - ti : 0, room_q = qj < ql ? ql - qj : 0;
		int64_t c64 = 0;
		if (MODE == 0) { if (both) c64 = min64(len, min64(room_t, room_q)); }
		else if (MODE == 1) { if (on_q) c64 = min64(len, room_q); }
		else { if (on_t) c64 = min64(len, room_t); }
		const int32_t c = (int32_t)c64; // (at most a sequence length; the units of a pass are disjoint stretches of one sequence: their sum fits too)
		const int32_t ic = wave_scan32(c, lane);
		if (lane == 63) s_wc[wave] = ic;
		__syncthreads();
		int32_t before = 0, total = 0;
#pragma unroll
		for (int v = 0; v < NW; ++v) {
			const int32_t a = s_wc[v];
			if (v < wave) before += a;
			total += a;
		}
		s_cstart[tid] = before + ic - c;
		s_ti[tid] = (int32_t)ti, s_qj[tid] = (int32_t)qj, s_word[tid] = word;
		__syncthreads();
		const int32_t cnt = min((int32_t)B, nw - base);
		for (int32_t u = tid; u < total; u += B) {
			int32_t lo = 0, hi = cnt; // the last word k of the pass with s_cstart[k] <= u: the one unit u belongs to (a word without units shares its start with its successor, which wins)
			while (hi - lo > 1) {
				const int32_t mid = (lo + hi) >> 1;
				if (s_cstart[mid] <= u) lo = mid; else hi = mid;
			}
			const int32_t off = u - s_cstart[lo], wt = s_ti[lo], wq = s_qj[lo];
			const int wop = (int)(s_word[lo] & 0xfu);
			if (MODE == 0) {
				const bool eq = t[(int64_t)wt + off] == q[(int64_t)wq + off];
				if (eq != (wop == 7)) atomicMin(&s_bad, base + lo); // rule (c)
			} else if (MODE == 1) map[wq + off] = wop == 1 ? -1 - wt : wt + off;
			else map[wt + off] = wop == 2 ? -1 - wq : wq + off;
		}
		__syncthreads(); // (the next pass overwrites the tables)
	}
	if (MODE == 0) {
#pragma unroll
		for (int k = 0; k < 7; ++k) {
			const uint32_t s = wave_sum32(acc[k]);
			if (lane == 0 && s) atomicAdd(&s_acc[k], s);
		}
		__syncthreads();
		if (tid == 0) {
			int32_t *o = A.summary + (int64_t)pair * 12;
			const int32_t bad = s_bad;
			o[0] = (int32_t)s_acc[0];
			o[1] = (int32_t)(uint32_t)(uint64_t)ct, o[2] = (int32_t)(uint32_t)(uint64_t)cq;
			o[3] = (int32_t)s_acc[1], o[4] = (int32_t)s_acc[2], o[5] = (int32_t)s_acc[3], o[6] = (int32_t)s_acc[4];
			o[7] = (int32_t)s_acc[5], o[8] = (int32_t)s_acc[6];
			o[9] = nw;
			o[10] = bad != INT32_MAX ? bad : (ct != tl || cq != ql) ? nw : -1;
			o[11] = 1;
		}
	}
}

template <int B>
int launch_as(const CigarOpsArgs &a, hipStream_t st)
{
	const dim3 grid((unsigned)a.n_pairs), block(B);
	if (a.mode == 0) hipLaunchKernelGGL((cigar_ops_kernel<B, 0>), grid, block, 0, st, a);
	else if (a.mode == 1) hipLaunchKernelGGL((cigar_ops_kernel<B, 1>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((cigar_ops_kernel<B, 2>), grid, block, 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace

// Threads per pair from the longest pair (target + query bases) of the batch.  A wave per pair serves reads (a 150 bp read has a handful of
// words and 150 bases: one pass, three rounds of bases); from 2 kb on a wave would walk tens of rounds per pass where four waves share them;
// a pair of the whole-device kernel's range (>= 64 kb) has the device to itself or nearly: the largest workgroup.
int cigar_ops_block(int64_t max_len) { return max_len <= 2048 ? 64 : max_len <= 65536 ? 256 : 1024; }

int launch_cigar_ops(const CigarOpsArgs &a, int block, void *stream)
{
	if (a.n_pairs <= 0) return 0;
	switch (block) {
	case 64:   return launch_as<64>(a, (hipStream_t)stream);
	case 256:  return launch_as<256>(a, (hipStream_t)stream);
	case 1024: return launch_as<1024>(a, (hipStream_t)stream);
	default: return -1;
	}
}

} // namespace mwf
