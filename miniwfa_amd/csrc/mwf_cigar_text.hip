// mwf_cigar_text.hip — the CIGARs of a batch as text, on the device (gfx950, wave64): the six products of include/miniwfa.h (MWF_TXT_*: CIGAR
// string, SAM M-form, cs tag, MD tag, the two gapped rows).  Off the align path: nothing here runs unless mwf_gpu_batch_text is called.
//
// A variable-length byte emitter in two launches of ONE kernel template (MODE 0 sizes, MODE 1 writes: the same walk decides both, so sizes and
// writes cannot disagree) with a one-workgroup scan between them that turns the per-pair lengths into offsets.  One workgroup per pair, no
// global atomics, plain vector stores.  The workgroup walks the pair's words in passes of one word per thread (a coalesced load), like
// mwf_cigar_ops.hip:
//   1. the (target, query) lengths the words consume are prefix-summed in 64 bits on top of a 64-bit carry: every word knows its (ti, qj); a
//      word is fine when its op is known, its length >= 1 and it ends inside both sequences — any other word makes the pair unrenderable
//      (empty text) and contributes no byte, so whatever the words claim no access leaves the pair's sequences;
//   2. the numbers that span words — SAM's <sum>M over a run of = / X words, MD's count of bases under = since the last X / D — come from a
//      SEGMENTED scan in the same step (a breaker word resets the sum), on top of a 64-bit carry of the open run / count: a run or a count
//      that spans a pass boundary comes out as one number;
//   3. every word's number of output bytes follows (digits of its number, its bases), is prefix-summed too, and — MODE 1 — the bytes of the
//      pass are spread over the LANES, not over the words: consecutive threads take consecutive output bytes and find their word by binary
//      search in LDS.  `5000I` is 5000 byte stores by the whole workgroup, consecutive lanes storing consecutive bytes.  Every store is
//      clipped to the pair's slice txt[off[i], off[i + 1]).
// Geometry: cigar_ops_block() (mwf_cigar_ops.hip) — 64 threads up to 2048 bases, 256 up to 65 536, 1024 beyond.
#include <hip/hip_runtime.h>
#include "miniwfa.h"
#include "mwf_internal.h"

namespace mwf {
namespace {

__device__ __forceinline__ int64_t wave_scan64(int64_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int64_t o = __shfl_up((long long)v, d, 64);
		if (lane >= d) v += o;
	}
	return v;
}

// inclusive segmented sum: f = a breaker lies at or before this lane (inside the wave), v = the sum since the last breaker (a breaker itself holds 0)
__device__ __forceinline__ void wave_seg_scan64(int &f, int64_t &v, int lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int of = __shfl_up(f, d, 64);
		const int64_t ov = __shfl_up((long long)v, d, 64);
		if (lane >= d) {
			if (!f) v += ov;
			f |= of;
		}
	}
}

__device__ __forceinline__ int n_digits(uint32_t v)
{
	return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

__device__ const uint32_t kPow10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};

// digit p (0: the leftmost) of v, which has nd digits
__device__ __forceinline__ uint8_t digit_at(uint32_t v, int nd, int p) { return (uint8_t)('0' + (v / kPow10[nd - 1 - p]) % 10u); }

__device__ __forceinline__ uint8_t cs_lower(uint8_t b) { return b >= 'A' && b <= 'Z' ? (uint8_t)(b | 0x20) : b; }

__device__ __forceinline__ uint32_t clamp_u32(int64_t v) { return v > 0xffffffffll ? 0xffffffffu : (uint32_t)v; } // (beyond 2^32 the pair is unrenderable anyway: its sums pass a sequence length)

// MODE 0: off[1 + pair] = the length of the pair's text; 1: write it to txt[off[pair], off[pair + 1]).  B threads, one pair.
template <int B, int MODE>
__global__ __launch_bounds__(B) void cigar_text_kernel(CigarTextArgs A)
{
	constexpr int NW = B / 64;
	constexpr int COMBINE_UNROLL = NW > 4 ? 1 : NW; // (sixteen waves unrolled would not fit the 128 registers of a 1024-thread workgroup)
	__shared__ int64_t s_cstart[B]; // output bytes of this pass before word k of the pass
	__shared__ int32_t s_ti[B], s_qj[B]; // where word k starts (only read for a word that is fine: inside its sequences, so 32 bits hold it)
	__shared__ uint32_t s_word[B], s_val[B]; // the word; the number it prints (its length, SAM: the run's sum, MD: the open count)
	__shared__ int64_t s_wt[NW], s_wq[NW], s_wv[NW], s_wc[NW];
	__shared__ int32_t s_wf[NW];
	__shared__ int32_t s_bad;

	const int32_t pair = (int32_t)blockIdx.x;
	const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int kind = A.kind;
	const int32_t tl = A.tl[pair], ql = A.ql[pair];
	int32_t nw = A.n_words[pair];
	// the batch's own CIGARs: a pair has one when the align finished it; foreign ones: when it has words
	const bool has = A.status ? A.status[pair] == ST_OK : nw > 0;
	if (nw < 0) nw = 0;
	int64_t out0 = 0, out_end = 0;
	if (MODE == 0) {
		if (!has) {
			if (tid == 0) A.off[1 + (int64_t)pair] = 0;
			return;
		}
	} else {
		out0 = A.off[pair], out_end = A.off[1 + (int64_t)pair];
		if (!has || out_end <= out0) return; // (no text: stopped, no words, unrenderable — the sizing launch said so)
	}
	const uint8_t *t = A.seqs + A.t_off[pair], *q = A.seqs + A.q_off[pair];
	const uint32_t *words = A.words + A.word_off[pair];
	uint8_t *txt = (uint8_t*)A.txt;
	int64_t ct = 0, cq = 0; // carries (the same in every thread): bases consumed by the passes so far,
	int64_t cc = 0;         // ... SAM's open M run / MD's open count,
	int64_t opos = 0;       // ... and the bytes of text so far
	if (tid == 0) s_bad = 0;
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
		// what is counted across words, and which words reset the count
		int64_t sv = 0;
		int sf = 0;
		if (kind == MWF_TXT_SAM) sv = both ? len : 0, sf = (on_t || on_q) && !both;
		else if (kind == MWF_TXT_MD) sv = in && op == 7 ? len : 0, sf = in && (op == 8 || op == 2);
		// 1. + 2. start positions, and the count that is open in front of this word
		const int64_t it = wave_scan64(dt, lane), iq = wave_scan64(dq, lane);
		wave_seg_scan64(sf, sv, lane);
		if (lane == 63) s_wt[wave] = it, s_wq[wave] = iq, s_wf[wave] = sf, s_wv[wave] = sv;
		int xf = __shfl_up(sf, 1, 64); // exclusive: what lies in front of this lane
		int64_t xv = __shfl_up((long long)sv, 1, 64);
		if (lane == 0) xf = 0, xv = 0;
		__syncthreads();
		int64_t ti = ct + it - dt, qj = cq + iq - dq;
		int pf = 0, af = 0; // the waves in front of this one / all waves, folded left to right
		int64_t pv = 0, av = 0;
#pragma unroll COMBINE_UNROLL
		for (int v = 0; v < NW; ++v) {
			const int64_t a = s_wt[v], b = s_wq[v], wv = s_wv[v];
			const int wf = s_wf[v];
			if (v < wave) ti += a, qj += b;
			ct += a, cq += b;
			if (v == wave) pf = af, pv = av;
			av = wf ? wv : av + wv, af |= wf;
		}
		int64_t c = xf ? xv : (pf ? pv + xv : cc + pv + xv); // the open count in front of this word
		cc = af ? av : cc + av;
		// a word is fine when its op is known, its length >= 1 and it ends inside both sequences
		const bool ok = (on_t || on_q) && len >= 1 && (!on_t || ti + len <= tl) && (!on_q || qj + len <= ql);
		if (in && !ok) s_bad = 1;
		// 3. the bytes this word prints
		uint32_t val = (uint32_t)len;
		int64_t osz = 0;
		if (ok) {
			switch (kind) {
			case MWF_TXT_CIGAR: osz = n_digits(val) + 1; break;
			case MWF_TXT_SAM:
				if (both) {
					const int nop = w + 1 < nw ? (int)(words[w + 1] & 0xfu) : 0;
					val = clamp_u32(c + len);
					osz = nop == 7 || nop == 8 ? 0 : n_digits(val) + 1; // the last word of its run prints the run
				} else osz = n_digits(val) + 1;
				break;
			case MWF_TXT_CS: osz = op == 7 ? 1 + n_digits(val) : op == 8 ? 3 * len : 1 + len; break;
			case MWF_TXT_MD:
				val = clamp_u32(c);
				osz = op == 8 ? n_digits(val) + 1 + 2 * (len - 1) : op == 2 ? n_digits(val) + 1 + len : 0; // (the bases of an X word behind its first: "0" and the byte)
				break;
			case MWF_TXT_ROW_T: case MWF_TXT_ROW_Q: osz = len; break;
			default: break;
			}
		}
		const int64_t ic = wave_scan64(osz, lane);
		if (lane == 63) s_wc[wave] = ic;
		if (MODE == 1) s_cstart[tid] = ic - osz, s_ti[tid] = (int32_t)ti, s_qj[tid] = (int32_t)qj, s_word[tid] = word, s_val[tid] = val;
		__syncthreads();
		if (s_bad) break; // (uniform: every store to s_bad lies before the barrier)
		int64_t before = 0, total = 0;
#pragma unroll COMBINE_UNROLL
		for (int v = 0; v < NW; ++v) {
			const int64_t a = s_wc[v];
			if (v < wave) before += a;
			total += a;
		}
		if (MODE == 1) {
			s_cstart[tid] += before;
			__syncthreads();
			const int32_t cnt = min((int32_t)B, nw - base);
			for (int64_t u = tid; u < total; u += B) {
				int32_t lo = 0, hi = cnt; // the last word k of the pass with s_cstart[k] <= u: the one byte u belongs to (a word without bytes shares its start with its successor, which wins)
				while (hi - lo > 1) {
					const int32_t mid = (lo + hi) >> 1;
					if (s_cstart[mid] <= u) lo = mid; else hi = mid;
				}
				const int64_t pos = out0 + opos + u;
				if (pos >= out_end) continue; // (clipped to the pair's slice)
				const int64_t o = u - s_cstart[lo];
				const int64_t wt = s_ti[lo], wq = s_qj[lo];
				const uint32_t wword = s_word[lo], wval = s_val[lo];
				const int wop = (int)(wword & 0xfu);
				const int nd = n_digits(wval);
				uint8_t byte;
				switch (kind) {
				case MWF_TXT_CIGAR: byte = o < nd ? digit_at(wval, nd, (int)o) : (uint8_t)(wop == 7 ? '=' : wop == 8 ? 'X' : wop == 1 ? 'I' : 'D'); break;
				case MWF_TXT_SAM: byte = o < nd ? digit_at(wval, nd, (int)o) : (uint8_t)(wop == 1 ? 'I' : wop == 2 ? 'D' : 'M'); break;
				case MWF_TXT_CS:
					if (wop == 7) byte = o == 0 ? (uint8_t)':' : digit_at(wval, nd, (int)o - 1);
					else if (wop == 8) {
						const int64_t k = (int64_t)((uint32_t)o / 3u); // (o < 3 len < 2^32)
						const int r = (int)(o - 3 * k);
						byte = r == 0 ? (uint8_t)'*' : cs_lower(r == 1 ? t[wt + k] : q[wq + k]);
					} else byte = o == 0 ? (uint8_t)(wop == 1 ? '+' : '-') : cs_lower(wop == 1 ? q[wq + o - 1] : t[wt + o - 1]);
					break;
				case MWF_TXT_MD:
					if (o < nd) byte = digit_at(wval, nd, (int)o);
					else if (wop == 2) byte = o == nd ? (uint8_t)'^' : t[wt + o - nd - 1];
					else {
						const int64_t r = o - nd; // even: the byte of base r / 2; odd: the "0" in front of base (r + 1) / 2
						byte = r & 1 ? (uint8_t)'0' : t[wt + (r >> 1)];
					}
					break;
				case MWF_TXT_ROW_T: byte = wop == 1 ? (uint8_t)'-' : t[wt + o]; break;
				default:            byte = wop == 2 ? (uint8_t)'-' : q[wq + o]; break;
				}
				txt[pos] = byte;
			}
		}
		opos += total;
		__syncthreads(); // (the next pass overwrites the tables)
	}
	const bool good = !s_bad && ct == tl && cq == ql;
	const uint32_t cend = clamp_u32(cc);
	const int nd_end = kind == MWF_TXT_MD ? n_digits(cend) : 0; // MD ends with the open count
	if (MODE == 0) {
		if (tid == 0) A.off[1 + (int64_t)pair] = good ? opos + nd_end : 0;
	} else if (good && tid < nd_end && out0 + opos + tid < out_end) txt[out0 + opos + tid] = digit_at(cend, nd_end, tid);
}

// off[1 .. n] holds the lengths; afterwards off[0 .. n] holds the offsets (off[0] = 0, off[i + 1] = off[i] + length i).  One workgroup.
__global__ __launch_bounds__(1024) void text_scan_kernel(int64_t *off, int32_t n)
{
	__shared__ int64_t s_w[16];
	const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
	int64_t carry = 0;
	if (tid == 0) off[0] = 0;
	for (int32_t base = 0; base < n; base += 1024) {
		const int32_t i = base + tid;
		const int64_t v = i < n ? off[1 + (int64_t)i] : 0;
		const int64_t inc = wave_scan64(v, lane);
		if (lane == 63) s_w[wave] = inc;
		__syncthreads();
		int64_t before = 0, total = 0;
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const int64_t a = s_w[k];
			if (k < wave) before += a;
			total += a;
		}
		if (i < n) off[1 + (int64_t)i] = carry + before + inc;
		carry += total;
		__syncthreads();
	}
}

template <int B>
int launch_as(const CigarTextArgs &a, hipStream_t st)
{
	const dim3 grid((unsigned)a.n_pairs), block(B);
	if (a.mode == 0) hipLaunchKernelGGL((cigar_text_kernel<B, 0>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((cigar_text_kernel<B, 1>), grid, block, 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace

int launch_cigar_text(const CigarTextArgs &a, int block, void *stream)
{
	if (a.n_pairs <= 0) return 0;
	if (a.kind < 0 || a.kind >= MWF_TXT_KINDS || a.mode < 0 || a.mode > 1) return -1;
	switch (block) {
	case 64:   return launch_as<64>(a, (hipStream_t)stream);
	case 256:  return launch_as<256>(a, (hipStream_t)stream);
	case 1024: return launch_as<1024>(a, (hipStream_t)stream);
	default: return -1;
	}
}

int launch_text_scan(int64_t *off, int32_t n, void *stream)
{
	hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, off, n);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace mwf
