// mwf_band2_kernel.h — the packed band kernel's template: the fast path for batches of pairs whose offsets fit 16 bits (targets below
// ~32 kb: BASELINE configs[2], read-length batches, chain-mode gap fills).  Seven units include it (through mwf_band2_dispatch.h) and say which
// instantiations they hold: mwf_band2.hip, mwf_band2_tab.hip, _nib, _e3, _e4, _bi, _bi_deep — and an eighth, mwf_band2_tab2.hip, the table form's second fold.  A unit picks the kernel's form by setting MWF_BAND2_FORM first.
//
// One workgroup per pair, a wave owns 256-column chunks (four columns per lane, K chunk slots per wave), E/F wavefronts in
// registers, one barrier per penalty; reference loops miniwfa.c:261-308 and :212-226, driver :397-426.  What makes it fast
// (DESIGN.md section 4.2 has the measurements):
//   * two columns per instruction: a lane's columns c0..c3 live in two registers (c0,c2) and (c1,c3) — the 16-bit H rows in HBM
//     hold a quad in that order — and the recurrence, the validity / room arithmetic of the match extension, the good bits and the
//     traceback byte are v_pk_* instructions on those pairs; neighbouring columns come from one DPP shift + one v_alignbit;
//   * rows read as DEAD beyond the window they were computed for (columns outside the window are stored dead, the chunk on either
//     side of the window is stored dead every penalty), so no read is ever masked and no window history is consulted;
//   * the sequence copy (2 bits per base, or bytes) starts at LDS address 0; the first probe of the match extension looks at 16
//     bases (8 bytes), its eight LDS reads are issued together; longer runs are walked per lane, then by the whole wave;
//   * kernel arguments are read from the kernarg segment where they are used (no SGPR spills from holding them for ever), the edge
//     table between neighbouring waves is addressed by immediates and written without exec masks, register histories are aged by
//     v_swap, the three per-penalty flags travel as one LDS word, rows are loaded only for chunks that are active.
// Results are bit-identical to the other kernels (tests/test_gpu_parity.py).
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "mwf_device.h"

// The form of the kernel a unit compiles: 0 plain, 1 table (mwf_band2_tab.hip), 2 four-bit (mwf_band2_nib.hip), 3 table with the second gap piece folded
// (mwf_band2_tab2.hip).  kTabProbe, kNib, kFold2Form and the kernel's name follow from it.
#ifndef MWF_BAND2_FORM
#define MWF_BAND2_FORM 0
#endif
#if MWF_BAND2_FORM == 1
#define MWF_BAND2_KERNEL wfa_band2_tab_kernel
#elif MWF_BAND2_FORM == 2
#define MWF_BAND2_KERNEL wfa_band2_nib_kernel
#elif MWF_BAND2_FORM == 3
#define MWF_BAND2_KERNEL wfa_band2_tab2_kernel
#else
#define MWF_BAND2_KERNEL wfa_band2_kernel
#endif

namespace mwf {

using namespace dev;

namespace {

extern __shared__ __attribute__((aligned(16))) uint8_t lds2[];

// Geometry constants (round 6: plain constants — rounds 3-5 overrode them with -D for experiments whose results are in profiles/HISTORY.md and the comments here;
// the experiment switches MWF_B2_XPREF / MWF_B2_MERGE_OFF / MWF_B2_NOPRIO and their dead branches are gone, see profiles/experiments/).
constexpr int kWideT = 512, kWideK = 3; // threads x chunk slots per wave of the widest two-per-CU geometry (24 chunks): 512 x 3; measured: 256 x 6 equal, 384 x 4 slower
constexpr int kWaves768 = 1;            // waves per SIMD the 768-thread geometry is compiled for (one workgroup per CU, up to 168 VGPRs; two per CU at 80 VGPRs: slower)
// chunk slots per wave of the 1024-thread geometry (16 waves, one workgroup per CU): 80 chunks = windows of up to 20 224 columns.  Measured on
// 1250 x 50 kb @ 3 % (windows of up to 16 900 columns): 4 slots 172 ms + 24 pairs re-run on the generic kernel = 240 ms, 5 slots (4 spilled VGPRs)
// 174.6 ms and no re-run, 6 slots (12 spilled) 177.0; 256 x 50 kb: 36.2 (+ 9 re-runs: 104) / 38.7 / 39.6 ms; generic kernel 279 and 78 ms.
constexpr int kSpanK = 5;
// Chunk slots per wave of the 512-thread geometry's copies on biased offsets (class 14 of mwf_plan.cpp: pairs of ~11-21 kb, two per CU instead of the span
// geometry's one).  Measured (ms per align; span geometry | 4 | 5 | 6 slots): 1024 x 12 kb @ 5 % 34.9 | 24.6 | 24.8 | 27.7, 1024 x 15 kb @ 4 % 35.6 | - | 25.1 | 25.7,
// 1024 x 17 kb @ 3 % 29.5 | - | 20.2 | 20.5, 512 x 18 kb @ 5 % 32.1 | - | - | 25.3, 1024 x 20 kb @ 3 % 37.3 | - | - | 26.9: five slots (40 chunks, 4 spilled VGPRs)
// while target + query stay below 3.5 of their span, six (48 chunks) up to 3.5 of theirs.  (Those are the default set's figures.  The other sets' copies — same slot
// counts, mwf_band2_bi.hip / mwf_band2_bi_deep.hip — against the span geometry: DESIGN.md section 4.2, profiles/band_biased/.)
constexpr int kW4K = 5;
constexpr int kSpanT = 1024;  // threads of the span geometry (measured: 768 x 7 slots — twelve waves, 168 VGPRs, no spills — 187.6 against 178.7 ms on 1250 x 50 kb, 768 x 6 189.6)
constexpr bool is_span(int T, int K) { return T == kSpanT && K == kSpanK; }
constexpr int kWideWaves = 4; // waves per SIMD the widest geometry is compiled for (4: 128 VGPRs, two 512-thread workgroups per CU)
constexpr int kChunk = 256;
constexpr int kFoldMaxLag = 8; // largest o1 + e1 the folded form of the packed kernel is launched for
constexpr int32_t kDeadPair = (int32_t)0x80008000u;
// The table form (mwf_band2_tab.hip: MWF_BAND2_FORM 1): the first probe of the match extension reads one halfword per sequence and
// column from a table of 8-mers (build_probe_table) instead of shifting sixteen bases out of two dwords of the 2-bit copy.  The kernel carries a name of its own.
constexpr bool kTabProbe = MWF_BAND2_FORM == 1 || MWF_BAND2_FORM == 3;
// The second fold (mwf_band2_tab2.hip: MWF_BAND2_FORM 3; band2_pass: kFold2): the table form, score-only, e2 == 1, with the row the SECOND gap piece opens from folded
// into its E2 / F2 registers one penalty ahead, as FOLD does with the first piece's.  Launched for o2 + e2 <= kFold2MaxLag.  The bound is the default penalties' lag
// (o2 + e2 = 16), and no more: the form's ageing period is a compile-time count that follows from the bound (kAgeOut), and every penalty of slack in it is one more masked
// run of each chunk a shrink leaves behind, for every pair — the default set is what the form is measured on, and a set with a longer lag keeps the table form.
constexpr bool kFold2Form = MWF_BAND2_FORM == 3;
constexpr int kFold2MaxLag = 16;
// The 4-bit form (mwf_band2_nib.hip: MWF_BAND2_FORM 2): the S2 paths — sequence copy, first probe, match walks — hold FOUR bits per base,
// eight bases per dword, base j at bits 4*(j & 7) of dword j >> 3, packed from the image bytes of a pair of 5 to 16 distinct bytes ("alpha16": 0x40 | code,
// mwf_alphabet.hip).  Everything that differs follows from two constants: kSeqSh, log2 of the bits per base, and kSeqDw, log2 of the bases per dword.  The kernel
// carries a name of its own; in the other forms both constants are the 2-bit form's and every expression folds to what it was.
constexpr bool kNib = MWF_BAND2_FORM == 2;
constexpr int kSeqSh = kNib ? 2 : 1, kSeqDw = kNib ? 3 : 4, kSeqPer = 1 << kSeqDw;
constexpr uint32_t kNibTag = 0x40; // high nibble of an image byte (MWF_ALPHA16_TAG, include/miniwfa.h)
// The table form's chunk chain (band2_pass: kChain).  A slot keeps its chunk for hundreds of penalties, and what the probe derives from the chunk alone — the room
// bounds rj of the lane's columns, the query's table index less j — is kept per slot in registers, computed where the slot's chunk is assigned (remap), for the
// instantiations that hold it within their register budget: 512 x 3 with and without traceback, 512 x 4 score-only (512 x 4 with traceback stands at 127 VGPRs).
constexpr bool band2_geo_cached(int T, int K, bool TB) { return kTabProbe && T == 512 && (K == 3 || (K == 4 && !TB)); }
constexpr int kTabSlack = 258; // table entries beyond tl + ql: target position tl, query position -1, and the query positions a chunk's columns beyond cmax clamp to (up to ql + 255)

__device__ __forceinline__ int32_t lo16(int32_t v) { return (int32_t)(int16_t)(v & 0xffff); }
__device__ __forceinline__ int32_t hi16(int32_t v) { return v >> 16; }
__device__ __forceinline__ int32_t pack2(int32_t a, int32_t b)
{
	typedef short short2_t __attribute__((ext_vector_type(2)));
	const short2_t v = __builtin_amdgcn_cvt_pk_i16(a, b); // saturating
	return __builtin_bit_cast(int32_t, v);
}

// four bytes at byte offset `off` of the sequence copy (which starts at LDS offset 0)
__device__ __forceinline__ uint32_t seq4(int32_t off)
{
	const uint32_t *p = (const uint32_t*)(lds2 + (off & ~3));
	return __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)off);
}

// leading equal bytes of a 4-byte probe result (0 bits = equal bytes): v_ffbl_b32 yields -1 for x == 0
__device__ __forceinline__ int32_t lead_eq(uint32_t x)
{
	int32_t fb;
	asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(x));
	return (int32_t)((uint32_t)fb >> 3);
}

// The recurrence with its traceback byte (dev::wf_cell, miniwfa.c:267-278, :289-306) written for few live registers.
template <bool WANT_TB>
__device__ __forceinline__ Cell cell16(int32_t hx, int32_t o1m, int32_t g1m, int32_t o2m, int32_t g2m,
                                       int32_t o1p, int32_t g1p, int32_t o2p, int32_t g2p)
{
	if (!WANT_TB) return wf_cell<false>(hx, o1m, g1m, o2m, g2m, o1p, g1p, o2p, g2p);
	Cell c;
	c.e1 = max(o1m, g1m);
	c.e2 = max(o2m, g2m);
	c.f1 = max(o1p, g1p) + 1;
	c.f2 = max(o2p, g2p) + 1;
	const int32_t e = max(c.e1, c.e2), f = max(c.f1, c.f2), g = max(e, f), m = hx + 1;
	c.h = max(m, g);
	// The byte from the RESULTS (so that the gap sources are read once and can stay 16-bit operands): H is the maximum of
	// m, e1, e2, f1, f2 and the reference's tie-breaking (mismatch, then E1, E2, F1, F2) is the first of them that equals it;
	// a gap state was extended iff it differs from what opening it would have given.
	const uint32_t z = c.h == m ? 0u : c.h == c.e1 ? 1u : c.h == c.e2 ? 3u : c.h == c.f1 ? 2u : 4u;
	c.tb = z | ((uint32_t)(c.e1 != o1m) << 3) | ((uint32_t)(c.f1 != o1p + 1) << 4) | ((uint32_t)(c.e2 != o2m) << 5) | ((uint32_t)(c.f2 != o2p + 1) << 6);
	(void)e, (void)f, (void)g;
	return c;
}

// Leading equal bytes of t[j..] and q[..] (aq: byte offset of the query base), at most eight looked at: three dwords of
// each sequence, two v_alignbyte's each.  Returns min(equal bytes, 9 if all eight are equal).
struct Probe8 { uint32_t t0, t1, t2, q0, q1, q2; };
__device__ __forceinline__ void probe8_issue(Probe8 &p, int32_t j, int32_t aq)
{
	const uint32_t *pt = (const uint32_t*)(lds2 + (j & ~3)), *pq = (const uint32_t*)(lds2 + (aq & ~3));
	p.t0 = pt[0], p.t1 = pt[1], p.t2 = pt[2], p.q0 = pq[0], p.q1 = pq[1], p.q2 = pq[2];
}
__device__ __forceinline__ int32_t probe8_count(const Probe8 &p, int32_t j, int32_t aq)
{
	const uint32_t x0 = __builtin_amdgcn_alignbyte(p.t1, p.t0, (uint32_t)j) ^ __builtin_amdgcn_alignbyte(p.q1, p.q0, (uint32_t)aq);
	const uint32_t x1 = __builtin_amdgcn_alignbyte(p.t2, p.t1, (uint32_t)j) ^ __builtin_amdgcn_alignbyte(p.q2, p.q1, (uint32_t)aq);
	return min(min(lead_eq(x0), lead_eq(x1) + 4), 9); // lead_eq is huge for "no difference"
}

// ---- 2-bit sequence copy (pairs of plain A/C/G/T): sixteen bases per dword, base j at bits 2*(j & 15) of dword j >> 4.
// One ds_read2_b32 and one v_alignbit per sequence give SIXTEEN bases from any position: the first probe of the match
// extension needs two LDS instructions instead of four (a wave issues one LDS instruction every 15-40 cycles,
// profiles/r02/lds_issue_rates_microbench.txt) and a run must be twice as long before the per-lane loop is entered.
__device__ __forceinline__ uint32_t seq16(int32_t base, int32_t j)
{
	const uint32_t *p = (const uint32_t*)(lds2 + base + ((j >> kSeqDw) << 2));
	return __builtin_amdgcn_alignbit(p[1], p[0], (uint32_t)j << kSeqSh);
}
// leading equal bases of a 16-base probe result (0 bits = equal); huge for "no difference"
__device__ __forceinline__ int32_t lead_eq2(uint32_t x)
{
	int32_t fb;
	asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(x));
	return (int32_t)((uint32_t)fb >> kSeqSh);
}
struct Probe16 { uint32_t t0, t1, q0, q1; };
__device__ __forceinline__ void probe16_issue(Probe16 &p, int32_t qbase, int32_t j, int32_t iq)
{
	const uint32_t *pt = (const uint32_t*)(lds2 + ((j >> 4) << 2)), *pq = (const uint32_t*)(lds2 + qbase + ((iq >> 4) << 2));
	p.t0 = pt[0], p.t1 = pt[1], p.q0 = pq[0], p.q1 = pq[1];
}
// min(equal bases, 17 if all sixteen are equal)
__device__ __forceinline__ int32_t probe16_count(const Probe16 &p, int32_t j, int32_t iq)
{
	return min(lead_eq2(__builtin_amdgcn_alignbit(p.t1, p.t0, (uint32_t)j << 1) ^ __builtin_amdgcn_alignbit(p.q1, p.q0, (uint32_t)iq << 1)), 17);
}
// exact-match run t[j..] == q[iq..] on the 2-bit copies, at most `room`, the first n0 known equal, walked by all 64 lanes:
// 1024 bases per trip (the 4-bit form: 8 bases per lane, 512 per trip).  Arguments wave-uniform.
__device__ __forceinline__ int32_t run_wave16(int32_t qbase, int32_t j, int32_t iq, int32_t room, int32_t n0, int32_t tbase = 0)
{
	const int32_t lane = threadIdx.x & 63;
	int32_t n = n0;
	while (n < room) {
		const int32_t off = n + kSeqPer * lane;
		int32_t m = 0;
		if (off < room) m = min(min(lead_eq2(seq16(tbase, j + off) ^ seq16(qbase, iq + off)), kSeqPer), room - off);
		const unsigned long long stop = __ballot(m < kSeqPer);
		if (stop == 0) { n += 64 * kSeqPer; continue; }
		const int32_t first = (int32_t)__builtin_ctzll(stop);
		n += kSeqPer * first + __builtin_amdgcn_readlane(m, first);
		break;
	}
	return min(n, room);
}
// Bytes -> 2 bits per base into LDS at `base` (two dwords of slack behind the last base).  Returns nonzero when a byte is not
// one of A, C, G, T.  code = (byte >> 1) & 3: A 0, C 1, T 2, G 3.
template <int T>
__device__ __forceinline__ uint32_t pack2bit(const uint8_t *src, int32_t len, int32_t base)
{
	uint32_t bad = 0;
	const int32_t n_dw = (len >> 4) + 2;
	for (int32_t w = threadIdx.x; w < n_dw; w += T) {
		uint32_t out = 0;
		const int32_t b0 = w << 4;
		if (b0 + 16 <= len) {
			uint32_t q[4];
			__builtin_memcpy(q, src + b0, 16);
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const uint32_t x = q[k], code = (x >> 1) & 0x03030303u;
				// the byte each code stands for: 0 'A' 0x41, 1 'C' 0x43, 2 'T' 0x54, 3 'G' 0x47
				const uint32_t lo1 = code & 0x01010101u, hi1 = (code >> 1) & 0x01010101u;
				const uint32_t expect = 0x41414141u + (lo1 & ~hi1) * 0x02u + (hi1 & ~lo1) * 0x13u + (hi1 & lo1) * 0x06u;
				bad |= x ^ expect;
				out |= ((code | code >> 6 | code >> 12 | code >> 18) & 0xffu) << (8 * k);
			}
		} else {
#pragma unroll 1
			for (int32_t k = 0; k < 16 && b0 + k < len; ++k) {
				const uint32_t x = src[b0 + k], code = (x >> 1) & 3u;
				bad |= x ^ ((0x47544341u >> (8 * code)) & 0xffu);
				out |= code << (2 * k);
			}
		}
		*(uint32_t*)(lds2 + base + 4 * w) = out;
	}
	return bad;
}

// The 4-bit form: image bytes (kNibTag | code) -> 4 bits per base into LDS at `base`, sixteen bytes (two dwords of the copy) per thread and step, two dwords of
// slack behind the last base.  Returns nonzero when a byte does not carry the tag: the pair was not copied for this form (the host re-runs it byte-wise).
template <int T>
__device__ __forceinline__ uint32_t pack4bit(const uint8_t *src, int32_t len, int32_t base)
{
	uint32_t bad = 0;
	const int32_t n_dw = (len >> 3) + 2;
	for (int32_t w = 2 * (int32_t)threadIdx.x; w < n_dw; w += 2 * T) {
		uint32_t out[2] = {0, 0};
		const int32_t b0 = w << 3;
		if (b0 + 16 <= len) {
			uint32_t q[4];
			__builtin_memcpy(q, src + b0, 16);
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const uint32_t x = q[k];
				bad |= (x & 0xf0f0f0f0u) ^ (kNibTag * 0x01010101u);
				uint32_t c = x & 0x0f0f0f0fu;
				c = (c | c >> 4) & 0x00ff00ffu;
				c = (c | c >> 8) & 0xffffu;
				out[k >> 1] |= c << (16 * (k & 1));
			}
		} else {
#pragma unroll 1
			for (int32_t k = 0; k < 16 && b0 + k < len; ++k) {
				const uint32_t x = src[b0 + k];
				bad |= (x & 0xf0u) ^ kNibTag;
				out[k >> 3] |= (x & 0xfu) << (4 * (k & 7));
			}
		}
		*(uint32_t*)(lds2 + base + 4 * w) = out[0];
		if (w + 1 < n_dw) *(uint32_t*)(lds2 + base + 4 * w + 4) = out[1];
	}
	return bad;
}

// The table form's probe table, from the 2-bit copies at `tbase` / `qbase` (after pack2bit and a barrier): halfword p <= tl holds the eight bases from target position p
// (the low 16 bits of seq16), halfword tl + 2 + q those from query position q, -1 <= q <= ql + 255 (zero outside [0, ql]).  The cell of column c at target
// position j probes halfwords j and j + c + 1: query position j + c - 1 - tl.  Bases behind the end of a sequence are whatever the copy's slack holds — the room clamp
// of the probe makes them irrelevant.  The table starts at LDS address 0.
template <int T>
__device__ __forceinline__ void build_probe_table(int32_t tl, int32_t ql, int32_t tbase, int32_t qbase)
{
	const int32_t n = tl + ql + kTabSlack;
	for (int32_t e = threadIdx.x; e < n; e += T) {
		const int32_t q = e - tl - 2;
		uint32_t v = 0;
		if (e <= tl) v = seq16(tbase, e);
		else if (q >= 0 && q <= ql) v = seq16(qbase, q);
		*(uint16_t*)(lds2 + 2 * e) = (uint16_t)v;
	}
}

__device__ __forceinline__ unsigned long long lane_mask(int32_t base, int32_t k, int32_t a, int32_t b)
{
	int32_t lmin = a - base - k, lmax = b - base - k;
	if (lmax < 0) return 0ull;
	lmin = lmin <= 0 ? 0 : (lmin + 3) >> 2;
	lmax = min(lmax >> 2, 63);
	if (lmin > lmax) return 0ull;
	return (~0ull >> (63 - lmax)) & (~0ull << lmin);
}

// exact-match run t[j..] == q[..] (aq = byte offset of the query base in LDS), at most `room`, the first n0 known equal,
// walked by all 64 lanes: 256 bytes per trip.  Arguments wave-uniform.
__device__ __forceinline__ int32_t run_wave2(int32_t j, int32_t aq, int32_t room, int32_t n0)
{
	const int32_t lane = threadIdx.x & 63;
	int32_t n = n0;
	while (n < room) {
		const int32_t off = n + 4 * lane;
		int32_t m = 0;
		if (off < room) {
			const uint32_t x = seq4(j + off) ^ seq4(aq + off);
			m = min(min(lead_eq(x), 4), room - off);
		}
		const unsigned long long stop = __ballot(m < 4);
		if (stop == 0) { n += 256; continue; }
		const int32_t first = (int32_t)__builtin_ctzll(stop);
		n += 4 * first + __builtin_amdgcn_readlane(m, first);
		break;
	}
	return min(n, room);
}

// ---- biased offsets (the 1024-thread geometry: targets of up to ~60 kb).  A 16-bit half holds  offset - B  with B = wide_bias(tl):
// live offsets are >= -1, i.e. halves >= -1 - B, and everything below is dead.  Every place that reads an offset as a number adds B
// back (the "+ 1" of j = k + 1 becomes "+ 1 + B": no instruction more); as unsigned 16-bit numbers the true values (up to 65 535)
// fit where signed ones would not.  Two things move towards the ends of the 16 bits by at most one per penalty and are CHECKED at
// every penalty that is a multiple of 256 (in the good-bit code of that penalty), with a margin of kBiasMargin > 2 x 256 + nH (what was
// computed since the last check but one is still being read from the H ring):
//   * dead values start at -32768 and a chain of them — F2 of the columns next to the lower window edge, which moves with the chain — gains
//     one per penalty: no value may lie in [-1 - B - kBiasMargin, -1 - B);
//   * offsets that ran past the end of the target (F of cells beyond the matrix keeps counting): no H above 32767 - kBiasMargin, i.e. more
//     than kBiasOver - kBiasMargin beyond the target's end.
// A pair that fails a check is handed back (ST_BAND_OVERFLOW: generic kernel).  With tl = 50 000 the dead side holds ~12 900 penalties.
constexpr int32_t kBiasOver = 1500, kBiasMargin = 600;
__device__ __forceinline__ int32_t wide_bias(int32_t tl) { return max(tl + kBiasOver - 32767, 0); }

template <int D, int NWK>
struct alignas(16) Band2Lds {
	Shared sh;
	// per age and chunk slot r (entry r + 1): {E1, E2 of columns (c1,c3) of lane 63 | F1, F2 of columns (c0,c2) of lane 0}; entry 0 mirrors
	// slot NWK-1 and entry NWK+1 slot 0, so that a slot finds its neighbours at fixed distances from its own entry
	int32_t edge[D][NWK + 2][4];
	int32_t dump[64 * 2 + (2 * NWK + 4) * 4]; // where the lanes that do not hold an outer column put theirs (no exec-mask games around the stores)
};

// ---- packed 16-bit arithmetic: two columns per register, every operation one VOP3P instruction.  Offsets are SIGNED halves here; what works on
// unsigned halves (pk_minu, pk_subsat, pk_nonzero_mask, pk_ne1, pk_mad) is shared with the generic kernel: mwf_device.h
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int32_t pk_max(int32_t a, int32_t b) { return MWF_BC(int32_t, __builtin_elementwise_max(MWF_BC(s16x2, a), MWF_BC(s16x2, b))); }
__device__ __forceinline__ int32_t pk_add(int32_t a, int32_t b) { return MWF_BC(int32_t, (s16x2)(MWF_BC(s16x2, a) + MWF_BC(s16x2, b))); }
__device__ __forceinline__ int32_t pk_sub(int32_t a, int32_t b) { return MWF_BC(int32_t, (s16x2)(MWF_BC(s16x2, a) - MWF_BC(s16x2, b))); }
__device__ __forceinline__ int32_t bfi(int32_t mask, int32_t a, int32_t b) { return (a & mask) | (b & ~mask); } // mask ? a : b, bitwise
__device__ __forceinline__ int32_t half_of(int32_t v, int hi) { return hi ? v >> 16 : (int32_t)(int16_t)(v & 0xffff); }
__device__ __forceinline__ int32_t pair_of(int32_t lo, int32_t hi) { return (int32_t)(((uint32_t)hi << 16) | ((uint32_t)lo & 0xffffu)); }

// A lane's four columns c0..c3 of a chunk live in two registers, A = (c0, c2) and B = (c1, c3): the columns to the left of A's
// are (c-1, c1) — B shifted in from the lane to the left — and those to the left of B's are A itself; to the right of A's: B, to
// the right of B's: (c2, c4).  `fill` supplies what lane 0 (lane 63) takes from beyond the chunk.
__device__ __forceinline__ int32_t left_of_A(int32_t B, int32_t fill) { return __builtin_amdgcn_alignbit(B, from_left(B, fill), 16); }
__device__ __forceinline__ int32_t right_of_B(int32_t A, int32_t fill) { return __builtin_amdgcn_alignbit(from_right(A, fill), A, 16); }

template <int T, int K, int E1, int E2, bool TB, bool S2, bool BI4, bool FOLD, typename ArgsT>
__device__ PassResult band2_pass(const ArgsT &A, const PairMem &M, Shared &sh, const int32_t edge_base, const int32_t qoff, bool trace_band)
{
	constexpr int NW = T / 64, NWK = NW * K, D = (E1 > E2 ? E1 : E2) + 1;
	constexpr bool BI = is_span(T, K) || BI4; // biased offsets with range checks (wide_bias): the span geometry and the four-slot 512-thread one's copy for long pairs
	constexpr bool TAB = kTabProbe && S2; // the first probe reads the 8-mer table in front of the 2-bit copies
	constexpr int FULL = TAB ? 8 : S2 ? kSeqPer : 8; // bases the first probe of the match extension looks at (one dword of the copy: sixteen at 2 bits, eight at 4)
	constexpr bool kChain = TAB;                          // the table form: the rare tests of a chunk are marked as such, an interior chunk without a long run falls through
	constexpr bool kGeo = TAB && band2_geo_cached(T, K, TB); // ... and the chunk's probe geometry is read from the slot's registers
	constexpr bool kFold2 = kFold2Form && TAB && FOLD && !TB && E2 == 1; // the second gap piece folded one penalty ahead (below)
	static_assert(!kFold2Form || kFold2, "the second fold exists on the table form, folded, score-only, e2 == 1");
	// a test that is rarely true, for the forms that say so; a macro of this function alone (#undef behind it), written in the condition itself: the hint is lowered
	// before inlining and does not survive a function or lambda boundary
#define MWF_RARE(x) (kChain ? __builtin_expect((x), 0) != 0 : (x))
	// FOLD (score-only, gap-open lag - mismatch lag == e1, i.e. o1 == x as in the default penalties): the row a penalty reads for its
	// mismatch term, H[s-x], IS the row the first gap piece opens from e1 penalties later (miniwfa.c:267-278: both E1 and F1 take
	// max(H[s-o1-e1], E1/F1[s-e1]) of a neighbouring column).  The registers that hold E1/F1 of the last e1 penalties therefore hold
	// max(E1, H[s-x]) (max(F1, H[s-x])) instead — the maximum is what the reference computes e1 penalties later — and the kernel does
	// not load the row of lag o1+e1 at all.  A chunk that left the window keeps running until the rows it computed have been folded
	// and aged out: kAgeOut penalties (the host asks for this form only when o1 + e1 <= kFoldMaxLag).
	// With traceback the byte must tell an opened first gap piece from an extended one (miniwfa.c:289-306) — the comparison the fold no
	// longer makes at the cell itself.  It makes it e1 penalties EARLIER, in the neighbouring column, where both terms are at hand:
	// E1[s] > H[s-x] there means "the E1 of penalty s+e1 one column on is an extension".  Bits 3 and 4 of a folded byte say that
	// (PairMem::tb_fwd), and the walk reads them from the cell an extension would come from (traceback_wave: one more byte per gap run).
	// kFold2 (e2 == 1): the same for the second piece, whose rows lie further apart.  Reference: E2[s][d] = max(H[s-o2-e2][d-1], E2[s-e2][d-1]), F2 likewise from d+1,
	// plus one.  The row H[s-o2-e2] is the row of lag o2 at penalty s - e2, so after penalty t the slot's E2 / F2 registers (and its edge-table entries) hold
	// max(E2[t][d], H[t-o2][d]) and max(F2[t][d], H[t-o2][d]), and penalty t + 1 takes them from the neighbouring column with no row of its own: per chunk ONE load of
	// the row of lag o2, column-aligned (no neighbour word, no shifts), consumed at the fold — the recurrence waits for the row of lag x alone.  The fold stands
	// behind the first probe of the match extension, not beside the E1 fold: the row of lag o2 is the one that misses L2, and there it has had the chunk's whole front
	// and the probe's LDS round trip to arrive.  (Beside the E1 fold, in front of put_edge, measured 13.6 against the table form's 11.4 and this placement's 10.8 ms
	// per step of the headline batch: profiles/band_fold2/, the patch with both placements in profiles/experiments/.)  The slot's edge-table entry is therefore stored
	// in two halves, the first piece's in front of the probe and the second piece's behind it.
	// Ageing: a chunk whose last penalty inside the window was t0 computed rows up to H[t0].  H[t0] is folded at penalty t0 + o2, the o2-th masked run (the folds before
	// it take the rows before it, the folds behind it rows the masked runs themselves stored dead); the E1 fold's last live row goes in at run x < o2.  The folded value
	// is read at t0 + o2 + e2 from the registers and from the edge table, and D = max(e1, e2) + 1 further runs overwrite all D ages of the table and every register age
	// with dead values: o2 + D runs.  With o2 + e2 <= kFold2MaxLag that is at most kFold2MaxLag - E2 + D (18 for the default set, which needs exactly that).
	constexpr int kAgeOut = kFold2 ? kFold2MaxLag - E2 + D : FOLD ? kFoldMaxLag : D;
	static_assert(!kFold2 || (kAgeOut >= kFoldMaxLag && kAgeOut < 128), "the second fold ages at least as long as the first; two shrinks are 256 penalties apart");
	constexpr int kAge = (NWK + 2) * 16; // bytes of one age of the edge table
	static_assert(D >= 2 && D <= 5, "edge-table ages"); // one table per penalty an E/F can be read back from, plus the one being written: epos[] rotates through them
	const int32_t tl = M.tl, ql = M.ql, cmax = tl + ql + 1;
	const int32_t tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
	const int32_t W = A.W, nH = A.pen.nH, lagx = A.pen.x, lag1 = A.pen.oe1, lag2 = A.pen.oe2;
	const int32_t B = BI ? wide_bias(tl) : 0;                   // a half holds offset - B
	const int32_t ONEB = BI ? both16(1 + B) : 0x00010001;       // k -> j = k + 1 as a true (unsigned) number
	// H rows: W int16 per row, a quad of columns 4q..4q+3 stored as (c0, c2, c1, c3) — the two registers of a lane, one 8-byte load;
	// 8 bytes of slack in front (lane 0 of chunk 0 looks one quad to the left; offsets are unsigned: the slack is part of `lane8`)
	char *const Hb = (char*)M.H;
	const uint32_t RS = (uint32_t)W << 1; // bytes per row
	const int32_t lag2r = kFold2 ? lag2 - E2 : lag2; // the lag of the row read for the second gap piece: kFold2 reads it e2 penalties early, at the fold
	const int32_t min_lag = min(lagx, min(lag1, lag2r));
	const bool relaxed_stores = min_lag >= 3; // rows written now are first loaded two penalties from now: stores may cross the barrier
	PassResult R;
	R.status = ST_OK, R.s = 0, R.info = 0, R.n_snap = 0, R.cells = 0;

	// per-thread wavefront state, two columns per register: [age - 1][slot][A / B]
	static_assert(E1 >= 1 && E1 <= 4 && (E2 == 1 || E2 == 2), "history depth");
	int32_t e1h[E1][K][2], f1h[E1][K][2], e2h[E2][K][2], f2h[E2][K][2];
#pragma unroll
	for (int k = 0; k < K; ++k)
#pragma unroll
		for (int i = 0; i < 2; ++i) {
#pragma unroll
			for (int a = 0; a < E1; ++a) e1h[a][k][i] = f1h[a][k][i] = kDeadPair;
#pragma unroll
			for (int a = 0; a < E2; ++a) e2h[a][k][i] = f2h[a][k][i] = kDeadPair;
		}
	// lane constants: local columns of A and B, byte offset of the lane's quad, of the neighbouring word it fetches
	const int32_t RA = pair_of(4 * lane, 4 * lane + 2); // (RB = RA + 1, RB1 = RA + 2 per half are recomputed where needed: registers are scarcer than adds)
	const uint32_t lane8 = ((uint32_t)lane << 3) + 8u;
	const int32_t nd = lane == 0 ? -4 : 8; // lane 0: B of the quad to the left; lane 63: A of the quad to the right
	const int32_t T0 = both16(cmax), TLp = both16(tl), TL1 = both16(tl + 1);
	// edge-table addresses: a slot's entry sits (k NW + 1) entries behind the wave's base.  Every lane stores its outer columns —
	// lane 63 (E) and lane 0 (F) into the table, the others into a dump — so that no store needs an exec mask.
	const int32_t ebase = edge_base + wave * 16, dump_base = edge_base + D * kAge + NW * 16; // (the mirror store reaches NW-1 entries back)
	const int32_t dump_lane = dump_base + lane * 8;
	int32_t epos[D]; // byte offset of the table of age a + 1 (penalty s_new - a - 1); the oldest is overwritten and becomes age 1
#pragma unroll
	for (int a = 0; a < D; ++a) epos[a] = a * kAge;

	// ---- every row read before it is written must read as dead around the origin: a slot that no penalty has written yet is only read
	// during the first nH - 1 penalties, whose windows (and the columns next to them) stay within nH + 1 columns of the origin
	{
		const int32_t reach = nH + 1 + 8, g_a = max(tl + 1 - reach, 0) >> 8, n_g = ((tl + 1 + reach) >> 8) - g_a + 1, per_row = n_g * 64;
		for (int32_t q = tid; q < nH * per_row; q += T) {
			const int32_t row = q / per_row, rem = q - row * per_row;
			*(int2*)(Hb + (size_t)((uint32_t)row * RS + (uint32_t)(g_a * 512 + rem * 8 + 8))) = make_int2(kDeadPair, kDeadPair);
		}
	}
	// ---- penalty 0 (reference wf_stripe_init, miniwfa.c:103-121) and its extension
	for (int32_t j = tid; j < D * (NWK + 2) * 4; j += T) *(int32_t*)(lds2 + edge_base + 4 * j) = kDeadPair;
	if (tid == 0) {
		for (int32_t j = 0; j < nH; ++j) sh.rng_lo[j] = 1, sh.rng_hi[j] = 0;
		for (int32_t j = 0; j < 12; ++j) (&sh.flags[0][0])[j] = 0;
		sh.rng_lo[0] = sh.rng_hi[0] = tl + 1;
		sh.word[3] = -1; // furthest offset seen at a forecast penalty (dev::window_forecast)
	}
	__syncthreads(); // (orders the dead rows before the origin's store)
	if (tid < 64) { // the origin's run, walked by the first wave
		const int32_t k0 = (S2 ? run_wave16(qoff, 0, 0, min(tl, ql), 0, TAB ? fresh(A).band_lds_tab : 0) : run_wave2(0, qoff, min(tl, ql), 0)) - 1;
		if (tid == 0) {
			const int32_t c = tl + 1, e = c & 3;
			*(int16_t*)(Hb + 8 + (size_t)(uint32_t)(((c & ~3) + ((e & 1) << 1) + (e >> 1)) << 1)) = (int16_t)(k0 - B);
			sh.word[1] = k0;
		}
	}
	__syncthreads();
	{
		const int32_t k0 = uni(sh.word[1]);
		if (k0 == tl - 1 && k0 == ql - 1) return R;
	}

	int32_t s = 0, wf_lo = tl + 1, wf_hi = tl + 1;
	int32_t curH = 0, par = 0;
	const uint32_t ring_bytes = (uint32_t)nH * RS;
	// rows of the coming penalty and of its three lags, as byte offsets that advance by one row per penalty (penalty 1 first)
	uint32_t bn = (uint32_t)(1 % nH) * RS, bx = (uint32_t)((nH - lagx + 1) % nH) * RS, b1 = (uint32_t)((nH - lag1 + 1) % nH) * RS, b2 = (uint32_t)((nH - lag2r + 1) % nH) * RS;
	// The rows of ONE chunk: H at the three lags (one 8-byte load each) and the word next to the chunk for the two gap-open rows.
	// (Requesting the coming penalty's rows of the wave's first chunk before or straight behind the barrier was measured in rounds 3-5: no gain, -3 % on the
	// folded form — the row loads are not what the critical wave waits for; the variants are in profiles/experiments/.)
	struct Rows { int2 HX, O1, O2; int32_t N1, N2; } pre;
	pre.HX = pre.O1 = pre.O2 = make_int2(0, 0), pre.N1 = pre.N2 = 0;
	auto load_rows = [&](Rows &r, const char *rx, const char *r1, const char *r2, uint32_t off) {
		const uint32_t noff = off + (uint32_t)nd;
		r.HX = *(const int2*)(rx + off), r.O2 = *(const int2*)(r2 + off);
		if (!kFold2) r.N2 = *(const int32_t*)(r2 + noff); // (kFold2: O2 is the row of lag o2, folded column by column — no neighbour word)
		if (!FOLD) r.O1 = *(const int2*)(r1 + off), r.N1 = *(const int32_t*)(r1 + noff);
	};
	const int64_t iter_limit = A.max_iter > 0 ? A.max_iter : INT64_MAX;
	// (kChain: `cells` holds what is LEFT of the iteration budget, iter_limit less the cells computed, and the test behind the barrier is its sign — the limit itself was
	// reloaded from the kernarg segment at every penalty, a scalar-memory round trip on every wave's path between two penalties; R.cells is rebuilt at the exit)
	int64_t cells = kChain ? iter_limit : 0, tb_used = 0;
	int32_t est_window = 0;
	const int32_t s_limit = A.max_s > 0 ? A.max_s : INT32_MAX;
	const int64_t rows_slot = TB ? A.rows_slot : 0, tb_slot_bytes = TB ? A.tb_slot_bytes : 0;

	// chunk of every slot of this wave under the mapping that starts at chunk gl (changes only when gl does)
	int32_t gl = (wf_lo > 1 ? wf_lo - 1 : 1) >> 8, gk[K];
	// (kGeo: the slot's probe geometry, a function of gk[k], the lane, tl and ql — the expressions of the chunk body, evaluated here.  gk[k] is assigned nowhere
	// else, so the registers are never stale.)
	int32_t grjA[K], grjB[K], gdA[K];
	auto remap = [&](int32_t g_lo) {
		const int32_t base = g_lo - g_lo % NWK;
#pragma unroll
		for (int k = 0; k < K; ++k) {
			int32_t g = base + wave + NW * k;
			if (g < g_lo) g += NWK;
			gk[k] = g;
			if (kGeo) {
				const int32_t cbp = both16(g * kChunk), xAc = pk_subsat(pk_subsat(T0, cbp), RA);
				grjA[k] = pk_minu(xAc, TLp), grjB[k] = pk_minu(pk_subsat(xAc, 0x00010001), TLp);
				gdA[k] = pk_add(pk_add(RA, cbp), 0x00010001);
			}
		}
	};
	remap(gl);
	int32_t idle[K]; // penalties since the slot last held an active chunk (registers and edge-table entries start dead)
#pragma unroll
	for (int k = 0; k < K; ++k) idle[k] = kAgeOut;
	int32_t up_wait = 0, up_min = 0; // penalties for which the window has started above chunk gl, the lowest start among them
	// Window epoch.  What a penalty's header derives about this wave's slots depends only on the chunks the window meets, ga = lo >> 8 and
	// gb = hi >> 8, on the mapping start gl and on the slots' ages — and an edge moves one column per penalty, so the same answers hold for
	// about a hundred penalties on end.  The header therefore keeps them in one scalar, `est`, together with the key they were derived for
	// (`ekey`: gl_next, gb and ga - gl_next packed, or 0), and a penalty whose key is the same reuses them (the fast header): no activity
	// compares, no priority ladder (the priority persists by itself), no overflow tests, no remap comparison behind the barrier.  The key
	// is only kept when nothing else is in motion: no slot ageing, no remap pending (gl_next == gl, up_wait == 0), the coarse overflow and
	// three-slot tests false, i.e. false for every window with these chunks.  Every other penalty runs the full header.
	// est: per slot k bits 4k..4k+3 = runs | holds the lo edge (g == ga) | holds the hi edge (g == gb) | ageing (outside the window);
	// bit 24 / 25: this wave stores the dead chunk below / above the window;
	// kChain, bit 26 + k: slot k runs the chunk that holds column ql + 1, the only one the end cell can lie in (a function of gk[k], which a remap alone changes — and
	// a remap drops the key).
	int32_t ekey = 0;
	// Gated off, i.e. the full header every penalty: the span geometry (the cached word costs its folded score-only form its last free register — scratch where it had
	// none) and the 64-thread geometry (one wave per pair: nothing is repeated eight times, and 2048 x 400 bp measured 0.366 -> 0.404 ms with the fast header).
	constexpr bool kEpoch = !is_span(T, K) && T != 64;
	uint32_t est = 0;
	static_assert(kEpoch || ((NW & (NW - 1)) == 0 && !(T == 512 && K == 4)), "the full header of the gated geometries is written for a power-of-two wave count and no three-slot note");
	static_assert(K <= 6, "slot classes of the window epoch: four bits per slot below bit 24");
	constexpr bool kLeanTail = kChain; // the table form: the rare work behind a chunk's extension hangs on bits of est alone
	static_assert(!kLeanTail || (kEpoch && K <= 4), "the table form keeps one more bit per slot in est, from bit 26 on");
	constexpr uint32_t kRunBits = 0x111111u & ((1u << (4 * K)) - 1u); // the "runs" bit of every slot

	// One penalty; returns true when the pass ends.  A depth-2 history is two registers, [0] the newer: the penalty reads [1] for the last
	// time, overwrites it, and the two trade places (v_swap_b32) — no copies, and a slot that is skipped leaves its registers alone.
	// Depth 3 and 4 (gap extensions of 3 and 4): the penalty reads and overwrites the oldest, [E - 1], and the new value trades places with
	// its neighbour E - 1 times on its way to [0] — a rotation by one, every other age one place older.
	auto step = [&]() __attribute__((always_inline)) -> bool {
		constexpr int P1 = E1 - 1, P2 = E2 - 1;
#ifdef MWF_B2_TIMING
		const uint64_t tm0 = __builtin_readcyclecounter();
#endif
		const int32_t lo = wf_lo > 1 ? wf_lo - 1 : 1;       // miniwfa.c:417-418
		const int32_t hi = wf_hi < cmax ? wf_hi + 1 : cmax;
		const int32_t lo_p = lo, hi_p = hi;
		const int32_t s_new = s + 1;
		const int32_t newH = curH + 1 == nH ? 0 : curH + 1;
		const int32_t npar = par + 1 == 3 ? 0 : par + 1;
		const int32_t origin = lo & ~3;
		const int32_t row_bytes = (hi | 3) - origin + 1;
		if (TB) {
			if (s_new - 1 >= rows_slot) { R.status = ST_ROWS_OVERFLOW; return true; }
			if (tb_used + row_bytes > tb_slot_bytes) { R.status = ST_TB_OVERFLOW; return true; }
		}
		// the window of penalty s_new+1 lies inside [lo-1, hi+1] whatever the flags say; it must fit the register span
		const int32_t gl_next = (lo > 1 ? lo - 1 : 1) >> 8;
		const int32_t ga = lo >> 8, gb = hi >> 8; // chunks [ga, gb] meet the window
		const int32_t key = gl_next | gb << 15 | 1 << 29 | (ga - gl_next) << 30; // (never 0, never negative)
		const bool fast = kEpoch && key == ekey; // uniform: the slot state of the last full header holds
		uint32_t st = est;
		bool act[K]; // (only where the epoch is gated off)
		if (!kEpoch) {
			if (gb - min(ga, gl + 1) + 3 > NWK - 1) // (only then can the exact test fail)
				if (((hi < cmax ? hi + 1 : cmax) >> 8) - min(gl_next, gl) + 1 > NWK - 1) { R.status = ST_BAND_OVERFLOW; return true; }
			if (BI && cmax - lo > 65535) { R.status = ST_BAND_OVERFLOW; return true; }
		} else if (!fast) {
			bool hold = true; // may the coming penalties reuse what this header derives?
			// (the mapping follows a window that moves UP kAgeOut penalties late — the chunks it leaves behind still run, see below)
			if (gb - min(ga, gl + 1) + 3 > NWK - 1) { // (only then can the exact test fail)
				if (((hi < cmax ? hi + 1 : cmax) >> 8) - min(gl_next, gl) + 1 > NWK - 1) { R.status = ST_BAND_OVERFLOW; return true; }
				hold = false;
			}
			// (the four-slot form of the 512-thread geometry notes whether the three-slot form would have held the pair: the host's choice for the next align)
			if (T == 512 && K == 4 && R.n_snap == 0 && gb - ga + 3 > 23) {
				if (((hi < cmax ? hi + 1 : cmax) >> 8) - gl_next + 1 > 23) R.n_snap = 1;
				hold = false;
			}
			// (biased offsets, sequences beyond 32 kb: the room arithmetic holds ql - d in 16 unsigned bits; lo >= 256 ga for as long as the key holds)
			if (BI) {
				if (cmax - lo > 65535) { R.status = ST_BAND_OVERFLOW; return true; }
				if (cmax - (ga << 8) > 65535) hold = false;
			}
			const int32_t gspan = gb - ga;
			int n_busy = 0;
			st = 0;
#pragma unroll
			for (int k = 0; k < K; ++k) {
				// a chunk that left the window: its columns are not computed any more, i.e. their E/F are dead.  It runs through the ordinary
				// code D more times (every column outside the window: masked dead — rare, a window edge crosses a chunk boundary inwards only
				// at a shrink), which ages the slot's registers and edge-table entries; after that there is nothing left to do.
				if ((uint32_t)(gk[k] - ga) <= (uint32_t)gspan) {
					idle[k] = 0;
					st |= (1u | (gk[k] == ga ? 2u : 0u) | (gk[k] == gb ? 4u : 0u)) << (4 * k);
					if (kLeanTail && (uint32_t)(ql + 1 - gk[k] * kChunk) < (uint32_t)kChunk) st |= 1u << (26 + k);
					if (k < 2 || k == K - 1) ++n_busy;
				} else if (idle[k] < kAgeOut) {
					++idle[k];
					st |= 9u << (4 * k);
					hold = false;
				}
			}
			// the waves with the most chunks to do set the pace of the penalty: let them issue first.  Chunks are dealt round-robin from
			// chunk ga on: the wave at distance p from it holds ceil((n - p) / NW) of the n active chunks.
			// One priority level per active chunk of the wave (0 ... 3), kept through the barrier and the next header: 18.4 -> 17.7 ms on
			// 1024 x 10 kb against "two or more chunks: 3, else 0"; stepping it down as chunks complete 19.1, other maps 17.8 ... 18.3, one more
			// level for a wave that walked a long run at the last penalty: no change.
			if ((NW & (NW - 1)) == 0) {
				// this wave holds ceil(left / NW) chunks; the waves that hold the window's first or last chunk (masks, liveness) count one more (17.7 -> 17.45 ms)
				const int32_t pos = (wave - ga) & (NW - 1);
				const int32_t left = gspan + 1 - pos + ((pos == 0 || ((gb - wave) & (NW - 1)) == 0) ? NW : 0);
				if (left > 2 * NW) __builtin_amdgcn_s_setprio(3);
				else if (left > NW) __builtin_amdgcn_s_setprio(2);
				else if (left > 0) __builtin_amdgcn_s_setprio(1);
				else __builtin_amdgcn_s_setprio(0);
			} else {
				if (n_busy >= 3) __builtin_amdgcn_s_setprio(3);
				else if (n_busy == 2) __builtin_amdgcn_s_setprio(2);
				else if (n_busy == 1) __builtin_amdgcn_s_setprio(1);
				else __builtin_amdgcn_s_setprio(0);
			}
			// every row must read as dead next to the chunks it was computed for: which wave stores them (the waves next to the window's ends hold the fewest chunks)
			if (ga >= 1 && wave == (ga - 1) % NW) st |= 1u << 24;
			if (wave == (gb + 1) % NW) st |= 1u << 25;
			est = st, ekey = kEpoch && hold ? ~key : -1; // (negative: this penalty ran the full header; the bookkeeping behind the barrier turns ~key into key unless the mapping moves)
		}
		const char *const rowx = Hb + bx, *const row1 = Hb + b1, *const row2 = Hb + b2;
		char *const rown = Hb + bn;
		const bool track_good = (((256 - (s_new & 255)) & 255) < nH); // a shrink can still see this slice
		// edge table: the ages to read (penalties s_new-E1 and s_new-E2) and the one to overwrite, as LDS addresses
		const int32_t rE1 = ebase + epos[E1 - 1], rE2 = ebase + epos[E2 - 1];
		const int32_t wE = lane == 63 ? ebase + epos[D - 1] : dump_lane, wF = lane == 0 ? ebase + epos[D - 1] : dump_lane;
		auto put_edge = [&](int k, int32_t e1b, int32_t e2b, int32_t f1a, int32_t f2a) {
			*(int2*)(lds2 + wE + (k * NW + 1) * 16) = make_int2(e1b, e2b);
			*(int2*)(lds2 + wF + (k * NW + 1) * 16 + 8) = make_int2(f1a, f2a);
			if (k == K - 1 && wave == NW - 1) *(int2*)(lds2 + wE - (NW - 1) * 16) = make_int2(e1b, e2b);  // slot NWK-1 is slot 0's left neighbour
			if (k == 0 && wave == 0) *(int2*)(lds2 + wF + (NWK + 1) * 16 + 8) = make_int2(f1a, f2a);       // slot 0 is slot NWK-1's right neighbour
		};
		// (kFold2: an entry's first-piece halves (h = 0) and second-piece halves (h = 1) stored apart, four bytes each)
		auto put_edge_half = [&](int k, int h, int32_t eb, int32_t fa) {
			*(int32_t*)(lds2 + wE + (k * NW + 1) * 16 + 4 * h) = eb;
			*(int32_t*)(lds2 + wF + (k * NW + 1) * 16 + 8 + 4 * h) = fa;
			if (k == K - 1 && wave == NW - 1) *(int32_t*)(lds2 + wE - (NW - 1) * 16 + 4 * h) = eb;
			if (k == 0 && wave == 0) *(int32_t*)(lds2 + wF + (NWK + 1) * 16 + 8 + 4 * h) = fa;
		};
		// (not in the widest geometry: what it hands back goes to the generic kernel, several times slower — it would only do so at penalty 1024
		// and beyond 1.5 x its span, and the bookkeeping costs the headline kernel 21 more spilled SGPRs)
		// (the span geometry forecasts later: what it hands back goes to the generic kernel, twice as slow — no more)
		// (none in the four-slot 512-thread geometry either — measured: a tight one at penalty 1024 costs its batches 6 % in spilled SGPRs and hands back pairs that
		// are then re-run alone, 1024 x 12 kb @ 5 % 34.2 against 24.7 ms)
		const bool forecast = NWK < 24 ? (s_new == 64 || s_new == 256 || s_new == 1024) : NWK >= 64 ? (s_new == 1024 || s_new == 4096) : false; // uniform: look at how far the pair has come (dev::window_forecast)
		int32_t far = kDeadPair;
		const int32_t cfin = ql + 1; // the end cell (tl-1, ql-1) lies on diagonal ql-tl, i.e. in this column

		if (wave == 0) { // (the whole wave stores the same words: no exec mask to set up)
			sh.rng_lo[newH] = lo, sh.rng_hi[newH] = hi;
			sh.flags[npar + 1 == 3 ? 0 : npar + 1][0] = 0; // the flag word of the NEXT penalty (its last readers passed the previous barrier)
			if (TB) M.row_off[s_new - 1] = tb_used, M.row_lo[s_new - 1] = origin;
#ifndef MWF_B2_TIMING // (the timing build keeps per-phase cycle counts in the trace buffer instead)
			if (trace_band && s_new - 1 < fresh(A).dbg_cap) M.dbg[2 * (s_new - 1)] = lo, M.dbg[2 * (s_new - 1) + 1] = hi;
#endif
		}

		if (!kEpoch) { // (the gated geometries: activity and priority where the full header always had them, behind wave 0's stores)
#pragma unroll
			for (int k = 0; k < K; ++k) act[k] = (uint32_t)(gk[k] - ga) <= (uint32_t)(gb - ga);
			const int32_t pos = (wave - ga) & (NW - 1);
			const int32_t left = gb - ga + 1 - pos + ((pos == 0 || ((gb - wave) & (NW - 1)) == 0) ? NW : 0);
			if (left > 2 * NW) __builtin_amdgcn_s_setprio(3);
			else if (left > NW) __builtin_amdgcn_s_setprio(2);
			else if (left > 0) __builtin_amdgcn_s_setprio(1);
			else __builtin_amdgcn_s_setprio(0);
		}
#ifdef MWF_B2_TIMING
		int n_act = 0;
#pragma unroll
		for (int k = 0; k < K; ++k) n_act += (kEpoch ? (st >> (4 * k) & 9u) == 1u : act[k]) ? 1 : 0;
#endif

#ifdef MWF_B2_TIMING
		const uint64_t tm1 = __builtin_readcyclecounter();
#endif
		int n_stores = 0;
		// ---- every row must read as dead next to the chunks it was computed for (a later window reaches at most nH + 1 columns
		// beyond this one: the reference's pads, miniwfa.c:96-99); the waves next to the window's ends hold the fewest chunks.  These
		// stores go first: the store that may stay in flight across the barrier (relaxed_stores) is then a chunk's own.
		// (who stores them is part of the slot state; the row is new each penalty)
		if (kEpoch ? (st & (1u << 24)) != 0 : (ga >= 1 && wave == (ga - 1) % NW)) *(int2*)(rown + ((uint32_t)((ga - 1) << 9) + lane8)) = make_int2(kDeadPair, kDeadPair);
		if (kEpoch ? (st & (1u << 25)) != 0 : wave == (gb + 1) % NW) *(int2*)(rown + ((uint32_t)((gb + 1) << 9) + lane8)) = make_int2(kDeadPair, kDeadPair);
#if MWF_B2_TIMING == 2
#ifndef MWF_B2_TIMED_CHUNK
#define MWF_B2_TIMED_CHUNK 0 // which of the wave's running chunks of a penalty is timed: 0 the first, 1 the second (zeros where the wave runs fewer)
#endif
		int chunks_seen = 0;
		uint32_t ct[4] = {0, 0, 0, 0};
#endif
#pragma unroll
		for (int k = 0; k < K; ++k) {
			// the slot's class: one bit test and one branch for a slot with nothing to do; an ageing slot runs through the ordinary code
			const uint32_t cls = st >> (4 * k);
			if (kEpoch) {
				if (!(cls & 1u)) continue; // uniform
			} else if (!act[k]) {
				if (idle[k] >= kAgeOut) continue; // uniform
				++idle[k];
			} else idle[k] = 0;
			const bool edgy = (cls & 0xeu) != 0; // uniform: holds a window edge or lies outside the window — every other running chunk is interior, ga < g < gb
			// (the window bounds are laundered per slot: what the chunk code derives from them stays inside this branch instead of being
			// computed up front by waves that hold no active chunk)
			int32_t lo = uni(lo_p), hi = uni(hi_p);
			asm volatile("" : "+s"(lo), "+s"(hi));
			const int32_t g = gk[k], cb = g * kChunk, c0 = cb + 4 * lane;
			// ---- rows: H at the three lags (one 8-byte load each) and the word next to the chunk for the two gap-open rows
#if MWF_B2_TIMING == 2
			uint64_t tc0 = 0, tc1 = 0, tc2 = 0, tc3 = 0, tc4 = 0;
			const bool timed = chunks_seen++ == MWF_B2_TIMED_CHUNK;
			if (timed) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tc0) :: "memory");
#endif
			const uint32_t off = (uint32_t)(cb << 1) + lane8;
			// (measured and dropped, round 4: the rows of EVERY chunk the wave will run requested at the top of the penalty — 16 more VGPRs — 19.4 against 17.35 ms)
			load_rows(pre, rowx, row1, row2, off);
			const int2 HX = pre.HX, O1 = pre.O1, O2 = pre.O2;
			const int32_t N1 = pre.N1, N2 = pre.N2;
			// gap-extension sources: E of column c-1, F of column c+1, e1 (e2) penalties ago; lane 0 / lane 63 take the neighbouring
			// slot's outer columns from the edge table
			const int32_t xE1 = *(const int32_t*)(lds2 + rE1 + k * NW * 16), xE2 = *(const int32_t*)(lds2 + rE2 + k * NW * 16 + 4);
			const int32_t xF1 = *(const int32_t*)(lds2 + rE1 + (k * NW + 2) * 16 + 8), xF2 = *(const int32_t*)(lds2 + rE2 + (k * NW + 2) * 16 + 12);
			const bool inside = (kEpoch && !edgy) || (cb >= lo && cb + kChunk - 1 <= hi); // uniform: every column of the chunk belongs to the window (an interior chunk's do by definition)

			// ---- recurrence (dev::wf_cell, miniwfa.c:267-278) on pairs of columns
			const int32_t E1a = e1h[P1][k][0], E1b = e1h[P1][k][1], F1a = f1h[P1][k][0], F1b = f1h[P1][k][1];
			const int32_t E2a = e2h[P2][k][0], E2b = e2h[P2][k][1], F2a = f2h[P2][k][0], F2b = f2h[P2][k][1];
			const int32_t o1mA = FOLD ? 0 : left_of_A(O1.y, N1), o2mA = kFold2 ? 0 : left_of_A(O2.y, N2), g1mA = left_of_A(E1b, xE1), g2mA = left_of_A(E2b, xE2);
			const int32_t o1pB = FOLD ? 0 : right_of_B(O1.x, N1), o2pB = kFold2 ? 0 : right_of_B(O2.x, N2), g1pB = right_of_B(F1a, xF1), g2pB = right_of_B(F2a, xF2);
			const int32_t ONE = 0x00010001;
			// (FOLD: the E1 / F1 registers already hold the maximum with the row the gap opens from; kFold2: the E2 / F2 registers too)
			int32_t ne1A = FOLD ? g1mA : pk_max(o1mA, g1mA), ne2A = kFold2 ? g2mA : pk_max(o2mA, g2mA);
			int32_t ne1B = FOLD ? E1a : pk_max(O1.x, E1a), ne2B = kFold2 ? E2a : pk_max(O2.x, E2a);
			const int32_t pf1A = FOLD ? F1b : pk_max(O1.y, F1b), pf2A = kFold2 ? F2b : pk_max(O2.y, F2b); // F before its + 1
			const int32_t pf1B = FOLD ? g1pB : pk_max(o1pB, g1pB), pf2B = kFold2 ? g2pB : pk_max(o2pB, g2pB);
			int32_t nf1A = pk_add(pf1A, ONE), nf2A = pk_add(pf2A, ONE), nf1B = pk_add(pf1B, ONE), nf2B = pk_add(pf2B, ONE);
			const int32_t mA = pk_add(HX.x, ONE), mB = pk_add(HX.y, ONE);
			// (kChain: the four partial maxima first, then the two last ones — one VALU instruction between the halves' last maxima, so that neither follows the
			// packed instruction it depends on directly: the hazard nop between A's last two maxima is gone; checked in the assembly, 4 -> 3 s_nop per chunk)
			int32_t hA, hB;
			if (kChain) {
				const int32_t gA = pk_max(mA, pk_max(ne1A, ne2A)), gB = pk_max(mB, pk_max(ne1B, ne2B)), fA = pk_max(nf1A, nf2A), fB = pk_max(nf1B, nf2B);
				__builtin_amdgcn_sched_group_barrier(0x2, 1, 0);
				hA = pk_max(gA, fA), hB = pk_max(gB, fB);
			} else {
				hA = pk_max(pk_max(mA, pk_max(ne1A, ne2A)), pk_max(nf1A, nf2A));
				hB = pk_max(pk_max(mB, pk_max(ne1B, ne2B)), pk_max(nf1B, nf2B));
			}
#if MWF_B2_TIMING == 2
			if (timed) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tc1) : "v"(hA), "v"(hB) : "memory");
#endif
			uint32_t tbw = 0;
			if (TB) {
				// The byte from the RESULTS (miniwfa.c:289-306): H is the maximum of m, e1, e2, f1, f2 and the reference's tie-breaking
				// (mismatch, then E1, E2, F1, F2 = codes 0, 1, 3, 2, 4) is the first of them that equals it; a gap state was extended iff it
				// differs from what opening it would have given.  n* = 1 where different: z = nm (1 + ne1 (2 + ne2 (2 nf1 - 1))).
				const int32_t TWO = 0x00020002, NEG1 = (int32_t)0xffffffffu, EIGHT = 0x00080008, C16 = 0x00100010, C32 = 0x00200020, C64 = 0x00400040;
				int32_t zA = pk_mad(pk_ne1(hA, nf1A), TWO, NEG1), zB = pk_mad(pk_ne1(hB, nf1B), TWO, NEG1);
				zA = pk_mad(pk_ne1(hA, ne2A), zA, TWO), zB = pk_mad(pk_ne1(hB, ne2B), zB, TWO);
				zA = pk_mad(pk_ne1(hA, ne1A), zA, ONE), zB = pk_mad(pk_ne1(hB, ne1B), zB, ONE);
				zA = pk_mad(pk_ne1(hA, mA), zA, 0), zB = pk_mad(pk_ne1(hB, mB), zB, 0);
				if (!FOLD) {
					zA = pk_mad(pk_ne1(ne1A, o1mA), EIGHT, zA), zB = pk_mad(pk_ne1(ne1B, O1.x), EIGHT, zB);
					zA = pk_mad(pk_ne1(pf1A, O1.y), C16, zA), zB = pk_mad(pk_ne1(pf1B, o1pB), C16, zB);
				}
				zA = pk_mad(pk_ne1(ne2A, o2mA), C32, zA), zB = pk_mad(pk_ne1(ne2B, O2.x), C32, zB);
				zA = pk_mad(pk_ne1(pf2A, O2.y), C64, zA), zB = pk_mad(pk_ne1(pf2B, o2pB), C64, zB);
				tbw = (uint32_t)zA | ((uint32_t)zB << 8); // bytes in column order: c0 = A.lo, c1 = B.lo, c2 = A.hi, c3 = B.hi
			}
			// ---- lane geometry of the chunk: j = k + 1 may reach rj = min(tl, ql - d); query index = j + d, d = c - 1 - tl
			const int32_t cbp = both16(cb);
			const int32_t xA = pk_sub(pk_sub(T0, cbp), RA);                  // ql - d of A's columns (garbage beyond cmax, where H is dead)
			// (the table form: ql - d clamped at zero, so that a column beyond cmax probes query position d <= ql + 255 — inside the table — and not tl + d.
			// Both subtractions saturate: a running chunk has cb <= cmax today — hi <= cmax, an ageing slot was in the window once, the remap waits for it to
			// age out — but the probe's bounds must not rest on that: a chunk beyond cmax gets rj = 0 like a column beyond it, not a wrapped difference)
			const int32_t xAc = TAB ? pk_subsat(pk_subsat(T0, cbp), RA) : xA;
			const int32_t rjA = kGeo ? grjA[k] : pk_minu(xAc, TLp), rjB = kGeo ? grjB[k] : pk_minu(TAB ? pk_subsat(xAc, ONE) : pk_sub(xA, ONE), TLp);
			// (the table form: the query's table index is j + c + 1, no target length in it)
			const int32_t dA = kGeo ? gdA[k] : TAB ? pk_add(pk_add(RA, cbp), ONE) : pk_sub(pk_add(RA, cbp), TL1), dB = pk_add(dA, ONE);
			// ---- the rare work in front of the extension — the chunk sticks out of the window, holds a window edge, a shrink is near — behind ONE
			// uniform test: an interior chunk (most chunks) pays one branch for the three (a uniform branch costs a wave 17-31 cycles,
			// profiles/r05/branch_rates_microbench.txt): 1024 x 10 kb -2 % score-only, -3 % with CIGAR.  (The rare work behind the extension — end
			// cell, good-bit words, flag word — under the same test as well: no further gain, seven more spilled SGPRs; left as it was.)
			// (not in the span geometry and the score-only five / six-slot copies on biased offsets: that much slot state leaves no scalar register for the
			// flag — 1250 x 50 kb +1.6 %, 1024 x 15 kb +1.7 %; with CIGAR the biased copies gain 2 % like the rest)
			const bool on_lo = kEpoch ? (cls & 2u) != 0 : g == ga, on_hi = kEpoch ? (cls & 4u) != 0 : g == gb; // uniform
			const bool special = is_span(T, K) || (BI4 && !TB) || (kEpoch ? edgy : !inside || on_lo || on_hi) || track_good; // (!inside implies edgy)
			// ---- a chunk that sticks out of the window: the columns outside are not computed by the reference — dead
			int32_t outA = 0, outB = 0; // 0xffff in the halves of columns outside [lo, hi]
			uint32_t bits = 0, gbits = 0;
			if (MWF_RARE(special)) { // uniform
			if (MWF_RARE(!inside)) { // uniform
				const int32_t lo_r = both16(min(max(lo - cb, 0), 256)), hi_r1 = both16(min(max(hi - cb + 1, 0), 256));
				const int32_t RB = pk_add(RA, 0x00010001), RB1 = pk_add(RA, 0x00020002);
				outA = pk_nonzero_mask(pk_subsat(lo_r, RA) | pk_subsat(RB, hi_r1));
				outB = pk_nonzero_mask(pk_subsat(lo_r, RB) | pk_subsat(RB1, hi_r1));
				hA = bfi(outA, kDeadPair, hA), hB = bfi(outB, kDeadPair, hB);
				ne1A = bfi(outA, kDeadPair, ne1A), ne1B = bfi(outB, kDeadPair, ne1B);
				ne2A = bfi(outA, kDeadPair, ne2A), ne2B = bfi(outB, kDeadPair, ne2B);
				nf1A = bfi(outA, kDeadPair, nf1A), nf1B = bfi(outB, kDeadPair, nf1B);
				nf2A = bfi(outA, kDeadPair, nf2A), nf2B = bfi(outB, kDeadPair, nf2B);
			}
			// ---- edge rule (miniwfa.c:325-326): H is the max of the five, so "any live" == "H live"; one lane holds the edge column
			if (on_lo || on_hi) { // uniform
				if (on_lo) {
					const int32_t rel = lo - cb;
					const int32_t v = half_of(__builtin_amdgcn_readlane((rel & 1) ? hB : hA, rel >> 2), (rel >> 1) & 1);
					bits |= v >= -1 - B ? 1u : 0u;
				}
				if (on_hi) {
					const int32_t rel = hi - cb;
					const int32_t v = half_of(__builtin_amdgcn_readlane((rel & 1) ? hB : hA, rel >> 2), (rel >> 1) & 1);
					bits |= v >= -1 - B ? 2u : 0u;
				}
			}
			// good bits: some array holds an in-matrix offset (miniwfa.c:139-142) <=> j <= rj for a live value (dead: j is huge)
			if (track_good) { // uniform
				auto bad = [&](int32_t v, int32_t rj) { return pk_subsat(pk_add(v, ONEB), rj); }; // zero iff good
				const int32_t bA = pk_minu(pk_minu(bad(hA, rjA), pk_minu(bad(ne1A, rjA), bad(nf1A, rjA))), pk_minu(bad(ne2A, rjA), bad(nf2A, rjA))) | outA;
				const int32_t bB = pk_minu(pk_minu(bad(hB, rjB), pk_minu(bad(ne1B, rjB), bad(nf1B, rjB))), pk_minu(bad(ne2B, rjB), bad(nf2B, rjB))) | outB;
				gbits = (uint32_t)((bA & 0xffff) == 0) | (uint32_t)((bB & 0xffff) == 0) << 1 | (uint32_t)(((uint32_t)bA >> 16) == 0) << 2 | (uint32_t)(((uint32_t)bB >> 16) == 0) << 3;
				if (BI && (s_new & 255) == 0) { // uniform: the range checks of wide_bias
					const int32_t width = both16(kBiasMargin), from = both16(-1 - B - kBiasMargin), top = both16(32768 - kBiasMargin);
					auto stray = [&](int32_t v, int32_t lo_end) { return pk_subsat(width, pk_sub(v, lo_end)); }; // nonzero iff lo_end <= v < lo_end + kBiasMargin
					const int32_t any = stray(hA, from) | stray(hB, from) | stray(ne1A, from) | stray(ne1B, from) | stray(ne2A, from) | stray(ne2B, from) |
					                    stray(nf1A, from) | stray(nf1B, from) | stray(nf2A, from) | stray(nf2B, from) | stray(hA, top) | stray(hB, top);
					if (__ballot(any != 0)) bits |= 0x80u;
				}
			}
			if (kLeanTail && bits != 0 && lane == 0) atomicOr((unsigned int*)&sh.flags[npar][0], bits); // (bits is uniform)
			} // special
			// ---- the new E/F are final: age the registers, publish this chunk's outer columns for the neighbouring slots
			if (FOLD) { // with the row read for the mismatch term: what the gap opens from e1 penalties from now (HX is not masked: it is dead outside ITS window)
				ne1A = pk_max(ne1A, HX.x), ne1B = pk_max(ne1B, HX.y), nf1A = pk_max(nf1A, HX.x), nf1B = pk_max(nf1B, HX.y);
				if (TB) { // the forward bits: this cell's E1 / F1 (dead outside the window) exceed the H a gap would be opened from
					const int32_t EIGHT = 0x00080008, C16 = 0x00100010;
					const int32_t fA = pk_mad(pk_ne1(ne1A, HX.x), EIGHT, pk_mad(pk_ne1(nf1A, HX.x), C16, 0));
					const int32_t fB = pk_mad(pk_ne1(ne1B, HX.y), EIGHT, pk_mad(pk_ne1(nf1B, HX.y), C16, 0));
					tbw |= (uint32_t)fA | ((uint32_t)fB << 8);
				}
			}
			// (kFold2: the second piece's registers are folded, written and published behind the first probe, below)
			e1h[P1][k][0] = ne1A, e1h[P1][k][1] = ne1B, f1h[P1][k][0] = nf1A, f1h[P1][k][1] = nf1B;
			if (!kFold2) e2h[P2][k][0] = ne2A, e2h[P2][k][1] = ne2B, f2h[P2][k][0] = nf2A, f2h[P2][k][1] = nf2B;
#pragma unroll
			for (int i = 0; i < 2; ++i) {
#pragma unroll
				for (int a = E1 - 1; a > 0; --a) {
					asm volatile("v_swap_b32 %0, %1" : "+v"(e1h[a - 1][k][i]), "+v"(e1h[a][k][i]));
					asm volatile("v_swap_b32 %0, %1" : "+v"(f1h[a - 1][k][i]), "+v"(f1h[a][k][i]));
				}
#pragma unroll
				for (int a = E2 - 1; a > 0; --a) {
					asm volatile("v_swap_b32 %0, %1" : "+v"(e2h[a - 1][k][i]), "+v"(e2h[a][k][i]));
					asm volatile("v_swap_b32 %0, %1" : "+v"(f2h[a - 1][k][i]), "+v"(f2h[a][k][i]));
				}
			}
			if (kFold2) put_edge_half(k, 0, ne1B, nf1A); // (the second piece's halves follow behind the probe)
			else put_edge(k, ne1B, ne2B, nf1A, nf2A);

#if MWF_B2_TIMING == 2
			if (timed) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tc2) : "v"(hA), "v"(hB), "v"(rjA), "v"(dA) : "memory");
#endif
			// ---- match extension, first probe (FULL bases): j clamped to rj makes room = rj - j zero for dead and phantom offsets
			const int32_t jA = pk_minu(pk_add(hA, ONEB), rjA), jB = pk_minu(pk_add(hB, ONEB), rjB);
			const int32_t iqA = pk_add(jA, dA), iqB = pk_add(jB, dB);
			int32_t cnt[4]; // columns c0 (A.lo), c1 (B.lo), c2 (A.hi), c3 (B.hi)
			if (TAB) {
				// Eight halfword reads — table entries j and j + c + 1 of the four columns — back to back and waited for once, as below.  A half of the
				// packed registers becomes a byte address by adding it to itself (SDWA); the table starts at LDS address 0.  j <= rj <= tl and
				// j + c + 1 <= tl + ql + 257: every address lies inside the table.
				uint32_t tv[4], qv[4];
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const uint32_t J = (uint32_t)((u & 1) ? jB : jA), Q = (uint32_t)((u & 1) ? iqB : iqA);
					uint32_t ta, qa;
					if (u & 2) {
						asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(ta) : "v"(J));
						asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(qa) : "v"(Q));
					} else {
						asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_0" : "=v"(ta) : "v"(J));
						asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_0" : "=v"(qa) : "v"(Q));
					}
					asm volatile("ds_read_u16 %0, %1" : "=v"(tv[u]) : "v"(ta));
					asm volatile("ds_read_u16 %0, %1" : "=v"(qv[u]) : "v"(qa));
				}
				asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(qv[0]), "+v"(qv[1]), "+v"(qv[2]), "+v"(qv[3]));
#pragma unroll
				for (int u = 0; u < 4; ++u) asm("v_ffbl_b32 %0, %1" : "=v"(cnt[u]) : "v"(tv[u] ^ qv[u])); // first differing bit, -1 for none: halved after packing (below)
			} else if (S2) {
				// Eight LDS reads (two dwords of each sequence for each of the four columns) go out back to back and are waited for ONCE:
				// left to itself the compiler recycles one register quad and pays four dependent LDS round trips.  Inline asm: the
				// reads keep their order (volatile), the single wait takes every result as an operand so that no use can move above it.
				// (Addresses are LDS byte addresses: the dynamic LDS of this kernel starts at 0 — it has no static LDS.)
				uint64_t tw[4], qw[4];
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const uint32_t J = (uint32_t)((u & 1) ? jB : jA), Q = (uint32_t)((u & 1) ? iqB : iqA);
					// (the 4-bit form: dword (j >> 3), byte address (j >> 3) << 2 — up to 31 000 for the 62 000 bases of the span geometry: it fits the half)
					const uint32_t ta = kNib ? ((u & 2) ? (J >> 17) & 0x7ffcu : (J >> 1) & 0x7ffcu) : (u & 2) ? (J >> 18) & 0x3ffcu : (J >> 2) & 0x3ffcu;
					const uint32_t qa = (kNib ? ((u & 2) ? (Q >> 19) : ((Q >> 3) & 0x1fffu)) : ((u & 2) ? (Q >> 20) : ((Q >> 4) & 0xfffu))) * 4u + (uint32_t)qoff;
					asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(tw[u]) : "v"(ta));
					asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=v"(qw[u]) : "v"(qa));
				}
				asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tw[0]), "+v"(tw[1]), "+v"(tw[2]), "+v"(tw[3]), "+v"(qw[0]), "+v"(qw[1]), "+v"(qw[2]), "+v"(qw[3]));
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const uint32_t J = (uint32_t)((u & 1) ? jB : jA), Q = (uint32_t)((u & 1) ? iqB : iqA);
					// v_alignbit uses bits 4:0 of the shift.  Bit 15 of the LOW half must not leak into a high half's shift: j never has it (j <= rj <=
					// tl < 32767), a query index can — column 0 (the pad column, lane 0 of chunk 0) clamps to index -1
					// (biased offsets: targets beyond 32 kb — j has a bit 15 too)
					// (the 4-bit form: the shift is (j & 7) * 4; bits 14 AND 15 of the low half would land in a high half's shift, and j has a bit 14 from 16 384 on: masked always)
					const uint32_t tsh = kNib ? ((u & 2) ? (J >> 14) & 28u : J << 2) : (u & 2) ? (BI ? (J >> 15) & 30u : J >> 15) : J << 1;
					const uint32_t qsh = kNib ? ((u & 2) ? (Q >> 14) & 28u : Q << 2) : (u & 2) ? (Q >> 15) & 30u : Q << 1;
					cnt[u] = lead_eq2(__builtin_amdgcn_alignbit((uint32_t)(tw[u] >> 32), (uint32_t)tw[u], tsh) ^ __builtin_amdgcn_alignbit((uint32_t)(qw[u] >> 32), (uint32_t)qw[u], qsh));
				}
			} else {
				// six probe words per column: two columns in flight (one where three slots of state must fit 128 VGPRs)
				constexpr int PF = (K >= 3 && T >= 512) ? 1 : 2;
#pragma unroll
				for (int h2 = 0; h2 < 4 / PF; ++h2) {
					Probe8 pr[PF];
					int32_t jj[PF], aq[PF];
#pragma unroll
					for (int v = 0; v < PF; ++v) {
						const int u = PF * h2 + v;
						jj[v] = (int32_t)((uint32_t)((u & 1) ? jB : jA) >> ((u & 2) ? 16 : 0) & 0xffffu);
						aq[v] = (int32_t)((uint32_t)((u & 1) ? iqB : iqA) >> ((u & 2) ? 16 : 0) & 0xffffu) + qoff;
						probe8_issue(pr[v], jj[v], aq[v]);
					}
#pragma unroll
					for (int v = 0; v < PF; ++v) cnt[PF * h2 + v] = probe8_count(pr[v], jj[v], aq[v]);
				}
			}
			typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
			int32_t cA = MWF_BC(int32_t, (us2_t)__builtin_amdgcn_cvt_pk_u16((uint32_t)cnt[0], (uint32_t)cnt[2])); // saturating
			int32_t cB = MWF_BC(int32_t, (us2_t)__builtin_amdgcn_cvt_pk_u16((uint32_t)cnt[1], (uint32_t)cnt[3]));
			if (TAB) cA = MWF_BC(int32_t, (us2_t)(MWF_BC(us2_t, cA) >> 1)), cB = MWF_BC(int32_t, (us2_t)(MWF_BC(us2_t, cB) >> 1)); // bits -> bases; "no difference" (0xffff) stays above FULL
			if (kFold2) { // the second fold: with the row of lag o2, what the second piece opens from e2 = 1 penalty from now; unmasked like HX (dead outside ITS window).
				// Masks, good bits and the edge rule saw the values before the fold; the registers and the edge table take the folded ones.  First use of O2.
				int32_t px = O2.x, py = O2.y;
				asm volatile("" : "+v"(px), "+v"(py)); // (volatile: stays behind the probe's wait, and the wait for the row with it)
				ne2A = pk_max(ne2A, px), ne2B = pk_max(ne2B, py), nf2A = pk_max(nf2A, px), nf2B = pk_max(nf2B, py);
				e2h[P2][k][0] = ne2A, e2h[P2][k][1] = ne2B, f2h[P2][k][0] = nf2A, f2h[P2][k][1] = nf2B;
				put_edge_half(k, 1, ne2B, nf2A);
			}
#if MWF_B2_TIMING == 2
			if (timed) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tc3) : "v"(cA), "v"(cB) : "memory");
#endif
			const int32_t FULLp = both16(FULL);
			const int32_t m9A = pk_minu(cA, pk_sub(rjA, jA)), m9B = pk_minu(cB, pk_sub(rjB, jB)); // > FULL: the whole probe matched, room left
			int32_t nmA = pk_minu(m9A, FULLp), nmB = pk_minu(m9B, FULLp);
			const int32_t pendp = pk_subsat(m9A, FULLp) | pk_subsat(m9B, FULLp);
			// ---- a run of >= FULL matches continues (the cells near the alignment path, and one first probe in 4^FULL by chance).  Each
			// lane first walks its own runs, four trips at most; what is still open then the whole wave walks.
			if (MWF_RARE(__ballot(pendp != 0) != 0)) {
				const int32_t tb0 = TAB ? fresh(A).band_lds_tab : 0; // where the target's 2-bit copy starts
				int32_t hv[4] = {half_of(hA, 0) + B, half_of(hB, 0) + B, half_of(hA, 1) + B, half_of(hB, 1) + B}; // true offsets
				int32_t nmat[4] = {(int32_t)((uint32_t)nmA & 0xffffu), (int32_t)((uint32_t)nmB & 0xffffu), (int32_t)((uint32_t)nmA >> 16), (int32_t)((uint32_t)nmB >> 16)};
				const uint32_t pend = (uint32_t)(((uint32_t)m9A & 0xffffu) > (uint32_t)FULL) | (uint32_t)(((uint32_t)m9B & 0xffffu) > (uint32_t)FULL) << 1 |
				                      (uint32_t)(((uint32_t)m9A >> 16) > (uint32_t)FULL) << 2 | (uint32_t)(((uint32_t)m9B >> 16) > (uint32_t)FULL) << 3;
				uint32_t open = 0;
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					if (__ballot((pend >> i) & 1u) == 0) continue; // uniform
					if ((pend >> i) & 1u) {
						int32_t n = FULL; // pend is only set for a full first probe of an in-matrix cell with room left
						const int32_t j = hv[i] + 1, q = c0 + i - 1 - tl + j, rm = min(tl - j, ql - q), aqq = qoff + q;
						for (int trip = 0; n < rm; ++trip) {
							if (trip == 4) { open |= 1u << i; break; }
							if (S2) {
								const int32_t m = min(lead_eq2(seq16(tb0, j + n) ^ seq16(qoff, q + n)), kSeqPer);
								n += m;
								if (m < kSeqPer) break;
							} else {
								const uint32_t xa = seq4(j + n) ^ seq4(aqq + n), xb = seq4(j + n + 4) ^ seq4(aqq + n + 4);
								if (xa | xb) { n += xa ? min(lead_eq(xa), 4) : 4 + min(lead_eq(xb), 4); break; }
								n += 8;
							}
						}
						nmat[i] = min(n, rm);
					}
				}
				for (unsigned long long owners = __ballot(open != 0); owners; owners &= owners - 1) {
					const int32_t src = (int32_t)__builtin_ctzll(owners);
					const int32_t c0s = cb + 4 * src;
					const uint32_t ob = (uint32_t)__builtin_amdgcn_readlane((int32_t)open, src);
#pragma unroll
					for (int i = 0; i < 4; ++i) {
						if (!((ob >> i) & 1u)) continue; // uniform
						const int32_t hh = __builtin_amdgcn_readlane(hv[i], src);
						const int32_t j = hh + 1, q = c0s + i - 1 - tl + j, rm = min(tl - j, ql - q);
						const int32_t n = S2 ? run_wave16(qoff, j, q, rm, FULL + 4 * kSeqPer, tb0) : run_wave2(j, qoff + q, rm, 40);
						nmat[i] = lane == src ? n : nmat[i];
					}
				}
				nmA = pair_of(nmat[0], nmat[2]), nmB = pair_of(nmat[1], nmat[3]);
			}
			const int32_t hxA = pk_add(hA, nmA), hxB = pk_add(hB, nmB); // extended
			if (forecast) far = pk_max(far, pk_max(hxA, hxB));
			// ---- termination test of the extension sweep (miniwfa.c:405-409): only column ql+1 can hold the end cell
			unsigned long long fm = 0;
			int32_t done_info = 0;
			// (kChain: two levels — the slot's bit in est says that the chunk holds the column at all, and only such a chunk compares it with the window: one bit test
			// on every other chunk's path instead of three compares)
			bool end_bit = false;
			if constexpr (kLeanTail) end_bit = MWF_RARE((st & (1u << (26 + k))) != 0) && cfin >= lo && cfin <= hi;
			if (MWF_RARE(kLeanTail ? end_bit : (uint32_t)(cfin - cb) < (uint32_t)kChunk && cfin >= lo && cfin <= hi)) { // uniform
				const int32_t rel = cfin - cb, hi_half = (rel >> 1) & 1;
				const int32_t hv = half_of((rel & 1) ? hxB : hxA, hi_half) + B, nm = (int32_t)((uint32_t)((rel & 1) ? nmB : nmA) >> (hi_half ? 16 : 0) & 0xffffu);
				const uint32_t f = (uint32_t)(lane == (rel >> 2)) & (uint32_t)(hv == tl - 1) & inm_bit(ql - tl, hv - nm, tl, ql);
				done_info = (f && nm == 0) ? (int32_t)((tbw >> (8 * (rel & 3))) & 7u) : 0;
				fm = __ballot(f != 0);
				// (kChain: the flag word gets the end cell's bits here and a window edge's in the block above — the only places they can come from — so that a chunk
				// that is neither tests nothing behind its store)
				if (kLeanTail && fm) {
					const uint32_t fin = 4u | (uint32_t)__builtin_amdgcn_readlane(done_info, (int32_t)__builtin_ctzll(fm)) << 4;
					if (lane == 0) atomicOr((unsigned int*)&sh.flags[npar][0], fin);
				}
			}
			*(int2*)(rown + off) = make_int2(hxA, hxB);
			if (!kLeanTail) ++n_stores;
#if MWF_B2_TIMING == 2
			if (timed) {
				asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tc4) : "v"(hxA), "v"(hxB) : "memory");
				ct[0] = (uint32_t)min(tc1 - tc0, (uint64_t)4095), ct[1] = (uint32_t)min(tc2 - tc1, (uint64_t)4095);
				ct[2] = (uint32_t)min(tc3 - tc2, (uint64_t)4095), ct[3] = (uint32_t)min(tc4 - tc3, (uint64_t)4095);
			}
#endif
			if (TB && c0 >= origin && c0 <= hi) *(uint32_t*)(M.tb + tb_used - origin + c0) = tbw;
			if (MWF_RARE(track_good)) {
				unsigned long long *gword = M.good + (int64_t)newH * fresh(A).GW + g * 4;
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const unsigned long long m = __ballot((gbits >> i) & 1u);
					if (lane == 0) gword[i] = m;
				}
			}
			if (!kLeanTail) {
				if (fm) bits |= 4u | (uint32_t)__builtin_amdgcn_readlane(done_info, (int32_t)__builtin_ctzll(fm)) << 4;
				if (kChain) { // (bits is uniform: a scalar test that falls through instead of an exec mask and a taken branch)
					if (MWF_RARE(bits != 0))
						if (lane == 0) atomicOr((unsigned int*)&sh.flags[npar][0], bits);
				} else if (bits && lane == 0) atomicOr((unsigned int*)&sh.flags[npar][0], bits);
			}
		}

		if (forecast) {
			const int32_t m = wave_max(max(lo16(far), hi16(far))) + B;
			if (lane == 0 && m >= 0) atomicMax(&sh.word[3], m);
		}
		// Everything older than this penalty's last operations must be complete before another wave may load it (vmcnt retires
		// in issue order).  With every lag >= 3 the rows written now are first loaded two penalties from now: the youngest store
		// may stay in flight across the barrier.
#ifdef MWF_B2_TIMING
		const uint64_t tm2 = __builtin_readcyclecounter();
#endif
		// the coming penalty: its rows, and the request for the first active chunk's (five loads, younger than every store)
		if constexpr (!kChain) { // (kChain: behind the barrier, while the flag word is on its way)
			bn = bn + RS == ring_bytes ? 0u : bn + RS, bx = bx + RS == ring_bytes ? 0u : bx + RS;
			b1 = b1 + RS == ring_bytes ? 0u : b1 + RS, b2 = b2 + RS == ring_bytes ? 0u : b2 + RS;
		}
		// (the table form: "some slot of this wave stored a row" is a function of the slot classes — a chunk that runs stores — not a counter kept by every chunk)
		const bool young_store = relaxed_stores && (kLeanTail ? (st & kRunBits) != 0 : n_stores > 0) && !TB && !track_good;
		if (young_store) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
		else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#ifdef MWF_B2_TIMING
		const uint64_t tm3 = __builtin_readcyclecounter();
#endif
		__builtin_amdgcn_s_barrier();
		asm volatile("" ::: "memory");

		// ---- bookkeeping, identical on every thread
		// (kChain: the read of the flag word is issued here and waited for behind everything that does not depend on it — the row offsets, the penalty's counters, the
		// edge-table rotation, the slot mapping; the wait stood one instruction behind the read, a whole LDS round trip on every wave's path behind the barrier)
		uint32_t fl = 0;
		int32_t flv = 0;
		if constexpr (kChain) {
			static_assert(!kChain || !BI, "the range checks of the biased offsets leave before the penalty turns");
			asm volatile("ds_read_b32 %0, %1" : "=v"(flv) : "v"((uint32_t)(uintptr_t)&sh.flags[npar][0]) : "memory");
			bn = bn + RS == ring_bytes ? 0u : bn + RS, bx = bx + RS == ring_bytes ? 0u : bx + RS;
			b1 = b1 + RS == ring_bytes ? 0u : b1 + RS, b2 = b2 + RS == ring_bytes ? 0u : b2 + RS;
		} else fl = (uint32_t)uni(sh.flags[npar][0]);
#ifdef MWF_B2_TIMING
		if (trace_band && tid == (fresh(A).max_iter < 0 ? (int32_t)-fresh(A).max_iter : 0) && s_new - 1 < fresh(A).dbg_cap) { // cycles: header | chunks, drain | barrier+flags; chunks this wave ran in bits 28..
			const uint64_t tm4 = __builtin_readcyclecounter();
#if MWF_B2_TIMING == 2 // the first active chunk of the wave: rows + recurrence | masks, liveness, geometry, edge stores | first probe | walks, store
			M.dbg[2 * (s_new - 1)] = (int32_t)(ct[0] | ct[1] << 12 | (uint32_t)n_act << 28);
			M.dbg[2 * (s_new - 1) + 1] = (int32_t)(ct[2] | ct[3] << 12);
			(void)tm4;
#else
			M.dbg[2 * (s_new - 1)] = (int32_t)(min((uint32_t)(tm1 - tm0), 65535u) | min((uint32_t)(tm2 - tm1), 65535u) << 16);
			M.dbg[2 * (s_new - 1) + 1] = (int32_t)(min((uint32_t)(tm3 - tm2), 4095u) | min((uint32_t)(tm4 - tm3), 65535u) << 12 | (uint32_t)n_act << 28);
#endif
		}
#endif
		int32_t done = 0, payload = 0;
		if constexpr (!kChain) {
			if (fl & 1u) wf_lo = lo;
			if (fl & 2u) wf_hi = hi;
			done = (int32_t)((fl >> 2) & 1u), payload = (int32_t)((fl >> 4) & 7u);
			if (BI && (fl & 0x80u)) { R.status = ST_BAND_OVERFLOW; return true; } // a value came near the end of its 16-bit range (wide_bias)
		}
		s = s_new, curH = newH, par = npar;
		{
			const int32_t oldest = epos[D - 1];
#pragma unroll
			for (int a = D - 1; a > 0; --a) epos[a] = epos[a - 1];
			epos[0] = oldest;
		}
		// The slot mapping follows the window's start: down at once (the slot that wraps held a chunk beyond the window's reach under the old
		// mapping: long idle), up only when the chunks below the start have been out of the window for kAgeOut penalties — until then
		// they age (and, FOLD, fold the rows they computed) in place.  A slot that wrapped while it aged would run the chunk NWK further up
		// through the ordinary code, and that chunk's dead stores may lie beyond the end of the row (found by profiles/fuzz_fold.py: a
		// 2.3 kb unrelated pair on four slots lost cells of the NEXT row that way — n_iter off by 82).
		// (a penalty that took the fast header has gl_next == gl and up_wait == 0: the key, which is not negative then, says so.  A mapping that moves, or waits to, drops the key.)
		if (!kEpoch || ekey < 0) {
			if (gl_next < gl) gl = gl_next, remap(gl), up_wait = 0, ekey = 0;
			else if (gl_next > gl) {
				up_min = up_wait == 0 ? gl_next : min(up_min, gl_next);
				if (++up_wait > kAgeOut) gl = up_min, remap(gl), up_wait = 0;
				ekey = 0;
			} else up_wait = 0, ekey = ~ekey; // (-1, nothing to keep, becomes 0: no key)
		}
		if (TB) tb_used += row_bytes;
		if constexpr (kChain) {
			asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(flv));
			fl = (uint32_t)__builtin_amdgcn_readfirstlane(flv);
			if (fl & 1u) wf_lo = lo;
			if (fl & 2u) wf_hi = hi;
			done = (int32_t)((fl >> 2) & 1u), payload = (int32_t)((fl >> 4) & 7u);
		}
		if ((s & 0xff) == 0) { // shrink (reference wf_stripe_shrink, miniwfa.c:144-171) on the interleaved good bits
			if (tid == 0) sh.red[0] = 0x7fffffff, sh.red[1] = -1;
			__syncthreads();
			const int32_t gfirst = wf_lo >> 8, n_words = ((wf_hi >> 8) - gfirst + 1) * 4, GWc = fresh(A).GW;
			for (int32_t q = tid; q < n_words; q += T) {
				const int32_t gg = gfirst + (q >> 2), kq = q & 3, base = gg * kChunk;
				unsigned long long m = 0;
				for (int32_t j = 0; j < nH; ++j)
					if (sh.rng_lo[j] <= sh.rng_hi[j] && sh.rng_lo[j] <= base + kChunk - 1 && sh.rng_hi[j] >= base) m |= M.good[(int64_t)j * GWc + gg * 4 + kq];
				m &= lane_mask(base, kq, wf_lo, wf_hi);
				if (m) {
					atomicMin(&sh.red[0], base + 4 * (int32_t)__builtin_ctzll(m) + kq);
					atomicMax(&sh.red[1], base + 4 * (63 - (int32_t)__builtin_clzll(m)) + kq);
				}
			}
			__syncthreads();
			const int32_t glo = uni(sh.red[0]), ghi = uni(sh.red[1]);
			if (ghi < 0) { R.status = ST_INTERNAL; return true; }
			wf_lo = glo, wf_hi = ghi;
		}
		if (kChain) cells -= hi - lo + 1;
		else cells += hi - lo + 1;
		if ((kChain ? cells < 0 : cells > iter_limit) || s > s_limit) { // miniwfa.c:422-425
			R.status = ST_STOPPED;
			return true;
		}
		if (done) {
			R.info = payload;
			return true;
		}
		if (forecast) { // will the window outgrow the chunks this workgroup holds? then hand the pair back now, with the estimate
			est_window = window_forecast(s, uni(sh.word[3]), tl, ql, (NWK - 1) * kChunk - 64, NWK >= 24 && NWK < 64); // (the window this geometry is chosen for: kBand*Window in mwf_plan.cpp)
			if (est_window) { R.status = ST_BAND_OVERFLOW; return true; }
		}
		return false;
	};
	for (;;)
		if (step()) break;
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	if (kChain) cells = (fresh(A).max_iter > 0 ? fresh(A).max_iter : INT64_MAX) - cells;
	R.s = s, R.cells = est_window ? -(int64_t)est_window : cells; // (a pair handed back early: the window it is expected to need, negated, for the host's choice of the next kernel)
	return R;
}
#undef MWF_RARE

// Workgroups share a CU: 2 x 512, 4 x 256, 8 x 128 or 16 x 64 threads = 4 waves per SIMD, i.e. at most 128 VGPRs; with traceback
// the smaller ones get 168 (3 per SIMD).  768 threads: one workgroup per CU.
// (gap extensions of 3 and 4 keep these bounds: profiles/band_deep/band2_deep_registers.txt has what that spills, DESIGN.md section 4.2 what was measured;
// likewise the five / six-slot copies on biased offsets of the sets beyond (2,1): profiles/band_biased/band2_biased_registers.txt)
constexpr int band2_waves(int T, int K, bool TB)
{
	return is_span(T, K) ? (T == 1024 ? 4 : 3) : T == 1024 ? 4 : T == kWideT ? kWideWaves : T <= 512 ? ((TB && T < 512) ? 3 : 4) : kWaves768;
}
template <int T, int K, int E1, int E2, bool TB, bool S2, bool BI4 = false, bool FOLD = false>
__global__ __launch_bounds__(T, band2_waves(T, K, TB)) void MWF_BAND2_KERNEL(const BatchArgs)
{
	constexpr int NWK = (T / 64) * K, D = (E1 > E2 ? E1 : E2) + 1;
	// the arguments are read from the kernarg segment where they are used (dev::kernel_args / dev::fresh), never held for the kernel's lifetime
	KArgs &A0 = kernel_args();
	// the sequence copy starts at LDS offset 0 (the probes' inline-asm reads take LDS byte addresses): true while this kernel has no
	// static LDS — trap rather than compute on the wrong bytes should that ever change
	if ((uint32_t)(uintptr_t)lds2 != 0u) __builtin_trap();
	// the bookkeeping words and the edge table sit behind the sequence copy
	typedef Band2Lds<D, NWK> LdsT;
	const int32_t lds_seq = A0.band_lds_seq;
	LdsT *const L = (LdsT*)(lds2 + lds_seq);
	Shared &sh = L->sh;
	const int32_t edge_base = lds_seq + (int32_t)offsetof(LdsT, edge);
	CigLocal cig_loc;
	cig_loc.base = 0, cig_loc.left = 0;
	for (int32_t round = 0;; ++round) {
		KArgs &A = fresh(A0);
		// a work counter, or — queue == null: a launch of one workgroup per pair — pair blockIdx.x and nothing else (no counter to zero first)
		// (one counter: at the ~3-6 million pairs per second of these geometries its ~12.7 ns per pair do not show — 20 000 x 1 kb 6.2 Gbp/s with the lane
		// kernel's partitioned counters, 6.3 without)
		if (threadIdx.x == 0) sh.item = A.queue ? (int32_t)atomicAdd(A.queue, 1) : (round == 0 ? (int32_t)blockIdx.x : A.n_pairs), sh.word[2] = 0;
		__syncthreads();
		const int32_t item = uni(sh.item);
		__syncthreads();
		if (item >= A.n_pairs) break;
		const int32_t pair = A.order ? A.order[item] : item;
		PairMem M;
		pair_mem(A, (int32_t)blockIdx.x, pair, M);
		constexpr bool TAB = kTabProbe && S2;
		const int32_t toff = TAB ? A.band_lds_tab : 0; // (the table form: the probe table comes first, the 2-bit copies behind it)
		const int32_t qoff = toff + (S2 ? ((M.tl >> kSeqDw) + 2) * 4 : ((M.tl + 3) & ~3) + 8); // both sequences start on a dword
		PassResult R;
		R.status = ST_OK, R.s = 0, R.info = 0, R.n_snap = 0, R.cells = 0;
		if (S2) {
			uint32_t bad = kNib ? pack4bit<T>(M.ts, M.tl, toff) : pack2bit<T>(M.ts, M.tl, toff);
			bad |= kNib ? pack4bit<T>(M.qs, M.ql, qoff) : pack2bit<T>(M.qs, M.ql, qoff);
			// a base other than A/C/G/T: the host re-runs the pair on the byte-wise copy of this kernel
			if (bad) sh.word[2] = 1;
			__syncthreads();
			if (uni(sh.word[2])) R.status = ST_ALPHABET;
			if (TAB) { // (read only behind the barriers in front of the first penalty)
				if (2 * (M.tl + M.ql + kTabSlack) > toff) R.status = ST_BAND_OVERFLOW; // (the host sizes the table for the launch's longest pair)
				else if (R.status == ST_OK) build_probe_table<T>(M.tl, M.ql, toff, qoff);
			}
		} else {
			for (int32_t j = threadIdx.x; j < M.tl; j += T) lds2[j] = M.ts[j];
			for (int32_t j = threadIdx.x; j < M.ql; j += T) lds2[qoff + j] = M.qs[j];
			__syncthreads();
		}
		const bool trace = A.dbg && pair == A.debug_pair;
		if (R.status == ST_OK) R = band2_pass<T, K, E1, E2, TB, S2, BI4, FOLD>(A, M, sh, edge_base, qoff, trace);
		if (T == 512 && K == 4 && R.n_snap && threadIdx.x == 0 && fresh(A0).report_wide) atomicOr((unsigned int*)(fresh(A0).cig_head + 1), 1u); // (mwf_plan.cpp: PlanCache::wide_state)
		R.n_snap = 0;
		if (S2 && !kNib) M.t2 = lds2 + toff, M.q2 = lds2 + qoff; // the traceback's back-match reads the 2-bit copies in LDS (the 4-bit form: the image bytes in the arena)
		if (TB && FOLD) M.tb_fwd = 1;
		finish_pair(fresh(A0), M, (int32_t)blockIdx.x, pair, R, R.status, 0, T <= 256 ? &cig_loc : nullptr); // (block mode: the geometries of the short pairs — thousands per launch)
	}
}

template <int T, int K, int E1, int E2>
constexpr int lds_tail() { return (int)sizeof(Band2Lds<(E1 > E2 ? E1 : E2) + 1, (T / 64) * K>); }

// The folded form (band2_pass: FOLD) is launched for o1 == x, two row loads less per chunk: the one statement of the runtime condition ...
inline bool band2_folds(const Penalty &p, bool band_fold) { return band_fold && p.oe1 - p.x == p.e1 && p.oe1 < kFoldMaxLag; }
// ... and of which instantiations have a folded copy: the 512-thread (and wider) geometries on 2-bit sequence copies with e1 == 2 — the default penalties and
// main.c's -a preset (the byte-wise geometry serves the rare pairs outside plain A/C/G/T, and a folded copy of every kernel for e1 == 1 penalties bought nothing a
// benchmark showed; round 6 pruning: 132 -> 62 kernels in the main object); the 4-bit form folds its score-only kernels alone.
constexpr bool band2_has_folded(int T, int E1, bool TB, bool S2) { return T >= 512 && S2 && E1 == 2 && !(kNib && TB); }
// The table form exists folded only (its units' callers check band2_folds first), so its occupancy is asked of the folded kernel; every other form has each
// instantiation unfolded, and the unfolded kernel answers for both (same registers and LDS: profiles/alpha16/band2_nib_registers.txt).
constexpr bool kFoldedOnly = kTabProbe;

template <int T, int K, int E1, int E2, bool TB, bool S2, bool BI4, bool FOLD>
void launch_kernel(const BatchArgs &a, int grid, int lds, hipStream_t st)
{
	// the attribute is per device and this may run on several host threads (mwf_wfa_batch_multi): set it on every launch that needs it
	if (lds > 48 * 1024) {
		(void)hipFuncSetAttribute(reinterpret_cast<const void*>(&MWF_BAND2_KERNEL<T, K, E1, E2, TB, S2, BI4, FOLD>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
		(void)hipGetLastError();
	}
	// diagnostics: which instantiation this launch is — the eight template arguments, as tests/band_matrix.py lists them — and how many pairs it was given;
	// the table form adds a line of its own, the 4-bit form writes its own instead
	if (getenv("MWF_DEBUG")) {
		if (kNib)
			fprintf(stderr, "[libmwf_hip] band2 nib launch: wfa_band2_nib_kernel T %d K %d E1 %d E2 %d TB %d S2 %d BI4 %d FOLD %d, %d pairs, grid %d, lds %d B\n", T, K, E1, E2, (int)TB, (int)S2, (int)BI4, (int)FOLD, (int)a.n_pairs, grid, lds);
		else
			fprintf(stderr, "[libmwf_hip] band2 launch: T %d K %d E1 %d E2 %d TB %d S2 %d BI4 %d FOLD %d, %d pairs, grid %d\n", T, K, E1, E2, (int)TB, (int)S2, (int)BI4, (int)FOLD, (int)a.n_pairs, grid);
		if (kTabProbe) fprintf(stderr, "[libmwf_hip] band2 table probe: table %d B, lds %d B\n", (int)a.band_lds_tab, lds);
		if (kFold2Form) fprintf(stderr, "[libmwf_hip] band2 second fold: wfa_band2_tab2_kernel, row of lag %d folded one penalty ahead (o2 + e2 %d, bound %d)\n", (int)(a.pen.oe2 - a.pen.e2), (int)a.pen.oe2, kFold2MaxLag);
	}
	hipLaunchKernelGGL((MWF_BAND2_KERNEL<T, K, E1, E2, TB, S2, BI4, FOLD>), dim3(grid), dim3(T), lds, st, a);
}

template <int T, int K, int E1, int E2, bool TB, bool S2, bool BI4 = false>
void launch_variant(const BatchArgs &a, int grid, int lds, hipStream_t st)
{
	if constexpr (kFoldedOnly) return launch_kernel<T, K, E1, E2, TB, S2, BI4, true>(a, grid, lds, st);
	else {
		if constexpr (band2_has_folded(T, E1, TB, S2)) {
			if (band2_folds(a.pen, a.band_fold)) return launch_kernel<T, K, E1, E2, TB, S2, BI4, true>(a, grid, lds, st);
		}
		launch_kernel<T, K, E1, E2, TB, S2, BI4, false>(a, grid, lds, st);
	}
}

template <int T, int K, int E1, int E2, bool TB, bool S2, bool BI4 = false>
int occ_variant(int lds)
{
	int n = 0;
	return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, MWF_BAND2_KERNEL<T, K, E1, E2, TB, S2, BI4, kFoldedOnly>, T, lds) == hipSuccess ? n : 0;
}

// The sequence copy an instantiation reads follows from its geometry: the byte-wise geometry (768 threads) takes every pair outside plain A/C/G/T that the packed
// kernel takes, every other one — 64 ... 512 threads x 3 slots, 512 x 4 and more, the span geometry — exists on 2-bit copies only (the host knows: choose_kernel).
constexpr bool band2_geo_seq2(int T) { return T != 768; }

template <int T, int K, int E1, int E2, bool BI4 = false>
int launch_one(const BatchArgs &a0, int grid, int lds_seq, int lds_tab, bool seq2, hipStream_t st)
{
	constexpr bool S2 = band2_geo_seq2(T);
	if (seq2 != S2) return -1;
	BatchArgs a = a0;
	a.band_lds_seq = lds_seq, a.band_lds_tab = lds_tab; // (the table is read by the table form alone; every other form is launched with lds_tab 0)
	const int lds = lds_seq + lds_tail<T, K, E1, E2>();
	if constexpr (kFold2Form) { // score-only kernels alone: a CIGAR launch is the table form's
		if (a.want_cigar) return -1;
		launch_variant<T, K, E1, E2, false, S2, BI4>(a, grid, lds, st);
	} else {
		if (a.want_cigar) launch_variant<T, K, E1, E2, true, S2, BI4>(a, grid, lds, st);
		else launch_variant<T, K, E1, E2, false, S2, BI4>(a, grid, lds, st);
	}
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int T, int K, int E1, int E2, bool BI4 = false>
int occ_one(int lds_seq, bool seq2, bool tb)
{
	constexpr bool S2 = band2_geo_seq2(T);
	if (seq2 != S2) return 0;
	const int lds = lds_seq + lds_tail<T, K, E1, E2>();
	if constexpr (kFold2Form) return tb ? 0 : occ_variant<T, K, E1, E2, false, S2, BI4>(lds);
	else return tb ? occ_variant<T, K, E1, E2, true, S2, BI4>(lds) : occ_variant<T, K, E1, E2, false, S2, BI4>(lds);
}

} // namespace

} // namespace mwf

