// mwf_ends.hip — ends-free (semi-global) and extension alignment: wfa_ends_kernel<T, EXT>.  The contract is include/miniwfa.h (mwf_ends_t): the cheapest
// global alignment of t[tb, te) against q[qb, qe) where up to t_beg / q_beg bases in front of and t_end / q_end bases behind the aligned
// ranges are free.
//
// The pass is the generic kernel's one-column-per-lane pass (mwf_kernels.hip forward_pass: one workgroup per pair, persistent workgroups
// on a work counter, 32-bit ring rows in the engine's ring pool, traceback bytes in its arena, the same band bookkeeping and n_iter) with
// three differences:
//   * the origin is a window of diagonals [-min(t_beg, tl), min(q_beg, ql)] — H[d] = (d < 0 ? -d : 0) - 1, then extended — which may be
//     wider than the workgroup: penalty 0 takes the same trip loop as every later penalty;
//   * the end rule is tested on every in-matrix H cell after its extension: a cell in the query's last row with at most t_end target
//     bases behind it, or in the target's last column with at most q_end query bases behind it.  The first penalty with such a cell is
//     the answer and the lowest column wins (the order of the reference's sweep): an LDS atomicMin on the column picks it, then the one
//     lane that owns that column publishes its offset and start state;
//   * the traceback starts at that cell and, where it leaves the matrix, clips what the begin allowance covers instead of emitting it.
// With four zero allowances all three reduce to the global pass: s, n_iter and the CIGAR words are those of the generic kernel.
//
// Extension alignment (mwf_ext_t, same header) is the same pass, driver and kernel under a compile-time EXT flag: the allowances are fixed at
// {0, INT32_MAX, 0, INT32_MAX}; every tested cell also forms a = bases consumed and the penalty's largest a (lowest column among equals) goes
// through one 64-bit LDS atomicMax per wave into a slot of the penalty's parity set; after the penalty's barrier the best V = A a - 2 s so far (B),
// the furthest a (F) and the remembered cell are uniform scalars, the drop rule stops the pass beside the end rule, and the traceback starts
// at the remembered cell.  The non-EXT instantiations hold none of it.
//
// Per-pair allowances and a per-pair diagonal band (mwf_band_t, same header) are run-time properties of the same four kernels: ends_pair reads the pair's
// allowances and band (EndsArgs::pp_ends / pp_band; null: the kernarg scalars, no band) into uniform values, applies the feasibility rule — a pair whose band
// admits no alignment gets the stopped record without a pass — and hands the pass the band as a column range [blo, bhi]; the pass intersects the origin
// window with it and grows a slice no further than it.  Without a band blo = 1 and bhi = tl + ql + 1, the limits the growth has always had.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mwf_ends.h"

#include "mwf_device.h"

namespace mwf {

using namespace dev;

namespace {

// the kernel's argument block read from the kernarg segment where it is needed (as dev::kernel_args does for a plain BatchArgs)
typedef const EndsArgs __attribute__((address_space(4))) KEnds;
__device__ __forceinline__ KEnds &ends_args()
{
	KEnds *p = (KEnds*)__builtin_amdgcn_kernarg_segment_ptr(); // EndsArgs is the kernel's only parameter
	asm volatile("" : "+s"(p));
	return *p;
}

constexpr int32_t kNoEnd = 0x7fffffff; // "no end cell yet" in the column minimum (flags[.][2])

// EXT: the penalty's best cell, one slot per penalty (mod 3) beside dev::Shared's flag sets (cleared two penalties ahead, as they are).  A key is
// (a + 1) << 33 | inverted column << 3 | start state: the largest is the largest a, then the lowest column, and the whole record rides on one
// atomic (a + 1 and the column are below 2^30: the host refuses tl + ql + 2 >= 2^30); 0 is "no in-matrix cell at this penalty".
struct ExtShared {
	unsigned long long key[3];
};
constexpr uint32_t kExtColMask = 0x3fffffffu;
__device__ __forceinline__ unsigned long long ext_key(int32_t a, int32_t c, int32_t pay)
{
	return (unsigned long long)(uint32_t)(a + 1) << 33 | (unsigned long long)(~(uint32_t)c & kExtColMask) << 3 | (uint32_t)pay;
}
// The largest key of the wave (uniform): six DPP steps — within quads, within rows of 16, then lane 15 of a row into the next row and lane 31 into the
// upper half — leave it in lane 63.  Both halves of a key move under the same control; a lane the row mask leaves out sees its own key.  (The same
// reduction by __shfl_xor is twelve ds_bpermute in a chain of six LDS round trips: measured 1.12 ... 1.21 x the ends-free pass where this is
// 1.08 ... 1.12 x)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long ext_dpp_max(unsigned long long key)
{
	const int32_t lo = (int32_t)(uint32_t)key, hi = (int32_t)(uint32_t)(key >> 32);
	const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
	const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
	const unsigned long long other = (unsigned long long)ohi << 32 | olo;
	return other > key ? other : key;
}
__device__ __forceinline__ unsigned long long ext_wave_max(unsigned long long key)
{
	key = ext_dpp_max<0xb1, 0xf>(key);  // quad_perm:[1,0,3,2]
	key = ext_dpp_max<0x4e, 0xf>(key);  // quad_perm:[2,3,0,1]
	key = ext_dpp_max<0x124, 0xf>(key); // row_ror:4
	key = ext_dpp_max<0x128, 0xf>(key); // row_ror:8
	key = ext_dpp_max<0x142, 0xa>(key); // row_bcast:15 into rows 1 and 3
	key = ext_dpp_max<0x143, 0xc>(key); // row_bcast:31 into rows 2 and 3
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)key, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)(uint32_t)(key >> 32), 63);
	return (unsigned long long)hi << 32 | lo;
}

// What a pair's pass and traceback read instead of the kernarg allowances: the pair's own allowances (or the batch's) and its band in columns, all uniform.
struct PairEnds {
	int32_t t_beg, t_end, q_beg, q_end;
	int32_t blo, bhi; // the band, clamped to the matrix: columns blo..bhi (1..cmax when there is none)
};

struct EndsResult {
	int32_t status;
	int32_t s;        // final penalty
	int32_t info;     // start state of the traceback
	int32_t te, qe;   // the end cell: target and query bases consumed
	int64_t cells;    // n_iter
	int32_t ext[4];   // EXT: mwf_ext_t's info = {V, s_stop, why, F}
};

// One forward pass over a pair.  TB: store traceback bytes.  EXT: the extension rule (xs: its slots; otherwise not used).
template <int T, bool TB, bool EXT>
__device__ EndsResult ends_pass(KEnds &E, const PairEnds &pe, const PairMem &M, Shared &sh, ExtShared *xs)
{
	KArgs &A = E.b;
	Penalty P;
	P.x = A.pen.x, P.oe1 = A.pen.oe1, P.e1 = A.pen.e1, P.oe2 = A.pen.oe2, P.e2 = A.pen.e2, P.o1 = A.pen.o1, P.o2 = A.pen.o2;
	P.nH = A.pen.nH, P.n1 = A.pen.n1, P.n2 = A.pen.n2;
	const int32_t tl = M.tl, ql = M.ql, cmax = tl + ql + 1; // columns 1..cmax hold diagonals -tl..ql
	const int32_t tid = threadIdx.x, lane = tid & 63, wave0 = tid & ~63;
	const int64_t W = A.W;
	const int32_t t_end = pe.t_end, q_end = pe.q_end;
	const int32_t blo = pe.blo, bhi = pe.bhi; // 1 <= blo <= bhi <= cmax
	EndsResult R;
	R.status = ST_OK, R.s = 0, R.info = 0, R.te = -1, R.qe = -1, R.cells = 0;

	// the end rule on cell (column c, diagonal d, offset k) of flag set `set`; a lane's columns ascend over its trips, so its first hit is its lowest
	int32_t cand_c = kNoEnd, cand_k = 0, cand_pay = 0;
	auto end_test = [&](int32_t c, int32_t d, int32_t k, int32_t pay, int32_t set) {
		const int32_t i = d + k;
		if ((i == ql - 1 && tl - 1 - k <= t_end) || (k == tl - 1 && ql - 1 - i <= q_end)) {
			if (cand_c == kNoEnd) cand_c = c, cand_k = k, cand_pay = pay;
			atomicMin(&sh.flags[set][2], c);
		}
	};
	// after the penalty's barrier: the lowest end column, if any; its owner hands offset and start state to everybody (uniform result)
	auto pick_end = [&](int32_t endc) {
		if (cand_c == endc) sh.word[0] = cand_k, sh.word[1] = cand_pay;
		__syncthreads();
		const int32_t k = uni(sh.word[0]);
		R.info = uni(sh.word[1]);
		R.te = k + 1, R.qe = endc - 1 - tl + k + 1;
	};
	// EXT.  A lane's best cell of the penalty (its columns ascend over its trips: a strict > keeps its lowest) ...
	int32_t run_a = -1, run_c = 0, run_pay = 0;
	auto ext_cell = [&](int32_t c, int32_t d, int32_t k, int32_t pay) {
		const int32_t a = d + 2 * k + 2; // (i + 1) + (k + 1)
		if (a > run_a) run_a = a, run_c = c, run_pay = pay;
	};
	// ... goes to the penalty's slot, one atomic per wave that has a cell ...
	auto ext_publish = [&](int32_t set) {
		if (__ballot(run_a >= 0) == 0) return;
		const unsigned long long key = ext_wave_max(run_a >= 0 ? ext_key(run_a, run_c, run_pay) : 0ull);
		if (lane == 0) atomicMax(&xs->key[set], key);
		run_a = -1;
	};
	// ... and after the penalty's barrier steps 1-3 of the rule run on uniform scalars: B and its cell, F
	// (B and F fit 32 bits: 0 <= B <= A F <= A (tl + ql), which the host keeps below 2^31; the key of B's cell is decoded once, at the end)
	const int32_t ext_A = EXT ? E.match : 0, ext_Z = EXT ? E.zdrop : -1;
	int32_t ext_B = -1, ext_F = 0, ext_why = 0;
	int32_t best_s = 0;
	uint32_t best_lo = 0, best_hi = 0;
	auto ext_take = [&](int32_t set, int32_t s) {
		const unsigned long long key = xs->key[set];
		const uint32_t lo32 = (uint32_t)uni((int32_t)(key & 0xffffffffu)), hi32 = (uint32_t)uni((int32_t)(key >> 32));
		if ((lo32 | hi32) == 0) return;
		const int32_t a = (int32_t)(hi32 >> 1) - 1;
		const int64_t V = (int64_t)ext_A * a - 2 * (int64_t)s;
		if (V > ext_B) ext_B = (int32_t)V, best_s = s, best_lo = lo32, best_hi = hi32;
		if (a > ext_F) ext_F = a;
	};
	// step 4's drop, at penalty s
	auto ext_drop = [&](int32_t s) { return ext_Z >= 0 && (int64_t)ext_B - (int64_t)ext_A * ext_F + 2 * (int64_t)s > ext_Z; };
	// the pass ended at penalty s: the answer is the remembered cell
	auto ext_finish = [&](int32_t s) {
		const int32_t a = (int32_t)(best_hi >> 1) - 1, c = (int32_t)(~(((best_hi & 1u) << 29) | (best_lo >> 3)) & kExtColMask);
		const int32_t d = c - 1 - tl, k = (a - d - 2) >> 1;
		R.s = best_s, R.info = (int32_t)(best_lo & 7u), R.te = k + 1, R.qe = d + k + 1;
		R.ext[0] = ext_B, R.ext[1] = s, R.ext[2] = ext_why, R.ext[3] = ext_F;
	};

	// ---- penalty 0: the origin window, cut to the band (the feasibility rule of ends_pair left it non-empty), and its extension; E and F are dead
	const int32_t lo0 = max(tl + 1 - min(pe.t_beg, tl), blo), hi0 = min(tl + 1 + min(pe.q_beg, ql), bhi);
	if (tid == 0) {
		for (int32_t j = 0; j < P.nH; ++j) sh.rng_lo[j] = 1, sh.rng_hi[j] = 0;
		for (int32_t j = 0; j < 3; ++j) sh.flags[j][0] = sh.flags[j][1] = sh.flags[j][3] = 0, sh.flags[j][2] = kNoEnd;
		if constexpr (EXT) xs->key[0] = xs->key[1] = xs->key[2] = 0;
		sh.rng_lo[0] = lo0, sh.rng_hi[0] = hi0;
	}
	__syncthreads();
	for (int32_t c0 = (lo0 & ~63) + wave0; c0 <= hi0; c0 += T) {
		const int32_t c = c0 + lane;
		if (c >= lo0 && c <= hi0) {
			const int32_t d = c - 1 - tl;
			const int32_t k = extend_run(M.ts, M.qs, tl, ql, (d < 0 ? -d : 0) - 1, d); // (every origin cell is inside the matrix)
			end_test(c, d, k, 0, 0);
			if constexpr (EXT) ext_cell(c, d, k, 0);
			M.H[c] = k;
			M.E1[c] = M.F1[c] = M.E2[c] = M.F2[c] = kNegInf;
		}
	}
	if constexpr (EXT) ext_publish(0);
	__syncthreads();
	{
		const int32_t endc = uni(sh.flags[0][2]);
		if constexpr (EXT) { // the origin cell is the first candidate, and the only one if it already meets an edge
			ext_take(0, 0);
			if (endc != kNoEnd) {
				ext_finish(0);
				return R;
			}
		} else
		if (endc != kNoEnd) { // an end cell at no cost (identical sequences, an exact substring, an empty alignment the allowances cover)
			pick_end(endc);
			return R;
		}
	}

	int32_t s = 0, wf_lo = lo0, wf_hi = hi0; // live band, in columns
	int32_t curH = 0, cur1 = 0, cur2 = 0, par = 0;
	int64_t cells = 0, tb_used = 0;

	for (;;) {
		// ---- window of the new slice (miniwfa.c:417-418), held inside the band (blo <= wf_lo and wf_hi <= bhi throughout)
		const int32_t lo = wf_lo > blo ? wf_lo - 1 : blo;
		const int32_t hi = wf_hi < bhi ? wf_hi + 1 : bhi;
		const int32_t w = hi - lo + 1;
		const int32_t s_new = s + 1;
		const int32_t newH = curH + 1 == P.nH ? 0 : curH + 1;
		const int32_t new1 = cur1 + 1 == P.n1 ? 0 : cur1 + 1;
		const int32_t new2 = cur2 + 1 == P.n2 ? 0 : cur2 + 1;
		const int32_t npar = par + 1 == 3 ? 0 : par + 1;
		if (TB) {
			if (s_new - 1 >= A.rows_slot) { R.status = ST_ROWS_OVERFLOW; break; }
			if (tb_used + w > A.tb_slot_bytes) { R.status = ST_TB_OVERFLOW; break; }
		}
		// ---- source slices (reference wf_next_prep, miniwfa.c:243-259)
		int32_t jx = newH - P.x;    if (jx < 0) jx += P.nH;
		int32_t j1 = newH - P.oe1;  if (j1 < 0) j1 += P.nH;
		int32_t j2 = newH - P.oe2;  if (j2 < 0) j2 += P.nH;
		int32_t jg1 = newH - P.e1;  if (jg1 < 0) jg1 += P.nH;
		int32_t jg2 = newH - P.e2;  if (jg2 < 0) jg2 += P.nH;
		const int32_t r1 = new1 + 1 == P.n1 ? 0 : new1 + 1; // row of penalty s_new - e1 in the E1/F1 ring
		const int32_t r2 = new2 + 1 == P.n2 ? 0 : new2 + 1;
		Src sx, so1, so2, se1, sf1, se2, sf2;
		sx.p  = M.H + jx * W,   sx.lo  = uni(sh.rng_lo[jx]),  sx.hi  = uni(sh.rng_hi[jx]);
		so1.p = M.H + j1 * W,   so1.lo = uni(sh.rng_lo[j1]),  so1.hi = uni(sh.rng_hi[j1]);
		so2.p = M.H + j2 * W,   so2.lo = uni(sh.rng_lo[j2]),  so2.hi = uni(sh.rng_hi[j2]);
		se1.p = M.E1 + r1 * W,  se1.lo = uni(sh.rng_lo[jg1]), se1.hi = uni(sh.rng_hi[jg1]);
		sf1.p = M.F1 + r1 * W,  sf1.lo = se1.lo,              sf1.hi = se1.hi;
		se2.p = M.E2 + r2 * W,  se2.lo = uni(sh.rng_lo[jg2]), se2.hi = uni(sh.rng_hi[jg2]);
		sf2.p = M.F2 + r2 * W,  sf2.lo = se2.lo,              sf2.hi = se2.hi;
		// columns for which no read can leave a source window
		const int32_t ilo = max(max(lo, sx.lo), max(max(so1.lo, so2.lo), max(se1.lo, se2.lo)) + 1);
		const int32_t ihi = min(min(hi, sx.hi), min(min(so1.hi, so2.hi), min(se1.hi, se2.hi)) - 1);
		int32_t *dH = M.H + newH * W, *dE1 = M.E1 + new1 * W, *dF1 = M.F1 + new1 * W, *dE2 = M.E2 + new2 * W, *dF2 = M.F2 + new2 * W;
		uint8_t *tbrow = TB ? M.tb + tb_used - lo : 0; // tbrow[c] is the byte of column c
		// a shrink at the next multiple of 256 can still see this slice (miniwfa.c:148-154)
		const bool track_good = (((256 - (s_new & 255)) & 255) < P.nH);
		unsigned long long *gword = M.good + (int64_t)newH * A.GW;

		if (tid == 0) {
			sh.rng_lo[newH] = lo, sh.rng_hi[newH] = hi;
			// the flag set of the NEXT penalty: its last readers passed the previous barrier, its next writers start after this penalty's
			const int32_t nn = npar + 1 == 3 ? 0 : npar + 1;
			sh.flags[nn][0] = sh.flags[nn][1] = sh.flags[nn][3] = 0, sh.flags[nn][2] = kNoEnd;
			if constexpr (EXT) xs->key[nn] = 0;
			if (TB) M.row_off[s_new - 1] = tb_used, M.row_lo[s_new - 1] = lo;
		}
		cand_c = kNoEnd;

		// ---- advance + extend over the window, 64 columns per wave per trip
		for (int32_t c0 = (lo & ~63) + wave0; c0 <= hi; c0 += T) {
			const int32_t c = c0 + lane;
			Cell v;
			bool active = true;
			if (c0 >= ilo && c0 + 63 <= ihi) { // interior wave: plain coalesced loads
				v = wf_cell<TB>(sx.at(c), so1.at(c - 1), se1.at(c - 1), so2.at(c - 1), se2.at(c - 1),
				                so1.at(c + 1), sf1.at(c + 1), so2.at(c + 1), sf2.at(c + 1));
			} else {
				active = c >= lo && c <= hi;
				const int32_t cc = active ? c : lo; // keep idle lanes on a valid address
				v = wf_cell<TB>(sx.rd(cc), so1.rd(cc - 1), se1.rd(cc - 1), so2.rd(cc - 1), se2.rd(cc - 1),
				                so1.rd(cc + 1), sf1.rd(cc + 1), so2.rd(cc + 1), sf2.rd(cc + 1));
			}
			const int32_t d = c - 1 - tl;
			if (track_good) {
				const bool g = active && (in_matrix(d, v.h, tl, ql) || in_matrix(d, v.e1, tl, ql) || in_matrix(d, v.f1, tl, ql) ||
				                          in_matrix(d, v.e2, tl, ql) || in_matrix(d, v.f2, tl, ql));
				const unsigned long long m = __ballot(g);
				if (lane == 0) gword[c0 >> 6] = m;
			}
			if (active) {
				// edge rule (miniwfa.c:325-326): H is the max of the five, so "any of them live" == "H live"
				if (c == lo && v.h >= -1) sh.flags[npar][0] = 1;
				if (c == hi && v.h >= -1) sh.flags[npar][1] = 1;
				int32_t k = v.h;
				if (in_matrix(d, k, tl, ql)) {
					k = extend_run(M.ts, M.qs, tl, ql, k, d);
					const int32_t pay = k == v.h ? (int32_t)(v.tb & 7u) : 0; // start state: as at miniwfa.c:405-407
					end_test(c, d, k, pay, npar);
					if constexpr (EXT) ext_cell(c, d, k, pay);
				}
				dH[c] = k, dE1[c] = v.e1, dF1[c] = v.f1, dE2[c] = v.e2, dF2[c] = v.f2;
				if (TB) tbrow[c] = (uint8_t)v.tb;
			}
		}
		if constexpr (EXT) ext_publish(npar);
		__syncthreads();

		// ---- bookkeeping, identical on every thread
		if (uni(sh.flags[npar][0])) wf_lo = lo;
		if (uni(sh.flags[npar][1])) wf_hi = hi;
		const int32_t endc = uni(sh.flags[npar][2]);
		s = s_new, curH = newH, cur1 = new1, cur2 = new2, par = npar;
		if (TB) tb_used += w;
		if ((s & 0xff) == 0) { // shrink (reference wf_stripe_shrink, miniwfa.c:144-171)
			if (tid == 0) sh.red[0] = 0x7fffffff, sh.red[1] = -1;
			__syncthreads();
			const int32_t wfirst = wf_lo >> 6, wlast = wf_hi >> 6;
			for (int32_t wi = wfirst + tid; wi <= wlast; wi += T) {
				unsigned long long m = 0;
				for (int32_t j = 0; j < P.nH; ++j)
					m |= M.good[(int64_t)j * A.GW + wi] & window_mask(wi << 6, sh.rng_lo[j], sh.rng_hi[j]);
				m &= window_mask(wi << 6, wf_lo, wf_hi);
				if (m) {
					atomicMin(&sh.red[0], (wi << 6) + (int32_t)__builtin_ctzll(m));
					atomicMax(&sh.red[1], (wi << 6) + 63 - (int32_t)__builtin_clzll(m));
				}
			}
			__syncthreads();
			const int32_t glo = uni(sh.red[0]), ghi = uni(sh.red[1]);
			if (ghi < 0) { R.status = ST_INTERNAL; break; }
			wf_lo = glo, wf_hi = ghi;
		}
		cells += w;
		if ((A.max_iter > 0 && cells > A.max_iter) || (A.max_s > 0 && s > A.max_s)) { // miniwfa.c:422-425
			R.status = ST_STOPPED;
			break;
		}
		if constexpr (EXT) { // steps 1-3, then the two ends of the pass: an edge of the matrix, or the drop against the furthest anti-diagonal
			ext_take(par, s);
			if (endc != kNoEnd) break;
			if (ext_drop(s)) { ext_why = 1; break; }
		} else
		if (endc != kNoEnd) {
			pick_end(endc);
			break;
		}
	}
	R.s = s, R.cells = cells;
	if constexpr (EXT) {
		if (R.status == ST_OK) ext_finish(s);
	}
	return R;
}

// Traceback on the first wave (dev::traceback_wave with the start cell and the end of the walk of an ends-free alignment): from cell
// (qe - 1, te - 1) back until the walk leaves the matrix with L = i + 1 query or k + 1 target bases in front of it; min(L, begin
// allowance) of them are clipped — that is qb or tb — and the rest is one I or D run, merged with an adjacent run of the same operation.
// Ops are written backwards from the end of the scratch buffer.  Returns n_cigar (>= 0) or -1 when the buffer is too small or the walk
// ran out of rows.
__device__ int32_t ends_traceback(KEnds &E, const PairEnds &pe, const PairMem &M, uint32_t *scratch, int64_t cap, const EndsResult &R, int32_t *tb_out, int32_t *qb_out)
{
	KArgs &A = E.b;
	const auto &P = A.pen;
	const int32_t lane = threadIdx.x & 63;
	int32_t i = R.qe - 1, k = R.te - 1, row = R.s - 1, last = R.info;
	int64_t pos = cap;
	int32_t run_op = -1, run_len = 0;
	bool overflow = false;
	auto push = [&](int32_t op, int32_t len) { // reference wf_cigar_push1, miniwfa.c:51-62
		if (op == run_op) { run_len += len; return; }
		if (run_op >= 0) {
			if (pos == 0) { overflow = true; return; }
			--pos;
			if (lane == 0) scratch[pos] = (uint32_t)run_len << 4 | (uint32_t)run_op;
		}
		run_op = op, run_len = len;
	};
	// the byte of the cell the walk stands on is requested as soon as the cell is known, before the back-match along its diagonal
	uint32_t x_next = 0;
	if (row >= 0 && i >= 0 && k >= 0) x_next = tb_byte(M, row, i - k + M.tl + 1);
	// every 40 rows the 64 lanes fetch the byte in the walk's current column of the next 64 rows: the steps through those rows find their lines in L2
	int32_t pf_at = row;
	while (i >= 0 && k >= 0 && !overflow) {
		uint32_t pf = 0;
		const bool pf_now = row <= pf_at && row > 0;
		if (pf_now) {
			const int32_t r = row - 1 - lane, col = i - k + M.tl + 1;
			if (r >= 0) {
				int64_t at = M.row_off[r] + (col - M.row_lo[r]);
				at = min(max(at, (int64_t)0), (int64_t)A.tb_slot_bytes - 1); // (an older row may not reach this column: any byte of the arena will do)
				pf = M.tb[at];
			}
			pf_at = row - 40;
		}
		if (last == 0) { // greedy back-match (miniwfa.c:335-341)
			int32_t run = 0;
			bool open = true;
			// far from the start of both sequences: eight bases per lane, 512 per trip
			while (i - run >= 511 && k - run >= 511) {
				const int32_t ii = i - run - 8 * lane, kk = k - run - 8 * lane;
				const uint64_t x = ld8(M.qs + ii - 7) ^ ld8(M.ts + kk - 7);
				const int32_t m8 = x ? (int32_t)(__builtin_clzll(x) >> 3) : 8; // equal bases from the top byte down
				const unsigned long long stop = __ballot(m8 < 8);
				if (stop == 0) { run += 512; continue; }
				const int32_t first = (int32_t)__builtin_ctzll(stop);
				run += 8 * first + __builtin_amdgcn_readlane(m8, first);
				open = false;
				break;
			}
			while (open) { // 64 bases per trip
				const int32_t ii = i - run - lane, kk = k - run - lane;
				const bool eq = ii >= 0 && kk >= 0 && M.qs[ii] == M.ts[kk];
				const unsigned long long m = __ballot(eq);
				const int32_t n = m == ~0ull ? 64 : (int32_t)__builtin_ctzll(~m);
				run += n;
				open = n == 64;
			}
			if (run > 0) push(7, run);
			i -= run, k -= run;
			if (i < 0 || k < 0) break;
		}
		if (row < 0) { overflow = true; break; } // (penalty 0 is all matches: the walk must have left the matrix by now)
		if (pf_now) asm volatile("" :: "v"(pf)); // (the prefetched bytes have arrived — and stay in L2)
		const uint32_t x = x_next;
		const int32_t state = last == 0 ? (int32_t)(x & 7u) : last;           // :346
		const int32_t ext = state > 0 ? (int32_t)(x >> (state + 2)) & 1 : 0;  // :347
		if (state == 0) { push(8, 1); --i, --k; row -= P.x; }
		else if (state == 1) { push(1, 1); --i; row -= ext ? P.e1 : P.oe1; }
		else if (state == 3) { push(1, 1); --i; row -= ext ? P.e2 : P.oe2; }
		else if (state == 2) { push(2, 1); --k; row -= ext ? P.e1 : P.oe1; }
		else { push(2, 1); --k; row -= ext ? P.e2 : P.oe2; }
		last = (state > 0 && ext) ? state : 0;                                // :365
		if (row >= 0 && i >= 0 && k >= 0) x_next = tb_byte(M, row, i - k + M.tl + 1);
	}
	int32_t tb = 0, qb = 0;
	if (i >= 0) { // query bases in front of the walk: clip what q_beg covers, insert the rest
		const int32_t L = i + 1;
		qb = min(L, pe.q_beg);
		if (L > qb) push(1, L - qb);
	} else if (k >= 0) {
		const int32_t L = k + 1;
		tb = min(L, pe.t_beg);
		if (L > tb) push(2, L - tb);
	}
	push(-2, 0); // flush the pending run
	*tb_out = tb, *qb_out = qb;
	if (overflow) return -1;
	return (int32_t)(cap - pos);
}

// One pair: the pass, the traceback on the first wave, the CIGAR into the pool, the per-pair outputs (dev::finish_pair plus the ranges).
template <int T, bool EXT>
__device__ void ends_pair(KEnds &E, Shared &sh, ExtShared *xs, int32_t slot, int32_t pair)
{
	KArgs &A = E.b;
	PairMem M;
	pair_mem(A, slot, pair, M);
	// the pair's allowances and band: one scalar load each where the launch has per-pair arrays
	PairEnds pe;
	pe.t_beg = E.t_beg, pe.t_end = E.t_end, pe.q_beg = E.q_beg, pe.q_end = E.q_end;
	if (E.pp_ends) {
		const int32_t *p = E.pp_ends + 4 * (int64_t)pair;
		pe.t_beg = uni(p[0]), pe.t_end = uni(p[1]), pe.q_beg = uni(p[2]), pe.q_end = uni(p[3]);
	}
	const int32_t tl = M.tl, ql = M.ql;
	pe.blo = 1, pe.bhi = tl + ql + 1;
	bool feasible = true;
	if (E.pp_band) {
		const int32_t *p = E.pp_band + 2 * (int64_t)pair;
		const int32_t d_lo = uni(p[0]), d_hi = uni(p[1]);
		// the feasibility rule (mwf_ends_band.h ends_band_feasible, restated): the band clamped to [-tl, ql] is non-empty and meets the origin diagonals
		// [-min(t_beg, tl), min(q_beg, ql)] and the end diagonals [ql - tl - min(q_end, ql), ql - tl + min(t_end, tl)].  Every term lies in [-tl, ql].
		feasible = d_lo <= d_hi && d_lo <= ql && d_hi >= -tl;
		if (feasible) {
			const int32_t dl = max(d_lo, -tl), dh = min(d_hi, ql);
			feasible = dl <= min(pe.q_beg, ql) && dh >= -min(pe.t_beg, tl) && dl <= ql - tl + min(pe.t_end, tl) && dh >= ql - tl - min(pe.q_end, ql);
			pe.blo = dl + tl + 1, pe.bhi = dh + tl + 1;
		}
	}
	EndsResult R;
	if (feasible) R = A.want_cigar ? ends_pass<T, true, EXT>(E, pe, M, sh, xs) : ends_pass<T, false, EXT>(E, pe, M, sh, xs);
	else R.status = ST_STOPPED, R.s = 0, R.info = 0, R.te = R.qe = -1, R.cells = 0; // nothing inside the band: the stopped record with n_iter == 0
	int32_t status = R.status, n_cigar = 0, tb = -1, qb = -1;
	int64_t cig_off = 0;
	if (A.want_cigar && status == ST_OK) {
		__syncthreads();
		if (threadIdx.x < 64) {
			uint32_t *scratch = A.cig_scratch + (int64_t)slot * A.cig_scratch_slot;
			n_cigar = ends_traceback(E, pe, M, scratch, A.cig_scratch_slot, R, &tb, &qb);
			if (n_cigar < 0) status = ST_INTERNAL, n_cigar = 0;
			else {
				unsigned long long off = 0;
				if (threadIdx.x == 0) off = atomicAdd(A.cig_head, (unsigned long long)n_cigar);
				off = ((unsigned long long)(uint32_t)uni((int32_t)(off >> 32)) << 32) | (uint32_t)uni((int32_t)(off & 0xffffffffu));
				if ((int64_t)off + n_cigar > A.cig_pool_words) status = ST_CIGAR_OVERFLOW, n_cigar = 0;
				else {
					cig_off = (int64_t)off;
					const uint32_t *src = scratch + (A.cig_scratch_slot - n_cigar);
					for (int32_t j = threadIdx.x; j < n_cigar; j += 64) A.cig_pool[off + j] = src[j];
				}
			}
		}
	}
	if (threadIdx.x == 0) {
		// -1 is the reference's "stopped" answer (miniwfa.c:427); a pair the host still has to re-run holds -2
		A.out_s[pair] = status == ST_OK ? R.s : status == ST_STOPPED ? -1 : -2;
		A.out_iter[pair] = R.cells;
		A.out_ncig[pair] = n_cigar;
		A.out_cigoff[pair] = cig_off;
		A.out_cells1[pair] = 0;
		A.out_status[pair] = status;
		const bool ok = status == ST_OK, walked = ok && A.want_cigar;
		int32_t *rng = E.out_range + 4 * (int64_t)pair;
		rng[0] = ok ? tb : -1, rng[1] = ok ? R.te : -1, rng[2] = ok ? qb : -1, rng[3] = ok ? R.qe : -1;
		if constexpr (EXT) {
			if (!A.want_cigar && ok) rng[0] = rng[2] = 0; // (an extension begins at the origin: known without the walk)
			int32_t *info = E.out_info + 4 * (int64_t)pair;
			for (int32_t j = 0; j < 4; ++j) info[j] = ok ? R.ext[j] : -1;
		}
		E.sub_t_off[pair] = A.t_off[pair] + (walked ? tb : 0), E.sub_tl[pair] = walked ? R.te - tb : 0;
		E.sub_q_off[pair] = A.q_off[pair] + (walked ? qb : 0), E.sub_ql[pair] = walked ? R.qe - qb : 0;
	}
	__syncthreads();
}

// Persistent workgroups: each pulls pairs from a shared counter until the batch is drained.
template <int T, bool EXT>
__global__ __launch_bounds__(T, 1) void wfa_ends_kernel(const EndsArgs)
{
	__shared__ Shared sh;
	ExtShared *xs = nullptr;
	if constexpr (EXT) {
		__shared__ ExtShared ext_slots; // (the kernel's own: dev::Shared is the generic kernel's too)
		xs = &ext_slots;
	}
	KEnds &E0 = ends_args();
	for (;;) {
		KEnds &E = fresh(E0);
		if (threadIdx.x == 0) sh.item = (int32_t)atomicAdd(E.b.queue, 1);
		__syncthreads();
		const int32_t item = uni(sh.item);
		__syncthreads();
		if (item >= E.b.n_pairs) break;
		const int32_t pair = E.b.order ? E.b.order[item] : item;
		ends_pair<T, EXT>(E, sh, xs, (int32_t)blockIdx.x, pair);
	}
}

typedef void (*EndsKernel)(const EndsArgs);
EndsKernel ends_form(int block, bool ext)
{
	if (ext) return block == 256 ? &wfa_ends_kernel<256, true> : block == 512 ? &wfa_ends_kernel<512, true> : nullptr;
	return block == 256 ? &wfa_ends_kernel<256, false> : block == 512 ? &wfa_ends_kernel<512, false> : nullptr;
}

} // namespace

int launch_ends(const EndsArgs &a, int grid, int block, void *stream)
{
	if (a.b.pen.nH > kMaxRing) return -1; // (the window table of dev::Shared; the host refuses such penalty sets)
	const EndsKernel kernel = ends_form(block, a.ext != 0);
	if (!kernel) return -1;
	if (getenv("MWF_DEBUG")) fprintf(stderr, "[libmwf_hip] %s launch: T %d, %d pairs, grid %d, allowances %d %d %d %d, match %d, zdrop %d, per-pair allowances %d, band %d\n", a.ext ? "extension" : "ends-free", block, (int)a.b.n_pairs, grid, a.t_beg, a.t_end, a.q_beg, a.q_end, a.match, a.zdrop, a.pp_ends ? 1 : 0, a.pp_band ? 1 : 0);
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

int ends_kernel_occupancy(int block, bool ext)
{
	const EndsKernel kernel = ends_form(block, ext);
	int n = 0;
	if (!kernel || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, 0) != hipSuccess) return 0;
	return n;
}

} // namespace mwf
