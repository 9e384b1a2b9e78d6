// mwf_plan_classes.h — the size classes of a batch, stated once: their names, what a launch of each asks for (geometry, sequence-copy form, kernel),
// where its pairs go when they do not fit, the order the classes run in, the bits of a pair's flag byte, and the rule that gives a pair its class.
// Host only, no HIP header: tests/host/plan_classes.cpp builds the rule stand-alone.  mwf_plan.cpp is the one user of everything but the names.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include "mwf_internal.h"

namespace mwf {
namespace host {

// Size classes.  One long pair must not push a thousand short ones onto the slow kernel (mwf_wfa_chain's gap fills are exactly such a mix): pairs are
// grouped by what their window can grow to, and every group runs on the kernel that suits it.  (The numbers are those of PlanCache::cls0 since round 3.)
enum PairClass : int8_t {
	CLS_GENERIC = 0,      // the generic kernel: whatever no other class takes
	CLS_WIDE = 1,         // packed band kernel, 512 threads x 3 or 4 chunk slots
	CLS_SMALL = 2,        // ... 256 threads
	CLS_TINY = 3,         // ... 128 threads
	CLS_MICRO = 4,        // ... 64 threads
	CLS_LOWMEM = 5,       // two-pass low-memory pairs (opt.step > 0 and a penalty bound that can reach it): the generic kernel
	CLS_WIDE_BYTES = 6,   // the four band classes again for the pairs the host knows not to be plain A/C/G/T (byte-wise sequence copy from the start)
	CLS_SMALL_BYTES = 7,
	CLS_TINY_BYTES = 8,
	CLS_MICRO_BYTES = 9,
	CLS_LANE = 10,        // short pairs on the one-diagonal-per-lane kernel (mwf_lane.hip); what outgrows its 64 columns moves to the band classes
	CLS_MID = 11,         // mid-size pairs of a small batch on the one-workgroup-per-pair, rings-in-LDS kernel (mwf_mid.hip); what outgrows its span moves to the band classes
	CLS_LANE_BYTES = 12,  // the pairs of CLS_LANE the host knows not to be plain A/C/G/T — reads with an N —: the lane kernel on byte-wise copies
	// pairs too long (or with windows too wide) for the 512-thread packed geometry on its 1024-thread span geometry: targets of up to ~60 kb on biased
	// 16-bit offsets, windows of up to ~16 000 columns; what outgrows it moves to the generic kernel
	CLS_SPAN = 13,
	// pairs of up to ~21 kb per sequence whose worst-case penalty rules out plain 16-bit offsets: the 512-thread geometry with five or six chunk slots, which computes on
	// biased offsets with range checks like the span geometry but keeps two pairs per CU (windows of up to 9920 / 11 968 columns; what outgrows them moves to the span geometry).
	// Built for every set the band kernel takes (band2_biased512_supported): where e2 == 2 — main.c's -a preset — the class starts at ~6.6 kb, 1024 x 10 kb batches are its.
	CLS_BIASED = 14,
	// ("alpha16", gap extensions (2,1)) the class-3 pairs of the four band classes on the 4-bit 512-thread geometry, and those of CLS_SPAN and CLS_BIASED on the 4-bit span
	// geometry (mwf_band2_nib.hip); hand-backs as for the plain pairs of their fallback class — window overflow to the next 4-bit geometry, then the generic kernel
	CLS_WIDE_NIB = 15,
	CLS_SPAN_NIB = 16,
	kNumClasses = 17
};

// the geometry a launch asks choose_kernel for
enum Geom : int8_t {
	GEOM_CHOOSE = 0, // by the window of the launch's pairs (and its window hint)
	GEOM_MICRO,      // packed band kernel, 64 threads
	GEOM_TINY,       // 128
	GEOM_SMALL,      // 256
	GEOM_LANE,       // mwf_lane.hip
	GEOM_MID,        // mwf_mid.hip
	GEOM_BIASED,     // 512 threads, five / six chunk slots on biased offsets
	GEOM_SPAN        // 1024 threads
};
constexpr int geom_small_block(Geom g) { return g == GEOM_MICRO ? 64 : g == GEOM_TINY ? 128 : g == GEOM_SMALL ? 256 : 0; } // threads of the three small geometries (0: not one of them)

// the sequence copy of a launch's pairs
enum CopyForm : int8_t {
	COPY_2BIT = 0, // 2 bits per base where the kernel and "seq2bit" have that form (a pair outside plain A/C/G/T comes back as ST_ALPHABET)
	COPY_BYTES,    // pairs known not to be plain A/C/G/T
	COPY_NIB       // "alpha16": 4 bits per base, class-3 pairs
};

// mwf_gpu_batch_t::h_flags
enum : int8_t {
	FLAG_STEP0 = 1,        // runs as high-memory although opt.step > 0 (its penalty bound is below step)
	FLAG_COOP_SHARED = 2,  // shared the whole-device kernel with other pairs
	FLAG_COOP_GAVE_UP = 8, // a wait of the whole-device kernel ran into its spin limit: the pair was given to one workgroup (once)
	FLAG_COOP_WIDE = 16,   // its window outgrew the whole-device kernel's 64-column slots: 256-column ones from now on
	FLAG_COOP_NARROW = 32, // a pass of the whole-device kernel ran it on 64-column slots
	FLAG_THREE_SLOTS = 64  // ran on the plain three-slot 512-thread geometry — the only one whose LATE overflow says "this batch's wide class needs four slots"
};

struct ClassRow {
	const char *name;
	Geom geom;
	CopyForm copy;
	int8_t want_kind;   // what its launch asks choose_kernel for when classes are on: 0 generic, 2 band
	PairClass fallback; // h_class of its pairs: the band class (or generic) the re-run of a pair it hands back starts from; the rule narrows it where the lengths say more
	bool by_work;       // on the shared work counter of a 512- or 1024-thread geometry: dealt by predicted work, largest first
	bool wide;          // on the 512-thread geometry of three or four slots
	int8_t retry_slot;  // the batch's device-side list its lane launch hands pairs back through (-1: none)
};
constexpr ClassRow kClassTable[kNumClasses] = {
	{"generic", GEOM_CHOOSE, COPY_2BIT, 0, CLS_GENERIC, false, false, -1},
	{"wide", GEOM_CHOOSE, COPY_2BIT, 2, CLS_WIDE, true, true, -1},
	{"small", GEOM_SMALL, COPY_2BIT, 2, CLS_SMALL, false, false, -1},
	{"tiny", GEOM_TINY, COPY_2BIT, 2, CLS_TINY, false, false, -1},
	{"micro", GEOM_MICRO, COPY_2BIT, 2, CLS_MICRO, false, false, -1},
	{"low-mem", GEOM_CHOOSE, COPY_2BIT, 0, CLS_GENERIC, false, false, -1},
	{"wide-bytes", GEOM_CHOOSE, COPY_BYTES, 2, CLS_WIDE, true, false, -1},
	{"small-bytes", GEOM_SMALL, COPY_BYTES, 2, CLS_SMALL, false, false, -1},
	{"tiny-bytes", GEOM_TINY, COPY_BYTES, 2, CLS_TINY, false, false, -1},
	{"micro-bytes", GEOM_MICRO, COPY_BYTES, 2, CLS_MICRO, false, false, -1},
	{"lane", GEOM_LANE, COPY_2BIT, 2, CLS_MICRO, false, false, 0},
	{"mid", GEOM_MID, COPY_2BIT, 2, CLS_SMALL, false, false, -1},
	{"lane-bytes", GEOM_LANE, COPY_BYTES, 2, CLS_MICRO, false, false, 1},
	{"span", GEOM_SPAN, COPY_2BIT, 2, CLS_SPAN, true, false, -1},
	{"biased", GEOM_BIASED, COPY_2BIT, 2, CLS_WIDE, true, false, -1},
	{"wide-nib", GEOM_CHOOSE, COPY_NIB, 2, CLS_WIDE, true, true, -1},
	{"span-nib", GEOM_SPAN, COPY_NIB, 2, CLS_SPAN, true, false, -1},
};
constexpr const ClassRow &row(int c) { return kClassTable[c]; }
constexpr bool is_band_size_class(int c) { return c == CLS_WIDE || c == CLS_SMALL || c == CLS_TINY || c == CLS_MICRO; }
constexpr PairClass bytes_twin(PairClass c) { return c == CLS_WIDE ? CLS_WIDE_BYTES : c == CLS_SMALL ? CLS_SMALL_BYTES : c == CLS_TINY ? CLS_TINY_BYTES : c == CLS_MICRO ? CLS_MICRO_BYTES : c; }

// The order the classes run in: largest workspace first, so that later groups never have to grow a buffer.
constexpr PairClass kRunOrder[kNumClasses] = {CLS_LOWMEM, CLS_GENERIC, CLS_SPAN, CLS_BIASED, CLS_SPAN_NIB, CLS_WIDE, CLS_WIDE_NIB, CLS_WIDE_BYTES, CLS_SMALL, CLS_SMALL_BYTES,
                                              CLS_TINY, CLS_TINY_BYTES, CLS_MICRO, CLS_MICRO_BYTES, CLS_MID, CLS_LANE, CLS_LANE_BYTES};
constexpr bool run_order_is_permutation()
{
	for (int c = 0; c < kNumClasses; ++c) {
		int seen = 0;
		for (int k = 0; k < kNumClasses; ++k) seen += kRunOrder[k] == c;
		if (seen != 1) return false;
	}
	return true;
}
// the classes dealt by work lie side by side in the run order: one stretch of the processing order holds all their pairs
constexpr int by_work_first()
{
	for (int k = 0; k < kNumClasses; ++k)
		if (row(kRunOrder[k]).by_work) return k;
	return kNumClasses;
}
constexpr int by_work_end() // one past the last
{
	int e = 0;
	for (int k = 0; k < kNumClasses; ++k)
		if (row(kRunOrder[k]).by_work) e = k + 1;
	return e;
}
constexpr bool by_work_is_contiguous()
{
	for (int k = by_work_first(); k < by_work_end(); ++k)
		if (!row(kRunOrder[k]).by_work) return false;
	return true;
}
static_assert(run_order_is_permutation(), "kRunOrder must name every class once");
static_assert(by_work_first() < by_work_end() && by_work_is_contiguous(), "the classes dealt by predicted work must be contiguous in kRunOrder");

// widest window the 64-, 128- and 256-thread packed band variants are chosen for: (waves x 3 chunks - 1) x 256 - 64 columns
constexpr int64_t kBandMicroWindow = (1 * 3 - 1) * 256 - 64, kBandTinyWindow = (2 * 3 - 1) * 256 - 64, kBandSmallWindow = (4 * 3 - 1) * 256 - 64;
constexpr int64_t kBandWideWindow = (8 * 3 - 1) * 256 - 64;
// The 512-thread geometry with FOUR chunk slots per wave (32 chunks, 119 VGPRs, still two workgroups per CU; 2-bit sequence copies only): 2 % slower than
// three slots on windows those hold (1024 x 10 kb @ 5 %: 17.7 against 17.4 ms) — and 17.7 against 24.8 ms on a batch in which ONE pair outgrows them
// late and is re-run alone (three of four seeds of that batch shape, profiles/r04/wide4.txt).  Taken when a forecast or the batch's last align says so.
constexpr int64_t kBandWide4Window = (8 * 4 - 1) * 256 - 64;
// ... and the 1024-thread span geometry (16 waves x kBand2SpanK chunks, offsets biased by the target length: mwf_band2_kernel.h wide_bias)
constexpr int64_t kBandSpanMaxSeq = 62000;
constexpr int64_t band_window(int64_t chunks) { return (chunks - 1) * 256 - 64; } // ... of a geometry that holds `chunks` 256-column chunks

// Upper bound on the optimal penalty: delete the whole target, insert the whole query.
inline int64_t penalty_bound(const Penalty &p, int32_t max_s, int64_t tl, int64_t ql, bool honour_max_s)
{
	auto gap = [&](int64_t L) -> int64_t { return L == 0 ? 0 : std::min<int64_t>(p.o1 + L * p.e1, p.o2 + L * p.e2); };
	int64_t b = gap(tl) + gap(ql);
	// the core pass stops one penalty after max_s (miniwfa.c:422); the low-memory first pass never stops (:569-589)
	if (honour_max_s && max_s > 0) b = std::min<int64_t>(b, (int64_t)max_s + 1);
	return b;
}

// What the per-pair rule depends on besides the pair: fixed for one align.
struct ClassRule {
	Penalty pen;
	int32_t max_s = 0, step = 0; // opt.max_s, opt.step
	bool low_mem = false;        // a CIGAR-mode call with opt.step > 0
	// what the kernels answer for these penalties
	bool band2_ok = false, lane_ok = false, mid_ok_pen = false, biased512_ok = false, nib_ok = false; // band2_supported, lane_supported, mid_supported, band2_biased512_supported, band2_nib_supported
	int biased512_chunks = 0, span_chunks = 0;                                                        // band2_biased512_chunks, band2_span_chunks
	int (*mid_lds_bytes)(const Penalty &p, int groups, int64_t seq_bytes) = nullptr;                   // (mwf_mid.hip; never called while mid_batch is false)
	// tunables (mwf_gpu_s) and what the batch says
	int force_kind = -1, block = 0, band_pack = -1, band_span = 1, seq2bit = 1, wide_slots = 0, alpha16 = 0, lane_max_len = 0;
	int mid_cap = 0;           // "mid_max_pairs" with its default (one per CU) filled in
	bool div_aware = true;
	float div_est = 0;         // mwf_gpu_batch_t::div_est
	bool know_acgt = false;    // the host looked at the batch's bytes (and 2-bit copies are on): a pair's `acgt` means something
	bool alpha_active = false; // "alpha_remap": the align reads the copies
	// derived by finish()
	bool classes = false, small_only = false, pack_pen = false, span_pen = false, lane_on = false, nib_set = false;
	bool mid_batch = false;    // the mid kernel may take pairs of this batch at all
	double div_r = 1.0, div_lane = 1.0;
	int64_t lane_limit = 0;    // longest sequence of a pair the lane kernel is tried for, weighed by div_lane (finish(): lane_max_len; the plan lowers or stretches it by the batch)

	void finish()
	{
		// Kernel and block size forced by the caller (tests, tuning) keep the whole batch in one group.
		classes = force_kind < 0 && block == 0 && band2_ok && band_pack != 0;
		lane_on = lane_max_len > 0 && lane_ok;
		lane_limit = lane_max_len;
		// the mid kernel (a workgroup per pair, one per CU) serves a FEW pairs: a batch of at most mid_cap pairs, or the at most mid_cap pairs of a
		// larger batch that are neither short reads (lane kernel) nor long — mwf_wfa_chain's gap fills are hundreds of
		// tiny pairs and a handful of longer ones, and the handful sets the call's time
		mid_batch = force_kind < 0 && block == 0 && mid_cap > 0 && mid_ok_pen;
		// Penalties the packed band kernel is not instantiated for (gap extensions other than (2,1), (2,2), (1,1): minimap2's asm5 has 3 and 1) leave the generic kernel for
		// everything above — but the lane and mid kernels read their penalties at run time: read batches and a few mid-size pairs still get them (20 000 x 150 bp with
		// e1 = 3: 4.8 ms on the generic kernel, a thirteenth of that on the lane kernel).  What outgrows them goes to the generic kernel.
		small_only = force_kind < 0 && block == 0 && !band2_ok && band_pack != 0;
		pack_pen = band_pack != 0 && band2_ok;
		span_pen = pack_pen && band_span != 0 && seq2bit != 0;
		nib_set = alpha16 != 0 && alpha_active && seq2bit != 0 && band_pack != 0 && band_span != 0 && nib_ok && !low_mem;
		// The classes' length limits stand for "the window stays inside the span at ~5 % divergence".  Where the batch's own divergence is known
		// (estimate_divergence: batches built from host memory) the lengths are weighed by it: three times as diverged = as if three times as long.
		// Only upwards of the prior, and a little downwards: a class too narrow costs a second run, one too wide a few per cent.
		div_r = div_est > 0 && div_aware ? std::min(8.0, std::max(0.7, (double)div_est / 0.05)) : 1.0;
		div_lane = div_est > 0 && div_aware ? std::min(8.0, std::max(0.45, (double)div_est / 0.05)) : 1.0;
	}
	// a pair of alphabet class `alpha` (mwf_alphabet_class16) takes the 4-bit route
	bool nib_pair(int alpha) const { return nib_set && alpha == 3; }
};

struct PairPlan {
	PairClass cls = CLS_GENERIC, fallback = CLS_GENERIC;
	int8_t flags = 0;
	int64_t bound = 0, bound1 = 0, exp_win = 0; // penalty bound with and without max_s; the window the pair is expected to reach (0: divergence unknown)
	bool mid_candidate = false;                 // allow_mid was false and the mid kernel would take the pair: it moves there if such pairs are few
	bool mid_bytes = false;                     // a mid pair the host knows not to be plain A/C/G/T: the (few) pairs of its class all take the byte-wise copy
};

// the two narrowest band classes' admission by window and weighed length (CLS_GENERIC: neither)
inline PairClass micro_or_tiny(const ClassRule &R, int64_t window, int64_t lenw)
{
	// (round 5: the limits leave the mean window at 5 % — 0.27 (tl+ql) — a quarter of margin below each class's widest window; round 4's left 4-18 %,
	// and 2 kb pairs, just inside the 128-thread class, were re-run at 7.8 %: profiles/r04/chooser_regression.txt)
	// (... at 5 %.  A batch the sketch puts at 8 % and more outgrows the 64-thread class earlier than its weight says — the sketch reads low up there, and a pair
	// whose penalty stays below 256 is never shrunk, its window is 2 s + 1: 2000 x 350 bp @ 10 % lost 876 pairs, 20 000 x 380 bp 18 473, to a second run)
	if (window <= kBandMicroWindow || lenw + 1 <= (R.div_est >= 0.06f && R.div_aware ? 1000 : 1400)) return CLS_MICRO;
	if (window <= kBandTinyWindow || lenw + 1 <= 3600) return CLS_TINY;
	return CLS_GENERIC;
}

// Class of one pair.  acgt: the host's look at its bytes (read only where R.know_acgt); alpha: its alphabet class (-1: none); allow_mid: the mid kernel may take it.
// Low-memory mode (opt.step > 0): a pair whose penalty cannot reach `step` never takes a snapshot (the first one is due at
// penalty step-1, miniwfa.c:585), so its low-memory result IS its high-memory result, n_iter included — such pairs (the
// gap fills of mwf_wfa_auto's chain fallback, which inherit step = 5000) run in the classes as high-memory pairs; only
// genuinely long pairs go through the two-pass kernel (CLS_LOWMEM).
// (inlined into the plan's per-pair loop: as a call it costs the first align of a 40 000 x 150 bp batch a tenth of its time, profiles/plan_refactor/plan_timing.txt)
#if defined(__GNUC__)
__attribute__((always_inline))
#endif
inline PairPlan classify_pair(const ClassRule &R, int64_t tl, int64_t ql, bool acgt, int alpha, bool allow_mid)
{
	PairPlan r;
	const Penalty &P0 = R.pen;
	const int64_t len = tl + ql;
	const bool not_acgt = R.know_acgt && !acgt;
	// A pair of very different lengths must open a gap of |tl - ql|: its window reaches that diagonal whatever its divergence (two columns per
	// penalty of the gap, until the matrix ends), so the length limits see it as if it were longer — beyond what indels of a related pair add up
	// to.  (Found on mwf_wfa_chain's gap fills: a 54 x 740 fill sat in the 64-thread class and was run twice, every call.)
	const int64_t skew = std::abs(tl - ql), skew_len = 6 * std::max<int64_t>(0, skew - len / 16);
	const int64_t lenw = (int64_t)((double)len * R.div_r) + skew_len; // the pair's length as the classes' limits should see it
	// the window the pair is expected to reach (0.27 (tl+ql) at 5 %), plus 15 %, where the divergence is known: the long classes' length limits
	// were drawn for ~3 % (configs[4]) and sent 20 kb pairs at 15 % and 50 kb pairs at 5 % through the span geometry for nothing
	const int64_t exp_win = R.div_est > 0 && R.div_aware ? std::min<int64_t>(len + 1, (int64_t)(6.2 * R.div_est * (double)len) + 64) : 0;
	const int64_t bound1 = penalty_bound(P0, R.max_s, tl, ql, false);
	const int64_t bound = R.max_s > 0 ? std::min<int64_t>(bound1, (int64_t)R.max_s + 1) : bound1; // (= penalty_bound(..., true))
	r.bound = bound, r.bound1 = bound1, r.exp_win = exp_win;
	const bool step0 = R.low_mem && bound1 < R.step;
	PairClass c = R.low_mem && !step0 ? CLS_LOWMEM : CLS_GENERIC;
	const bool packable = tl + bound < 32767 && R.pack_pen;
	if (R.classes && c == CLS_GENERIC) {
		const int64_t window = std::min<int64_t>(len + 1, 2 * bound + 3);
		// A window cannot outgrow min(tl+ql+1, 2 x penalty bound + 3); in practice it stays far below tl+ql (a quarter of
		// it at 5 % divergence), so a pair is also given to a small kernel when it is merely short — if its window does
		// outgrow that span, finalize() moves it to the wide band kernel, and from there to the generic one.
		// (a pair too long for the packed band kernel goes to the generic kernel with 16-bit ring rows where those apply: faster than
		// the unpacked band kernel and no window overflows to re-run, see choose_kernel)
		// (... unless the span geometry of the packed kernel takes it: windows of up to ~16 000 columns — a 50 kb pair at 3 % —, which is
		// where the pairs whose windows will mostly fit are drawn: tl + ql below seven spans; bench.py long_batches)
		const bool nib_i = R.nib_pair(alpha); // (its 4-bit copy stands where a plain pair's 2-bit copy does: the long classes admit it)
		const bool span_ok = R.span_pen && tl <= kBandSpanMaxSeq && ql <= kBandSpanMaxSeq && (!not_acgt || nib_i);
		const PairClass narrow = packable ? micro_or_tiny(R, window, lenw) : CLS_GENERIC;
		if (span_ok && R.band_span == 2) c = CLS_SPAN;
		else if (narrow != CLS_GENERIC) c = narrow;
		else if (packable && (window <= kBandSmallWindow || lenw + 1 <= 8200)) c = CLS_SMALL;
		else if (packable && (lenw + 1 <= 4 * (int64_t)(8 * 3 * 256) || window <= kBandWideWindow)) c = CLS_WIDE;
		// (tl + ql up to 3.5 of its spans: a 12 kb pair at 5 % needs ~6000 of the 7872 columns; 512 x 15 kb @ 5 % — windows of ~7500 — lost 44 pairs to late
		// overflows, 30.7 against 24.9 ms on the span geometry from the start)
		else if (span_ok && R.biased512_ok && R.wide_slots != 3 && (exp_win ? exp_win + 768 <= band_window((int64_t)R.biased512_chunks + 8) : len + 1 <= 7 * (int64_t)((R.biased512_chunks + 8) * 256) / 2)) c = CLS_BIASED;
		else if (span_ok && ((exp_win ? exp_win + 768 <= band_window(R.span_chunks) : len + 1 <= 7 * R.span_chunks * 256) || window <= band_window(R.span_chunks))) c = CLS_SPAN;
	}
	r.fallback = row(c).fallback;
	r.flags = (int8_t)(step0 ? FLAG_STEP0 : 0);
	// the class the pair's lengths would give it, for the admission to the lane and mid kernels where the band kernel itself cannot serve (their offsets are 16 bits too)
	PairClass c_adm = c;
	if (R.small_only && c == CLS_GENERIC && tl + bound < 32767) c_adm = micro_or_tiny(R, std::min<int64_t>(len + 1, 2 * bound + 3), lenw);
	// short pairs: a window of 64 diagonals holds them while the penalty stays below ~45 (a 200 bp pair at 5 %)
	// (in a batch small enough for the mid kernel the lane kernel keeps the pairs of up to 320 bases: 16 x 400 bp 0.31 ms on the lane
	// kernel — pairs that outgrow its chunks are re-run — against 0.13 on the mid kernel, 1 x 300 bp 56 against 68 us; profiles/r04/lane_vs_mid.txt)
	// (the lane kernel's limit is a window — its chunks — and a window is proportional to divergence x length: the weight goes further down for it than for the
	// classes, 2000 x 450 bp @ 2 % 0.14 against 0.27 ms on the 64-thread geometry; profiles/r06/lane_crossover.txt)
	const bool to_lane = (R.classes || R.small_only) && R.lane_on && is_band_size_class(c_adm) && (int64_t)((double)std::max(tl, ql) * R.div_lane) <= R.lane_limit && skew <= 24;
	if (to_lane) c = not_acgt ? CLS_LANE_BYTES : CLS_LANE, r.fallback = R.classes ? CLS_MICRO : CLS_SMALL; // (where an overflow goes: the re-run of "band" pairs takes the mid kernel for a handful, else whatever choose_kernel has for the penalties)
	// a few mid-size pairs: a workgroup each, rings in LDS (a penalty then costs a fraction of what it costs the band kernels).  Admitted
	// when the span the LDS can hold beside the sequences covers the window of a pair at ~6 % divergence (about 0.3 (tl+ql)) and the gap its lengths
	// force — or every column the pair can ever reach; 16-bit offsets.
	if (R.mid_batch && !to_lane && (c == CLS_GENERIC || is_band_size_class(c)) && (!R.low_mem || step0) && tl + bound < 32760) {
		const int64_t seq_lds = ((tl + 7) & ~7LL) + 16 + ((ql + 7) & ~7LL) + 32;
		const int64_t window = std::min<int64_t>(len + 1, 2 * bound + 3);
		const int64_t want = std::min<int64_t>(window, lenw * 34 / 100 + 128) + 2 * P0.nH;
		int groups = (int)std::min<int64_t>((window + 2 * P0.nH + 63) / 64, 128);
		while (groups > 1 && R.mid_lds_bytes(P0, groups, seq_lds) > 158 * 1024) --groups;
		// (the span lies around the middle of diagonals 0 and ql - tl, mwf_mid.hip: all the columns a window can reach — the matrix, or what the penalty
		// bound allows either side of diagonal 0 — plus the dead margins)
		const int64_t C = (int64_t)groups * 64, left = tl + 1 + (ql - tl) / 2 - C / 2, right = left + C - 1;
		const bool holds_all = std::max<int64_t>(1, tl + 1 - (bound + 1)) - P0.nH >= left && std::min<int64_t>(len + 1, tl + 1 + bound + 1) + P0.nH <= right;
		if (R.mid_lds_bytes(P0, groups, seq_lds) <= 158 * 1024 && (holds_all || (C >= want && skew < groups * 32))) {
			if (!allow_mid) {
				// (a large batch: counted; the pairs move to the mid kernel afterwards if they are few, and only the band kernels' SMALL classes give
				// pairs away — wide windows are the 512-thread geometry's work whatever their number)
				r.mid_candidate = c_adm == CLS_TINY || c_adm == CLS_MICRO;
			} else {
				r.fallback = is_band_size_class(c) || (R.classes && packable) ? CLS_SMALL : CLS_GENERIC; // where an overflow goes: the wide packed band kernel, else generic
				c = CLS_MID;
				r.mid_bytes = not_acgt;
			}
		}
	}
	if (((is_band_size_class(c) && packable) || c == CLS_SPAN || c == CLS_BIASED) && R.nib_pair(alpha)) c = is_band_size_class(c) ? CLS_WIDE_NIB : CLS_SPAN_NIB;
	else if (is_band_size_class(c) && not_acgt && packable) c = bytes_twin(c);
	r.cls = c;
	return r;
}

} // namespace host
} // namespace mwf
