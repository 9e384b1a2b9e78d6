// mwf_plan_retry.h — what happens to a pair that did not finish where it ran, stated once: the routes a re-run can take, what the launch of each asks for
// (kRouteTable, in launch order), and the rule that gives an unfinished pair its route (reroute_pair: a pure function, it prints and writes nothing).
// Host only, no HIP header: tests/host/plan_retry.cpp builds the rule stand-alone.  mwf_plan.cpp (finalize) is the one user.
#pragma once
#include "mwf_plan_classes.h"

namespace mwf {
namespace host {

// Where an unfinished pair goes next.  The first kNumRoutes are lists that finalize() launches, in this order within a round; the rest end the call.
enum Route : int8_t {
	ROUTE_COOP_ALONE = 0,  // the whole-device kernel again, the device to itself (and, where the decision says so, a larger arena)
	ROUTE_ENDS_FEWER,      // the ends-free kernel on fewer workgroups (= larger traceback slots)
	ROUTE_GENERIC,         // the generic kernel
	ROUTE_GENERIC32,       // ... with 32-bit ring rows: an offset outgrew (or is forecast to outgrow) the 16-bit ones
	ROUTE_BAND_WIDE,       // the band kernel's 512-thread geometry, by the pairs' forecast windows (a handful of short pairs: the mid kernel)
	ROUTE_BAND_SPAN,       // ... its 1024-thread span geometry
	ROUTE_BAND_BYTES,      // ... its byte-wise form: not plain A/C/G/T
	ROUTE_FEWER_GENERIC,   // the generic kernel on fewer workgroups
	ROUTE_FEWER_BAND,      // the band kernel on fewer workgroups
	kNumRoutes,
	ROUTE_FAIL_TB = kNumRoutes, // the traceback does not fit in device memory
	ROUTE_FAIL_SNAP,            // the low-memory snapshots do not
	ROUTE_FAIL_STATUS           // a status no re-run answers
};
constexpr bool is_failure(Route r) { return r >= kNumRoutes; }

// workgroups of a re-run at most: as many as the align's largest launch had; as many as the kernel keeps resident; finalize()'s tb_slots (an eighth of the last round's), one per pair
enum RouteSlots : int8_t { SLOTS_GRID0 = 0, SLOTS_ALL, SLOTS_TB };
enum RouteLaunch : int8_t { LAUNCH_PAIR = 0, LAUNCH_ENDS, LAUNCH_COOP }; // run_batch_kernel, run_ends_kernel, run_coop_pair (pair by pair: the other fields do not apply)
struct RouteRow {
	const char *name;
	RouteLaunch launch;
	int8_t want_kind;    // LaunchReq::want_kind (3: the ends-free kernel)
	RouteSlots slots;
	bool use_forecast;   // the window hint of the launch: the widest forecast of its pairs (+ 25 %), if every pair came back with one
	Geom geom;
	bool span_if_all;    // ... GEOM_SPAN instead where every pair of the list is of CLS_SPAN
	CopyForm copy;
	bool nib_split;      // "alpha16": the class-3 pairs of the list apart from the rest, on the 4-bit form of the same geometry
	bool ring16_allowed;
};
constexpr RouteRow kRouteTable[kNumRoutes] = {
	{"coop-alone", LAUNCH_COOP, 1, SLOTS_ALL, false, GEOM_CHOOSE, false, COPY_2BIT, false, true},
	{"ends-fewer", LAUNCH_ENDS, 3, SLOTS_TB, false, GEOM_CHOOSE, false, COPY_2BIT, false, true},
	{"generic", LAUNCH_PAIR, 0, SLOTS_GRID0, false, GEOM_CHOOSE, false, COPY_2BIT, false, true},
	{"generic32", LAUNCH_PAIR, 0, SLOTS_GRID0, false, GEOM_CHOOSE, false, COPY_2BIT, false, false},
	{"band-wide", LAUNCH_PAIR, 2, SLOTS_ALL, true, GEOM_CHOOSE, false, COPY_2BIT, true, true},
	{"band-span", LAUNCH_PAIR, 2, SLOTS_ALL, false, GEOM_SPAN, false, COPY_2BIT, true, true},
	{"band-bytes", LAUNCH_PAIR, 2, SLOTS_ALL, false, GEOM_CHOOSE, false, COPY_BYTES, false, true},
	{"fewer-generic", LAUNCH_PAIR, 0, SLOTS_TB, false, GEOM_CHOOSE, false, COPY_2BIT, false, true},
	{"fewer-band", LAUNCH_PAIR, 2, SLOTS_TB, false, GEOM_CHOOSE, true, COPY_2BIT, true, true},
};
// a round in which such a list has pairs divides tb_slots by eight
constexpr bool takes_fewer_slots(Route r) { return kRouteTable[r].slots == SLOTS_TB; }

// What the rule reads besides the pair: fixed for one finalize() (tb_slots: for one round of it).
struct RetryRule {
	int band_span = 1, seq2bit = 1, force_kind = -1, block = 0; // tunables (mwf_gpu_s)
	int64_t tb_budget_mb = 0, coop_tb_mult = 1;
	int32_t step = 0;        // opt.step
	int64_t span_window = 0; // widest window of the band kernel's span geometry
	int tb_slots = 1;
	bool (*coop_can_grow)(void *ctx) = nullptr; // can the whole-device traceback arena still grow?  (asks the device: called only for a pair that reaches the question)
	void *ctx = nullptr;
};
struct PairState {
	int64_t tl = 0, ql = 0;
	int32_t status = 0;
	int8_t kind = 0, h_class = 0, h_flags = 0; // mwf_gpu_batch_t::h_kind, h_class, h_flags
	int64_t n_iter = 0;                        // the pair's n_iter word: a pair handed back EARLY carries the window it is expected to need, negated
};
enum RouteWarning : int8_t { WARN_NONE = 0, WARN_COOP_GAVE_UP, WARN_COOP_SPAN }; // (the second is printed once per finalize())
struct RouteDecision {
	Route route = ROUTE_FAIL_STATUS;
	int step0 = 0;                   // which of the route's two lists: 1 runs as high-memory although opt.step > 0
	int8_t h_class = 0, h_flags = 0; // the pair's new class and flags
	bool wide_needs_four = false, grow_coop = false; // the batch's wide class was shown to need four chunk slots per wave; the whole-device arena doubles
	RouteWarning warn = WARN_NONE;
};

// Where a pair that is neither ST_OK nor ST_STOPPED goes next:
//   window outgrew a band kernel's span   -> the wide band kernel, from there the span geometry or the generic kernel
//   traceback / snapshot arena too small  -> the same kernel on fewer workgroups (= larger slots)
//   whole-device kernel: alone if it shared the device; a larger arena while memory lasts; a wait that gave up or a window beyond the device's span -> the generic kernel
inline RouteDecision reroute_pair(const RetryRule &R, const PairState &p)
{
	RouteDecision d;
	d.h_class = p.h_class, d.h_flags = p.h_flags;
	const int32_t st = p.status;
	const int kind = p.kind, step0 = p.h_flags & FLAG_STEP0;
	auto go = [&](Route r, int z) { d.route = r, d.step0 = z; return d; };
	if (kind == 3) { // an ends-free pair only ever runs on its own kernel: again on fewer workgroups, unless it already had the whole budget
		return go(st != ST_TB_OVERFLOW ? ROUTE_FAIL_STATUS : R.tb_slots == 1 ? ROUTE_FAIL_TB : ROUTE_ENDS_FEWER, 0);
	} else if (st == ST_BAND_OVERFLOW && kind == 0) {
		return go(ROUTE_GENERIC32, step0); // an offset outgrew the generic kernel's 16-bit ring rows: 32-bit rows
	} else if (st == ST_ALPHABET && kind == 2 && p.h_class == CLS_SPAN) {
		d.h_class = CLS_GENERIC; // (the span geometry has no byte-wise form)
		return go(ROUTE_GENERIC, step0);
	} else if (st == ST_ALPHABET && kind == 2) {
		return go(ROUTE_BAND_BYTES, step0); // not plain ACGT: the byte-wise band kernel of the same class
	} else if (st == ST_BAND_OVERFLOW && kind == 2) {
		// (a forecast no band class holds goes straight to the generic kernel)
		const int64_t est = p.n_iter < 0 ? -p.n_iter : 0;
		// (a pair of the wide class that outgrew its three chunk slots per wave LATE — that geometry carries no forecast — is re-run alone, ~7 ms for a
		// 10 kb pair beside the batch's 17: the next align of this batch takes the four-slot geometry for the class)
		// (only a pair that really ran on that geometry says so: CLS_BIASED pairs on biased offsets and re-runs of mid / lane pairs carry CLS_WIDE as well)
		d.wide_needs_four = (p.h_flags & FLAG_THREE_SLOTS) && est == 0;
		d.h_flags = (int8_t)(p.h_flags & ~FLAG_THREE_SLOTS);
		// what outgrew (or is forecast to outgrow) the 512-thread geometry: the 1024-thread span geometry, if the pair fits that
		const bool span_ok = is_band_size_class(p.h_class) && R.band_span != 0 && R.seq2bit != 0 && R.force_kind < 0 && R.block == 0 &&
		                     p.tl <= kBandSpanMaxSeq && p.ql <= kBandSpanMaxSeq && est <= R.span_window;
		// (a forecast the four-slot 512-thread geometry holds — the re-run takes four slots for it; beyond it the span geometry at once:
		// round 4 sent forecasts of up to 1.5 x the THREE-slot window here and re-ran them on three slots, which by their own forecast could not hold them)
		// (every class but generic and wide: a pair of the span geometry whose forecast is that small takes this way too, as it always has)
		if (p.h_class != CLS_GENERIC && p.h_class != CLS_WIDE && est <= kBandWide4Window) return d.h_class = CLS_WIDE, go(ROUTE_BAND_WIDE, step0);
		if (span_ok) return d.h_class = CLS_SPAN, go(ROUTE_BAND_SPAN, step0);
		d.h_class = CLS_GENERIC;
		// (a forecast also says whether the generic kernel's 16-bit ring rows can hold the pair — offsets up to 65 532, i.e. target length
		// + final penalty, about half the window: 50 kb pairs at 15 % ran them for nothing before taking the 32-bit rows)
		return go(est > 0 && p.tl + est / 2 + 64 > 65000 ? ROUTE_GENERIC32 : ROUTE_GENERIC, step0);
	} else if (kind == 1 && st == ST_INTERNAL && !(p.h_flags & FLAG_COOP_GAVE_UP)) {
		// a wait between workgroups of the whole-device kernel ran into its spin limit (they were not all resident, e.g.
		// the device is shared): the one-workgroup kernel needs no such thing
		d.warn = WARN_COOP_GAVE_UP, d.h_flags = (int8_t)(p.h_flags | FLAG_COOP_GAVE_UP);
		return go(ROUTE_GENERIC, step0);
	} else if (kind == 1 && (st == ST_BAND_OVERFLOW || st == ST_TB_OVERFLOW || st == ST_SNAP_OVERFLOW)) {
		if (p.h_flags & FLAG_COOP_SHARED) return go(ROUTE_COOP_ALONE, 0); // had a share of the workgroups and of the arena: now alone
		if (st == ST_BAND_OVERFLOW && (p.h_flags & FLAG_COOP_NARROW) && !(p.h_flags & FLAG_COOP_WIDE)) {
			d.h_flags = (int8_t)(p.h_flags | FLAG_COOP_WIDE); // its window outgrew the 64-column slots: again with 256-column ones
			return go(ROUTE_COOP_ALONE, 0);
		}
		if (st == ST_BAND_OVERFLOW) return d.warn = WARN_COOP_SPAN, go(ROUTE_GENERIC, step0);
		if (R.tb_budget_mb == 0 && R.coop_tb_mult < ((int64_t)1 << 20) && R.coop_can_grow(R.ctx)) return d.grow_coop = true, go(ROUTE_COOP_ALONE, 0);
		if (R.step > 0 && !step0) return go(ROUTE_GENERIC, 0); // the first-pass traceback does not fit: true two-pass mode
		return go(ROUTE_FAIL_TB, step0);
	} else if (st == ST_TB_OVERFLOW || st == ST_SNAP_OVERFLOW) {
		if (R.tb_slots == 1) return go(st == ST_TB_OVERFLOW ? ROUTE_FAIL_TB : ROUTE_FAIL_SNAP, step0); // already had the whole budget
		return go(kind == 2 ? ROUTE_FEWER_BAND : ROUTE_FEWER_GENERIC, step0);
	}
	return go(ROUTE_FAIL_STATUS, step0);
}

} // namespace host
} // namespace mwf
