// mwf_plan.cpp — the plan / launch / retry layer of libmwf_hip.so's host side: penalties, which kernel and geometry serves a set of pairs
// (choose_kernel), the size classes of a batch (mwf_gpu_batch_align; the classes and their rule: mwf_plan_classes.h), one launch of the one-workgroup-per-pair
// kernels (run_batch_kernel) or of the ends-free kernel (run_ends_kernel), the passes of the whole-device kernel (run_coop_group) and the re-runs of what did not
// fit where it ran (finalize; the routes and their rule: mwf_plan_retry.h).  Split from mwf_engine.cpp in round 5 (no behaviour change).
#include "mwf_engine.h"
#include "mwf_plan_retry.h"
#include "mwf_ends_band.h"

namespace mwf {
namespace host {

// ---- penalties, kernel choice -----------------------------------------------------------------------------------------

Penalty make_penalty(const mwf_opt_t &o)
{
	Penalty p;
	p.x = o.x, p.o1 = o.o1, p.o2 = o.o2, p.e1 = o.e1, p.e2 = o.e2;
	p.oe1 = o.o1 + o.e1, p.oe2 = o.o2 + o.e2;
	int32_t mp = std::max(p.x, std::max(p.oe1, p.oe2)); // reference miniwfa.c:390-392
	p.nH = mp + 1, p.n1 = p.e1 + 1, p.n2 = p.e2 + 1;
	return p;
}

const char *validate(const mwf_opt_t &o)
{
	if (o.x < 1 || o.e1 < 1 || o.e2 < 1) return "x, e1 and e2 must be >= 1 (a zero lag would make a wavefront depend on itself)";
	if (o.o1 < 0 || o.o2 < 0) return "gap-open penalties must be >= 0";
	if (std::max<int64_t>(o.x, std::max<int64_t>((int64_t)o.o1 + o.e1, (int64_t)o.o2 + o.e2)) + 1 > kBigRing) return "max(x, o1+e1, o2+e2) must be < 4096";
	if (o.step < 0) return "step must be >= 0";
	return nullptr;
}

// Upper bound on the optimal penalty (mwf_plan_classes.h)
int64_t penalty_bound(const mwf_opt_t &o, int64_t tl, int64_t ql, bool honour_max_s) { return penalty_bound(make_penalty(o), o.max_s, tl, ql, honour_max_s); }

inline int64_t band_span_window() { return band_window(band2_span_chunks()); }

// the per-slot workspace of a launch (size_slots)
struct SlotSizes {
	int32_t W = 0, GW = 0; // row stride (columns), good-bit words per row
	int64_t ring_slot_ints = 0, rows_slot = 0, cig_scratch_slot = 0, tb_slot_bytes = 0;
};

struct Plan {
	int kind = 0;              // 0: generic kernel, 2: band kernel, 3: ends-free kernel
	BandGeom band{0, 0, 0, 0, 0, 0};
	int block = 256, grid = 1;
	SlotSizes ws;
	int64_t snap_slot_ints = 0, snap_meta_slot = 0, seg_slot = 0;
	bool low_mem = false, cigar = false;
	bool ext = false;          // kind 3: the extension form of the kernel (mwf_ext_t)
};

typedef mwf_gpu_batch_t::PlanCache::GI GroupInfo;

// order of pair ids: longest pair first (with std::stable_sort)
static auto longer_first(const mwf_gpu_batch_t *b)
{
	return [b](int32_t x, int32_t y) { return (int64_t)b->h_tl[x] + b->h_ql[x] > (int64_t)b->h_tl[y] + b->h_ql[y]; };
}

// One launch of the one-workgroup-per-pair kernels, as its caller asks for it (run_batch_kernel).
struct LaunchReq {
	mwf_opt_t opt{};
	const int32_t *d_order = nullptr; // the launch's pairs (device) ...
	int32_t n_items = 0;              // ... and how many
	int slots = 1 << 30;              // at most this many workgroups: as many as the chosen kernel can keep resident (retries ask for fewer, larger slots)
	GroupInfo group;                  // the maxima over the launch's pairs
	Geom geom = GEOM_CHOOSE;
	CopyForm copy = COPY_2BIT;
	int want_kind = -1;               // -1: the engine's "force_kind", 0 generic, 2 band
	int64_t window_hint = 0;          // the widest window the pairs are expected to reach (0: unknown)
	bool ring16_allowed = true;       // false: the re-run of pairs whose offsets outgrew the generic kernel's 16-bit ring rows
	int retry_list = 0;               // re-runs without the host: 1 the launch fills the batch's device-side list, 2 the launch takes its pairs from it
	int retry_slot = 0;               // ... which of the batch's kRetrySlots lists
	bool report_wide = false;         // the wide class's measuring launch: four slots, and the kernel notes whether three would have held every pair
	bool timed_begin = false, timed_end = false; // the events that bracket all launches of an align call (not the retries)
};

int cached_occupancy(mwf_gpu_t *g, const Penalty &P, const Plan &pl, int lds_e2_cols, bool stream_pass, bool ring16 = false);

// Which kernel serves a set of pairs.  The band kernel keeps E/F in registers and therefore only holds windows up to
// its span; it has no low-memory first pass.
void choose_kernel(mwf_gpu_t *g, const LaunchReq &rq, const Penalty &P, Plan &pl)
{
	const mwf_opt_t &opt = rq.opt;
	const int want_kind = rq.want_kind >= 0 ? rq.want_kind : g->force_kind; // -1 automatic, 0 generic, 2 band
	const int64_t max_len = rq.group.max_len, max_bound = rq.group.max_bound, max_seq_lds = rq.group.max_seq_lds, max_tl = rq.group.max_tl, window_hint = rq.window_hint;
	Geom geom = rq.geom;
	const bool bytes_only = rq.copy == COPY_BYTES; // pairs that are not plain ACGT: no 2-bit (or 4-bit) copies
	pl.kind = 0;
	const bool low_mem = (opt.flag & MWF_F_CIGAR) && opt.step > 0;
	// packed band kernel (mwf_band2.hip): 16-bit offsets
	const bool can_packed = band2_supported(P) && g->band_pack != 0;
	if (geom == GEOM_LANE && want_kind != 0 && !low_mem && lane_supported(P)) { // the short-pair class: one wave per pair, one diagonal per lane
		// The rows of all chunks are allocated whatever the window does, and LDS is what bounds the waves per CU (four chunks with the default
		// penalties: 14.5 KB, eleven waves; three: thirteen).  Three hold penalties up to ~110: 40 000 x 150 bp @ 5 % 0.68 against 0.79 ms with one
		// pair re-run, 20 000 x 200 bp 0.52 / 0.61 with ten, 20 000 x 150 bp @ 10 % 0.75 / 0.93 with 499 (profiles/r03/lane_kernel_probe.txt).
		const int chunks = g->lane_chunks > 0 ? g->lane_chunks : max_len <= 400 ? 3 : 4;
		// 2-bit sequence copies from ~450 bases of target + query on (measured: 20 000 x 250 bp 0.624 against 0.650 ms with byte copies, 40 000 x
		// 150 bp 0.664 against 0.617 — packing costs more than the shorter extension trips save; profiles/r04/short_reads_step.txt)
		BandGeom lg{64, 1, 64 * chunks, lane_lds_bytes(P, chunks, max_seq_lds), (g->seq2bit != 0 && !bytes_only && max_len >= 450) ? 1 : 0, 1};
		if (lg.lds_bytes <= 60 * 1024) { // (deep rings — large gap-open costs — with a raised lane_max_len: the band classes below take the pairs)
			pl.kind = 2, pl.band = lg;
			return;
		}
	}
	if (geom == GEOM_MID && want_kind != 0 && !low_mem && mid_supported(P)) { // a few mid-size pairs: one workgroup per pair, every ring in LDS (mwf_mid.hip)
		// the span: as many 64-column groups as the LDS holds beside the sequences (a window is about twice the final penalty wide: a 2 kb
		// pair at 5 % needs ~1100 columns), never more than the widest possible window plus the dead margins
		const int64_t want_cols = (std::min<int64_t>(max_len + 1, 2 * max_bound + 3) + 2 * P.nH + 63) / 64 * 64;
		int groups = (int)std::min<int64_t>(want_cols / 64, 128);
		while (groups > 1 && mid_lds_bytes(P, groups, max_seq_lds) > 158 * 1024) --groups;
		const int lds = mid_lds_bytes(P, groups, max_seq_lds);
		if (lds <= 158 * 1024) {
			// eight waves while the windows stay below ~700 columns (pairs of up to ~1.2 kb at 5 %), else sixteen (measured: 1 kb 0.255 against
			// 0.314 ms, 2 kb 0.572 / 0.556, 4 kb 1.60 / 1.43; profiles/mid_kernel_probe.py)
			// (window_hint: the widest window the class's pairs are expected to reach — a pair of very different lengths opens a gap its length does not tell)
			const int64_t by_len = window_hint > 0 ? std::max<int64_t>(max_len, window_hint * 100 / 28) : max_len;
			const int block = g->mid_block ? g->mid_block : (by_len <= 1000 ? 256 : by_len <= 2500 ? 512 : 1024); // (4 x 400 bp: 131 us on four waves, 145 on eight)
			const int seq2 = g->seq2bit != 0 && !bytes_only;
			pl.kind = 2, pl.band = BandGeom{block, 1, 64 * groups, lds, seq2, 2};
			return;
		}
	}
	if (want_kind == 0 || low_mem || !can_packed) return;
	if (geom == GEOM_BIASED) { // the 512-thread geometry with five / six chunk slots on biased offsets (the caller checked the lengths: kBandSpanMaxSeq); 2-bit copies only
		const int64_t need_lds = ((max_len >> 4) + 4) * 4;
		if (g->seq2bit == 0 || bytes_only || need_lds > 70 * 1024 || !band2_biased512_supported(P)) return;
		// (five chunk slots per wave while target + query stay below 3.5 of that span, else six)
		// (... or when the class was admitted on a forecast window — divergence known, window_hint = the class's largest — that five slots cannot hold: the
		// admission test is against the SIX-slot window, a 17 kb pair at 10 % must not start on five and overflow)
		const bool six = max_len + 1 > 7 * (int64_t)(band2_biased512_chunks() * 256) / 2 || (window_hint > 0 && window_hint + 768 > ((int64_t)band2_biased512_chunks() - 1) * 256 - 64);
		const int chunks = band2_biased512_chunks() + (six ? 8 : 0);
		pl.kind = 2, pl.band = BandGeom{512, 2, chunks * 256, (int)((need_lds + 15) / 16 * 16), 1, 0}; // (packed 2: the copy that computes on biased offsets)
		// The geometry is worth its registers only two to a CU.  The launch adds the set's own edge table to the sequence copy — max(e1, e2) + 1 ages of
		// chunks + 2 entries, 2.0 KB for (2,1) on five slots, 3.9 KB for (4,1) on six — so the kernel is asked, with this class's longest pair in LDS:
		// fewer than two resident workgroups, and the pairs take the span geometry as they would without these copies.
		pl.cigar = (opt.flag & MWF_F_CIGAR) != 0;
		if (cached_occupancy(g, P, pl, 0, false) >= 2) return;
		pl.kind = 0, pl.band = BandGeom{0, 0, 0, 0, 0, 0}, geom = GEOM_SPAN;
	}
	if (geom == GEOM_SPAN) { // the span geometry (the caller checked the lengths of every pair: kBandSpanMaxSeq); 2-bit sequence copies only
		// ("alpha16", a launch of class-3 pairs: 4-bit copies — eight bases per dword, 62 000 bases per sequence about 62 KB)
		const bool nib = rq.copy == COPY_NIB && band2_nib_supported(P);
		const int64_t need_lds = nib ? ((max_len >> 3) + 4) * 4 : ((max_len >> 4) + 4) * 4;
		if (g->band_span == 0 || g->seq2bit == 0 || bytes_only || need_lds > 150 * 1024) return;
		pl.kind = 2, pl.band = BandGeom{1024, 1, (int)band2_span_chunks() * 256, (int)((need_lds + 15) / 16 * 16), 1, 0, 0, nib ? 1 : 0};
		return;
	}
	// (window_hint: pairs a kernel handed back early come with the window they are expected to need, dev::window_forecast — the re-run
	// takes the class that fits that, not the one that fits the worst case)
	const int64_t max_window = window_hint > 0 ? std::min<int64_t>(std::min<int64_t>(max_len + 1, 2 * max_bound + 3), window_hint) : std::min<int64_t>(max_len + 1, 2 * max_bound + 3);
	BandGeom bg;
	bg.packed = 0, bg.seq2 = 0, bg.lane = 0, bg.tab = 0, bg.nib = 0;
	// Packed variants (E/F registers as int16 pairs): valid when no offset (a target index, plus at most one per penalty for
	// offsets that ran past the matrix) and no penalty count can reach 32767.  They halve the state registers, which is
	// what lets several workgroups share a CU — one pair's barrier phase then overlaps another's compute:
	//   window <=  448:  64 threads x 3 chunks, sixteen pairs per CU (twelve with traceback): short reads
	//   window <= 1216: 128 threads x 3 chunks, eight pairs per CU (six with traceback)
	//   window <= 2752: 256 threads x 3 chunks, four (three)
	//   wider:          512 x 3, two per CU — with traceback too (35.4 ms on the 1024 x 10 kb batch with ~100 bytes of scratch per
	//                   lane, against 43.4 ms for 768 x 2 with one workgroup per CU)
	// (measured alternatives on the 1024 x 10 kb batch: 1024 threads x 2 chunks spills and runs 50 ms, 768 x 2 42 ms; 768 x 2 at two
	// workgroups per CU — 80 VGPRs, six spilled — 18.2 against 17.8 ms, round 4)
	// Pairs whose offsets do not fit 16 bits take the generic kernel — with 16-bit ring rows where those apply, else 32-bit rows.  (The
	// unpacked band kernel of round 1, mwf_band.hip, lost to it wherever both applied — 512 x 20 kb @ 1 %: 5.4 against 8.0 ms, 512 x 50 kb
	// @ 0.3 %: 4.2 / 5.9, and 1024 x 12 kb @ 5 %: 42 against 101 ms with its window overflows re-run, profiles/r03/mid_pairs_kernels.txt —
	// and was removed in round 4.)
	const bool range_ok = max_tl + max_bound < 32767;
	if (!range_ok) return;
	bg.packed = 1;
	bg.block = max_window <= kBandMicroWindow ? 64 : max_window <= kBandTinyWindow ? 128 : max_window <= kBandSmallWindow ? 256 : 512;
	// forced geometry (tests, tuning)
	if (g->block == 64 || g->block == 128 || g->block == 256 || g->block == 512 || g->block == 768) bg.block = g->block;
	// geometry picked by the caller for a size class (pairs short enough that their window should stay inside a small span)
	if (g->block == 0 && geom_small_block(geom)) bg.block = geom_small_block(geom);
	// "alpha16", a launch of class-3 pairs: the 4-bit form exists on the 512-thread geometry (three or four slots) whatever the window class (a forced 768 stays byte-wise)
	const bool nib = rq.copy == COPY_NIB && g->seq2bit != 0 && !bytes_only && band2_nib_supported(P) && bg.block != 768;
	if (nib) bg.block = 512;
	bg.span = bg.block / 64 * (bg.block != 768 ? 3 : 2) * 256;
	// (a forced 512-thread block with "wide_slots" 4: four slots whatever the window — tests of the four-slot kernels on short pairs)
	const bool four_slots = bg.block == 512 && ((g->block == 0 && window_hint > kBandWideWindow && window_hint <= kBandWide4Window) || (g->block == 512 && g->wide_slots == 4));
	if (four_slots) bg.span = 512 / 64 * 4 * 256;
	if (want_kind != 2 && max_len + 1 > 4 * (int64_t)bg.span) return; // windows will mostly outgrow the span: go generic at once
	const int64_t lds_cap = bg.block >= 768 ? 140 * 1024 : bg.block >= 512 ? 70 * 1024 : bg.block == 256 ? 36 * 1024 : bg.block == 128 ? 18 * 1024 : 9 * 1024;
	// the packed kernel's sequence copy holds 2 bits per base unless that is switched off (or this is the re-run of pairs that
	// are not plain ACGT): a quarter of the LDS, half the LDS instructions per probe
	const bool seq2 = g->seq2bit != 0 && !bytes_only;
	const int64_t need_lds = nib ? ((max_len >> 3) + 4) * 4 : seq2 ? ((max_len >> 4) + 4) * 4 : max_seq_lds;
	bg.lds_bytes = need_lds <= lds_cap ? (int)((need_lds + 15) / 16 * 16) : 0;
	bg.seq2 = seq2 && bg.lds_bytes > 0;
	// byte-wise copy (pairs outside plain ACGT) with wide windows: three slots of state plus six probe words per column do not fit the 128
	// VGPRs two 512-thread workgroups per CU leave each wave (~500 bytes of scratch); 768 x 2 holds the same 24 chunks without spilling
	// Round 6: the byte-wise copy exists in ONE geometry, 768 x 2 (24 chunks like 512 x 3, one workgroup per CU) — whatever the window class or a forced block:
	// pairs outside plain A/C/G/T are rare (reads with an N take the lane kernel's byte-wise copy), and a byte-wise twin of every geometry was 40 % of this
	// kernel family's code.  The 768-thread geometry in turn has no 2-bit form.
	if (bg.block == 768) bg.seq2 = 0, bg.lds_bytes = max_seq_lds <= 140 * 1024 ? (int)((max_seq_lds + 15) / 16 * 16) : 0;
	else if (!bg.seq2) {
		bg.block = 768, bg.span = 768 / 64 * 2 * 256;
		bg.lds_bytes = max_seq_lds <= 140 * 1024 ? (int)((max_seq_lds + 15) / 16 * 16) : 0;
	}
	if (bg.lds_bytes == 0) return; // the packed kernel keeps the sequences in LDS: what does not fit takes the generic kernel
	bg.nib = nib && bg.seq2 && bg.block == 512; // (4-bit copies that do not fit the cap: the byte-wise geometry above)
	pl.kind = 2, pl.band = bg;
	// The table form (mwf_band2_tab.hip): the 512-thread geometry on 2-bit copies, default gap extensions, folded — the first probe of the match extension reads
	// per-position 8-mer tables, one halfword per base of target and query (plus 258 entries of slack) in front of the 2-bit copies.  Worth its LDS only while two
	// workgroups share a CU: the kernel is asked with the launch's real LDS size (a 10 kb pair: 40.7 KB of table + 5 KB of copies + 5.2 KB of bookkeeping words and edge table); otherwise the plain form, wfa_band2_kernel.
	// (the budget only spares the query: a CU's 160 KB over two workgroups, less 6 KB for the bookkeeping words and the edge table — 5.2 KB on four slots; cached_occupancy decides)
	if (g->probe_table && bg.block == 512 && bg.seq2 && !bg.nib && band2_tab_supported(P, g->band_fold)) {
		const int64_t tab = (2 * (max_len + 258) + 15) / 16 * 16;
		const int64_t budget = g->probe_table_lds > 0 ? g->probe_table_lds : (160 / 2 - 6) * 1024;
		if (tab + bg.lds_bytes <= budget) {
			pl.band.tab = (int)tab, pl.band.lds_bytes = (int)(tab + bg.lds_bytes);
			pl.cigar = (opt.flag & MWF_F_CIGAR) != 0;
			// ... and score-only, where band2_tab2_supported holds, with the second gap piece folded as well (mwf_band2_tab2.hip; "band_fold2" 0: never): same LDS, same table
			pl.band.fold2 = (!pl.cigar && g->band_fold2 && band2_tab2_supported(P)) ? 1 : 0;
			if (cached_occupancy(g, P, pl, 0, false) < 2) pl.band = bg;
		}
	}
}

// resident workgroups per CU of a kernel variant (one runtime query per variant and engine)
int cached_occupancy(mwf_gpu_t *g, const Penalty &P, const Plan &pl, int lds_e2_cols, bool stream_pass, bool ring16)
{
	OccKey key;
	if (pl.kind == 3) key.kind = 3, key.block = pl.block, key.ext = pl.ext;
	else if (pl.kind == 2) {
		key.kind = 2, key.block = pl.band.block, key.packed = pl.band.packed, key.lane = pl.band.lane, key.slots512 = pl.band.block == 512 ? pl.band.span / 2048 : 0;
		key.e1 = P.e1, key.e2 = P.e2, key.lds_bytes = pl.band.lds_bytes, key.cigar = pl.cigar, key.seq2 = pl.band.seq2 != 0, key.tab = pl.band.tab > 0, key.nib = pl.band.nib != 0, key.fold2 = pl.band.fold2 != 0;
	} else key.block = pl.block, key.stream_pass = stream_pass, key.ring16 = ring16, key.big_ring = P.nH > kMaxRing, key.lds_e2_cols = lds_e2_cols;
	auto it = g->occ_cache.find(key);
	if (it != g->occ_cache.end()) return it->second;
	const int per = pl.kind == 3 ? ends_kernel_occupancy(pl.block, pl.ext)
	              : pl.kind == 2 && pl.band.lane == 2 ? 1 // (mwf_mid.hip: most of a CU's LDS per workgroup)
	              : pl.kind == 2 && pl.band.lane ? lane_kernel_occupancy(pl.band.lds_bytes, pl.cigar)
	              : pl.kind == 2 ? band2_kernel_occupancy(P, pl.band, pl.cigar)
	              : P.nH > kMaxRing ? bigring_kernel_occupancy()
	                             : batch_kernel_occupancy(pl.block, stream_pass, lds_e2_cols, ring16);
	g->occ_cache[key] = per;
	return per;
}

int64_t tb_budget_bytes(mwf_gpu_t *g)
{
	if (g->tb_budget_mb > 0) return g->tb_budget_mb << 20;
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)8 << 30, tot = fr;
	// leave a fifth of what is free right now alone, and never claim more than a quarter of the device for one engine
	// (the drop-in API is re-entrant: other host threads have engines of their own); the arena is kept between calls
	int64_t b = (int64_t)(fr / 5 * 4) + (int64_t)g->tb.bytes;
	return std::min<int64_t>(b, std::min<int64_t>((int64_t)64 << 30, (int64_t)(tot / 4)));
}

// Per device: one-workgroup-per-pair launches take it shared (just around the launch), the whole-device kernel takes it
// exclusively for its whole run and first waits for everything already running on the device (any engine's stream), so that
// no other kernel of this process holds CUs while its workgroups wait for one another.
std::shared_mutex g_dev_gate[kMaxDevices];

// ---- what the launch functions share ------------------------------------------------------------------------------------

// generic and ends-free kernel: four waves per pair, eight once the windows are wide (measured on 1250 x 50 kb: 708 ms against 782 ms)
static int64_t widest_window(const GroupInfo &G) { return std::min<int64_t>(G.max_len + 1, 2 * G.max_bound + 3); }
static int window_block(int64_t widest) { return widest >= 8192 ? 512 : 256; }
static int window_block(const GroupInfo &G) { return window_block(widest_window(G)); }
// row stride: whole 256-column chunks plus room for the band kernel's neighbour loads past the last chunk; a good-bit word per 64 columns
static void set_row_stride(SlotSizes &ws, int64_t max_len) { ws.W = (int32_t)((max_len + 3 + 255) / 256 * 256 + 512), ws.GW = ws.W / 64 + 2; }
// traceback bytes of a pair at worst: every penalty as wide as the whole matrix
static int64_t tb_worst(const GroupInfo &G) { return (G.max_bound + 1) * (G.max_len + 1) + 8 * (G.max_bound + 2); }

// ---- ends-free and extension launches under per-pair bands (mwf_ends_band.h) ----
// One more pair of an ends-free launch's maxima: its penalty bound — the banded one where the batch's last align has bands (gap(tl) + gap(ql) leaves the
// band) — and, as the window it is expected to reach, the width of its clamped band.
static void ends_group_add(const mwf_gpu_batch_t *b, GroupInfo &G, int32_t i, const Penalty &P, int32_t max_s)
{
	const int64_t tl = b->h_tl[i], ql = b->h_ql[i];
	if (!b->band_last) { G.add(tl, ql, penalty_bound(P, max_s, tl, ql, true), 0, 0); return; }
	const mwf_band_t &B = b->h_band[(size_t)i];
	G.add(tl, ql, ends_band_penalty_bound(P.x, P.o1, P.e1, P.o2, P.e2, max_s, tl, ql, true), 0, band_clamped(tl, ql, B.d_lo, B.d_hi).width());
}
// the widest window of such a launch: the band's width where there is one
static int64_t ends_widest_window(const mwf_gpu_batch_t *b, const GroupInfo &G)
{
	const int64_t w = widest_window(G);
	return b->band_last ? std::min<int64_t>(w, std::max<int64_t>(G.max_exp_win, 1)) : w;
}

// The workspace of `grid` slots of a one-workgroup-per-pair launch, sized and allocated: rings, good bits and, in CIGAR mode, traceback arena (a slot holds `worst`
// bytes, or its share of the budget), row metadata and CIGAR scratch.  The traceback budget is looked up here, and only when the arena has to grow.
static int size_slots(mwf_gpu_t *g, const Penalty &P, const GroupInfo &G, int grid, bool cigar, int64_t worst, bool rings_in_lds, SlotSizes &ws)
{
	set_row_stride(ws, G.max_len);
	ws.ring_slot_ints = rings_in_lds ? 64 : (int64_t)(P.nH + 2 * P.n1 + 2 * P.n2) * ws.W;
	const size_t S = (size_t)grid;
	if (ensure(g, g->ring, S * ws.ring_slot_ints * 4)) return -1;
	if (ensure(g, g->good, S * (size_t)P.nH * ws.GW * 8)) return -1;
	if (!cigar) return 0;
	ws.rows_slot = G.max_bound + 2, ws.cig_scratch_slot = G.max_len + 2;
	// the device is only asked how much is free when the arena at hand cannot hold the worst case
	int64_t per = worst;
	if ((int64_t)g->tb.bytes < (int64_t)S * worst || g->tb_budget_mb > 0) per = std::min(per, std::max<int64_t>(tb_budget_bytes(g), (int64_t)g->tb.bytes) / (int64_t)S);
	if (g->tb_budget_mb > 0) per = std::min(per, (g->tb_budget_mb << 20) / (int64_t)S);
	ws.tb_slot_bytes = std::max<int64_t>(4096, per) / 4 * 4; // rows are padded to dwords
	if (ensure(g, g->tb, S * (size_t)ws.tb_slot_bytes)) return -1;
	if (ensure(g, g->row_off, S * (size_t)ws.rows_slot * 8)) return -1;
	if (ensure(g, g->row_lo, S * (size_t)ws.rows_slot * 4)) return -1;
	return ensure(g, g->cig_scratch, S * (size_t)ws.cig_scratch_slot * 4);
}

// What every launch sets the same way: inputs (remapped: "alpha_remap", class-1 pairs' offsets lead to their copies), penalties and limits, the per-slot arrays and
// their sizes, CIGAR pool, outputs.
static void fill_args(BatchArgs &a, const mwf_gpu_t *g, const mwf_gpu_batch_t *b, const mwf_opt_t &opt, const Penalty &P, bool cigar, const SlotSizes &ws, bool remapped)
{
	a.seqs = b->d_seqs, a.t_off = remapped ? b->d_rt_off : b->d_t_off, a.q_off = remapped ? b->d_rq_off : b->d_q_off, a.tl = b->d_tl, a.ql = b->d_ql;
	a.pen = P, a.want_cigar = cigar ? 1 : 0, a.max_s = opt.max_s, a.max_iter = opt.max_iter;
	a.debug_pair = b->debug_pair;
	a.ring = (int32_t*)g->ring.p, a.ring_slot_ints = ws.ring_slot_ints, a.W = ws.W, a.good = (unsigned long long*)g->good.p, a.GW = ws.GW;
	a.tb = cigar ? (uint8_t*)g->tb.p : nullptr, a.tb_slot_bytes = ws.tb_slot_bytes;
	a.row_off = cigar ? (int64_t*)g->row_off.p : nullptr, a.row_lo = cigar ? (int32_t*)g->row_lo.p : nullptr, a.rows_slot = ws.rows_slot;
	a.cig_scratch = cigar ? (uint32_t*)g->cig_scratch.p : nullptr, a.cig_scratch_slot = ws.cig_scratch_slot;
	a.cig_pool = b->d_cig_pool, a.cig_head = b->d_cig_head, a.cig_pool_words = b->cig_pool_words;
	a.out_s = b->d_s, a.out_iter = b->d_iter, a.out_ncig = b->d_ncig, a.out_cigoff = b->d_cigoff;
	a.out_status = b->d_status, a.out_cells1 = b->d_cells1, a.out_dbg = b->d_dbg4;
}

// A fresh work counter: the first kQueueSlots launches of an align call use the ones its reset kernel zeroed, the others zero the first.
static int take_counter(mwf_gpu_t *g, int32_t *&queue)
{
	if (g->queue_clean && g->queue_next < kQueueSlots) { queue = (int32_t*)g->queue.p + g->queue_next++; return 0; }
	queue = (int32_t*)g->queue.p;
	HIP_TRY(g, hipMemsetAsync(g->queue.p, 0, 4, g->stream)); // (stream order: the launch that used it last is complete by then)
	return 0;
}

// The launch itself, not while a whole-device kernel runs; the events that bracket the kernels of an align call (every workspace allocation is already done); the
// batch's largest grid and the engine's record of its last launch.
template <class Launch>
static int launch_gated(mwf_gpu_t *g, mwf_gpu_batch_t *b, const LaunchReq &rq, const Plan &pl, int packed, const char *what, Launch launch)
{
	if (rq.timed_begin) HIP_TRY(g, hipEventRecord(g->ev0, g->stream));
	std::shared_lock<std::shared_mutex> gate(g_dev_gate[g->device % kMaxDevices]);
	const int lrc = launch();
	gate.unlock();
	if (lrc != 0) { g->err = what; return -1; }
	b->last_grid = std::max(b->last_grid, pl.grid);
	if (rq.timed_end) HIP_TRY(g, hipEventRecord(g->ev1, g->stream));
	g->ev_pending |= rq.timed_end;
	g->stats.n_launches += 1;
	g->stats.grid = std::max(g->stats.grid, pl.grid), g->stats.block = pl.block, g->stats.kernel_kind = pl.kind;
	g->stats.packed = packed, g->stats.lowmem_two_pass = pl.low_mem ? 1 : 0;
	return 0;
}

// Run the one-workgroup-per-pair kernel over the request's pairs on at most rq.slots workgroups; *ran_kind: the kernel that took them (0 generic, 2 band).
int run_batch_kernel(mwf_gpu_t *g, mwf_gpu_batch_t *b, const LaunchReq &rq, int *ran_kind)
{
	const mwf_opt_t &opt = rq.opt;
	const int32_t n_items = rq.n_items;
	const int64_t max_len = rq.group.max_len, max_bound = rq.group.max_bound, max_bound1 = rq.group.max_bound1, max_tl = rq.group.max_tl;
	int slots = rq.slots;
	const Penalty P = make_penalty(opt);
	Plan pl;
	pl.cigar = (opt.flag & MWF_F_CIGAR) != 0;
	pl.low_mem = pl.cigar && opt.step > 0;
	pl.block = g->block > 0 && g->block != 768 ? g->block : window_block(rq.group);
	choose_kernel(g, rq, P, pl);
	// `slots` is an upper bound from the caller (retries ask for fewer, larger slots); the chosen kernel's own residency
	// bounds it as well
	int per_cu, lds_e2_cols = 0;
	bool ring16 = false;
	if (pl.kind == 2) {
		pl.block = pl.band.block;
		per_cu = cached_occupancy(g, P, pl, 0, false);
	} else {
		// wide windows (the 512-thread choice above), default gap extension: E2/F2 stay in LDS while the window fits 16 k columns
		if (g->lds_e2 && pl.block == 512 && g->block == 0 && P.e2 == 1 && !g->scalar_generic && !pl.low_mem && P.nH <= kMaxRing) {
			lds_e2_cols = 16384;
			// 16-bit ring rows halve the traffic of this HBM-bound kernel.  An offset is a target index (or runs past the matrix by
			// at most one per penalty), so they hold while target length + penalty < 65530: taken optimistically for pairs whose
			// penalty would have to exceed an eighth of their length to break that; a pair that does comes back as
			// ST_BAND_OVERFLOW and is re-run with 32-bit rows.  The LDS copy of E2/F2 is coded the same way: 64 KB instead of 128.
			// Round 2 took them only for batches of at least as many pairs as CUs (with fewer the decoding and coding of the rows was pure
			// overhead: 64 x 50 kb 88 ms against 73).  With the recurrence on the packed codes and 2-bit sequence copies the 16-bit kernel is
			// the faster one at every batch size (profiles/ring16_small_batches.py: 8 pairs 63.8 against 67.4 ms, 64: 67.9 / 71.3, 200: 72.6 /
			// 90.7; with traceback 67.6 / 77.8 ... 71.9 / 103.9): taken whenever the offsets fit.
			// (round 5: where the batch's divergence is known — estimate_divergence — the penalty is guessed from it, ~5.2 per diverged base
			// with the default costs plus a third: 50 kb pairs at 5 % reach penalty 12 500 and never fitted, 64 of 64 were run twice)
			const int64_t s_guess = b->div_est > 0 && g->div_aware ? (int64_t)(6.9 * b->div_est * (double)max_tl) + 256 : max_len / 8;
			ring16 = g->ring16 != 0 && rq.ring16_allowed && max_tl + std::max<int64_t>(s_guess, max_len / 8) < 65500;
			// 32-bit: one workgroup per CU either way (128 KB of LDS): twelve waves fit its 168-VGPR budget, 490 ms against 519 ms with eight
			// 16-bit: 512 threads, two workgroups per CU (64 KB of LDS each, 128 VGPRs) — 354 ms on 1250 x 50 kb against 375 ms for
			// 768 threads and one per CU (479 ms with 32-bit rows); with traceback the 512-thread copy spills too much: 768 (451 against 477 ms)
			// (the built LDS2 forms are listed once, mwf_kernels.hip with_generic_form; launch_batch and batch_kernel_occupancy answer -1 / 0 for any other:
			// a new choice here needs its instantiation there)
			pl.block = ring16 ? (pl.cigar ? 768 : 512) : 768;
		}
		if (P.nH > kMaxRing) pl.block = 256; // the big-ring form of the generic kernel (launch_batch): one column per lane, 256 threads
		per_cu = cached_occupancy(g, P, pl, lds_e2_cols, !g->scalar_generic, ring16);
	}
	slots = std::max(1, std::min(slots, g->n_cu * std::max(1, per_cu)));
	if (P.nH > kMaxRing) {
		// a deep ring is (nH + 2 n1 + 2 n2) rows of tl+ql columns per resident workgroup (times two in low-memory mode): fewer
		// workgroups rather than a tenth of the device in rings
		const int64_t per_slot = (int64_t)(P.nH + 2 * P.n1 + 2 * P.n2) * ((max_len + 3 + 255) / 256 * 256 + 512) * 4 * (pl.low_mem ? 2 : 1);
		slots = (int)std::max<int64_t>(1, std::min<int64_t>(slots, (int64_t)(g->total_mem / 10) / std::max<int64_t>(per_slot, 1)));
	}
	pl.grid = std::max(1, std::min<int>(slots, n_items));
	if (getenv("MWF_DEBUG"))
		fprintf(stderr, "[libmwf_hip] kernel kind %d: block %d packed %d lds %d B, %d workgroup(s) per CU, %d slots, %d pairs; span %d seq2 %d lane %d tab %d nib %d grid %d hint %lld\n", pl.kind, pl.block,
		        pl.band.packed, pl.band.lds_bytes, per_cu, slots, n_items, pl.band.span, pl.band.seq2, pl.band.lane, pl.band.tab, pl.band.nib, pl.grid, (long long)rq.window_hint);
	int64_t worst = tb_worst(rq.group);
	// the second pass of the low-memory mode collapses the band to one diagonal at every checkpoint (miniwfa.c:413-416) and consecutive
	// checkpoints are at most step+nH penalties apart, so a row is never wider than about 2*(step+nH)
	if (pl.low_mem && opt.step > 2 * P.nH) worst = std::min(worst, (max_bound + 1) * std::min<int64_t>(max_len + 1, 2 * (int64_t)(opt.step + 2 * P.nH) + 8) + 8 * (max_bound + 2));
	if (pl.kind == 2 && pl.band.lane == 1) worst = (std::min<int64_t>(max_bound, 256) + 2) * pl.band.span; // its rows: the span wide, fewer than 256 of them
	if (pl.kind == 2 && pl.band.lane == 2) worst = (max_bound + 2) * pl.band.span;                          // rows of the span's width, one per penalty
	if (size_slots(g, P, rq.group, pl.grid, pl.cigar, worst, pl.kind == 2 && pl.band.lane, pl.ws)) return -1; // (the lane and mid kernels' rings are in LDS)
	const size_t S = (size_t)pl.grid;
	if (pl.low_mem) {
		const int64_t NS = P.nH + 2 * P.n1 + 2 * P.n2;
		const int64_t n_snap_max = max_bound1 / opt.step + 2; // first pass: bound without max_s
		pl.seg_slot = n_snap_max;
		pl.snap_meta_slot = n_snap_max * (4 + 4 * NS);
		// a snapshot holds every array-slice of the shadow ring; windows are at most min(2s+1, whole matrix) wide
		int64_t worst = 0;
		for (int64_t j = 1; j <= n_snap_max; ++j)
			worst += NS * std::min<int64_t>(max_len + 1, 2 * j * opt.step + 3);
		const int64_t budget = (int64_t)(std::max<int64_t>(tb_budget_bytes(g), (int64_t)g->snap.bytes) / 4 / (int64_t)S);
		pl.snap_slot_ints = std::max<int64_t>(1024, std::min(worst, budget));
		if (ensure(g, g->sring, S * pl.ws.ring_slot_ints * 4)) return -1;
		if (ensure(g, g->snap, S * (size_t)pl.snap_slot_ints * 4)) return -1;
		if (ensure(g, g->snap_meta, S * (size_t)pl.snap_meta_slot * 4)) return -1;
		if (ensure(g, g->seg, S * (size_t)pl.seg_slot * 8)) return -1;
	}

	BatchArgs a;
	memset(&a, 0, sizeof(a));
	fill_args(a, g, b, opt, P, pl.cigar, pl.ws, b->alpha_active);
	a.order = rq.d_order, a.n_pairs = n_items;
	a.timeline = g->timeline;
	// A launch of one workgroup per pair on the kernels that take it (lane, mid, packed band) needs no work counter: workgroup i aligns
	// pair i.  Otherwise a fresh counter (take_counter).  The lane kernel takes a set of 64 counters (kLaneCounters above).
	if (pl.kind == 2 && pl.band.lane == 1 && n_items > pl.grid) {
		a.queue_parts = kLaneCounters;
		if (g->queue_clean && g->lane_set_next < kLaneSets) a.queue = (int32_t*)g->queue.p + kQueueSlots + (g->lane_set_next++) * kLaneCounters * kLaneStride;
		else {
			a.queue = (int32_t*)g->queue.p + kQueueSlots;
			HIP_TRY(g, hipMemsetAsync(a.queue, 0, (size_t)kLaneCounters * kLaneStride * 4, g->stream)); // (stream order: the launch that used it last is complete by then)
		}
	} else if (pl.kind == 2 && pl.band.lane == 1) a.queue = nullptr;
	else if (pl.kind == 2 && (pl.band.lane || pl.band.packed) && n_items <= pl.grid && !g->queue_clean) a.queue = nullptr;
	else if (take_counter(g, a.queue)) return -1;
	// re-runs without the host (BatchArgs::retry_ids): this launch fills the batch's list / takes its pairs from it
	if (rq.retry_list == 1) a.retry_ids = b->d_retry_ids + rq.retry_slot * kRetryCap, a.retry_cap = kRetryCap, a.retry_count = (unsigned int*)(b->d_cig_head + 2 + rq.retry_slot);
	if (rq.retry_list == 2) a.n_pairs_dev = (const unsigned int*)(b->d_cig_head + 2 + rq.retry_slot), a.queue = nullptr, a.queue_parts = 0;
	a.scalar_generic = g->scalar_generic;
	a.band_fold = g->band_fold ? 1 : 0;
	a.lds_e2_cols = lds_e2_cols;
	a.ring16 = ring16 ? 1 : 0;
	a.lane_chunks = pl.kind == 2 && pl.band.lane ? pl.band.span / 64 : 0;
	a.step = pl.low_mem ? opt.step : 0;
	a.sring = pl.low_mem ? (int32_t*)g->sring.p : nullptr;
	// block mode leaves up to one partly used block per workgroup behind; the pool's slack (batch_common) covers kCigBlockGrid of them per align —
	// one align can make several block-mode launches (size classes, byte-wise twins, re-runs): a launch the slack no longer covers takes words singly
	a.cig_block = 0;
	if (b->cig_block > 0 && pl.grid <= b->cig_block_left) a.cig_block = b->cig_block, b->cig_block_left -= pl.grid;
	a.report_wide = rq.report_wide ? 1 : 0;
	a.snap = pl.low_mem ? (int32_t*)g->snap.p : nullptr, a.snap_slot_ints = pl.snap_slot_ints;
	a.snap_meta = pl.low_mem ? (int32_t*)g->snap_meta.p : nullptr, a.snap_meta_slot = pl.snap_meta_slot;
	a.seg = pl.low_mem ? (int32_t*)g->seg.p : nullptr, a.seg_slot = pl.seg_slot;
	a.dbg = b->debug_pair >= 0 ? (int32_t*)g->dbg.p : nullptr;
	a.dbg_cap = b->debug_pair >= 0 ? (int32_t)(g->dbg.bytes / 8) : 0;

	const int packed = pl.kind == 2 ? (pl.band.lane == 2 ? 33 : pl.band.lane ? 32 : (pl.band.packed ? 1 : 0)) : (ring16 ? 16 : 0);
	if (ran_kind) *ran_kind = pl.kind;
	return launch_gated(g, b, rq, pl, packed, "kernel launch failed", [&] {
		return pl.kind == 2 && pl.band.lane == 2 ? launch_mid(a, pl.grid, pl.band.block, pl.band.lds_bytes, pl.band.seq2 != 0, g->stream)
		     : pl.kind == 2 && pl.band.lane ? launch_lane(a, pl.grid, pl.band.lds_bytes, pl.band.seq2 != 0, g->stream)
		     : pl.kind == 2 ? launch_band2(a, pl.grid, pl.band, g->stream)
		                    : launch_batch(a, pl.grid, pl.block, g->stream);
	});
}

// One launch of the ends-free kernel (mwf_ends.hip) over the request's pairs on at most rq.slots workgroups, under the batch's allowances (b->ends); of the request it
// reads the options, the pairs, the slots, the maxima and the events.  The workspace is the generic kernel's: the penalty of the global problem bounds the ends-free
// one (the global alignment is one of the alignments it chooses from).
int run_ends_kernel(mwf_gpu_t *g, mwf_gpu_batch_t *b, const LaunchReq &rq, int *ran_kind)
{
	const mwf_opt_t &opt = rq.opt;
	const Penalty P = make_penalty(opt);
	Plan pl;
	const int64_t widest = ends_widest_window(b, rq.group);
	pl.kind = 3, pl.cigar = (opt.flag & MWF_F_CIGAR) != 0, pl.block = window_block(widest); // (without bands: window_block(rq.group))
	pl.ext = b->ext_last; // (the form follows the batch, not the request: finalize()'s re-runs repeat the align's mode)
	const int per_cu = cached_occupancy(g, P, pl, 0, false);
	const int slots = std::max(1, std::min(rq.slots, g->n_cu * std::max(1, per_cu)));
	pl.grid = std::max(1, std::min<int>(slots, rq.n_items));
	// (under bands no row of the traceback is wider than the widest band)
	const int64_t worst = b->band_last ? (rq.group.max_bound + 1) * widest + 8 * (rq.group.max_bound + 2) : tb_worst(rq.group);
	if (size_slots(g, P, rq.group, pl.grid, pl.cigar, worst, false, pl.ws)) return -1;
	if (getenv("MWF_DEBUG"))
		fprintf(stderr, "[libmwf_hip] kernel kind 3: block %d, %d workgroup(s) per CU, %d slots, %d pairs; grid %d, traceback %lld B per slot\n", pl.block, per_cu, slots, rq.n_items, pl.grid, (long long)pl.ws.tb_slot_bytes);

	EndsArgs e;
	memset(&e, 0, sizeof(e));
	BatchArgs &a = e.b;
	fill_args(a, g, b, opt, P, pl.cigar, pl.ws, false); // (always the original bytes)
	a.order = rq.d_order, a.n_pairs = rq.n_items;
	if (take_counter(g, a.queue)) return -1;
	a.debug_pair = -1, a.out_dbg = nullptr;
	e.t_beg = b->ends.t_beg, e.t_end = b->ends.t_end, e.q_beg = b->ends.q_beg, e.q_end = b->ends.q_end;
	e.out_range = b->d_range, e.sub_t_off = b->d_sub_t_off, e.sub_q_off = b->d_sub_q_off, e.sub_tl = b->d_sub_tl, e.sub_ql = b->d_sub_ql;
	e.ext = pl.ext, e.match = b->ext.match, e.zdrop = b->ext.zdrop, e.out_info = b->d_ext_info;
	e.pp_ends = b->pp_ends_last ? b->d_pp_ends : nullptr, e.pp_band = b->band_last ? b->d_pp_band : nullptr; // (as the form: what the batch's last align read)
	if (ran_kind) *ran_kind = 3;
	return launch_gated(g, b, rq, pl, 0, "kernel launch failed (ends-free)", [&] { return launch_ends(e, pl.grid, pl.block, g->stream); });
}

// ---- whole-device kernel ------------------------------------------------------------------------------------------------

// Its workgroups wait for one another, so all of them must be resident: launches on one device are serialised process-wide
// (two host threads' engines would otherwise starve each other until the spin limit), and the call returns after the kernels
// completed.  Other processes' kernels can still hold CUs; that is what the bounded waits and the fallback are for.

int coop_grid_limit(mwf_gpu_t *g)
{
	if (g->coop_grid < 0) g->coop_grid = std::min(sys_max_grid(), g->n_cu);
	return g->coop_grid_cap > 0 ? std::min(g->coop_grid, g->coop_grid_cap) : g->coop_grid;
}

// Workgroups per pair when `n` pairs of at most `len` columns share the device: as many as the widest possible window can
// use when the pair is alone (it can then never outgrow them); when several pairs run side by side, as many as a window of
// a third of tl+ql needs (windows stay near a quarter at 3-5 % divergence) — a pair that does outgrow its group is re-run
// alone by finalize().  The per-penalty latency does not depend on the group size (C4-like 150 kb pair: 151 ms on 256
// workgroups, 141 ms on 64), so pairs side by side multiply the throughput.
int coop_group_size(int n_cu, int64_t len, bool alone, int ow = 256)
{
	int G = n_cu;
	// (the systolic kernel's slots own `ow` = 240 of their 256 columns, and a few chunks beyond the window take part)
	const int64_t chunks = alone ? len / ow + (ow == 256 ? 3 : 8) : len / ow / 3 + (ow == 256 ? 8 : 12);
	while (G > (alone ? 64 : 16) && chunks <= coop_chunk_slots(G / 2)) G /= 2;
	return G;
}

// Up to n_cu / group size pairs side by side on the whole-device kernel, each on its own group of workgroups (mwf_sys.hip).
// Everything is enqueued on the stream: first pass, and in low-memory mode the checkpoint walk over its traceback matrix
// and the second pass, then traceback + outputs.
int run_coop_group(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t &opt, const std::vector<int32_t> &pairs, int Gs, bool first, bool last)
{
	const Penalty P = make_penalty(opt);
	const bool cigar = (opt.flag & MWF_F_CIGAR) != 0, low_mem = cigar && opt.step > 0;
	const int n_groups = (int)pairs.size();
	if (n_groups < 1 || Gs < 1 || (int64_t)Gs * n_groups > coop_grid_limit(g)) { g->err = "whole-device kernel cannot be made resident"; return -1; }
	GroupInfo M;
	bool traced = false;
	for (int32_t pair : pairs) {
		M.add(b->h_tl[pair], b->h_ql[pair], penalty_bound(opt, b->h_tl[pair], b->h_ql[pair], true), penalty_bound(opt, b->h_tl[pair], b->h_ql[pair], false), 0);
		traced |= b->debug_pair == pair;
	}
	const int64_t len = M.max_len, bound = M.max_bound, bound1 = M.max_bound1;
	SlotSizes ws; // (per pair; the systolic passes below get their own ring and good-bit shapes, set_cols())
	set_row_stride(ws, len);
	ws.ring_slot_ints = (int64_t)P.nH * ws.W;
	const int64_t TC = coop_chunk_slots(Gs);
	const size_t NG = (size_t)n_groups;
	const int sysP = g->sys_p, sysP2 = g->sys_p;
	// Columns per lane of the systolic kernel, per pass: one column per lane (64-column slots that own 48) quarters the
	// per-column work a wave does per penalty — what a chain of penalties on a narrow window waits for — but needs five times
	// the slots; taken while the window is EXPECTED to fit them (first pass: a fifth of tl+ql, real pairs stay far below;
	// second pass of the low-memory mode: the band collapses at every checkpoint, miniwfa.c:413-416).  A pair whose window
	// outgrows the slots comes back as ST_BAND_OVERFLOW and is re-run with four columns per lane (finalize()).
	auto window_cap = [&](int c) -> int64_t { return (TC - 4) * (int64_t)sys_owned_cols(sysP, c) - 2 * (257 + sysP); };
	bool wide_again = false;
	for (int32_t pair : pairs) wide_again |= (b->h_flags[pair] & FLAG_COOP_WIDE) != 0;
	// (first-pass window: a fifth of tl+ql — or, where the batch's divergence is known, 6.5 d (tl+ql): 50 kb pairs at 15 % outgrew the 64-column slots and ran twice)
	const int64_t est1 = std::min<int64_t>(len + 1, std::max<int64_t>(8192, b->div_est > 0 && g->div_aware ? (int64_t)(6.5 * b->div_est * (double)len) : len / 5));
	const int64_t est2 = std::min<int64_t>(len + 1, 2 * ((int64_t)opt.step + 2 * P.nH) + 8);
	const int c_first = g->sys_c ? g->sys_c : (!wide_again && est1 <= window_cap(1)) ? 1 : 4;
	const int c_second = g->sys_c ? g->sys_c : (!wide_again && est2 <= window_cap(1)) ? 1 : 4;
	// (the systolic kernel has private H rings per chunk slot, sys_ring below: no ring of whole rows — 1 GB for the 5 Mb pair — is allocated here any more)
	// Low-memory mode (opt.step > 0), two ways to the checkpoints:
	//   walk     — the first pass stores its whole traceback (s^2 bytes: 55 GB for the 5 Mb pair) and the checkpoints are
	//              read off it by walking the recorded choices back (fast while that fits the budget);
	//   two-pass — the reference's way (miniwfa.c:551-601): the first pass stores no traceback, carries provenance through
	//              shadow registers / rows and takes a snapshot every `step` penalties: a few GB for the 5 Mb pair.
	// Chosen by what the walk variant's arena would be against the budget ("lowmem_budget_mb", default 8 GB).
	bool two_pass = false;
	if (low_mem) {
		// automatic: 8 GB.  opt.step > 0 asks for the reference's low-memory mode (miniwfa.c:551-601; README.md:55-64: the 5 Mb MHC pair in 4 GB
		// instead of 50): a first pass that would hold more traceback than that takes the two-pass form — provenance carried through the
		// systolic kernel, snapshots of (nH + 2 e1 + 2 e2) array-slices every `step` penalties — and the device footprint stays within a few GB.
		const int64_t budget = g->lowmem_budget_mb > 0 ? g->lowmem_budget_mb << 20 : (int64_t)8 << 30;
		two_pass = std::max<int64_t>((int64_t)1 << 30, 6000 * len) * (int64_t)NG * g->coop_tb_mult * (c_first == 1 ? 12 : 9) / 8 > budget;
	}
	// misc, per group: flags | +1024 barrier words | +2048 pass state
	const size_t misc_bytes = 4096;
	if (ensure(g, g->coop_misc, NG * misc_bytes + 4096)) return -1; // (+ the pair ids behind the last group)
	int64_t rows_slot = 0, tb_bytes = 0, cig_scratch = 0, seg_slot = 0;
	if (cigar) {
		rows_slot = std::max(bound, bound1) + 2;
		cig_scratch = len + 2;
		// Arena: the worst case (every row as wide as the matrix) is out of reach for long pairs, so start from a cap that
		// holds the real ones (s^2 bytes: 51 GB for the MHC pair) and let finalize() double it after an overflow.  An
		// arena that is already large enough is reused as is, so repeated calls never re-allocate.
		// (first guess: 6000 bytes per column of the matrix' perimeter — 1.8 GB for a 150 kb pair that needs 0.7, 60 GB for the
		// 5 Mb pair that needs 55: a traceback of s^2 bytes with s about 2.5 % of tl+ql)
		const int64_t worst = NG * (rows_slot + 1) * (len + 8);
		int64_t guess = std::min<int64_t>(g->coop_tb_cap, std::max<int64_t>((int64_t)1 << 30, 6000 * len) * (int64_t)NG);
		// two-pass: only the second pass stores traceback, and its rows are at most about 2*(step+nH) wide (the band collapses
		// to one diagonal at every checkpoint, miniwfa.c:413-416); s is guessed as 3 % of tl+ql
		if (two_pass) guess = std::min<int64_t>(guess, std::max<int64_t>((int64_t)64 << 20, (len * 3 / 100 + 1024) * std::min<int64_t>(len + 1, 2 * (int64_t)(opt.step + 2 * P.nH) + 8)) * (int64_t)NG);
		// (the systolic kernel stores 256 bytes per penalty and chunk slot that takes part, a few slots beyond the window included)
		const int64_t lay = (two_pass ? c_second : c_first) == 1 ? 12 : (two_pass ? c_second : c_first) == 2 ? 10 : 9; // the pass whose traceback sets the size: 64-column slots own 48 (4/3 of the exact rows), 256-column ones 240 (the second pass of the low-memory mode is narrow: it fits whatever the first needed)
		// (+ a few slots of margin per epoch of 256 penalties; epochs by the guessed penalty, not by the worst case — 10 M penalties for the 5 Mb pair, 20 GB of margin)
		const int64_t ep_guess = (len * 3 / 100 + 1024) / 256 + 2;
		guess = std::min<int64_t>(g->coop_tb_cap, guess / 8 * lay + ep_guess * 8 * 65536 * (int64_t)NG);
		int64_t want = std::min(worst / 8 * lay + (rows_slot / 256 + 2) * 8 * 65536 * (int64_t)NG, g->tb_budget_mb > 0 ? (g->tb_budget_mb << 20) : guess * g->coop_tb_mult);
		if ((int64_t)g->tb.bytes >= want) want = (int64_t)g->tb.bytes;
		else {
			size_t fr = 0, tot = 0;
			if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)8 << 30;
			want = std::min<int64_t>(want, (int64_t)(fr / 10 * 9) + (int64_t)g->tb.bytes);
		}
		tb_bytes = std::max<int64_t>(4096, want / (int64_t)NG) / 4 * 4; // per pair
		if (ensure(g, g->row_off, NG * (size_t)rows_slot * 8)) return -1;
		if (ensure(g, g->row_lo, NG * (size_t)rows_slot * 4)) return -1;
		if (ensure(g, g->cig_scratch, NG * (size_t)cig_scratch * 4)) return -1;
		if (low_mem) {
			seg_slot = bound1 / opt.step + 2;
			if (ensure(g, g->seg, NG * (size_t)seg_slot * 8)) return -1;
		}
		if (ensure(g, g->tb, NG * (size_t)tb_bytes)) return -1;
	}
	int64_t snap_slot_ints = 0, snap_meta_slot = 0;
	if (two_pass) {
		// shadow H rows; snapshots: (nH + 2 e1 + 2 e2) array-slices x the window at every `step` penalties, windows about as
		// wide as the penalty: ~ NS * s^2 / step ints with s guessed as 3 % of tl+ql (doubled with the arena after an overflow)
		// (systolic layout: a snapshot holds NS array-slices of every owned column of the chunks that take part in its epoch — the window plus
		// 2 x 265 columns and a chunk; the window at snapshot j is about 2 j step wide; s is guessed as 3 % of tl+ql, doubled with the arena after an overflow)
		const int64_t NS = P.nH + 2 * P.e1 + 2 * P.e2, s_guess = len * 3 / 100 + 1024, n_guess = s_guess / opt.step + 2;
		int64_t cols = 0;
		for (int64_t j = 1; j <= n_guess; ++j) cols += std::min<int64_t>(len + 1, 2 * j * opt.step) + 1100;
		snap_meta_slot = (bound1 / opt.step + 256 / opt.step + 4) * 8; // (+ the snapshots of the last epoch's surplus penalties)
		snap_slot_ints = std::min<int64_t>(std::max<int64_t>((int64_t)4 << 20, NS * cols) * g->coop_tb_mult, ((int64_t)48 << 30) / 4) / 4 * 4;
		if (ensure(g, g->sys_sring, NG * (size_t)TC * P.nH * 256 * 4)) return -1;
		if (ensure(g, g->snap, NG * (size_t)snap_slot_ints * 4)) return -1;
		if (ensure(g, g->snap_meta, NG * (size_t)snap_meta_slot * 4)) return -1;
	}
	if (traced) {
		if (ensure(g, g->dbg, (size_t)8 * (bound + 2))) return -1;
		HIP_TRY(g, hipMemsetAsync(g->dbg.p, 0, g->dbg.bytes, g->stream));
	}

	const int64_t sys_rows = std::max(bound, bound1) + 2, sys_log_ints = 2 * (sys_rows + 256 + 8), sys_ep_words = 2 * (sys_rows / 256 + 3);
	const int sys_nef = 2 * P.e1 + 2 * P.e2; // E/F register arrays per column: what a lane publishes and parks besides its H rows
	const int64_t sys_box_group = TC * 2 * std::max(sys_box_ints(sysP, sys_nef, two_pass), sys_box_ints(sysP2, sys_nef, false)), sys_park_group = TC * sys_park_ints(sys_nef, two_pass);
	if (ensure(g, g->sys_ring, NG * (size_t)TC * P.nH * 256 * 4)) return -1;
	if (ensure(g, g->sys_good, NG * (size_t)P.nH * TC * 4 * 8)) return -1;
	if (ensure(g, g->sys_box, NG * (size_t)sys_box_group * 4)) return -1;
	if (ensure(g, g->sys_prog, NG * (size_t)TC * 64)) return -1;
	if (ensure(g, g->sys_log, NG * (size_t)sys_log_ints * 4)) return -1;
	if (ensure(g, g->sys_ep, NG * (size_t)sys_ep_words * 8)) return -1;
	if (ensure(g, g->sys_park, NG * (size_t)sys_park_group * 4)) return -1;
	BatchArgs a;
	memset(&a, 0, sizeof(a));
	ws.rows_slot = rows_slot, ws.cig_scratch_slot = cig_scratch, ws.tb_slot_bytes = tb_bytes;
	fill_args(a, g, b, opt, P, cigar, ws, b->alpha_active);
	a.n_pairs = b->n;
	a.step = low_mem ? opt.step : 0;
	a.seg = low_mem ? (int32_t*)g->seg.p : nullptr, a.seg_slot = seg_slot;
	a.sring = two_pass ? (int32_t*)g->sys_sring.p : nullptr; // (provenance of the systolic kernel's private H rings: the same shape, set_cols())
	a.snap = two_pass ? (int32_t*)g->snap.p : nullptr, a.snap_slot_ints = snap_slot_ints;
	a.snap_meta = two_pass ? (int32_t*)g->snap_meta.p : nullptr, a.snap_meta_slot = snap_meta_slot;
	a.dbg = traced && n_groups == 1 ? (int32_t*)g->dbg.p : nullptr; // the band trace is a single-pair diagnostic
	a.dbg_cap = a.dbg ? (int32_t)(g->dbg.bytes / 8) : 0;
	a.coop_pair = pairs[0];
	a.coop_spin_limit = (uint32_t)g->coop_spin_limit;
	a.coop_groups = n_groups, a.coop_group_size = Gs;
	// (the granule fields of BatchArgs — the edge array, its stride, the provenance offset — belonged to the removed per-penalty hand-off kernel and no device code reads them:
	// they stay zero from the memset, and leave BatchArgs with the next change that touches the kernels — mwf_internal.h is part of every kernel's fingerprint)
	a.coop_flags = (int32_t*)g->coop_misc.p, a.coop_misc_stride = (int64_t)misc_bytes;
	a.coop_sync = (unsigned int*)((char*)g->coop_misc.p + 1024);
	a.coop_state = (int32_t*)((char*)g->coop_misc.p + 2048);
	int32_t *d_ids = (int32_t*)((char*)g->coop_misc.p + NG * misc_bytes);
	HIP_TRY(g, hipMemcpyAsync(d_ids, pairs.data(), NG * 4, hipMemcpyHostToDevice, g->stream));
	a.coop_pair_ids = d_ids;

	// the same launch on the systolic kernel: a private H ring per chunk slot, its own good-bit rows, hand-off boxes, edge log
	BatchArgs as = a;
	as.ring = (int32_t*)g->sys_ring.p, as.good = (unsigned long long*)g->sys_good.p; // (sized for four columns per lane)
	as.rows_slot = sys_rows;
	as.sys_p = sysP;
	as.sys_coop_launch = 1;
	as.sys_spread = 1; // consecutive chunks on consecutive workgroups: 763 against 787 ms on the 5 Mb pair, 63.5 against 65.0 on the 150 kb pair
	as.sys_box = (int32_t*)g->sys_box.p, as.sys_box_stride = sys_box_group;
	as.sys_prog = (unsigned long long*)g->sys_prog.p, as.sys_prog_stride = TC * 8;
	as.sys_log = (int32_t*)g->sys_log.p, as.sys_log_stride = sys_log_ints;
	as.sys_ep = cigar ? (int64_t*)g->sys_ep.p : nullptr, as.sys_ep_stride = sys_ep_words;
	as.sys_park = (int32_t*)g->sys_park.p, as.sys_park_stride = sys_park_group;
	auto reset_sys = [&](bool all) -> int { // counters at zero, nothing published
		for (size_t q = 0; q < NG; ++q) {
			char *m = (char*)g->coop_misc.p + q * misc_bytes;
			if (all) { HIP_TRY(g, hipMemsetAsync(m, 0, 4096, g->stream)); }
			else HIP_TRY(g, hipMemsetAsync(m + 1024, 0, 1024, g->stream));
		}
		HIP_TRY(g, hipMemsetAsync(g->sys_prog.p, 0, NG * (size_t)TC * 64, g->stream));
		return 0;
	};
	std::unique_lock<std::shared_mutex> lock(g_dev_gate[g->device % kMaxDevices]);
	HIP_TRY(g, hipDeviceSynchronize()); // kernels of other engines (other host threads) on this device: let them drain first
	if (reset_sys(true)) return -1;
	if (first) HIP_TRY(g, hipEventRecord(g->ev0, g->stream));
	auto set_cols = [&](int c) { as.sys_c = c, as.ring_slot_ints = TC * P.nH * 64 * c, as.GW = (int32_t)(TC * c); };
	set_cols(c_first);
	a.coop_pass = as.coop_pass = two_pass ? 3 : low_mem ? 1 : 0;
	g->stats.lowmem_two_pass = two_pass ? 1 : 0;
	if (const int rc = launch_sys_pass(as, Gs * n_groups, g->stream)) { g->err = rc == kSysNotResident ? "whole-device kernel cannot be made resident" : "kernel launch failed (whole-device pass)"; return -1; }
	g->stats.n_launches += 1;
	if (low_mem) {
		if (two_pass ? launch_sys_trace(as, g->stream) : launch_sys_walk(as, g->stream)) { g->err = "kernel launch failed (checkpoints)"; return -1; }
		if (reset_sys(false)) return -1; // barrier counters and progress words of the second pass
		a.coop_pass = as.coop_pass = 2;
		as.sys_p = sysP2;
		set_cols(c_second);
		// the second pass is not traced: the band trace of a low-memory run is that of its second pass, traced below
		if (const int rc = launch_sys_pass(as, Gs * n_groups, g->stream)) { g->err = rc == kSysNotResident ? "whole-device kernel cannot be made resident" : "kernel launch failed (second pass)"; return -1; }
		g->stats.n_launches += 2;
	}
	if (launch_sys_finish(as, g->stream)) { g->err = "kernel launch failed (traceback)"; return -1; }
	g->stats.n_launches += 1;
	if (last) {
		HIP_TRY(g, hipEventRecord(g->ev1, g->stream));
		g->ev_pending = true;
	}
	g->stats.grid = Gs * n_groups, g->stats.block = 512, g->stats.kernel_kind = 1;
	b->last_grid = std::max(b->last_grid, Gs * n_groups);
	for (int32_t pair : pairs) b->h_kind[pair] = 1, b->h_flags[pair] = (int8_t)((b->h_flags[pair] & ~(FLAG_COOP_SHARED | FLAG_COOP_NARROW)) | (n_groups > 1 ? FLAG_COOP_SHARED : 0) | ((c_first == 1 || (low_mem && c_second == 1)) ? FLAG_COOP_NARROW : 0));
	HIP_TRY(g, hipStreamSynchronize(g->stream)); // the device stays ours until the kernels are through
	return 0;
}

// one pair with the device to itself
int run_coop_pair(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t &opt, int32_t pair, bool first, bool last)
{
	const int G = coop_group_size(coop_grid_limit(g), (int64_t)b->h_tl[pair] + b->h_ql[pair], true, sys_owned_cols(g->sys_p, 4));
	return run_coop_group(g, b, opt, std::vector<int32_t>{pair}, G, first, last);
}

// can the whole-device traceback arena still grow? (free memory beyond what it already holds)
bool coop_can_grow(mwf_gpu_t *g)
{
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
	return (int64_t)(fr / 10 * 9) > (int64_t)g->tb.bytes / 2; // room for at least half as much again
}

// ---- one align call, step by step ------------------------------------------------------------------------------------------

// Where the result arrays lie.  A small score-only batch (the single pair of a drop-in call) gets them in a page of pinned host
// memory that the kernels write directly: results() then waits for the stream and reads them — no copy to enqueue and wait
// for (a 200 bp call: ~8 us).  The CIGAR counter is device-side atomics: CIGAR-mode batches keep everything in the block.
static int place_results(mwf_gpu_t *g, mwf_gpu_batch_t *b, bool cigar)
{
	const BlockLayout L = layout_block((size_t)b->n, 0, false); // (only differences between result offsets are used)
	bool pin = g->res_pin_on && !cigar && b->n <= 64 && L.out_end - L.head <= 4096 && (g->res_pin_owner == nullptr || g->res_pin_owner == b);
	if (pin && !g->res_pin && hipHostMalloc(&g->res_pin, 4096, hipHostMallocDefault) != hipSuccess) (void)hipGetLastError(), g->res_pin = nullptr, pin = false;
	if (pin != b->out_in_pin || (pin && g->res_pin_owner != b)) {
		if (b->busy) HIP_TRY(g, hipStreamSynchronize(g->stream)); // an align nobody waited for still writes the old arrays
		char *base = pin ? (char*)g->res_pin - L.head : (char*)b->block.p + (b->out_off - L.head);
		b->d_status = (int32_t*)(base + L.status), b->d_s = (int32_t*)(base + L.s), b->d_ncig = (int32_t*)(base + L.ncig);
		b->d_iter = (int64_t*)(base + L.iter), b->d_cigoff = (int64_t*)(base + L.cigoff), b->d_cells1 = (int64_t*)(base + L.cells1);
		if (g->res_pin_owner == b && !pin) g->res_pin_owner = nullptr;
		if (pin) g->res_pin_owner = b;
		b->out_in_pin = pin;
	}
	if (cigar && !b->d_cig_pool) {
		if (take_block(g, g->spare_cig, b->cig, (size_t)b->cig_pool_words * 4)) return -1;
		b->d_cig_pool = (uint32_t*)b->cig.p;
	}
	return 0;
}

// The plan of the last align applies when nothing it was derived from changed: the options that classify pairs and the tunables.  Leaves the batch's
// longest pair and largest penalty bound in the cache either way.
static void revalidate_plan(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t &opt, const Penalty &P0)
{
	mwf_gpu_batch_t::PlanCache &PC = b->plan;
	const int32_t ok[8] = {opt.flag & MWF_F_CIGAR, opt.x, opt.o1, opt.e1, opt.o2, opt.e2, opt.step, opt.max_s};
	// the tunables as a generation count (every mwf_gpu_set() bumps it) + the engine the plan was made on + the traced pair
	const int64_t tk[3] = {g->tun_gen, (int64_t)(intptr_t)g, b->debug_pair};
	if (PC.valid && (memcmp(ok, PC.opt_key, sizeof(ok)) || memcmp(tk, PC.tun_key, sizeof(tk)))) PC.valid = false;
	if (!PC.valid) memcpy(PC.opt_key, ok, sizeof(ok)), memcpy(PC.tun_key, tk, sizeof(tk)), PC.has_groups = false, PC.wide_state = 0;
	if (PC.valid) return;
	int64_t max_len = 0, max_bound = 0;
	for (int32_t i = 0; i < b->n; ++i) {
		max_len = std::max<int64_t>(max_len, (int64_t)b->h_tl[i] + b->h_ql[i]);
		max_bound = std::max(max_bound, penalty_bound(P0, opt.max_s, b->h_tl[i], b->h_ql[i], true));
	}
	PC.max_len = max_len, PC.max_bound = max_bound, PC.valid = true;
}

// Every pair "not run", CIGAR pool and work counters at zero: one small kernel — unless the result arrays can be written from here
// (the pinned result page of a small score-only batch: the single pair of a drop-in call) or came up initialised with the batch
// (a small batch's first align); the kernels of such a call then run without a work counter where they can (run_batch_kernel).
// preset: no reset kernel ran.
static int reset_results(mwf_gpu_t *g, mwf_gpu_batch_t *b, bool was_busy, bool &preset)
{
	g->queue_next = 0, g->lane_set_next = 0;
	preset = false;
	if (b->out_in_pin && !was_busy) {
		for (int32_t i = 0; i < b->n; ++i) b->d_status[i] = -1, b->d_s[i] = -2;
		preset = true;
	} else if (b->results_preinit) preset = true;
	b->results_preinit = false;
	g->queue_clean = !preset;
	b->cig_block_left = kCigBlockGrid;
	if (!preset && launch_reset(b->d_status, b->d_s, b->n, b->d_cig_head, (int32_t*)g->queue.p, kQueueInts, g->stream)) { g->err = "kernel launch failed (reset)"; return -1; }
	std::fill(b->h_flags.begin(), b->h_flags.end(), 0);
	return 0;
}

// A few long pairs: each one gets the whole device in turn.  taken: the batch ran here.
static int route_whole_device(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t &opt, const Penalty &P0, int64_t max_len, bool &taken)
{
	taken = false;
	// (round 3: from 20 000 bases of target + query on, a batch of up to sixteen pairs is faster on the whole-device kernel than one
	// workgroup per pair on any other — 1 x 12 kb 4.1 against 6.4 ms, 16 x 25 kb 11.5 / 20.5, 1 x 32 kb 9.6 / 26.1, a single 10 kb pair
	// 3.4 against 5.8 ms on the packed band kernel; profiles/r03/few_long_pairs.txt)
	// (with traceback already from 15 000 on: 1 x 10 kb 5.1 against 7.2 ms on the packed band kernel, 16 x 8 kb 5.2 / 6.2)
	const int64_t coop_len = g->coop_min_len > 0 ? g->coop_min_len : ((opt.flag & MWF_F_CIGAR) ? 15000 : 20000);
	// The whole-device kernel takes time ~ (tl+ql) per round of pairs side by side (each on its own group of workgroups); the generic kernel
	// runs up to 256 (512) pairs at once in time ~ (tl+ql)^2.  Measured at 3 % divergence (profiles/few_long_pairs.py, round 3): 50 kb pairs
	// 22 ms per round of 16 against 60 ms for any number of them on the generic kernel, 100 kb pairs 44 ms per round of 8 against 245 ms,
	// 150 kb pairs 68 ms against 545 ms — the whole-device kernel wins while the batch needs fewer than about 2.7 (tl+ql)/100 000 rounds.
	bool coop = g->force_kind == 1;
	int n_cu_coop = 0;
	if (coop || (g->force_kind < 0 && max_len >= coop_len && coop_supported(P0))) {
		n_cu_coop = coop_grid_limit(g);
		const int coop_side_by_side = n_cu_coop > 0 ? std::max(1, n_cu_coop / coop_group_size(n_cu_coop, max_len, false, sys_owned_cols(g->sys_p, 4))) : 1;
		// (low-memory mode: the alternative is the generic kernel's two-pass form, three times its high-memory time — 17 x 30 kb @ 5 % 186 ms against 50 ms per round of
		// sixteen here, 48 x 100 kb @ 3 % 694 ms against 555 ms in six rounds of eight: at least four rounds, where the rule above allowed one round of 30 kb pairs;
		// profiles/r06/routing_survey_long_before.txt, _after.txt)
		const bool lowmem_call = (opt.flag & MWF_F_CIGAR) && opt.step > 0;
		const int64_t coop_rounds = lowmem_call ? std::max<int64_t>(4, max_len * 32 / 1000000) : std::max<int64_t>(1, max_len * 27 / 1000000);
		int64_t coop_max_pairs = std::max<int64_t>(1, std::min<int64_t>(256, coop_rounds * coop_side_by_side));
		if (max_len < 65536) coop_max_pairs = std::min<int64_t>(coop_max_pairs, lowmem_call ? 48 : 16); // (measured up to sixteen)
		coop = coop || b->n <= coop_max_pairs;
	}
	if (!coop) return 0;
	if (!coop_supported(P0)) { g->err = "whole-device kernel does not support these penalties"; return -2; }
	if (n_cu_coop < 1) { g->err = "whole-device kernel cannot be made resident"; return -1; }
	std::vector<int32_t> idx(b->h_order.begin(), b->h_order.end());
	std::stable_sort(idx.begin(), idx.end(), longer_first(b));
	for (size_t at = 0; at < idx.size();) {
		const int64_t len0 = (int64_t)b->h_tl[idx[at]] + b->h_ql[idx[at]];
		const int Gs = coop_group_size(n_cu_coop, len0, false, sys_owned_cols(g->sys_p, 4));
		const size_t n_side = std::min<size_t>(idx.size() - at, (size_t)std::max(1, n_cu_coop / Gs));
		const bool last = at + n_side == idx.size();
		if (n_side <= 1 || b->debug_pair >= 0) { // alone (also: band traces are single-pair diagnostics)
			if (run_coop_pair(g, b, opt, idx[at], at == 0, at + 1 == idx.size())) return -1;
			at += 1;
			continue;
		}
		if (run_coop_group(g, b, opt, std::vector<int32_t>(idx.begin() + at, idx.begin() + at + n_side), Gs, at == 0, last)) return -1;
		at += n_side;
	}
	taken = true;
	return 0;
}

// what the class rule depends on (mwf_plan_classes.h), from the engine, the batch and the call's options
static ClassRule make_rule(const mwf_gpu_t *g, const mwf_gpu_batch_t *b, const mwf_opt_t &opt, const Penalty &P0)
{
	ClassRule R;
	R.pen = P0, R.max_s = opt.max_s, R.step = opt.step, R.low_mem = (opt.flag & MWF_F_CIGAR) && opt.step > 0;
	R.band2_ok = band2_supported(P0), R.lane_ok = lane_supported(P0), R.mid_ok_pen = mid_supported(P0), R.biased512_ok = band2_biased512_supported(P0), R.nib_ok = band2_nib_supported(P0);
	R.biased512_chunks = band2_biased512_chunks(), R.span_chunks = band2_span_chunks(), R.mid_lds_bytes = mid_lds_bytes;
	R.force_kind = g->force_kind, R.block = g->block, R.band_pack = g->band_pack, R.band_span = g->band_span, R.seq2bit = g->seq2bit, R.wide_slots = g->wide_slots, R.alpha16 = g->alpha16;
	R.lane_max_len = g->lane_max_len, R.mid_cap = g->mid_max_pairs < 0 ? g->n_cu : g->mid_max_pairs;
	R.div_aware = g->div_aware, R.div_est = b->div_est, R.know_acgt = !b->h_acgt.empty() && g->seq2bit != 0, R.alpha_active = b->alpha_active;
	R.finish();
	return R;
}

static int pair_alpha(const mwf_gpu_batch_t *b, int32_t i) { return (size_t)i < b->h_alpha.size() ? b->h_alpha[(size_t)i] : -1; }

struct ClassPlan {
	GroupInfo gi[kNumClasses];
	bool mid_bytes = false;
};

struct PairInfo { int64_t bound, bound1, exp_win; }; // what the rule worked out for a pair besides its class: the maxima of its group are made of these

// the maxima of every class's group (a function of its own: inlined behind the per-pair rule the loop ran at half its speed, profiles/plan_refactor/plan_timing.txt)
#if defined(__GNUC__)
__attribute__((noinline))
#endif
static void group_maxima(const mwf_gpu_batch_t *b, const std::vector<int8_t> &cls, const std::vector<PairInfo> &info, double div_r, ClassPlan &cp)
{
	for (int32_t i = 0; i < b->n; ++i) {
		const int64_t tl = b->h_tl[i], ql = b->h_ql[i], len = tl + ql;
		const int c = cls[(size_t)i];
		const PairInfo &pi = info[(size_t)i];
		// (the mid class: the window its pairs are expected to reach, forced gap included — its launch picks the workgroup size by it)
		const int64_t exp_win = row(c).geom == GEOM_MID ? std::min<int64_t>(len + 1, (int64_t)((double)len * div_r * 0.28) + 2 * std::abs(tl - ql)) : pi.exp_win;
		cp.gi[c].add(tl, ql, pi.bound, pi.bound1, exp_win);
	}
}

// Class of every pair (cls; b->h_class and b->h_flags get fallback and flags) and the maxima of every class's group.
static void classify_and_group(mwf_gpu_t *g, mwf_gpu_batch_t *b, const ClassRule &rule, std::vector<int8_t> &cls, ClassPlan &cp)
{
	// (a copy of its own: the per-pair loop stores bytes — h_class, h_flags, cls —, which may alias anything reached through a reference, and the rule's
	// fields would be read again for every pair; profiles/plan_refactor/plan_timing.txt)
	ClassRule R = rule;
	const bool mid_ok = R.mid_batch && b->n <= R.mid_cap;
	// A batch of reads whose lengths straddle the limit is not split for a few pairs: where most of the pairs up to 10 % beyond the limit lie below it, the rest follow
	// them (2000 x 300 bp with 28 pairs beyond: 0.37 ms as one lane launch, 0.50 with a launch of their own)
	int64_t lane_limit = mid_ok ? std::min(g->lane_max_len, 320) : g->lane_max_len;
	if (R.lane_on && !mid_ok && (R.classes || R.small_only)) {
		int64_t n_lo = 0, n_hi = 0;
		for (int32_t i = 0; i < b->n; ++i) {
			const int64_t w = (int64_t)((double)std::max(b->h_tl[i], b->h_ql[i]) * R.div_lane);
			if (std::abs(b->h_tl[i] - b->h_ql[i]) > 24) continue;
			n_lo += w <= lane_limit, n_hi += w > lane_limit && w <= lane_limit * 11 / 10;
		}
		if (n_hi > 0 && n_lo >= n_hi) lane_limit = lane_limit * 11 / 10;
	}
	R.lane_limit = lane_limit;
	std::vector<PairInfo> info((size_t)b->n);
	std::vector<int8_t> mid_cand;   // large batches: pairs the mid kernel would take if they are few
	int32_t n_cand = 0;
	if (R.mid_batch && !mid_ok) mid_cand.assign((size_t)b->n, 0);
	// (inlined at both of its uses, like the rule itself: as a call through the closure it costs the first align of a 40 000 x 150 bp batch 0.07 ms)
	auto classify = [&](int32_t i, bool allow_mid) __attribute__((always_inline)) {
		const PairPlan pp = classify_pair(R, b->h_tl[i], b->h_ql[i], R.know_acgt ? b->h_acgt[i] != 0 : true, pair_alpha(b, i), allow_mid);
		info[(size_t)i] = PairInfo{pp.bound, pp.bound1, pp.exp_win};
		b->h_class[i] = pp.fallback, b->h_flags[i] = pp.flags;
		if (pp.mid_candidate && !mid_cand.empty() && !mid_cand[(size_t)i]) mid_cand[(size_t)i] = 1, ++n_cand;
		cp.mid_bytes |= pp.mid_bytes;
		cls[(size_t)i] = pp.cls;
	};
	for (int32_t i = 0; i < b->n; ++i) classify(i, mid_ok);
	if (getenv("MWF_DEBUG")) fprintf(stderr, "[libmwf_hip] classes of %d pairs: divergence estimate %.4f (weight %.2f)\n", b->n, (double)b->div_est, R.div_r);
	if (n_cand > 0 && n_cand <= R.mid_cap)
		for (int32_t i = 0; i < b->n; ++i)
			if (mid_cand[(size_t)i]) classify(i, true);
	group_maxima(b, cls, info, R.div_r, cp);
}

// The processing order: groups in run order, longest first inside a group (the persistent workgroups finish together; the classes on the shared
// work counter then by predicted work, below).  b->h_len_order is sorted longest first and that order is stable: one pass over it deals the pairs to their groups.
static int order_pairs(mwf_gpu_t *g, mwf_gpu_batch_t *b, const std::vector<int8_t> &cls, const ClassPlan &cp)
{
	int32_t start[kNumClasses], end[kNumClasses]; // every class's stretch of the order
	std::vector<int32_t> order((size_t)b->n);
	{
		int32_t at = 0;
		for (PairClass c : kRunOrder) start[c] = at, at += cp.gi[c].n, end[c] = at;
	}
	if (b->h_len_order.empty()) {
		b->h_len_order.resize((size_t)b->n);
		std::iota(b->h_len_order.begin(), b->h_len_order.end(), 0);
		std::stable_sort(b->h_len_order.begin(), b->h_len_order.end(), longer_first(b));
	}
	{
		int32_t next[kNumClasses];
		std::copy(start, start + kNumClasses, next);
		for (int32_t i : b->h_len_order) order[(size_t)next[cls[i]]++] = i;
	}
	// The classes on the shared work counter — the 512-thread geometries (wide, its biased, 4-bit and byte-wise copies) and the 1024-thread span
	// geometry (ClassRow::by_work) — are dealt by predicted WORK, largest first: in an equal-length batch "longest first" says nothing about how long a pair takes.
	// 1024 x 10 kb at 5 %: s 2118 ... 2838 (sd 118) on one length; the pairs dealt last finished far apart while CUs idled (the drain).
	// The estimate: s ~ (tl + ql) x d, d from the share of the query's 8-mers found in the target over the WHOLE pair (correlation 0.88 with s;
	// the batch sketch's 1500-base prefix 0.34).  A class that fits on the device at once (no more pairs than workgroups) has nothing to deal.
	auto dealt = [&](PairClass c) { return row(c).by_work && cp.gi[c].n > 2 * g->n_cu; }; // (two workgroups per CU on the 512-thread geometries; the span geometry holds fewer)
	bool reorder = false;
	for (PairClass c : kRunOrder) reorder |= dealt(c);
	if (reorder && g->work_order != 0 && (g->work_order != 2 || (int32_t)b->h_iter.size() == b->n)) {
		const int32_t lo = start[kRunOrder[by_work_first()]], hi = end[kRunOrder[by_work_end() - 1]]; // (kRunOrder keeps them side by side)
		std::vector<double> key((size_t)b->n, 0.0);
		if (g->work_order == 1) {
			// one workgroup per pair reads both sequences from the device (at align: the caller's arrays need only be valid then); the pair ids go up in
			// the order array, which gets the final order below
			if (upload_segments(g, (char*)b->d_order, std::vector<Seg>{Seg{order.data() + lo, (size_t)(hi - lo) * 4}})) return -1;
			b->h_order.clear();
			if (launch_pair_sketch(b->d_seqs, b->alpha_active ? b->d_rt_off : b->d_t_off, b->d_tl, b->alpha_active ? b->d_rq_off : b->d_q_off, b->d_ql, b->d_order, hi - lo, b->d_dbg4, g->stream)) { g->err = "kernel launch failed (pair sketch)"; return -1; }
			std::vector<int32_t> hits((size_t)(hi - lo));
			HIP_TRY(g, hipMemcpyAsync(hits.data(), b->d_dbg4, hits.size() * 4, hipMemcpyDeviceToHost, g->stream)); // (scratch behind the results: written by this align's kernels only with MWF_F_DEBUG)
			HIP_TRY(g, hipStreamSynchronize(g->stream));
			for (int32_t k = lo; k < hi; ++k) {
				const int32_t i = order[(size_t)k], tl = b->h_tl[i], ql = b->h_ql[i];
				key[(size_t)i] = (double)((int64_t)tl + ql) * sketch_divergence(hits[(size_t)(k - lo)], std::max(ql - 7, 0), tl);
			}
		} else if (g->work_order == 2) {
			for (int32_t k = lo; k < hi; ++k) key[(size_t)order[(size_t)k]] = (double)b->h_iter[(size_t)order[(size_t)k]];
		}
		for (PairClass c : kRunOrder) {
			if (!dealt(c)) continue;
			const auto first = order.begin() + start[c], last = order.begin() + end[c];
			if (g->work_order == 3) std::reverse(first, last); // (shortest first: the other bound of the measurement)
			else std::sort(first, last, [&](int32_t x, int32_t y) {
				if (key[(size_t)x] != key[(size_t)y]) return key[(size_t)x] > key[(size_t)y];
				const int64_t lx = (int64_t)b->h_tl[x] + b->h_ql[x], ly = (int64_t)b->h_tl[y] + b->h_ql[y];
				return lx != ly ? lx > ly : x < y;
			});
		}
	}
	if (order != b->h_order) {
		b->h_order.swap(order);
		if (upload_segments(g, (char*)b->d_order, std::vector<Seg>{Seg{b->h_order.data(), b->h_order.size() * 4}})) return -1; // (waits for earlier work on the stream first)
	}
	return 0;
}

// One launch per class that has pairs, in run order; everything a launch asks for comes from the class's row of kClassTable.
static int launch_classes(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t &opt, const ClassRule &R, const ClassPlan &cp, bool preset)
{
	mwf_gpu_batch_t::PlanCache &PC = b->plan;
	int n_groups = 0, done_groups = 0;
	for (const GroupInfo &G : cp.gi) n_groups += G.n > 0;
	mwf_opt_t opt_hi = opt;
	opt_hi.step = 0;
	size_t at = 0;
	for (PairClass c : kRunOrder) {
		const GroupInfo &G = cp.gi[c];
		const ClassRow &T = row(c);
		if (G.n == 0) continue;
		++done_groups;
		// (the lane class of a batch of reads hands its overflows to a follow-up launch on the device, below)
		const bool lane_retry = T.retry_slot >= 0 && g->dev_retry && G.n >= 1024 && !preset && g->force_kind < 0 && g->block == 0 && R.mid_ok_pen && G.max_len <= 1200 &&
		                        G.max_tl + G.max_bound < 32760 && !R.low_mem;
		// (a forced kernel or block keeps the batch in one group: the 4-bit form then only where every pair of it is class 3)
		bool all_nib = !R.classes && c == CLS_GENERIC && g->force_kind != 0;
		for (int32_t i = 0; all_nib && i < b->n; ++i) all_nib = R.nib_pair(pair_alpha(b, i));
		// the 512-thread geometry of three or four slots: four when asked for, or until an align has shown that three hold every pair (then the kernel reports)
		const bool four_slots = T.wide && (g->wide_slots == 4 || (g->wide_slots == 0 && PC.wide_state != 1 && g->queue_clean));
		LaunchReq rq;
		rq.opt = c == CLS_LOWMEM ? opt : opt_hi;
		rq.d_order = b->d_order + at, rq.n_items = G.n, rq.group = G;
		rq.geom = T.geom;
		rq.copy = all_nib ? COPY_NIB : (T.geom == GEOM_MID && cp.mid_bytes) ? COPY_BYTES : T.copy;
		rq.want_kind = (R.classes || T.geom == GEOM_LANE || T.geom == GEOM_MID) ? T.want_kind : -1; // (without classes only the lane and mid kernels' groups name their kernel)
		rq.window_hint = four_slots ? kBandWide4Window : (T.geom == GEOM_BIASED || T.geom == GEOM_MID) ? G.max_exp_win : 0;
		rq.report_wide = four_slots;
		rq.retry_list = lane_retry ? 1 : 0, rq.retry_slot = lane_retry ? T.retry_slot : 0;
		rq.timed_begin = done_groups == 1, rq.timed_end = !lane_retry && done_groups == n_groups;
		int ran = 0;
		const int rc = run_batch_kernel(g, b, rq, &ran);
		if (T.wide && g->wide_slots == 0 && PC.wide_state == 0 && g->queue_clean && ran == 2 && g->stats.block == 512) PC.wide_measured = true;
		// Batches of reads: what the lane kernel hands back (a window that left its chunks: one read in tens of thousands) is re-run by a follow-up launch of
		// the mid kernel, whose span holds the widest window such a pair can have — from a list the lane kernel filled ON THE DEVICE.  Round 4 read the status
		// words back, launched, waited and read them again: ~0.2 ms behind a 0.5 ms launch.  (An empty list costs the launch of a few idle workgroups.)
		if (rc == 0 && lane_retry) {
			const mwf_gpu_stats_t keep = g->stats;
			// (every entry of the list — the mid kernel strides over it by its grid —, on at most 32 workgroups: an empty list costs the launch of a few idle ones)
			LaunchReq r2;
			r2.opt = opt_hi, r2.d_order = b->d_retry_ids + T.retry_slot * kRetryCap, r2.n_items = kRetryCap, r2.slots = 32, r2.group = G;
			r2.geom = GEOM_MID, r2.copy = T.copy, r2.want_kind = 2, r2.retry_list = 2, r2.retry_slot = T.retry_slot, r2.timed_end = done_groups == n_groups;
			int ran2 = 0;
			const int rc2 = run_batch_kernel(g, b, r2, &ran2);
			const int32_t launches = g->stats.n_launches;
			g->stats = keep, g->stats.n_launches = launches; // (the statistics describe the class's own launch)
			if (rc2) return -1;
			b->dev_retry_used = true;
		}
		if (rc) return -1;
		const bool three_slots = T.wide && ran == 2 && g->stats.block == 512 && !four_slots;
		for (size_t j = at; j < at + (size_t)G.n; ++j) {
			const int32_t i = b->h_order[j];
			b->h_kind[i] = (int8_t)ran, b->h_flags[i] = (int8_t)((b->h_flags[i] & ~FLAG_THREE_SLOTS) | (three_slots ? FLAG_THREE_SLOTS : 0));
		}
		at += (size_t)G.n;
	}
	return 0;
}

// what every align call resets: the batch's record of its last align and what was derived from that align's CIGARs, the engine's statistics
static void begin_align(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t &opt, bool ends_free)
{
	b->opt = opt, b->ends_last = ends_free, b->ext_last = false; // (mwf_gpu_batch_align_ext sets ext_last after this)
	b->pp_ends_last = b->band_last = false;                      // (... and the per-pair calls these: no other align reads the arrays)
	b->aligned = false, b->finalized = false, b->h_cig_valid = false;
	b->summary_valid = false, b->map_valid[0] = b->map_valid[1] = false, std::fill(b->text_valid, b->text_valid + MWF_TXT_KINDS, false); // (summaries, maps and text describe the previous align's CIGARs)
	b->last_grid = 0, b->n_retries = 0, b->dev_retry_used = false;
	g->stats = mwf_gpu_stats_t{};
	if (ends_free) g->stats.kernel_kind = 3;
}

} // namespace host
} // namespace mwf

extern "C" {

int mwf_gpu_batch_align(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt)
{
	if (!g || !b || !opt) return -1;
	if (const char *why = validate(*opt)) { g->err = why; return -2; }
	(void)hipSetDevice(g->device);
	begin_align(g, b, *opt, false);
	if (b->n == 0) { b->aligned = b->finalized = true, b->alpha_known = g->alpha_remap != 0; return 0; } // (an empty batch: nothing to classify or copy, and with "alpha_remap" 1 its zero classes are known)
	if (alpha_prepare(g, b)) return -1; // ("alpha_remap": classes and copies first — the plan below follows them)
	if (place_results(g, b, (opt->flag & MWF_F_CIGAR) != 0)) return -1;
	const Penalty P0 = make_penalty(*opt);
	mwf_gpu_batch_t::PlanCache &PC = b->plan;
	revalidate_plan(g, b, *opt, P0);
	if (PC.max_len + 4 >= ((int64_t)1 << 31)) { g->err = "tl+ql must be below 2^31-4"; return -2; }
	if (b->debug_pair >= 0 && ensure(g, g->dbg, (size_t)8 * (PC.max_bound + 2))) return -1;
	const bool was_busy = b->busy;
	b->busy = true;
	PC.wide_measured = false;
	bool preset = false, whole_device = false;
	if (reset_results(g, b, was_busy, preset)) return -1;
	if (const int rc = route_whole_device(g, b, *opt, P0, PC.max_len, whole_device)) return rc;
	if (!whole_device) {
		ClassRule R = make_rule(g, b, *opt, P0);
		ClassPlan cp;
		if (PC.has_groups) { // same lengths, same options, same tunables as last time: classes, order (already on the device) and maxima as they were
			b->h_class = PC.cls0, b->h_flags = PC.flags0;
			std::copy(PC.gi, PC.gi + kNumClasses, cp.gi);
			cp.mid_bytes = PC.mid_bytes;
		} else {
			std::vector<int8_t> cls((size_t)b->n); // class of every pair
			classify_and_group(g, b, R, cls, cp);
			if (order_pairs(g, b, cls, cp)) return -1;
			PC.cls0 = b->h_class, PC.flags0 = b->h_flags, PC.mid_bytes = cp.mid_bytes, PC.has_groups = true;
			std::copy(cp.gi, cp.gi + kNumClasses, PC.gi);
		}
		if (launch_classes(g, b, *opt, R, cp, preset)) return -1;
	}
	b->aligned = true;
	return 0;
}

// Ends-free alignment (include/miniwfa.h, mwf_ends_t): one launch of mwf_ends.hip's kernel over all pairs, longest first.  No size classes, no whole-device
// route, no sequence copies; the plan cache of the plain align is left alone, so that a later mwf_gpu_batch_align finds what its last one left.
// ... and extension alignment (mwf_ext_t) with it: the same launch under the EXT form of the kernel, `ext` non-null.
// pp_ends: the n pairs' own allowances (`ends` is then its first entry), band: their bands; either may be null.
static int align_ends_or_ext(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ends_t *ends, const mwf_ext_t *ext, const mwf_ends_t *pp_ends = nullptr,
                             const mwf_band_t *band = nullptr)
{
	if (const char *why = validate(*opt)) { g->err = why; return -2; }
	if (pp_ends)
		for (int32_t i = 0; i < b->n; ++i)
			if (pp_ends[i].t_beg < 0 || pp_ends[i].t_end < 0 || pp_ends[i].q_beg < 0 || pp_ends[i].q_end < 0) {
				g->err = "ends-free alignment: every allowance (t_beg, t_end, q_beg, q_end) must be >= 0: pair " + std::to_string(i);
				return -2;
			}
	if (ext) {
		if (ext->match < 1) { g->err = "extension alignment: match must be >= 1"; return -2; }
		if (ext->zdrop < -1) { g->err = "extension alignment: zdrop must be >= 0, or -1 for no drop rule"; return -2; }
		for (int32_t i = 0; i < b->n; ++i) {
			const int64_t len2 = (int64_t)b->h_tl[i] + b->h_ql[i] + 2;
			if (len2 >= ((int64_t)1 << 30)) { g->err = "extension alignment: tl+ql+2 must be below 2^30"; return -2; }
			if (ext->match * len2 >= ((int64_t)1 << 31)) { g->err = "extension alignment: match * (tl+ql+2) must be below 2^31"; return -2; }
		}
	}
	if (ends->t_beg < 0 || ends->t_end < 0 || ends->q_beg < 0 || ends->q_end < 0) { g->err = "ends-free alignment: every allowance (t_beg, t_end, q_beg, q_end) must be >= 0"; return -2; }
	if ((opt->flag & MWF_F_CIGAR) && opt->step > 0) { g->err = "ends-free alignment has no low-memory mode: MWF_F_CIGAR needs opt.step == 0"; return -2; }
	const Penalty P0 = make_penalty(*opt);
	if (P0.nH > kMaxRing) { g->err = "ends-free alignment: max(x, o1+e1, o2+e2) must be < 256"; return -2; }
	(void)hipSetDevice(g->device);
	int64_t longest = 0;
	for (int32_t i = 0; i < b->n; ++i) longest = std::max<int64_t>(longest, (int64_t)b->h_tl[i] + b->h_ql[i]);
	if (longest + 4 >= ((int64_t)1 << 31)) { g->err = "tl+ql must be below 2^31-4"; return -2; }
	begin_align(g, b, *opt, true);
	b->ends = *ends;
	if (ext) b->ext_last = true, b->ext = *ext;
	if (b->n == 0) { b->aligned = b->finalized = true; return 0; }
	const size_t N = (size_t)b->n;
	b->pp_ends_last = pp_ends != nullptr, b->band_last = band != nullptr;
	if (band) b->h_band.assign(band, band + N);
	LaunchReq rq; // every pair, longest first, on as many workgroups as stay resident
	for (int32_t i = 0; i < b->n; ++i) ends_group_add(b, rq.group, i, P0, opt->max_s);
	if (!b->ends_buf.p) { // [range | info | sub_t_off | sub_q_off | sub_tl | sub_ql | order | pp_ends | pp_band]
		const size_t r_bytes = align_up(N * 16, 16), o_bytes = N * 8, l_bytes = align_up(N * 4, 16);
		if (ensure(g, b->ends_buf, 3 * r_bytes + 3 * o_bytes + 3 * l_bytes)) return -1;
		char *base = (char*)b->ends_buf.p;
		b->d_range = (int32_t*)base, base += r_bytes;
		b->d_ext_info = (int32_t*)base, base += r_bytes;
		b->d_sub_t_off = (int64_t*)base, base += o_bytes;
		b->d_sub_q_off = (int64_t*)base, base += o_bytes;
		b->d_sub_tl = (int32_t*)base, base += l_bytes;
		b->d_sub_ql = (int32_t*)base, base += l_bytes;
		b->d_ends_order = (int32_t*)base, base += l_bytes;
		b->d_pp_ends = (int32_t*)base, base += r_bytes;
		b->d_pp_band = (int32_t*)base;
		if (upload_segments(g, (char*)b->d_ends_order, std::vector<Seg>{Seg{b->h_len_order.data(), N * 4}})) { release(g, b->ends_buf); return -1; }
	}
	// (stream order: a kernel of the batch's previous align that still reads the arrays is through before the copies land)
	if (pp_ends && upload_segments(g, (char*)b->d_pp_ends, std::vector<Seg>{Seg{pp_ends, N * sizeof(mwf_ends_t)}})) return -1;
	if (band && upload_segments(g, (char*)b->d_pp_band, std::vector<Seg>{Seg{band, N * sizeof(mwf_band_t)}})) return -1;
	if (place_results(g, b, (opt->flag & MWF_F_CIGAR) != 0)) return -1;
	const bool was_busy = b->busy;
	b->busy = true;
	bool preset = false;
	if (reset_results(g, b, was_busy, preset)) return -1;
	rq.opt = *opt, rq.d_order = b->d_ends_order, rq.n_items = b->n, rq.timed_begin = rq.timed_end = true;
	if (run_ends_kernel(g, b, rq, nullptr)) return -1;
	std::fill(b->h_kind.begin(), b->h_kind.end(), (int8_t)3);
	b->aligned = true;
	return 0;
}

int mwf_gpu_batch_align_ends(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ends_t *ends)
{
	if (!g || !b || !opt || !ends) return -1;
	return align_ends_or_ext(g, b, opt, ends, nullptr);
}

// Extension alignment (include/miniwfa.h, mwf_ext_t): the ends-free launch with the allowances of an extension from an anchor, under the score rule.
int mwf_gpu_batch_align_ext(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ext_t *ext)
{
	if (!g || !b || !opt || !ext) return -1;
	const mwf_ends_t ends = {0, INT32_MAX, 0, INT32_MAX};
	return align_ends_or_ext(g, b, opt, &ends, ext);
}

// Ends-free alignment with the pairs' own allowances and bands (include/miniwfa.h, mwf_band_t): the same launch; the kernel reads the arrays per pair.
int mwf_gpu_batch_align_ends_pp(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ends_t *ends, int32_t n_ends, const mwf_band_t *band)
{
	if (!g || !b || !opt) return -1;
	if (!ends) { g->err = "ends-free alignment: ends must not be NULL"; return -2; }
	if (n_ends != 1 && n_ends != b->n) { g->err = "ends-free alignment: n_ends must be 1 or the batch's number of pairs"; return -2; }
	return align_ends_or_ext(g, b, opt, ends, nullptr, n_ends == 1 ? nullptr : ends, band);
}

// ... and extension alignment under the pairs' bands
int mwf_gpu_batch_align_ext_band(mwf_gpu_t *g, mwf_gpu_batch_t *b, const mwf_opt_t *opt, const mwf_ext_t *ext, const mwf_band_t *band)
{
	if (!g || !b || !opt || !ext) return -1;
	if (!band) { g->err = "extension alignment: band must not be NULL"; return -2; }
	const mwf_ends_t ends = {0, INT32_MAX, 0, INT32_MAX};
	return align_ends_or_ext(g, b, opt, &ends, ext, nullptr, band);
}

} // extern "C"

namespace mwf {
namespace host {

// ---- after the launches: results, and the re-runs of what did not fit where it ran (the rule and the routes: mwf_plan_retry.h) --------------------------

// The fixed-size results, once the batch's kernels are through: into b->host_out and from there into h_status, h_s, h_ncig, h_iter, h_cigoff, h_cells1.
static int fetch_results(mwf_gpu_t *g, mwf_gpu_batch_t *b)
{
	const size_t n = (size_t)b->n;
	std::vector<char> &host = b->host_out;
	const BlockLayout L = layout_block(n, 0, false); // (only differences between result offsets are used)
	// a score-only, high-memory align: n_cigar, CIGAR offsets and first-pass cells are zero by construction — only head, status, s and
	// n_iter come back (16 of the 36 bytes per pair)
	const bool lean = !(b->opt.flag & MWF_F_CIGAR);
	const size_t need = lean ? b->out_bytes_score : b->out_bytes;
	if (n == 0) { HIP_TRY(g, hipStreamSynchronize(g->stream)); return 0; }
	b->h_cig_valid = false;
	if (b->out_in_pin) { // the kernels wrote the engine's pinned result page (score-only: no CIGAR words)
		HIP_TRY(g, hipStreamSynchronize(g->stream));
		memcpy(host.data(), g->res_pin, b->out_bytes);
		memset(host.data(), 0, 8);
	} else if (lean) {
		if (download(g, host.data(), (const char*)b->block.p + b->out_off, need)) return -1;
		memset(host.data() + need, 0, b->out_bytes - need);
	} else {
		// a small CIGAR-mode batch (the single pair of a drop-in call): the head of its CIGAR pool comes back with the results, one wait
		// for both copies — when the pool's used part turns out to fit it, fetch_cigars() has nothing left to copy
		const size_t spec = (b->opt.flag & MWF_F_CIGAR) && b->d_cig_pool && n <= 64 ? (size_t)std::min<int64_t>(b->cig_pool_words, 1024) : 0;
		const size_t cig_at = align_up(b->out_bytes, 64);
		if (spec > 0 && pin_reserve(g, cig_at + spec * 4) == 0) {
			HIP_TRY(g, hipMemcpyAsync(g->pin, (const char*)b->block.p + b->out_off, b->out_bytes, hipMemcpyDeviceToHost, g->stream));
			HIP_TRY(g, hipMemcpyAsync((char*)g->pin + cig_at, b->d_cig_pool, spec * 4, hipMemcpyDeviceToHost, g->stream));
			HIP_TRY(g, hipStreamSynchronize(g->stream));
			g->pin_busy[0] = g->pin_busy[1] = false;
			memcpy(host.data(), g->pin, b->out_bytes);
			unsigned long long used = 0;
			memcpy(&used, host.data(), 8);
			if (used <= spec) {
				b->h_cig.assign((const uint32_t*)((const char*)g->pin + cig_at), (const uint32_t*)((const char*)g->pin + cig_at) + used);
				b->h_cig_valid = true; // (a re-run fetches again and decides again)
			}
		} else if (download(g, host.data(), (const char*)b->block.p + b->out_off, b->out_bytes)) return -1;
	}
	const char *o = host.data() - L.head;
	memcpy(&b->cig_used, o + L.head, 8);
	b->cig_used = std::min<int64_t>(b->cig_used, b->cig_pool_words); // (the head advances in whole blocks: its last step may point past the pool)
	memcpy(b->h_status.data(), o + L.status, n * 4), memcpy(b->h_s.data(), o + L.s, n * 4), memcpy(b->h_ncig.data(), o + L.ncig, n * 4);
	memcpy(b->h_iter.data(), o + L.iter, n * 8), memcpy(b->h_cigoff.data(), o + L.cigoff, n * 8), memcpy(b->h_cells1.data(), o + L.cells1, n * 8);
	return 0;
}

// pairs a follow-up launch re-ran from the device-side list count as re-runs too (the third word of the head: BatchArgs::retry_count)
static void count_device_retries(mwf_gpu_batch_t *b)
{
	if (!b->dev_retry_used) return;
	for (int slot = 0; slot < kRetrySlots; ++slot) { // (what a list could not hold stayed ST_BAND_OVERFLOW and is counted by the host path)
		uint32_t k = 0;
		memcpy(&k, b->host_out.data() + 16 + 8 * slot, 4);
		b->n_retries += (int32_t)std::min<uint32_t>(k, (uint32_t)kRetryCap);
	}
}

// the four-slot kernels' report (reset to 0 by the align's reset kernel): did any pair need more than three slots hold?
static void note_wide_slots(mwf_gpu_batch_t *b)
{
	if (!b->plan.wide_measured) return;
	uint32_t aux = 0;
	memcpy(&aux, b->host_out.data() + 8, 4);
	if (b->plan.wide_state == 0) b->plan.wide_state = (aux & 1u) ? 2 : 1;
	b->plan.wide_measured = false;
}

static bool low_mem_call(const mwf_opt_t &o) { return (o.flag & MWF_F_CIGAR) && o.step > 0; }

// the pair lists of one round of re-runs: [route][step0 index]
struct RetryLists {
	std::vector<int32_t> ids[kNumRoutes][2];
	size_t n = 0;                           // pairs on them
	bool grow_coop = false, fewer = false;  // a pair asked for a larger whole-device arena; a fewer-slots list has pairs
};

// Route every unfinished pair: the rule's decision applied — the pair's new class and flags, the wide class's state, the warnings — and the pair on its list.
// -3 / -4: a pair that no re-run can finish.
static int route_unfinished(mwf_gpu_t *g, mwf_gpu_batch_t *b, const RetryRule &R, int round, bool &coop_warned, RetryLists &L)
{
	static const bool dbg_route = getenv("MWF_DEBUG_REROUTE") != nullptr; // (diagnostics: why a pair is run again)
	const size_t n = (size_t)b->n;
	for (size_t i = 0; i < n; ++i) {
		const int32_t st = b->h_status[i];
		if (st == ST_OK || st == ST_STOPPED) continue;
		const int kind = b->h_kind[i];
		if (dbg_route) fprintf(stderr, "[libmwf_hip] re-route: pair %zu (tl %d ql %d) status %d kind %d class %d flags %d n_iter word %lld round %d\n", i, b->h_tl[i], b->h_ql[i], st, kind, (int)b->h_class[i], (int)b->h_flags[i], (long long)b->h_iter[i], round);
		const RouteDecision d = reroute_pair(R, PairState{b->h_tl[i], b->h_ql[i], st, (int8_t)kind, b->h_class[i], b->h_flags[i], b->h_iter[i]});
		if (d.route == ROUTE_FAIL_STATUS) {
			g->err = "pair " + std::to_string(i) + " failed on the device with status " + std::to_string(st) + (kind == 3 ? " (ends-free)" : "");
			return -3;
		}
		if (is_failure(d.route)) {
			g->err = std::string(d.route == ROUTE_FAIL_TB ? "traceback" : "low-memory snapshots") + " of pair " + std::to_string(i) + " (tl=" + std::to_string(b->h_tl[i]) + ", ql=" + std::to_string(b->h_ql[i]) +
			         ") do not fit in device memory" + (b->opt.step > 0 || kind == 3 ? "" : "; set opt.step > 0 (low-memory mode)");
			return -4;
		}
		if (d.warn == WARN_COOP_GAVE_UP) fprintf(stderr, "[libmwf_hip] warning: whole-device kernel gave up waiting for a workgroup on pair %d; re-running it on one workgroup (slow)\n", (int)i);
		if (d.warn == WARN_COOP_SPAN && !coop_warned) fprintf(stderr, "[libmwf_hip] warning: wavefront of pair %d outgrew the whole-device kernel's span; re-running it on one workgroup (slow)\n", (int)i), coop_warned = true;
		if (d.wide_needs_four) b->plan.wide_state = 2;
		b->h_class[i] = d.h_class, b->h_flags[i] = d.h_flags;
		L.grow_coop |= d.grow_coop, L.fewer |= takes_fewer_slots(d.route), ++L.n;
		L.ids[d.route][d.step0].push_back((int32_t)i);
	}
	return 0;
}

// One list on its route's launch function: longest pair first, the maxima, the ids into g->retry_ids (the previous re-run's kernels are through: every list ends with
// a stream synchronisation), the launch, the wait for it; h_kind gets the kernel that ran.
static int run_list(mwf_gpu_t *g, mwf_gpu_batch_t *b, std::vector<int32_t> &ids, const RouteRow &T, int step0, int slots, Geom geom, CopyForm copy)
{
	if (ids.empty()) return 0;
	int64_t hint = 0;
	if (T.use_forecast) { // every pair of the re-run came back with a forecast: the class that holds the widest of them (+ 25 %)
		for (int32_t i : ids) {
			if (b->h_iter[i] >= 0) { hint = 0; break; }
			hint = std::max<int64_t>(hint, -b->h_iter[i] * 5 / 4 + 64);
		}
		// (every forecast of this re-run is at most kBandWide4Window: the margin must not push the hint past the four-slot geometry, back onto three slots)
		if (hint > kBandWide4Window && T.want_kind == 2 && geom == GEOM_CHOOSE) hint = kBandWide4Window;
	}
	std::stable_sort(ids.begin(), ids.end(), longer_first(b));
	LaunchReq rq;
	rq.opt = b->opt;
	if (step0) rq.opt.step = 0;
	const mwf_opt_t &o = rq.opt;
	if (T.launch == LAUNCH_ENDS) { // (the align's own sizing: under bands the banded bound and the bands' widths)
		const Penalty P = make_penalty(o);
		for (int32_t i : ids) ends_group_add(b, rq.group, i, P, o.max_s);
	} else
	for (int32_t i : ids) rq.group.add(b->h_tl[i], b->h_ql[i], penalty_bound(o, b->h_tl[i], b->h_ql[i], true), penalty_bound(o, b->h_tl[i], b->h_ql[i], false), 0);
	const GroupInfo &G = rq.group;
	DevBuf &tmp = g->retry_ids;
	if (ensure(g, tmp, std::max<size_t>(ids.size() * 4, 4096))) return -1;
	if (upload_segments(g, (char*)tmp.p, std::vector<Seg>{Seg{ids.data(), ids.size() * 4}})) return -1;
	// a handful of short pairs that outgrew the lane kernel (one read in tens of thousands): the mid kernel, whose span holds the widest
	// window such a pair can have at all, takes a fraction of what a lone workgroup of the band classes takes (one 150 bp pair: 0.18 ms
	// of band kernel in every align of the 40 000-pair batch, profiles/r04/rocprof_lane_kernel_40000x150bp.txt)
	const int mid_cap = g->mid_max_pairs < 0 ? g->n_cu : g->mid_max_pairs;
	const bool to_mid = T.want_kind == 2 && T.use_forecast && copy != COPY_NIB && g->force_kind < 0 && g->block == 0 && (int)ids.size() <= mid_cap && mid_supported(make_penalty(o)) && G.max_len <= 1200 &&
	                    G.max_tl + G.max_bound < 32760 && !low_mem_call(o);
	rq.d_order = (const int32_t*)tmp.p, rq.n_items = G.n, rq.slots = slots;
	rq.geom = to_mid ? GEOM_MID : geom, rq.copy = copy, rq.want_kind = T.want_kind, rq.window_hint = hint, rq.ring16_allowed = T.ring16_allowed;
	// (a re-run whose forecast is clamped to the four-slot window asks for the report as the wide class's measuring launch does, as it always has: nothing reads
	// the word after a re-run — finalize() looked at it before, and the next align's reset kernel zeroes it)
	rq.report_wide = rq.geom == GEOM_CHOOSE && hint == kBandWide4Window;
	int ran = 0;
	if (T.launch == LAUNCH_ENDS ? run_ends_kernel(g, b, rq, &ran) : run_batch_kernel(g, b, rq, &ran)) return -1;
	if (hipStreamSynchronize(g->stream) != hipSuccess) return -1;
	for (int32_t i : ids) b->h_kind[i] = (int8_t)ran;
	return 0;
}

// The lists of one round: for each of the two step0 indices, kRouteTable's order (the whole-device and ends-free lists hold their pairs under index 0); every launch
// as its route's row says.
static int run_routes(mwf_gpu_t *g, mwf_gpu_batch_t *b, RetryLists &L, int grid0, int tb_slots)
{
	// (as the plan's nib_pair: the pair's copy holds image bytes and the set has 4-bit kernels — a re-run respects the class)
	const bool nib_on = g->alpha16 != 0 && b->alpha_active && g->seq2bit != 0 && g->band_pack != 0 && g->band_span != 0 && band2_nib_supported(make_penalty(b->opt)) && !low_mem_call(b->opt);
	for (int z = 0; z < 2; ++z)
		for (int r = 0; r < kNumRoutes; ++r) {
			const RouteRow &T = kRouteTable[r];
			std::vector<int32_t> &ids = L.ids[r][z];
			if (ids.empty()) continue;
			if (T.launch == LAUNCH_COOP) {
				for (int32_t i : ids)
					if (run_coop_pair(g, b, b->opt, i, false, false)) return -1;
				continue;
			}
			const int slots = T.slots == SLOTS_GRID0 ? grid0 : T.slots == SLOTS_ALL ? 1 << 30 : std::max(1, std::min<int>(tb_slots, (int)ids.size()));
			const bool all_span = T.span_if_all && std::all_of(ids.begin(), ids.end(), [&](int32_t i) { return b->h_class[i] == CLS_SPAN; });
			const Geom geom = all_span ? GEOM_SPAN : T.geom;
			if (!T.nib_split || (z == 0 && low_mem_call(b->opt))) { // (index 1 runs as high-memory)
				if (run_list(g, b, ids, T, z, slots, geom, T.copy)) return -1;
				continue;
			}
			// a band re-run on sequence copies: the class-3 pairs of the list ("alpha16") apart from the rest, on the 4-bit form of the same geometry
			std::vector<int32_t> nib_ids, rest;
			for (int32_t i : ids) (nib_on && (size_t)i < b->h_alpha.size() && b->h_alpha[(size_t)i] == 3 ? nib_ids : rest).push_back(i);
			if (run_list(g, b, rest, T, z, slots, geom, COPY_2BIT) || run_list(g, b, nib_ids, T, z, slots, geom, COPY_NIB)) return -1;
		}
	return 0;
}

// Wait for the batch; re-run what did not fit where it ran, in at most 16 rounds (a round whose fewer-slots lists have pairs leaves them an eighth of the workgroups).
int finalize(mwf_gpu_t *g, mwf_gpu_batch_t *b)
{
	if (b->finalized) return 0;
	if (!b->aligned) { g->err = "batch was not aligned"; return -1; }
	const size_t n = (size_t)b->n;
	b->h_s.resize(n), b->h_ncig.resize(n), b->h_status.resize(n), b->h_iter.resize(n), b->h_cigoff.resize(n), b->h_cells1.resize(n);
	if (b->host_out.size() < b->out_bytes) b->host_out.resize(b->out_bytes);
	if (fetch_results(g, b)) return -1;
	count_device_retries(b);
	note_wide_slots(b);
	b->busy = false;
	RetryRule R;
	R.band_span = g->band_span, R.seq2bit = g->seq2bit, R.force_kind = g->force_kind, R.block = g->block, R.tb_budget_mb = g->tb_budget_mb;
	R.step = b->opt.step, R.span_window = band_span_window();
	R.coop_can_grow = [](void *ctx) { return coop_can_grow((mwf_gpu_t*)ctx); }, R.ctx = g;
	int tb_slots = std::max(1, b->last_grid);
	const int grid0 = tb_slots;
	bool coop_warned = false;
	for (int round = 0; round < 16; ++round) {
		RetryLists L;
		R.tb_slots = tb_slots, R.coop_tb_mult = g->coop_tb_mult;
		if (const int rc = route_unfinished(g, b, R, round, coop_warned, L)) return rc;
		if (L.n == 0) break;
		b->n_retries += (int32_t)L.n;
		if (L.grow_coop) g->coop_tb_mult *= 2;
		if (L.fewer) tb_slots = std::max(1, tb_slots / 8);
		if (run_routes(g, b, L, grid0, tb_slots)) return -1;
		if (fetch_results(g, b)) return -1;
	}
	// nothing may be handed out as a result that is not one
	for (size_t i = 0; i < n; ++i)
		if (b->h_status[i] != ST_OK && b->h_status[i] != ST_STOPPED) {
			g->err = "pair " + std::to_string(i) + " is still unfinished after every retry (status " + std::to_string(b->h_status[i]) + ")";
			return -3;
		}
	g->stats.cells = 0, g->stats.cells_pass1 = 0, g->stats.n_retries = b->n_retries;
	for (size_t i = 0; i < n; ++i) g->stats.cells += b->h_iter[i], g->stats.cells_pass1 += b->h_cells1[i];
	b->finalized = true;
	return 0;
}

// every CIGAR of the batch in one copy (the used part of the pool)
int fetch_cigars(mwf_gpu_t *g, mwf_gpu_batch_t *b)
{
	if (b->h_cig_valid) return 0;
	if (int rc = finalize(g, b)) return rc;
	if (b->h_cig_valid) return 0; // came back with the results (small batch)
	b->h_cig.resize((size_t)std::max<int64_t>(b->cig_used, 0));
	if (b->cig_used > 0 && download(g, b->h_cig.data(), b->d_cig_pool, (size_t)b->cig_used * 4)) return -1;
	b->h_cig_valid = true;
	return 0;
}

} // namespace host
} // namespace mwf
