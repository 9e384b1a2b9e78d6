// mwf_engine.h — what the three host files of libmwf_hip.so share: the engine and batch objects, the device-memory helpers
// (mwf_memory.cpp), the plan / launch / retry layer (mwf_plan.cpp) and the C ABI (mwf_engine.cpp).  Internal: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <numeric>
#include <string>
#include <chrono>
#include <cmath>
#include <functional>
#include <thread>
#include <tuple>
#include <vector>
#include "miniwfa.h"
#include "kalloc.h"
#include "mwf_internal.h"
#include "mwf_ends.h"
#include "mwf_plan_classes.h"

namespace mwf {
namespace host {


[[noreturn]] inline void fatal(const char *what, const char *detail)
{
	fprintf(stderr, "[libmwf_hip] fatal: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
	abort();
}

// One device buffer that only grows.
struct DevBuf {
	void *p = nullptr;
	size_t bytes = 0;
};

constexpr size_t kPinHalfMax = (size_t)16 << 20; // pinned staging: two halves of at most this many bytes
constexpr int kCigBlock = 256, kCigBlockGrid = 8192, kCigBlockPairs = 4096; // CIGAR pool in block mode (batch_common)
constexpr int kQueueSlots = 64;                  // work counters zeroed at the start of an align call, one per launch
// The lane kernel's launches (tens of thousands of read pairs) take a SET of kLaneCounters work counters, each on a cache line of its own:
// counter c deals the pairs c, c + 64, c + 128 ... of the order to the waves with blockIdx % 64 == c.  (One counter for all: 40 000 atomics on
// one address, ~12.7 ns each — 0.51 of the kernel's 0.61 ms.)  kLaneSets sets per align call, behind the plain counters in the same buffer.
constexpr int kLaneCounters = 64, kLaneStride = 32, kLaneSets = 4, kQueueInts = kQueueSlots + kLaneSets * kLaneCounters * kLaneStride;
constexpr int kMaxDevices = 64;

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What distinguishes two kernel variants for the occupancy query (cached_occupancy, mwf_plan.cpp).  kind 2: the band family, 0: the generic kernel, 3: the ends-free
// kernel (mwf_ends.hip: its block and whether it is the extension form); the fields of the other family stay zero.
struct OccKey {
	int kind = 0, block = 0;
	bool ext = false;
	// band family
	int packed = 0, lane = 0, slots512 = 0, e1 = 0, e2 = 0, lds_bytes = 0; // slots512: span / 2048 of the 512-thread geometry (its chunk slots per wave: 3 ... 6), else 0
	bool cigar = false, seq2 = false, tab = false, nib = false, fold2 = false;
	// generic kernel
	bool stream_pass = false, ring16 = false, big_ring = false;
	int lds_e2_cols = 0;
	auto tied() const { return std::tie(kind, block, ext, packed, lane, slots512, e1, e2, lds_bytes, cigar, seq2, tab, nib, fold2, stream_pass, ring16, big_ring, lds_e2_cols); }
	bool operator<(const OccKey &o) const { return tied() < o.tied(); }
};


} // namespace host
} // namespace mwf

using namespace mwf;
using namespace mwf::host;


struct mwf_gpu_s {
	int device = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	int n_cu = 0;
	size_t total_mem = 0;
	std::string err;
	// tunables
	int block = 0;              // 0: choose from the batch
	bool dev_retry = true;      // batches of reads: the pairs the lane kernel hands back are re-run by a follow-up launch from a device-side list, without the host
	bool band_fold = true;      // packed band kernel: the folded score-only form where the penalties allow it (o1 == x)
	bool probe_table = true;    // packed band kernel: the table form of the first probe (mwf_band2_tab.hip) where it applies and two workgroups still share a CU (0: never)
	bool band_fold2 = true;     // packed band kernel, table form, score-only: the second gap piece folded too (mwf_band2_tab2.hip) where band2_tab2_supported holds (0: never)
	int64_t probe_table_lds = 0; // mwf_gpu_test_hook "probe_table_lds": LDS bytes (table + sequence copies) above which a launch keeps the plain form (0: 74 KB, choose_kernel) — tests of the fall-back
	bool div_aware = true;      // weigh the size classes' length limits by the batch's estimated divergence (batches built from host memory)
	int64_t tun_gen = 0;        // bumped by every successful mwf_gpu_set(): a cached plan of an align (PlanCache) is only replayed under the tunables it was made under
	int64_t coop_min_len = 0;
	int64_t tb_budget_mb = 0;   // 0: automatic
	int force_kind = -1;
	int work_order = 1;         // deal order of the band classes on the shared work counter (mwf_plan.cpp): 0 length, 1 predicted work (per-pair 8-mer sketch),
	                            // 2 the n_iter of the batch's previous align (the bound a prediction can reach), 3 shortest first — mwf_gpu_test_hook "work_order"
	int64_t *timeline = nullptr; // mwf_gpu_test_hook "timeline": device array of [pair][4] int64 that a probe build of the packed band kernel fills (BatchArgs::timeline)
	int res_pin_on = 1;        // small score-only batches: results written straight into pinned host memory (0: always copied back)
	int lane_chunks = 0;       // its window: 64-column chunks of LDS rows (1-4; 0: three for pairs of up to 400 bases of target + query, else four); a penalty only passes over the chunks the window has reached
	int lane_max_len = 325;    // (weighed by the batch's divergence / 5 % where known.  Round 3 set 400 against the band kernel of that round; against round 6's 64-thread geometry the lane kernel
	                           // wins up to ~370 bases at 5 %, ~200 at 10 %, everywhere at 2 %, and loses by half beyond: 2000 x 450 bp @ 5 % 1.46 against 0.77 ms, profiles/r06/lane_crossover.txt)
	                           // pairs whose longer sequence has at most this many bases try the one-diagonal-per-lane kernel first (0: never)
	int mid_max_pairs = -1;    // a batch of at most this many pairs may use the one-workgroup-per-pair, rings-in-LDS kernel (mwf_mid.hip) for its mid-size pairs (-1: one per CU; 0: never)
	int mid_block = 0;         // its threads per workgroup: 0 by span (256 up to 512 columns, else 1024), 256, 1024
	int band_pack = -1;        // int16-packed E/F registers in the band kernel: 0 never, otherwise whenever the value ranges allow
	int wide_slots = 0;        // chunk slots per wave of the 512-thread packed geometry: 0 by batch (four until an align has shown that three hold every pair), 3, 4
	int band_span = 1;         // the 1024-thread geometry of the packed band kernel (80 chunks, biased offsets: pairs of up to ~60 kb whose windows stay below ~20 000 columns): 0 never, 2: every pair it can take (tests)
	int ring16 = 1;            // generic kernel with E2/F2 in LDS: 16-bit ring rows in HBM while target length + penalty fits 16 bits (0: never)
	int seq2bit = 1;           // packed band kernel: 2-bit sequence copy in LDS for pairs of plain A/C/G/T (0: always bytes)
	int alpha_remap = 0;       // 1: pairs of at most four distinct bytes are copied into a per-batch arena with their bytes mapped onto A/C/G/T and planned as plain pairs (alpha_prepare, mwf_memory.cpp); 0: never
	int alpha16 = 0;           // 1 (with alpha_remap 1 only): pairs of 5 to 16 distinct bytes are class 3, copied as 0x40 | code, and take the packed band kernel's 4-bit form under gap extensions (2,1)
	int64_t alpha_arena_budget = -1; // mwf_gpu_test_hook "alpha_arena_budget": bytes an arena may take (-1: four fifths of what is free) — tests of the fall-back
	int lds_e2 = 1;            // generic kernel: keep E2/F2 in LDS where that applies (0: never)
	int scalar_generic = 0;    // 1: the generic kernel's original one-column-per-lane pass everywhere (comparison / fallback)
	int64_t coop_spin_limit = 1 << 23; // polls (about a microsecond each) before the whole-device kernel gives up on a workgroup
	int64_t coop_tb_cap = (int64_t)96 << 30; // whole-device traceback arena: first allocation never above this ...
	int64_t coop_tb_mult = 1;                // ... times this; doubled after an overflow while memory lasts
	int64_t lowmem_budget_mb = 0; // whole-device low-memory mode: first-pass traceback above this many MB -> true two-pass (0: automatic)
	int sys_p = 8;             // whole-device (systolic) kernel: penalties per hand-off block (4, 8 or 16)
	int sys_c = 0;             // its columns per lane: 0 automatic (1 while the window is expected to fit the slots that way, else 4), 1, 4
	// workspace (per-stream pool)
	DevBuf ring, sring, good, tb, row_off, row_lo, cig_scratch, snap, snap_meta, seg, queue, dbg, coop_misc;
	DevBuf retry_ids;          // pair ids of a re-run (finalize): kept by the engine — round 4 allocated and freed one per re-run, a hipMalloc + hipFree of ~0.15 ms behind a 0.5 ms launch
	DevBuf sys_box, sys_prog, sys_log, sys_ep, sys_park, sys_ring, sys_sring, sys_good;
	DevBuf spare_block, spare_cig; // allocations of freed batches, waiting for the next batch
	int queue_next = 0;            // next unused work counter of the current align call
	int lane_set_next = 0;         // ... and next unused set of lane-kernel counters
	bool queue_clean = false;      // the work counters were zeroed by this align call's reset kernel (else a launch that needs one zeroes it itself)
	// pinned staging
	void *pin = nullptr;
	size_t pin_half = 0;
	hipEvent_t pin_ev[2] = {nullptr, nullptr};
	void *res_pin = nullptr;            // 4 KB of pinned host memory the kernels write a small score-only batch's results into (no copy back)
	const void *res_pin_owner = nullptr; // the batch whose result pointers currently lie in it
	bool pin_busy[2] = {false, false}; // a copy out of that half may still be in flight (pin_ev tells)
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	bool ev_pending = false;
	hipEvent_t ev_alpha[4] = {nullptr, nullptr, nullptr, nullptr}; // around the last align's classification launch [0, 1] and copy launch [2, 3] of mwf_alphabet.hip (created on first use)
	bool alpha_timed[2] = {false, false};                           // ... which of them that align made
	mwf_gpu_stats_t stats{};
	int64_t dev_bytes = 0, dev_bytes_peak = 0; // device memory this engine holds right now / held at most since the last "trim"
	std::map<OccKey, int> occ_cache;           // kernel variant -> resident workgroups per CU
	int coop_grid = -1;
	int coop_grid_cap = 0;      // "coop_grid": at most this many workgroups for the whole-device kernel (0: one per CU)
};

struct mwf_gpu_batch_s {
	mwf_gpu_t *g = nullptr;
	int32_t n = 0;
	bool owns_inputs = false;
	DevBuf block;              // the batch's one device allocation: [order | inputs (when owned) | results]
	const uint8_t *d_seqs = nullptr;
	int64_t seq_bytes = 0;
	const int64_t *d_t_off = nullptr, *d_q_off = nullptr;
	const int32_t *d_tl = nullptr, *d_ql = nullptr;
	std::vector<int32_t> h_tl, h_ql;
	int64_t max_seq_lds = 0;   // LDS bytes the band kernel needs to hold the longest pair's sequences
	int64_t max_tl = 0;        // longest target (offsets are target indices: bounds what a 16-bit offset must hold)
	int32_t *d_order = nullptr;
	std::vector<int32_t> h_order;   // what d_order holds: pair ids, grouped by size class, longest first inside a class
	std::vector<int32_t> h_len_order; // pair ids, longest pair first (stable): what every grouping is dealt from
	std::vector<int8_t> h_class;    // where a pair that is handed back starts again, as a PairClass: CLS_GENERIC, one of the four band classes CLS_WIDE ... CLS_MICRO, or CLS_SPAN
	                                // (the plan's PairPlan::fallback — a biased pair carries CLS_WIDE, a lane pair CLS_MICRO; every re-route moves it on: reroute_pair, mwf_plan_retry.h)
	std::vector<int8_t> h_kind;     // kernel that ran the pair last (0 generic, 1 whole-device, 2 band, 3 ends-free)
	float div_est = 0;              // divergence of the batch as a k-mer sketch of a few of its pairs saw it while the batch was built from host memory (0: unknown)
	std::vector<int8_t> h_acgt;     // from the host's look at the bytes while a batch is built from host memory: 1 both sequences are plain
	                                // A/C/G/T, 0 not (such a pair goes to the byte-wise sequence copy at once); empty: unknown (wrapped device
	                                // buffers — the 2-bit copy finds out on the device and the pair comes back as ST_ALPHABET)
	// "alpha_remap" (alpha_prepare, mwf_memory.cpp).  While alpha_active, h_acgt is 1 for the pairs of classes 0 and 1 and the align kernels take their
	// offsets from d_rt_off / d_rq_off: the batch's own for classes 0 and 2, the copy in the arena (as an offset from d_seqs) for class 1.
	std::vector<int8_t> h_acgt_host; // h_acgt as the upload made it (empty: wrapped) — what h_acgt goes back to
	std::vector<int8_t> h_alpha;    // class of every pair (mwf_alphabet_class): from the host twin while an uploaded batch was packed, from the kernel's classification at every align of a wrapped one
	std::vector<uint32_t> h_sym;    // ... and its distinct bytes (AlphabetArgs::sym: kAlphaSymWords words per pair)
	std::vector<int8_t> h_alpha_up; // the classes the upload's host twin found, class 3 included (empty: wrapped); h_alpha is this view under the engine's "alpha16"
	int alpha16_laid_out = -1;      // the "alpha16" the arena was laid out for
	DevBuf alpha_cls;               // device: [sym: n x kAlphaSymWords uint32 | cls: n int8]
	DevBuf alpha_arena;             // device: [t_off: n int64 | q_off: n int64 | dst_t, dst_q: the copy launch's destinations, n int64 each | ids of the class-1 pairs: n int32 | 64 bytes | the copies, each sequence on a 16-byte boundary | 64 bytes]
	const int64_t *d_rt_off = nullptr, *d_rq_off = nullptr;
	bool alpha_known = false;       // h_alpha describes the last align (mwf_gpu_batch_alphabet)
	bool alpha_active = false;      // the last align read the copies
	bool alpha_laid_out = false;    // the arena's offsets (and, uploaded batches, its copies) are in place for h_alpha
	std::vector<int8_t> h_flags;    // FLAG_* (mwf_plan_classes.h): FLAG_STEP0 from the plan; the others say where the pair ran last, for finalize()'s re-routes
	// results: one region of the block, fetched by one copy
	unsigned long long *d_cig_head = nullptr;
	int32_t *d_status = nullptr, *d_s = nullptr, *d_ncig = nullptr, *d_dbg4 = nullptr;
	int64_t *d_iter = nullptr, *d_cigoff = nullptr, *d_cells1 = nullptr;
	size_t out_off = 0, out_bytes = 0;
	bool out_in_pin = false;        // the result arrays lie in the engine's pinned result page (small score-only batches)
	bool results_preinit = false;   // the device result arrays came up initialised with the batch's upload (status -1, s -2, CIGAR counter 0): its first align needs no reset kernel
	DevBuf cig;                     // CIGAR pool (allocated by the first CIGAR-mode align)
	uint32_t *d_cig_pool = nullptr;
	int64_t cig_pool_words = 0;
	int32_t cig_block = 0;          // > 0: the pool is sized for workgroups that take it in blocks of this many words (batches of thousands of pairs)
	// state of the last align
	bool aligned = false, finalized = false, busy = false;
	mwf_opt_t opt{};
	std::vector<int32_t> h_s, h_ncig, h_status;
	std::vector<int64_t> h_iter, h_cigoff, h_cells1;
	int64_t cig_used = 0;           // words of the pool in use (known after finalize)
	int32_t cig_block_left = 0;     // block mode: workgroups (= partly used blocks the pool has slack for) the launches of this align may still spend; reset by every align
	std::vector<uint32_t> h_cig;    // host copy of the used part of the pool (fetch_cigars)
	bool h_cig_valid = false;
	// What the last align worked out from the pair lengths alone — size classes, processing order, per-class maxima — keyed by the
	// options and tunables it depends on: lengths do not change between aligns of a batch, so the next align with the same key skips
	// the per-pair pass (40 000 read pairs: ~2.5 ms of host work per align before, profiles/r04/short_reads.txt)
	struct PlanCache {
		bool valid = false;
		int32_t opt_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		int64_t tun_key[3] = {0, 0, 0}; // the engine's tun_gen, the engine, the traced pair
		int64_t max_len = 0, max_bound = 0;
		bool has_groups = false, mid_bytes = false;
		// The wide class (512-thread geometry) holds 24 chunks with three slots per wave and 32 with four (2 % slower where three suffice).  0: not known yet —
		// four slots, and the kernel reports whether three would have held every pair; 1: three hold this batch under these options; 2: four are needed.
		int8_t wide_state = 0;
		bool wide_measured = false; // this align's first launch of the class ran on four slots with the report word zeroed
		// the maxima over a set of pairs (a class's group, the list of a re-run): what a launch sizes its kernel and workspace by
		struct GI {
			int32_t n = 0;
			int64_t max_len = 0, max_bound = 0, max_bound1 = 0, max_tl = 0, max_seq_lds = 0, max_exp_win = 0; // max_seq_lds: LDS bytes that hold the longest pair's sequences as bytes
			// one more pair: its lengths, its penalty bound with and without max_s, the window it is expected to reach
			// (the last three by reference, as group_maxima's loop has always read them: given values the compiler pairs max_bound and max_bound1 into one 128-bit
			// update whose 64-bit compares it has to emulate, and the first align of a 40 000-pair batch takes 0.1 ms longer; profiles/retry_refactor/plan_timing.txt)
			void add(int64_t tl, int64_t ql, const int64_t &bound, const int64_t &bound1, const int64_t &exp_win)
			{
				++n;
				max_len = std::max(max_len, tl + ql), max_bound = std::max(max_bound, bound), max_bound1 = std::max(max_bound1, bound1);
				max_tl = std::max(max_tl, tl), max_exp_win = std::max(max_exp_win, exp_win);
				max_seq_lds = std::max<int64_t>(max_seq_lds, ((tl + 3) & ~3LL) + 8 + ((ql + 3) & ~3LL) + 16);
			}
		} gi[kNumClasses];
		std::vector<int8_t> cls0, flags0;
	} plan;
	std::vector<char> host_out;     // the fixed-size results as they came back (finalize)
	size_t out_bytes_score = 0;     // leading part of the result region a score-only, high-memory align needs back: head, status, s, n_iter
	// geometry and counters of the last align of THIS batch (finalize() must not read the engine's: another batch may have
	// been aligned on the same engine in between)
	int32_t last_grid = 0, n_retries = 0;
	int32_t *d_retry_ids = nullptr;  // [kRetrySlots][kRetryCap] pairs a launch handed back for its follow-up launch; their count is the third word of the head (d_cig_head + 2)
	bool dev_retry_used = false;     // this align made such a follow-up launch: the count is added to n_retries
	// debug band trace (tests)
	int32_t debug_pair = -1;
	// products of mwf_cigar_ops.hip (summary, coordinate maps): allocated on first use, stale after the next align, freed with the batch
	DevBuf ops_summary, ops_map[2], ops_map_off[2];
	bool summary_valid = false, map_valid[2] = {false, false};
	std::vector<int64_t> h_map_off[2]; // n + 1 offsets into the map (which 0: prefix sums of ql, 1: of tl); empty until first asked for
	bool map_off_uploaded[2] = {false, false}; // ops_map_off[which] holds h_map_off[which] (set only after the upload succeeded)
	// products of mwf_cigar_text.hip: one pool and one offset array (n + 1 int64) per kind, same lifetime
	DevBuf ops_text[MWF_TXT_KINDS], ops_text_off[MWF_TXT_KINDS];
	bool text_valid[MWF_TXT_KINDS] = {false, false, false, false, false, false};
	int64_t text_total[MWF_TXT_KINDS] = {0, 0, 0, 0, 0, 0}; // bytes of text in the pool
	int64_t ops_max_len = -1;          // longest pair (tl + ql): what the workgroup size of those kernels is chosen by (-1: not computed yet)
	// ends-free alignment (mwf_gpu_batch_align_ends; kernel: mwf_ends.hip).  One allocation, made by the first such align and freed with the batch:
	// [range: n x 4 int32 | info: n x 4 int32 | sub_t_off, sub_q_off: n int64 each | sub_tl, sub_ql: n int32 each | order: n int32, longest pair first | the per-pair arrays below]
	bool ends_last = false;            // the batch's last align was ends-free or an extension: h_kind is 3 for every pair, ranges exist, maps do not
	bool ext_last = false;             // ... an extension (mwf_gpu_batch_align_ext): the kernel's EXT form, info exists
	mwf_ends_t ends{};                 // its allowances (finalize()'s re-runs use them)
	mwf_ext_t ext{};                   // ... and, after an extension, its parameters (likewise)
	DevBuf ends_buf;
	int32_t *d_range = nullptr, *d_ext_info = nullptr, *d_sub_tl = nullptr, *d_sub_ql = nullptr, *d_ends_order = nullptr;
	int64_t *d_sub_t_off = nullptr, *d_sub_q_off = nullptr;
	// per-pair allowances and bands (mwf_gpu_batch_align_ends_pp / _ext_band): two more arrays at the end of ends_buf,
	// [pp_ends: n x 4 int32 | pp_band: n x 2 int32], uploaded by those calls.  The flags say whether the batch's last align read them: finalize()'s re-runs
	// repeat them, every other align clears them.
	int32_t *d_pp_ends = nullptr, *d_pp_band = nullptr;
	bool pp_ends_last = false, band_last = false;
	std::vector<mwf_band_t> h_band;    // the bands of that align (band_last): what a launch's penalty bound and widest window are sized by
};


#define HIP_TRY(g, call)                                                              \
	do {                                                                              \
		hipError_t e_ = (call);                                                       \
		if (e_ != hipSuccess) {                                                       \
			(g)->err = std::string(#call) + ": " + hipGetErrorString(e_);             \
			return -1;                                                                \
		}                                                                             \
	} while (0)

namespace mwf {
namespace host {

// ---- mwf_memory.cpp: device buffers that only grow, recycled batch blocks, the pinned staging buffer, batches from host memory
void account(mwf_gpu_t *g, int64_t delta);
int ensure(mwf_gpu_t *g, DevBuf &b, size_t bytes);
void release(mwf_gpu_t *g, DevBuf &b);
int take_block(mwf_gpu_t *g, DevBuf &spare, DevBuf &out, size_t bytes);
void give_block(mwf_gpu_t *g, DevBuf &spare, DevBuf &b);
int pin_reserve(mwf_gpu_t *g, size_t half);
struct Seg { const void *src; size_t len; }; // src == nullptr: `len` zero bytes
int upload_segments(mwf_gpu_t *g, char *dst, const std::vector<Seg> &segs);
int download(mwf_gpu_t *g, void *dst, const void *src, size_t bytes);
struct BlockLayout {
	size_t order = 0, t_off = 0, q_off = 0, tl = 0, ql = 0, seqs = 0, in_end = 0;
	size_t head = 0, status = 0, s = 0, ncig = 0, iter = 0, cigoff = 0, cells1 = 0, score_end = 0, out_end = 0, dbg4 = 0, retry = 0, total = 0;
};
constexpr int kRetryCap = 256; // ids a launch can hand to its follow-up launch on the device (BatchArgs::retry_ids)
constexpr int kRetrySlots = 2; // lists (and counters: words 2 and 3 of the head) per batch: one per lane class, so that the second class's follow-up never sees the first one's pairs
BlockLayout layout_block(size_t n, size_t seq_bytes, bool owned);
mwf_gpu_batch_t *batch_common(mwf_gpu_t *g, int32_t n, const int32_t *h_tl, const int32_t *h_ql, size_t seq_bytes, bool owned, BlockLayout &L);
mwf_gpu_batch_t *batch_from_host(mwf_gpu_t *g, int32_t n, const int32_t *tl, const char *const *ts, const int32_t *ql, const char *const *qs,
                                 const char *packed, int64_t packed_bytes, const int64_t *p_t_off, const int64_t *p_q_off);
float estimate_divergence_device(mwf_gpu_t *g, mwf_gpu_batch_t *b);
int alpha_prepare(mwf_gpu_t *g, mwf_gpu_batch_t *b); // "alpha_remap": classes, arena and copies of the align that is about to be planned (0 also when it fell back to the original bytes)
int alphabet_scan16(const uint8_t *t, size_t tl, const uint8_t *q, size_t ql, uint8_t sym[16]); // mwf_dbg.cpp: the class of mwf_alphabet_class16 and, classes 1 and 3, the distinct bytes ascending (the last repeated up to four / sixteen)
int alphabet_scan(const uint8_t *t, size_t tl, const uint8_t *q, size_t ql, uint8_t sym[4]); // mwf_dbg.cpp: the class of mwf_alphabet_class and, class 1, the distinct bytes ascending (the last repeated up to four)
double sketch_divergence(int32_t hit, int32_t tot, int32_t lt); // one pair's divergence from the hits of its query's `tot` 8-mers in a target of lt bases
extern "C" int mwf_gpu_test_hook(mwf_gpu_t *g, const char *name, int64_t value); // mwf_engine.cpp: forced kernels / geometries / failure paths for tests/ and profiles/
// ---- mwf_async.cpp: submit / wait and the opt-in coalescing of single calls
int64_t coalesce_window_us();
void exact_coalesced(void *km, const mwf_opt_t *opt, int32_t tl, const char *ts, int32_t ql, const char *qs, mwf_rst_t *r); // 8-mer sketch of a few pairs of a device-resident batch (0: unknown)

// ---- mwf_plan.cpp: penalties, kernel choice, launches, the whole-device passes, re-runs
Penalty make_penalty(const mwf_opt_t &o);
const char *validate(const mwf_opt_t &o);
int64_t penalty_bound(const mwf_opt_t &o, int64_t tl, int64_t ql, bool honour_max_s);
int coop_grid_limit(mwf_gpu_t *g);
int finalize(mwf_gpu_t *g, mwf_gpu_batch_t *b);
int fetch_cigars(mwf_gpu_t *g, mwf_gpu_batch_t *b);

} // namespace host
} // namespace mwf
