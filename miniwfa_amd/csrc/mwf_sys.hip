// mwf_sys.hip — one sequence pair across the whole device, systolic form (BASELINE configs 2 and 4: a 150 kb pair, a 5 Mb pair).
//
// A single pair is a strictly sequential chain of penalties (reference miniwfa.c:397-426); the only parallelism is across the
// diagonals of one wavefront, and the only dependence of lag 1 is E2/F2 of the neighbouring diagonal.  Rounds 1-2 (mwf_coop.hip, removed) exchanged
// the outer columns of every 256-column chunk between neighbouring waves at EVERY penalty and polled the fate of the two edge
// columns at every penalty: 5-6 us per penalty, whatever the window, because a penalty costs two dependent cross-CU round trips.
// Here the exchange happens once per block of P penalties (P = 8):
//   * a chunk slot computes 256 columns but owns only the inner 256 - 2P; the P columns on either side are a halo that
//     duplicates the neighbours' outer columns.  After the hand-off every column of the slot is exact; each penalty computed
//     without one loses one column per side (a cell reads columns c-1, c, c+1 of older wavefronts), so after P penalties exactly
//     the owned columns are still exact — nothing is masked, the garbage in the halo simply never reaches an owned column;
//   * every slot has a PRIVATE ring of H rows ([nH][256], halo included) and keeps E/F in registers: between hand-offs a wave
//     talks to nobody — no granule waits, no flag polls, no workgroup barrier; waves of one workgroup drift freely;
//   * at the end of a block a slot publishes what its two neighbours' halos must become — H of its outer P owned columns for
//     the block's P penalties (stored as it goes), their E/F registers, and its view of the window edges — with write-through
//     stores, then a progress word; it then waits for both neighbours' progress words and refreshes its own halo;
//   * the window (reference wf_lo/wf_hi, grown by the liveness of the edge cells, miniwfa.c:417-418, :325-326) is tracked by
//     every slot for itself: the slot that OWNS an edge column computes its liveness exactly and logs the new edge; a slot whose
//     valid columns do not contain the edge cannot be affected by it within the block; at the hand-off the exact chain of the
//     block's edges is re-derived from the owners' published values (see refresh());
//   * everything global happens once per EPOCH of 256 penalties, where the reference shrinks the band (miniwfa.c:144-171) and a
//     device-wide barrier is needed anyway: which slots take part in the next epoch (the window can grow by at most one column
//     per penalty and side), the end cell / stop rules (acted upon at the epoch's end: at most 255 surplus penalties), n_iter
//     (from the edge log), the traceback layout.
// Traceback bytes are laid out per epoch and slot (256 bytes per slot and penalty, dev::tb_byte); the second pass of the
// low-memory mode collapses the window at its checkpoints exactly as the reference does (miniwfa.c:413-416) — every slot
// knows the checkpoints in advance.  The provenance pass of the two-pass low-memory mode (SEG, round 5) runs here as well: shadow
// registers, a shadow H ring and shadow halves of the hand-off boxes; snapshots need nothing global (see sys_pass).
// Results are bit-identical to the other kernels (tests/test_gpu_parity.py, tests/test_long_pairs.py).
#include "mwf_sys_pass.h"

namespace mwf {

namespace {

// Checkpoints of the true low-memory mode: chase the provenance of the end cell back through the snapshots (reference wf_traceback_seg,
// miniwfa.c:528-549).  An index decodes to (slice, owner chunk, column) with the snapshot's chunk range; the slice gives the penalty: H ring
// slices and E/F registers are numbered by age (0 = the penalty the snapshot was taken behind).
__global__ void sys_trace_kernel(const BatchArgs A)
{
	if (threadIdx.x != 0) return;
	const int32_t grp = (int32_t)blockIdx.x; // one block per pair
	int32_t *st = group_state(A, grp);
	st[3] = 0;
	if (st[0] != ST_OK) return;
	const Penalty &P = A.pen;
	PairMem M;
	sys_pair_mem(A, grp, group_pair(A, grp), M);
	const int32_t n_snap = st[6];
	if (n_snap > A.seg_slot) { st[0] = ST_SNAP_OVERFLOW; return; }
	int32_t last = st[2];
	for (int32_t j = n_snap - 1; j >= 0; --j) {
		const int32_t *meta = M.snap_meta + (int64_t)j * 8;
		const int64_t base = (int64_t)(uint32_t)meta[0] | (int64_t)meta[1] << 32;
		const int32_t S = meta[2], gA = meta[4], n_ep = meta[5], OW = meta[6], per = n_ep * OW;
		if (last < 0 || per <= 0) { st[0] = ST_INTERNAL; return; }
		const int32_t id = last / per, rem = last - id * per, col = (gA + rem / OW) * OW + rem % OW;
		int32_t age;
		if (id < P.nH) age = id;
		else {
			const int32_t q = id - P.nH;
			if (q < P.e1) age = q;
			else if (q < 2 * P.e1) age = q - P.e1;
			else if (q < 2 * P.e1 + P.e2) age = q - 2 * P.e1;
			else if (q < 2 * P.e1 + 2 * P.e2) age = q - 2 * P.e1 - P.e2;
			else { st[0] = ST_INTERNAL; return; }
		}
		M.seg[2 * j] = S - age, M.seg[2 * j + 1] = col;
		last = M.snap[base + last];
	}
	if (last != -1) { st[0] = ST_INTERNAL; return; } // the chain must end at the origin (reference asserts, miniwfa.c:542,547)
	st[3] = n_snap;
}

// Checkpoints of the low-memory mode from the full traceback matrix of a first pass (
// reference miniwfa.c:495-549): the same walk over this kernel's traceback layout.
__global__ void sys_walk_kernel(const BatchArgs A)
{
	// One wave, every lane walking the same chain (their loads are one broadcast): a step is one dependent byte of a matrix written long ago — a round trip
	// to HBM.  Every 40 rows the 64 lanes fetch the byte in the walk's column of the next 64 rows together, so that the steps through them hit L2
	// (dev::traceback_wave does the same).
	const int32_t lane = (int32_t)threadIdx.x;
	const int32_t grp = (int32_t)blockIdx.x; // one block per pair
	int32_t *st = group_state(A, grp);
	if (lane == 0) st[3] = 0;
	if (st[0] != ST_OK) return;
	const Penalty &P = A.pen;
	PairMem M;
	sys_pair_mem(A, grp, group_pair(A, grp), M);
	const int32_t s_final = st[1], step = A.step;
	const int32_t n_seg = s_final / step;
	if (n_seg > A.seg_slot) { if (lane == 0) st[0] = ST_SNAP_OVERFLOW; return; }
	int32_t arr = 0, s = s_final, col = M.ql + 1; // array 0=H 1=E1 2=F1 3=E2 4=F2; the end cell is on diagonal ql-tl
	int32_t j = n_seg - 1, pf_at = s_final;
	while (j >= 0) {
		const int32_t Sj = (j + 1) * step - 1;
		if (s <= Sj) { // first cell of the chain that already existed at snapshot j
			if (lane == 0) M.seg[2 * j] = s, M.seg[2 * j + 1] = col;
			--j;
			continue;
		}
		if (s <= 0) { if (lane == 0) st[0] = ST_INTERNAL; return; }
		if (s <= pf_at && M.ep && A.tb_slot_bytes > 0) {
			const int32_t r = s - 2 - lane;
			uint32_t pf = 0;
			if (r >= 0) {
				const int64_t base = M.ep[2 * (r >> 8)], gn = M.ep[2 * (r >> 8) + 1];
				const int32_t g = col / M.ep_ow;
				int64_t at = base + ((int64_t)(r & 255) * (int32_t)(gn >> 32) + (g - (int32_t)(gn & 0xffffffff))) * M.ep_kw + (col - (g * M.ep_ow - M.ep_p));
				at = min(max(at, (int64_t)0), (int64_t)A.tb_slot_bytes - 1); // (an older row may not reach this column: any byte of the arena will do)
				pf = M.tb[at];
			}
			asm volatile("" :: "v"(pf));
			pf_at = s - 40;
		}
		const uint32_t x = tb_byte(M, s - 1, col);
		if (arr == 0) {
			const uint32_t z = x & 7u;
			if (z == 0) s -= P.x;
			else arr = (int32_t)z == 1 ? 1 : (int32_t)z == 2 ? 2 : (int32_t)z == 3 ? 3 : 4;
		} else if (arr == 1) { if (x & 0x08u) s -= P.e1; else s -= P.oe1, arr = 0; col -= 1; }
		else if (arr == 2) { if (x & 0x10u) s -= P.e1; else s -= P.oe1, arr = 0; col += 1; }
		else if (arr == 3) { if (x & 0x20u) s -= P.e2; else s -= P.oe2, arr = 0; col -= 1; }
		else { if (x & 0x40u) s -= P.e2; else s -= P.oe2, arr = 0; col += 1; }
	}
	if (lane == 0) st[3] = n_seg;
}

__global__ __launch_bounds__(64) void sys_finish_kernel(const BatchArgs A)
{
	const int32_t grp = (int32_t)blockIdx.x; // one block per pair
	const int32_t pair = group_pair(A, grp);
	PairMem M;
	sys_pair_mem(A, grp, pair, M);
	const int32_t *st1 = group_state(A, grp), *st = A.step > 0 && A.want_cigar ? st1 + 8 : st1;
	PassResult R;
	int32_t status = st1[0] != ST_OK ? st1[0] : st[0];
	R.status = status, R.s = st[1], R.info = st[2], R.n_snap = 0;
	R.cells = (int64_t)(uint32_t)st[4] | (int64_t)st[5] << 32;
	const int64_t cells1 = A.step > 0 && A.want_cigar ? ((int64_t)(uint32_t)st1[4] | (int64_t)st1[5] << 32) : 0;
	if (A.dbg && (status == ST_OK || status == ST_STOPPED)) { // band trace (diagnostics): lo,hi of every slice, from the edge log
		const int32_t *logL = A.sys_log + (int64_t)grp * A.sys_log_stride, *logH = logL + A.sys_log_stride / 2;
		const int32_t cmax = M.tl + M.ql + 1, n_seg = A.step > 0 && A.want_cigar ? seg_effective(M.seg, st1[3]) : 0;
		for (int32_t sp = threadIdx.x; sp < R.s && sp < A.dbg_cap; sp += 64) {
			int32_t a = logL[sp], b = logH[sp];
			for (int32_t j = 0; j < n_seg; ++j)
				if (M.seg[2 * j] == sp) a = b = M.seg[2 * j + 1];
			M.dbg[2 * sp] = a > 1 ? a - 1 : 1, M.dbg[2 * sp + 1] = b < cmax ? b + 1 : cmax;
		}
	}
	finish_pair(A, M, grp, pair, R, status, cells1);
}

} // namespace

int64_t sys_chunk_slots(int grid) { return (int64_t)grid * kNW * kK; }
int64_t coop_chunk_slots(int grid) { return sys_chunk_slots(grid); }
// penalties the whole-device kernel is instantiated for; the per-slot window history lives in LDS
bool coop_supported(const Penalty &p)
{
	const bool built = (p.e1 == 2 && p.e2 == 1) || (p.e1 == 2 && p.e2 == 2) || (p.e1 == 1 && p.e2 == 1);
	const bool deep = (p.e1 == 3 || p.e1 == 4) && (p.e2 == 1 || p.e2 == 2); // mwf_sys_deep.hip
	return (built || deep) && p.nH <= kMaxRing;
}
int sys_owned_cols(int p, int c) { return 64 * c - 2 * p; }
bool sys_p_supported(int p)
{
#ifdef MWF_SYS_ALL_P
	return p == 4 || p == 8 || p == 16;
#else
	return p == 8; // the product build instantiates one block length (P = 4 and 16 measured slower)
#endif
}
bool sys_c_supported(int c)
{
#ifdef MWF_SYS_C2
	if (c == 2) return true; // (experiment: 128-column slots)
#endif
	return c == 1 || c == 4;
}

// One workgroup per CU.  That a workgroup of the form being launched fits a CU at all (registers, LDS, scratch) is checked where the form is known:
// launch_pass_pc (mwf_sys_pass.h) asks the runtime once per form and returns kSysNotResident instead of launching.
int sys_max_grid()
{
	int dev = 0, n_cu = 0;
	if (hipGetDevice(&dev) != hipSuccess) return 0;
	if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
	return n_cu; // every workgroup resident, which the waits between them rely on
}

int launch_sys_pass(const BatchArgs &a, int grid, void *stream)
{
	if (a.pen.e1 == 2 && a.pen.e2 == 1) return launch_pass_d<2, 1, true>(a, grid, (hipStream_t)stream);
	if (a.pen.e1 == 2 && a.pen.e2 == 2) return launch_pass_d<2, 2, true>(a, grid, (hipStream_t)stream);
	if (a.pen.e1 == 1 && a.pen.e2 == 1) return launch_pass_d<1, 1, false>(a, grid, (hipStream_t)stream);
	return launch_sys_pass_deep(a, grid, stream);
}

int launch_sys_trace(const BatchArgs &a, void *stream)
{
	hipLaunchKernelGGL(sys_trace_kernel, dim3(a.coop_groups > 0 ? a.coop_groups : 1), dim3(64), 0, (hipStream_t)stream, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_sys_walk(const BatchArgs &a, void *stream)
{
	hipLaunchKernelGGL(sys_walk_kernel, dim3(a.coop_groups > 0 ? a.coop_groups : 1), dim3(64), 0, (hipStream_t)stream, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_sys_finish(const BatchArgs &a, void *stream)
{
	hipLaunchKernelGGL(sys_finish_kernel, dim3(a.coop_groups > 0 ? a.coop_groups : 1), dim3(64), 0, (hipStream_t)stream, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace mwf
