// mwf_sketch.hip — the small kernels around an align call that are no alignment kernels: the reset of the per-pair outputs and work
// counters, and the 8-mer sketches (divergence of a wrapped batch, predicted work per pair).  A unit of their own, so that an edit
// here leaves the source hash of every alignment kernel (build.py kernel_fingerprint) as it was.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "mwf_internal.h"

namespace mwf {

// Start of an align call: every pair "not run" (status -1, s -2: not final), CIGAR pool and work queue at zero.
__global__ void reset_kernel(int32_t *status, int32_t *s, int32_t n, unsigned long long *cig_head, int32_t *queue, int32_t n_queue)
{
	const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i < n) status[i] = -1, s[i] = -2;
	if (i < n_queue) queue[i] = 0; // the work counters of the align call's launches (the grid covers n_queue)
	if (i == 0) cig_head[0] = 0ull, cig_head[1] = 0ull, cig_head[2] = 0ull, cig_head[3] = 0ull; // (the second word: flags of the align's kernels for the host, BatchArgs::cig_head + 1; the third and fourth: BatchArgs::retry_count of the two lane classes)
}

int launch_reset(int32_t *status, int32_t *s, int32_t n, unsigned long long *cig_head, int32_t *queue, int32_t n_queue, void *stream)
{
	const int grid = (std::max(n, n_queue) + 255) / 256 > 0 ? (std::max(n, n_queue) + 255) / 256 : 1;
	hipLaunchKernelGGL(reset_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, status, s, n, cig_head, queue, n_queue);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- divergence sketch of a device-resident batch (mwf_gpu_batch_wrap: the host never sees the bytes).  The same statistic as
// host::estimate_divergence (mwf_memory.cpp) computes while it packs a batch from host memory: how many of the 8-mers of a query's
// prefix (up to 1500 bases) occur in its target's prefix — (1 - d)^8 plus chance hits.  One workgroup per sampled pair (at most 16:
// pair k n / samples), the 4^8-bit set in LDS; out[k] = hits.  The reference has no size classes to get wrong (one loop serves any
// divergence, miniwfa.c:396-426): this is what lets the classes of a WRAPPED batch follow its divergence too.
constexpr int kSketchK = 8, kSketchLen = 1500;
__device__ __forceinline__ uint32_t sketch_kmer(const uint8_t *p)
{
	uint32_t h = 0;
#pragma unroll
	for (int i = 0; i < kSketchK; ++i) h = (h << 2) | ((p[i] >> 1) & 3u);
	return h;
}
// hits of the query's 8-mers in the target: the calling workgroup's 256 threads, the 4^8-bit set in LDS; the count lands in *hits
__device__ __forceinline__ void sketch_hits(const uint8_t *t, int32_t lt, const uint8_t *q, int32_t lq, uint32_t *bits, int32_t *hits)
{
	for (int32_t j = threadIdx.x; j < (1 << (2 * kSketchK)) / 32; j += 256) bits[j] = 0;
	if (threadIdx.x == 0) *hits = 0;
	__syncthreads();
	for (int32_t j = threadIdx.x; j + kSketchK <= lt; j += 256) {
		const uint32_t h = sketch_kmer(t + j);
		atomicOr(&bits[h >> 5], 1u << (h & 31));
	}
	__syncthreads();
	int32_t mine = 0;
	for (int32_t j = threadIdx.x; j + kSketchK <= lq; j += 256) {
		const uint32_t h = sketch_kmer(q + j);
		mine += (int32_t)((bits[h >> 5] >> (h & 31)) & 1u);
	}
	if (mine) atomicAdd(hits, mine);
	__syncthreads();
}
__global__ __launch_bounds__(256) void sketch_kernel(const uint8_t *seqs, const int64_t *t_off, const int32_t *tl, const int64_t *q_off, const int32_t *ql,
                                                      int32_t n, int32_t samples, int32_t *out)
{
	__shared__ uint32_t bits[(1 << (2 * kSketchK)) / 32];
	__shared__ int32_t hits;
	const int32_t i = (int32_t)((int64_t)blockIdx.x * n / samples);
	sketch_hits(seqs + t_off[i], min(tl[i], kSketchLen), seqs + q_off[i], min(ql[i], kSketchLen), bits, &hits);
	if (threadIdx.x == 0) out[blockIdx.x] = hits;
}

int launch_sketch(const uint8_t *seqs, const int64_t *t_off, const int32_t *tl, const int64_t *q_off, const int32_t *ql, int32_t n, int32_t samples, int32_t *out, void *stream)
{
	hipLaunchKernelGGL(sketch_kernel, dim3(samples), dim3(256), 0, (hipStream_t)stream, seqs, t_off, tl, q_off, ql, n, samples, out);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- per-pair work sketch (mwf_plan.cpp: the deal order of the band classes on the shared work counter).  A pair's penalty s — and with it the
// penalties its workgroup runs — grows with its divergence, and an equal-length batch at 5 % holds pairs of s 2118 ... 2838: dealt by length, the
// last ones finish far apart while CUs idle.  The same statistic as sketch_kernel over the WHOLE sequences (a 1500-base prefix correlates 0.34 with s,
// the whole pair 0.88): one workgroup per pair order[k] (order null: pair k), out[k] = hits.  ~20 kB read per 10 kb pair, once per plan.
__global__ __launch_bounds__(256) void pair_sketch_kernel(const uint8_t *seqs, const int64_t *t_off, const int32_t *tl, const int64_t *q_off, const int32_t *ql,
                                                           const int32_t *order, int32_t *out)
{
	__shared__ uint32_t bits[(1 << (2 * kSketchK)) / 32];
	__shared__ int32_t hits;
	const int32_t i = order ? order[blockIdx.x] : (int32_t)blockIdx.x;
	sketch_hits(seqs + t_off[i], tl[i], seqs + q_off[i], ql[i], bits, &hits);
	if (threadIdx.x == 0) out[blockIdx.x] = hits;
}

int launch_pair_sketch(const uint8_t *seqs, const int64_t *t_off, const int32_t *tl, const int64_t *q_off, const int32_t *ql, const int32_t *order, int32_t n, int32_t *out, void *stream)
{
	if (n <= 0) return 0;
	hipLaunchKernelGGL(pair_sketch_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, seqs, t_off, tl, q_off, ql, order, out);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace mwf
