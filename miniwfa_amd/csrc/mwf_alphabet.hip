// mwf_alphabet.hip — per-pair alphabet classes and the remapped copies of pairs of at most four ("alpha_remap") or sixteen ("alpha16") distinct bytes, on the device (gfx950, wave64).  Off the align
// path: nothing here runs unless the engine's "alpha_remap" tunable is 1 (alpha_prepare, mwf_memory.cpp).
//
// Every fast path holds sequences at 2 bits per base, which takes plain upper-case A/C/G/T.  The recurrence only needs the equality relation
// between bytes, so a pair with at most four distinct bytes (lower case, U for T, bases coded 0..3) aligns exactly as its image under a bijection
// of those bytes onto A, C, G, T does: same s, n_iter and CIGAR.  The rule, the same as the host twin's (mwf_alphabet_class, mwf_dbg.cpp): the
// distinct bytes of target and query together, in ascending byte value, map to "ACGT"[rank].
//
// One workgroup per pair, over an index list, two launches (AlphabetArgs::mode), no global atomics, plain vector stores:
//   0  classify: the presence set of the pair's bytes — 256 bits, eight words per thread, gathered with 16-byte loads between a bytewise head
//      (up to the first 16-byte boundary: the head of a sequence is not aligned) and a bytewise tail; OR-reduced across the wave in registers
//      and across the waves through LDS.  Its population count and one mask give the class; thread 0 writes the class and, for classes 1 and 3, the
//      distinct bytes in ascending order (sixteen bytes per pair).  A batch built from host memory skips this launch: the host twin saw the bytes while it packed.
//   1  copy, class-1 pairs: every byte b becomes "ACGT"[how many of the pair's three lowest distinct bytes are below b], 16 bytes per
//      thread and step (an unaligned load, an aligned store: the host puts every copy on a 16-byte boundary), head and tail bytewise.
//      Class-3 pairs ("alpha16": five to sixteen distinct bytes, in ascending order the codes 0 ... 15): the workgroup first builds a 256-entry byte
//      table in LDS — entry b = 0x40 | how many of the pair's symbols are below b — and the same copy loop looks every byte up in it.
// The workgroup also enters the copies' offsets in the per-pair offset arrays the align kernels will be given.
// No access leaves [t_off, t_off + tl) / [q_off, q_off + ql) of the source or [dst_t, dst_t + tl) / [dst_q, dst_q + ql) of the arena.
// Geometry: the host picks the workgroup size for the launch from the longest pair of the batch (alphabet_block below), as mwf_cigar_ops.hip does.
#include <hip/hip_runtime.h>
#include "mwf_internal.h"

namespace mwf {
namespace {

// 'A' 65, 'C' 67, 'G' 71, 'T' 84: bits of presence word 2 (bytes 64 .. 95)
constexpr uint32_t kAcgtWord2 = (1u << 1) | (1u << 3) | (1u << 7) | (1u << 20);

__device__ __forceinline__ void note(uint32_t (&m)[8], uint32_t x)
{
	const uint32_t w = x >> 5, bit = 1u << (x & 31u);
#pragma unroll
	for (int k = 0; k < 8; ++k) m[k] |= w == (uint32_t)k ? bit : 0u;
}

__device__ __forceinline__ void note4(uint32_t (&m)[8], uint32_t v)
{
	note(m, v & 0xffu), note(m, (v >> 8) & 0xffu), note(m, (v >> 16) & 0xffu), note(m, v >> 24);
}

template <int B>
__device__ __forceinline__ void scan_range(const uint8_t *p, int32_t len, uint32_t (&m)[8])
{
	const int tid = (int)threadIdx.x;
	const int32_t head = min(len, (int32_t)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u));
	for (int32_t j = tid; j < head; j += B) note(m, p[j]);
	const int32_t n16 = (len - head) >> 4;
	const uint4 *w = (const uint4*)(p + head);
	for (int32_t k = tid; k < n16; k += B) {
		const uint4 v = w[k];
		note4(m, v.x), note4(m, v.y), note4(m, v.z), note4(m, v.w);
	}
	for (int32_t j = head + (n16 << 4) + tid; j < len; j += B) note(m, p[j]);
}

__device__ __forceinline__ uint32_t remap1(uint32_t b, uint32_t m0, uint32_t m1, uint32_t m2)
{
	const uint32_t rank = (b > m0 ? 1u : 0u) + (b > m1 ? 1u : 0u) + (b > m2 ? 1u : 0u);
	return (0x54474341u >> (8u * rank)) & 0xffu; // "ACGT"
}

__device__ __forceinline__ uint32_t remap4(uint32_t v, uint32_t m0, uint32_t m1, uint32_t m2)
{
	return remap1(v & 0xffu, m0, m1, m2) | remap1((v >> 8) & 0xffu, m0, m1, m2) << 8 | remap1((v >> 16) & 0xffu, m0, m1, m2) << 16 | remap1(v >> 24, m0, m1, m2) << 24;
}

// class 3: through the workgroup's table (the caller's barrier stands between its stores and these reads)
__device__ __forceinline__ uint32_t table4(const uint8_t *tab, uint32_t v)
{
	return (uint32_t)tab[v & 0xffu] | (uint32_t)tab[(v >> 8) & 0xffu] << 8 | (uint32_t)tab[(v >> 16) & 0xffu] << 16 | (uint32_t)tab[v >> 24] << 24;
}

template <int B>
__device__ __forceinline__ void copy_range16(const uint8_t *src, uint8_t *dst, int32_t len, const uint8_t *tab)
{
	const int tid = (int)threadIdx.x;
	const int32_t head = min(len, (int32_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u)); // (0 where the host laid the arena out)
	for (int32_t j = tid; j < head; j += B) dst[j] = tab[src[j]];
	const int32_t n16 = (len - head) >> 4;
	uint4 *w = (uint4*)(dst + head);
	for (int32_t k = tid; k < n16; k += B) {
		uint32_t q[4];
		__builtin_memcpy(q, src + head + ((int64_t)k << 4), 16);
		uint4 o;
		o.x = table4(tab, q[0]), o.y = table4(tab, q[1]), o.z = table4(tab, q[2]), o.w = table4(tab, q[3]);
		w[k] = o;
	}
	for (int32_t j = head + (n16 << 4) + tid; j < len; j += B) dst[j] = tab[src[j]];
}

template <int B>
__device__ __forceinline__ void copy_range(const uint8_t *src, uint8_t *dst, int32_t len, uint32_t m0, uint32_t m1, uint32_t m2)
{
	const int tid = (int)threadIdx.x;
	const int32_t head = min(len, (int32_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u)); // (0 where the host laid the arena out)
	for (int32_t j = tid; j < head; j += B) dst[j] = (uint8_t)remap1(src[j], m0, m1, m2);
	const int32_t n16 = (len - head) >> 4;
	uint4 *w = (uint4*)(dst + head);
	for (int32_t k = tid; k < n16; k += B) {
		uint32_t q[4];
		__builtin_memcpy(q, src + head + ((int64_t)k << 4), 16);
		uint4 o;
		o.x = remap4(q[0], m0, m1, m2), o.y = remap4(q[1], m0, m1, m2), o.z = remap4(q[2], m0, m1, m2), o.w = remap4(q[3], m0, m1, m2);
		w[k] = o;
	}
	for (int32_t j = head + (n16 << 4) + tid; j < len; j += B) dst[j] = (uint8_t)remap1(src[j], m0, m1, m2);
}

// MODE 0: classify; 1: copy.  B threads, one pair.
template <int B, int MODE>
__global__ __launch_bounds__(B) void alphabet_kernel(AlphabetArgs A)
{
	constexpr int NW = B / 64;
	const int32_t pair = A.ids ? A.ids[blockIdx.x] : (int32_t)blockIdx.x;
	const int tid = (int)threadIdx.x;
	const int32_t tl = A.tl[pair], ql = A.ql[pair];
	const uint8_t *t = A.seqs + A.t_off[pair], *q = A.seqs + A.q_off[pair];
	if (MODE == 1) {
		const int cls = A.cls[pair]; // (uniform: one pair per workgroup)
		if (cls != 1 && cls != 3) return;
		const uint32_t *sw = A.sym + (int64_t)pair * kAlphaSymWords;
		uint8_t *base = const_cast<uint8_t*>(A.seqs);
		const int64_t dt = A.dst_t[blockIdx.x], dq = A.dst_q[blockIdx.x];
		if (cls == 3) {
			__shared__ uint8_t s_tab[256];
			uint32_t s4[kAlphaSymWords];
#pragma unroll
			for (int k = 0; k < kAlphaSymWords; ++k) s4[k] = sw[k];
			for (int bb = tid; bb < 256; bb += B) { // (the symbols ascend and the last one is repeated: the count of those below b is b's code)
				uint32_t rank = 0;
#pragma unroll
				for (int k = 0; k < 4 * kAlphaSymWords; ++k) rank += ((s4[k >> 2] >> (8 * (k & 3))) & 0xffu) < (uint32_t)bb ? 1u : 0u;
				s_tab[bb] = (uint8_t)(0x40u | (rank & 15u));
			}
			__syncthreads();
			copy_range16<B>(t, base + dt, tl, s_tab);
			copy_range16<B>(q, base + dq, ql, s_tab);
		} else {
			const uint32_t s = sw[0], m0 = s & 0xffu, m1 = (s >> 8) & 0xffu, m2 = (s >> 16) & 0xffu;
			copy_range<B>(t, base + dt, tl, m0, m1, m2);
			copy_range<B>(q, base + dq, ql, m0, m1, m2);
		}
		if (tid == 0) A.out_t_off[pair] = dt, A.out_q_off[pair] = dq;
		return;
	}
	__shared__ uint32_t s_m[NW][8];
	uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	scan_range<B>(t, tl, m);
	scan_range<B>(q, ql, m);
#pragma unroll
	for (int k = 0; k < 8; ++k) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) m[k] |= (uint32_t)__shfl_xor((int32_t)m[k], d, 64);
	}
	if (NW > 1) {
		if ((tid & 63) == 0) {
#pragma unroll
			for (int k = 0; k < 8; ++k) s_m[tid >> 6][k] = m[k];
		}
		__syncthreads();
	}
	if (tid != 0) return;
	if (NW > 1) {
		for (int v = 1; v < NW; ++v) {
#pragma unroll
			for (int k = 0; k < 8; ++k) m[k] |= s_m[v][k];
		}
	}
	int count = 0;
	uint32_t other = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k) count += __popc(m[k]), other |= k == 2 ? (m[k] & ~kAcgtWord2) : m[k];
	const int cls = other == 0 ? 0 : count <= 4 ? 1 : (A.alpha16 && count <= 16) ? 3 : 2;
	uint32_t sym[kAlphaSymWords] = {0, 0, 0, 0};
	auto put = [&](int at, uint32_t b) { // (constant indices once unrolled: the record stays in registers)
#pragma unroll
		for (int k = 0; k < kAlphaSymWords; ++k) sym[k] |= (at >> 2) == k ? b << (8 * (at & 3)) : 0u;
	};
	if (cls == 1 || cls == 3) {
		const int fill = cls == 1 ? 4 : 16;
		int have = 0;
		uint32_t last = 0;
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			uint32_t w = m[k];
			while (w) {
				last = (uint32_t)(32 * k + __ffs((int)w) - 1);
				put(have++, last);
				w &= w - 1;
			}
		}
		for (; have < fill; ++have) put(have, last);
	}
	A.cls[pair] = (int8_t)cls;
#pragma unroll
	for (int k = 0; k < kAlphaSymWords; ++k) A.sym[(int64_t)pair * kAlphaSymWords + k] = sym[k];
}

template <int B>
int launch_as(const AlphabetArgs &a, hipStream_t st)
{
	const dim3 grid((unsigned)a.n_pairs), block(B);
	if (a.mode == 0) hipLaunchKernelGGL((alphabet_kernel<B, 0>), grid, block, 0, st, a);
	else hipLaunchKernelGGL((alphabet_kernel<B, 1>), grid, block, 0, st, a);
	return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace

// Threads per pair from the longest pair (target + query bases) of the batch: a wave for reads (a 150 bp pair is nineteen 16-byte loads), four
// waves from 2 kb on, sixteen for a pair of the whole-device kernel's range.
int alphabet_block(int64_t max_len) { return max_len <= 2048 ? 64 : max_len <= 65536 ? 256 : 1024; }

int launch_alphabet(const AlphabetArgs &a, int block, void *stream)
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
