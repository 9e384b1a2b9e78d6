// mwf_ends_band.h — the diagonal band of an ends-free or extension alignment (include/miniwfa.h, mwf_band_t) as pure functions of the pair's lengths,
// its allowances and its band: the clamp, the feasibility rule and the penalty bound.  mwf_plan.cpp sizes launches by them, mwf_ends.hip restates the
// feasibility rule on the device, tests/host/ends_band_sanitize.cpp sweeps them under sanitizers.  Nothing here includes anything of the engine, and every
// intermediate is 64 bits wide: allowances up to INT32_MAX and band ends anywhere in int32 meet lengths up to 2^31 without overflow.
#pragma once
#include <stdint.h>
#include <algorithm>

namespace mwf {

// an inclusive range of diagonals (d = query index - target index); lo > hi: empty
struct DiagRange {
	int64_t lo, hi;
	bool empty() const { return lo > hi; }
	int64_t width() const { return empty() ? 0 : hi - lo + 1; }
	bool meets(const DiagRange &o) const { return !empty() && !o.empty() && lo <= o.hi && o.lo <= hi; }
};

// the band as the pass uses it: [d_lo, d_hi] clamped to the diagonals the matrix has, [-tl, ql]
inline DiagRange band_clamped(int64_t tl, int64_t ql, int64_t d_lo, int64_t d_hi) { return DiagRange{std::max<int64_t>(d_lo, -tl), std::min<int64_t>(d_hi, ql)}; }
// the diagonals an alignment may begin on: the origin window [-min(t_beg, tl), min(q_beg, ql)] ...
inline DiagRange origin_diagonals(int64_t tl, int64_t ql, int64_t t_beg, int64_t q_beg) { return DiagRange{-std::min<int64_t>(t_beg, tl), std::min<int64_t>(q_beg, ql)}; }
// ... and end on: the query's last row with at most t_end target bases behind the cell, the target's last column with at most q_end query bases behind it
inline DiagRange end_diagonals(int64_t tl, int64_t ql, int64_t t_end, int64_t q_end) { return DiagRange{ql - tl - std::min<int64_t>(q_end, ql), ql - tl + std::min<int64_t>(t_end, tl)}; }

// Feasibility: an alignment whose every cell lies inside the band exists iff the clamped band is non-empty and meets both sets.  (One diagonal of each
// intersection and the gap between them stay inside the band, an interval.)  Allowances are >= 0.  For an extension, {0, INT32_MAX, 0, INT32_MAX}, this is
// d_lo <= 0 <= d_hi.
inline bool ends_band_feasible(int64_t tl, int64_t ql, int64_t t_beg, int64_t t_end, int64_t q_beg, int64_t q_end, int64_t d_lo, int64_t d_hi)
{
	const DiagRange B = band_clamped(tl, ql, d_lo, d_hi);
	return B.meets(origin_diagonals(tl, ql, t_beg, q_beg)) && B.meets(end_diagonals(tl, ql, t_end, q_end));
}

// Upper bound on the penalty of a banded alignment, for any feasible band: that path is at most min(tl, ql) diagonal steps and one gap of at most
// max(tl, ql) bases.  (mwf_plan_classes.h penalty_bound, gap(tl) + gap(ql), leaves the band.)  max_s > 0 with honour_max_s: capped at max_s + 1, as there.
inline int64_t ends_band_penalty_bound(int64_t x, int64_t o1, int64_t e1, int64_t o2, int64_t e2, int64_t max_s, int64_t tl, int64_t ql, bool honour_max_s)
{
	auto gap = [&](int64_t L) -> int64_t { return L == 0 ? 0 : std::min<int64_t>(o1 + L * e1, o2 + L * e2); };
	int64_t b = x * std::min(tl, ql) + std::max(gap(tl), gap(ql));
	if (honour_max_s && max_s > 0) b = std::min<int64_t>(b, max_s + 1);
	return b;
}

} // namespace mwf
