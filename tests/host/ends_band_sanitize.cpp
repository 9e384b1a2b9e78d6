// The pure rules of a banded ends-free alignment (miniwfa_amd/csrc/mwf_ends_band.h) stand-alone, for tests/test_ends_band_cpu.py: built with
// -fsanitize=address,undefined, nothing loaded into python.
//   ends_band_sanitize          sweeps (tl, ql, allowances, band) grids — INT32_MAX allowances, INT32_MIN / INT32_MAX band ends, lengths up to 2^31 - 5 —
//                               and checks the feasibility rule against a brute-force restatement on small pairs, the clamp and the bound against their
//                               definitions; prints "ends_band_sanitize OK"
//   ends_band_sanitize rule     reads lines "tl ql t_beg t_end q_beg q_end d_lo d_hi x o1 e1 o2 e2 max_s" and prints "feasible width bound" per line
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "mwf_ends_band.h"

using namespace mwf;

// the rule by enumeration: some diagonal of the band that the matrix has is an origin diagonal, and some is an end diagonal
static bool brute_feasible(int64_t tl, int64_t ql, int64_t t_beg, int64_t t_end, int64_t q_beg, int64_t q_end, int64_t d_lo, int64_t d_hi)
{
	bool origin = false, end = false;
	for (int64_t d = -tl; d <= ql; ++d) {
		if (d < d_lo || d > d_hi) continue;
		// an alignment may begin at (qb, 0) with qb <= q_beg (diagonal qb) or at (0, tb) with tb <= t_beg (diagonal -tb)
		if ((d >= 0 && d <= q_beg) || (d <= 0 && -d <= t_beg)) origin = true;
		// ... and end at (ql, te) with tl - te <= t_end (diagonal ql - te) or at (qe, tl) with ql - qe <= q_end (diagonal qe - tl)
		const int64_t te = ql - d, qe = d + tl;
		if ((te >= 0 && te <= tl && tl - te <= t_end) || (qe >= 0 && qe <= ql && ql - qe <= q_end)) end = true;
	}
	return origin && end;
}

static int fail(const char *what, int64_t a, int64_t b, int64_t c, int64_t d)
{
	fprintf(stderr, "ends_band_sanitize: %s (%lld %lld %lld %lld)\n", what, (long long)a, (long long)b, (long long)c, (long long)d);
	return 1;
}

static int sweep()
{
	const int32_t allow[] = {0, 1, 2, 5, INT32_MAX};
	const int32_t ends_of_band[] = {INT32_MIN, INT32_MIN + 1, -7, -3, -1, 0, 1, 2, 6, INT32_MAX - 1, INT32_MAX};
	long long n = 0, n_feasible = 0;
	for (int32_t tl = 0; tl <= 5; ++tl)
		for (int32_t ql = 0; ql <= 5; ++ql)
			for (int32_t t_beg : allow)
				for (int32_t t_end : allow)
					for (int32_t q_beg : allow)
						for (int32_t q_end : allow)
							for (int32_t d_lo : ends_of_band)
								for (int32_t d_hi : ends_of_band) {
									const bool got = ends_band_feasible(tl, ql, t_beg, t_end, q_beg, q_end, d_lo, d_hi);
									if (got != brute_feasible(tl, ql, t_beg, t_end, q_beg, q_end, d_lo, d_hi)) return fail("feasibility", tl, ql, d_lo, d_hi);
									const DiagRange B = band_clamped(tl, ql, d_lo, d_hi);
									if (B.lo < -(int64_t)tl || B.hi > ql || B.width() < 0 || B.width() > (int64_t)tl + ql + 1) return fail("clamp", tl, ql, d_lo, d_hi);
									if (got && B.empty()) return fail("feasible but empty", tl, ql, d_lo, d_hi);
									++n, n_feasible += got;
								}
	if (n_feasible == 0 || n_feasible == n) return fail("the grid holds only one answer", n, n_feasible, 0, 0);
	// the longest pairs the library takes, every allowance and band end at the limits of int32: no overflow anywhere (the sanitizer is the check), and
	// the answers that are known
	const int32_t big[] = {0, 1, INT32_MAX / 2, INT32_MAX - 5};
	for (int32_t tl : big)
		for (int32_t ql : big) {
			if ((int64_t)tl + ql + 4 >= ((int64_t)1 << 31)) continue;
			for (int32_t a : {0, 1, INT32_MAX})
				for (int32_t d_lo : ends_of_band)
					for (int32_t d_hi : ends_of_band) {
						const bool got = ends_band_feasible(tl, ql, a, a, a, a, d_lo, d_hi);
						if (d_lo > d_hi && got) return fail("an empty band is feasible", tl, ql, d_lo, d_hi);
						if (d_lo == INT32_MIN && d_hi == INT32_MAX && !got && (a == INT32_MAX || tl == ql)) return fail("the whole matrix is infeasible", tl, ql, a, 0);
						if (a == 0 && got != (d_lo <= 0 && d_hi >= 0 && d_lo <= (int64_t)ql - tl && d_hi >= (int64_t)ql - tl)) return fail("zero allowances", tl, ql, d_lo, d_hi);
						(void)band_clamped(tl, ql, d_lo, d_hi).width();
					}
			// the extension's rule: d_lo <= 0 <= d_hi
			for (int32_t d_lo : ends_of_band)
				for (int32_t d_hi : ends_of_band)
					if (ends_band_feasible(tl, ql, 0, INT32_MAX, 0, INT32_MAX, d_lo, d_hi) != (d_lo <= 0 && d_hi >= 0)) return fail("extension", tl, ql, d_lo, d_hi);
			const int64_t b = ends_band_penalty_bound(255, 127, 127, 254, 1, 0, tl, ql, true);
			if (b < 0) return fail("bound", tl, ql, b, 0);
			if (ends_band_penalty_bound(4, 4, 2, 15, 1, 100, tl, ql, true) > 101) return fail("bound under max_s", tl, ql, 0, 0);
		}
	// the header's example: two 100-base sequences under band {0} cost 400; the plain bound is 230
	if (ends_band_penalty_bound(4, 4, 2, 15, 1, 0, 100, 100, true) < 400) return fail("bound of the example", 0, 0, 0, 0);
	printf("ends_band_sanitize OK: %lld cases, %lld feasible\n", n, n_feasible);
	return 0;
}

static int rule_lines()
{
	long long v[14];
	for (;;) {
		int got = 0;
		for (; got < 14; ++got)
			if (scanf("%lld", &v[got]) != 1) break;
		if (got == 0 && feof(stdin)) return 0;
		if (got != 14) return 2;
		printf("%d %lld %lld\n", (int)ends_band_feasible(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]), (long long)band_clamped(v[0], v[1], v[6], v[7]).width(),
		       (long long)ends_band_penalty_bound(v[8], v[9], v[10], v[11], v[12], v[13], v[0], v[1], true));
	}
}

int main(int argc, char **argv)
{
	if (argc == 1) return sweep();
	if (argc == 2 && !strcmp(argv[1], "rule")) return rule_lines();
	fprintf(stderr, "usage: ends_band_sanitize [rule < lines]\n");
	return 1;
}
