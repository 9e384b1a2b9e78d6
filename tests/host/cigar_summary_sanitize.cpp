// Stand-alone driver for mwf_cigar_summary (csrc/mwf_dbg.cpp) on malformed CIGARs.  tests/test_cigar_ops_cpu.py compiles it together with
// mwf_dbg.cpp under -fsanitize=address,undefined and runs it as a child process: the sequences live in heap blocks of exactly their length,
// so a read outside ts[0,tl) / qs[0,ql) is an AddressSanitizer report, and the expected records are checked as well.
// The pair and the cases are those of tests/cigar_ops_ref.py (HAND_T, HAND_Q, HAND_CASES): CIGAR 10= 1X 3D 8= 2I 12=.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "miniwfa.h"

static int failures = 0;

static void check(const char *name, const std::vector<uint32_t> &words, int32_t tl, const char *t, int32_t ql, const char *q, const int32_t (&want)[12])
{
	// exact-size heap copies: no terminator, no slack
	char *ts = (char*)malloc(tl > 0 ? tl : 1), *qs = (char*)malloc(ql > 0 ? ql : 1);
	if (tl > 0) memcpy(ts, t, tl);
	if (ql > 0) memcpy(qs, q, ql);
	uint32_t *w = (uint32_t*)malloc(words.empty() ? 4 : words.size() * 4);
	if (!words.empty()) memcpy(w, words.data(), words.size() * 4);
	mwf_opt_t opt;
	memset(&opt, 0, sizeof(opt));
	opt.x = 4, opt.o1 = 4, opt.e1 = 2, opt.o2 = 15, opt.e2 = 1;
	mwf_aln_summary_t s;
	mwf_cigar_summary(&opt, (int32_t)words.size(), w, tl, tl > 0 ? ts : nullptr, ql, ql > 0 ? qs : nullptr, &s);
	const int32_t got[12] = {s.score, s.t_len, s.q_len, s.n_eq, s.n_x, s.n_ins, s.n_del, s.n_ins_runs, s.n_del_runs, s.n_words, s.first_bad, s.flags};
	for (int k = 0; k < 12; ++k)
		if (got[k] != want[k]) {
			fprintf(stderr, "%s: field %d is %d, expected %d\n", name, k, got[k], want[k]);
			++failures;
		}
	free(ts), free(qs), free(w);
}

int main()
{
	static_assert(sizeof(mwf_aln_summary_t) == 48, "mwf_aln_summary_t is twelve int32");
	const char *T = "ACGTTGCAACGCATGGATCCTACGATCGGATTAC", *Q = "ACGTTGCAACTGGATCCTATTCGATCGGATTAC";
	const int32_t tl = 34, ql = 33;
	const uint32_t EQ = 7, X = 8, I = 1, D = 2, BIG = 0x0fffffffu;
	const std::vector<uint32_t> W = {10u << 4 | EQ, 1u << 4 | X, 3u << 4 | D, 8u << 4 | EQ, 2u << 4 | I, 12u << 4 | EQ};
	auto with = [&](size_t k, uint32_t word) { std::vector<uint32_t> v = W; v[k] = word; return v; };
	check("clean", W, tl, T, ql, Q, {22, 34, 33, 30, 1, 2, 3, 1, 1, 6, -1, 1});
	check("op15", with(3, 8u << 4 | 15u), tl, T, ql, Q, {22, 26, 25, 22, 1, 2, 3, 1, 1, 6, 3, 1});
	check("eq_plus7", with(5, 19u << 4 | EQ), tl, T, ql, Q, {22, 41, 40, 37, 1, 2, 3, 1, 1, 6, 5, 1});
	check("eq_plus7_mid", with(0, 17u << 4 | EQ), tl, T, ql, Q, {22, 41, 40, 37, 1, 2, 3, 1, 1, 6, 0, 1});
	check("dropped", std::vector<uint32_t>(W.begin(), W.end() - 1), tl, T, ql, Q, {22, 22, 21, 18, 1, 2, 3, 1, 1, 5, 5, 1});
	check("huge", with(2, BIG << 4 | D), tl, T, ql, Q, {(int32_t)(4 + 15 + BIG + 8), (int32_t)(31 + BIG), 33, 30, 1, 2, (int32_t)BIG, 1, 1, 6, 2, 1});
	check("wrap", std::vector<uint32_t>(20, BIG << 4 | EQ), tl, T, ql, Q, {0, 0x3FFFFFEC, 0x3FFFFFEC, 0x3FFFFFEC, 0, 0, 0, 0, 0, 20, 0, 1});
	check("no_words", {}, tl, T, ql, Q, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1});
	check("empty_pair", {}, 0, T, 0, Q, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 1});
	// words that start beyond the ends: an X and an = far outside, an insertion against an empty query
	check("beyond", {BIG << 4 | D, 5u << 4 | X, 5u << 4 | EQ}, tl, T, ql, Q, {(int32_t)(15 + BIG + 20), (int32_t)(BIG + 10), 10, 5, 5, 0, (int32_t)BIG, 0, 1, 3, 0, 1});
	check("ins_vs_empty", {3u << 4 | I}, 0, T, 0, Q, {10, 0, 3, 0, 0, 3, 0, 1, 0, 1, 0, 1});
	if (failures) return 1;
	printf("cigar_summary_sanitize OK\n");
	return 0;
}
