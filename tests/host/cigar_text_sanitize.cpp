// Stand-alone driver for mwf_cigar_text (csrc/mwf_dbg.cpp): the hand pair's six products and the unrenderable word sets.
// tests/test_cigar_text_cpu.py compiles it together with mwf_dbg.cpp under -fsanitize=address,undefined and runs it as a child process: the
// sequences and dst live in heap blocks of exactly their size, so a read outside ts[0,tl) / qs[0,ql) or a write beyond cap is an
// AddressSanitizer report.  The pair is that of tests/cigar_ops_ref.py (HAND_T, HAND_Q): CIGAR 10= 1X 3D 8= 2I 12=; the unrenderable sets are
// what cigar_ops_ref.malformed_variants makes of it (op15, eq_plus7, dropped, huge) plus a word of length 0 and kind 6.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "miniwfa.h"

static int failures = 0;

static void fail(const char *name, int kind, const char *what)
{
	fprintf(stderr, "%s, kind %d: %s\n", name, kind, what);
	++failures;
}

// want == nullptr: the words are not renderable (-1, dst untouched)
static void check(const char *name, int kind, const std::vector<uint32_t> &words, int32_t tl, const char *t, int32_t ql, const char *q, const char *want)
{
	// exact-size heap copies: no terminator, no slack
	char *ts = (char*)malloc(tl > 0 ? tl : 1), *qs = (char*)malloc(ql > 0 ? ql : 1);
	if (tl > 0) memcpy(ts, t, tl);
	if (ql > 0) memcpy(qs, q, ql);
	uint32_t *w = (uint32_t*)malloc(words.empty() ? 4 : words.size() * 4);
	if (!words.empty()) memcpy(w, words.data(), words.size() * 4);
	const char *tp = tl > 0 ? ts : nullptr, *qp = ql > 0 ? qs : nullptr;
	const int32_t n = (int32_t)words.size();
	const int64_t len = mwf_cigar_text(kind, n, w, tl, tp, ql, qp, nullptr, 0);
	if (!want) {
		if (len != -1) fail(name, kind, "expected -1");
		char *dst = (char*)malloc(64);
		memset(dst, '#', 64);
		if (mwf_cigar_text(kind, n, w, tl, tp, ql, qp, dst, 64) != -1) fail(name, kind, "expected -1 with a buffer");
		for (int k = 0; k < 64; ++k) if (dst[k] != '#') { fail(name, kind, "dst was written"); break; }
		free(dst);
	} else {
		const int64_t wl = (int64_t)strlen(want);
		if (len != wl) fail(name, kind, "wrong length");
		else for (int64_t cap : {wl, wl - 1, wl / 2}) { // dst is a block of exactly cap bytes
			if (cap < 0) continue;
			char *dst = (char*)malloc(cap > 0 ? cap : 1);
			if (mwf_cigar_text(kind, n, w, tl, tp, ql, qp, cap > 0 ? dst : nullptr, cap) != wl) fail(name, kind, "the return depends on cap");
			if (cap > 0 && memcmp(dst, want, (size_t)cap)) fail(name, kind, "wrong text");
			free(dst);
		}
	}
	free(ts), free(qs), free(w);
}

int main()
{
	const char *T = "ACGTTGCAACGCATGGATCCTACGATCGGATTAC", *Q = "ACGTTGCAACTGGATCCTATTCGATCGGATTAC";
	const int32_t tl = 34, ql = 33;
	const uint32_t EQ = 7, X = 8, I = 1, D = 2, BIG = 0x0fffffffu;
	const std::vector<uint32_t> W = {10u << 4 | EQ, 1u << 4 | X, 3u << 4 | D, 8u << 4 | EQ, 2u << 4 | I, 12u << 4 | EQ};
	auto with = [&](size_t k, uint32_t word) { std::vector<uint32_t> v = W; v[k] = word; return v; };
	const char *hand[MWF_TXT_KINDS] = {"10=1X3D8=2I12=", "11M3D8M2I12M", ":10*gt-cat:8+tt:12", "10G0^CAT20",
	                                   "ACGTTGCAACGCATGGATCCTA--CGATCGGATTAC", "ACGTTGCAACT---GGATCCTATTCGATCGGATTAC"};
	for (int kind = 0; kind < MWF_TXT_KINDS; ++kind) {
		check("clean", kind, W, tl, T, ql, Q, hand[kind]);
		check("op15", kind, with(3, 8u << 4 | 15u), tl, T, ql, Q, nullptr);
		check("eq_plus7", kind, with(5, 19u << 4 | EQ), tl, T, ql, Q, nullptr);
		check("dropped", kind, std::vector<uint32_t>(W.begin(), W.end() - 1), tl, T, ql, Q, nullptr);
		check("huge", kind, with(3, BIG << 4 | EQ), tl, T, ql, Q, nullptr);
		check("huge_del", kind, with(2, BIG << 4 | D), tl, T, ql, Q, nullptr);
		check("len0", kind, {10u << 4 | EQ, 1u << 4 | X, 3u << 4 | D, 0u << 4 | I, 8u << 4 | EQ, 2u << 4 | I, 12u << 4 | EQ}, tl, T, ql, Q, nullptr);
		check("twenty_huge", kind, std::vector<uint32_t>(20, BIG << 4 | EQ), tl, T, ql, Q, nullptr);
		check("ins_vs_empty", kind, {3u << 4 | I}, 0, T, 0, Q, nullptr);
		check("no_words", kind, {}, tl, T, ql, Q, nullptr);
		check("empty_pair", kind, {}, 0, T, 0, Q, kind == MWF_TXT_MD ? "0" : "");
	}
	check("kind6", MWF_TXT_KINDS, W, tl, T, ql, Q, nullptr);
	check("kind-1", -1, W, tl, T, ql, Q, nullptr);
	if (failures) return 1;
	printf("cigar_text_sanitize OK\n");
	return 0;
}
