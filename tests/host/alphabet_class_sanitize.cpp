// Stand-alone driver for mwf_alphabet_class (csrc/mwf_dbg.cpp).  tests/test_alpha_remap_cpu.py compiles it together with mwf_dbg.cpp under
// -fsanitize=address,undefined and runs it as a child process: the sequences live in heap blocks of exactly their length, so a read outside
// ts[0,tl) / qs[0,ql) is an AddressSanitizer report, and the classes and maps are checked as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "miniwfa.h"

static int failures = 0;

// want_syms: for class 1 the distinct bytes in ascending order (they map to A, C, G, T in that order)
static void check(const char *name, const std::string &t, const std::string &q, int32_t want_cls, const std::string &want_syms)
{
	const int32_t tl = (int32_t)t.size(), ql = (int32_t)q.size();
	// exact-size heap copies: no terminator, no slack
	char *ts = (char*)malloc(tl > 0 ? tl : 1), *qs = (char*)malloc(ql > 0 ? ql : 1);
	if (tl > 0) memcpy(ts, t.data(), tl);
	if (ql > 0) memcpy(qs, q.data(), ql);
	uint8_t *map = (uint8_t*)malloc(256);
	memset(map, 0xee, 256);
	const int32_t cls = mwf_alphabet_class(tl, tl > 0 ? ts : nullptr, ql, ql > 0 ? qs : nullptr, map);
	if (cls != want_cls) fprintf(stderr, "%s: class %d, expected %d\n", name, cls, want_cls), ++failures;
	uint8_t want[256];
	memset(want, 0, 256);
	if (want_cls == 1)
		for (size_t k = 0; k < want_syms.size(); ++k) want[(uint8_t)want_syms[k]] = (uint8_t)"ACGT"[k];
	if (memcmp(map, want, 256) != 0) fprintf(stderr, "%s: map differs\n", name), ++failures;
	if (mwf_alphabet_class(tl, tl > 0 ? ts : nullptr, ql, ql > 0 ? qs : nullptr, nullptr) != want_cls) fprintf(stderr, "%s: class without a map differs\n", name), ++failures;
	free(ts), free(qs), free(map);
}

int main()
{
	std::string T = "ACGTTGCAACGCATGGATCCTACGATCGGATTAC", Q = "ACGTTGCAACTGGATCCTATTCGATCGGATTAC";
	auto lower = [](std::string s) { for (char &c : s) c = (char)(c | 0x20); return s; };
	auto swap_tu = [](std::string s) { for (char &c : s) if (c == 'T') c = 'U'; return s; };
	check("plain", T, Q, 0, "");
	check("lower", lower(T), lower(Q), 1, "acgt");
	check("acgu", swap_tu(T), swap_tu(Q), 1, "ACGU");
	check("one", std::string(40, 'x'), std::string(3, 'x'), 1, "x");
	check("two", std::string("\0\1\1\0\0", 5), std::string("\1\1\0", 3), 1, std::string("\0\1", 2));
	check("four_bytes", std::string("\x00\x7f\x80\xff\x80", 5), std::string("\xff\x00", 2), 1, std::string("\x00\x7f\x80\xff", 4));
	check("five", T + "N", Q, 2, "");
	check("fifth_last_q", T, Q.substr(0, Q.size() - 1) + "N", 2, "");
	check("fifth_in_t", T.substr(0, 9) + "N" + T.substr(10), Q, 2, "");
	check("mixed_case", T, lower(Q), 2, "");
	check("both_empty", "", "", 0, "");
	check("empty_t", "", lower(Q), 1, "acgt");
	check("empty_q", swap_tu(T), "", 1, "ACGU");
	// long enough for several blocks of the scan, the fifth symbol in the very last byte of the query
	std::string LT, LQ;
	for (int k = 0; k < 200; ++k) LT += lower(T), LQ += lower(Q);
	check("long_lower", LT, LQ, 1, "acgt");
	check("long_fifth_last", LT, LQ.substr(0, LQ.size() - 1) + "n", 2, "");
	if (failures) return 1;
	printf("alphabet_class_sanitize OK\n");
	return 0;
}
