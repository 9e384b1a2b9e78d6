// Stand-alone driver for mwf_alphabet_class16 (csrc/mwf_dbg.cpp).  tests/test_alpha16_cpu.py compiles it together with mwf_dbg.cpp under
// -fsanitize=address,undefined and runs it as a child process: the sequences live in heap blocks of exactly their length, so a read outside
// ts[0,tl) / qs[0,ql) is an AddressSanitizer report, and the classes and maps are checked as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "miniwfa.h"

static int failures = 0;

// want_syms: for classes 1 and 3 the distinct bytes in ascending order (class 1: they map to A, C, G, T; class 3: to MWF_ALPHA16_TAG | 0, 1, ...)
static void check(const char *name, const std::string &t, const std::string &q, int32_t want_cls, const std::string &want_syms)
{
	const int32_t tl = (int32_t)t.size(), ql = (int32_t)q.size();
	// exact-size heap copies: no terminator, no slack
	char *ts = (char*)malloc(tl > 0 ? tl : 1), *qs = (char*)malloc(ql > 0 ? ql : 1);
	if (tl > 0) memcpy(ts, t.data(), tl);
	if (ql > 0) memcpy(qs, q.data(), ql);
	uint8_t *map = (uint8_t*)malloc(256);
	memset(map, 0xee, 256);
	const int32_t cls = mwf_alphabet_class16(tl, tl > 0 ? ts : nullptr, ql, ql > 0 ? qs : nullptr, map);
	if (cls != want_cls) fprintf(stderr, "%s: class %d, expected %d\n", name, cls, want_cls), ++failures;
	uint8_t want[256];
	memset(want, 0, 256);
	if (want_cls == 1)
		for (size_t k = 0; k < want_syms.size(); ++k) want[(uint8_t)want_syms[k]] = (uint8_t)"ACGT"[k];
	if (want_cls == 3)
		for (size_t k = 0; k < want_syms.size(); ++k) want[(uint8_t)want_syms[k]] = (uint8_t)(MWF_ALPHA16_TAG | k);
	if (memcmp(map, want, 256) != 0) fprintf(stderr, "%s: map differs\n", name), ++failures;
	if (mwf_alphabet_class16(tl, tl > 0 ? ts : nullptr, ql, ql > 0 ? qs : nullptr, nullptr) != want_cls) fprintf(stderr, "%s: class without a map differs\n", name), ++failures;
	// classes 0 and 1: class and map of mwf_alphabet_class; 2 and 3: its class 2
	uint8_t *map4 = (uint8_t*)malloc(256);
	const int32_t cls4 = mwf_alphabet_class(tl, tl > 0 ? ts : nullptr, ql, ql > 0 ? qs : nullptr, map4);
	if (cls4 != (want_cls == 3 ? 2 : want_cls)) fprintf(stderr, "%s: mwf_alphabet_class gives %d\n", name, cls4), ++failures;
	if (want_cls <= 1 && memcmp(map, map4, 256) != 0) fprintf(stderr, "%s: map differs from mwf_alphabet_class's\n", name), ++failures;
	free(ts), free(qs), free(map), free(map4);
}

int main()
{
	std::string T = "ACGTTGCAACGCATGGATCCTACGATCGGATTAC", Q = "ACGTTGCAACTGGATCCTATTCGATCGGATTAC";
	auto lower = [](std::string s) { for (char &c : s) c = (char)(c | 0x20); return s; };
	std::string s16, s17;
	for (int k = 0; k < 17; ++k) (k < 16 ? s16 : s17) += (char)(100 + k);
	s17 = s16 + s17;
	check("plain", T, Q, 0, "");
	check("lower", lower(T), lower(Q), 1, "acgt");
	check("one", std::string(40, 'x'), std::string(3, 'x'), 1, "x");
	check("four_bytes", std::string("\x00\x7f\x80\xff\x80", 5), std::string("\xff\x00", 2), 1, std::string("\x00\x7f\x80\xff", 4));
	check("five", T + "N", Q, 3, "ACGNT");
	check("fifth_last_q", T, Q.substr(0, Q.size() - 1) + "N", 3, "ACGNT");
	check("mixed_case", T, lower(Q), 3, "ACGTacgt");
	check("bytes_00_ff", std::string("\x00\xff", 2) + T, Q + "N", 3, std::string("\x00", 1) + "ACGNT" + "\xff");
	check("sixteen", s16, s16.substr(8), 3, s16);
	check("sixteen_split", s16.substr(0, 9), s16.substr(9), 3, s16);
	check("seventeen", s17, Q, 2, "");
	check("seventeenth_last_q", s16, s16.substr(3) + (char)116, 2, "");
	check("both_empty", "", "", 0, "");
	check("empty_t", "", Q + "N", 3, "ACGNT");
	check("empty_q", T + "RY", "", 3, "ACGRTY");
	// long enough for several blocks of the scan; the fifth and the seventeenth symbol in the very last byte of the query
	std::string LT, LQ;
	for (int k = 0; k < 200; ++k) LT += T, LQ += Q;
	check("long_fifth_last", LT, LQ.substr(0, LQ.size() - 1) + "n", 3, "ACGTn");
	check("long_seventeenth_last", LT + s16.substr(0, 12), LQ + (char)120, 2, "");
	if (failures) return 1;
	printf("alphabet_class16_sanitize OK\n");
	return 0;
}
