// mwf_dbg.cpp — CIGAR self-checks of the drop-in ABI (reference mwf-dbg.c:6-31).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "miniwfa.h"

namespace mwf {
namespace host {

// The alphabet class of one pair (mwf_alphabet_class below; the device twin is mwf_alphabet.hip) from the presence set of its bytes, 256 bits.
// sym (class 1 only): the distinct bytes in ascending order, the last one repeated up to four.  A pair of five or more distinct bytes is
// left as soon as a block of 1024 bytes has shown them.  Never reads outside t[0,tl) / q[0,ql).
int alphabet_scan(const uint8_t *t, size_t tl, const uint8_t *q, size_t ql, uint8_t sym[4])
{
	uint64_t m[4] = {0, 0, 0, 0};
	auto count = [&]() { return __builtin_popcountll(m[0]) + __builtin_popcountll(m[1]) + __builtin_popcountll(m[2]) + __builtin_popcountll(m[3]); };
	for (int side = 0; side < 2; ++side) {
		const uint8_t *p = side ? q : t;
		const size_t n = side ? ql : tl;
		for (size_t at = 0; at < n; at += 1024) {
			const size_t end = at + 1024 < n ? at + 1024 : n;
			for (size_t j = at; j < end; ++j) m[p[j] >> 6] |= 1ull << (p[j] & 63u);
			if (count() > 4) return 2;
		}
	}
	constexpr uint64_t acgt = (1ull << ('A' - 64)) | (1ull << ('C' - 64)) | (1ull << ('G' - 64)) | (1ull << ('T' - 64));
	if (!m[0] && !m[2] && !m[3] && !(m[1] & ~acgt)) return 0;
	int have = 0;
	uint8_t last = 0;
	for (int k = 0; k < 4; ++k)
		for (uint64_t w = m[k]; w; w &= w - 1) sym[have++] = last = (uint8_t)(64 * k + __builtin_ctzll(w));
	for (; have < 4; ++have) sym[have] = last;
	return 1;
}

// The class of mwf_alphabet_class16: as above with class 3, five to sixteen distinct bytes, between 1 and 2.  sym (classes 1 and 3): the distinct bytes in
// ascending order, the last one repeated — class 1 up to four with the other twelve 0 (alphabet_scan's four), class 3 up to sixteen.  A pair of seventeen or more is
// left as soon as a block of 1024 bytes has shown them.  Never reads outside t[0,tl) / q[0,ql).
int alphabet_scan16(const uint8_t *t, size_t tl, const uint8_t *q, size_t ql, uint8_t sym[16])
{
	uint64_t m[4] = {0, 0, 0, 0};
	auto count = [&]() { return __builtin_popcountll(m[0]) + __builtin_popcountll(m[1]) + __builtin_popcountll(m[2]) + __builtin_popcountll(m[3]); };
	memset(sym, 0, 16);
	for (int side = 0; side < 2; ++side) {
		const uint8_t *p = side ? q : t;
		const size_t n = side ? ql : tl;
		for (size_t at = 0; at < n; at += 1024) {
			const size_t end = at + 1024 < n ? at + 1024 : n;
			for (size_t j = at; j < end; ++j) m[p[j] >> 6] |= 1ull << (p[j] & 63u);
			if (count() > 16) return 2;
		}
	}
	constexpr uint64_t acgt = (1ull << ('A' - 64)) | (1ull << ('C' - 64)) | (1ull << ('G' - 64)) | (1ull << ('T' - 64));
	if (!m[0] && !m[2] && !m[3] && !(m[1] & ~acgt)) return 0;
	const int cls = count() <= 4 ? 1 : 3, fill = cls == 1 ? 4 : 16;
	int have = 0;
	uint8_t last = 0;
	for (int k = 0; k < 4; ++k)
		for (uint64_t w = m[k]; w; w &= w - 1) sym[have++] = last = (uint8_t)(64 * k + __builtin_ctzll(w));
	for (; have < fill; ++have) sym[have] = last;
	return cls;
}

} // namespace host
} // namespace mwf

extern "C" {

int32_t mwf_alphabet_class16(int32_t tl, const char *ts, int32_t ql, const char *qs, uint8_t map[256])
{
	uint8_t sym[16];
	const int cls = mwf::host::alphabet_scan16((const uint8_t*)ts, tl > 0 ? (size_t)tl : 0, (const uint8_t*)qs, ql > 0 ? (size_t)ql : 0, sym);
	if (map) {
		memset(map, 0, 256);
		if (cls == 1)
			for (int k = 0; k < 4; ++k)
				if (k == 0 || sym[k] != sym[k - 1]) map[sym[k]] = (uint8_t)"ACGT"[k];
		if (cls == 3)
			for (int k = 0; k < 16; ++k)
				if (k == 0 || sym[k] != sym[k - 1]) map[sym[k]] = (uint8_t)(MWF_ALPHA16_TAG | k);
	}
	return cls;
}

int32_t mwf_alphabet_class(int32_t tl, const char *ts, int32_t ql, const char *qs, uint8_t map[256])
{
	uint8_t sym[4] = {0, 0, 0, 0};
	const int cls = mwf::host::alphabet_scan((const uint8_t*)ts, tl > 0 ? (size_t)tl : 0, (const uint8_t*)qs, ql > 0 ? (size_t)ql : 0, sym);
	if (map) {
		memset(map, 0, 256);
		if (cls == 1)
			for (int k = 0; k < 4; ++k)
				if (k == 0 || sym[k] != sym[k - 1]) map[sym[k]] = (uint8_t)"ACGT"[k];
	}
	return cls;
}

// Penalty and consumed lengths implied by a CIGAR: '='/'X'/'M' advance both sequences, 'I' the
// query, 'D' the target; an indel run of length L costs min(o1+L*e1, o2+L*e2), 'X' costs x per base.
int32_t mwf_cigar2score(const mwf_opt_t *opt, int32_t n_cigar, const uint32_t *cigar, int32_t *tl, int32_t *ql)
{
	int64_t score = 0;
	int32_t on_t = 0, on_q = 0;
	for (int32_t i = 0; i < n_cigar; ++i) {
		const int32_t op = (int32_t)(cigar[i] & 0xf), len = (int32_t)(cigar[i] >> 4);
		switch (op) {
		case 1: case 2: {
			const int64_t p1 = opt->o1 + (int64_t)len * opt->e1, p2 = opt->o2 + (int64_t)len * opt->e2;
			score += p1 < p2 ? p1 : p2;
			if (op == 1) on_q += len; else on_t += len;
			break;
		}
		case 8: score += (int64_t)len * opt->x; /* fall through */
		case 0: case 7: on_t += len, on_q += len; break;
		default: break;
		}
	}
	if (tl) *tl = on_t;
	if (ql) *ql = on_q;
	return (int32_t)score;
}

// Lengths must match exactly (hard failure, like the reference's assert); a CIGAR that costs more
// than the reported penalty only draws a warning (reference mwf-dbg.c:30).
void mwf_assert_cigar(const mwf_opt_t *opt, int32_t n_cigar, const uint32_t *cigar, int32_t tl0, int32_t ql0, int32_t s0)
{
	int32_t tl = 0, ql = 0;
	const int32_t s = mwf_cigar2score(opt, n_cigar, cigar, &tl, &ql);
	if (tl != tl0 || ql != ql0) {
		fprintf(stderr, "[mwf_assert_cigar] CIGAR consumes (%d,%d) bases, sequences are (%d,%d)\n", tl, ql, tl0, ql0);
		abort();
	}
	if (s > s0) fprintf(stderr, "[mwf_assert_cigar] s0=%d, s=%d\n", s0, s);
}

// Host twin of the device summary (mwf_cigar_ops.hip): counters and score as mwf_cigar2score counts them (ops 1, 2, 7, 8 only), and
// first_bad by the rule in include/miniwfa.h.  Positions run in 64 bits; a base is only ever read at an index below its sequence's length.
void mwf_cigar_summary(const mwf_opt_t *opt, int32_t n_cigar, const uint32_t *cigar, int32_t tl, const char *ts, int32_t ql, const char *qs,
                       mwf_aln_summary_t *out)
{
	int64_t ti = 0, qj = 0; // (below 2^59 for any int32 count of 28-bit lengths)
	uint64_t score = 0; // (wraps, never overflows: only its low 32 bits are stored)
	int64_t n_eq = 0, n_x = 0, n_ins = 0, n_del = 0, ins_runs = 0, del_runs = 0;
	int32_t first_bad = -1;
	if (n_cigar < 0) n_cigar = 0;
	for (int32_t w = 0; w < n_cigar; ++w) {
		const int32_t op = (int32_t)(cigar[w] & 0xf);
		const int64_t len = (int64_t)(cigar[w] >> 4);
		bool bad = false;
		if (op == 1 || op == 2) {
			const int64_t p1 = opt->o1 + len * opt->e1, p2 = opt->o2 + len * opt->e2;
			score += (uint64_t)(p1 < p2 ? p1 : p2);
			if (op == 1) bad = qj + len > ql, n_ins += len, ++ins_runs, qj += len;
			else bad = ti + len > tl, n_del += len, ++del_runs, ti += len;
		} else if (op == 7 || op == 8) {
			bad = ti + len > tl || qj + len > ql;
			if (!bad && first_bad < 0) { // (the bases decide nothing once an earlier word is bad)
				const int64_t room_t = ti < tl ? tl - ti : 0, room_q = qj < ql ? ql - qj : 0;
				const int64_t m = len < room_t ? (len < room_q ? len : room_q) : (room_t < room_q ? room_t : room_q);
				for (int64_t k = 0; k < m && !bad; ++k) bad = (ts[ti + k] == qs[qj + k]) != (op == 7);
			}
			if (op == 8) score += (uint64_t)(len * opt->x), n_x += len;
			else n_eq += len;
			ti += len, qj += len;
		} else bad = true;
		if (bad && first_bad < 0) first_bad = w;
	}
	if (first_bad < 0 && (ti != tl || qj != ql)) first_bad = n_cigar;
	auto low32 = [](int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; };
	out->score = (int32_t)(uint32_t)score, out->t_len = low32(ti), out->q_len = low32(qj);
	out->n_eq = low32(n_eq), out->n_x = low32(n_x), out->n_ins = low32(n_ins), out->n_del = low32(n_del);
	out->n_ins_runs = low32(ins_runs), out->n_del_runs = low32(del_runs);
	out->n_words = n_cigar, out->first_bad = first_bad, out->flags = 1;
}

// Host twin of the device text (mwf_cigar_text.hip): the six products by the rule table in include/miniwfa.h.  The words are checked first
// (known op, length >= 1, inside both sequences, ending at (tl, ql)), so the rendering below only ever indexes ts[0,tl) / qs[0,ql).
namespace {
struct TextOut { // counts every byte, stores the first `cap` of them
	char *dst;
	int64_t cap, n;
	void put(char c) { if (n < cap) dst[n] = c; ++n; }
	void num(uint64_t v)
	{
		char buf[20];
		int k = 0;
		do buf[k++] = (char)('0' + v % 10), v /= 10; while (v);
		while (k) put(buf[--k]);
	}
};
inline char cs_lower(char b) { return b >= 'A' && b <= 'Z' ? (char)(b | 0x20) : b; }
}

int64_t mwf_cigar_text(int32_t kind, int32_t n_cigar, const uint32_t *cigar, int32_t tl, const char *ts, int32_t ql, const char *qs,
                       char *dst, int64_t cap)
{
	if (kind < 0 || kind >= MWF_TXT_KINDS || tl < 0 || ql < 0) return -1;
	if (n_cigar < 0) n_cigar = 0;
	if (cap < 0) cap = 0;
	int64_t ti = 0, qj = 0;
	for (int32_t w = 0; w < n_cigar; ++w) {
		const int32_t op = (int32_t)(cigar[w] & 0xf);
		const int64_t len = (int64_t)(cigar[w] >> 4);
		if ((op != 1 && op != 2 && op != 7 && op != 8) || len < 1) return -1;
		if (op != 1) ti += len;
		if (op != 2) qj += len;
		if (ti > tl || qj > ql) return -1;
	}
	if (ti != tl || qj != ql) return -1;
	TextOut o{dst, cap, 0};
	uint64_t run = 0; // SAM: the open M run; MD: the open count of bases under '='
	ti = qj = 0;
	for (int32_t w = 0; w < n_cigar; ++w) {
		const int32_t op = (int32_t)(cigar[w] & 0xf);
		const int64_t len = (int64_t)(cigar[w] >> 4);
		const bool both = op == 7 || op == 8;
		switch (kind) {
		case MWF_TXT_CIGAR: o.num((uint64_t)len), o.put("MIDNSHP=X"[op]); break;
		case MWF_TXT_SAM:
			if (both) {
				run += (uint64_t)len;
				if (w + 1 == n_cigar || ((cigar[w + 1] & 0xf) != 7 && (cigar[w + 1] & 0xf) != 8)) o.num(run), o.put('M'), run = 0;
			} else o.num((uint64_t)len), o.put(op == 1 ? 'I' : 'D');
			break;
		case MWF_TXT_CS:
			if (op == 7) o.put(':'), o.num((uint64_t)len);
			else if (op == 8) for (int64_t k = 0; k < len; ++k) o.put('*'), o.put(cs_lower(ts[ti + k])), o.put(cs_lower(qs[qj + k]));
			else {
				o.put(op == 1 ? '+' : '-');
				for (int64_t k = 0; k < len; ++k) o.put(cs_lower(op == 1 ? qs[qj + k] : ts[ti + k]));
			}
			break;
		case MWF_TXT_MD:
			if (op == 7) run += (uint64_t)len;
			else if (op == 8) for (int64_t k = 0; k < len; ++k) o.num(run), o.put(ts[ti + k]), run = 0;
			else if (op == 2) {
				o.num(run), o.put('^'), run = 0;
				for (int64_t k = 0; k < len; ++k) o.put(ts[ti + k]);
			}
			break;
		case MWF_TXT_ROW_T: for (int64_t k = 0; k < len; ++k) o.put(op == 1 ? '-' : ts[ti + k]); break;
		default:            for (int64_t k = 0; k < len; ++k) o.put(op == 2 ? '-' : qs[qj + k]); break;
		}
		if (op != 1) ti += len;
		if (op != 2) qj += len;
	}
	if (kind == MWF_TXT_MD) o.num(run);
	return o.n;
}

} // extern "C"
