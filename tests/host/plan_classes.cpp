// The plan layer's class table and per-pair rule (miniwfa_amd/csrc/mwf_plan_classes.h) stand-alone, for tests/test_plan_classes_cpu.py: built with
// -fsanitize=address,undefined, nothing loaded into python.
//   plan_classes table          one line per class: number name geom copy want_kind fallback by_work wide retry_slot; then "order" and the run order
//   plan_classes classify       reads lines "x o1 e1 o2 e2  band2 lane biased512  biased_chunks span_chunks  wide_slots band_span lane_max_len  tl ql" (the five after
//                               the penalties: what band2_supported, lane_supported, band2_biased512_supported answer for the set, and band2_biased512_chunks and
//                               band2_span_chunks) and prints "class fallback" per line
// The other tunables are the engine's defaults under "div_aware" 0 and "mid_max_pairs" 0 (the mid kernel's LDS size lives in a .hip unit), every pair plain A/C/G/T.
#include <cstdio>
#include <cstring>
#include "mwf_internal.h"
#include "mwf_plan_classes.h"

using namespace mwf;
using namespace mwf::host;

static int print_table()
{
	for (int c = 0; c < kNumClasses; ++c) {
		const ClassRow &T = row(c);
		printf("%d %s %d %d %d %d %d %d %d\n", c, T.name, (int)T.geom, (int)T.copy, (int)T.want_kind, (int)T.fallback, (int)T.by_work, (int)T.wide, (int)T.retry_slot);
	}
	printf("order");
	for (PairClass c : kRunOrder) printf(" %d", (int)c);
	printf("\n");
	return 0;
}

static int classify_lines()
{
	int x, o1, e1, o2, e2, band2, lane, biased, biased_chunks, span_chunks, wide_slots, band_span, lane_max_len;
	long long tl, ql;
	while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld", &x, &o1, &e1, &o2, &e2, &band2, &lane, &biased, &biased_chunks, &span_chunks, &wide_slots, &band_span, &lane_max_len, &tl, &ql) == 15) {
		ClassRule R;
		Penalty &p = R.pen;
		p.x = x, p.o1 = o1, p.o2 = o2, p.e1 = e1, p.e2 = e2, p.oe1 = o1 + e1, p.oe2 = o2 + e2; // (mwf_plan.cpp make_penalty)
		p.nH = std::max(x, std::max(p.oe1, p.oe2)) + 1, p.n1 = e1 + 1, p.n2 = e2 + 1;
		R.band2_ok = band2 != 0, R.lane_ok = lane != 0, R.biased512_ok = biased != 0;
		R.biased512_chunks = biased_chunks, R.span_chunks = span_chunks;
		R.wide_slots = wide_slots, R.band_span = band_span, R.lane_max_len = lane_max_len;
		R.div_aware = false, R.mid_cap = 0;
		R.finish();
		const PairPlan pp = classify_pair(R, tl, ql, true, -1, false);
		printf("%d %d\n", (int)pp.cls, (int)pp.fallback);
	}
	return feof(stdin) ? 0 : 2; // (a line that does not parse)
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "table")) return print_table();
	if (argc == 2 && !strcmp(argv[1], "classify")) return classify_lines();
	fprintf(stderr, "usage: plan_classes table | classify < lines\n");
	return 1;
}
