// The retry layer's route table and re-route rule (miniwfa_amd/csrc/mwf_plan_retry.h) stand-alone, for tests/test_plan_retry_cpu.py: built with
// -fsanitize=address,undefined, nothing loaded into python.
//   plan_retry table     one line per route, in launch order: number name launch want_kind slots use_forecast geom span_if_all copy nib_split ring16_allowed fewer
//   plan_retry reroute   reads lines "band_span seq2bit force_kind block tb_budget_mb coop_tb_mult step span_window tb_slots can_grow  tl ql status kind class flags n_iter"
//                        and prints "route step0 class flags wide_needs_four grow_coop warn asked" per line (asked: the rule asked whether the arena can grow)
#include <cstdio>
#include <cstring>
#include "mwf_plan_retry.h"

using namespace mwf;
using namespace mwf::host;

static int print_table()
{
	for (int r = 0; r < kNumRoutes; ++r) {
		const RouteRow &T = kRouteTable[r];
		printf("%d %s %d %d %d %d %d %d %d %d %d %d\n", r, T.name, (int)T.launch, (int)T.want_kind, (int)T.slots, (int)T.use_forecast, (int)T.geom, (int)T.span_if_all, (int)T.copy, (int)T.nib_split,
		       (int)T.ring16_allowed, (int)takes_fewer_slots((Route)r));
	}
	return 0;
}

struct Grow { bool answer; int asked; };

static int reroute_lines()
{
	RetryRule R;
	PairState p;
	long long tb_budget_mb, coop_tb_mult, span_window, tl, ql, n_iter;
	int step, can_grow, status, kind, cls, flags;
	while (scanf("%d %d %d %d %lld %lld %d %lld %d %d %lld %lld %d %d %d %d %lld", &R.band_span, &R.seq2bit, &R.force_kind, &R.block, &tb_budget_mb, &coop_tb_mult, &step, &span_window, &R.tb_slots, &can_grow,
	             &tl, &ql, &status, &kind, &cls, &flags, &n_iter) == 17) {
		Grow grow{can_grow != 0, 0};
		R.tb_budget_mb = tb_budget_mb, R.coop_tb_mult = coop_tb_mult, R.step = step, R.span_window = span_window;
		R.coop_can_grow = [](void *ctx) { Grow *w = (Grow*)ctx; ++w->asked; return w->answer; }, R.ctx = &grow;
		p.tl = tl, p.ql = ql, p.status = status, p.kind = (int8_t)kind, p.h_class = (int8_t)cls, p.h_flags = (int8_t)flags, p.n_iter = n_iter;
		const RouteDecision d = reroute_pair(R, p);
		printf("%d %d %d %d %d %d %d %d\n", (int)d.route, d.step0, (int)d.h_class, (int)d.h_flags, (int)d.wide_needs_four, (int)d.grow_coop, (int)d.warn, grow.asked);
	}
	return feof(stdin) ? 0 : 2; // (a line that does not parse)
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "table")) return print_table();
	if (argc == 2 && !strcmp(argv[1], "reroute")) return reroute_lines();
	fprintf(stderr, "usage: plan_retry table | reroute < lines\n");
	return 1;
}
