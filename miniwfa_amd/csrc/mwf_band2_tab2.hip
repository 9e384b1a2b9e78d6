// mwf_band2_tab2.hip — the packed band kernel's table form with the SECOND gap piece folded one penalty ahead (mwf_band2_kernel.h: kFold2Form, band2_pass: kFold2):
// two row loads per chunk instead of three, and the recurrence waits for the row of lag x alone.
// 512 threads x 3 and x 4 chunk slots, gap extensions (2,1), 2-bit copies, folded, score-only: two kernels, wfa_band2_tab2_kernel.  With traceback, and for every
// penalty set band2_tab2_supported refuses, a launch keeps the table form (mwf_band2_tab.hip), whose LDS layout this form shares.
// This unit defines launch_band2_tab2, band2_occupancy_tab2 and band2_tab2_supported and nothing else.
#define MWF_BAND2_FORM 3
#include "mwf_band2_dispatch.h"

namespace mwf {

namespace {
struct Unit {
	using Sets = Tab2Sets;
	using BiasedSets = NoSets;
	static constexpr unsigned geos = kGeoWide;
};
// (the host asks for nothing else: choose_kernel, BandGeom::fold2)
bool tab2_geom_ok(const Penalty &p, const BandGeom &g)
{
	return g.packed == 1 && g.block == 512 && g.seq2 != 0 && g.tab > 0 && g.tab % 16 == 0 && g.lds_bytes > g.tab && g.fold2 != 0 && band2_tab2_supported(p);
}
} // namespace

// the one statement of when the second fold applies: where the table form does (its sets, o1 == x), e2 == 1 (the fold is one penalty ahead), o2 >= 3 (the row of lag
// o2 is now the nearest one a chunk loads: the youngest store may still cross the barrier, band2_pass: relaxed_stores) and o2 + e2 within the bound the ageing
// period is compiled for (kFold2MaxLag)
bool band2_tab2_supported(const Penalty &p)
{
	return has_pen_set(Unit::Sets{}, p.e1, p.e2) && band2_folds(p, true) && p.e2 == 1 && p.oe2 - p.e2 >= 3 && p.oe2 <= kFold2MaxLag;
}

int launch_band2_tab2(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	if (!tab2_geom_ok(a.pen, g) || !a.band_fold || a.want_cigar) return -1;
	return band2_unit_launch<Unit>(a, grid, g, stream);
}

int band2_occupancy_tab2(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (!tab2_geom_ok(p, g) || cigar) return 0;
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
