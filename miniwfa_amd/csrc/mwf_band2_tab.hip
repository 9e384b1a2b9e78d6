// mwf_band2_tab.hip — the packed band kernel's table form: the first probe of the match extension reads per-position 8-mer tables in LDS (mwf_band2_kernel.h: kTabProbe).
// 512 threads x 3 and x 4 chunk slots, gap extensions (2,1), 2-bit copies, folded, with and without traceback: four kernels, wfa_band2_tab_kernel.
// This unit defines launch_band2_tab, band2_occupancy_tab and band2_tab_supported and nothing else.
#define MWF_BAND2_FORM 1
#include "mwf_band2_dispatch.h"

namespace mwf {

namespace {
struct Unit {
	using Sets = TabSets;
	using BiasedSets = NoSets;
	static constexpr unsigned geos = kGeoWide;
};
// (the host asks for nothing else: choose_kernel, BandGeom::tab)
bool tab_geom_ok(const Penalty &p, const BandGeom &g)
{
	return g.packed == 1 && g.block == 512 && g.seq2 != 0 && g.tab > 0 && g.tab % 16 == 0 && g.lds_bytes > g.tab && band2_tab_supported(p, true);
}
} // namespace

// the one statement of when the table form applies: its kernels exist folded only (mwf_band2_kernel.h: kFoldedOnly)
bool band2_tab_supported(const Penalty &p, bool band_fold) { return has_pen_set(Unit::Sets{}, p.e1, p.e2) && band2_folds(p, band_fold); }

int launch_band2_tab(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	if (!tab_geom_ok(a.pen, g) || !a.band_fold) return -1;
	return band2_unit_launch<Unit>(a, grid, g, stream); // (g.tab becomes BatchArgs::band_lds_tab in launch_one)
}

int band2_occupancy_tab(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (!tab_geom_ok(p, g)) return 0;
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
