// mwf_band2_nib.hip — the packed band kernel's 4-bit form: pairs of 5 to 16 distinct bytes ("alpha16": an N, IUPAC codes, mixed case) on 512 x 3, 512 x 4 and the span
// geometry, gap extensions (2,1), with traceback (never folded) and score-only folded / unfolded: nine kernels.  The sequence copy, the first probe and the match walks
// hold 4 bits per base (mwf_band2_kernel.h: kNib), the kernel is wfa_band2_nib_kernel, and this unit defines launch_band2_nib, band2_occupancy_nib and
// band2_nib_supported and nothing else.
#define MWF_BAND2_FORM 2
#include "mwf_band2_dispatch.h"

namespace mwf {

namespace {
struct Unit {
	using Sets = NibSets;
	using BiasedSets = NoSets;
	static constexpr unsigned geos = kGeoWide | kGeoSpan;
};
bool nib_geom_ok(const Penalty &p, const BandGeom &g)
{
	return g.nib != 0 && g.packed == 1 && g.seq2 != 0 && g.tab == 0 && g.lds_bytes > 0 && (g.block == 512 || g.block == kSpanT) && band2_nib_supported(p);
}
} // namespace

bool band2_nib_supported(const Penalty &p) { return has_pen_set(Unit::Sets{}, p.e1, p.e2) && p.nH <= kMaxRing; }

int launch_band2_nib(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	if (!nib_geom_ok(a.pen, g)) return -1;
	return band2_unit_launch<Unit>(a, grid, g, stream);
}

int band2_occupancy_nib(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (!nib_geom_ok(p, g)) return 0;
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
