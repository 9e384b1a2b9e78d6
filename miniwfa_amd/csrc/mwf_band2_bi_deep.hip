// mwf_band2_bi_deep.hip — the packed band kernel's (mwf_band2_kernel.h) five- and six-slot copies of the 512-thread geometry on biased offsets (class 14 of
// mwf_plan.cpp) for gap extensions (3, 1), (3, 2) and (4, 1), never folded.  A unit of its own so that it compiles beside mwf_band2.hip; it defines
// launch_band2_bi2 and band2_occupancy_bi2 and nothing else.  Registers and scratch: profiles/band_biased/band2_biased_registers.txt.
#include "mwf_band2_dispatch.h"

namespace mwf {

namespace {
struct Unit {
	using Sets = BiDeepSets;
	using BiasedSets = BiDeepSets;
	static constexpr unsigned geos = kGeoBiased;
};
} // namespace

int launch_band2_bi2(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	if (g.packed != 2) return -1; // (this unit holds the copies on biased offsets and nothing else)
	return band2_unit_launch<Unit>(a, grid, g, stream);
}

int band2_occupancy_bi2(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (g.packed != 2) return 0;
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
