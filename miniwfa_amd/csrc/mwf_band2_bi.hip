// mwf_band2_bi.hip — the packed band kernel's (mwf_band2_kernel.h) five- and six-slot copies of the 512-thread geometry on biased offsets (class 14 of mwf_plan.cpp:
// pairs of up to ~21 kb that plain 16-bit offsets cannot be promised to hold, two workgroups per CU) for gap extensions (2, 2) — main.c's -a preset, folded and
// not — and (1, 1).  A unit of its own so that it compiles beside mwf_band2.hip; it defines launch_band2_bi1 and band2_occupancy_bi1 and nothing else.
// Registers and scratch: profiles/band_biased/band2_biased_registers.txt.
#include "mwf_band2_dispatch.h"

namespace mwf {

namespace {
struct Unit {
	using Sets = BiSets;
	using BiasedSets = BiSets;
	static constexpr unsigned geos = kGeoBiased;
};
} // namespace

int launch_band2_bi1(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	if (g.packed != 2) return -1; // (this unit holds the copies on biased offsets and nothing else)
	return band2_unit_launch<Unit>(a, grid, g, stream);
}

int band2_occupancy_bi1(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (g.packed != 2) return 0;
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
