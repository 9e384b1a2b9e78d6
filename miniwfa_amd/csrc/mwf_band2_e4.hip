// mwf_band2_e4.hip — the packed band kernel (mwf_band2_kernel.h) for gap extensions (4, 1): the same template with E1 / F1 histories of 4 penalties and an edge
// table of 5 ages.  A unit of its own so that it compiles beside mwf_band2.hip; it defines launch_band2_e4 and band2_occupancy_e4 and nothing else.
// Geometries: 64 ... 512 x 3, 512 x 4 and the 1024 x 5 span geometry on 2-bit copies, 768 x 2 byte-wise, each with and
// without traceback — never folded, no copies on biased offsets.  (4, 2) missed its gate and is not built.
// Registers and scratch: profiles/band_deep/band2_deep_registers.txt.
#include "mwf_band2_dispatch.h"

namespace mwf {

namespace {
struct Unit {
	using Sets = E4Sets; // (4,1) alone
	using BiasedSets = NoSets;
	static constexpr unsigned geos = kGeoPlain;
};
} // namespace

int launch_band2_e4(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	if (g.packed == 2) return -1; // (no copies of the 512-thread geometry on biased offsets in this unit: mwf_band2_bi_deep.hip)
	return band2_unit_launch<Unit>(a, grid, g, stream);
}

int band2_occupancy_e4(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (g.packed == 2) return 0;
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
