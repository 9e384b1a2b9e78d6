// mwf_band2.hip — the packed band kernel's main unit: the fast path for batches of pairs whose offsets fit 16 bits (targets below ~32 kb: BASELINE configs[2],
// read-length batches, chain-mode gap fills).  The kernel is mwf_band2_kernel.h; mwf_band2_dispatch.h says which unit holds which instantiations.  This one holds
// gap extensions (2,1), (2,2) and (1,1) on every geometry — of the 512 x 5 / 512 x 6 copies on biased offsets (2,1)'s alone — and routes every other launch
// of the family to the unit that holds it: launch_band2, band2_kernel_occupancy, the "supported" predicates and the two chunk counts the planner sizes by.
#include "mwf_band2_dispatch.h"

namespace mwf {

// Three constants of the kernel that the tests' restatement of its rules reads from the text of this file (tests/band_matrix.py, BAND2_SRC: the fold's lag bound,
// the two margins of the biased offsets) — so the test suite of the revision before the template moved to mwf_band2_kernel.h still imports against this
// library.  The definitions are the header's; the compiler holds this statement of them equal, so it cannot become a second source.
namespace band2_text {
constexpr int kFoldMaxLag = 8;
constexpr int32_t kBiasOver = 1500, kBiasMargin = 600;
static_assert(kFoldMaxLag == mwf::kFoldMaxLag && kBiasOver == mwf::kBiasOver && kBiasMargin == mwf::kBiasMargin, "mwf_band2.hip: the copy of the kernel's constants is out of date");
} // namespace band2_text

namespace {
struct Unit {
	using Sets = MainSets;
	using BiasedSets = MainBiasedSets;
	static constexpr unsigned geos = kGeoBiased | kGeoPlain;
};
} // namespace

// the packed kernel: (e1,e2) instantiated, sequences fit LDS (the host checks), every H lag >= 1
bool band2_supported(const Penalty &p)
{
	return (has_pen_set(MainSets{}, p.e1, p.e2) || has_pen_set(E3Sets{}, p.e1, p.e2) || has_pen_set(E4Sets{}, p.e1, p.e2)) && p.nH <= kMaxRing; // (window table in LDS; rows read as dead up to 256 columns beyond their window)
}

// (the sets whose copies on biased offsets are built: (2,1) in this unit, the others in mwf_band2_bi.hip / mwf_band2_bi_deep.hip; (4,2) is not on this kernel at all)
bool band2_biased512_supported(const Penalty &p)
{
	return has_pen_set(MainBiasedSets{}, p.e1, p.e2) || has_pen_set(BiSets{}, p.e1, p.e2) || has_pen_set(BiDeepSets{}, p.e1, p.e2);
}

int band2_span_chunks() { return kSpanT / 64 * kSpanK; }
int band2_biased512_chunks() { return 8 * kW4K; }

int launch_band2(const BatchArgs &a, int grid, const BandGeom &g0, void *stream)
{
	const int e1 = a.pen.e1;
	BandGeom g = g0;
	if (g.nib) return launch_band2_nib(a, grid, g, stream); // the 4-bit form (mwf_band2_nib.hip); no other form reads its copies
	if (g.tab > 0) { // the table form; a geometry it refuses runs the plain form on the same sequence copies
		if (g.fold2) { // ... with the second gap piece folded where the plan asked for it; what that unit refuses (a CIGAR launch) is the table form's
			const int rc2 = launch_band2_tab2(a, grid, g, stream);
			if (rc2 != -1) return rc2;
		}
		const int rc = launch_band2_tab(a, grid, g, stream);
		if (rc != -1) return rc;
		g.lds_bytes -= g.tab, g.tab = 0;
	}
	if (g.packed == 2 && !has_pen_set(MainBiasedSets{}, e1, a.pen.e2)) return e1 <= 2 ? launch_band2_bi1(a, grid, g, stream) : launch_band2_bi2(a, grid, g, stream);
	if (e1 == 3) return launch_band2_e3(a, grid, g, stream);
	if (e1 == 4) return launch_band2_e4(a, grid, g, stream);
	return band2_unit_launch<Unit>(a, grid, g, stream);
}

int band2_kernel_occupancy(const Penalty &p, const BandGeom &g, bool cigar)
{
	if (g.nib) return band2_occupancy_nib(p, g, cigar);
	if (g.tab > 0 && g.fold2 && !cigar) return band2_occupancy_tab2(p, g, cigar);
	if (g.tab > 0) return band2_occupancy_tab(p, g, cigar); // (0 for a geometry the table form refuses: choose_kernel then keeps the plain form)
	if (g.packed == 2 && !has_pen_set(MainBiasedSets{}, p.e1, p.e2)) return p.e1 <= 2 ? band2_occupancy_bi1(p, g, cigar) : band2_occupancy_bi2(p, g, cigar);
	if (p.e1 == 3) return band2_occupancy_e3(p, g, cigar);
	if (p.e1 == 4) return band2_occupancy_e4(p, g, cigar);
	return band2_unit_occupancy<Unit>(p, g, cigar);
}

} // namespace mwf
