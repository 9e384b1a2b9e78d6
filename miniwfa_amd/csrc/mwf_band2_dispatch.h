// mwf_band2_dispatch.h — which instantiations of the packed band kernel (mwf_band2_kernel.h) exist, and how a launch finds its own: host code only.
//
// Seven units instantiate the template, so that they compile side by side; no kernel is in two of them:
//   mwf_band2.hip          (2,1), (2,2), (1,1) on every geometry; (2,1) alone on the 512 x 5 / 512 x 6 copies on biased offsets (class 14 of mwf_plan.cpp)
//   mwf_band2_e3.hip       (3,1), (3,2) — minimap2's asm5 / asm20-like sets — on every geometry but those copies, never folded
//   mwf_band2_e4.hip       (4,1), likewise
//   mwf_band2_bi.hip       the copies on biased offsets of (2,2), folded and not, and (1,1)
//   mwf_band2_bi_deep.hip  ... of (3,1), (3,2), (4,1)
//   mwf_band2_tab.hip      the table form of the first probe (wfa_band2_tab_kernel): (2,1) on 512 x 3 and 512 x 4, folded only
//   mwf_band2_nib.hip      the 4-bit form (wfa_band2_nib_kernel): (2,1) on 512 x 3, 512 x 4 and the span geometry
// and an eighth, added behind them:
//   mwf_band2_tab2.hip     the table form with the second gap piece folded too (wfa_band2_tab2_kernel): (2,1) on 512 x 3 and 512 x 4, folded, score-only
// (4,2) is not built: its 10 kb batches run on the span geometry (e2 == 2: the worst-case penalty does not fit plain 16-bit offsets), where 24 history registers
// per slot spill ~100 VGPRs, and gained 1.17 x / 1.13 x over the generic kernel — below what its code is worth.
//
// A unit is a struct of three facts (Band2Unit below): its penalty sets, those of them that have copies on biased offsets, and its geometry classes.  band2_select
// walks exactly those, so a unit's object holds its list and nothing else — an arm that can never run would still instantiate its kernels on the device —, and the
// "supported" predicates of mwf_internal.h are computed from the same lists.  An instantiation is added as one line in its unit's list, together with its entry in
// the matrix of the tests (tests/band_matrix.py and its siblings).
#pragma once
#include "mwf_band2_kernel.h"

namespace mwf {

namespace {

// ---- penalty sets: a type list of (E1, E2), tried one by one against the launch's (e1, e2)
template <int E1, int E2> struct PenSet { static constexpr int e1 = E1, e2 = E2; };
template <class... S> struct PenSets {};

template <class... S>
constexpr bool has_pen_set(PenSets<S...>, int e1, int e2) { return ((e1 == S::e1 && e2 == S::e2) || ...); }

// f(PenSet<E1, E2>{}) for the set of the list that equals (e1, e2); `none` when the list has no such set
// (the sets are tried, and with them instantiated, in the order of the list: the kernels lie in the code object in that order)
template <class R, class F>
R for_pen_set(PenSets<>, int, int, R none, F &&) { return none; }
template <class R, class F, class S0, class... S>
R for_pen_set(PenSets<S0, S...>, int e1, int e2, R none, F &&f)
{
	if (e1 == S0::e1 && e2 == S0::e2) return f(S0{});
	return for_pen_set(PenSets<S...>{}, e1, e2, none, f);
}

#ifdef MWF_BAND_DEV // development builds (timing probes, profiles/asm_band2.sh): the main unit holds (2,1) alone, and no unit the 64 / 128 / 256-thread geometries
// (band2_supported then says so too — false for (2,2) and (1,1), which run on the generic kernel — where it used to say true and the launch came back -1)
using MainSets = PenSets<PenSet<2, 1>>;
#else
using MainSets = PenSets<PenSet<2, 1>, PenSet<2, 2>, PenSet<1, 1>>;
#endif
using E3Sets = PenSets<PenSet<3, 1>, PenSet<3, 2>>;
using E4Sets = PenSets<PenSet<4, 1>>;
using MainBiasedSets = PenSets<PenSet<2, 1>>; // (2,1)'s copies on biased offsets stay in the main unit
using BiSets = PenSets<PenSet<2, 2>, PenSet<1, 1>>;
using BiDeepSets = PenSets<PenSet<3, 1>, PenSet<3, 2>, PenSet<4, 1>>;
using TabSets = PenSets<PenSet<2, 1>>;
using NibSets = PenSets<PenSet<2, 1>>;
using Tab2Sets = PenSets<PenSet<2, 1>>;
using NoSets = PenSets<>;

// ---- geometries: a BandGeom names its compile-time geometry (T threads, K chunk slots per wave, BI4 biased offsets) by block, span and packed
template <int T_, int K_, bool BI4_ = false> struct Geo { static constexpr int T = T_, K = K_; static constexpr bool BI4 = BI4_; };

inline bool geom_four_slots(const BandGeom &g) { return g.block == 512 && g.span > 512 / 64 * kWideK * kChunk; } // 32 chunks: windows of up to 7872 columns
inline bool geom_five_slots(const BandGeom &g) { return geom_four_slots(g) && g.packed == 2; }                     // ... on biased offsets (pairs of up to ~18 kb)
inline bool geom_six_slots(const BandGeom &g) { return g.block == 512 && g.span > 8 * kW4K * kChunk && g.packed == 2; } // ... (pairs of up to ~21 kb)

enum : unsigned {
	kGeoBiased = 1, // 512 x 5, 512 x 6 on biased offsets
	kGeoWide = 2,   // 512 x 3, 512 x 4
	kGeoBytes = 4,  // 768 x 2, byte-wise sequence copies
	kGeoSpan = 8,   // 1024 x 5
#ifdef MWF_BAND_DEV
	kGeoSmall = 0,
#else
	kGeoSmall = 16, // 256, 128, 64 threads x 3
#endif
	kGeoPlain = kGeoWide | kGeoBytes | kGeoSpan | kGeoSmall
};

// f(Geo<T, K, BI4>{}) for the geometry `g` asks for, among the classes in GEOS; `none` when it is in none of them
template <unsigned GEOS, class R, class F>
R for_band_geom(const BandGeom &g, R none, F &&f)
{
	if constexpr ((GEOS & kGeoBiased) != 0) {
		if (geom_six_slots(g)) return f(Geo<512, kW4K + 1, true>{});
		if (geom_five_slots(g)) return f(Geo<512, kW4K, true>{});
	}
	if constexpr ((GEOS & kGeoWide) != 0) {
		if (geom_four_slots(g)) return f(Geo<512, 4>{});
		if (g.block == 512) return f(Geo<kWideT, kWideK>{});
	}
	if constexpr ((GEOS & kGeoBytes) != 0) {
		if (g.block == 768) return f(Geo<768, 2>{});
	}
	if constexpr ((GEOS & kGeoSpan) != 0) {
		if (g.block == kSpanT) return f(Geo<kSpanT, kSpanK>{});
	}
	if constexpr ((GEOS & kGeoSmall) != 0) {
		if (g.block == 256) return f(Geo<256, 3>{});
		if (g.block == 128) return f(Geo<128, 3>{});
		if (g.block == 64) return f(Geo<64, 3>{});
	}
	return none;
}

// ---- a unit: struct { using Sets, using BiasedSets (those of Sets with copies on biased offsets); static constexpr unsigned geos; }
// f(Geo, PenSet) for the unit's instantiation that (e1, e2) and `g` ask for, `none` when it holds none (the geometry first: a copy on biased offsets looks (e1, e2)
// up in BiasedSets, every other geometry in Sets)
template <class U, class R, class F>
R band2_select(int e1, int e2, const BandGeom &g, R none, F &&f)
{
	return for_band_geom<U::geos>(g, none, [&](auto geo) {
		using Sets = std::conditional_t<decltype(geo)::BI4, typename U::BiasedSets, typename U::Sets>;
		return for_pen_set(Sets{}, e1, e2, none, [&](auto set) { return f(geo, set); });
	});
}

// the two entry points of a unit: -1 / 0 mean "this unit does not hold that launch" (or the geometry's sequence copy is not the launch's: launch_one), -2 a failed launch
template <class U>
int band2_unit_launch(const BatchArgs &a, int grid, const BandGeom &g, void *stream)
{
	return band2_select<U>(a.pen.e1, a.pen.e2, g, -1, [&](auto geo, auto set) {
		using G = decltype(geo);
		using S = decltype(set);
		return launch_one<G::T, G::K, S::e1, S::e2, G::BI4>(a, grid, g.lds_bytes, g.tab, g.seq2 != 0, (hipStream_t)stream);
	});
}

template <class U>
int band2_unit_occupancy(const Penalty &p, const BandGeom &g, bool cigar)
{
	return band2_select<U>(p.e1, p.e2, g, 0, [&](auto geo, auto set) {
		using G = decltype(geo);
		using S = decltype(set);
		return occ_one<G::T, G::K, S::e1, S::e2, G::BI4>(g.lds_bytes, g.seq2 != 0, cigar);
	});
}

} // namespace

} // namespace mwf
