// mwf_band2_bi_deep.hip — the packed band kernel's (mwf_band2.hip) five- and six-slot copies of the 512-thread geometry on biased offsets (class 14 of
// mwf_plan.cpp) for gap extensions (3, 1), (3, 2) and (4, 1), never folded.  A unit of its own so that it compiles beside mwf_band2.hip; it defines
// launch_band2_bi2 and band2_occupancy_bi2 and nothing else (mwf_band2.hip: MWF_BAND2_BIASED).  Registers and scratch:
// profiles/band_biased/band2_biased_registers.txt.
#define MWF_BAND2_BIASED 2
#include "mwf_band2.hip"
