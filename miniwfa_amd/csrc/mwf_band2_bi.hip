// mwf_band2_bi.hip — the packed band kernel's (mwf_band2.hip) five- and six-slot copies of the 512-thread geometry on biased offsets (class 14 of mwf_plan.cpp:
// pairs of up to ~21 kb that plain 16-bit offsets cannot be promised to hold, two workgroups per CU) for gap extensions (2, 2) — main.c's -a preset, folded and
// not — and (1, 1).  A unit of its own so that it compiles beside mwf_band2.hip; it defines launch_band2_bi1 and band2_occupancy_bi1 and nothing else
// (mwf_band2.hip: MWF_BAND2_BIASED).  Registers and scratch: profiles/band_biased/band2_biased_registers.txt.
#define MWF_BAND2_BIASED 1
#include "mwf_band2.hip"
