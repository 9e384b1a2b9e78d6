// mwf_band2_nib.hip — the packed band kernel's 4-bit form: pairs of 5 to 16 distinct bytes ("alpha16": an N, IUPAC codes, mixed case) on 512 x 3, 512 x 4 and the span
// geometry, gap extensions (2,1).  mwf_band2.hip again with MWF_BAND2_NIB set: the sequence copy, the first probe and the match walks hold 4 bits per base, the kernel is
// wfa_band2_nib_kernel, and of the host side only launch_band2_nib / band2_occupancy_nib / band2_nib_supported are defined here.
#define MWF_BAND2_NIB 1
#include "mwf_band2.hip"
