// mwf_band2_tab.hip — the packed band kernel's table form: the first probe of the match extension reads per-position 8-mer tables in LDS (mwf_band2.hip: kTabProbe).
// 512 threads x 3 and x 4 chunk slots, gap extensions (2,1), 2-bit copies, folded, with and without traceback: four kernels, wfa_band2_tab_kernel.
// The template and its helpers are mwf_band2.hip's; this unit instantiates its own dispatch (launch_band2_tab, band2_occupancy_tab) and nothing else.
#define MWF_BAND2_TAB 1
#include "mwf_band2.hip"
