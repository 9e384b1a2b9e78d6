// mwf_band2_e3.hip — the packed band kernel (mwf_band2.hip) for gap extensions (3, 1) and (3, 2): the same template with E1 / F1 histories of 3 penalties and
// an edge table of 4 ages.  A unit of its own so that it compiles beside mwf_band2.hip; it defines launch_band2_e3 and band2_occupancy_e3 and nothing else
// (mwf_band2.hip: MWF_BAND2_DEEP).  Geometries: 64 ... 512 x 3, 512 x 4 and the 1024 x 5 span geometry on 2-bit copies, 768 x 2 byte-wise, each with and
// without traceback — never folded, no copies on biased offsets.  Registers and scratch: profiles/band_deep/band2_deep_registers.txt.
#define MWF_BAND2_DEEP 3
#include "mwf_band2.hip"
