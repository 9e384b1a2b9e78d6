// mwf_band2_e4.hip — the packed band kernel (mwf_band2.hip) for gap extensions (4, 1): the same template with E1 / F1 histories of 4 penalties and an edge
// table of 5 ages.  A unit of its own so that it compiles beside mwf_band2.hip; it defines launch_band2_e4 and band2_occupancy_e4 and nothing else
// (mwf_band2.hip: MWF_BAND2_DEEP).  Geometries: 64 ... 512 x 3, 512 x 4 and the 1024 x 5 span geometry on 2-bit copies, 768 x 2 byte-wise, each with and
// without traceback — never folded, no copies on biased offsets.  (4, 2) missed its gate and is not built.
// Registers and scratch: profiles/band_deep/band2_deep_registers.txt.
#define MWF_BAND2_DEEP 4
#include "mwf_band2.hip"
