// mwf_sys_deep.hip — the whole-device kernel (mwf_sys.hip, mwf_sys_pass.h) for gap extensions of 3 and 4: (e1, e2) in {3, 4} x {1, 2}, minimap2's asm5-like
// sets among them.  The same template with histories of E1 / E2 penalties: a lane carries NEF = 2 e1 + 2 e2 = 8 to 12 E/F arrays per column (the sets of
// mwf_sys.hip: 4 to 8), publishes (P + NEF) C ints per hand-off block and parks NEF C of them.  A unit of its own so that it compiles beside mwf_sys.hip.
// Forms built per set: the plain (undeferred) score, traceback and provenance passes on one and on four columns per lane — the deferred forms of the
// (2, 1) set already spill at four columns per lane, and nothing has been measured that would pay for them here.
#include "mwf_sys_pass.h"

namespace mwf {

int launch_sys_pass_deep(const BatchArgs &a, int grid, void *stream)
{
	if (a.pen.e1 == 3 && a.pen.e2 == 1) return launch_pass_d<3, 1, false>(a, grid, (hipStream_t)stream);
	if (a.pen.e1 == 3 && a.pen.e2 == 2) return launch_pass_d<3, 2, false>(a, grid, (hipStream_t)stream);
	if (a.pen.e1 == 4 && a.pen.e2 == 1) return launch_pass_d<4, 1, false>(a, grid, (hipStream_t)stream);
	if (a.pen.e1 == 4 && a.pen.e2 == 2) return launch_pass_d<4, 2, false>(a, grid, (hipStream_t)stream);
	return -1;
}

} // namespace mwf
