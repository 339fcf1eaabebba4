// Host-side launch plumbing shared by the persistent kernels' launchers (definitions: prof.hip).
#pragma once
#include "dispatch_core.h"

namespace morig {

// compute units of the current device (cached per device; 256 when the runtime cannot say)
int cu_count();
// CUs the caller wants left alone by the persistent kernels (set while long single-CU kernels such as FPS run on another
// stream: a persistent workgroup that cannot be placed until they finish would hold back its whole static tile list)
void set_reserved_cus(int n);
int reserved_cus();
// grid of a persistent launch with `units` workgroups' worth of work: one workgroup per CU, a multiple of 8 (XCDs) -- the CUs rounded
// down to a multiple of 8, less the reserved CUs rounded up to 8, at least 8; a short launch is rounded up to 8
int persistent_grid(int units);
// the environment switches of the GEMM / EdgeConv launch path (dispatch_core.h), parsed once per process. The two that a call reads
// again come with the copy its entry point takes: MORIG_NO_DMA for morig_gemm, MORIG_NO_EDGE_PC for morig_edgeconv (one getenv per
// launch, as before: at one mesh per forward a launch is a few microseconds of host time)
const Switches& switches();
Switches gemm_switches();
Switches edge_switches();
// MORIG_DEBUG_FLAGS (ablation switches for tools/microbench.py; 0 in production), parsed once per process
int debug_flags();

}  // namespace morig
