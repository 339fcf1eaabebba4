// Host-side launch plumbing shared by the persistent kernels' launchers (definitions: prof.hip).
#pragma once

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
// MORIG_DEBUG_FLAGS (ablation switches for tools/microbench.py; 0 in production), parsed once per process
int debug_flags();

}  // namespace morig
