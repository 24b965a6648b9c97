// mesh_resources_probe.hip -- ONE one-pass three-sample variant of k_mesh, for tests/test_mesh_resources_host.py: compiled through
// tools/kernel_resources.sh (MESH_SRC=this file) with the defines of a family (-DMESH_T=double -DMESH_FULL=0) and -DPROBE_FILE=0 | 1 | 3,
// the register file (1,1) | (2,2) | (2,4) as launch_mesh numbers them.  What the compiler reports for a kernel does not depend on the
// other kernels of its unit, so these are the figures of the library's own instantiation (sdf_mesh_inst.hip), at a twelfth of the time.
#include "sdf_device.h"

namespace sdfk {
#if PROBE_FILE == 0
template __global__ void k_mesh<MESH_T, (MESH_FULL != 0), 1, 1, 3, 1024, false>(const uint32_t *, const MESH_T *, MeshArgs);
#elif PROBE_FILE == 1
template __global__ void k_mesh<MESH_T, (MESH_FULL != 0), 2, 2, 3, 1024, false>(const uint32_t *, const MESH_T *, MeshArgs);
#elif PROBE_FILE == 3
template __global__ void k_mesh<MESH_T, (MESH_FULL != 0), 2, 4, 3, 1024, false>(const uint32_t *, const MESH_T *, MeshArgs);
#else
#error "PROBE_FILE: 0, 1 or 3"
#endif
}  // namespace sdfk
