#!/bin/sh
# Builds libsdf_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
# One object per translation unit of this directory; the comments below say which unit gets which flags and why.
# -ffp-contract=off: the interpreter must round like NumPy (separate multiply and add);
# fused multiply-adds are written explicitly where the reference goes through BLAS.
# The fused sample+march kernel is instantiated per family (float64, with / without the trigonometric ops) in its own
# translation unit so the families compile in parallel.  (float32 sampling of the meshing path: removed in round 5.)
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# -structurizecfg-skip-uniform-regions: every branch of the tape interpreter is wave-uniform and its dispatch is a
# scalar jump through a table (asm goto + s_setpc, sdf_interp.h); the structurizer has to leave that alone -- a build of
# the interpreters WITHOUT the option faults on the device.  The option is NOT safe for kernels whose lanes diverge
# (r03: it miscompiled k_expand), so only the interpreters' translation units get it and every other kernel lives in
# sdf_plain.hip / sdf_weld.hip.
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -mllvm -structurizecfg-skip-uniform-regions=1"
mkdir -p build
rm -f libsdf_hip.so build/*.o
# what built the library goes INTO the library (sdf_build_info(): compiler version + the interpreters' flags): a box without the
# test suite can still say which toolchain its .so came from; tools/isa_check.py (run by build()) checks what that toolchain made
INFO="$($HIPCC --version | grep -m1 -i 'HIP version' | tr -d '"' | sed 's/^ *//'); $($HIPCC --version | grep -m1 -i 'clang version' | tr -d '"' | cut -c1-60); flags: $FLAGS"
pids=""
$HIPCC $FLAGS "-DSDF_BUILD_INFO=\"$INFO\"" -c -o build/sdf_hip.o sdf_hip.hip "$@" & pids="$pids $!"
$HIPCC $FLAGS -c -o build/sdf_bounds.o sdf_bounds.hip "$@" & pids="$pids $!"
# (the sphere tracer k_render: a tape interpreter whose loops are all wave-uniform, see sdf_render.hip)
$HIPCC $FLAGS -c -o build/sdf_render.o sdf_render.hip "$@" & pids="$pids $!"
# (the vertex normals of the indexed export k_vertex_normals: a tape interpreter, six wave-uniform passes, see sdf_normals.hip)
$HIPCC $FLAGS -c -o build/sdf_normals.o sdf_normals.hip "$@" & pids="$pids $!"
# (the wall-thickness probe k_vertex_thickness: a tape interpreter whose loops are all wave-uniform, see sdf_thickness.hip)
$HIPCC $FLAGS -c -o build/sdf_thickness.o sdf_thickness.hip "$@" & pids="$pids $!"
$HIPCC $FLAGS -DMESH_T=double -DMESH_FULL=0 -DMESH_NAME=sdf_launch_mesh_f64 -c -o build/mesh_f64.o sdf_mesh_inst.hip "$@" & pids="$pids $!"
$HIPCC $FLAGS -DMESH_T=double -DMESH_FULL=1 -DMESH_NAME=sdf_launch_mesh_f64_full -c -o build/mesh_f64_full.o sdf_mesh_inst.hip "$@" & pids="$pids $!"
# (every kernel that is not a tape interpreter: built WITHOUT the structurizer option, see sdf_plain.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_plain.o sdf_plain.hip "$@" & pids="$pids $!"
# (host code only -- the runtime every unit shares, the meshing paths through device memory, the readers of a finished mesh, the
# multi-GPU step: they launch through the launchers of sdf_plain / sdf_normals / sdf_thickness / sdf_weld and, for the one interpreter kernel
# among them, k_eval_tiles, through enqueue_eval_tiles of sdf_hip.hip, so they take the plain flags)
for u in sdf_runtime sdf_chunked sdf_mesh_out sdf_comm; do
    $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/$u.o $u.hip "$@" & pids="$pids $!"
done
# (the mesh-to-level-set voxelizer: plain kernels, float64 rounded like NumPy's, see sdf_level_set.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_level_set.o sdf_level_set.hip "$@" & pids="$pids $!"
# (the exact Euclidean distance transform of `text` / `image`: plain kernels, integer arithmetic and one float64 sqrt, see sdf_edt.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_edt.o sdf_edt.hip "$@" & pids="$pids $!"
# (the moments and the edge census of a mesh: plain kernels, float64 rounded like NumPy's, and hipCUB's radix sort, see sdf_measure.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_measure.o sdf_measure.hip "$@" & pids="$pids $!"
# (the connected shells of a mesh and their selection: plain kernels, integer atomics, and the scan of sdf_prims.hip, see sdf_components.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_components.o sdf_components.hip "$@" & pids="$pids $!"
# (the mesh simplified by vertex clustering with quadric vertices: plain kernels, float64 rounded like NumPy's, hipCUB's radix sort and the scan of sdf_prims.hip, see sdf_simplify.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_simplify.o sdf_simplify.hip "$@" & pids="$pids $!"
# (the mesh mended -- duplicate triangles dropped, oppositely wound pairs cancelled: plain kernels, integers only, hipCUB's radix sort, the scan of sdf_prims.hip and the copy of sdf_components.hip, see sdf_mend.hip)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -c -o build/sdf_mend.o sdf_mend.hip "$@" & pids="$pids $!"
# (the weld uses hipCUB's radix sort and scan; it has no floating-point arithmetic of its own)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -c -o build/sdf_weld.o sdf_weld.hip "$@" & pids="$pids $!"
# (numbering flagged items for the mesh readers: hipCUB's exclusive int scan, instantiated here once; no floating point, the weld's flags)
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -c -o build/sdf_prims.o sdf_prims.hip "$@" & pids="$pids $!"
for p in $pids; do wait $p; done
exec $HIPCC --offload-arch=gfx950 -fPIC -shared -o libsdf_hip.so build/sdf_hip.o build/mesh_f64.o build/mesh_f64_full.o \
    build/sdf_bounds.o build/sdf_render.o build/sdf_normals.o build/sdf_thickness.o build/sdf_weld.o build/sdf_plain.o build/sdf_level_set.o build/sdf_edt.o \
    build/sdf_runtime.o build/sdf_chunked.o build/sdf_mesh_out.o build/sdf_comm.o build/sdf_measure.o build/sdf_components.o build/sdf_simplify.o build/sdf_mend.o build/sdf_prims.o
