#!/bin/bash
# Register / scratch / spill table of every k_mesh variant of one (precision, FULL) family, from the compiler's
# own remarks (-Rpass-analysis=kernel-resource-usage); cross-compiles, no GPU needed:
#   tools/kernel_resources.sh double 1        (T = double|float, FULL = 0|1|both)   [extra hipcc flags...]
# FULL = both: the two families one after the other (their compiles run side by side).  -DMESH_PROF=1 among the extra flags: the
# instrumented kernels k_mesh_prof (SDF_MESH_PROF=1).  A name reads k_mesh<T,FULL,NP,ND,NS,BLOCK,TWOPASS>.
# MESH_SRC=<file>: another unit than sdf_mesh_inst.hip that instantiates k_mesh with the same defines (tests/native/mesh_resources_probe.hip:
# one variant per compile, a few seconds instead of most of a minute).
T=${1:-double}; FULL=${2:-0}; shift; shift
cd "$(dirname "$0")/../sdf_amd/csrc"
family() {
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result \
        -mllvm -structurizecfg-skip-uniform-regions=1 -DMESH_T=$T -DMESH_FULL=$1 -DMESH_NAME=probe \
        -I. -Rpass-analysis=kernel-resource-usage -c -o /dev/null "${MESH_SRC:-sdf_mesh_inst.hip}" "${@:2}" 2>&1 | grep remark |
      sed 's/.*remark: *//; s/ \[-Rpass.*//' |
      awk '/Function Name/{if(l)print l; l=$0; next}{l=l" | "$0}END{print l}' |
      sed 's/Function Name: _ZN4sdfk6k_meshI/k_mesh</; s/Function Name: _ZN4sdfk11k_mesh_profI/k_mesh_prof</; s/EEvPKjPKT_NS_8MeshArgsE/>/; s/ELi/,/g; s/ELb/,/g; s/Lb/,/; s/E>/>/; s/AGPRs: 0 | //; s/Dynamic Stack: False | //; s/ | LDS Size.*//'
}
if [ "$FULL" = both ]; then
    tmp=$(mktemp)
    family 1 "$@" > "$tmp" & pid=$!
    family 0 "$@"
    wait $pid; cat "$tmp"; rm -f "$tmp"
else
    family "$FULL" "$@"
fi
