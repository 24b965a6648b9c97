#!/bin/sh
# development build: recompile ONLY the named objects of sdf_amd/csrc/build.units and relink (build.sh, what build() runs, always
# rebuilds everything; an unknown name or none lists the names).   tools/devbuild.sh sdf_generate sdf_plain
SDF_BUILD_ONLY="${*:--}" exec sh "$(dirname "$0")/../sdf_amd/csrc/build.sh"
