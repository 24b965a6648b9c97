#!/bin/sh
# Builds libsdf_hip.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
# One object per line of build.units: that table says which translation unit gets which flag class and why.  The classes are spelt
# here, once.  The compiles run in parallel, each with this script's arguments behind its own; the first one that fails stops the build.
# SDF_BUILD_ONLY="object ..." (tools/devbuild.sh): compile only those lines, keep the other objects as they are, link them all.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC"
NOFP="$COMMON -Wno-unused-result"
PLAIN="$COMMON -ffp-contract=off -Wno-unused-result"
INTERP="$PLAIN -mllvm -structurizecfg-skip-uniform-regions=1"
INFO="$($HIPCC --version | grep -m1 -i 'HIP version' | tr -d '"' | sed 's/^ *//'); $($HIPCC --version | grep -m1 -i 'clang version' | tr -d '"' | cut -c1-60); flags: $INTERP"
UNITS=$(grep -v '^ *#' build.units)
NAMES=$(echo "$UNITS" | awk 'NF { printf "%s ", $1 }')
for u in $SDF_BUILD_ONLY; do
    case " $NAMES" in *" $u "*) ;; *) echo "usage: tools/devbuild.sh object ...   ($u is none of: $NAMES)" >&2; exit 2 ;; esac
done
mkdir -p build
[ -n "${SDF_BUILD_ONLY+set}" ] || rm -f libsdf_hip.so build/*.o
pids=""
objs=""
while read -r obj src class defs; do
    [ -n "$obj" ] || continue
    objs="$objs build/$obj.o"
    case " ${SDF_BUILD_ONLY-$obj} " in *" $obj "*) ;; *) continue ;; esac
    case $class in
        interp) flags=$INTERP ;; plain) flags=$PLAIN ;; nofp) flags=$NOFP ;;
        *) echo "build.units: $obj has the unknown flag class $class" >&2; exit 2 ;;
    esac
    info=""
    case $defs in BUILD_INFO) defs=""; info="-DSDF_BUILD_INFO=\"$INFO\"" ;; esac
    $HIPCC $flags $defs ${info:+"$info"} -c -o build/$obj.o $src "$@" & pids="$pids $!"
done <<EOF
$UNITS
EOF
for p in $pids; do wait $p; done
exec $HIPCC --offload-arch=gfx950 -fPIC -shared -o libsdf_hip.so $objs
