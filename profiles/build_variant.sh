#!/bin/bash
# Build a variant of the library with extra flags for the band / whole-device kernels (e.g. -DMWF_SYS_TIMING -DMWF_BAND_DEV)
# into profiles/_<name>_libmwf_hip.so; the other objects come from the regular build (miniwfa_amd/csrc/build).  The band units and the full
# list of sources are miniwfa_amd/build.py's.
# Usage: profiles/build_variant.sh <name> <flags...>     then run with MWF_HIP_LIB=profiles/_<name>_libmwf_hip.so
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
C=miniwfa_amd/csrc
[ -f $C/build/mwf_engine.cpp.o ] || python miniwfa_amd/build.py > /dev/null
mkdir -p /tmp/mwf_variant_$NAME
KERNELS="$(python miniwfa_amd/build.py --list-band-units) mwf_sys.hip mwf_sys_deep.hip mwf_mid.hip mwf_lane.hip mwf_cigar_ops.hip"
OBJS=""
for f in $KERNELS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -Wno-unused-value -I include -I $C "$@" -c $C/$f -o /tmp/mwf_variant_$NAME/$f.o &
  OBJS="$OBJS /tmp/mwf_variant_$NAME/$f.o"
done
wait
for f in $(python miniwfa_amd/build.py --list-sources); do
  case " $KERNELS " in *" $f "*) ;; *) OBJS="$OBJS $C/build/$f.o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared $OBJS -o profiles/_${NAME}_libmwf_hip.so -lpthread
echo profiles/_${NAME}_libmwf_hip.so
