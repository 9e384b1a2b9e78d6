#!/bin/bash
# Build a variant of the library in which only the packed band kernel's units (miniwfa_amd/build.py: BAND2_UNITS) are compiled with extra flags; every
# other object comes from the regular build (miniwfa_amd/csrc/build).  Usage: profiles/build_band2_variant.sh <name> <flags...>  -> profiles/_<name>_libmwf_hip.so
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
C=miniwfa_amd/csrc
[ -f $C/build/mwf_engine.cpp.o ] || python miniwfa_amd/build.py > /dev/null
UNITS=$(python miniwfa_amd/build.py --list-band-units)
mkdir -p /tmp/mwf_b2_$NAME
OBJS=""
for f in $UNITS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -Wno-unused-value -I include -I $C "$@" -c $C/$f -o /tmp/mwf_b2_$NAME/$f.o &
  OBJS="$OBJS /tmp/mwf_b2_$NAME/$f.o"
done
wait
for f in $(python miniwfa_amd/build.py --list-sources); do
  case " $UNITS " in *" $f "*) ;; *) OBJS="$OBJS $C/build/$f.o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared $OBJS -o profiles/_${NAME}_libmwf_hip.so -lpthread
echo profiles/_${NAME}_libmwf_hip.so
