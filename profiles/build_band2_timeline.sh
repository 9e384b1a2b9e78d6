#!/bin/bash
# Probe build of the per-pair timeline (BatchArgs::timeline, mwf_gpu_test_hook "timeline"): the packed band kernel with
# experiments/band2_timeline.patch applied to its template (mwf_band2_kernel.h) — two stores of thread 0 per pair —, its units (miniwfa_amd/build.py:
# BAND2_UNITS) compiled against the patched header and linked with every other object of the regular build.
# Kept out of the product kernel: the stores move the SGPR spill counts of the 512-thread instantiations (59 -> 61 on <512,3,2,1> folded score-only,
# 63 -> 60 on <512,4,2,1>; VGPRs unchanged).  Usage: profiles/build_band2_timeline.sh  -> profiles/_timeline_libmwf_hip.so (MWF_HIP_LIB=...)
set -e
cd "$(dirname "$0")/.."
C=miniwfa_amd/csrc
[ -f $C/build/mwf_engine.cpp.o ] || python miniwfa_amd/build.py > /dev/null
UNITS=$(python miniwfa_amd/build.py --list-band-units)
T=$(mktemp -d)
cp $C/mwf_band2_kernel.h $T/mwf_band2_kernel.h
patch -s -d $T -p3 < profiles/experiments/band2_timeline.patch
OBJS=""
for f in $UNITS; do   # (a quoted #include looks beside the including file first: the units and the dispatch header are copied beside the patched template)
  cp $C/$f $C/mwf_band2_dispatch.h $T/
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -I include -I $C -c $T/$f -o $T/$f.o &
  OBJS="$OBJS $T/$f.o"
done
wait
for f in $(python miniwfa_amd/build.py --list-sources); do
  case " $UNITS " in *" $f "*) ;; *) OBJS="$OBJS $C/build/$f.o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared $OBJS -o profiles/_timeline_libmwf_hip.so -lpthread
rm -rf $T
echo profiles/_timeline_libmwf_hip.so
