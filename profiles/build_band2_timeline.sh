#!/bin/bash
# Probe build of the per-pair timeline (BatchArgs::timeline, mwf_gpu_test_hook "timeline"): the packed band kernel with
# experiments/band2_timeline.patch applied — two stores of thread 0 per pair — linked with every other object of the regular build.
# Kept out of the product kernel: the stores move the SGPR spill counts of the 512-thread instantiations (59 -> 61 on <512,3,2,1> folded score-only,
# 63 -> 60 on <512,4,2,1>; VGPRs unchanged).  Usage: profiles/build_band2_timeline.sh  -> profiles/_timeline_libmwf_hip.so (MWF_HIP_LIB=...)
set -e
cd "$(dirname "$0")/.."
C=miniwfa_amd/csrc
[ -f $C/build/mwf_engine.cpp.o ] || python miniwfa_amd/build.py > /dev/null
T=$(mktemp -d)
cp $C/mwf_band2.hip $T/mwf_band2.hip
patch -s -d $T -p3 < profiles/experiments/band2_timeline.patch
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -I include -I $C -c $T/mwf_band2.hip -o $T/mwf_band2.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared $T/mwf_band2.o $C/build/mwf_sys.hip.o $C/build/mwf_mid.hip.o $C/build/mwf_lane.hip.o \
  $C/build/mwf_kernels.hip.o $C/build/mwf_engine.cpp.o $C/build/mwf_memory.cpp.o $C/build/mwf_plan.cpp.o $C/build/mwf_chain.cpp.o $C/build/mwf_async.cpp.o $C/build/kalloc.cpp.o $C/build/mwf_dbg.cpp.o -o profiles/_timeline_libmwf_hip.so -lpthread
rm -rf $T
echo profiles/_timeline_libmwf_hip.so
