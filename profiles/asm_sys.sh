#!/bin/bash
# Development aid: compile the whole-device kernel's two units (mwf_sys.hip, mwf_sys_deep.hip) to gfx950 assembly and print the register / spill
# table of every instantiation: wfa_sys_kernel<E1, E2, P, DEFER, TB, C> and wfa_sys_seg_kernel<E1, E2, P, DEFER, C> (the provenance pass).
# Usage: profiles/asm_sys.sh [extra flags] > profiles/sys_registers.txt
cd "$(dirname "$0")/../miniwfa_amd/csrc" || exit 1
tmp=$(mktemp -d) || exit 1
for unit in mwf_sys mwf_sys_deep; do
	/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -I ../../include -I . "$@" --offload-device-only -S $unit.hip -o "$tmp/$unit.s" 2>&1 | grep -v hip-link &
done
wait
printf "%-20s %-14s %18s %12s %6s %12s\n" "kernel" "template args" "scratch bytes/lane" "sgpr spills" "vgprs" "vgpr spills"
echo "(wfa_sys_kernel<E1,E2,P,DEFER,TB,C>, wfa_sys_seg_kernel<E1,E2,P,DEFER,C>; 512 threads per workgroup: at most 256 VGPRs)"
for unit in mwf_sys mwf_sys_deep; do
	echo "== $unit.hip"
	grep -E "sgpr_spill_count|\.vgpr_count|vgpr_spill_count|private_segment_fixed_size:|\.name:" "$tmp/$unit.s" | paste - - - - - | sed 's/ \+/ /g' | grep wfa_sys |
		sed -E 's/.*\.name: *[A-Za-z0-9_]*(wfa_sys_(seg_)?kernel)I([A-Za-z0-9]*)EEvNS_9BatchArgsE/\1 \3/; s/Li//g; s/Lb//g; s/E/,/g; s/,( |$)/ /' |
		awk '{sub(/,$/, "", $2); printf "%-20s %-14s %18s %12s %6s %12s\n", $1, $2, $4, $6, $8, $10}' | sort
done
rm -rf "$tmp"
