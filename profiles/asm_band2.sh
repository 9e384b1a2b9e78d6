#!/bin/bash
# Development aid: compile a unit of the packed band kernel (default: the first of miniwfa_amd/build.py's BAND2_UNITS, the main unit; dev subset of variants:
# MWF_BAND_DEV) to gfx950 assembly and print the register / spill table.
# Usage: [UNIT=mwf_band2_tab.hip] profiles/asm_band2.sh [extra flags]   -> /tmp/band2_new.s, /tmp/n512.s (the 512x3 score-only folded 2-bit kernel)
cd "$(dirname "$0")/.." || exit 1
UNIT=${UNIT:-$(python miniwfa_amd/build.py --list-band-units | cut -d' ' -f1)}
cd miniwfa_amd/csrc || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-const-variable -I ../../include -I . -DMWF_BAND_DEV "$@" --offload-device-only -S $UNIT -o /tmp/band2_new.s 2>&1 | grep -v hip-link
grep -E "sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size:|\.name:" /tmp/band2_new.s | paste - - - - - | sed 's/ \+/ /g' | sed 's/.*wfa_band2_\(tab_\|nib_\)\?kernelI//'
awk '/^_ZN3mwf12_GLOBAL__N_1[0-9]+wfa_band2_(tab_|nib_)?kernelILi512ELi3ELi2ELi1ELb0ELb1ELb0ELb1EEEvNS_9BatchArgsE:/{p=1} p{print} /^\.Lfunc_end/{if(p){exit}}' /tmp/band2_new.s > /tmp/n512.s
grep "amdhsa_group_segment_fixed_size" /tmp/band2_new.s | sort | uniq -c
