#!/bin/bash
# Print per-kernel VGPRs / spilled VGPRs / scratch / static LDS / occupancy for one HIP source (dev
# tool). Usage: resusage.sh [csrc/file.hip [extra compiler flags, e.g. -DBN_DEV]]
f=${1:-csrc/antt_bs.hip}
shift
o=$(mktemp --suffix=.o)
trap 'rm -f "$o"' EXIT
hipcc -O3 --offload-arch=gfx950 -std=c++17 -I"$(dirname "$0")/../../include" "$@" -c "$f" -o "$o" \
  -Rpass-analysis=kernel-resource-usage 2>&1 | grep remark | sed 's/.*remark: //; s/ \[-Rpass.*//' |
  awk '/Function Name/{name=$3} /VGPRs:/{v=$2} /VGPRs Spill/{sp=$3} /ScratchSize/{sc=$3} /Occupancy/{o=$3} /LDS Size/{print name, "vgpr=" v, "spill=" sp, "scratch=" sc, "lds=" $4, "occ=" o}'
