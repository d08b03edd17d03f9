#!/bin/bash
# Registers, scratch, LDS and occupancy of the numDisparities 272..512 instances (sm_deep.hip, all
# eight units) and of every kernel of sm_api.hip, from the compiler's resource remarks.
# Usage: bash tools/deepd_resources.sh [csrc-dir] > resources.txt
#   one line per kernel: unit name vgpr= agpr= sgpr= scratch= lds= waves=
# Pass the csrc directory of another checkout to list it (the sm_api lines of a parent and a
# branch listing must be equal: `grep '^api ' | diff`).
SRC="${1:-$(cd "$(dirname "$0")/../stereo_match_amd/csrc" && pwd)}"
T=$(mktemp -d)
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC --cuda-device-only -c -Rpass-analysis=kernel-resource-usage"
summarise() {
  sed 's/ *\[-Rpass-analysis=kernel-resource-usage\]//' |
    awk -v u="$1" '/Function Name:/ {n=$NF} / VGPRs:/ {v=$NF} /AGPRs:/ {a=$NF} /TotalSGPRs:/ {s=$NF}
      /ScratchSize/ {sc=$NF} /Occupancy/ {o=$NF}
      /LDS Size/ {print u, n, "vgpr=" v, "agpr=" a, "sgpr=" s, "scratch=" sc, "lds=" $NF, "waves=" o}'
}
cd "$SRC" || exit 1
if [ -f sm_deep.hip ]; then
  for u in 0 1 2 3 4 5 6 7; do
    (/opt/rocm/bin/hipcc $FLAGS -DDEEP_UNIT=$u -o $T/d$u.o sm_deep.hip 2>&1 | summarise deep$u > $T/r_d$u.txt) &
  done
fi
(/opt/rocm/bin/hipcc $FLAGS -o $T/api.o sm_api.hip 2>&1 | summarise api > $T/r_api.txt) &
wait
cat $T/r_*.txt | c++filt | sort
rm -rf "$T"
