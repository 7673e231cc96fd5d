#!/bin/bash
# A/B of the cascaded-section kernels' chunk length C and tile workgroup size (k_sos.hip: SP_SOS_C, SP_SOS_WG).
# Builds one library per variant under build/sos_ab/ (the in-tree build's other objects + k_sos.hip with -D overrides)
# and runs `tools/cfgbench.py --only sos` on each through SP_LIB_PATH, two rounds, interleaved.
#   usage: tools/sos_ab.sh [C:WG ...]        (default: 32:256 16:256 64:128; needs `make` first)
set -e
cd "$(dirname "$0")/.."
OUT=build/sos_ab
mkdir -p $OUT
variants=${*:-"32:256 16:256 64:128"}
others=$(ls build/obj/*.o | grep -v '/k_sos\.o$')
for v in $variants; do
  c=${v%%:*}; wg=${v#*:}
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fno-slp-vectorize --offload-arch=gfx950 -Iinclude -Ipyfft_amd/csrc \
    -DSP_SOS_C=$c -DSP_SOS_WG=$wg -c pyfft_amd/csrc/k_sos.hip -o $OUT/k_sos_${c}_${wg}.o
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $others $OUT/k_sos_${c}_${wg}.o -o $OUT/libspectral_${c}_${wg}.so
done
# every run's own exit status is checked: after a failure (a fault, an abort, a time limit) nothing more is started
set +e
for round in 1 2; do
  for v in $variants; do
    c=${v%%:*}; wg=${v#*:}
    echo "[$round] C=$c WG=$wg"
    SP_LIB_PATH=$OUT/libspectral_${c}_${wg}.so timeout -k 10 300 python tools/cfgbench.py --only sos --reps 3 > $OUT/run.log 2>&1
    rc=$?
    grep sos $OUT/run.log
    if [ $rc -ne 0 ]; then
      echo "C=$c WG=$wg: exit status $rc -- stopping"
      tail -n 20 $OUT/run.log
      exit $rc
    fi
  done
done
