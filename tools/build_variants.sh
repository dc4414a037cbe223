#!/bin/bash
# Builds decode-kernel variants as separate libraries for A/B timing
# (select one with PA_AMD_LIB=pa_amd/variants/libsb_<name>.so).
# A variant's flags go to every unit that includes sb_dev_core.h, built side
# by side; the other objects are the library's own.
set -e
cd "$(dirname "$0")/../pa_amd"
make -s
mkdir -p variants
UNITS="sb_decode sb_list"
build() {
  name=$1; shift
  mkdir -p _build/variants/$name
  pids=
  for u in $UNITS; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function "$@" -x hip -c csrc/$u.hip -o _build/variants/$name/$u.hip.o &
    pids="$pids $!"
  done
  for p in $pids; do wait $p; done
  /opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -fPIC -o variants/libsb_$name.so _build/variants/$name/*.o $(ls _build/*.o | grep -v -E "/(${UNITS// /|})\.hip\.o$") -l:liblz4.so.1 -l:libzstd.so.1 -lpthread
}
pids=
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  build $name $flags &
  pids="$pids $!"
done
for p in $pids; do wait $p; done
ls variants
