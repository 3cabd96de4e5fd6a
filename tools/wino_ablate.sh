#!/bin/bash
# Build ablated variants of the Winograd kernel (profiling only; results are numerically wrong by construction) next to the
# library: gen6d_amd/csrc/_abl/libgen6d_wA.so, A = 1..5 (see WINO_ABLATE in wino_common.h: both units of the F(2x2,3x3) family are
# rebuilt, wino_conv.hip for the fp32 kernel and wino16_conv.hip for the 16-bit ones, whose own ablation is A = 6).  Run
# tools/wino_ablate_run.sh on the GPU.
set -e
cd "$(dirname "$0")/../gen6d_amd/csrc"
make -s
mkdir -p _abl
OTHERS=$(ls *.o | grep -v -e wino_conv.o -e wino16_conv.o)
for a in ${ABL:-1 2 3 4 5}; do
  for u in wino wino16; do
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -fno-slp-vectorize -DWINO_ABLATE=$a -c ${u}_conv.hip -o _abl/${u}_$a.o
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OTHERS _abl/wino_$a.o _abl/wino16_$a.o -o _abl/libgen6d_w$a.so
done
