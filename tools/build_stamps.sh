#!/bin/bash
# Tools-only build of the native library with the in-kernel time stamps of the persistent GEMM and of the 16-bit flash attention compiled
# in (-DMGEA_PH_STAMPS): tools/libmgea_hip_stamps.so, loaded by tools/gemm_bf16_stamps.py / tools/attn_stamps.py through MGEA_LIB_PATH.
# The product library never has them.  The sources are the Makefile's SRCS; gemm16 and attn16 are rebuilt with the defines, the others
# are taken from build/ (or built plainly if they are not there).
# build_stamps.sh [ablate bits]: with bits, the whole-tile K loop is built without LDS-DMA (1) / fragment reads (2) / MFMAs (4) ->
# tools/libmgea_hip_stamps_a<bits>.so (timings only, wrong results)
set -e
ABL=${1:-0}
SUF=""; [ "$ABL" != "0" ] && SUF="_a$ABL"
cd "$(dirname "$0")/../music-generation-emotion-adaptive_amd/csrc"
mkdir -p build_stamps
OBJS=""
for src in $(sed -n 's/^SRCS *:= *//p' Makefile); do
  f=${src%.hip}
  if [ $f = gemm16 ] || [ $f = attn16 ]; then
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -DMGEA_PH_STAMPS -DMGEA_PH_ABLATE=$ABL -c $f.hip -o build_stamps/$f.o
  elif [ -f build/$f.o ]; then
    cp build/$f.o build_stamps/$f.o
  else
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -c $f.hip -o build_stamps/$f.o
  fi
  OBJS="$OBJS build_stamps/$f.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/libmgea_hip_stamps$SUF.so $OBJS
ls -la ../../tools/libmgea_hip_stamps$SUF.so
