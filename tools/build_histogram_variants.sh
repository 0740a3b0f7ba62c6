#!/bin/bash
# usage: tools/build_histogram_variants.sh [HG_AGGREGATE values, default "0 1 2"]
# builds build/hist_ab/libgenodsp_hip_agg<k>.so: the library with gdsp_histogram.hip compiled -DHG_AGGREGATE=<k> and every
# other object as the default build made it (run `make -C genodsp_amd/csrc` first).  Time one with
#   python tools/bench_histogram.py --lib build/hist_ab/libgenodsp_hip_agg0.so
set -e
cd "$(dirname "$0")/.."
FLAGS='--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result -Iinclude -Igenodsp_amd/csrc'
mkdir -p build/hist_ab
others=$(ls build/csrc/*.o | grep -v gdsp_histogram.o)
for k in ${@:-0 1 2}; do
  hipcc $FLAGS -DHG_AGGREGATE=$k -c genodsp_amd/csrc/gdsp_histogram.hip -o build/hist_ab/gdsp_histogram_agg$k.o
  hipcc --offload-arch=gfx950 -shared -fPIC -o build/hist_ab/libgenodsp_hip_agg$k.so $others build/hist_ab/gdsp_histogram_agg$k.o
  echo "built build/hist_ab/libgenodsp_hip_agg$k.so"
done
