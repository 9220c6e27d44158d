#!/bin/bash
# Build the host test library of the BF matcher's epipolar tile cull (csrc/orb_tri_cull.h through tri_cull_host.cpp;
# no HIP, no GPU). Output: tests/cpp/build/libtricull.so. The float arithmetic is stated operation by operation, as
# in the device build: no fma contraction.
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$R/tests/cpp/build"
g++ -std=c++17 -O2 -fPIC -shared -ffp-contract=off -Wall \
  "$R/tests/cpp/tri_cull_host.cpp" -o "$R/tests/cpp/build/libtricull.so"
