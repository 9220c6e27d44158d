#!/bin/bash
# Build the KeyFrameDatabase drop-in test (needs liborbamd.so built). Output: tests/cpp/build/test_kfdb
set -e
R=$(cd "$(dirname "$0")/../../.." && pwd)
mkdir -p "$R/tests/cpp/build"
g++ -std=c++14 -O1 -ffp-contract=off -pthread -Wall -Wno-unused-function \
  -I "$R/tests/cpp/kfdb" -I "$R/cooperative-orb-slam_amd/host" -I "$R/include" \
  "$R/tests/cpp/kfdb/test_kfdb.cpp" "$R/cooperative-orb-slam_amd/host/KeyFrameDatabase_amd.cc" \
  "$R/cooperative-orb-slam_amd/host/orbamd_status.cc" \
  -L "$R/cooperative-orb-slam_amd/lib" -lorbamd \
  -Wl,-rpath,"$R/cooperative-orb-slam_amd/lib" -Wl,-rpath,/opt/rocm/lib \
  -o "$R/tests/cpp/build/test_kfdb"
