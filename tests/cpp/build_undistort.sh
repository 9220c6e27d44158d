#!/bin/bash
# Build the undistortion programs (need liborbamd.so built). Outputs under tests/cpp/build/:
#   test_undistort            the drop-in Frame::UndistortKeyPoints / ComputeImageBounds (test_undistort.cpp)
#   test_undistort_asan       the same program's host part with csrc/undistort.c under ASan + UBSan, stand-alone
#   bench_undistort_latency   the one-frame latency of mvKeysUn in its three settings (bench_undistort_latency.cpp)
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
H="$R/cooperative-orb-slam_amd/host"
mkdir -p "$R/tests/cpp/build"
g++ -std=c++14 -O1 -ffp-contract=off -pthread -Wall -Wno-unused-function \
  -I "$R/tests/cpp/cvmin" -I "$H" -I "$R/include" \
  "$R/tests/cpp/test_undistort.cpp" "$H/Frame_undistort_amd.cc" "$H/ORBextractor.cc" "$H/orbamd_status.cc" \
  -L "$R/cooperative-orb-slam_amd/lib" -lorbamd \
  -Wl,-rpath,"$R/cooperative-orb-slam_amd/lib" -Wl,-rpath,/opt/rocm/lib \
  -o "$R/tests/cpp/build/test_undistort"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
gcc -std=c11 -ffp-contract=off $SAN -Wall -c "$R/cooperative-orb-slam_amd/csrc/undistort.c" \
  -o "$R/tests/cpp/build/undistort_asan.o"
g++ -std=c++14 -ffp-contract=off $SAN -Wall -Wno-unused-function -DORBAMD_UNDISTORT_HOST_ONLY \
  -I "$R/tests/cpp/cvmin" -I "$H" -I "$R/include" \
  "$R/tests/cpp/test_undistort.cpp" "$H/Frame_undistort_amd.cc" "$R/tests/cpp/build/undistort_asan.o" \
  -o "$R/tests/cpp/build/test_undistort_asan"
g++ -std=c++14 -O2 -Wall -I "$R/include" "$R/tests/cpp/bench_undistort_latency.cpp" \
  -L "$R/cooperative-orb-slam_amd/lib" -lorbamd \
  -Wl,-rpath,"$R/cooperative-orb-slam_amd/lib" -Wl,-rpath,/opt/rocm/lib \
  -o "$R/tests/cpp/build/bench_undistort_latency"
