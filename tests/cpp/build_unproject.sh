#!/bin/bash
# Build the Frame::UnprojectStereo host-unit programs (no library needed). Outputs under tests/cpp/build/:
#   test_unproject        csrc/unproject.c over tests/golden/unproject_vectors.txt (test_unproject.c)
#   test_unproject_asan   the same under ASan + UBSan, stand-alone
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$R/tests/cpp/build"
gcc -std=c11 -O2 -ffp-contract=off -Wall -I "$R/include" \
  "$R/tests/cpp/test_unproject.c" "$R/cooperative-orb-slam_amd/csrc/unproject.c" \
  -o "$R/tests/cpp/build/test_unproject"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
gcc -std=c11 -ffp-contract=off $SAN -Wall -I "$R/include" \
  "$R/tests/cpp/test_unproject.c" "$R/cooperative-orb-slam_amd/csrc/unproject.c" \
  -o "$R/tests/cpp/build/test_unproject_asan"
