#!/bin/bash
# Build the Frame::isInFrustum host-unit programs (no library needed). Outputs under tests/cpp/build/:
#   test_frustum        csrc/frustum.c over tests/golden/frustum_vectors.txt (test_frustum.c)
#   test_frustum_asan   the same under ASan + UBSan, stand-alone
#   check_logf          tools/check_logf.c, the C statement of the device logf against libm
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$R/tests/cpp/build"
gcc -std=c11 -O2 -ffp-contract=off -Wall -I "$R/include" \
  "$R/tests/cpp/test_frustum.c" "$R/cooperative-orb-slam_amd/csrc/frustum.c" \
  -o "$R/tests/cpp/build/test_frustum" -lm
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
gcc -std=c11 -ffp-contract=off $SAN -Wall -I "$R/include" \
  "$R/tests/cpp/test_frustum.c" "$R/cooperative-orb-slam_amd/csrc/frustum.c" \
  -o "$R/tests/cpp/build/test_frustum_asan" -lm
gcc -O2 -ffp-contract=off -Wall "$R/tools/check_logf.c" -o "$R/tests/cpp/build/check_logf" -lm
