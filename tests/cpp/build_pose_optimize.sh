#!/bin/bash
# Build the PoseOptimization host-unit programs (no library needed). Outputs under tests/cpp/build/:
#   test_pose_optimize        csrc/pose_optimize.c over tests/golden/pose_vectors.txt (test_pose_optimize.c)
#   test_pose_optimize_asan   the same under ASan + UBSan, stand-alone
#   check_so3_sincos          tools/check_so3_sincos.c, the C statement of so3_sincos against libm
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$R/tests/cpp/build"
SRC="$R/tests/cpp/test_pose_optimize.c $R/cooperative-orb-slam_amd/csrc/pose_optimize.c"
gcc -std=c11 -O2 -ffp-contract=off -Wall -I "$R/include" $SRC -o "$R/tests/cpp/build/test_pose_optimize" -lm
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
gcc -std=c11 -ffp-contract=off $SAN -Wall -I "$R/include" $SRC -o "$R/tests/cpp/build/test_pose_optimize_asan" -lm
gcc -std=c11 -O2 -ffp-contract=off -Wall -I "$R/cooperative-orb-slam_amd/csrc" "$R/tools/check_so3_sincos.c" \
    -o "$R/tests/cpp/build/check_so3_sincos" -lm
