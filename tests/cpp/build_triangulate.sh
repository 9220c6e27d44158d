#!/bin/bash
# Build the CreateNewMapPoints host-unit programs (no library needed). Outputs under tests/cpp/build/:
#   test_triangulate        csrc/triangulate.c over tests/golden/triangulate_vectors.txt (test_triangulate.c)
#   test_triangulate_asan   the same under ASan + UBSan, stand-alone
#   check_atan2f            tools/check_atan2f.c, the C statement of the device atan2f against libm
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$R/tests/cpp/build"
SRC="$R/tests/cpp/test_triangulate.c $R/cooperative-orb-slam_amd/csrc/triangulate.c $R/cooperative-orb-slam_amd/csrc/unproject.c"
gcc -std=c11 -O2 -ffp-contract=off -Wall -I "$R/include" $SRC -o "$R/tests/cpp/build/test_triangulate" -lm
SAN="-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1"
gcc -std=c11 -ffp-contract=off $SAN -Wall -I "$R/include" $SRC -o "$R/tests/cpp/build/test_triangulate_asan" -lm
gcc -O2 -ffp-contract=off -Wall "$R/tools/check_atan2f.c" -o "$R/tests/cpp/build/check_atan2f" -lm
