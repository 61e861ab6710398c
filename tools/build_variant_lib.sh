#!/bin/bash
# libsbwtgpu built with extra -D switches, for A/B runs: tools/build_variant_lib.sh <name> [-DX=1 ...]  ->  sbwt_amd/lib/lib_<name>.so
# The sources are the build driver's (sbwt_amd.build.GPU_SRCS): this script keeps no list of its own.
set -e
NAME=$1; shift
cd "$(dirname "$0")/.."
SRCS=$(python3 -c 'from sbwt_amd.build import GPU_SRCS; print(" ".join(GPU_SRCS))')
mkdir -p sbwt_amd/lib
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -w "$@" -o sbwt_amd/lib/lib_$NAME.so $SRCS -ldl
