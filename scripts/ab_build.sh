#!/bin/bash
# build an A/B candidate step library into abtest/ (scratch, git-ignored): bash scripts/ab_build.sh NAME CSRC_COPY_DIR [extra hipcc flags]
# (CSRC_COPY_DIR: a whole copy of allsteps_isaaclab_amd/csrc, e.g. `cp -r allsteps_isaaclab_amd/csrc abtest/csrc_NAME`,
#  with the phase header under test edited: its allsteps_kernels.hip is compiled, every "x.h" it includes is the
#  copy's own, and -iquote resolves its ../../include paths from this tree's csrc; allsteps_abi.hip is this tree's)
set -e
cd "$(dirname "$0")/.."
N=$1; SRC=$2; shift 2
[ -f "$SRC/allsteps_kernels.hip" ] || { echo "usage: ab_build.sh NAME CSRC_COPY_DIR [flags]: no $SRC/allsteps_kernels.hip" >&2; exit 2; }
mkdir -p abtest
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -I include \
  -iquote allsteps_isaaclab_amd/csrc -DAS_BUILD_ID=\"abtest-$N\" -fPIC -shared -Wno-unused-result "$@" \
  -o abtest/$N.so "$SRC/allsteps_kernels.hip" allsteps_isaaclab_amd/csrc/allsteps_abi.hip
echo built abtest/$N.so
