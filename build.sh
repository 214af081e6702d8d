#!/bin/bash
# Build libmmd_amd.so for gfx950 (cross-compiles without a GPU).  Usage: ./build.sh [extra hipcc flags]
# -fno-slp-vectorize: the SLP vectorizer pairs fp32 ops into v_pk_* wherever it can and pays for it with v_mov shuffles; the
# kernels use packed fp32 arithmetic only where it is written out (GroupNorm + Mish epilogue, the guide's (x, y) pairs).
set -e
cd "$(dirname "$0")"
mkdir -p mmd_amd/lib
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-function -fno-slp-vectorize \
  mmd_amd/csrc/unet.hip mmd_amd/csrc/unet_f16.hip mmd_amd/csrc/unet_layers.hip mmd_amd/csrc/guide.hip mmd_amd/csrc/cons_tables.hip mmd_amd/csrc/sdf_grid.hip mmd_amd/csrc/grid_route.hip mmd_amd/csrc/route_seeds.hip mmd_amd/csrc/window_goals.hip mmd_amd/csrc/window_seeds.hip mmd_amd/csrc/window_apart.hip mmd_amd/csrc/window_aside.hip mmd_amd/csrc/fleet_epoch.hip mmd_amd/csrc/fleet_report.hip mmd_amd/csrc/api.hip mmd_amd/csrc/multi_agent.hip mmd_amd/csrc/postprocess.hip mmd_amd/csrc/round_pick.hip mmd_amd/csrc/trial_stats.hip -o mmd_amd/lib/libmmd_amd.so "$@"
echo "built mmd_amd/lib/libmmd_amd.so"
