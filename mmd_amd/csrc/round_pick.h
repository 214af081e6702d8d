// The round's pick (round_pick.hip) as the sampling loop enqueues it (api.hip): checked once per call, launched per stream chunk.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mmd_amd.h"

namespace mmd {

// the arguments of a pick of n_robots x samples_per_robot samples, before any launch
int round_pick_check(const char* who, const mmd_guide_desc* env, const mmd_round_pick* p, const float* x_dev, int n_robots, int samples_per_robot);

// the two kernels for robots [robot_first, robot_first + n) of the call (whose samples are x_dev [n_robots * samples_per_robot, H, 4]) on `st`
int round_pick_launch(const mmd_guide_desc* env, const mmd_round_pick* p, const float* x_dev, int n_robots, int robot_first, int n,
                      int samples_per_robot, hipStream_t st);

}  // namespace mmd
