// macjd_env_motion.hip — the env step of a MOVING scenario (include/macjd.h, macjd_motion_io).
//
// A translation unit of its own for the MOV instantiations of env_step_kernel (macjd_env_step.h, IO = MotionStepIO<...>):
// the per-env-table path of the step with the table column chosen by the env's step counter (frame-major tables, one
// contiguous block of MACJD_PE_ROWS doubles per env-step) and the position columns of the env's state row rewritten with the
// next frame's positions.  Every kernel built in macjd_env.hip compiles exactly as before.  The host side (validation, span
// checks, the many-step launch's counter advance) is in macjd_env.hip: launch_step_moving, the one dispatch function of the
// moving modes.
#include "macjd_env_step.h"

namespace macjd {

// position part of a reset (macjd_env_reset_moving): frame-0 positions into the masked envs' state rows
__global__ void env_reset_motion_kernel(int64_t n_envs, int n_pos, const float* __restrict__ positions,
                                        const int32_t* __restrict__ position_columns, float* state, int64_t st_se,
                                        const uint8_t* mask) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_envs; e += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[e]) continue;
        for (int i = 0; i < n_pos; ++i) state[e * st_se + position_columns[i]] = positions[i];
    }
}

// launch_motion_sized<FAST, SCAN = false, PAT = false>
MACJD_LAUNCH_MOTION(MotionStepIO<FastStepIO>) { return launch_motion_sized<true, false, false>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionStepIO<macjd_step_io>) { return launch_motion_sized<false, false, false>(J, R, grid, block, stream, dev, io); }

void launch_motion_reset(dim3 grid, dim3 block, hipStream_t stream, int64_t n_envs, int n_pos, const float* positions,
                         const int32_t* position_columns, float* state, int64_t st_se, const uint8_t* mask) {
    hipLaunchKernelGGL(env_reset_motion_kernel, grid, block, 0, stream, n_envs, n_pos, positions, position_columns, state, st_se,
                       mask);
}

}  // namespace macjd
