// Launch plan of an env_step_kernel launch (one lane per work item): a pure function of the batch, kept free of HIP so that a
// host compiler can build it (tests/env_plan_check.cpp).
#pragma once
#include <stdint.h>

namespace macjd {

// Small batches: one wave per workgroup spreads the envs over more CUs (latency-bound regime); from 2^16 items: 256-lane
// workgroups, tables staged once per workgroup.  The full grid (full_x, full_y) gives every item a lane of its own
// (production variants: no grid-stride loop), `strided` is the capped grid of the general variants' grid-stride loop.
// `blocks` counts the workgroups over all items (the production variants form their index from it in 32 bits).
struct LanePlan {
    int block;
    int64_t blocks, full_x;
    int32_t full_y;
    unsigned strided;
};

// many_T > 0: a many-step launch, many_T steps of each env as n_envs * many_T work items.  The block size follows the item
// count; the full grid is (envs / block, steps).
inline LanePlan lane_plan(int64_t n_envs, int32_t many_T) {
    const int64_t items = n_envs * (many_T > 0 ? many_T : 1);
    const int block = (items >= (1 << 16)) ? 256 : 64;
    const int64_t blocks = (items + block - 1) / block;
    // 64-lane workgroups need no cap: fewer than 2^16 items are at most 1024 of them
    const int64_t strided = (block == 256 && blocks > 256 * 8) ? 256 * 8 : blocks;
    return {block, blocks, many_T > 0 ? (n_envs + block - 1) / block : blocks, many_T > 0 ? many_T : 1, (unsigned)strided};
}

}  // namespace macjd
