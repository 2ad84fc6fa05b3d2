// macjd_tdlambda.h — the return scan of td_lambda_loss_kernel (macjd_nets.hip): lambda-returns of macjd_tdlambda_io
// (include/macjd_nets.h) by a suffix scan over affine maps, and the block sums of the loss against them.
//
// The recursion G[t] = r[t] + boot[t] ((1 - lam[t]) tq[t] + lam[t] G[t+1]) is the affine map G[t] = a[t] + c[t] G[t+1] with
//   a[t] = r[t] + (boot[t] (1 - lam[t])) tq[t],   c[t] = boot[t] lam[t]      (c[t] = 0 exactly at a stop)
// and maps compose: (a, c)_t o (a, c)_u = (a_t + c_t a_u, c_t c_u).
//
// Order of the arithmetic (the float32 model in tests/td_lambda_model.py restates it):
//   * wave w of the 16 takes the episodes w, w + 16, ..; an episode is walked in chunks of 64 steps from its LAST chunk to
//     its first, lane l holding step 64 chunk + l (lanes past Tm1 hold the identity-free stop a = 0, c = 0);
//   * inside a chunk six rounds k = 1, 2, 4, 8, 16, 32: lane l with l + k < 64 takes (a, c) of lane l + k and sets
//     a = fma(c, a', a) — skipped where c == 0, so nothing behind a stop is even multiplied — then c = c c';
//   * G = fma(c, carry, a) (again skipped where c == 0), carry = the G of lane 0 of the chunk behind (0 for the last one);
//   * the four sums (filled, e^2 with e = (y - G) filled, y, G): each thread adds its steps in the order it meets them
//     (episodes ascending, chunks descending), then wave_sum across the wave, then wave_sum over the 16 wave values by
//     wave 0 — no atomics, nothing depends on a workgroup count.
#pragma once
#include <hip/hip_runtime.h>

#include "macjd_tdloss.h"

namespace macjd {

struct tdl_chunk {   // one lane's operands of one (episode, chunk) item
    float r, tq, y, m;
    bool term, valid;
    int b, t;
};

__device__ __forceinline__ tdl_chunk tdl_load(const macjd_tdloss_io& io, const int item, const int n_chunks, const int wave,
                                              const int lane) {
    tdl_chunk c;
    const int e = item / n_chunks;
    c.b = wave + 16 * e;
    c.t = 64 * (n_chunks - 1 - (item - e * n_chunks)) + lane;
    c.valid = c.t < io.Tm1;
    c.r = c.tq = c.y = c.m = 0.0f;
    c.term = true;
    if (c.valid) {
        const int64_t b = c.b, t = c.t;
        c.r = io.reward[b * io.r_sb + t * io.r_st];
        c.tq = io.tq[b * io.tq_sb + t];
        c.y = io.y[b * io.y_sb + t];
        c.term = io.terminated[b * io.t_sb + t * io.t_st] != 0;
        c.m = io.filled[b * io.f_sb + t * io.f_st] ? 1.0f : 0.0f;
    }
    return c;
}

// compose the maps of the lanes l .. 63 of a chunk into lane l (inclusive suffix scan)
__device__ __forceinline__ void tdl_scan(float& a, float& c, const int lane) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const float a2 = __shfl_down(a, k, 64), c2 = __shfl_down(c, k, 64);
        if (lane + k < 64) {
            if (c != 0.0f) a = fmaf(c, a2, a);
            c *= c2;
        }
    }
}

// the four block sums of one workgroup of 16 waves -> tot4 (LDS), read by everybody after the second barrier
__device__ __forceinline__ void tdl_block_sums(const float (&q)[4], float (&s4)[4][16], float (&tot4)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = wave_sum(q[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s4[k][wave] = w[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = (lane < 16) ? s4[k][lane] : 0.0f;
            t = wave_sum(t);
            if (lane == 0) tot4[k] = t;
        }
    }
    __syncthreads();
}

}  // namespace macjd
