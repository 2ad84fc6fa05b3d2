// macjd_gru_bwd.hip — back-propagation through time of the learner's GRU scan (gfx950, wave64).
// C-ABI and the per-step formulas: include/macjd_nets.h (macjd_gru_bwd_io).
//
// The backward of macjd_gru_sequence is the same strictly serial chain run from t = T-1 down to 0: the gradient that
// reaches h_{t-1} through the recurrence (the "carry") is  g z + W_hh^T dgh[t].  Stock autograd walks it as T x (a dozen
// small launches); here it is ONE launch with W_hh^T resident in registers, like the forward scan.
//
// Mapping: one workgroup per sequence (b, j), NW = H / 16 waves (4 at H = 64, 8 at H = 128).  The forward's K-split
// layout with the roles swapped:
//   * lane l owns the OUTPUT columns k = l + 64 i (i < U = H / 64) of the mat-vec  W_hh^T dgh;
//   * wave w owns a slice of the 3H-long REDUCTION: the rows (g, u) of W_hh with u in [16 w, 16 w + 16), g = r, z, n —
//     48 rows, 48 U weight VGPRs per lane (48 at H = 64, 96 at H = 128), loaded once as coalesced 256-B pieces;
//   * the same 16 units are the ones whose gate derivatives wave w evaluates (lane l works on unit 16 w + (l & 15); the
//     four copies within a wave are bit-identical, lanes 0..15 store).  The 48 dgh values a wave multiplies are therefore
//     its OWN registers: they reach the FMAs as SGPR operands through v_readlane with a compile-time lane, and the
//     3H-vector dgh never crosses waves.  (An LDS hand-over of dgh would need a second barrier per step.)
//   * the NW partial sums per column meet in a double-buffered LDS tile, ONE barrier per step, and are added in fixed
//     wave order (deterministic, no atomics) by the wave that owns the unit — only for its 16 units;
//   * the rows of step t-1 and t-2 (gi, gh, h_{t-2}/h_{t-3}, dh: 8 values per lane) are requested ahead of the chain into
//     a three-slot register ring indexed at compile time (the time loop is unrolled by 3), as in the forward scan;
//   * every element of dgi / dgh / dh0 is written by exactly one wave (unit slices are disjoint).
// No private array is indexed at run time (all loops over weights / ring slots unroll): the ISA shows no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/macjd.h"
#include "../../include/macjd_nets.h"
#include "macjd_err.h"
#include "macjd_gru_math.h"

namespace macjd {

template <int H, int NW>
__global__ void __launch_bounds__(64 * NW) gru_sequence_backward_kernel(const macjd_gru_bwd_io io) {
    static_assert(H == 16 * NW, "one wave per 16 hidden units");
    constexpr int U = H / 64;    // output columns per lane
    constexpr int KW = 16;       // hidden units (x 3 gates = reduction rows) per wave
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seq = blockIdx.x;  // b * J + j
    const int b = seq / io.J, j = seq - b * io.J;
    const int T = io.T;
    const int u = wave * KW + (lane & (KW - 1));   // the unit whose gate derivatives this lane evaluates
    const bool writer = lane < KW;
    const float* __restrict__ gi = io.gi;
    const float* __restrict__ gh = io.gh;
    const float* __restrict__ hs = io.h_all;
    const float* __restrict__ dh = io.dh_all;
    const float* __restrict__ whh = io.w_hh;
    float* __restrict__ dgi = io.dgi;
    float* __restrict__ dgh = io.dgh;

    __shared__ float s_part[2][NW][H];

    // W_hh rows (g, 16 wave + kk), columns lane + 64 i: resident for the whole sequence
    float w[3][KW][U];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int kk = 0; kk < KW; ++kk)
#pragma unroll
            for (int i = 0; i < U; ++i)
                w[g][kk][i] = whh[(int64_t)(g * H + wave * KW + kk) * H + lane + 64 * i];

    const float* h0p = io.h0 ? io.h0 + (int64_t)b * (io.h0_sb ? io.h0_sb : (int64_t)io.J * H) + (int64_t)j * H + u : nullptr;
    auto row = [&](int t) -> int64_t { return ((int64_t)b * T + t) * io.J + j; };

    // ring[slot] = {gi_r, gi_z, gi_n, gh_r, gh_z, gh_n, h_prev, dh} of one step, for this lane's unit
    float ring[3][8];
    auto request = [&](auto slot_c, int t) {
        constexpr int S = decltype(slot_c)::value;
        const int64_t r3 = row(t) * (3 * H) + u;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            ring[S][g] = gi[r3 + g * H];
            ring[S][3 + g] = gh[r3 + g * H];
        }
        ring[S][7] = dh[row(t) * H + u];
        const float* hp = t > 0 ? hs + row(t - 1) * H + u : h0p;
        ring[S][6] = hp ? *hp : 0.0f;
    };
    request(std::integral_constant<int, 0>{}, T - 1);
    request(std::integral_constant<int, 1>{}, T > 1 ? T - 2 : 0);

    float gz = 0.0f;   // g z of the previous (later-in-time) step, this lane's unit: the carry's elementwise half

    // the recurrence half of the carry for unit u: the NW partial sums of the step before, in fixed wave order
    auto carry_sum = [&](int buf) {
        float c = 0.0f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) c += s_part[buf][ww][u];
        return c;
    };

    // one step of the reverse chain; s counts steps from the END (t = T-1-s), SLOT = s % 3 at compile time
    auto step = [&](auto slot_c, int s) {
        constexpr int SLOT = decltype(slot_c)::value;
        constexpr int PRE = (SLOT + 2) % 3;
        const int t = T - 1 - s;
        request(std::integral_constant<int, PRE>{}, t >= 2 ? t - 2 : 0);   // two steps ahead, off the serial chain

        const float carry = s > 0 ? gz + carry_sum((s - 1) & 1) : 0.0f;
        const float g = ring[SLOT][7] + carry;
        const float ghn = ring[SLOT][5];
        const float r = gru_sigmoid(ring[SLOT][0] + ring[SLOT][3]);
        const float z = gru_sigmoid(ring[SLOT][1] + ring[SLOT][4]);
        const float n = gru_tanh(ring[SLOT][2] + r * ghn);
        const float da_n = g * (1.0f - z) * (1.0f - n * n);
        const float da_z = g * (ring[SLOT][6] - n) * z * (1.0f - z);
        const float da_r = da_n * ghn * r * (1.0f - r);
        const float d[3] = {da_r, da_z, da_n * r};   // dgh of this unit
        gz = g * z;
        if (writer) {
            const int64_t r3 = row(t) * (3 * H) + u;
            dgi[r3] = da_r;         dgi[r3 + H] = da_z;     dgi[r3 + 2 * H] = da_n;
            dgh[r3] = d[0];         dgh[r3 + H] = d[1];     dgh[r3 + 2 * H] = d[2];
        }
        // this wave's 48 terms of  W_hh^T dgh  for the lane's columns
        float acc[U];
#pragma unroll
        for (int i = 0; i < U; ++i) acc[i] = 0.0f;
#pragma unroll
        for (int gg = 0; gg < 3; ++gg)
#pragma unroll
            for (int kk = 0; kk < KW; ++kk) {
                const float dk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d[gg]), kk));
#pragma unroll
                for (int i = 0; i < U; ++i) acc[i] = fmaf(w[gg][kk][i], dk, acc[i]);
            }
        const int buf = s & 1;
#pragma unroll
        for (int i = 0; i < U; ++i) s_part[buf][wave][lane + 64 * i] = acc[i];
        __syncthreads();
    };

    for (int s = 0; s < T; s += 3) {
        step(std::integral_constant<int, 0>{}, s);
        if (s + 1 < T) step(std::integral_constant<int, 1>{}, s + 1);
        if (s + 2 < T) step(std::integral_constant<int, 2>{}, s + 2);
    }
    if (io.dh0 && writer) io.dh0[(int64_t)seq * H + u] = gz + carry_sum((T - 1) & 1);
}

}  // namespace macjd

using namespace macjd;

extern "C" int macjd_gru_sequence_backward_supported(int32_t H) { return (H == 64 || H == 128) ? 1 : 0; }

extern "C" int macjd_gru_sequence_backward(const macjd_gru_bwd_io* io, void* hip_stream) {
    if (!io) return set_err(MACJD_EINVAL, "%s", "macjd_gru_sequence_backward: NULL io");
    if (io->B <= 0 || io->T <= 0 || io->J <= 0)
        return set_err(MACJD_EINVAL, "%s", "macjd_gru_sequence_backward: bad B / T / J");
    if (!io->gi || !io->gh || !io->h_all || !io->w_hh || !io->dh_all || !io->dgi || !io->dgh)
        return set_err(MACJD_EINVAL, "%s", "macjd_gru_sequence_backward: NULL pointer");
    if (io->h0_sb < 0) return set_err(MACJD_EINVAL, "%s", "macjd_gru_sequence_backward: negative h0 stride");
    if (!macjd_gru_sequence_backward_supported(io->H))
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_gru_sequence_backward: H must be 64 or 128");
    if ((int64_t)io->B * io->J > 2147483647LL)
        return set_err(MACJD_EINVAL, "%s", "macjd_gru_sequence_backward: more than 2^31 - 1 sequences");
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 g((unsigned)((int64_t)io->B * io->J));
    if (io->H == 64) hipLaunchKernelGGL((gru_sequence_backward_kernel<64, 4>), g, dim3(256), 0, s, *io);
    else hipLaunchKernelGGL((gru_sequence_backward_kernel<128, 8>), g, dim3(512), 0, s, *io);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_gru_sequence_backward: %s", hipGetErrorString(e));
    return MACJD_OK;
}
