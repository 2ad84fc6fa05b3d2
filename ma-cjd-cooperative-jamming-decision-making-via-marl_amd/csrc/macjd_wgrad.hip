// macjd_wgrad.hip — split-K weight / bias gradient of a Linear layer on exact-f32 MFMA.  C-ABI: include/macjd_nets.h
//
//   dW[M,N] = gout[K,M]^T x inp[K,N]      db[M] = sum_k gout[k,:]
//
// In the learner's backward these products have tiny outputs (hyper-network and Q-head weights, 64..384 x 46..128)
// and a long reduction (K = B (T+1) = 3232 mixer rows, or B (T+1) J = 9696 agent rows).  A library GEMM tiles the
// OUTPUT, i.e. runs them on 6..12 workgroups for 25..50 us each; here the REDUCTION is tiled:
//   * grid = (N tiles, M tiles, K chunks), 64 x 64 output tile x 64-row chunk (WG_KC) per workgroup (4 waves as 2 x 2,
//     32 x 32 per wave = 2 x 2 accumulators of v_mfma_f32_16x16x4_f32);
//   * both operand chunks are staged into LDS with coalesced 16-byte loads, [WG_KC][80] floats each (row pitch
//     80 = 16 mod 32: the fragment reads `chunk[4 kk + (lane >> 4)][16 t + (lane & 15)]` of both operands hit 32
//     distinct banks per 32-lane group);
//   * the chunk's partial tile goes to workspace[chunk][M][N]; the bias partial (column sums of the staged gout
//     chunk) is produced by the workgroups of N-tile 0;
//   * wgrad_reduce_kernel sums the chunks in index order (deterministic, no float atomics).
// The grouped pair exists a second time (wgrad_*_many_norm_kernel, macjd_linear_wgrad_many_norm) for the learner's update:
// one problem contracted with a weight matrix into LayerNorm-parameter gradients in the partial launch's epilogue, the
// squares of every stored gradient and the optimiser's step counter in the reduce launch.  Its reduce launch has three
// kernels: slot sums only (wgrad_reduce_many_norm_kernel), with ROW PRODUCTS problems two global loads per lane and term
// (wgrad_reduce_many_rows_kernel) or — the default — blocks of 256 outputs on LDS-staged operand rows beside plain blocks
// (wgrad_reduce_rows_staged_kernel, block map in macjd_wgrad_map.h); the last two give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/macjd.h"
#include "../../include/macjd_nets.h"
#include "macjd_err.h"
#include "macjd_wgrad_map.h"

namespace macjd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#ifndef MACJD_WG_KC
#define MACJD_WG_KC 64    // rows of the reduction per work item: 41 KB of LDS, three workgroups per CU.  (128 rows = 82 KB = ONE
                          // workgroup per CU, whose load / multiply / store phases then never overlap another's: update 117.1 us
                          // vs 111.5; 32 rows: 115.9 — twice the partial tiles again.  With the one-lane-per-output reduce of
                          // round 2 the extra partials of 64-row items cost what the partial launch gained.)
#endif
#ifndef MACJD_WG_ABLATE
#define MACJD_WG_ABLATE 0   // timing-only builds (scripts/probe_wgrad.py): 1 no MFMA loop, 2 no global loads, 4 no partial store
#endif
#ifndef MACJD_WG_SUB
#define MACJD_WG_SUB 1      // WG_KC-row pieces per work item (2: piece s + 1 is loaded into registers while piece s is multiplied —
                            // measured slower on the update's problems: 18.3 vs 11.7 us, half the workgroups with twice the latency each)
#endif
constexpr int WG_BM = 64, WG_BN = 64, WG_KC = MACJD_WG_KC, WG_PITCH = 80, WG_SUB = MACJD_WG_SUB;
constexpr int WG_ROWS = WG_KC * WG_SUB;   // rows of the reduction per work item (= per partial tile in the workspace)

__host__ __device__ inline int64_t wg_pad(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// One problem as the kernels take it: macjd_wgrad_io without the fields only the host reads (kind, ext_chunks), so the
// argument blocks — and the code — of the launches that know no kinds are what they were before the kinds existed.
struct WgradDevIO {
    int64_t K;
    int32_t M, N;
    const float* gout; int64_t gout_ld;
    const float* inp;  int64_t inp_ld;
    float* dW;         int64_t dw_ld;
    float* db;
    float* workspace;
    const float* outer_vec;
    const float* outer_w;
};

inline WgradDevIO wg_dev(const macjd_wgrad_io& io) {
    WgradDevIO d;
    d.K = io.K; d.M = io.M; d.N = io.N; d.gout = io.gout; d.gout_ld = io.gout_ld; d.inp = io.inp; d.inp_ld = io.inp_ld;
    d.dW = io.dW; d.dw_ld = io.dw_ld; d.db = io.db; d.workspace = io.workspace; d.outer_vec = io.outer_vec; d.outer_w = io.outer_w;
    return d;
}

// fields of one problem as the partial-products body needs them (selected with compile-time indices from a batch)
struct WgradProb {
    int64_t K, gout_ld, inp_ld;
    int M, N, Mp, Np, n_chunks;
    const float* gout;
    const float* inp;
    float* workspace;
    bool want_db;
    const float* outer_vec;   // see macjd_wgrad_io
    const float* outer_w;
    const float* ln_W;        // LN bodies only: the problem is LayerNorm-contracted with this [M, N] matrix (macjd_wgrad_norm_io)
    int64_t ln_ld;
};

// LN: the body of the launch that knows LayerNorm-contracted problems (io.ln_W != nullptr, uniform per work item); the
// LN = false instantiation is the kernels' code as it was before that launch existed
template <bool LN>
__device__ __forceinline__ void wgrad_partial_body(const WgradProb& io, const int tn, const int tm, const int chunk,
                                                   float* __restrict__ sA, float* __restrict__ sB) {
    const int Mp = io.Mp, Np = io.Np;
    const int m0 = tm * WG_BM, n0 = tn * WG_BN;
    const int64_t k0 = (int64_t)chunk * WG_ROWS;
    const int tid = threadIdx.x;
    // ---- a WG_KC-row piece of both operands: 64 columns, 16 threads per row, 16-byte loads where aligned.  The piece is
    // loaded into registers (8 x 2 float4 per thread) and written to LDS in a second step, so that the loads of piece
    // s + 1 are in flight while piece s is multiplied (measured on the update's seven problems: loads ~10 us and MFMA
    // ~8 us of the launch were additive when each work item was load -> barrier -> multiply) ----
    // All loads are branch-free: rows past K and columns past M / N are read from CLAMPED (valid) addresses and zeroed by
    // selects afterwards.  A load under a divergent `if` makes hipcc wait for ALL outstanding loads at the join — the
    // first version guarded every element and so serialised its 8 x 2 row pieces, one memory latency after the other.
    // Width of a load is uniform per operand: 16 bytes (rows 16-byte aligned, tile inside the matrix), 8 bytes (even row
    // length: a column pair is inside or outside as a whole) or 4.
    constexpr int NIT = (WG_KC * 16) / 256;
    float4 va[NIT], vb[NIT];
    auto load_operand = [&](const float* __restrict__ base, const int64_t ld, const int cols, const int c0, const int piece,
                            float4* __restrict__ out) {
        const bool al16 = ((ld & 3) == 0) && ((((uintptr_t)base) & 15) == 0) && (c0 + 64 <= cols);
        const bool al8 = ((ld & 1) == 0) && ((cols & 1) == 0) && ((((uintptr_t)base) & 7) == 0) && cols >= 2;
        const int c4 = (tid & 15) * 4;
        int64_t roff[NIT];
        bool rok[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int64_t k = k0 + (int64_t)piece * WG_KC + ((it * 256 + tid) >> 4);
            rok[it] = k < io.K && !(MACJD_WG_ABLATE & 2);
            roff[it] = (k < io.K ? k : io.K - 1) * ld;
        }
        if (al16) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) out[it] = *reinterpret_cast<const float4*>(base + roff[it] + c0 + c4);
        } else if (al8) {
            const int ca = c0 + c4 < cols ? c0 + c4 : cols - 2, cb = c0 + c4 + 2 < cols ? c0 + c4 + 2 : cols - 2;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const float2 lo = *reinterpret_cast<const float2*>(base + roff[it] + ca);
                const float2 hi = *reinterpret_cast<const float2*>(base + roff[it] + cb);
                out[it] = float4{lo.x, lo.y, hi.x, hi.y};
            }
        } else {
            int cc[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) cc[e] = c0 + c4 + e < cols ? c0 + c4 + e : cols - 1;
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                out[it] = float4{base[roff[it] + cc[0]], base[roff[it] + cc[1]], base[roff[it] + cc[2]], base[roff[it] + cc[3]]};
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            out[it].x = (rok[it] && c0 + c4 + 0 < cols) ? out[it].x : 0.0f;
            out[it].y = (rok[it] && c0 + c4 + 1 < cols) ? out[it].y : 0.0f;
            out[it].z = (rok[it] && c0 + c4 + 2 < cols) ? out[it].z : 0.0f;
            out[it].w = (rok[it] && c0 + c4 + 3 < cols) ? out[it].w : 0.0f;
        }
    };
    auto load_piece = [&](const int piece) {
        load_operand(io.gout, io.gout_ld, io.M, m0, piece, va);
        load_operand(io.inp, io.inp_ld, io.N, n0, piece, vb);
        if (io.outer_vec) {   // (uniform) operand formed on the fly: (relu output > 0) ? vec[k] * w[m] : 0 — the very
            const int c4 = (tid & 15) * 4;   // expression of splitrelu_backward_kernel, so the products are bit-identical
            float w4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) w4[e] = io.outer_w[m0 + c4 + e < io.M ? m0 + c4 + e : io.M - 1];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int64_t k = k0 + (int64_t)piece * WG_KC + ((it * 256 + tid) >> 4);
                const float gv = io.outer_vec[k < io.K ? k : io.K - 1];
                va[it].x = (va[it].x > 0.0f) ? gv * w4[0] : 0.0f;
                va[it].y = (va[it].y > 0.0f) ? gv * w4[1] : 0.0f;
                va[it].z = (va[it].z > 0.0f) ? gv * w4[2] : 0.0f;
                va[it].w = (va[it].w > 0.0f) ? gv * w4[3] : 0.0f;
            }
        }
    };
    auto store_piece = [&]() {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = it * 256 + tid;
            const int r = idx >> 4, c4 = (idx & 15) * 4;
            *reinterpret_cast<float4*>(&sA[r * WG_PITCH + c4]) = va[it];
            *reinterpret_cast<float4*>(&sB[r * WG_PITCH + c4]) = vb[it];
        }
    };
    // ---- 32 x 32 per wave: acc[sm][sn] += A^T fragment x B fragment over the work item's rows ----
    const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* pa = sA + lk * WG_PITCH + wm + li;
    const float* pb = sB + lk * WG_PITCH + wn + li;
    bool contract = false;
    if constexpr (LN) contract = io.ln_W != nullptr;
    const bool bias_lane = (io.want_db || contract) && tn == 0 && tid < WG_BM;
    float bias_sum = 0.0f;
    // contracted problem: the 16 elements of W under this lane's accumulators, loaded here — before the products — from
    // clamped addresses and zeroed past M / N by selects (any other problem: 16 reads of one valid address, unused)
    float wl[2][2][4];
    if constexpr (LN) {
        const float* wbase = contract ? io.ln_W : io.gout;
        const int64_t wld = contract ? io.ln_ld : 0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + a * 16 + lk * 4 + r, n = n0 + wn + b * 16 + li;
                    const int mc = m < io.M ? m : io.M - 1, nc = n < io.N ? n : io.N - 1;
                    const float v = wbase[(int64_t)mc * wld + (contract ? nc : 0)];
                    wl[a][b][r] = (contract && m < io.M && n < io.N) ? v : 0.0f;
                }
    }
    // (LN bodies say what the expression amounts to with one piece per work item — k0 < K for every chunk: the loop's
    // "more" half, and the registers of a second piece in flight, then do not exist and the 16 values of W fit beside
    // the rest at three workgroups per CU)
    const int n_pieces = (LN && WG_SUB == 1) ? 1
        : (int)((((io.K - k0) < (int64_t)WG_ROWS ? (io.K - k0) : (int64_t)WG_ROWS) + WG_KC - 1) / WG_KC);
    load_piece(0);
    store_piece();
    __syncthreads();
    for (int piece = 0; piece < n_pieces; ++piece) {
        const bool more = piece + 1 < n_pieces;
        if (more) load_piece(piece + 1);       // in flight during the products below
        // Two fragment sets, ping-ponged and PINNED (as in macjd_mlp.hip): the four ds_reads of k-step kk + 1 are issued
        // right behind the first MFMA of k-step kk and consumed one step later, so their LDS latency hides behind three
        // MFMAs of 32 cycles.  Left alone the scheduler sinks every read next to its use: read -> lgkmcnt(0) -> 4 MFMA per
        // k-step, which ran the loop at a third of the MFMA rate (PMC, round 3, profiles/r03_wgrad_pmc.txt:
        // SQ_VALU_MFMA_BUSY_CYCLES = 4 096 per wave = the ideal 128 x 32, but 12 900 cycles of issue stall per wave).
        constexpr int KSTEPS = (MACJD_WG_ABLATE & 1) ? 2 : WG_KC / 4;
        float fa0 = pa[0], fa1 = pa[16], fb0 = pb[0], fb1 = pb[16];
        float ga0, ga1, gb0, gb1;
#pragma unroll 4
        for (int kk = 0; kk < KSTEPS; kk += 2) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0, fb0, acc[0][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            ga0 = pa[(kk + 1) * 4 * WG_PITCH]; ga1 = pa[(kk + 1) * 4 * WG_PITCH + 16];
            gb0 = pb[(kk + 1) * 4 * WG_PITCH]; gb1 = pb[(kk + 1) * 4 * WG_PITCH + 16];
            __builtin_amdgcn_sched_barrier(0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0, fb1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1, fb0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1, fb1, acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga0, gb0, acc[0][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            const int kn = (kk + 2 < KSTEPS) ? kk + 2 : KSTEPS - 1;   // past the end: re-read (unused)
            fa0 = pa[kn * 4 * WG_PITCH]; fa1 = pa[kn * 4 * WG_PITCH + 16];
            fb0 = pb[kn * 4 * WG_PITCH]; fb1 = pb[kn * 4 * WG_PITCH + 16];
            __builtin_amdgcn_sched_barrier(0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga0, gb1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga1, gb0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga1, gb1, acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // bias partial: column sums of the staged gout piece (N-tile 0 only), pieces added in order
        if (bias_lane) {
            float sp = 0.0f;
#pragma unroll 8
            for (int r = 0; r < WG_KC; ++r) sp += sA[r * WG_PITCH + tid];
            bias_sum += sp;
        }
        if (more) {
            __syncthreads();                   // every wave is done reading this piece
            store_piece();
            __syncthreads();
        }
    }
    if constexpr (LN) {
        if (contract) {   // (one N tile: n0 = 0) sum over this work item's 64 rows of W G_part and of W gb_part, fixed order
            __syncthreads();                       // every wave is done with the staged pieces: their LDS is reused
            float* gbs = sA;                       // [64] column sums of the gout piece = gb_part of rows m0 ..
            float* red = sB;                       // [2 row halves][dgamma, dbeta][64]
            if (tid < WG_BM) gbs[tid] = bias_sum;
            __syncthreads();
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float sg = 0.0f, sb = 0.0f;        // registers: a = 0 (r = 0..3), a = 1 (r = 0..3)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sg = fmaf(wl[a][b][r], acc[a][b][r], sg);
                        sb = fmaf(wl[a][b][r], gbs[wm + a * 16 + lk * 4 + r], sb);
                    }
                sg += __shfl_xor(sg, 16, 64); sg += __shfl_xor(sg, 32, 64);   // the four row groups of a wave: (g0 + g1) + (g2 + g3)
                sb += __shfl_xor(sb, 16, 64); sb += __shfl_xor(sb, 32, 64);
                if (lk == 0) {
                    red[((wave >> 1) * 2 + 0) * WG_BN + wn + b * 16 + li] = sg;
                    red[((wave >> 1) * 2 + 1) * WG_BN + wn + b * 16 + li] = sb;
                }
            }
            __syncthreads();
            if (tid < 2 * WG_BN) {                 // the two row halves: upper + lower
                const int which = tid >> 6, n = tid & 63;
                const float v = red[which * WG_BN + n] + red[(2 + which) * WG_BN + n];
                if (n < io.N) io.workspace[((int64_t)tm * io.n_chunks + chunk) * 2 * io.N + which * io.N + n] = v;
            }
            return;
        }
    }
    float* ws = io.workspace + (int64_t)chunk * Mp * Np;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + a * 16 + lk * 4 + r;   // C layout: row = (lane >> 4) * 4 + reg
                const int n = n0 + wn + b * 16 + li;           //           col = lane & 15
                if (!(MACJD_WG_ABLATE & 4) || acc[a][b][r] == 12345.678f) ws[(int64_t)m * Np + n] = acc[a][b][r];
            }
    if (bias_lane) io.workspace[(int64_t)io.n_chunks * Mp * Np + (int64_t)chunk * Mp + m0 + tid] = bias_sum;
}

// sum over the 64 lanes (every lane gets it): x + lane^32, then ^16 .. ^1 — the order of the optimiser's wave_sum
__device__ __forceinline__ float wgrad_wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__global__ void __launch_bounds__(256) wgrad_partial_kernel(const WgradDevIO io, const int Mp, const int Np) {
    __shared__ float sA[WG_KC * WG_PITCH];   // gout chunk  [k][m]
    __shared__ float sB[WG_KC * WG_PITCH];   // inp chunk   [k][n]
    WgradProb p;
    p.K = io.K; p.gout_ld = io.gout_ld; p.inp_ld = io.inp_ld; p.M = io.M; p.N = io.N; p.Mp = Mp; p.Np = Np;
    p.n_chunks = (int)gridDim.z; p.gout = io.gout; p.inp = io.inp; p.workspace = io.workspace; p.want_db = io.db != nullptr;
    p.outer_vec = io.outer_vec; p.outer_w = io.outer_w;
    wgrad_partial_body<false>(p, blockIdx.x, blockIdx.y, blockIdx.z, sA, sB);
}

// Sum of the K-chunk partials, fixed order (deterministic).  A workgroup owns 64 consecutive output elements; consecutive
// lanes = consecutive n (every load instruction of a wave reads one contiguous row piece of a partial tile); the chunks
// are taken in rounds of eight and round r belongs to wave r mod 4, so an output's <= 76 loads are in flight from four
// waves at once instead of queueing behind one lane (one lane per output: 12.6 us for the update's problems, a
// latency chain of ten rounds).  Order of the sum: wave w adds chunk 8 r + s (r = w, w + 4, ...) into its accumulator s,
// combines ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); the four waves' sums meet as (p0 + p1) + (p2 + p3).
__device__ __forceinline__ float wgrad_sum_rounds(const float* __restrict__ p, const int64_t stride, const int n_chunks, const int wave) {
    float a[8];
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) a[s8] = 0.0f;
    for (int c = 8 * wave; c < n_chunks; c += 32) {
        float v[8];
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) {   // (no branch around a load: past the last chunk the last chunk is read and dropped)
            const int cc = c + s8 < n_chunks ? c + s8 : n_chunks - 1;
            v[s8] = p[(int64_t)cc * stride];
        }
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) a[s8] += (c + s8 < n_chunks) ? v[s8] : 0.0f;
    }
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

constexpr int WG_RED = 64;   // outputs per reduce workgroup

// the four waves' sums of output `lane` -> the value (valid in wave 0)
__device__ __forceinline__ float wgrad_meet(float (*part)[WG_RED], const float mine, const int wave, const int lane) {
    part[wave][lane] = mine;
    __syncthreads();
    const float out = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    __syncthreads();   // (the caller's loop writes `part` again)
    return out;
}

__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const WgradDevIO io, const int Mp, const int Np,
                                                           const int n_chunks) {
    __shared__ float part[4][WG_RED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)io.M * io.N, all = total + (io.db ? io.M : 0);
    for (int64_t i0 = (int64_t)blockIdx.x * WG_RED; i0 < all; i0 += (int64_t)gridDim.x * WG_RED) {
        const int64_t i = i0 + lane < all ? i0 + lane : all - 1;   // (lanes past the end repeat the last output, never store)
        const float* src;
        int64_t stride;
        float* dst;
        if (i < total) {
            const int m = (int)(i / io.N), n = (int)(i - (int64_t)m * io.N);
            src = io.workspace + (int64_t)m * Np + n; stride = (int64_t)Mp * Np; dst = io.dW + (int64_t)m * io.dw_ld + n;
        } else {
            const int m = (int)(i - total);
            src = io.workspace + (int64_t)n_chunks * Mp * Np + m; stride = Mp; dst = io.db + m;
        }
        const float v = wgrad_meet(part, wgrad_sum_rounds(src, stride, n_chunks, wave), wave, lane);
        if (wave == 0 && i0 + lane < all) *dst = v;
    }
}

// ---- several problems in one launch pair (the backward pass of the learner defers its weight gradients) ----
struct WgradBatch {
    WgradDevIO io[MACJD_WGRAD_MAX_BATCH];
    int Mp[MACJD_WGRAD_MAX_BATCH], Np[MACJD_WGRAD_MAX_BATCH], chunks[MACJD_WGRAD_MAX_BATCH];
    int tiles_n[MACJD_WGRAD_MAX_BATCH], tiles_m[MACJD_WGRAD_MAX_BATCH];
    int64_t wg_start[MACJD_WGRAD_MAX_BATCH + 1];    // prefix of workgroups (tile x chunk work items) per problem
    int64_t out_start[MACJD_WGRAD_MAX_BATCH + 1];   // prefix of reduce work items (M N + M outputs) per problem
    int n;
};

// workgroup w works on problem p with wg_start[p] <= w < wg_start[p + 1]; the problem's fields are picked with
// compile-time indices only (a run-time index into the by-value table would copy the ~1 KB struct to scratch)
__global__ void __launch_bounds__(256) wgrad_partial_many_kernel(const WgradBatch b) {
    __shared__ float sA[WG_KC * WG_PITCH];
    __shared__ float sB[WG_KC * WG_PITCH];
    const int64_t w = blockIdx.x;
    WgradProb p;
    int tiles_n = b.tiles_n[0], tiles_m = b.tiles_m[0];
    int64_t start = 0;
#define MACJD_PICK(q)                                                                                               \
    p.K = b.io[q].K; p.gout_ld = b.io[q].gout_ld; p.inp_ld = b.io[q].inp_ld; p.M = b.io[q].M; p.N = b.io[q].N;       \
    p.Mp = b.Mp[q]; p.Np = b.Np[q]; p.n_chunks = b.chunks[q]; p.gout = b.io[q].gout; p.inp = b.io[q].inp;            \
    p.workspace = b.io[q].workspace; p.want_db = b.io[q].db != nullptr; tiles_n = b.tiles_n[q]; tiles_m = b.tiles_m[q]; \
    p.outer_vec = b.io[q].outer_vec; p.outer_w = b.io[q].outer_w;                                                    \
    start = b.wg_start[q];
    MACJD_PICK(0)
#pragma unroll
    for (int q = 1; q < MACJD_WGRAD_MAX_BATCH; ++q) {
        if (q < b.n && w >= b.wg_start[q]) { MACJD_PICK(q) }
    }
    const int local = (int)(w - start);
    const int tn = local % tiles_n, rest = local / tiles_n;
    const int tm = rest % tiles_m, chunk = rest / tiles_m;
    wgrad_partial_body<false>(p, tn, tm, chunk, sA, sB);
}

__global__ void __launch_bounds__(256) wgrad_reduce_many_kernel(const WgradBatch b) {
    __shared__ float part[4][WG_RED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total_all = b.out_start[b.n];
    for (int64_t g0 = (int64_t)blockIdx.x * WG_RED; g0 < total_all; g0 += (int64_t)gridDim.x * WG_RED) {
        const int64_t g = g0 + lane < total_all ? g0 + lane : total_all - 1;
        int M = b.io[0].M, N = b.io[0].N, Mp = b.Mp[0], Np = b.Np[0], n_chunks = b.chunks[0];
        int64_t start = 0, dw_ld = b.io[0].dw_ld;
        const float* workspace = b.io[0].workspace;
        float* dW = b.io[0].dW;
        float* db = b.io[0].db;
#pragma unroll
        for (int q = 1; q < MACJD_WGRAD_MAX_BATCH; ++q) {
            if (q < b.n && g >= b.out_start[q]) {
                M = b.io[q].M; N = b.io[q].N; Mp = b.Mp[q]; Np = b.Np[q]; n_chunks = b.chunks[q];
                start = b.out_start[q]; dw_ld = b.io[q].dw_ld; workspace = b.io[q].workspace; dW = b.io[q].dW; db = b.io[q].db;
            }
        }
        const int64_t i = g - start;
        const int64_t total = (int64_t)M * N;
        // (a problem without a bias output still owns M items behind its M N: they are summed and dropped)
        const bool is_w = i < total;
        const int m = is_w ? (int)(i / N) : (int)(i - total);
        const int n = is_w ? (int)(i - (int64_t)m * N) : 0;
        const float* src = is_w ? workspace + (int64_t)m * Np + n : workspace + (int64_t)n_chunks * Mp * Np + m;
        const float v = wgrad_meet(part, wgrad_sum_rounds(src, is_w ? (int64_t)Mp * Np : (int64_t)Mp, n_chunks, wave), wave, lane);
        if (wave == 0 && g0 + lane < total_all) {
            if (is_w) dW[(int64_t)m * dw_ld + n] = v;
            else if (db) db[m] = v;
        }
    }
}

// ---- the grouped launch pair that also serves the optimiser step (include/macjd_nets.h, macjd_wgrad_norm_io) ----
struct WgradNorm {
    int problem;             // the LayerNorm-contracted problem (-1: none)
    int slots;               // its tiles_m * n_chunks partial slots of [2][N]
    const float* W; int64_t w_ld;
    float* dgamma; float* dbeta;
    float* partials; float* step;
};

__global__ void __launch_bounds__(256) wgrad_partial_many_norm_kernel(const WgradBatch b, const WgradNorm ln) {
    __shared__ float sA[WG_KC * WG_PITCH];
    __shared__ float sB[WG_KC * WG_PITCH];
    const int64_t w = blockIdx.x;
    WgradProb p;
    int tiles_n = b.tiles_n[0], tiles_m = b.tiles_m[0];
    int64_t start = 0;
    MACJD_PICK(0)
    p.ln_W = ln.problem == 0 ? ln.W : nullptr;
#pragma unroll
    for (int q = 1; q < MACJD_WGRAD_MAX_BATCH; ++q) {
        if (q < b.n && w >= b.wg_start[q]) { MACJD_PICK(q) p.ln_W = ln.problem == q ? ln.W : nullptr; }
    }
    p.ln_ld = ln.w_ld;
    const int local = (int)(w - start);
    const int tn = local % tiles_n, rest = local / tiles_n;
    const int tm = rest % tiles_m, chunk = rest / tiles_m;
    wgrad_partial_body<true>(p, tn, tm, chunk, sA, sB);
}
#undef MACJD_PICK

// wgrad_reduce_many_kernel with (1) the contracted problem's 2 N outputs (item i = which * N + n sums element i of its
// `slots` slots of 2 N floats), (2) partials[workgroup] = sum of the squares of what the workgroup stored: per lane of
// wave 0 in item order, then wgrad_wave_sum, (3) the step counter.
//
// ROWS (wgrad_reduce_many_rows_kernel): problems whose bit is set in `rows_mask` are ROW PRODUCTS — term k of output (m, n)
// is gout[k, m] * inp[k, n] (bias output: gout[k, m]) read from the operands, b.chunks[] = K terms.  Every lane loads two
// values per term, (slot value, itself) or (gout, inp), and adds fmaf(first, second-or-1, acc): for a slot value that is
// acc + value, the very sum of the other instantiation.
__device__ __forceinline__ float wgrad_sum_rounds_rows(const float* __restrict__ pa, const int64_t sa, const float* __restrict__ pb,
                                                       const int64_t sb, const bool two, const int n_terms, const int wave) {
    float a[8];
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) a[s8] = 0.0f;
    for (int c = 8 * wave; c < n_terms; c += 32) {
        float v[8], x[8];
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) {   // (no branch around a load: past the last term the last term is read and dropped)
            const int cc = c + s8 < n_terms ? c + s8 : n_terms - 1;
            v[s8] = pa[(int64_t)cc * sa];
            x[s8] = pb[(int64_t)cc * sb];
        }
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) a[s8] = fmaf((c + s8 < n_terms) ? v[s8] : 0.0f, two ? x[s8] : 1.0f, a[s8]);
    }
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// MAPPED (the staged kernel's plain blocks): the body runs as block `mblock` of `mblocks`; else as its workgroup of the grid
template <bool ROWS, bool MAPPED = false>
__device__ __forceinline__ void wgrad_reduce_norm_body(const WgradBatch& b, const WgradNorm& ln, const unsigned rows_mask,
                                                       const unsigned mblock = 0, const unsigned mblocks = 0) {
    __shared__ float part[4][WG_RED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total_all = b.out_start[b.n];
    float sq = 0.0f;
    for (int64_t g0 = (int64_t)(MAPPED ? mblock : blockIdx.x) * WG_RED; g0 < total_all; g0 += (int64_t)(MAPPED ? mblocks : gridDim.x) * WG_RED) {
        const int64_t g = g0 + lane < total_all ? g0 + lane : total_all - 1;
        int M = b.io[0].M, N = b.io[0].N, Mp = b.Mp[0], Np = b.Np[0], n_chunks = b.chunks[0], prob = 0;
        int64_t start = 0, dw_ld = b.io[0].dw_ld;
        const float* workspace = b.io[0].workspace;
        float* dW = b.io[0].dW;
        float* db = b.io[0].db;
#pragma unroll
        for (int q = 1; q < MACJD_WGRAD_MAX_BATCH; ++q) {
            if (q < b.n && g >= b.out_start[q]) {
                M = b.io[q].M; N = b.io[q].N; Mp = b.Mp[q]; Np = b.Np[q]; n_chunks = b.chunks[q]; prob = q;
                start = b.out_start[q]; dw_ld = b.io[q].dw_ld; workspace = b.io[q].workspace; dW = b.io[q].dW; db = b.io[q].db;
            }
        }
        const int64_t i = g - start;
        const int64_t total = (int64_t)M * N;
        const bool is_ln = prob == ln.problem;
        const bool is_w = i < total;
        const int m = is_w ? (int)(i / N) : (int)(i - total);
        const int n = is_w ? (int)(i - (int64_t)m * N) : 0;
        const float* src = is_ln ? workspace + i : is_w ? workspace + (int64_t)m * Np + n : workspace + (int64_t)n_chunks * Mp * Np + m;
        const int64_t stride = is_ln ? (int64_t)2 * N : is_w ? (int64_t)Mp * Np : (int64_t)Mp;
        float mine;
        if constexpr (ROWS) {
            const float* gout = b.io[0].gout;
            const float* inp = b.io[0].inp;
            int64_t gout_ld = b.io[0].gout_ld, inp_ld = b.io[0].inp_ld;
#pragma unroll
            for (int q = 1; q < MACJD_WGRAD_MAX_BATCH; ++q) {
                if (q == prob) { gout = b.io[q].gout; inp = b.io[q].inp; gout_ld = b.io[q].gout_ld; inp_ld = b.io[q].inp_ld; }
            }
            const bool rows = ((rows_mask >> prob) & 1u) != 0;   // (never the contracted problem)
            const bool two = rows && is_w;
            const float* pa = rows ? gout + m : src;
            const int64_t sa = rows ? gout_ld : stride;
            mine = wgrad_sum_rounds_rows(pa, sa, two ? inp + n : pa, two ? inp_ld : sa, two, is_ln ? ln.slots : n_chunks, wave);
        } else {
            mine = wgrad_sum_rounds(src, stride, is_ln ? ln.slots : n_chunks, wave);
        }
        const float v = wgrad_meet(part, mine, wave, lane);
        if (wave == 0 && g0 + lane < total_all) {
            // (a problem without a bias output still owns M items behind its M N: summed, dropped, and not counted)
            float* dst = is_ln ? (i < N ? ln.dgamma + i : ln.dbeta + (i - N)) : is_w ? dW + (int64_t)m * dw_ld + n : db ? db + m : nullptr;
            if (dst) {
                *dst = v;
                sq = fmaf(v, v, sq);
            }
        }
    }
    if (wave == 0) {
        sq = wgrad_wave_sum(sq);
        if (lane == 0) {
            ln.partials[MAPPED ? mblock : blockIdx.x] = sq;
            if ((MAPPED ? mblock : blockIdx.x) == 0) ln.step[0] += 1.0f;   // nothing in this launch reads it; the optimiser launch reads the advanced value
        }
    }
}

__global__ void __launch_bounds__(256) wgrad_reduce_many_norm_kernel(const WgradBatch b, const WgradNorm ln) {
    wgrad_reduce_norm_body<false>(b, ln, 0u);
}

__global__ void __launch_bounds__(256) wgrad_reduce_many_rows_kernel(const WgradBatch b, const WgradNorm ln, const unsigned rows_mask) {
    wgrad_reduce_norm_body<true>(b, ln, rows_mask);
}

// ---- ROWS reduce, staged form (wgrad_reduce_rows_staged_kernel; block map: macjd_wgrad_map.h) ----
// A FAST block owns 256 consecutive weight items of one ROW PRODUCTS problem = four groups of 64, thread = item.  The `inp`
// rows [k][0, N) and the <= WGMAP_GCOLS `gout` columns of the block's items are staged once per block into LDS in slices
// of RS_KS terms (compact: row pitch N resp. WGMAP_GCOLS), so a term costs two ds_read_b32 and one fmaf per lane instead of
// two global loads behind a per-lane 64-bit address.  The slice behind the one being consumed is in flight in registers.
// Arithmetic per output is that of wgrad_sum_rounds_rows + wgrad_meet: term t goes into accumulator t % 32 (= "wave"
// (t / 8) % 4, slot t % 8) in increasing t, each eight combine as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)), the
// four sums meet as (p0 + p1) + (p2 + p3); one thread holds all 32.  Terms past K are SKIPPED; the plain kernel adds
// fmaf(0, last row's value, acc) there, which for finite operands leaves the same bits (acc + (+-0) = acc; an acc of -0
// would turn +0, and -0 == +0 in every later sum's value).  Wave j stores groups0 + j and writes its partial like wave 0
// of a plain block: fmaf(v, v, 0) per lane, wgrad_wave_sum.
// Global reads: element (k, col) only for k < K and col < N resp. inside the block's columns — lanes without an element
// re-read the slice's last valid row (no branch around a load) and do not write LDS; the products never read an LDS word
// that was not written for the current slice.  16-byte loads only where the host found base, ld and N multiples of 16
// bytes (vec, uniform per problem); else dwords.
#ifndef MACJD_RS_KS
#define MACJD_RS_KS 32      // terms per staged slice (a multiple of 32).  Measured on the benchmark's seven problems (K = 224), one visit:
                            //   32: 115 VGPRs, 17 KB of LDS, reduce launch alone back to back 10.2 us, 77.4 us per update
                            //   64: 144 VGPRs, 34 KB, 9.8 us alone, 77.7 us per update;  96: 227 VGPRs, 51 KB, 10.0 us, 78.3
                            // (the plain rows kernel: 14.6 us alone, 81.0 us per update; timing-only builds of the 64-term form whose
                            // fast blocks skipped their products, or their global loads: 10.0 each — what is left is the plain
                            // blocks' slot sums).  224, the whole K in flight, needs more than 256 registers
#endif
constexpr int RS_KS = MACJD_RS_KS;                          // at 32: 16 KB + 1 KB of LDS, 16 + 1 registers in flight
constexpr int RS_NIT = RS_KS * WGMAP_N_CAP / 256;           // floats of `inp` per thread and slice at N = WGMAP_N_CAP
constexpr int RS_GIT = (RS_KS * WGMAP_GCOLS + 255) / 256;   // floats of `gout` per thread and slice
constexpr int RS_LDS_BYTES = RS_KS * (WGMAP_N_CAP + WGMAP_GCOLS) * 4;
static_assert(RS_KS % 32 == 0 && WGMAP_N_CAP == 128 && WGMAP_GCOLS == 8, "a slice starts on accumulator 0; the staging maps");
static_assert(RS_LDS_BYTES <= 64 * 1024, "above the default limit of dynamic LDS the launch would need hipFuncSetAttribute");

struct RowsFastProb {
    const float* gout; const float* inp; float* dW;
    int64_t gout_ld, inp_ld, dw_ld, start;
    int K, N;
};

// VEC: 16-byte staging loads; WIDE (dword staging only): N > 64, a second column per lane
template <bool VEC, bool WIDE>
__device__ __forceinline__ void wgrad_rows_staged_body(const RowsFastProb& p, const int group0, const WgradNorm& ln,
                                                       float* __restrict__ sx, float* __restrict__ sg) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = p.N, K = p.K;
    const int i0 = group0 * WG_RED - (int)p.start;   // the block's first item inside the problem (uniform; < 64 * 8192)
    const int m_lo = i0 / N, gcols = (i0 + WGMAP_FAST_ITEMS - 1) / N - m_lo + 1;
    const int m = (i0 + tid) / N, n = i0 + tid - m * N;
    // Staging of a slice goes by rows, so no lane divides.  VEC: a float4 per lane, two rows per wave and load (lanes
    // 0..31 / 32..63), row 8 it + 2 wave + (lane >> 5); else a float per lane at columns lane and lane + 64, one row per wave
    // and load, row 4 it + wave.  Every load is unconditional (a load under a condition, even a uniform one, makes hipcc
    // copy the register array behind it and wait for the load first): a row past the slice's last is re-read from the last
    // valid row, a column past N from column N - 1; neither is written to LDS.
    const int W = N >> 2, half = lane >> 5, c4 = lane & 31;
    float pre[RS_NIT], gpre[RS_GIT];
    auto load_slice = [&](const int k0) {
        const int rows = K - k0 < RS_KS ? K - k0 : RS_KS;
        if constexpr (VEC) {
            const int cc = c4 < W ? c4 : W - 1;
#pragma unroll
            for (int it = 0; it < RS_KS / 8; ++it) {
                const int r = it * 8 + wave * 2 + half, rc = r < rows ? r : rows - 1;
                const float4 v = *reinterpret_cast<const float4*>(p.inp + (int64_t)(k0 + rc) * p.inp_ld + 4 * cc);
                pre[4 * it] = v.x; pre[4 * it + 1] = v.y; pre[4 * it + 2] = v.z; pre[4 * it + 3] = v.w;
            }
        } else {
            const int ca = lane < N ? lane : N - 1, cb = lane + 64 < N ? lane + 64 : N - 1;
#pragma unroll
            for (int it = 0; it < RS_KS / 4; ++it) {
                const int r = it * 4 + wave, rc = r < rows ? r : rows - 1;
                const float* row = p.inp + (int64_t)(k0 + rc) * p.inp_ld;
                pre[2 * it] = row[ca];
                if constexpr (WIDE) pre[2 * it + 1] = row[cb];
            }
        }
#pragma unroll
        for (int it = 0; it < RS_GIT; ++it) {
            const int e = it * 256 + tid, gr = e / WGMAP_GCOLS, gc = e % WGMAP_GCOLS;
            const int rc = gr < rows ? gr : rows - 1, cc = gc < gcols ? gc : gcols - 1;
            gpre[it] = p.gout[(int64_t)(k0 + rc) * p.gout_ld + m_lo + cc];
        }
    };
    auto store_slice = [&](const int k0) {
        const int rows = K - k0 < RS_KS ? K - k0 : RS_KS;
        if constexpr (VEC) {
#pragma unroll
            for (int it = 0; it < RS_KS / 8; ++it) {
                const int r = it * 8 + wave * 2 + half;
                if (r < rows && c4 < W)
                    reinterpret_cast<float4*>(sx)[r * W + c4] = float4{pre[4 * it], pre[4 * it + 1], pre[4 * it + 2], pre[4 * it + 3]};
            }
        } else {
#pragma unroll
            for (int it = 0; it < RS_KS / 4; ++it) {
                const int r = it * 4 + wave;
                if (r < rows && lane < N) sx[r * N + lane] = pre[2 * it];
                if constexpr (WIDE) {
                    if (r < rows && lane + 64 < N) sx[r * N + lane + 64] = pre[2 * it + 1];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < RS_GIT; ++it) {
            const int e = it * 256 + tid;
            if (e / WGMAP_GCOLS < rows && e % WGMAP_GCOLS < gcols) sg[e] = gpre[it];
        }
    };
    float acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.0f;
    const float* px = sx + n;
    const float* pg = sg + (m - m_lo);
    auto products = [&](const int t) {   // terms t .. t + 31 of the staged slice (t = 0 mod 32: accumulator j for term t + j)
#pragma unroll
        for (int j = 0; j < 32; ++j) acc[j] = fmaf(pg[(t + j) * WGMAP_GCOLS], px[(t + j) * N], acc[j]);
    };
    load_slice(0);
    int k0 = 0;
    for (; k0 + RS_KS < K; k0 += RS_KS) {   // the whole slices in front of the last one
        store_slice(k0);
        __syncthreads();
        load_slice(k0 + RS_KS);                // in flight during the products below
#pragma unroll
        for (int t = 0; t < RS_KS; t += 32) products(t);
        __syncthreads();                       // every wave is done reading this slice
    }
    store_slice(k0);                           // the last slice: 1 .. RS_KS terms
    __syncthreads();
    const int rows = K - k0;
    int t = 0;
    for (; t + 32 <= rows; t += 32) products(t);
    const int rem = rows - t;
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (j < rem) acc[j] = fmaf(pg[(t + j) * WGMAP_GCOLS], px[(t + j) * N], acc[j]);
    float pw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
        pw[w] = ((acc[8 * w] + acc[8 * w + 1]) + (acc[8 * w + 2] + acc[8 * w + 3])) + ((acc[8 * w + 4] + acc[8 * w + 5]) + (acc[8 * w + 6] + acc[8 * w + 7]));
    const float v = (pw[0] + pw[1]) + (pw[2] + pw[3]);
    p.dW[(int64_t)m * p.dw_ld + n] = v;
    const float sq = wgrad_wave_sum(fmaf(v, v, 0.0f));
    if (lane == 0) {
        ln.partials[group0 + wave] = sq;
        if (group0 == 0 && wave == 0) ln.step[0] += 1.0f;
    }
}

// `groups` = ceil(items / 64) <= WGMAP_MAX_GROUPS: a plain block runs the plain kernel's body for its one group (block g of
// `groups` blocks: one trip of its loop); the problem of a fast block is picked with compile-time indices only
__global__ void __launch_bounds__(256) wgrad_reduce_rows_staged_kernel(const WgradBatch b, const WgradNorm ln, const unsigned rows_mask,
                                                                       const unsigned vec_mask, const WgradRowsMap map, const unsigned groups) {
    // (dynamic: RS_LDS_BYTES; one set for the three instantiations of the fast body, 16-byte aligned behind the plain body's 1 KB.
    // A plain block is given the 17 KB too and never touches them: at 115 VGPRs four blocks per CU still fit, 72 KB of 160.)
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int bid = (int)blockIdx.x;
    int first = 0, g0 = map.group0[0], prob = map.prob[0];
#pragma unroll
    for (int s = 1; s < WGMAP_MAX_SEG; ++s) {
        if (s < map.n_seg && bid >= map.block_start[s]) { first = map.block_start[s]; g0 = map.group0[s]; prob = map.prob[s]; }
    }
    if (prob < 0) {
        wgrad_reduce_norm_body<true, true>(b, ln, rows_mask, (unsigned)(g0 + (bid - first)), groups);
        return;
    }
    RowsFastProb p;
#define MACJD_PICK_ROWS(q)                                                                                         \
    p.gout = b.io[q].gout; p.inp = b.io[q].inp; p.dW = b.io[q].dW; p.gout_ld = b.io[q].gout_ld;                   \
    p.inp_ld = b.io[q].inp_ld; p.dw_ld = b.io[q].dw_ld; p.start = b.out_start[q]; p.K = (int)b.io[q].K; p.N = b.io[q].N;
    MACJD_PICK_ROWS(0)
#pragma unroll
    for (int q = 1; q < MACJD_WGRAD_MAX_BATCH; ++q) {
        if (q == prob) { MACJD_PICK_ROWS(q) }
    }
#undef MACJD_PICK_ROWS
    float* sx = rs_lds;
    float* sg = rs_lds + RS_KS * WGMAP_N_CAP;
    const int group0 = g0 + WGMAP_FAST_GROUPS * (bid - first);
    if ((vec_mask >> prob) & 1u) wgrad_rows_staged_body<true, false>(p, group0, ln, sx, sg);
    else if (p.N > 64) wgrad_rows_staged_body<false, true>(p, group0, ln, sx, sg);
    else wgrad_rows_staged_body<false, false>(p, group0, ln, sx, sg);
}

static_assert(WGMAP_MAX_PROBLEMS == MACJD_WGRAD_MAX_BATCH && WGMAP_GROUP == WG_RED, "macjd_wgrad_map.h mirrors these");

}  // namespace macjd

extern "C" int64_t macjd_linear_wgrad_workspace_floats(int64_t K, int32_t M, int32_t N) {
    using namespace macjd;
    if (K < 1 || M < 1 || N < 1) return -1;
    const int64_t chunks = (K + WG_ROWS - 1) / WG_ROWS, Mp = wg_pad(M, WG_BM), Np = wg_pad(N, WG_BN);
    return chunks * Mp * Np + chunks * Mp;
}

extern "C" int macjd_linear_wgrad(const macjd_wgrad_io* io, void* hip_stream) {
    using namespace macjd;
    if (io && io->kind != MACJD_WGRAD_ORDINARY)
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_linear_wgrad: problem kinds are macjd_linear_wgrad_many_norm's");
    if (!io || io->K < 1 || io->M < 1 || io->N < 1 || !io->gout || !io->inp || !io->dW || !io->workspace)
        return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad: bad argument");
    if (io->gout_ld < io->M || io->inp_ld < io->N || io->dw_ld < io->N)
        return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad: bad leading dimension");
    if ((io->outer_vec == nullptr) != (io->outer_w == nullptr))
        return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad: outer_vec and outer_w go together");
    const int Mp = (int)wg_pad(io->M, WG_BM), Np = (int)wg_pad(io->N, WG_BN);
    const int64_t chunks = (io->K + WG_ROWS - 1) / WG_ROWS;
    if (chunks > 65535) return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_linear_wgrad: K too large");
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(wgrad_partial_kernel, dim3(Np / WG_BN, Mp / WG_BM, (unsigned)chunks), dim3(256), 0, s, wg_dev(*io), Mp, Np);
    const int64_t total = (int64_t)io->M * io->N + io->M;   // WG_RED output elements per workgroup
    const unsigned rblocks = (unsigned)((total + WG_RED - 1) / WG_RED < 8192 ? (total + WG_RED - 1) / WG_RED : 8192);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rblocks), dim3(256), 0, s, wg_dev(*io), Mp, Np, (int)chunks);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_linear_wgrad: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_linear_wgrad_many(const macjd_wgrad_io* ios, int32_t n, void* hip_stream) {
    using namespace macjd;
    if (!ios || n < 1 || n > MACJD_WGRAD_MAX_BATCH)
        return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad_many: 1..MACJD_WGRAD_MAX_BATCH problems");
    WgradBatch b{};
    b.n = n;
    for (int p = 0; p < n; ++p) {
        const macjd_wgrad_io* io = &ios[p];
        if (io->kind != MACJD_WGRAD_ORDINARY)
            return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_linear_wgrad_many: problem kinds are macjd_linear_wgrad_many_norm's");
        if (io->K < 1 || io->M < 1 || io->N < 1 || !io->gout || !io->inp || !io->dW || !io->workspace)
            return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad_many: bad argument");
        if (io->gout_ld < io->M || io->inp_ld < io->N || io->dw_ld < io->N)
            return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad_many: bad leading dimension");
        if ((io->outer_vec == nullptr) != (io->outer_w == nullptr))
            return set_err(MACJD_EINVAL, "%s", "macjd_linear_wgrad_many: outer_vec and outer_w go together");
        b.io[p] = wg_dev(*io);
        b.Mp[p] = (int)wg_pad(io->M, WG_BM);
        b.Np[p] = (int)wg_pad(io->N, WG_BN);
        b.chunks[p] = (int)((io->K + WG_ROWS - 1) / WG_ROWS);
        b.tiles_n[p] = b.Np[p] / WG_BN;
        b.tiles_m[p] = b.Mp[p] / WG_BM;
        b.wg_start[p + 1] = b.wg_start[p] + (int64_t)b.tiles_n[p] * b.tiles_m[p] * b.chunks[p];
        b.out_start[p + 1] = b.out_start[p] + (int64_t)io->M * io->N + io->M;
    }
    for (int p = n; p < MACJD_WGRAD_MAX_BATCH; ++p) {
        b.wg_start[p + 1] = b.wg_start[n];
        b.out_start[p + 1] = b.out_start[n];
        b.tiles_n[p] = b.tiles_m[p] = 1;
    }
    if (b.wg_start[n] > 0x7fffffff) return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_linear_wgrad_many: too many work items");
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(wgrad_partial_many_kernel, dim3((unsigned)b.wg_start[n]), dim3(256), 0, s, b);
    const int64_t total = b.out_start[n];
    const unsigned rblocks = (unsigned)((total + WG_RED - 1) / WG_RED < 8192 ? (total + WG_RED - 1) / WG_RED : 8192);
    hipLaunchKernelGGL(wgrad_reduce_many_kernel, dim3(rblocks), dim3(256), 0, s, b);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_linear_wgrad_many: %s", hipGetErrorString(err));
    return MACJD_OK;
}

// validation and tables of the grouped launches that know a contracted problem; returns MACJD_OK or the error set
static int wgrad_norm_batch(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem, macjd::WgradBatch* out, const char* who,
                            unsigned* rows_mask = nullptr) {
    using namespace macjd;
    if (!ios || n < 1 || n > MACJD_WGRAD_MAX_BATCH || ln_problem < -1 || ln_problem >= n)
        return set_err(MACJD_EINVAL, "%s: 1..MACJD_WGRAD_MAX_BATCH problems, ln_problem -1 or one of them", who);
    WgradBatch& b = *out;
    b = WgradBatch{};
    b.n = n;
    unsigned rows = 0;
    for (int p = 0; p < n; ++p) {
        const macjd_wgrad_io* io = &ios[p];
        const bool is_ln = p == ln_problem;
        const bool ext = io->kind == MACJD_WGRAD_EXT_SLOTS, rowp = io->kind == MACJD_WGRAD_ROW_PRODUCTS;
        if (io->kind != MACJD_WGRAD_ORDINARY && !ext && !rowp) return set_err(MACJD_EINVAL, "%s: unknown problem kind", who);
        if (io->M < 1 || io->N < 1 || (!io->dW && !is_ln)) return set_err(MACJD_EINVAL, "%s: bad argument", who);
        if (!rowp && !io->workspace) return set_err(MACJD_EINVAL, "%s: bad argument", who);
        if (ext) {   // the slots are there: the operands are not read
            if (io->ext_chunks < 1) return set_err(MACJD_EINVAL, "%s: ext_chunks must be >= 1", who);
        } else {
            if (io->K < 1 || !io->gout || !io->inp) return set_err(MACJD_EINVAL, "%s: bad argument", who);
            if (io->gout_ld < io->M || io->inp_ld < io->N) return set_err(MACJD_EINVAL, "%s: bad leading dimension", who);
            if ((io->outer_vec == nullptr) != (io->outer_w == nullptr))
                return set_err(MACJD_EINVAL, "%s: outer_vec and outer_w go together", who);
        }
        if (!is_ln && io->dw_ld < io->N) return set_err(MACJD_EINVAL, "%s: bad leading dimension", who);
        if (rowp && (is_ln || io->outer_vec || io->K > 0x7fffffff))
            return set_err(MACJD_EUNSUPPORTED, "%s: a row-products problem is not contracted and has no outer_vec", who);
        if (is_ln && (io->N > WG_BN || io->db))
            return set_err(MACJD_EUNSUPPORTED, "%s: the contracted problem has N <= 64 and no bias output", who);
        b.io[p] = wg_dev(*io);
        b.Mp[p] = (int)wg_pad(io->M, WG_BM);
        b.Np[p] = (int)wg_pad(io->N, WG_BN);
        // terms of an output in the reduce launch: partial tiles, the slots that are there already, or the rows themselves
        b.chunks[p] = ext ? io->ext_chunks : rowp ? (int)io->K : (int)((io->K + WG_ROWS - 1) / WG_ROWS);
        b.tiles_n[p] = b.Np[p] / WG_BN;
        b.tiles_m[p] = b.Mp[p] / WG_BM;
        // (a problem of kind != 0 has no work item in the partial-products launch)
        b.wg_start[p + 1] = b.wg_start[p] + ((ext || rowp) ? 0 : (int64_t)b.tiles_n[p] * b.tiles_m[p] * b.chunks[p]);
        b.out_start[p + 1] = b.out_start[p] + (is_ln ? (int64_t)2 * io->N : (int64_t)io->M * io->N + io->M);
        if (rowp) rows |= 1u << p;
    }
    for (int p = n; p < MACJD_WGRAD_MAX_BATCH; ++p) {
        b.wg_start[p + 1] = b.wg_start[n];
        b.out_start[p + 1] = b.out_start[n];
        b.tiles_n[p] = b.tiles_m[p] = 1;
    }
    if (b.wg_start[n] > 0x7fffffff) return set_err(MACJD_EUNSUPPORTED, "%s: too many work items", who);
    if (rows_mask) *rows_mask = rows;
    return MACJD_OK;
}

static unsigned wgrad_reduce_blocks(int64_t total) {
    using namespace macjd;
    return (unsigned)((total + WG_RED - 1) / WG_RED < 8192 ? (total + WG_RED - 1) / WG_RED : 8192);
}

extern "C" int32_t macjd_linear_wgrad_many_norm_partials(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem) {
    macjd::WgradBatch b;
    if (wgrad_norm_batch(ios, n, ln_problem, &b, "macjd_linear_wgrad_many_norm_partials") != MACJD_OK) return -1;
    return (int32_t)wgrad_reduce_blocks(b.out_start[n]);
}

extern "C" int64_t macjd_linear_wgrad_many_norm_work_items(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem) {
    macjd::WgradBatch b;
    if (wgrad_norm_batch(ios, n, ln_problem, &b, "macjd_linear_wgrad_many_norm_work_items") != MACJD_OK) return -1;
    return b.wg_start[n];
}

extern "C" int64_t macjd_wgrad_slot_floats(int32_t M, int32_t N, int64_t slots) {
    using namespace macjd;
    if (M < 1 || N < 1 || slots < 1) return -1;
    const int64_t Mp = wg_pad(M, WG_BM), Np = wg_pad(N, WG_BN);
    return slots * Mp * Np + slots * Mp;
}

// block map of the staged ROWS reduce for a validated batch; returns its blocks, or -1 where the plain rows kernel runs
// (the switch, no ROW PRODUCTS problem, the grid-stride case, or no fast block at all)
static int wgrad_rows_map(const macjd_wgrad_io* ios, const macjd::WgradBatch& b, unsigned rows_mask, uint32_t flags,
                          macjd::WgradRowsMap* map, unsigned* vec_mask) {
    using namespace macjd;
    if (!rows_mask || (flags & MACJD_WGRAD_PLAIN_ROWS)) return -1;
    int32_t M[MACJD_WGRAD_MAX_BATCH], N[MACJD_WGRAD_MAX_BATCH];
    bool fast_ok[MACJD_WGRAD_MAX_BATCH];
    unsigned vec = 0;
    for (int p = 0; p < b.n; ++p) {
        M[p] = b.io[p].M; N[p] = b.io[p].N;
        fast_ok[p] = ((rows_mask >> p) & 1u) && ios[p].K <= (1 << 30);
        if ((((uintptr_t)b.io[p].inp) & 15) == 0 && (b.io[p].inp_ld & 3) == 0 && (b.io[p].N & 3) == 0) vec |= 1u << p;
    }
    const int blocks = wgmap_build(b.n, b.out_start, M, N, fast_ok, map);
    bool any_fast = false;
    for (int s = 0; s < map->n_seg; ++s) any_fast = any_fast || map->prob[s] >= 0;
    *vec_mask = vec;
    return any_fast ? blocks : -1;
}

extern "C" int32_t macjd_linear_wgrad_many_norm_blocks(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem, uint32_t flags) {
    macjd::WgradBatch b;
    unsigned rows_mask = 0, vec_mask = 0;
    if (wgrad_norm_batch(ios, n, ln_problem, &b, "macjd_linear_wgrad_many_norm_blocks", &rows_mask) != MACJD_OK) return -1;
    macjd::WgradRowsMap map;
    const int blocks = wgrad_rows_map(ios, b, rows_mask, flags, &map, &vec_mask);
    return blocks >= 0 ? blocks : (int32_t)wgrad_reduce_blocks(b.out_start[n]);
}

static int wgrad_many_norm_launch(const macjd_wgrad_io* ios, int32_t n, const macjd_wgrad_norm_io* norm, uint32_t flags, void* hip_stream,
                                  const char* who);

extern "C" int macjd_linear_wgrad_many_norm(const macjd_wgrad_io* ios, int32_t n, const macjd_wgrad_norm_io* norm, void* hip_stream) {
    return wgrad_many_norm_launch(ios, n, norm, 0u, hip_stream, "macjd_linear_wgrad_many_norm");
}

extern "C" int macjd_linear_wgrad_many_norm_ex(const macjd_wgrad_io* ios, int32_t n, const macjd_wgrad_norm_io* norm, uint32_t flags,
                                               void* hip_stream) {
    return wgrad_many_norm_launch(ios, n, norm, flags, hip_stream, "macjd_linear_wgrad_many_norm_ex");
}

static int wgrad_many_norm_launch(const macjd_wgrad_io* ios, int32_t n, const macjd_wgrad_norm_io* norm, uint32_t flags, void* hip_stream,
                                  const char* who) {
    using namespace macjd;
    if (!norm || !norm->partials || !norm->step) return set_err(MACJD_EINVAL, "%s: bad argument", who);
    WgradBatch b;
    unsigned rows_mask = 0;
    const int rc = wgrad_norm_batch(ios, n, norm->ln_problem, &b, who, &rows_mask);
    if (rc != MACJD_OK) return rc;
    WgradNorm ln{};
    ln.problem = norm->ln_problem;
    ln.partials = norm->partials; ln.step = norm->step;
    if (ln.problem >= 0) {
        const bool ext_ln = ios[ln.problem].kind == MACJD_WGRAD_EXT_SLOTS;   // (slots contracted already: W is not read)
        if (!norm->dgamma || !norm->dbeta || (!ext_ln && (!norm->W || norm->w_ld < ios[ln.problem].N)))
            return set_err(MACJD_EINVAL, "%s: bad LayerNorm argument", who);
        ln.W = norm->W; ln.w_ld = norm->w_ld; ln.dgamma = norm->dgamma; ln.dbeta = norm->dbeta;
        ln.slots = ios[ln.problem].kind == MACJD_WGRAD_EXT_SLOTS ? b.chunks[ln.problem] : b.tiles_m[ln.problem] * b.chunks[ln.problem];
    }
    const unsigned rblocks = wgrad_reduce_blocks(b.out_start[n]);
    if ((int64_t)rblocks > (int64_t)norm->partials_cap) return set_err(MACJD_EINVAL, "%s: partials_cap too small", who);
    hipStream_t s = (hipStream_t)hip_stream;
    if (b.wg_start[n] > 0)   // (no problem of kind 0: nothing to multiply)
        hipLaunchKernelGGL(wgrad_partial_many_norm_kernel, dim3((unsigned)b.wg_start[n]), dim3(256), 0, s, b, ln);
    WgradRowsMap map;
    unsigned vec_mask = 0;
    const int sblocks = wgrad_rows_map(ios, b, rows_mask, flags, &map, &vec_mask);
    if (sblocks > 0)
        hipLaunchKernelGGL(wgrad_reduce_rows_staged_kernel, dim3((unsigned)sblocks), dim3(256), RS_LDS_BYTES, s, b, ln, rows_mask, vec_mask, map, rblocks);
    else if (rows_mask) hipLaunchKernelGGL(wgrad_reduce_many_rows_kernel, dim3(rblocks), dim3(256), 0, s, b, ln, rows_mask);
    else hipLaunchKernelGGL(wgrad_reduce_many_norm_kernel, dim3(rblocks), dim3(256), 0, s, b, ln);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        char msg[192];
        snprintf(msg, sizeof msg, "%s: %s", who, hipGetErrorString(err));
        return set_err(MACJD_EDEVICE, "%s", msg);
    }
    return MACJD_OK;
}
