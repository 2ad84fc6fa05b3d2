// macjd_mixer.hip — the QMix mixer (reference core/networks.py:250-315) as one MFMA chain per direction.
// C-ABI and the algebra: include/macjd_nets.h (macjd_mixerf_io).
//
// Geometry.  M = batch x steps is a few thousand rows (3232 for the reference batch), the widest layer has 384 output
// columns: tiling the rows 64 at a time (as the agent's dense-chain kernel does for its 10^4..10^5 rows) would leave
// 4/5 of the chip idle.  Here a workgroup owns 16 rows — ONE MFMA row tile — and its four waves split the output
// COLUMNS of each layer, so 3232 rows are 202 workgroups of 256 threads and a row's whole chain (LayerNorm, merged
// first layer, ReLU, both second layers, clamps, the two contractions with q and w_final, ELU) never leaves the
// workgroup:
//   phase 0  LayerNorm of the 16 rows (wave w: rows 4w..4w+3, 16 lanes per row)              -> LDS As [16][16 SQ]
//   phase 1  [16, 384] = As W1^T + b1, ReLU on the first 320 columns; wave w: column tiles 6w..6w+5  -> LDS Hs
//   phase 2  wave w = embed block e in [16w, 16w+16): the J tiles w1_raw[:, j, e-block] and the tile wf_raw[:, e-block]
//            stay in accumulators; hid = q . clamp(w1) + clamp(b1), ELU, . clamp(wf): registers; the sum over a row's
//            16 columns is a 4-step xor shuffle, the sum over the 4 embed blocks goes through 256 B of LDS.
// Operands.  A (activations) comes from LDS by ds_read_b128 with the permuted-k assignment of macjd_mlp.hip (lane group
// g supplies k = 16 Q + 4 g + jj in MFMA jj of quad Q: one float4 feeds four MFMAs; pitches = 8 mod 16 floats are
// conflict-free).  B (weights) is NOT staged: with 16 rows per workgroup a staged image would be read once, so every
// lane loads its own fragments W[16 t + (lane & 15)][16 Q + 4 g ..+3] straight from L2 (the weights are ~230 KB,
// shared by all workgroups), and ALL of them are requested at the top of the kernel — they depend on nothing — so the
// whole chain waits for memory once.  ~200 VGPRs of fragments at 3j/4r; one wave per SIMD has 512.
// Numerics: v_mfma_f32_16x16x4_f32 is an exact-f32 fmaf chain; the tail uses the same expressions (fmaf chain over the
// agents starting from clamp(b1), expm1f) as mixer_tail_kernel.
// Training.  The learner update's two forwards, the TD gradient and the backward are ONE launch (mixer_fused_train_kernel).
// It writes what the five weight-gradient products of macjd_wgrad.hip read: per row (1 117 floats a row at J = 3: 14.4 MB
// at M = 3232, K = 3232 in the split-K pass), or — STATIC, episodes whose state does not change in time — per 16-row tile
// of ONE episode: the tile's row 0 of sn / xhat / act and the tile's SUMS of gout1 / g_w1raw / g_wfraw / g_v, formed on
// chip in a fixed order (7 tiles x 32 episodes = 224 rows instead of 3232: under 1 MB, K = 224).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/macjd.h"
#include "../../include/macjd_nets.h"
#include "macjd_err.h"
#include "macjd_tdloss.h"

namespace macjd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));   // weight rows are only 4-byte aligned (S = 46)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#ifndef MACJD_MX_ABLATE
#define MACJD_MX_ABLATE 0   // timing experiments only (results wrong when non-zero): 1 no fragment loads, 2 no phase-1
#endif                      // MFMAs, 4 no phase-2 MFMAs, 8 no state loads, 16 no tail math
constexpr int MX_ABL = MACJD_MX_ABLATE;
constexpr int MX_HH = 128, MX_EM = 64;
constexpr int MX_N1 = 2 * MX_HH + 2 * MX_EM;   // 384 columns of the merged first layer
constexpr int MX_RELU = 2 * MX_HH + MX_EM;     // the first 320 of them pass a ReLU
constexpr int MX_LDH = MX_N1 + 8;              // LDS pitch of the first-layer output (= 8 mod 16)
constexpr int MX_KQ2 = MX_HH / 16;             // quads (16 k each) of the second layers

__device__ __forceinline__ float mx_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float mx_sum16(float x) {   // sum over the 16 lanes that share lane >> 4
    x += __shfl_xor(x, 1, 64);
    x += __shfl_xor(x, 2, 64);
    x += __shfl_xor(x, 4, 64);
    x += __shfl_xor(x, 8, 64);
    return x;
}

// Operand type (template parameter BF of every body / kernel below; macjd_mixerf_io.operand_dtype).  BF = false: exact
// f32, v_mfma_f32_16x16x4_f32.  BF = true: the same fragments, held as f32 (weights are the f32 parameters, activations
// the f32 LDS images) and rounded to bf16 (v_cvt_pk_bf16_f32, round to nearest even) right before each
// v_mfma_f32_16x16x32_bf16, which sums 32 k per instruction in f32.  Only the k each lane holds in a quad changes:
// k of element jj of quad Q (16 k) for lane group g.  f32: k = 16 Q + 4 g + jj feeds MFMA jj of the quad (the permuted
// assignment above).  bf16 (mx_kq + jj): quads pair up into 32-k steps, whose lane group g holds k = 32 P + 8 g + (0..7)
// (A[row lane & 15][k], B[k][col lane & 15]): quad 2P + h holds k = 32 P + 8 g + 4 h + jj.  An odd last quad (S <= 48
// at J = 3) is a half step: k = 16 Q + 4 g + jj in elements 0..3, zeros in 4..7 — no padding of the LDS rows or loads.
// (The f32 index expressions below are spelled out as before, behind `BF ? ... :`, so that the f32 instantiations
// compile to the same code as before the operand type existed.)
template <int NQ>
__device__ __forceinline__ constexpr int mx_kq(int Q, int g) {
    return ((NQ & 1) && Q == NQ - 1) ? 16 * Q + 4 * g : 32 * (Q >> 1) + 8 * g + 4 * (Q & 1);
}
__device__ __forceinline__ bf16x8 mx_pack_bf16(const f32x4& lo, const f32x4& hi) {
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3],
                  (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}
// A operand of 32-k step P from an f32 LDS row (row = base + (lane & 15) * pitch; pitches and bases are multiples of 8
// floats, so both halves are ds_read_b128)
template <int NQ>
__device__ __forceinline__ bf16x8 mx_a_bf16(const float* row, int P, int g) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(row + mx_kq<NQ>(2 * P, g));
    const f32x4 hi = (2 * P + 1 < NQ) ? *reinterpret_cast<const f32x4*>(row + mx_kq<NQ>(2 * P + 1, g))
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
    return mx_pack_bf16(lo, hi);
}
// B operand of 32-k step P from a lane's f32 fragments
template <int NQ>
__device__ __forceinline__ bf16x8 mx_b_bf16(const f32x4 (&B)[NQ], int P) {
    return mx_pack_bf16(B[2 * P], (2 * P + 1 < NQ) ? B[2 * P + 1] : f32x4{0.f, 0.f, 0.f, 0.f});
}
__device__ __forceinline__ f32x4 mx_mfma_bf16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// B fragments (all quads) of one 16-column tile whose weight row is `row` of a row-major [*, K] matrix.  No branch
// around any load: a divergent `if` with a load inside makes hipcc drain the memory counter (s_waitcnt vmcnt(0)) at
// every join, which serialised the ~50 fragment loads of a wave one L2 latency after the other (16 us per launch
// instead of ~5).  RAGGED (K not a multiple of 16, e.g. S = 46): the last quad is four dword loads from clamped
// addresses, zeroed past the row by selects (bf16 with NQ even: the last two quads, which share the last 32-k step).
// RAGGED = 2 (narrow rows, K <= 16 (NQ - 1), no shipped size): the quads in front of the last reach past the row as well —
// in the last rows past the matrix, where what they read meets zero activations but need not be finite — so EVERY quad
// takes the clamped form.  A variant of its own (see mixerf_narrow), so that the kernels of the shipped sizes stay as
// they are.
template <int NQ, int RAGGED, bool BF = false>
__device__ __forceinline__ void mx_load_frags(f32x4 (&dst)[NQ], const float* __restrict__ W, int K, int row, int g) {
    constexpr int NRAG = (BF && NQ % 2 == 0) ? 2 : 1;
    const float* p = W + (int64_t)row * K;
#pragma unroll
    for (int Q = 0; Q < NQ; ++Q) {
        const int k0 = BF ? mx_kq<NQ>(Q, g) : 16 * Q + 4 * g;
        if (MX_ABL & 1) {
            dst[Q] = f32x4{(float)row, (float)g, 1.0f, 0.5f};
        } else if (RAGGED == 0 || (RAGGED == 1 && Q < NQ - NRAG)) {   // compile-time
            dst[Q] = *reinterpret_cast<const f32x4_u*>(p + k0);
        } else {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int k = k0 + jj;
                const float v = p[k < K ? k : K - 1];
                dst[Q][jj] = (k < K) ? v : 0.0f;
            }
        }
    }
}

// Second layers + tail for this wave's embed block, shared by the forward kernel and the backward's recomputation:
// acc2[j] = tile (j, eb) of w1_raw WITHOUT its bias, accf = tile eb of wf_raw without its bias.
template <int J, bool BF>
__device__ __forceinline__ void mx_second_layers(const float* __restrict__ Hs, const f32x4 (&B2)[J][MX_KQ2],
                                                 const f32x4 (&Bf)[MX_KQ2], f32x4 (&acc2)[J], f32x4& accf, int li, int g) {
#pragma unroll
    for (int j = 0; j < J; ++j) acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    accf = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {
        const float* a1p = Hs + li * MX_LDH;
        const float* afp = a1p + MX_HH;
#pragma unroll
        for (int P = 0; P < ((MX_ABL & 4) ? 0 : MX_KQ2 / 2); ++P) {
            const bf16x8 a1 = mx_a_bf16<MX_KQ2>(a1p, P, g);
            const bf16x8 af = mx_a_bf16<MX_KQ2>(afp, P, g);
#pragma unroll
            for (int j = 0; j < J; ++j) acc2[j] = mx_mfma_bf16(a1, mx_b_bf16<MX_KQ2>(B2[j], P), acc2[j]);
            accf = mx_mfma_bf16(af, mx_b_bf16<MX_KQ2>(Bf, P), accf);
        }
        return;
    }
    const float* a1p = Hs + li * MX_LDH + 4 * g;            // h_w1: columns [0, Hh)
    const float* afp = a1p + MX_HH;                         // h_wf: columns [Hh, 2 Hh)
#pragma unroll
    for (int Q = 0; Q < ((MX_ABL & 4) ? 0 : MX_KQ2); ++Q) {
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(a1p + 16 * Q);
        const f32x4 af = *reinterpret_cast<const f32x4*>(afp + 16 * Q);
        // k-step outer, tiles inner: consecutive MFMAs go to different accumulators (a dependent one waits 40 cycles,
        // the issue interval is 32)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
            for (int j = 0; j < J; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[jj], B2[j][Q][jj], acc2[j], 0, 0, 0);
            accf = __builtin_amdgcn_mfma_f32_16x16x4f32(af[jj], Bf[Q][jj], accf, 0, 0, 0);
        }
    }
}

// v_raw of row (lane & 15): h_V . wV2 + bV2, valid in the lanes with g == 0 afterwards (every wave may call it)
__device__ __forceinline__ float mx_v_raw(const float* __restrict__ Hs, const float (&wv)[16], float bV2, int li, int g) {
    float s = 0.0f;   // wv[k] = wV2[16 g + k], preloaded
    const float* hv = Hs + li * MX_LDH + 2 * MX_HH + 16 * g;
#pragma unroll
    for (int k = 0; k < 16; ++k) s = fmaf(hv[k], wv[k], s);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    return s + bV2;
}

// LDS of one forward workgroup (the body below is a device function of (arguments, workgroup index, LDS): the eval and
// the target mixer of one learner update run as ONE grid, macjd_mixer_fused_forward_pair)
template <int SQ>
struct MixerFwdLds {
    alignas(16) float As[16 * (16 * SQ + 8)];
    alignas(16) float Hs[16 * MX_LDH];
    float part[4][16];
};

// LATE2: the second layers' fragments (B2 / Bf, 32 (J + 1) registers) are requested behind the first layer's MFMAs
// instead of at the top: ~130 fewer live registers at J = 3 — two workgroups per CU, which the paired launch (twice the
// workgroups) needs to stay one round — for one exposed L2 latency, which the CU's other workgroup covers.
// What the training kernel's backward takes over from its eval half's forward instead of recomputing or reloading it:
// the accumulator tiles of w1_raw / wf_raw (without bias), their biases, the rows of q and (wave 0) v_raw, and the
// forward's Q_tot of row (lane & 15) (wave 0, g == 0).
template <int J>
struct MixerKeep {
    f32x4 acc2[J], accf;
    float qv[4][J], b2e[J], bfe, v_raw, y;
};

// m0 = first row of the tile, wave = this wave's index among the body's four (the training kernel runs two bodies side
// by side in one eight-wave workgroup).  KEEP: hand the tiles / vectors above to the caller.  TILE (with SAVE): sn / xhat /
// act are [n_tiles, ...] and get ONE row, this tile's row 0, at row `tile` (the static-state training launch).
template <int J, int SQ, bool SAVE, bool LATE2 = false, bool KEEP = false, bool BF = false, bool NARROW = false, bool TILE = false>
__device__ __forceinline__ void mixer_fused_forward_body(const macjd_mixerf_io& io, const int64_t m0, const int wave,
                                                         MixerFwdLds<SQ>& L, MixerKeep<J>* keep = nullptr, const int64_t tile = 0) {
    constexpr int LDA = 16 * SQ + 8;
    constexpr int T1W = MX_N1 / 16 / 4;   // 6 first-layer column tiles per wave
    auto& As = L.As;
    auto& Hs = L.Hs;
    auto& part = L.part;
    const int lane = threadIdx.x & 63;
    const int li = lane & 15, g = lane >> 4;
    const int S = io.S;

    // ---- loads, oldest first = needed first (s_waitcnt counts in issue order): the state rows of the LayerNorm, then
    // every weight fragment of the launch; nothing below depends on anything but kernel arguments ----
    // (the bias / LayerNorm / V-head vectors too: a load next to its use sits behind the s_waitcnt vmcnt(0) that hipcc
    // puts at every divergent join, i.e. each one would cost a full memory latency AND drain the fragment loads)
    float x[SQ], lnw[SQ], lnb[SQ];
    {
        const int64_t m = m0 + 4 * wave + g;
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            const int col = li + 16 * c, cc = col < S ? col : S - 1;
            x[c] = (MX_ABL & 8) ? (float)col : io.s[(m < io.M ? m : io.M - 1) * io.s_ld + cc];
            lnw[c] = io.ln_w[cc];
            lnb[c] = io.ln_b[cc];
        }
    }
    float b1v[T1W], b2e[J], wv[16];
#pragma unroll
    for (int i = 0; i < T1W; ++i) b1v[i] = io.b1[16 * (T1W * wave + i) + li];
#pragma unroll
    for (int j = 0; j < J; ++j) b2e[j] = io.b2[j * MX_EM + 16 * wave + li];
    const float bfe = io.bf2[16 * wave + li];
#pragma unroll
    for (int k = 0; k < 16; ++k) wv[k] = io.wV2[16 * g + k];
    const float bV2 = io.bV2[0];
    f32x4 B1[T1W][SQ], B2[J][MX_KQ2], Bf[MX_KQ2];
#pragma unroll
    for (int i = 0; i < T1W; ++i) mx_load_frags<SQ, NARROW ? 2 : 1, BF>(B1[i], io.W1, S, 16 * (T1W * wave + i) + li, g);
    auto load_second = [&]() {
#pragma unroll
        for (int j = 0; j < J; ++j) mx_load_frags<MX_KQ2, false, BF>(B2[j], io.W2, MX_HH, j * MX_EM + 16 * wave + li, g);
        mx_load_frags<MX_KQ2, false, BF>(Bf, io.Wf2, MX_HH, 16 * wave + li, g);
    };
    if (!LATE2) load_second();
    // this lane's rows of q (rows 4g..4g+3 of the tile), for the tail
    float qv[4][J];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + 4 * g + r;
        const int64_t mc = m < io.M ? m : io.M - 1;   // clamped: rows past M are computed on the last row, never stored
#pragma unroll
        for (int j = 0; j < J; ++j) qv[r][j] = io.q[mc * J + j];
    }

    // ---- phase 0: LayerNorm (networks.py:283), wave w: rows 4w..4w+3, lane (g = row within the wave, li = column mod 16)
    {
        const int row = 4 * wave + g;
        const int64_t m = m0 + row;
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            x[c] = (li + 16 * c < S) ? x[c] : 0.0f;
            sum += x[c];
        }
        const float mean = mx_sum16(sum) / (float)S;
        float sq = 0.0f;
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            const float d = (li + 16 * c < S) ? x[c] - mean : 0.0f;
            sq = fmaf(d, d, sq);
        }
        const float rstd = rsqrtf(mx_sum16(sq) / (float)S + io.ln_eps);
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            const int col = li + 16 * c;
            const bool live = col < S;
            const float xh = live ? (x[c] - mean) * rstd : 0.0f;
            const float v = live ? xh * lnw[c] + lnb[c] : 0.0f;               // pad columns: 0 (they meet zero fragments)
            As[row * LDA + col] = v;
            if constexpr (TILE) {
                if (SAVE && live && row == 0) {
                    io.sn[tile * S + col] = v;
                    io.xhat[tile * S + col] = xh;
                }
            } else if (SAVE && live && m < io.M) {
                io.sn[m * S + col] = v;
                io.xhat[m * S + col] = xh;
            }
        }
    }
    __syncthreads();

    // ---- phase 1: merged first layer (networks.py:285-299), this wave's 6 column tiles ----
    {
        f32x4 acc[T1W];
#pragma unroll
        for (int i = 0; i < T1W; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BF) {
#pragma unroll
            for (int P = 0; P < ((MX_ABL & 2) ? 0 : (SQ + 1) / 2); ++P) {
                const bf16x8 a = mx_a_bf16<SQ>(As + li * LDA, P, g);
#pragma unroll
                for (int i = 0; i < T1W; ++i) acc[i] = mx_mfma_bf16(a, mx_b_bf16<SQ>(B1[i], P), acc[i]);
            }
        } else {
            const float* ap = As + li * LDA + 4 * g;
#pragma unroll
            for (int Q = 0; Q < ((MX_ABL & 2) ? 0 : SQ); ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int i = 0; i < T1W; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], B1[i][Q][jj], acc[i], 0, 0, 0);
            }
        }
        if (LATE2) load_second();
#pragma unroll
        for (int i = 0; i < T1W; ++i) {
            const int col = 16 * (T1W * wave + i) + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                float v = acc[i][r] + b1v[i];
                v = (col < MX_RELU) ? fmaxf(v, 0.0f) : v;
                Hs[row * MX_LDH + col] = v;
                if constexpr (TILE) {
                    if (SAVE && row == 0) io.act[tile * MX_N1 + col] = v;
                } else if (SAVE && m0 + row < io.M) io.act[(m0 + row) * MX_N1 + col] = v;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: second layers for embed block `wave`, tail (networks.py:301-310) ----
    f32x4 acc2[J], accf;
    mx_second_layers<J, BF>(Hs, B2, Bf, acc2, accf, li, g);
    const int e = 16 * wave + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        float hid = mx_clamp(Hs[row * MX_LDH + MX_RELU + e], -5.0f, 5.0f);
#pragma unroll
        for (int j = 0; j < J; ++j) hid = fmaf(qv[r][j], mx_clamp(acc2[j][r] + b2e[j], 0.0f, 5.0f), hid);   // bmm(q, w1) + b1
        const float h = hid > 0.0f ? hid : expm1f(hid);                                                       // F.elu
        const float t = mx_sum16(h * mx_clamp(accf[r] + bfe, 0.0f, 5.0f));                                    // bmm(hidden, w_final)
        if (li == 0) part[wave][row] = t;
    }
    const float v_raw = (wave == 0) ? mx_v_raw(Hs, wv, bV2, li, g) : 0.0f;
    __syncthreads();
    if (wave == 0 && g == 0) {
        const int64_t m = m0 + li;
        const float y = ((part[0][li] + part[1][li]) + (part[2][li] + part[3][li])) + mx_clamp(v_raw, -5.0f, 5.0f);
        if (m < io.M) io.y[m] = y;
        if (KEEP) keep->y = y;
    }
    if (KEEP) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            keep->acc2[j] = acc2[j];
            keep->b2e[j] = b2e[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) keep->qv[r][j] = qv[r][j];
        }
        keep->accf = accf;
        keep->bfe = bfe;
        keep->v_raw = v_raw;
    }
}

// (bf16 at J = 6: the bf16 copies of the operands push the fragments-up-front plan past the 512 registers — 20 B / lane
// of scratch — so the second layers' fragments are requested behind the first layer, LATE2)
template <int J, int SQ, bool SAVE, bool BF, bool NARROW>
__global__ void __launch_bounds__(256) mixer_fused_forward_kernel(const macjd_mixerf_io io) {
    __shared__ MixerFwdLds<SQ> L;
    mixer_fused_forward_body<J, SQ, SAVE, BF && J == 6, false, BF, NARROW>(io, (int64_t)blockIdx.x * 16, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), L);
}

// blockIdx.y = 0: the mixer whose activations are saved for a backward (io_a), 1: the plain one (io_b)
template <int J, int SQ, bool BF, bool NARROW>
__global__ void __launch_bounds__(256, (J <= 3) ? 2 : 1) mixer_fused_forward_pair_kernel(const macjd_mixerf_io io_a, const macjd_mixerf_io io_b) {
    __shared__ MixerFwdLds<SQ> L;
    const int64_t m0 = (int64_t)blockIdx.x * 16;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr bool LATE2 = (J <= 3) || (BF && J == 6);   // (bf16 at J = 6: see mixer_fused_forward_kernel)
    if (blockIdx.y == 0) mixer_fused_forward_body<J, SQ, true, LATE2, false, BF, NARROW>(io_a, m0, wave, L);
    else mixer_fused_forward_body<J, SQ, false, LATE2, false, BF, NARROW>(io_b, m0, wave, L);
}

// Backward (see the header): recompute the second layers from `act`, tail gradients, transposed second layers.
// TD = the gradient of the learner's TD loss w.r.t. this mixer's output is formed HERE instead of being read from io.gy
// (macjd_mixer_fused_backward_td): row m = (b, t) gets scale * mask * (y - (r + gamma (1 - term) tq)) for t < Tm1 and 0
// otherwise — td_loss_kernel's own expression, with scale = 2 / *tot_m from a launch that summed the batch's mask earlier
// (macjd_td_mask_sum: it needs the gathered batch only, so it runs long before).  Five loads per row, no reduction: the
// loss launch leaves the update's serial chain (its logged sums are computed off the chain by macjd_td_loss).
template <int J, bool TD, bool BF>
__global__ void __launch_bounds__(256) mixer_fused_backward_kernel(const macjd_mixerf_io io, const macjd_tdloss_io td,
                                                                    const float* __restrict__ tot_m) {
    constexpr int LDG = J * MX_EM + 8;      // pitch of g_w1raw in LDS (= 8 mod 16)
    constexpr int LDF = MX_EM + 8;
    constexpr int KQ1 = J * MX_EM / 16;     // quads of the transposed hyper_w_1.2 product
    constexpr int KQF = MX_EM / 16;
    __shared__ __attribute__((aligned(16))) float Hs[16 * MX_LDH];
    __shared__ __attribute__((aligned(16))) float G1[16 * LDG];
    __shared__ __attribute__((aligned(16))) float Gf[16 * LDF];
    __shared__ float gq_part[4][16][J];
    __shared__ float gv_s[16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    if (TD && td.stats && blockIdx.x == gridDim.x - 1) {   // the extra workgroup: the loss's logged sums (macjd_tdloss.h)
        td_loss_sums(td, false);
        return;
    }
    const int64_t m0 = (int64_t)blockIdx.x * 16;

    // ---- weight fragments, requested up front: forward orientation for the recomputation ...
    f32x4 B2[J][MX_KQ2], Bf[MX_KQ2];
#pragma unroll
    for (int j = 0; j < J; ++j) mx_load_frags<MX_KQ2, false, BF>(B2[j], io.W2, MX_HH, j * MX_EM + 16 * wave + li, g);
    mx_load_frags<MX_KQ2, false, BF>(Bf, io.Wf2, MX_HH, 16 * wave + li, g);
    // ... and transposed for the input gradients of the second layers: this wave's output columns are the hidden units
    // n = 16 (2 wave + tt) + li; B[k][n] = W2[k][n] with k = 16 Q + 4 g + jj the row (a w1_raw column): four strided
    // dwords per quad, each a coalesced 64-byte row piece over li
    // (J = 6: both fragment sets together would need more than the 512 registers; the transposed set is then
    // requested after the recomputation, when the forward set is dead)
    constexpr bool EARLY_D = (J <= 3);
    f32x4 D1[2][KQ1], Df[2][KQF];
    auto load_transposed = [&]() {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int n = 16 * (2 * wave + tt) + li;
#pragma unroll
            for (int Q = 0; Q < KQ1; ++Q)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) D1[tt][Q][jj] = io.W2[(int64_t)(BF ? mx_kq<KQ1>(Q, g) + jj : 16 * Q + 4 * g + jj) * MX_HH + n];
#pragma unroll
            for (int Q = 0; Q < KQF; ++Q)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) Df[tt][Q][jj] = io.Wf2[(int64_t)(BF ? mx_kq<KQF>(Q, g) + jj : 16 * Q + 4 * g + jj) * MX_HH + n];
        }
    };
    if (EARLY_D) load_transposed();
    float b2e[J], wv[16], wvo[4];
#pragma unroll
    for (int j = 0; j < J; ++j) b2e[j] = io.b2[j * MX_EM + 16 * wave + li];
    const float bfe = io.bf2[16 * wave + li];
#pragma unroll
    for (int k = 0; k < 16; ++k) wv[k] = io.wV2[16 * g + k];
#pragma unroll
    for (int i = 0; i < 4; ++i) wvo[i] = io.wV2[(threadIdx.x + 256 * i) & (MX_EM - 1)];   // for the V head's outer product
    const float bV2 = io.bV2[0];
    auto load_gy = [&](const int64_t mc) -> float {
        if constexpr (TD) {
            const int cols = (int)td.gy_cols;
            const int b = (int)(mc / cols), t = (int)(mc - (int64_t)b * cols);
            const int tc = t < td.Tm1 ? t : td.Tm1 - 1;     // clamped: no branch around the loads
            const float term = td.terminated[b * td.t_sb + tc * td.t_st] ? 1.0f : 0.0f;
            const float mk = td.filled[b * td.f_sb + tc * td.f_st] ? 1.0f : 0.0f;
            const float target = td.reward[b * td.r_sb + tc * td.r_st] + td.gamma * (1.0f - term) * td.tq[b * td.tq_sb + tc];
            const float scale = 2.0f / tot_m[0];
            const float gv = scale * mk * (td.y[b * td.y_sb + tc] - target);
            return t < td.Tm1 ? gv : 0.0f;
        } else {
            return io.gy[mc];
        }
    };
    const float gy_li = load_gy((m0 + li < io.M) ? m0 + li : io.M - 1);
    float qv[4][J], gyv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + 4 * g + r;
        const int64_t mc = m < io.M ? m : io.M - 1;   // clamped (no branch around a load); rows past M are never stored
        gyv[r] = load_gy(mc);
#pragma unroll
        for (int j = 0; j < J; ++j) qv[r][j] = io.q[mc * J + j];
    }
    // ---- the saved first-layer output of the 16 rows -> LDS (float4 pieces; rows past M: zeros) ----
    for (int idx = threadIdx.x; idx < 16 * (MX_N1 / 4); idx += 256) {
        const int row = idx / (MX_N1 / 4), c4 = idx - row * (MX_N1 / 4);
        const int64_t mc = (m0 + row < io.M) ? m0 + row : io.M - 1;
        *reinterpret_cast<f32x4*>(Hs + row * MX_LDH + 4 * c4) = *reinterpret_cast<const f32x4*>(io.act + mc * MX_N1 + 4 * c4);
    }
    __syncthreads();

    // ---- recompute w1_raw / wf_raw tiles of embed block `wave` and the tail, then its gradients ----
    f32x4 acc2[J], accf;
    mx_second_layers<J, BF>(Hs, B2, Bf, acc2, accf, li, g);
    const int e = 16 * wave + li;
    const float v_raw = (wave == 0) ? mx_v_raw(Hs, wv, bV2, li, g) : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const int64_t m = m0 + row;
        const float b1r = Hs[row * MX_LDH + MX_RELU + e];
        float hid = mx_clamp(b1r, -5.0f, 5.0f);
        float w1r[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            w1r[j] = acc2[j][r] + b2e[j];
            hid = fmaf(qv[r][j], mx_clamp(w1r[j], 0.0f, 5.0f), hid);
        }
        const float h = hid > 0.0f ? hid : expm1f(hid);
        const float wfr = accf[r] + bfe;
        const float ghid = gyv[r] * mx_clamp(wfr, 0.0f, 5.0f) * (hid > 0.0f ? 1.0f : h + 1.0f);   // ELU'(x) = elu(x) + 1, x <= 0
        const float gwf = (wfr >= 0.0f && wfr <= 5.0f) ? gyv[r] * h : 0.0f;                        // clamp passes inside [lo, hi]
        const float gb1 = (b1r >= -5.0f && b1r <= 5.0f) ? ghid : 0.0f;
        Gf[row * LDF + e] = gwf;
        if (m < io.M) {
            io.g_wfraw[m * MX_EM + e] = gwf;
            io.gout1[m * MX_N1 + MX_RELU + e] = gb1;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float gw = (w1r[j] >= 0.0f && w1r[j] <= 5.0f) ? ghid * qv[r][j] : 0.0f;
            G1[row * LDG + j * MX_EM + e] = gw;
            if (m < io.M) io.g_w1raw[m * (J * MX_EM) + j * MX_EM + e] = gw;
            const float t = mx_sum16(ghid * mx_clamp(w1r[j], 0.0f, 5.0f));
            if (li == 0) gq_part[wave][row][j] = t;
        }
    }
    if (!EARLY_D) load_transposed();
    if (wave == 0 && g == 0) {   // v = clamp(v_raw, -5, 5): row li
        const int64_t m = m0 + li;
        const float gv = (v_raw >= -5.0f && v_raw <= 5.0f) ? gy_li : 0.0f;
        gv_s[li] = gv;
        if (m < io.M) io.g_v[m] = gv;
    }
    __syncthreads();
    // dL/dq: the four embed blocks' partial sums in fixed order
    for (int idx = threadIdx.x; idx < 16 * J; idx += 256) {
        const int row = idx / J, j = idx - row * J;
        if (m0 + row < io.M)
            io.gq[(m0 + row) * J + j] = (gq_part[0][row][j] + gq_part[1][row][j]) + (gq_part[2][row][j] + gq_part[3][row][j]);
    }

    // ---- input gradients of the second layers, masked by the first layer's ReLU: columns [0, 2 Hh) of gout1 ----
    {
        f32x4 a1[2], af[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) { a1[tt] = f32x4{0.f, 0.f, 0.f, 0.f}; af[tt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        if constexpr (BF) {
#pragma unroll
            for (int P = 0; P < KQ1 / 2; ++P) {
                const bf16x8 a = mx_a_bf16<KQ1>(G1 + li * LDG, P, g);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) a1[tt] = mx_mfma_bf16(a, mx_b_bf16<KQ1>(D1[tt], P), a1[tt]);
            }
#pragma unroll
            for (int P = 0; P < KQF / 2; ++P) {
                const bf16x8 a = mx_a_bf16<KQF>(Gf + li * LDF, P, g);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) af[tt] = mx_mfma_bf16(a, mx_b_bf16<KQF>(Df[tt], P), af[tt]);
            }
        } else {
            const float* gp = G1 + li * LDG + 4 * g;
            const float* fp = Gf + li * LDF + 4 * g;
#pragma unroll
            for (int Q = 0; Q < KQ1; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(gp + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) a1[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], D1[tt][Q][jj], a1[tt], 0, 0, 0);
            }
#pragma unroll
            for (int Q = 0; Q < KQF; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(fp + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) af[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], Df[tt][Q][jj], af[tt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int n = 16 * (2 * wave + tt) + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const int64_t m = m0 + row;
                if (m < io.M) {
                    io.gout1[m * MX_N1 + n] = (Hs[row * MX_LDH + n] > 0.0f) ? a1[tt][r] : 0.0f;
                    io.gout1[m * MX_N1 + MX_HH + n] = (Hs[row * MX_LDH + MX_HH + n] > 0.0f) ? af[tt][r] : 0.0f;
                }
            }
        }
    }
    // the V head's one-output second layer: outer product g_v wV2, masked: columns [2 Hh, 2 Hh + Em)
#pragma unroll
    for (int i = 0; i < 16 * MX_EM / 256; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int row = idx / MX_EM, k = idx - row * MX_EM;
        if (m0 + row < io.M)
            io.gout1[(m0 + row) * MX_N1 + 2 * MX_HH + k] = (Hs[row * MX_LDH + 2 * MX_HH + k] > 0.0f) ? gv_s[row] * wvo[i] : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The learner update's mixers as ONE launch (macjd_mixer_fused_train): eval forward, target forward, the TD loss's
// gradient and the eval mixer's backward.  One workgroup of eight waves owns the 16-row tile [m0, m0 + 16):
//   waves 0-3  the eval mixer's forward body on rows [m0, m0 + 16) (activations saved, as the pair's saving half); its
//              first-layer output stays in LDS (= `act`) and its w1_raw / wf_raw tiles stay in registers (MixerKeep)
//   waves 4-7  the target mixer's forward body on rows [m0 + 1, m0 + 17) (loads clamped at M, as everywhere): eval row m's
//              TD target reads the target mixer's row m + 1, so every target value the tile's loss needs is made here
//   one barrier, then dL/dy of each row from LDS (td_loss_kernel's expression, see mixer_fused_backward_kernel<J, true>)
//   waves 0-3  tail gradients of embed block `wave` (the backward's expressions on the kept tiles)
//   waves 0-7  one column tile each of the transposed second-layer products (gout1's first 2 Hh columns; the backward
//              kernel's four waves do two each), dL/dq, the V head's outer product.
// Every output is the same expression in the same order as the pair + backward launches: bit-identical.
//
// STATIC (macjd_mixer_fused_train_static): the state, hence sn / xhat / act, is the same in every row of an episode, so a
// weight gradient sum_m g[m]^T x[m] is sum_tiles (sum of the tile's g rows)^T x[tile] as long as no tile straddles two
// episodes.  Workgroup b * TPE + k (TPE = ceil(T1 / 16), T1 = td.gy_cols) owns rows t = 16 k .. 16 k + 15 of episode b; rows
// with t >= T1 are dead: loads clamped into the episode (the target half's to the row behind it, which is where row
// T1 - 1's target row lies), nothing stored, not `live` for the loss, so their gradient operands are exact zeros.  y, the
// target's y and gq are per row, the same instruction sequence as above: bit-identical.  sn / xhat / act are [n_tiles, ...],
// one row per tile taken from its row 0; gout1 / g_w1raw / g_wfraw / g_v are [n_tiles, ...] per-tile SUMS of the per-row
// values above, each row under its own ReLU / clamp mask, in one fixed order and without atomics:
//   g_w1raw, g_wfraw, g_v, gout1's V block   column sums over LDS rows 0, 1, .. 15
//   gout1's h_w1 / h_wf / b1 blocks          accumulator-held: rows 4 g + (0, 1, 2, 3) in the lane, then + lane group g ^ 1,
//                                            then + lane groups g ^ 2 (two xor shuffles)
template <int J>
struct MixerTrainLds {
    MixerFwdLds<J> ev, tg;
    alignas(16) float G1[16 * (J * MX_EM + 8)];
    alignas(16) float Gf[16 * (MX_EM + 8)];
    float gq_part[4][16][J];
    float gv_s[16];
    float ys[16], tqs[16];   // eval Q_tot of row m0 + i, target Q_tot of row m0 + 1 + i
};

// mixer_fused_train_wgrad_kernel (STATIC, f32; macjd_mixer_fused_train_static_wgrad): behind all of the above the workgroup writes its slots of the
// Q-head's two weight-gradient problems and of the LayerNorm contraction (`wb`, include/macjd_nets.h).  LDS that is dead by
// then is reused — floats from the start of L.tg (dead since the first barrier): gs[384] a copy of the tile's gout1 sums,
// up[8][64] the partial u, sX[16 J][80] the Q-head input rows, sQ[64] gq per agent row; from the start of L.ev (dead after
// the column sums): sG[16 J][80] the masked outer product, sAq[16 J][64] the Q-head's ReLU output.
constexpr int WGB_PITCH = 80;              // = 16 mod 32, as the weight-gradient kernel's chunks
constexpr int WGB_GS = 0, WGB_UP = MX_N1, WGB_SX = MX_N1 + 8 * 64;

// what a thread holds of the tile's R = 16 J agent rows between request and use: its float4 pieces of the Q-head's ReLU
// output and of h (piece id = 512 it + thread: row id >> 4, columns 4 (id & 15) ..), and — thread r < R — row r's P and index
template <int J>
struct WgbLoads {
    static constexpr int R = 16 * J;
    static constexpr int NIT = (R * 16 + 511) / 512;
    float4 a[NIT], h[NIT];
    float p;
    int idx;      // the taken action, -1 when outside [0, A)
    int n_live;   // rows of the tile inside the episode (the others: clamped loads, exact zeros)
    int A;
};

// every load from a clamped (valid) address, no branch around a load
template <int J>
__device__ __forceinline__ void wgb_load(const macjd_mixer_wgrad_block& wb, const int64_t n0, const int64_t n_end, WgbLoads<J>& out) {
    constexpr int R = WgbLoads<J>::R, NIT = WgbLoads<J>::NIT;
    const int tid = threadIdx.x;
    out.n_live = (int)(n_end - n0 < R ? n_end - n0 : R);
    out.A = wb.A;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int id = it * 512 + tid;
        const int r = (id >> 4) < R ? (id >> 4) : R - 1, c4 = (id & 15) * 4;
        const int64_t n = n0 + r < n_end ? n0 + r : n_end - 1;
        out.a[it] = *reinterpret_cast<const float4*>(wb.act_q + n * wb.act_ld + c4);
        out.h[it] = *reinterpret_cast<const float4*>(wb.h + n * wb.h_ld + c4);
    }
}

// ... and thread r's (r < R; the others repeat row R - 1) index and P
template <int J>
__device__ __forceinline__ void wgb_load_row(const macjd_mixer_wgrad_block& wb, const int64_t n0, const int64_t n_end, WgbLoads<J>& out) {
    constexpr int R = WgbLoads<J>::R;
    const int tid = threadIdx.x;
    const int r = tid < R ? tid : R - 1;
    const int64_t n = n0 + r < n_end ? n0 + r : n_end - 1;
    out.p = wb.P[n];
    int64_t v;
    if (wb.idx_elem_size == 8) v = reinterpret_cast<const int64_t*>(wb.idx)[n];   // (uniform)
    else v = reinterpret_cast<const int32_t*>(wb.idx)[n];
    out.idx = (v >= 0 && v < wb.A) ? (int)v : -1;
}

// sX[r][0 .. 80) = [h[r], onehot(idx[r]), P[r], zeros]; dead rows all zero
template <int J>
__device__ __forceinline__ void wgb_stage_x(const WgbLoads<J>& l, float* __restrict__ sX) {
    constexpr int R = WgbLoads<J>::R, NIT = WgbLoads<J>::NIT;
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int id = it * 512 + tid;
        const int r = id >> 4, c4 = (id & 15) * 4;
        if (id < R * 16) {
            const bool live = r < l.n_live;
            float4 v = l.h[it];
            v.x = live ? v.x : 0.0f; v.y = live ? v.y : 0.0f; v.z = live ? v.z : 0.0f; v.w = live ? v.w : 0.0f;
            *reinterpret_cast<float4*>(sX + r * WGB_PITCH + c4) = v;
        }
    }
    if (tid < R) {
        const bool live = tid < l.n_live;
#pragma unroll
        for (int a = 0; a < 16; ++a)
            sX[tid * WGB_PITCH + 64 + a] = !live ? 0.0f : a == l.idx ? 1.0f : a == l.A ? l.p : 0.0f;
    }
}

// the tile's slots (macjd_mixer_wgrad_block).  Called by all 512 threads behind the column sums; two barriers inside.
template <int J>
__device__ __forceinline__ void wgb_finish(const macjd_mixer_wgrad_block& wb, const WgbLoads<J>& l, const float* xhat, const int S,
                                           const int64_t tile, const int64_t n_tiles, const float (*gq_part)[16][J],
                                           float* __restrict__ tg, float* __restrict__ ev) {
    constexpr int R = WgbLoads<J>::R, NIT = WgbLoads<J>::NIT;
    const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6, li = lane & 15, g = lane >> 4;
    const float* gs = tg + WGB_GS;
    float* up = tg + WGB_UP;
    const float* sX = tg + WGB_SX;
    float* sQ = tg + WGB_SX + R * WGB_PITCH;
    float* sG = ev;
    float* sAq = ev + R * WGB_PITCH;
    // u's weights (wave w: rows 48 w .. 48 w + 47 of W_first, lane = column, clamped) and this thread's four of w2
    constexpr int RUN = MX_N1 / 8;
    const int kc = lane < S ? lane : S - 1;
    float wv[RUN], w2v[4];
#pragma unroll
    for (int i = 0; i < RUN; ++i) wv[i] = wb.W_first[(int64_t)(RUN * wave8 + i) * wb.w_ld + kc];
#pragma unroll
    for (int e = 0; e < 4; ++e) w2v[e] = wb.w2[(tid & 15) * 4 + e];
    wgb_stage_x<J>(l, tg + WGB_SX);   // (L.tg: free already)
    __syncthreads();   // the column sums are done: L.ev is dead, gs and sX are complete
    {
        float u = 0.0f;
#pragma unroll
        for (int i = 0; i < RUN; ++i) u = fmaf(wv[i], gs[RUN * wave8 + i], u);
        up[wave8 * 64 + lane] = u;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int id = it * 512 + tid;
        const int r = id >> 4, c4 = (id & 15) * 4;
        if (id < R * 16) {
            const int row = r / J, j = r - row * J;
            const bool live = r < l.n_live;
            const float gq = (gq_part[0][row][j] + gq_part[1][row][j]) + (gq_part[2][row][j] + gq_part[3][row][j]);
            const float4 a = l.a[it];
            float4 gh, aq;
            gh.x = (live && a.x > 0.0f) ? gq * w2v[0] : 0.0f; aq.x = live ? a.x : 0.0f;
            gh.y = (live && a.y > 0.0f) ? gq * w2v[1] : 0.0f; aq.y = live ? a.y : 0.0f;
            gh.z = (live && a.z > 0.0f) ? gq * w2v[2] : 0.0f; aq.z = live ? a.z : 0.0f;
            gh.w = (live && a.w > 0.0f) ? gq * w2v[3] : 0.0f; aq.w = live ? a.w : 0.0f;
            *reinterpret_cast<float4*>(sG + r * WGB_PITCH + c4) = gh;
            *reinterpret_cast<float4*>(sAq + r * 64 + c4) = aq;
            if ((id & 15) == 0) sQ[r] = live ? gq : 0.0f;
        }
    }
    __syncthreads();
    const int N1 = 64 + l.A + 1, Np1 = (N1 + 63) / 64 * 64;
    // Q-head first layer: 4 x 5 tiles of 16 x 16 over the eight waves, rows ascending
    for (int t = wave8; t < 20; t += 8) {
        const int mt = t & 3, nt = t >> 2;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* pa = sG + g * WGB_PITCH + 16 * mt + li;
        const float* pb = sX + g * WGB_PITCH + 16 * nt + li;
#pragma unroll
        for (int kk = 0; kk < R / 4; ++kk)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk * 4 * WGB_PITCH], pb[kk * 4 * WGB_PITCH], acc, 0, 0, 0);
        const int n = 16 * nt + li;
        if (n < N1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wb.ws1[(tile * 64 + 16 * mt + 4 * g + r) * Np1 + n] = acc[r];
        }
    }
    if (wave8 == 0) {          // the LayerNorm slot: the eight runs of u as a fixed tree
        if (lane < S) {
            const float u = ((up[lane] + up[64 + lane]) + (up[128 + lane] + up[192 + lane])) +
                            ((up[256 + lane] + up[320 + lane]) + (up[384 + lane] + up[448 + lane]));
            wb.ln_slots[(tile * 2) * S + lane] = xhat[tile * S + lane] * u;
            wb.ln_slots[(tile * 2 + 1) * S + lane] = u;
        }
    } else if (wave8 == 1) {   // db1: column sums of g_hid, rows ascending
        float s = sG[lane];
#pragma unroll 8
        for (int r = 1; r < R; ++r) s += sG[r * WGB_PITCH + lane];
        wb.ws1[n_tiles * 64 * Np1 + tile * 64 + lane] = s;
    } else if (wave8 == 2) {   // dw2[m] = sum_r gq[r] act_q[r][m]
        float s = 0.0f;
#pragma unroll 8
        for (int r = 0; r < R; ++r) s = fmaf(sQ[r], sAq[r * 64 + lane], s);
        wb.ws2[tile * 64 * 64 + lane] = s;
    } else if (wave8 == 3 && lane == 0) {   // db2 = sum_r gq[r]
        float s = sQ[0];
        for (int r = 1; r < R; ++r) s += sQ[r];
        wb.ws2[n_tiles * 64 * 64 + tile * 64] = s;
    }
}

template <int J, bool BF, bool NARROW, bool STATIC = false>
__global__ void __launch_bounds__(512) mixer_fused_train_kernel(const macjd_mixerf_io io, const macjd_mixerf_io tio,
                                                                 const macjd_tdloss_io td, const float* __restrict__ tot_m) {
#define MX_TRAIN_WG 0
#include "macjd_mixer_train_body.h"
#undef MX_TRAIN_WG
}

template <int J, bool NARROW>
__global__ void __launch_bounds__(512) mixer_fused_train_wgrad_kernel(const macjd_mixerf_io io, const macjd_mixerf_io tio,
                                                                       const macjd_tdloss_io td, const float* __restrict__ tot_m,
                                                                       const macjd_mixer_wgrad_block wb) {
    constexpr bool BF = false, STATIC = true;
#define MX_TRAIN_WG 1
#include "macjd_mixer_train_body.h"
#undef MX_TRAIN_WG
}

// ---------------------------------------------------------------------------------------------------------------
// Wide scenarios (J = 12: BASELINE.json's 12 jammers / 16 radars, S = 184).  Same geometry and the same expressions as
// the kernels above, but the weight fragments of a whole layer no longer fit a lane's registers (first layer: 6 tiles x
// 12 quads = 288 VGPRs; hyper_w_1's second layer: 12 tiles x 8 quads = 384), so both layers run in PASSES whose
// fragments are loaded one pass ahead: the first layer two column tiles at a time, the J tiles of w1_raw PJ agents at
// a time.  The tail's fmaf chain over the agents runs in agent order across the passes, i.e. it is the chain of
// mixer_tail_kernel / the narrow kernels.
template <int PJ, bool BF>
__device__ __forceinline__ void mx_load_pass(f32x4 (&dst)[PJ][MX_KQ2], const float* __restrict__ W2, int j0, int wave, int li, int g) {
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj) mx_load_frags<MX_KQ2, false, BF>(dst[jj], W2, MX_HH, (j0 + jj) * MX_EM + 16 * wave + li, g);
}

template <int PJ, bool BF>
__device__ __forceinline__ void mx_pass_tiles(const float* __restrict__ Hs, const f32x4 (&B2)[PJ][MX_KQ2], f32x4 (&acc2)[PJ],
                                              int li, int g) {
#pragma unroll
    for (int j = 0; j < PJ; ++j) acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {
#pragma unroll
        for (int P = 0; P < MX_KQ2 / 2; ++P) {
            const bf16x8 a1 = mx_a_bf16<MX_KQ2>(Hs + li * MX_LDH, P, g);
#pragma unroll
            for (int j = 0; j < PJ; ++j) acc2[j] = mx_mfma_bf16(a1, mx_b_bf16<MX_KQ2>(B2[j], P), acc2[j]);
        }
        return;
    }
    const float* a1p = Hs + li * MX_LDH + 4 * g;            // h_w1: columns [0, Hh)
#pragma unroll
    for (int Q = 0; Q < MX_KQ2; ++Q) {
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(a1p + 16 * Q);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int j = 0; j < PJ; ++j) acc2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[jj], B2[j][Q][jj], acc2[j], 0, 0, 0);
    }
}

template <bool BF>
__device__ __forceinline__ void mx_wf_tile(const float* __restrict__ Hs, const f32x4 (&Bf)[MX_KQ2], f32x4& accf, int li, int g) {
    accf = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {
#pragma unroll
        for (int P = 0; P < MX_KQ2 / 2; ++P) accf = mx_mfma_bf16(mx_a_bf16<MX_KQ2>(Hs + li * MX_LDH + MX_HH, P, g), mx_b_bf16<MX_KQ2>(Bf, P), accf);
        return;
    }
    const float* afp = Hs + li * MX_LDH + 4 * g + MX_HH;    // h_wf: columns [Hh, 2 Hh)
#pragma unroll
    for (int Q = 0; Q < MX_KQ2; ++Q) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(afp + 16 * Q);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) accf = __builtin_amdgcn_mfma_f32_16x16x4f32(af[jj], Bf[Q][jj], accf, 0, 0, 0);
    }
}

template <int J, int SQ, bool SAVE, int PJ, bool BF, bool NARROW>
__device__ __forceinline__ void mixer_fused_forward_wide_body(const macjd_mixerf_io& io, const int blk, MixerFwdLds<SQ>& L) {
    static_assert(J % PJ == 0, "whole passes");
    constexpr int LDA = 16 * SQ + 8;
    constexpr int T1W = MX_N1 / 16 / 4;   // 6 first-layer column tiles per wave
    constexpr int P1W = 2;                // ... two per pass
    constexpr int NP = J / PJ;
    auto& As = L.As;
    auto& Hs = L.Hs;
    auto& part = L.part;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int64_t m0 = (int64_t)blk * 16;
    const int S = io.S;

    float x[SQ], lnw[SQ], lnb[SQ];
    {
        const int64_t m = m0 + 4 * wave + g;
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            const int col = li + 16 * c, cc = col < S ? col : S - 1;
            x[c] = io.s[(m < io.M ? m : io.M - 1) * io.s_ld + cc];
            lnw[c] = io.ln_w[cc];
            lnb[c] = io.ln_b[cc];
        }
    }
    float b1v[T1W], b2e[J], wv[16];
#pragma unroll
    for (int i = 0; i < T1W; ++i) b1v[i] = io.b1[16 * (T1W * wave + i) + li];
#pragma unroll
    for (int j = 0; j < J; ++j) b2e[j] = io.b2[j * MX_EM + 16 * wave + li];
    const float bfe = io.bf2[16 * wave + li];
#pragma unroll
    for (int k = 0; k < 16; ++k) wv[k] = io.wV2[16 * g + k];
    const float bV2 = io.bV2[0];
    // first-layer fragments of passes 0 and 1 (the third pass re-uses the first buffer)
    f32x4 B1a[P1W][SQ], B1b[P1W][SQ];
#pragma unroll
    for (int i = 0; i < P1W; ++i) mx_load_frags<SQ, NARROW ? 2 : 1, BF>(B1a[i], io.W1, S, 16 * (T1W * wave + i) + li, g);
#pragma unroll
    for (int i = 0; i < P1W; ++i) mx_load_frags<SQ, NARROW ? 2 : 1, BF>(B1b[i], io.W1, S, 16 * (T1W * wave + P1W + i) + li, g);
    float qv[4][J];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + 4 * g + r;
        const int64_t mc = m < io.M ? m : io.M - 1;
#pragma unroll
        for (int j = 0; j < J; ++j) qv[r][j] = io.q[mc * J + j];
    }

    // ---- phase 0: LayerNorm ----
    {
        const int row = 4 * wave + g;
        const int64_t m = m0 + row;
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            x[c] = (li + 16 * c < S) ? x[c] : 0.0f;
            sum += x[c];
        }
        const float mean = mx_sum16(sum) / (float)S;
        float sq = 0.0f;
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            const float d = (li + 16 * c < S) ? x[c] - mean : 0.0f;
            sq = fmaf(d, d, sq);
        }
        const float rstd = rsqrtf(mx_sum16(sq) / (float)S + io.ln_eps);
#pragma unroll
        for (int c = 0; c < SQ; ++c) {
            const int col = li + 16 * c;
            const bool live = col < S;
            const float xh = live ? (x[c] - mean) * rstd : 0.0f;
            const float v = live ? xh * lnw[c] + lnb[c] : 0.0f;
            As[row * LDA + col] = v;
            if (SAVE && live && m < io.M) {
                io.sn[m * S + col] = v;
                io.xhat[m * S + col] = xh;
            }
        }
    }
    __syncthreads();

    // ---- phase 1: merged first layer, this wave's 6 column tiles in three passes of two ----
    auto first_layer_pass = [&](const f32x4 (&B1)[P1W][SQ], int pass) {
        f32x4 acc[P1W];
#pragma unroll
        for (int i = 0; i < P1W; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BF) {
#pragma unroll
            for (int P = 0; P < (SQ + 1) / 2; ++P) {
                const bf16x8 a = mx_a_bf16<SQ>(As + li * LDA, P, g);
#pragma unroll
                for (int i = 0; i < P1W; ++i) acc[i] = mx_mfma_bf16(a, mx_b_bf16<SQ>(B1[i], P), acc[i]);
            }
        } else {
            const float* ap = As + li * LDA + 4 * g;
#pragma unroll
            for (int Q = 0; Q < SQ; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int i = 0; i < P1W; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], B1[i][Q][jj], acc[i], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < P1W; ++i) {
            const int t = P1W * pass + i;
            const int col = 16 * (T1W * wave + t) + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                float v = acc[i][r] + b1v[t];
                v = (col < MX_RELU) ? fmaxf(v, 0.0f) : v;
                Hs[row * MX_LDH + col] = v;
                if (SAVE && m0 + row < io.M) io.act[(m0 + row) * MX_N1 + col] = v;
            }
        }
    };
    first_layer_pass(B1a, 0);
#pragma unroll
    for (int i = 0; i < P1W; ++i) mx_load_frags<SQ, NARROW ? 2 : 1, BF>(B1a[i], io.W1, S, 16 * (T1W * wave + 2 * P1W + i) + li, g);
    // second-layer fragments of the first agent pass and of w_final: in flight under the rest of phase 1
    f32x4 B2a[PJ][MX_KQ2], B2b[PJ][MX_KQ2], Bf[MX_KQ2];
    mx_load_pass<PJ, BF>(B2a, io.W2, 0, wave, li, g);
    mx_load_frags<MX_KQ2, false, BF>(Bf, io.Wf2, MX_HH, 16 * wave + li, g);
    first_layer_pass(B1b, 1);
    first_layer_pass(B1a, 2);
    __syncthreads();

    // ---- phase 2: second layers for embed block `wave` in NP agent passes, tail ----
    const int e = 16 * wave + li;
    float hid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) hid[r] = mx_clamp(Hs[(4 * g + r) * MX_LDH + MX_RELU + e], -5.0f, 5.0f);
    f32x4 accf;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        f32x4 acc2[PJ];
        if (p + 1 < NP) {
            if (p & 1) mx_load_pass<PJ, BF>(B2a, io.W2, (p + 1) * PJ, wave, li, g);
            else mx_load_pass<PJ, BF>(B2b, io.W2, (p + 1) * PJ, wave, li, g);
        }
        if (p & 1) mx_pass_tiles<PJ, BF>(Hs, B2b, acc2, li, g);
        else mx_pass_tiles<PJ, BF>(Hs, B2a, acc2, li, g);
        if (p == 0) mx_wf_tile<BF>(Hs, Bf, accf, li, g);
#pragma unroll
        for (int jj = 0; jj < PJ; ++jj) {
            const int j = p * PJ + jj;
#pragma unroll
            for (int r = 0; r < 4; ++r) hid[r] = fmaf(qv[r][j], mx_clamp(acc2[jj][r] + b2e[j], 0.0f, 5.0f), hid[r]);   // bmm(q, w1) + b1
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const float h = hid[r] > 0.0f ? hid[r] : expm1f(hid[r]);                                   // F.elu
        const float t = mx_sum16(h * mx_clamp(accf[r] + bfe, 0.0f, 5.0f));                         // bmm(hidden, w_final)
        if (li == 0) part[wave][row] = t;
    }
    const float v_raw = (wave == 0) ? mx_v_raw(Hs, wv, bV2, li, g) : 0.0f;
    __syncthreads();
    if (wave == 0 && g == 0) {
        const int64_t m = m0 + li;
        if (m < io.M) io.y[m] = ((part[0][li] + part[1][li]) + (part[2][li] + part[3][li])) + mx_clamp(v_raw, -5.0f, 5.0f);
    }
}

template <int J, int SQ, bool SAVE, int PJ, bool BF, bool NARROW>
__global__ void __launch_bounds__(256) mixer_fused_forward_wide_kernel(const macjd_mixerf_io io) {
    __shared__ MixerFwdLds<SQ> L;
    mixer_fused_forward_wide_body<J, SQ, SAVE, PJ, BF, NARROW>(io, blockIdx.x, L);
}

template <int J, int SQ, int PJ, bool BF, bool NARROW>
__global__ void __launch_bounds__(256) mixer_fused_forward_wide_pair_kernel(const macjd_mixerf_io io_a, const macjd_mixerf_io io_b) {
    __shared__ MixerFwdLds<SQ> L;
    if (blockIdx.y == 0) mixer_fused_forward_wide_body<J, SQ, true, PJ, BF, NARROW>(io_a, blockIdx.x, L);
    else mixer_fused_forward_wide_body<J, SQ, false, PJ, BF, NARROW>(io_b, blockIdx.x, L);
}

template <int J, int PJ, bool TD, bool BF>
__global__ void __launch_bounds__(256) mixer_fused_backward_wide_kernel(const macjd_mixerf_io io, const macjd_tdloss_io td,
                                                                         const float* __restrict__ tot_m) {
    static_assert(J % PJ == 0, "whole passes");
    constexpr int NP = J / PJ;
    constexpr int LDG = PJ * MX_EM + 8;     // pitch of ONE pass of g_w1raw in LDS (= 8 mod 16)
    constexpr int LDF = MX_EM + 8;
    constexpr int KQP = PJ * MX_EM / 16;    // quads of one pass of the transposed hyper_w_1.2 product
    constexpr int KQF = MX_EM / 16;
    __shared__ __attribute__((aligned(16))) float Hs[16 * MX_LDH];
    __shared__ __attribute__((aligned(16))) float G1[16 * LDG];
    __shared__ __attribute__((aligned(16))) float Gf[16 * LDF];
    __shared__ float gq_part[4][16][J];
    __shared__ float gv_s[16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    if (TD && td.stats && blockIdx.x == gridDim.x - 1) {   // the extra workgroup: the loss's logged sums (macjd_tdloss.h)
        td_loss_sums(td, false);
        return;
    }
    const int64_t m0 = (int64_t)blockIdx.x * 16;

    f32x4 B2a[PJ][MX_KQ2], B2b[PJ][MX_KQ2], Bf[MX_KQ2];
    mx_load_pass<PJ, BF>(B2a, io.W2, 0, wave, li, g);
    mx_load_frags<MX_KQ2, false, BF>(Bf, io.Wf2, MX_HH, 16 * wave + li, g);
    float b2e[J], wv[16], wvo[4];
#pragma unroll
    for (int j = 0; j < J; ++j) b2e[j] = io.b2[j * MX_EM + 16 * wave + li];
    const float bfe = io.bf2[16 * wave + li];
#pragma unroll
    for (int k = 0; k < 16; ++k) wv[k] = io.wV2[16 * g + k];
#pragma unroll
    for (int i = 0; i < 4; ++i) wvo[i] = io.wV2[(threadIdx.x + 256 * i) & (MX_EM - 1)];
    const float bV2 = io.bV2[0];
    auto load_gy = [&](const int64_t mc) -> float {
        if constexpr (TD) {
            const int cols = (int)td.gy_cols;
            const int b = (int)(mc / cols), t = (int)(mc - (int64_t)b * cols);
            const int tc = t < td.Tm1 ? t : td.Tm1 - 1;
            const float term = td.terminated[b * td.t_sb + tc * td.t_st] ? 1.0f : 0.0f;
            const float mk = td.filled[b * td.f_sb + tc * td.f_st] ? 1.0f : 0.0f;
            const float target = td.reward[b * td.r_sb + tc * td.r_st] + td.gamma * (1.0f - term) * td.tq[b * td.tq_sb + tc];
            const float scale = 2.0f / tot_m[0];
            const float gv = scale * mk * (td.y[b * td.y_sb + tc] - target);
            return t < td.Tm1 ? gv : 0.0f;
        } else {
            return io.gy[mc];
        }
    };
    const float gy_li = load_gy((m0 + li < io.M) ? m0 + li : io.M - 1);
    float qv[4][J], gyv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + 4 * g + r;
        const int64_t mc = m < io.M ? m : io.M - 1;
        gyv[r] = load_gy(mc);
#pragma unroll
        for (int j = 0; j < J; ++j) qv[r][j] = io.q[mc * J + j];
    }
    for (int idx = threadIdx.x; idx < 16 * (MX_N1 / 4); idx += 256) {
        const int row = idx / (MX_N1 / 4), c4 = idx - row * (MX_N1 / 4);
        const int64_t mc = (m0 + row < io.M) ? m0 + row : io.M - 1;
        *reinterpret_cast<f32x4*>(Hs + row * MX_LDH + 4 * c4) = *reinterpret_cast<const f32x4*>(io.act + mc * MX_N1 + 4 * c4);
    }
    __syncthreads();

    // ---- sweep 1: recompute the w1_raw tiles of embed block `wave` pass by pass (kept: 4 J values per lane), hid ----
    const int e = 16 * wave + li;
    float w1r[J][4], hid[4], b1r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        b1r[r] = Hs[(4 * g + r) * MX_LDH + MX_RELU + e];
        hid[r] = mx_clamp(b1r[r], -5.0f, 5.0f);
    }
    f32x4 accf;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        f32x4 acc2[PJ];
        if (p + 1 < NP) {
            if (p & 1) mx_load_pass<PJ, BF>(B2a, io.W2, (p + 1) * PJ, wave, li, g);
            else mx_load_pass<PJ, BF>(B2b, io.W2, (p + 1) * PJ, wave, li, g);
        }
        if (p & 1) mx_pass_tiles<PJ, BF>(Hs, B2b, acc2, li, g);
        else mx_pass_tiles<PJ, BF>(Hs, B2a, acc2, li, g);
        if (p == 0) mx_wf_tile<BF>(Hs, Bf, accf, li, g);
#pragma unroll
        for (int jj = 0; jj < PJ; ++jj) {
            const int j = p * PJ + jj;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                w1r[j][r] = acc2[jj][r] + b2e[j];
                hid[r] = fmaf(qv[r][j], mx_clamp(w1r[j][r], 0.0f, 5.0f), hid[r]);
            }
        }
    }
    const float v_raw = (wave == 0) ? mx_v_raw(Hs, wv, bV2, li, g) : 0.0f;
    float ghid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const int64_t m = m0 + row;
        const float h = hid[r] > 0.0f ? hid[r] : expm1f(hid[r]);
        const float wfr = accf[r] + bfe;
        ghid[r] = gyv[r] * mx_clamp(wfr, 0.0f, 5.0f) * (hid[r] > 0.0f ? 1.0f : h + 1.0f);
        const float gwf = (wfr >= 0.0f && wfr <= 5.0f) ? gyv[r] * h : 0.0f;
        const float gb1 = (b1r[r] >= -5.0f && b1r[r] <= 5.0f) ? ghid[r] : 0.0f;
        Gf[row * LDF + e] = gwf;
        if (m < io.M) {
            io.g_wfraw[m * MX_EM + e] = gwf;
            io.gout1[m * MX_N1 + MX_RELU + e] = gb1;
        }
    }
    if (wave == 0 && g == 0) {
        const int64_t m = m0 + li;
        const float gv = (v_raw >= -5.0f && v_raw <= 5.0f) ? gy_li : 0.0f;
        gv_s[li] = gv;
        if (m < io.M) io.g_v[m] = gv;
    }

    // ---- sweep 2: per agent pass, the tile gradients -> LDS / HBM, then that pass's share of the transposed product ----
    f32x4 a1[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) a1[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {
        // this pass's transposed fragments: rows k = p PJ Em + 16 Q + 4 g + jj of W2, column n = 16 (2 wave + tt) + li
        f32x4 D1[2][KQP];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int n = 16 * (2 * wave + tt) + li;
#pragma unroll
            for (int Q = 0; Q < KQP; ++Q)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) D1[tt][Q][jj] = io.W2[(int64_t)(BF ? p * PJ * MX_EM + mx_kq<KQP>(Q, g) + jj : p * PJ * MX_EM + 16 * Q + 4 * g + jj) * MX_HH + n];
        }
        if (p > 0) __syncthreads();          // the previous pass's readers of G1 are done
#pragma unroll
        for (int jj = 0; jj < PJ; ++jj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const int64_t m = m0 + row;
                // (w1r is indexed with the run-time pass: selected through a compile-time scan so that it stays in registers)
                float w = 0.0f, qj = 0.0f;
#pragma unroll
                for (int pp = 0; pp < NP; ++pp) {
                    w = (pp == p) ? w1r[pp * PJ + jj][r] : w;
                    qj = (pp == p) ? qv[r][pp * PJ + jj] : qj;
                }
                const int j = p * PJ + jj;
                const float gw = (w >= 0.0f && w <= 5.0f) ? ghid[r] * qj : 0.0f;
                G1[row * LDG + jj * MX_EM + e] = gw;
                if (m < io.M) io.g_w1raw[m * (J * MX_EM) + j * MX_EM + e] = gw;
                const float t = mx_sum16(ghid[r] * mx_clamp(w, 0.0f, 5.0f));
                if (li == 0) gq_part[wave][row][j] = t;
            }
        }
        __syncthreads();
        if constexpr (BF) {
#pragma unroll
            for (int P = 0; P < KQP / 2; ++P) {
                const bf16x8 a = mx_a_bf16<KQP>(G1 + li * LDG, P, g);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) a1[tt] = mx_mfma_bf16(a, mx_b_bf16<KQP>(D1[tt], P), a1[tt]);
            }
        } else {
            const float* gp = G1 + li * LDG + 4 * g;
#pragma unroll
            for (int Q = 0; Q < KQP; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(gp + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) a1[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], D1[tt][Q][jj], a1[tt], 0, 0, 0);
            }
        }
    }
    // dL/dq: the four embed blocks' partial sums in fixed order (gq_part complete: barrier inside the last pass)
    for (int idx = threadIdx.x; idx < 16 * J; idx += 256) {
        const int row = idx / J, j = idx - row * J;
        if (m0 + row < io.M)
            io.gq[(m0 + row) * J + j] = (gq_part[0][row][j] + gq_part[1][row][j]) + (gq_part[2][row][j] + gq_part[3][row][j]);
    }
    {
        f32x4 Df[2][KQF], af[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int n = 16 * (2 * wave + tt) + li;
            af[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int Q = 0; Q < KQF; ++Q)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) Df[tt][Q][jj] = io.Wf2[(int64_t)(BF ? mx_kq<KQF>(Q, g) + jj : 16 * Q + 4 * g + jj) * MX_HH + n];
        }
        if constexpr (BF) {
#pragma unroll
            for (int P = 0; P < KQF / 2; ++P) {
                const bf16x8 a = mx_a_bf16<KQF>(Gf + li * LDF, P, g);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) af[tt] = mx_mfma_bf16(a, mx_b_bf16<KQF>(Df[tt], P), af[tt]);
            }
        } else {
            const float* fp = Gf + li * LDF + 4 * g;
#pragma unroll
            for (int Q = 0; Q < KQF; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(fp + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) af[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], Df[tt][Q][jj], af[tt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int n = 16 * (2 * wave + tt) + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const int64_t m = m0 + row;
                if (m < io.M) {
                    io.gout1[m * MX_N1 + n] = (Hs[row * MX_LDH + n] > 0.0f) ? a1[tt][r] : 0.0f;
                    io.gout1[m * MX_N1 + MX_HH + n] = (Hs[row * MX_LDH + MX_HH + n] > 0.0f) ? af[tt][r] : 0.0f;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 16 * MX_EM / 256; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int row = idx / MX_EM, k = idx - row * MX_EM;
        if (m0 + row < io.M)
            io.gout1[(m0 + row) * MX_N1 + 2 * MX_HH + k] = (Hs[row * MX_LDH + 2 * MX_HH + k] > 0.0f) ? gv_s[row] * wvo[i] : 0.0f;
    }
}

// Narrow state rows: S so small that first-layer fragment quads in front of the last one reach past a row of W1
// (mx_load_frags, RAGGED = 2).  No shipped scenario is (S = 24 / 46 / 92 / 184 at J = 2 / 3 / 6 / 12): those keep the kernels
// that load whole quads there.
static bool mixerf_narrow(const macjd_mixerf_io* io) {
    const int nrag = (io->operand_dtype && io->J % 2 == 0) ? 2 : 1;   // NRAG of mx_load_frags
    return io->S <= 16 * (io->J - nrag);
}
// (only the f32 operand type has NARROW instantiations: mixerf_check turns narrow rows away at bf16)

static int mixerf_check(const macjd_mixerf_io* io, bool backward, bool gy_from_td = false) {
    if (!io) return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused: NULL io");
    if (io->operand_dtype != 0 && io->operand_dtype != 1)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused: operand_dtype must be 0 (f32) or 1 (bf16)");
    if (!macjd_mixer_fused_supported(io->J, io->S, io->Hh, io->Em))
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_mixer_fused: unsupported J / S / Hh / Em (see include/macjd_nets.h)");
    if (io->operand_dtype == 1 && mixerf_narrow(io))
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_mixer_fused: bf16 operands need S > 16 (J - 1) (even J: 16 (J - 2)), see include/macjd_nets.h");
    if (io->M < 0 || !io->q || !io->W2 || !io->b2 || !io->Wf2 || !io->bf2 || !io->wV2 || !io->bV2)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused: bad M / NULL input");
    if (!backward) {
        if (!io->s || io->s_ld < io->S || !io->ln_w || !io->ln_b || !io->W1 || !io->b1 || !io->y)
            return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_forward: NULL input / output or bad s_ld");
        if (io->save && (!io->sn || !io->xhat || !io->act))
            return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_forward: save needs sn / xhat / act");
    } else if (!io->act || (!io->gy && !gy_from_td) || !io->gq || !io->gout1 || !io->g_w1raw || !io->g_wfraw || !io->g_v) {
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_backward: NULL input / output");
    }
    if (((uintptr_t)io->act) & 15)   // (weights may sit anywhere in a flat parameter vector: their fragment loads assume 4 bytes)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused: act must be 16-byte aligned");
    return MACJD_OK;
}

// launches of one operand type and row kind (the entry points below have checked the arguments)
template <bool BF, bool NARROW>
static void mixerf_launch_forward(const macjd_mixerf_io* io, dim3 grid, dim3 block, hipStream_t s) {
#define MACJD_MXF(J_, SQ_)                                                                                          \
    do {                                                                                                            \
        if (io->save) hipLaunchKernelGGL((mixer_fused_forward_kernel<J_, SQ_, true, BF, NARROW>), grid, block, 0, s, *io);  \
        else hipLaunchKernelGGL((mixer_fused_forward_kernel<J_, SQ_, false, BF, NARROW>), grid, block, 0, s, *io);          \
    } while (0)
    if (io->J == 2) MACJD_MXF(2, 2);
    else if (io->J == 3) MACJD_MXF(3, 3);
    else if (io->J == 6) MACJD_MXF(6, 6);
    else if (io->save) hipLaunchKernelGGL((mixer_fused_forward_wide_kernel<12, 12, true, 4, BF, NARROW>), grid, block, 0, s, *io);
    else hipLaunchKernelGGL((mixer_fused_forward_wide_kernel<12, 12, false, 4, BF, NARROW>), grid, block, 0, s, *io);
#undef MACJD_MXF
}

template <bool BF, bool NARROW>
static void mixerf_launch_pair(const macjd_mixerf_io* saved, const macjd_mixerf_io* plain, dim3 grid, dim3 block, hipStream_t s) {
    if (saved->J == 2) hipLaunchKernelGGL((mixer_fused_forward_pair_kernel<2, 2, BF, NARROW>), grid, block, 0, s, *saved, *plain);
    else if (saved->J == 3) hipLaunchKernelGGL((mixer_fused_forward_pair_kernel<3, 3, BF, NARROW>), grid, block, 0, s, *saved, *plain);
    else if (saved->J == 6) hipLaunchKernelGGL((mixer_fused_forward_pair_kernel<6, 6, BF, NARROW>), grid, block, 0, s, *saved, *plain);
    else hipLaunchKernelGGL((mixer_fused_forward_wide_pair_kernel<12, 12, 4, BF, NARROW>), grid, block, 0, s, *saved, *plain);
}

template <bool TD, bool BF>
static void mixerf_launch_backward(const macjd_mixerf_io* io, const macjd_tdloss_io& td, const float* tot_m, dim3 grid, dim3 block,
                                   hipStream_t s) {
    if (io->J == 2) hipLaunchKernelGGL((mixer_fused_backward_kernel<2, TD, BF>), grid, block, 0, s, *io, td, tot_m);
    else if (io->J == 3) hipLaunchKernelGGL((mixer_fused_backward_kernel<3, TD, BF>), grid, block, 0, s, *io, td, tot_m);
    else if (io->J == 6) hipLaunchKernelGGL((mixer_fused_backward_kernel<6, TD, BF>), grid, block, 0, s, *io, td, tot_m);
    else hipLaunchKernelGGL((mixer_fused_backward_wide_kernel<12, 4, TD, BF>), grid, block, 0, s, *io, td, tot_m);
}

template <bool BF, bool NARROW>
static void mixerf_launch_train(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                const float* tot_m, dim3 grid, dim3 block, hipStream_t s) {
    if (eval->J == 2) hipLaunchKernelGGL((mixer_fused_train_kernel<2, BF, NARROW>), grid, block, 0, s, *eval, *target, *td, tot_m);
    else hipLaunchKernelGGL((mixer_fused_train_kernel<3, BF, NARROW>), grid, block, 0, s, *eval, *target, *td, tot_m);
}

template <bool BF, bool NARROW>
static void mixerf_launch_train_static(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                       const float* tot_m, dim3 grid, dim3 block, hipStream_t s) {
    if (eval->J == 2) hipLaunchKernelGGL((mixer_fused_train_kernel<2, BF, NARROW, true>), grid, block, 0, s, *eval, *target, *td, tot_m);
    else hipLaunchKernelGGL((mixer_fused_train_kernel<3, BF, NARROW, true>), grid, block, 0, s, *eval, *target, *td, tot_m);
}

// floats of `slots` slots of an [M, N] weight-gradient problem with their bias rows (= macjd_wgrad_slot_floats: tiles of 64)
static int64_t mixerf_wgrad_slot_floats(int64_t M, int64_t N, int64_t slots) {
    const int64_t Mp = (M + 63) / 64 * 64, Np = (N + 63) / 64 * 64;
    return slots * Mp * Np + slots * Mp;
}

template <bool NARROW>
static void mixerf_launch_train_wgrad(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                      const float* tot_m, const macjd_mixer_wgrad_block* wg, dim3 grid, dim3 block, hipStream_t s) {
    if (eval->J == 2) hipLaunchKernelGGL((mixer_fused_train_wgrad_kernel<2, NARROW>), grid, block, 0, s, *eval, *target, *td, tot_m, *wg);
    else hipLaunchKernelGGL((mixer_fused_train_wgrad_kernel<3, NARROW>), grid, block, 0, s, *eval, *target, *td, tot_m, *wg);
}

// the argument checks the two training entry points share (`eval` with the output pointers its kernel writes through)
static int mixerf_train_check(const char* fn, const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                              const float* tot_m) {
    int rc = mixerf_check(eval, false);
    if (rc != MACJD_OK) return rc;
    rc = mixerf_check(eval, true, true);
    if (rc != MACJD_OK) return rc;
    rc = mixerf_check(target, false);
    if (rc != MACJD_OK) return rc;
    if (!eval->save || target->save) return set_err(MACJD_EINVAL, "%s: the eval mixer saves, the target mixer does not", fn);
    if (eval->J != target->J || eval->S != target->S || eval->M != target->M)
        return set_err(MACJD_EINVAL, "%s: the two mixers differ in J / S / M", fn);
    if (eval->operand_dtype != target->operand_dtype)
        return set_err(MACJD_EINVAL, "%s: the two mixers differ in operand_dtype", fn);
    if (eval->J != 2 && eval->J != 3) return set_err(MACJD_EINVAL, "%s: J must be 2 or 3", fn);
    if (!td || !tot_m || td->B < 1 || td->Tm1 < 1 || !td->y || !td->tq || !td->reward || !td->terminated || !td->filled)
        return set_err(MACJD_EINVAL, "%s: bad TD-loss argument", fn);
    if (td->gy_cols < td->Tm1 + 1 || (int64_t)td->B * td->gy_cols != eval->M)
        return set_err(MACJD_EINVAL, "%s: rows must be B x gy_cols with gy_cols > Tm1", fn);
    // the loss reads eval row (b, t) and target row (b, t + 1) of the two outputs, which this launch keeps in LDS
    if (td->y != eval->y || td->y_sb != td->gy_cols || td->tq != target->y + 1 || td->tq_sb != td->gy_cols)
        return set_err(MACJD_EINVAL, "%s: td->y / td->tq must be eval->y / target->y + 1 with row pitch gy_cols", fn);
    return MACJD_OK;
}

}  // namespace macjd

extern "C" int macjd_mixer_fused_supported(int32_t J, int32_t S, int32_t Hh, int32_t Em) {
    if (Hh != macjd::MX_HH || Em != macjd::MX_EM || S < 1) return 0;
    return (J == 2 && S <= 32) || (J == 3 && S <= 48) || (J == 6 && S <= 96) || (J == 12 && S <= 192);
}

extern "C" int macjd_mixer_fused_forward(const macjd_mixerf_io* io, void* hip_stream) {
    using namespace macjd;
    const int rc = mixerf_check(io, false);
    if (rc != MACJD_OK) return rc;
    if (io->M == 0) return MACJD_OK;
    const dim3 grid((unsigned)((io->M + 15) / 16)), block(256);
    hipStream_t s = (hipStream_t)hip_stream;
    const bool narrow = mixerf_narrow(io);
    if (io->operand_dtype) mixerf_launch_forward<true, false>(io, grid, block, s);
    else narrow ? mixerf_launch_forward<false, true>(io, grid, block, s) : mixerf_launch_forward<false, false>(io, grid, block, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_mixer_fused_forward: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_mixer_fused_forward_pair(const macjd_mixerf_io* saved, const macjd_mixerf_io* plain, void* hip_stream) {
    using namespace macjd;
    int rc = mixerf_check(saved, false);
    if (rc != MACJD_OK) return rc;
    rc = mixerf_check(plain, false);
    if (rc != MACJD_OK) return rc;
    if (!saved->save || plain->save) return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_forward_pair: the first mixer saves, the second does not");
    if (saved->J != plain->J || saved->S != plain->S || saved->M != plain->M)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_forward_pair: the two mixers differ in J / S / M");
    if (saved->operand_dtype != plain->operand_dtype)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_forward_pair: the two mixers differ in operand_dtype");
    if (saved->M == 0) return MACJD_OK;
    const dim3 grid((unsigned)((saved->M + 15) / 16), 2), block(256);
    hipStream_t s = (hipStream_t)hip_stream;
    const bool narrow = mixerf_narrow(saved);
    if (saved->operand_dtype) mixerf_launch_pair<true, false>(saved, plain, grid, block, s);
    else narrow ? mixerf_launch_pair<false, true>(saved, plain, grid, block, s) : mixerf_launch_pair<false, false>(saved, plain, grid, block, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_mixer_fused_forward_pair: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_mixer_fused_backward(const macjd_mixerf_io* io, void* hip_stream) {
    using namespace macjd;
    const int rc = mixerf_check(io, true);
    if (rc != MACJD_OK) return rc;
    if (io->M == 0) return MACJD_OK;
    const dim3 grid((unsigned)((io->M + 15) / 16)), block(256);
    hipStream_t s = (hipStream_t)hip_stream;
    const macjd_tdloss_io none{};
    if (io->operand_dtype) mixerf_launch_backward<false, true>(io, none, nullptr, grid, block, s);
    else mixerf_launch_backward<false, false>(io, none, nullptr, grid, block, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_mixer_fused_backward: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_mixer_fused_backward_td(const macjd_mixerf_io* io, const macjd_tdloss_io* td, const float* tot_m,
                                             void* hip_stream) {
    using namespace macjd;
    const int rc = mixerf_check(io, true, true);
    if (rc != MACJD_OK) return rc;
    if (!td || !tot_m || td->B < 1 || td->Tm1 < 1 || !td->y || !td->tq || !td->reward || !td->terminated || !td->filled)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_backward_td: bad TD-loss argument");
    if (td->gy_cols < td->Tm1 || (int64_t)td->B * td->gy_cols != io->M || td->y_sb < td->Tm1 || td->tq_sb < td->Tm1)
        return set_err(MACJD_EINVAL, "%s", "macjd_mixer_fused_backward_td: rows must be B x gy_cols with gy_cols >= Tm1");
    if (io->M == 0) return MACJD_OK;
    // td->stats != NULL: one workgroup more, which computes the loss's logged sums (stats[0..2]) beside the others
    const dim3 grid((unsigned)((io->M + 15) / 16) + (td->stats ? 1u : 0u)), block(256);
    hipStream_t s = (hipStream_t)hip_stream;
    if (io->operand_dtype) mixerf_launch_backward<true, true>(io, *td, tot_m, grid, block, s);
    else mixerf_launch_backward<true, false>(io, *td, tot_m, grid, block, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_mixer_fused_backward_td: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_mixer_fused_train(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                       const float* tot_m, void* hip_stream) {
    using namespace macjd;
    const int rc = mixerf_train_check("macjd_mixer_fused_train", eval, target, td, tot_m);
    if (rc != MACJD_OK) return rc;
    if (eval->M == 0) return MACJD_OK;
    const dim3 grid((unsigned)((eval->M + 15) / 16)), block(512);
    hipStream_t s = (hipStream_t)hip_stream;
    const bool narrow = mixerf_narrow(eval);
    if (eval->operand_dtype) mixerf_launch_train<true, false>(eval, target, td, tot_m, grid, block, s);
    else narrow ? mixerf_launch_train<false, true>(eval, target, td, tot_m, grid, block, s) : mixerf_launch_train<false, false>(eval, target, td, tot_m, grid, block, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_mixer_fused_train: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_mixer_fused_train_static(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                              const float* tot_m, const macjd_mixer_static_io* st, void* hip_stream) {
    return macjd_mixer_fused_train_static_wgrad(eval, target, td, tot_m, st, nullptr, hip_stream);
}

extern "C" int macjd_mixer_fused_train_static_wgrad(const macjd_mixerf_io* eval, const macjd_mixerf_io* target,
                                                    const macjd_tdloss_io* td, const float* tot_m, const macjd_mixer_static_io* st,
                                                    const macjd_mixer_wgrad_block* wg, void* hip_stream) {
    using namespace macjd;
    const char* fn = wg ? "macjd_mixer_fused_train_static_wgrad" : "macjd_mixer_fused_train_static";
    if (!eval || !st) return set_err(MACJD_EINVAL, "%s: NULL argument", fn);
    if (!st->sn || !st->xhat || !st->act || !st->gout1_sum || !st->g_w1raw_sum || !st->g_wfraw_sum || !st->g_v_sum)
        return set_err(MACJD_EINVAL, "%s: NULL compact output", fn);
    // the per-row forms are not written here: a caller that passes one expects what this launch does not deliver
    if (eval->sn || eval->xhat || eval->act || eval->gout1 || eval->g_w1raw || eval->g_wfraw || eval->g_v)
        return set_err(MACJD_EINVAL, "%s: the per-row sn / xhat / act / gout1 / g_w1raw / g_wfraw / g_v must be NULL", fn);
    // the kernel writes through the eval block's pointers: in this mode they are the [n_tiles, ...] buffers
    macjd_mixerf_io ev = *eval;
    ev.sn = st->sn; ev.xhat = st->xhat; ev.act = st->act;
    ev.gout1 = st->gout1_sum; ev.g_w1raw = st->g_w1raw_sum; ev.g_wfraw = st->g_wfraw_sum; ev.g_v = st->g_v_sum;
    const int rc = mixerf_train_check(fn, &ev, target, td, tot_m);
    if (rc != MACJD_OK) return rc;
    const int64_t n_tiles = (int64_t)td->B * ((td->gy_cols + 15) / 16);
    if (st->n_tiles != n_tiles || n_tiles > 0x7fffffff)
        return set_err(MACJD_EINVAL, "%s: n_tiles must be B x ceil(gy_cols / 16)", fn);
    if (wg) {
        if (ev.operand_dtype) return set_err(MACJD_EUNSUPPORTED, "%s: f32 operands only", fn);
        if (!wg->act_q || !wg->h || !wg->idx || !wg->P || !wg->w2 || !wg->ws1 || !wg->ws2 || !wg->ln_slots || !wg->W_first)
            return set_err(MACJD_EINVAL, "%s: NULL member of the weight-gradient block", fn);
        if (wg->H != 64 || wg->A < 1 || wg->A > 15) return set_err(MACJD_EUNSUPPORTED, "%s: H = 64 and 1 <= A <= 15", fn);
        if ((((uintptr_t)wg->act_q) & 15) || (((uintptr_t)wg->h) & 15) || (wg->act_ld & 3) || (wg->h_ld & 3) || wg->act_ld < wg->H ||
            wg->h_ld < wg->H || (wg->idx_elem_size != 4 && wg->idx_elem_size != 8) || wg->w_ld < ev.S)
            return set_err(MACJD_EINVAL, "%s: bad stride, alignment or index size in the weight-gradient block", fn);
        if (wg->ws1_floats < mixerf_wgrad_slot_floats(wg->H, wg->H + wg->A + 1, n_tiles) ||
            wg->ws2_floats < mixerf_wgrad_slot_floats(1, wg->H, n_tiles) || wg->ln_floats < n_tiles * 2 * ev.S)
            return set_err(MACJD_EINVAL, "%s: a workspace of the weight-gradient block is smaller than n_tiles slots", fn);
    }
    const dim3 grid((unsigned)n_tiles), block(512);
    hipStream_t s = (hipStream_t)hip_stream;
    const bool narrow = mixerf_narrow(&ev);
    if (wg) narrow ? mixerf_launch_train_wgrad<true>(&ev, target, td, tot_m, wg, grid, block, s) : mixerf_launch_train_wgrad<false>(&ev, target, td, tot_m, wg, grid, block, s);
    else if (ev.operand_dtype) mixerf_launch_train_static<true, false>(&ev, target, td, tot_m, grid, block, s);
    else narrow ? mixerf_launch_train_static<false, true>(&ev, target, td, tot_m, grid, block, s) : mixerf_launch_train_static<false, false>(&ev, target, td, tot_m, grid, block, s);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_mixer_fused_train_static: %s", hipGetErrorString(err));
    return MACJD_OK;
}
