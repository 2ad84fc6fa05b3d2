// macjd_actor_grad.hip — gradient of the MP-DQN actor objective  L = - sum_n m_n sum_a Q(h_n, a, P_a(x_n))  down to the
// output gradients of the three actor layers, ONE launch, exact float32 (v_mfma_f32_16x16x4_f32).  C-ABI and the
// per-row formulas: include/macjd_nets.h (macjd_actor_grad_io).
//
// A workgroup is 4 waves = 64 rows; each wave owns 16 rows for the whole chain
//     x -> a1 -> a2 -> u -> P = sigmoid(u)       three dense layers on MFMA (operand order of macjd_mlp.hip)
//     P -> g3                                    per-action Q-head term on VALU, [N, A, H] never materialised
//     g3 -> g2 -> g1                             two transposed products on MFMA
// and keeps its activations in ONE private LDS strip [16][lda]: every stage reads its whole input into the matrix
// cores (all output tiles accumulate in registers, at most 8 tiles = 32 registers) before it overwrites the strip
// with its output, so the chain needs no barrier of its own.  The ReLU masks of a1 / a2 stay in registers as bits:
// the C tile of a forward layer (col = lane & 15 = unit, row = (lane >> 4) * 4 + reg) is the C tile of the transposed
// product that needs the mask, same lane, same register.
//
// Weights: one layer's image at a time in LDS (at 12j/16r the three images do not fit beside the strips), staged by
// the whole workgroup with plain loads (16 B per lane where the rows allow, eight rows in flight per wave) into rows of
// pitch = 8 (mod 16) floats, pad rows / columns zero.  The SAME image
// of torch's [out, in] matrix serves both directions:
//     forward     y[i, o] = sum_k act[i, k] W[o, k]    B fragment = one ds_read_b128 along W's row o
//     transposed  g[i, k] = sum_o gout[i, o] W[o, k]   B fragment = four ds_read_b32 down W's column k
// (the native layout IS the K x N operand of the transposed product: no transposed copy).  As in macjd_mlp.hip a quad
// of four MFMAs covers 16 k-values with lane group g = lane >> 4 supplying k = 16 Q + 4 g + j in MFMA j.
// Stage order: W1a, W2a, W3a + the Q-head's action / power columns, (W3a stays), W2a again.
//
// Q-head term (one wave, its 16 rows): lane (row = lane & 15, g = lane >> 4) holds base[row, k], w2[k], wp[k] for the
// H / 4 hidden units k = 16 i + 4 g + j in registers and walks the actions; z = base + W1q[k, H + a] + wp P,
// Q_a = w2 . relu(z) + b2, s_a = sum_k w2 wp [z > 0]; two xor-shuffles sum the four lane groups.
// g3 = -m s_a P (1 - P); a row with m = 0 gets +0, hence exact zeros all the way down.
// Every output element is written exactly once; no atomics, no workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/macjd.h"
#include "../../include/macjd_nets.h"
#include "macjd_err.h"

namespace macjd {

typedef float ag_f32x4 __attribute__((ext_vector_type(4)));

constexpr int AG_WAVES = 4;
constexpr int AG_LDS_BYTES = 160 * 1024;
constexpr int AG_MAX_TILES = 8;     // output tiles of one stage (hidden width <= 128)
constexpr int AG_G3_COL = 48;       // strip column where g3 starts (P occupies [0, 48))

__host__ __device__ inline int ag_pitch(int width) { return ((width + 7) / 16) * 16 + 8; }   // = 8 (mod 16), >= width
__host__ __device__ inline int ag_r16(int n) { return (n + 15) & ~15; }

struct AgGeom {
    int lda;        // strip pitch
    int ldw[3];     // image pitch of W1a / W2a / W3a
    int qw_off;     // float offset of the Q-head columns behind W3a's image
    int img_floats; // image region
};

// Whole workgroup: W [N, K] row-major -> image rows of pitch ldw, padded with zeros to [r16(N)][r16(K)].  VW floats per
// lane and load; the loads of AG_STAGE_ROWS rows are issued before the first LDS store, so a wave pays one memory latency
// per batch, not per row (one row at a time, staging W1a at 12j/16r was ~100 dependent round trips per lane).
constexpr int AG_STAGE_ROWS = 8;
template <int VW>
__device__ __forceinline__ void ag_stage_rows(float* __restrict__ img, int ldw, const float* __restrict__ W, int K, int N) {
    typedef float vec_t __attribute__((ext_vector_type(VW)));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int K16 = ag_r16(K), N16 = ag_r16(N);
    for (int c = VW * lane; c < K16; c += VW * 64) {          // VW divides K here, so a vector is all inside or all pad
        for (int r0 = wave; r0 < N16; r0 += AG_WAVES * AG_STAGE_ROWS) {
            vec_t v[AG_STAGE_ROWS];
#pragma unroll
            for (int u = 0; u < AG_STAGE_ROWS; ++u) {
                const int r = r0 + u * AG_WAVES;
                v[u] = (r < N && c < K) ? *(const vec_t*)(W + (int64_t)r * K + c) : vec_t(0.0f);
            }
#pragma unroll
            for (int u = 0; u < AG_STAGE_ROWS; ++u) {
                const int r = r0 + u * AG_WAVES;
                if (r < N16) *(vec_t*)(img + r * ldw + c) = v[u];
            }
        }
    }
}
__device__ __forceinline__ void ag_stage(float* __restrict__ img, int ldw, const float* __restrict__ W, int K, int N) {
    if ((K & 3) == 0 && (((uintptr_t)W) & 15) == 0) ag_stage_rows<4>(img, ldw, W, K, N);   // wave-uniform
    else ag_stage_rows<1>(img, ldw, W, K, N);
}

// acc[t] (t < nt) = sum over `quads` groups of 16 k-values of A (this wave's strip rows) x B (the image).
template <bool TRANS>
__device__ __forceinline__ void ag_dense(const float* __restrict__ a_ptr, const float* __restrict__ img, int ldw,
                                         int quads, int nt, ag_f32x4* acc) {
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < AG_MAX_TILES; ++t) acc[t] = ag_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < quads; ++q) {
        const ag_f32x4 a = *(const ag_f32x4*)(a_ptr + 16 * q);
        ag_f32x4 b[AG_MAX_TILES];
#pragma unroll
        for (int t = 0; t < AG_MAX_TILES; ++t) {
            if (t < nt) {
                if (!TRANS) {
                    b[t] = *(const ag_f32x4*)(img + (16 * t + li) * ldw + 16 * q + 4 * lk);
                } else {
                    const float* p = img + (16 * q + 4 * lk) * ldw + 16 * t + li;
                    b[t] = ag_f32x4{p[0], p[ldw], p[2 * ldw], p[3 * ldw]};
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < AG_MAX_TILES; ++t)
                if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[t][j], acc[t], 0, 0, 0);
    }
}

// ReLU layer epilogue: a = relu(acc + bias) -> strip, global `out` [N, width], mask bits (bit 4 t + r).
__device__ __forceinline__ uint32_t ag_relu_out(const ag_f32x4* acc, int nt, const float* __restrict__ bias, int width,
                                                float* __restrict__ strip, int lda, float* __restrict__ out, int64_t row0,
                                                int64_t n_rows) {
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    uint32_t mask = 0;
#pragma unroll
    for (int t = 0; t < AG_MAX_TILES; ++t) {
        if (t < nt) {
            const int o = 16 * t + li;
            const float bv = o < width ? bias[o] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * lk + r;
                const float v = fmaxf(acc[t][r] + bv, 0.0f);
                if (v > 0.0f) mask |= 1u << (4 * t + r);
                strip[row * lda + o] = v;      // pad columns hold relu(0) = 0
                if (o < width && row0 + row < n_rows) out[(row0 + row) * width + o] = v;
            }
        }
    }
    return mask;
}

// Transposed-product epilogue: g = acc where the mask bit is set, else +0 -> global `out` [N, width] (and the strip).
template <bool TO_STRIP>
__device__ __forceinline__ void ag_masked_out(const ag_f32x4* acc, int nt, uint32_t mask, int width, float* __restrict__ strip,
                                              int lda, float* __restrict__ out, int64_t row0, int64_t n_rows) {
    const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < AG_MAX_TILES; ++t) {
        if (t < nt) {
            const int o = 16 * t + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * lk + r;
                const float v = ((mask >> (4 * t + r)) & 1u) ? acc[t][r] : 0.0f;
                if (TO_STRIP) strip[row * lda + o] = v;   // pad columns: mask bit clear -> 0
                if (o < width && row0 + row < n_rows) out[(row0 + row) * width + o] = v;
            }
        }
    }
}

// The per-action Q-head term for this wave's 16 rows: reads P from strip columns [0, A), writes g3 to global memory
// and to strip columns [AG_G3_COL, AG_G3_COL + 16 nt3) (pad columns zero), qsum to global memory.
template <int H>
__device__ __forceinline__ void ag_qhead(const macjd_actor_grad_io& io, float* __restrict__ strip, int lda,
                                         const float* __restrict__ qw /* LDS [A + 1][H]: W1q[:, H + a] */, int nt3,
                                         int64_t row0) {
    constexpr int HQ = H / 4;
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    const int A = io.A;
    const int64_t row = row0 + li;
    const bool valid = row < io.n_rows;
    float bz[HQ], w2r[HQ], wpr[HQ];
#pragma unroll
    for (int i = 0; i < HQ / 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 16 * i + 4 * g + j;
            bz[4 * i + j] = valid ? io.base[row * io.base_ld + k] : 0.0f;
            w2r[4 * i + j] = io.w2q[k];
            wpr[4 * i + j] = qw[A * H + k];
        }
    const float m = valid ? io.m[row] : 0.0f;
    const float b2 = io.b2q ? io.b2q[0] : 0.0f;
    float qs = 0.0f;
    for (int a = 0; a < A; ++a) {
        const float P = strip[li * lda + a];
        float s = 0.0f, qv = 0.0f;
#pragma unroll
        for (int i = 0; i < HQ / 4; ++i) {
            const ag_f32x4 col = *(const ag_f32x4*)(qw + a * H + 16 * i + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * i + j;
                const float z = fmaf(wpr[e], P, bz[e] + col[j]);
                const bool pos = z > 0.0f;
                qv = pos ? fmaf(w2r[e], z, qv) : qv;
                s = pos ? fmaf(w2r[e], wpr[e], s) : s;
            }
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        qv += __shfl_xor(qv, 16, 64);
        qv += __shfl_xor(qv, 32, 64);
        qs += qv + b2;
        const float g3 = (m != 0.0f) ? -m * s * P * (1.0f - P) : 0.0f;
        if (g == (a & 3)) {
            strip[li * lda + AG_G3_COL + a] = g3;
            if (valid) io.g3[row * A + a] = g3;
        }
    }
    for (int a = A + g; a < 16 * nt3; a += 4) strip[li * lda + AG_G3_COL + a] = 0.0f;
    if (g == 0 && valid && io.qsum) io.qsum[row] = qs;
}

__global__ void __launch_bounds__(64 * AG_WAVES) actor_gradient_kernel(const macjd_actor_grad_io io, const AgGeom gm) {
    extern __shared__ __attribute__((aligned(16))) float ag_lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int S = io.S, Ha = io.Ha, A = io.A, H = io.H, lda = gm.lda;
    const int ntH = (Ha + 15) / 16, nt3 = (A + 15) / 16;
    float* strip = ag_lds + wave * 16 * lda;
    float* img = ag_lds + AG_WAVES * 16 * lda;
    const int64_t row0 = (int64_t)blockIdx.x * 64 + wave * 16;
    const float* a_ptr = strip + li * lda + 4 * lk;
    ag_f32x4 acc[AG_MAX_TILES];

    // ---- this wave's 16 input rows (missing rows and pad columns zero) + W1a
    const int S16 = ag_r16(S);
    for (int c = lane; c < S16; c += 64) {            // the 16 rows' loads in flight together
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = (row0 + r < io.n_rows && c < S) ? io.x[(row0 + r) * io.x_ld + c] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) strip[r * lda + c] = v[r];
    }
    ag_stage(img, gm.ldw[0], io.W1a, S, Ha);
    __syncthreads();
    ag_dense<false>(a_ptr, img, gm.ldw[0], S16 / 16, ntH, acc);
    const uint32_t mask1 = ag_relu_out(acc, ntH, io.b1a, Ha, strip, lda, io.a1, row0, io.n_rows);
    __syncthreads();                                  // everyone is done with W1a's image
    ag_stage(img, gm.ldw[1], io.W2a, Ha, Ha);
    __syncthreads();
    ag_dense<false>(a_ptr, img, gm.ldw[1], ntH, ntH, acc);
    const uint32_t mask2 = ag_relu_out(acc, ntH, io.b2a, Ha, strip, lda, io.a2, row0, io.n_rows);
    __syncthreads();
    // ---- W3a and, behind it, the Q-head's action / power columns as [A + 1][H]
    ag_stage(img, gm.ldw[2], io.W3a, Ha, A);
    float* qw = img + gm.qw_off;
    for (int idx = threadIdx.x; idx < (A + 1) * H; idx += 64 * AG_WAVES) {
        const int k = idx / (A + 1), a = idx - k * (A + 1);      // consecutive threads: consecutive addresses of W1q
        qw[a * H + k] = io.W1q[(int64_t)k * io.w1_ld + H + a];
    }
    __syncthreads();
    ag_dense<false>(a_ptr, img, gm.ldw[2], ntH, nt3, acc);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (t < nt3) {
            const int o = 16 * t + li;
            const float bv = o < A ? io.b3a[o] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) strip[(4 * lk + r) * lda + o] = 1.0f / (1.0f + expf(-(acc[t][r] + bv)));   // the forward kernels' sigmoid
        }
    }
    if (H == 64) ag_qhead<64>(io, strip, lda, qw, nt3, row0);
    else ag_qhead<128>(io, strip, lda, qw, nt3, row0);
    // ---- g2 = (g3 W3a) [a2 > 0]: W3a's image is still there
    ag_dense<true>(a_ptr + AG_G3_COL, img, gm.ldw[2], nt3, ntH, acc);
    ag_masked_out<true>(acc, ntH, mask2, Ha, strip, lda, io.g2, row0, io.n_rows);
    __syncthreads();                                  // everyone is done with W3a's image and the Q-head columns
    ag_stage(img, gm.ldw[1], io.W2a, Ha, Ha);
    __syncthreads();
    ag_dense<true>(a_ptr, img, gm.ldw[1], ntH, ntH, acc);
    ag_masked_out<false>(acc, ntH, mask1, Ha, strip, lda, io.g1, row0, io.n_rows);
}

// 1 and the geometry when the shape is supported, else 0
static int ag_geometry(int32_t S, int32_t Ha, int32_t H, int32_t A, AgGeom* out) {
    if (S < 1 || S > 256 || Ha < 1 || Ha > 128 || A < 1 || A > 33 || !(H == 64 || H == 128)) return 0;
    const int ntH = (Ha + 15) / 16, nt3 = (A + 15) / 16;
    if (!(ntH == 1 || ntH == 2 || ntH == 3 || ntH == 4 || ntH == 8)) return 0;   // macjd_mlp_forward's tile counts
    AgGeom g;
    const int widest = ag_r16(S) > ag_r16(Ha) ? ag_r16(S) : ag_r16(Ha);
    g.lda = ag_pitch(widest > AG_G3_COL + 16 * nt3 ? widest : AG_G3_COL + 16 * nt3);
    g.ldw[0] = ag_pitch(ag_r16(S));
    g.ldw[1] = g.ldw[2] = ag_pitch(ag_r16(Ha));
    const int i1 = ag_r16(Ha) * g.ldw[0], i2 = ag_r16(Ha) * g.ldw[1];
    g.qw_off = ag_r16(A) * g.ldw[2];
    const int i3 = g.qw_off + (A + 1) * H;
    g.img_floats = i1 > i2 ? (i1 > i3 ? i1 : i3) : (i2 > i3 ? i2 : i3);
    if ((size_t)(AG_WAVES * 16 * g.lda + g.img_floats) * 4 > (size_t)AG_LDS_BYTES) return 0;
    if (out) *out = g;
    return 1;
}

}  // namespace macjd

extern "C" int macjd_actor_gradient_supported(int32_t S, int32_t Ha, int32_t H, int32_t A) {
    return macjd::ag_geometry(S, Ha, H, A, nullptr);
}

extern "C" int macjd_actor_gradient(const macjd_actor_grad_io* io, void* hip_stream) {
    using namespace macjd;
    if (!io) return set_err(MACJD_EINVAL, "%s", "macjd_actor_gradient: NULL io");
    if (io->n_rows < 1 || io->S < 1 || io->Ha < 1 || io->H < 1 || io->A < 1)
        return set_err(MACJD_EINVAL, "%s", "macjd_actor_gradient: non-positive size");
    if (!io->x || !io->base || !io->m || !io->W1a || !io->b1a || !io->W2a || !io->b2a || !io->W3a || !io->b3a || !io->W1q ||
        !io->w2q || !io->a1 || !io->a2 || !io->g3 || !io->g2 || !io->g1)
        return set_err(MACJD_EINVAL, "%s", "macjd_actor_gradient: NULL pointer");
    if (io->x_ld < io->S || io->base_ld < io->H || io->w1_ld < (int64_t)io->H + io->A + 1)
        return set_err(MACJD_EINVAL, "%s", "macjd_actor_gradient: row stride smaller than the row");
    AgGeom g;
    if (!ag_geometry(io->S, io->Ha, io->H, io->A, &g))
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_actor_gradient: shape outside the supported range");
    const int64_t n_tiles = (io->n_rows + 63) / 64;
    if (n_tiles > 0x7fffffff) return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_actor_gradient: too many rows");
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)actor_gradient_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AG_LDS_BYTES);
        attr_set = true;
    }
    const size_t lds_bytes = (size_t)(AG_WAVES * 16 * g.lda + g.img_floats) * 4;
    hipLaunchKernelGGL(actor_gradient_kernel, dim3((unsigned)n_tiles), dim3(64 * AG_WAVES), lds_bytes, (hipStream_t)hip_stream,
                       *io, g);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_actor_gradient: %s", hipGetErrorString(err));
    return MACJD_OK;
}
