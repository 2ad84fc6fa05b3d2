// macjd_env_motion_pe.hip — PER-ENV moving scenarios (include/macjd.h, macjd_motion_pe_io).
//
// A translation unit of its own for
//   * motion_pe_compile_kernel: the device frame compiler (macjd_motion_pe_compile).  One lane per (env, frame), env fastest:
//     a wave's 64 lanes are 64 consecutive envs of one frame, so every store into the tiled tables is one contiguous piece
//     of a row.  Plain IEEE float64 in the order include/macjd.h states (the build has -ffp-contract=off); no LDS.
//   * the MOV instantiations of env_step_kernel on per-env frame tables (macjd_env_step.h, IO = MotionPeStepIO<...>): the
//     frame-table path of the moving step with row stride = the env tile, tile index (e / tile) * F + f, column e % tile.
//   * the position part of a reset on per-env frame tables.
// Every kernel built in the other translation units compiles exactly as before.  The host side of the step / reset entry
// points (validation, span checks, the many-step launch's counter advance) is in macjd_env.hip: launch_step_moving, the one
// dispatch function of the moving modes.
#include "macjd_env_step.h"
#include "macjd_err.h"

namespace macjd {

// Input rows of the compiler (include/macjd.h, MACJD_MOTION_PE_IN_ROWS): block offsets in rows
struct MpeIn {
    int Pn, D, rd_pen, gr, num, rloss, rlatm, Ga, pmin, pmax, gj, jloss, jlatm, bj, tp0, tvdt, rp0, rvdt, jp0, jvdt;
    __host__ __device__ MpeIn(int R, int J) {
        Pn = 0; D = R; rd_pen = 2 * R; gr = 3 * R; num = 4 * R; rloss = 5 * R; rlatm = 6 * R; Ga = 7 * R;
        pmin = 8 * R; pmax = pmin + J; gj = pmax + J; jloss = gj + J; jlatm = jloss + J; bj = jlatm + J;
        tp0 = bj + J; tvdt = tp0 + 2; rp0 = tvdt + 2; rvdt = rp0 + 2 * R; jp0 = rvdt + 2 * R; jvdt = jp0 + 2 * J;
    }
};

struct MotionPeCompileArgs {
    int64_t n_envs;
    int32_t R, J, F, tile;
    double c0, pd_A, pd_c1, pd_denB;
    const double* in_tables;
    const uint8_t* in_weak;
    double* frames;
    uint8_t* frame_flags;
    double* frame_snr_no;   // optional
    float* positions;
};

// Item (e, f), f = blockIdx.y in 0..F: frame f of env e.  f < F writes the frame's rows, flags and snr_no; every f writes the
// positions.  Lanes past n_envs (the last tile's padding included) store nothing.
template <int JT, int RT>
__global__ void __launch_bounds__(256) motion_pe_compile_kernel(const MotionPeCompileArgs a) {
    const int R = RT ? RT : a.R, J = JT ? JT : a.J;
    constexpr int NR = RT ? RT : 1;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_envs) return;
    const int f = (int)blockIdx.y;
    const int F = a.F;
    const int64_t w = a.tile, tl = e / w, col = e - tl * w;
    const MpeIn o(R, J);
    const int in_rows = 12 * R + 10 * J + 4;
    const double* __restrict__ in = a.in_tables + tl * in_rows * w + col;
    const uint8_t* __restrict__ wk = a.in_weak + tl * J * w + col;
    auto row = [&](int t) { return in[(int64_t)t * w]; };
    const double fd = (double)f;
    auto moved = [&](int p0_row, int vdt_row) { return row(p0_row) + fd * row(vdt_row); };
    const int n_pos = 2 * R + 2 * J;
    float* __restrict__ pos = a.positions + ((tl * (F + 1) + f) * n_pos) * w + col;
    const bool frame = f < F;
    const int64_t tf = tl * F + f;   // tile index of the frame's blocks
    double* __restrict__ fr = a.frames + tf * (6 * R + 3 * J + J * R) * w + col;
    uint8_t* __restrict__ ff = a.frame_flags + tf * (J * R) * w + col;
    double* __restrict__ fs = a.frame_snr_no ? a.frame_snr_no + tf * R * w + col : nullptr;
    const PdConsts pdk = pd_consts(a.pd_A, a.pd_c1, a.pd_denB);

    const double tx = moved(o.tp0, o.tvdt), ty = moved(o.tp0 + 1, o.tvdt + 1);
    double rxs[NR], rys[NR];   // compiled sizes keep the radars' positions for the jammer paths; generic sizes recompute
#pragma unroll
    for (int r = 0; r < (RT ? RT : R); ++r) {
        const double rx = moved(o.rp0 + 2 * r, o.rvdt + 2 * r), ry = moved(o.rp0 + 2 * r + 1, o.rvdt + 2 * r + 1);
        if constexpr (RT != 0) { rxs[r] = rx; rys[r] = ry; }
        pos[(int64_t)(2 * r) * w] = (float)rx;
        pos[(int64_t)(2 * r + 1) * w] = (float)ry;
        if (frame) {
            // target path of radar r
            const double dx = rx - tx, dy = ry - ty;
            const double d = sqrt(dx * dx + dy * dy);
            const double sd = d > 1e-6 ? d : 1e-6;
            const double d4 = (sd * sd) * (sd * sd);
            const double den = ((a.c0 * d4) * row(o.rloss + r)) * row(o.rlatm + r);
            const double Ps = den <= 1e-18 ? 0.0 : row(o.num + r) / den;
            const double GaPs = row(o.Ga + r) * Ps;
            const double Pn = row(o.Pn + r);
            const double q = Pn > 1e-18 ? GaPs / Pn : 0.0;
            const double snr_no = 0.0 > q ? 0.0 : q;   // Python max(0.0, q)
            fr[(int64_t)(r) * w] = GaPs;
            fr[(int64_t)(R + r) * w] = Pn;
            fr[(int64_t)(2 * R + r) * w] = row(o.D + r);
            fr[(int64_t)(3 * R + r) * w] = det_prob(snr_no, pdk);
            fr[(int64_t)(4 * R + r) * w] = row(o.rd_pen + r);
            fr[(int64_t)(5 * R + r) * w] = row(o.gr + r);
            if (fs) fs[(int64_t)r * w] = snr_no;
        }
    }
#pragma unroll
    for (int j = 0; j < (JT ? JT : J); ++j) {
        const double jx = moved(o.jp0 + 2 * j, o.jvdt + 2 * j), jy = moved(o.jp0 + 2 * j + 1, o.jvdt + 2 * j + 1);
        pos[(int64_t)(2 * R + 2 * j) * w] = (float)jx;
        pos[(int64_t)(2 * R + 2 * j + 1) * w] = (float)jy;
        if (frame) {
            fr[(int64_t)(6 * R + j) * w] = row(o.pmin + j);
            fr[(int64_t)(6 * R + J + j) * w] = row(o.pmax + j);
            fr[(int64_t)(6 * R + 2 * J + j) * w] = row(o.gj + j);
            const double loss = row(o.jloss + j), latm = row(o.jlatm + j), bj = row(o.bj + j);
            const uint8_t weak = wk[(int64_t)j * w];
#pragma unroll
            for (int r = 0; r < (RT ? RT : R); ++r) {
                double rx, ry;
                if constexpr (RT != 0) { rx = rxs[r]; ry = rys[r]; }
                else { rx = moved(o.rp0 + 2 * r, o.rvdt + 2 * r); ry = moved(o.rp0 + 2 * r + 1, o.rvdt + 2 * r + 1); }
                const double dx = jx - rx, dy = jy - ry;
                const double d = sqrt(dx * dx + dy * dy);
                double denom = -1.0;
                uint8_t flag = 0;
                if (d > 1e-6) {
                    const double d2 = d * d;
                    const bool big = d2 > 1e-9;
                    const double dsq = big ? d2 : 1e-9;
                    denom = ((dsq * loss) * latm) * bj;
                    flag = (!big && weak) ? (uint8_t)MACJD_JR_WEAK_DENOM : (uint8_t)0;
                }
                fr[(int64_t)(6 * R + 3 * J + j * R + r) * w] = denom;
                ff[(int64_t)(j * R + r) * w] = flag;
            }
        }
    }
}

// position part of a reset (macjd_env_reset_moving_pe): each masked env's own frame-0 positions into its state row
__global__ void env_reset_motion_pe_kernel(int64_t n_envs, int n_pos, int n_frames, int tile, const float* __restrict__ positions,
                                           const int32_t* __restrict__ position_columns, float* state, int64_t st_se,
                                           const uint8_t* mask) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_envs; e += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[e]) continue;
        const int64_t tl = e / tile, col = e - tl * tile;
        const float* __restrict__ pos = positions + (tl * (n_frames + 1) * n_pos) * tile + col;
        for (int i = 0; i < n_pos; ++i) state[e * st_se + position_columns[i]] = pos[(int64_t)i * tile];
    }
}

// launch_motion_sized<FAST, SCAN = false, PAT = false>
MACJD_LAUNCH_MOTION(MotionPeStepIO<FastStepIO>) { return launch_motion_sized<true, false, false>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionPeStepIO<macjd_step_io>) { return launch_motion_sized<false, false, false>(J, R, grid, block, stream, dev, io); }

void launch_motion_pe_reset(dim3 grid, dim3 block, hipStream_t stream, int64_t n_envs, int n_pos, int n_frames, int tile,
                            const float* positions, const int32_t* position_columns, float* state, int64_t st_se,
                            const uint8_t* mask) {
    hipLaunchKernelGGL(env_reset_motion_pe_kernel, grid, block, 0, stream, n_envs, n_pos, n_frames, tile, positions,
                       position_columns, state, st_se, mask);
}

}  // namespace macjd

extern "C" int macjd_motion_pe_compile(const macjd_motion_pe_compile_desc* d, void* hip_stream) {
    using macjd::set_err;
    const char* me = "macjd_motion_pe_compile";
    if (!d) return set_err(MACJD_EINVAL, "%s: NULL descriptor", me);
    const int R = d->n_radars, J = d->n_jammers;
    if (R < 1 || R > MACJD_MAX_RADARS || J < 1 || J > MACJD_MAX_JAMMERS) return set_err(MACJD_EINVAL, "%s: n_radars / n_jammers out of range", me);
    if (d->n_envs < 0 || d->n_frames < 1 || d->n_frames > 65534 || d->tile < 1)
        return set_err(MACJD_EINVAL, "%s: needs n_envs >= 0, 1 <= n_frames <= 65534, tile >= 1", me);
    if (!d->in_tables || !d->in_weak || !d->frames || !d->frame_flags || !d->positions)
        return set_err(MACJD_EINVAL, "%s: in_tables / in_weak / frames / frame_flags / positions is NULL", me);
    if (d->n_envs == 0) return MACJD_OK;
    macjd::MotionPeCompileArgs a{};
    a.n_envs = d->n_envs; a.R = R; a.J = J; a.F = d->n_frames; a.tile = d->tile;
    a.c0 = d->four_pi_cubed; a.pd_A = d->pd_A; a.pd_c1 = d->pd_c1; a.pd_denB = d->pd_denB;
    a.in_tables = d->in_tables; a.in_weak = d->in_weak;
    a.frames = d->frames; a.frame_flags = d->frame_flags; a.frame_snr_no = d->frame_snr_no; a.positions = d->positions;
    const int block = d->n_envs >= 256 ? 256 : 64;
    const int64_t bx = (d->n_envs + block - 1) / block;
    if (bx > 0x7fffffff) return set_err(MACJD_EINVAL, "%s: too many envs for one launch", me);
    const dim3 g((unsigned)bx, (unsigned)(d->n_frames + 1)), b(block);
    hipStream_t stream = (hipStream_t)hip_stream;
    if (J == 3 && R == 4) hipLaunchKernelGGL((macjd::motion_pe_compile_kernel<3, 4>), g, b, 0, stream, a);
    else if (J == 6 && R == 8) hipLaunchKernelGGL((macjd::motion_pe_compile_kernel<6, 8>), g, b, 0, stream, a);
    else if (J == 2 && R == 2) hipLaunchKernelGGL((macjd::motion_pe_compile_kernel<2, 2>), g, b, 0, stream, a);
    else hipLaunchKernelGGL((macjd::motion_pe_compile_kernel<0, 0>), g, b, 0, stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_motion_pe_compile launch: %s", hipGetErrorString(err));
    return MACJD_OK;
}
