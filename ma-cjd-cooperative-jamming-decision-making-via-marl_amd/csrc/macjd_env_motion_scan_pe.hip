// macjd_env_motion_scan_pe.hip — PER-ENV moving scenarios under SCANNING radars (include/macjd.h, macjd_motion_scan_pe_io).
//
// A translation unit of its own for
//   * motion_scan_pe_compile_kernel: the device compiler of the beam frames (macjd_motion_scan_pe_compile).  One lane per
//     (env, frame f < F), env fastest: a wave's 64 lanes are 64 consecutive envs of one frame, so every store into the tiled
//     tables is one contiguous piece of a row.  It runs after macjd_motion_pe_compile on the same stream and reads that
//     compiler's GaPs / Pn / pd_no / gr rows and frame_snr_no.  Arithmetic of an item, plain IEEE float64 in this order (the
//     build has -ffp-contract=off: no fused multiply-add), fd = (double)f:
//       position per axis   p = p0 + fd * vdt                       (the first compiler's expression: the same bits)
//       bearing of object o from radar r:  a = atan2(oy - ry, ox - rx);  d = a * deg_per_rad;  b = d - 360.0 * floor(d / 360.0)
//                           bear_tgt[r]: o = the target;  bear_jam[j * R + r]: o = jammer j
//       side lobe           gr_side = gr * rho;  GaPs_side = GaPs * (rho * rho);
//                           snr_no_side = max(0, Pn > 1e-18 ? GaPs_side / Pn : 0);  pd_no_side = det_prob(snr_no_side)
//       levels k = 1..L     the same four expressions with rho_lvl[k - 1]
//       copies              level 0 = the main rows (GaPs, frame_snr_no, pd_no, gr), level L + 1 = the side rows; half_beam,
//                           sweep, sweep_mod, az0, inv_width copied through; the snr_no row = frame_snr_no
//     The only step whose bits are not pinned by IEEE 754 is the device library's atan2.  No LDS.
//   * the MOV && SCAN instantiations of env_step_kernel on per-env frame tables (macjd_env_step.h, IO =
//     MotionScanPeStepIO<...>), with and without PAT: the moving-scanning step with row stride = the env tile, tile index
//     (e / tile) * F + f, column e % tile for the step's own rows, the scan rows and the pattern's level rows.  The size-bounded
//     loops are unrolled by an explicit count, as in macjd_env_motion_scan.hip.
//   * the beam part of a reset on per-env beam frames.
// Every kernel built in the other translation units compiles exactly as before.  The host side of the step / reset entry
// points (validation, span checks) is in macjd_env.hip: launch_step_moving, the one dispatch function of the moving modes.
#define MACJD_ENV_PRAGMA(x) _Pragma(#x)
#define MACJD_ENV_UNROLL_SIZED(N) MACJD_ENV_PRAGMA(unroll N)
#include "macjd_env_step.h"
#include "macjd_err.h"

namespace macjd {

struct MotionScanPeCompileArgs {
    int64_t n_envs;
    int32_t R, J, F, tile, L;
    double deg_per_rad, pd_A, pd_c1, pd_denB;
    const double* in_tables;
    const double* scan_in;
    const double* frames;
    const double* frame_snr_no;
    double* scan_frames;
    double* pattern_frames;   // L > 0
};

// wrap(deg(atan2(oy - ry, ox - rx))) in the order the header comment states
__device__ __forceinline__ double bearing_deg(double rx, double ry, double ox, double oy, double deg_per_rad) {
    const double a = atan2(oy - ry, ox - rx);
    const double d = a * deg_per_rad;
    return d - 360.0 * floor(d / 360.0);
}

// Item (e, f), f = blockIdx.y in 0..F-1: the scan rows (and under a pattern the level rows) of frame f of env e.  Lanes past
// n_envs (the last tile's padding included) store nothing.
__global__ void __launch_bounds__(256) motion_scan_pe_compile_kernel(const MotionScanPeCompileArgs a) {
    const int R = a.R, J = a.J, L = a.L;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_envs) return;
    const int f = (int)blockIdx.y;
    const int64_t w = a.tile, tl = e / w, col = e - tl * w;
    const int64_t tf = tl * a.F + f;   // tile index of the frame's blocks
    // input rows of the first compiler that hold the positions (MACJD_MOTION_PE_IN_ROWS)
    const int in_rows = 12 * R + 10 * J + 4;
    const int tp0 = 8 * R + 6 * J, tvdt = tp0 + 2, rp0 = tvdt + 2, rvdt = rp0 + 2 * R, jp0 = rvdt + 2 * R, jvdt = jp0 + 2 * J;
    const double* __restrict__ in = a.in_tables + tl * in_rows * w + col;
    const int sin_rows = 4 * R + 1 + (L > 0 ? R + L : 0);
    const double* __restrict__ si = a.scan_in + tl * sin_rows * w + col;
    const double* __restrict__ fr = a.frames + tf * (6 * R + 3 * J + J * R) * w + col;
    const double* __restrict__ fs = a.frame_snr_no + tf * R * w + col;
    double* __restrict__ sf = a.scan_frames + tf * (10 * R + J * R) * w + col;
    const int64_t lvR = (int64_t)(L + 2) * R;
    double* __restrict__ pf = L > 0 ? a.pattern_frames + tf * (R + 4 * lvR) * w + col : nullptr;
    const PdConsts pdk = pd_consts(a.pd_A, a.pd_c1, a.pd_denB);
    const double fd = (double)f;
    auto moved = [&](int p0_row, int vdt_row) { return in[(int64_t)p0_row * w] + fd * in[(int64_t)vdt_row * w]; };
    const double rho = si[(int64_t)(4 * R) * w];
    const double tx = moved(tp0, tvdt), ty = moved(tp0 + 1, tvdt + 1);
    for (int r = 0; r < R; ++r) {
        const double rx = moved(rp0 + 2 * r, rvdt + 2 * r), ry = moved(rp0 + 2 * r + 1, rvdt + 2 * r + 1);
        const double GaPs = fr[(int64_t)r * w], Pn = fr[(int64_t)(R + r) * w];
        const double pd_no = fr[(int64_t)(3 * R + r) * w], gr = fr[(int64_t)(5 * R + r) * w];
        const double snr_no = fs[(int64_t)r * w];
        // one lobe level of gain rho_k: gr_k, GaPs_k, snr_no_k, pd_no_k by the host's side-lobe expressions
        auto level = [&](double rho_k, double& gr_k, double& GaPs_k, double& snr_k, double& pd_k) {
            gr_k = gr * rho_k;
            GaPs_k = GaPs * (rho_k * rho_k);
            const double q = Pn > 1e-18 ? GaPs_k / Pn : 0.0;
            snr_k = 0.0 > q ? 0.0 : q;   // Python max(0.0, q)
            pd_k = det_prob(snr_k, pdk);
        };
        double gr_s, GaPs_s, snr_s, pd_s;
        level(rho, gr_s, GaPs_s, snr_s, pd_s);
        sf[(int64_t)(0 * R + r) * w] = si[(int64_t)(0 * R + r) * w];   // half_beam
        sf[(int64_t)(1 * R + r) * w] = si[(int64_t)(1 * R + r) * w];   // sweep
        sf[(int64_t)(2 * R + r) * w] = si[(int64_t)(2 * R + r) * w];   // sweep_mod
        sf[(int64_t)(3 * R + r) * w] = si[(int64_t)(3 * R + r) * w];   // az0
        sf[(int64_t)(4 * R + r) * w] = bearing_deg(rx, ry, tx, ty, a.deg_per_rad);
        sf[(int64_t)(5 * R + r) * w] = GaPs_s;
        sf[(int64_t)(6 * R + r) * w] = snr_no;
        sf[(int64_t)(7 * R + r) * w] = snr_s;
        sf[(int64_t)(8 * R + r) * w] = pd_s;
        sf[(int64_t)(9 * R + r) * w] = gr_s;
        for (int j = 0; j < J; ++j) {
            const double jx = moved(jp0 + 2 * j, jvdt + 2 * j), jy = moved(jp0 + 2 * j + 1, jvdt + 2 * j + 1);
            sf[(int64_t)(10 * R + j * R + r) * w] = bearing_deg(rx, ry, jx, jy, a.deg_per_rad);
        }
        if (L > 0) {
            // level tables GaPs | snr_no | pd_no | gr, each [(L + 2) R] level-major after inv_width's R rows
            auto lrow = [&](int tab, int k) -> double& { return pf[((int64_t)R + tab * lvR + (int64_t)k * R + r) * w]; };
            pf[(int64_t)r * w] = si[(int64_t)(4 * R + 1 + r) * w];   // inv_width
            lrow(0, 0) = GaPs; lrow(1, 0) = snr_no; lrow(2, 0) = pd_no; lrow(3, 0) = gr;
            for (int k = 1; k <= L; ++k) {
                double gr_k, GaPs_k, snr_k, pd_k;
                level(si[(int64_t)(5 * R + 1 + (k - 1)) * w], gr_k, GaPs_k, snr_k, pd_k);
                lrow(0, k) = GaPs_k; lrow(1, k) = snr_k; lrow(2, k) = pd_k; lrow(3, k) = gr_k;
            }
            lrow(0, L + 1) = GaPs_s; lrow(1, L + 1) = snr_s; lrow(2, L + 1) = pd_s; lrow(3, L + 1) = gr_s;
        }
    }
}

// beam part of a reset (macjd_env_reset_moving_scan_pe): each masked env's own frame-0 az0 row into theta_a and its state row
__global__ void env_reset_motion_scan_pe_kernel(int64_t n_envs, int R, int J, int n_frames, int tile,
                                                const double* __restrict__ scan_frames, double* theta_a, int64_t a_se, int64_t a_sx,
                                                float* state, int64_t st_se, int32_t st_col0, int32_t st_col_step, const uint8_t* mask) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_envs; e += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[e]) continue;
        const int64_t tl = e / tile, col = e - tl * tile;
        const double* __restrict__ sp = scan_frames + (tl * n_frames * (10 * R + J * R)) * tile + col;   // frame 0
        for (int r = 0; r < R; ++r) {
            const double a0 = sp[(int64_t)(3 * R + r) * tile];   // row block az0
            theta_a[e * a_se + (int64_t)r * a_sx] = a0;
            if (state) state[e * st_se + st_col0 + (int64_t)r * st_col_step] = (float)a0;
        }
    }
}

// launch_motion_sized<FAST, SCAN = true, PAT>
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPeStepIO<FastStepIO>>) { return launch_motion_sized<true, true, false>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPeStepIO<macjd_step_io>>) { return launch_motion_sized<false, true, false>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPePatStepIO<FastStepIO>>) { return launch_motion_sized<true, true, true>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPePatStepIO<macjd_step_io>>) { return launch_motion_sized<false, true, true>(J, R, grid, block, stream, dev, io); }

void launch_motion_scan_pe_reset(dim3 grid, dim3 block, hipStream_t stream, int64_t n_envs, int R, int J, int n_frames, int tile,
                                 const double* scan_frames, double* theta_a, int64_t a_se, int64_t a_sx, float* state,
                                 int64_t st_se, int32_t st_col0, int32_t st_col_step, const uint8_t* mask) {
    hipLaunchKernelGGL(env_reset_motion_scan_pe_kernel, grid, block, 0, stream, n_envs, R, J, n_frames, tile, scan_frames, theta_a,
                       a_se, a_sx, state, st_se, st_col0, st_col_step, mask);
}

}  // namespace macjd

extern "C" int macjd_motion_scan_pe_compile(const macjd_motion_scan_pe_compile_desc* d, void* hip_stream) {
    using macjd::set_err;
    const char* me = "macjd_motion_scan_pe_compile";
    if (!d) return set_err(MACJD_EINVAL, "%s: NULL descriptor", me);
    const int R = d->n_radars, J = d->n_jammers, L = d->n_levels;
    if (R < 1 || R > MACJD_MAX_RADARS || J < 1 || J > MACJD_MAX_JAMMERS) return set_err(MACJD_EINVAL, "%s: n_radars / n_jammers out of range", me);
    if (L < 0 || L > MACJD_MAX_PATTERN_LEVELS) return set_err(MACJD_EINVAL, "%s: n_levels outside 0..MACJD_MAX_PATTERN_LEVELS", me);
    if (d->n_envs < 0 || d->n_frames < 1 || d->n_frames > 65534 || d->tile < 1)
        return set_err(MACJD_EINVAL, "%s: needs n_envs >= 0, 1 <= n_frames <= 65534, tile >= 1", me);
    if (!d->in_tables || !d->scan_in || !d->frames || !d->frame_snr_no || !d->scan_frames)
        return set_err(MACJD_EINVAL, "%s: in_tables / scan_in / frames / frame_snr_no / scan_frames is NULL", me);
    if ((d->pattern_frames != nullptr) != (L > 0))
        return set_err(MACJD_EINVAL, "%s: pattern_frames and n_levels > 0 go together (both or neither)", me);
    if (d->n_envs == 0) return MACJD_OK;
    macjd::MotionScanPeCompileArgs a{};
    a.n_envs = d->n_envs; a.R = R; a.J = J; a.F = d->n_frames; a.tile = d->tile; a.L = L;
    a.deg_per_rad = d->deg_per_rad; a.pd_A = d->pd_A; a.pd_c1 = d->pd_c1; a.pd_denB = d->pd_denB;
    a.in_tables = d->in_tables; a.scan_in = d->scan_in; a.frames = d->frames; a.frame_snr_no = d->frame_snr_no;
    a.scan_frames = d->scan_frames; a.pattern_frames = d->pattern_frames;
    const int block = d->n_envs >= 256 ? 256 : 64;
    const int64_t bx = (d->n_envs + block - 1) / block;
    if (bx > 0x7fffffff) return set_err(MACJD_EINVAL, "%s: too many envs for one launch", me);
    const dim3 g((unsigned)bx, (unsigned)d->n_frames), b(block);
    hipLaunchKernelGGL(macjd::motion_scan_pe_compile_kernel, g, b, 0, (hipStream_t)hip_stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_motion_scan_pe_compile launch: %s", hipGetErrorString(err));
    return MACJD_OK;
}
