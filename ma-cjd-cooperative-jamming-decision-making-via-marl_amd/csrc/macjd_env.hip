// macjd_env.hip — batched radar-jamming environment step for MI355X (gfx950, wave64).
//
// One lane = one environment.  The kernel is the batched form of
// ElectromagneticEnvironment.step (reference simulation/environment.py:221-477) with the helpers it
// calls (core/radar.py:67-82 detection probability, :90-119 SEARCH/TRACK FSM; core/jammer.py:56-98
// received jamming power).  All arithmetic is float64 in the reference's operation order (the TU is
// built with -ffp-contract=off: Python never fuses multiply-add), except the power /
// received-power numerator which follows NumPy-2's float32 weak-scalar promotion when the power
// action arrives as float32 (see include/macjd.h, MACJD_STEP_ARITH_F64).
//
// Data movement (HBM-bound streaming kernel; see DESIGN.md for the byte count):
//   * per-env inputs/outputs are addressed through caller-supplied element strides, so the runner
//     can keep actions agent-major ([J,E]: every load instruction is a fully coalesced 256-B row) while
//     the reference-shaped env-major layout ([E,J]) stays valid;
//   * per-radar constants that are indexed by the (compile-time unrolled) radar loop are read
//     through wave-uniform scalar loads from the scenario table;
//   * tables that are indexed by the lane's *chosen target radar* (jammer->radar path denominators,
//     D, Pn, receive gain) are staged once per workgroup into LDS and gathered with ds_read.
//
// The whole scenario is templated on (J, R) for the BASELINE.json configurations so that the
// suppression / deception accumulators live in registers; a generic (0,0) instantiation covers
// every other size up to MACJD_MAX_*.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <stddef.h>
#include <string.h>
#include <type_traits>

#include "../../include/macjd.h"
#include "macjd_env_dev.h"
#include "macjd_env_plan.h"
#include "macjd_env_step.h"
#include "macjd_err.h"
#include "macjd_philox.h"

namespace macjd {

static thread_local char g_err[512] = "";
int set_err(int code, const char* fmt, const char* a) {
    snprintf(g_err, sizeof(g_err), fmt, a);
    return code;
}

// Process-wide switches of the env launches, read from the environment ONCE (macjd_reload_options re-reads them: tests
// and A/B runs that change a switch inside one process).
static EnvOptions g_env_options = {true, true, false};
static bool g_env_options_loaded = false;
static void load_env_options() {
    const char* a = getenv("MACJD_ENV_REGULAR");
    const char* b = getenv("MACJD_ENV_PD32");
    const char* c = getenv("MACJD_GRU_SCAN");
    g_env_options.regular = !(a && a[0] == '0');
    g_env_options.pd32 = !(b && b[0] == '0');
    g_env_options.gru_ksplit = c && !strcmp(c, "ksplit");
    g_env_options_loaded = true;
}
const EnvOptions& env_options() {
    if (!g_env_options_loaded) load_env_options();
    return g_env_options;
}

// ---------------------------------------------------------------------------------------------
// env_step_slots_kernel: one lane = one (env, slot) pair, slot = a jammer or a radar.
//
// Workgroup = 64 consecutive envs x (NJW jammer waves + NRW radar waves).  Lane l of every wave works on
// env 64*blockIdx.x + l, so agent-major / radar-major tensors are read and written as whole 256-B rows.
//   phase 1  jammer waves: decode, power, r_p term, received power          -> LDS (prj, meta, r_p term)
//   phase 2  jammer waves: deception false-target Pd + Monte-Carlo hit      -> LDS (1 - min(pd_f, .999999))
//            radar waves (concurrently): suppression sum in jammer order, SNR, Pd, detection draw, FSM,
//            r_d / r_j(suppression) terms; pd / snr / track outputs           -> LDS (r_d, r_j terms)
//   phase 3  radar waves: per-radar deception product in jammer order        -> LDS
//   phase 4  wave 0: the three ordered sums (radar / jammer index order, as the reference), outputs.
// The arithmetic, operation order and RNG slots are identical to env_step_kernel (and the reference);
// only the placement on lanes changes: the per-env critical path is two Pd evaluations instead of J + R,
// there is no per-lane J x R select chain and no divergent deception branch inside a radar/jammer lane.
// Tables indexed by the lane's chosen target radar (<= 128-B rows of a <= 11.5 KB table shared by the whole
// grid) are gathered straight from L1/L2; radar-wave constants are wave-uniform scalar loads.
template <int J, int R, int NJW, int NRW>
__global__ void __launch_bounds__(64 * (NJW + NRW)) env_step_slots_kernel(const DevTables* __restrict__ tb,
                                                                          const macjd_step_io io) {
    constexpr int JPW = (J + NJW - 1) / NJW;
    constexpr int RPW = (R + NRW - 1) / NRW;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t e_raw = (int64_t)blockIdx.x * 64 + lane;
    const bool active = e_raw < io.n_envs;
    const int64_t e = active ? e_raw : io.n_envs - 1;  // clamp: inactive lanes compute on a valid env, store nothing

    __shared__ double s_prj[J][64];
    __shared__ double s_rpterm[J][64];
    __shared__ double s_hitfac[J][64];
    __shared__ int s_meta[J][64];  // bits 0..7 target radar, bit 8 valid suppression, bit 9 valid deception
    __shared__ double s_rd[R][64], s_rjs[R][64], s_rjd[R][64];

    const PdConsts pdk = pd_consts(tb->pd_A, tb->pd_c1, tb->pd_denB);
    const bool arith32 = (io.P32 != nullptr) && !(io.flags & MACJD_STEP_ARITH_F64);
    const int32_t step_before = io.step[e];
    const uint32_t episode = io.episode ? (uint32_t)io.episode[e] : 0u;
    const bool jam_wave = wave < NJW;
    // deception slots R .. R+J-1: when they all live in ONE Philox block (3j/4r: slots 4..6 of block 1) the jammer
    // waves generate it in phase 1, off the post-barrier path; otherwise a block per deceiving lane in phase 2
    constexpr bool DEC_ONE_BLOCK = (R >> 2) == ((R + J - 1) >> 2);
    Philox4 dec_blk;
    if (DEC_ONE_BLOCK && jam_wave && !io.u)
        dec_blk = env_philox_block(io.seed, (uint64_t)(io.env_offset + e), episode, (uint32_t)step_before, (uint32_t)(R >> 2));

    // ---------------- phase 1: jammer lanes, environment.py:248-302 ----------------
    double my_prj[JPW];
    int my_meta[JPW];
    double u_radar[RPW];   // radar waves are idle in phase 1: they draw their detection uniforms now (the draws
                           // depend only on (env, step, slot), not on the actions), off the post-barrier path
    if (!jam_wave) {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = (wave - NJW) + rr * NRW;
            u_radar[rr] = (r < R) ? draw_uniform(io, e, episode, r, (uint32_t)step_before) : 2.0;
        }
    }
    if (jam_wave) {
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int j = wave + jj * NJW;  // wave-uniform
            my_prj[jj] = 0.0;
            my_meta[jj] = 0;
            if (j < J) {
                const int32_t T = io.T[e * io.T_se + (int64_t)j * io.T_sx];
                const bool is_jamming = (T >= 1) && (T <= 2 * R);
                const int target = is_jamming ? ((T + 1) / 2 - 1) : 0;
                const int jtype = T % 2;
                const double pmin = tb->pmin[j], pmax = tb->pmax[j];
                const double power_range = pmax - pmin;
                double actual_d, norm;
                float actual_f = 0.0f;
                if (arith32) {
                    float Pc = io.P32[e * io.P_se + (int64_t)j * io.P_sx];
                    Pc = Pc < 0.0f ? 0.0f : (Pc > 1.0f ? 1.0f : Pc);
                    actual_f = (float)pmin + Pc * (float)power_range;
                    actual_d = (double)actual_f;
                    norm = (power_range > 1e-6) ? (double)((actual_f - (float)pmin) / (float)power_range) : 0.0;
                } else {
                    double Pc = io.P64 ? io.P64[e * io.P_se + (int64_t)j * io.P_sx]
                                       : (double)io.P32[e * io.P_se + (int64_t)j * io.P_sx];
                    Pc = Pc < 0.0 ? 0.0 : (Pc > 1.0 ? 1.0 : Pc);
                    actual_d = pmin + Pc * power_range;
                    norm = (power_range > 1e-6) ? (actual_d - pmin) / power_range : 0.0;
                }
                const double denom = tb->denom[j * R + target];
                const bool recorded = is_jamming && (actual_d > 0.0) && (denom >= 0.0);
                double prj = 0.0;
                if (recorded && denom > 1e-18) {
                    const double grj = tb->gr[target];
                    if (arith32) {
                        const float num = (actual_f * (float)tb->gj[j]) * (float)grj;
                        prj = (tb->flags[j * R + target] & MACJD_JR_WEAK_DENOM) ? (double)(num / (float)denom)
                                                                               : (double)num / denom;
                    } else {
                        prj = (actual_d * tb->gj[j] * grj) / denom;
                    }
                    prj = (prj > 0.0) ? prj : 0.0;
                }
                const int meta = target | ((recorded && jtype == 1) ? 0x100 : 0) | ((recorded && jtype == 0) ? 0x200 : 0);
                my_prj[jj] = prj;
                my_meta[jj] = meta;
                s_prj[j][lane] = prj;
                s_meta[j][lane] = meta;
                s_rpterm[j][lane] = tb->rp_max + (tb->rp_min - tb->rp_max) * norm;  // environment.py:377
                if (io.prj64 && active) io.prj64[e * J + j] = recorded ? prj : -1.0;
            }
        }
    }
    __syncthreads();

    // ---------------- phase 2 ----------------
    if (jam_wave) {
        // deception: false-target detection, environment.py:410-434
#pragma unroll
        for (int jj = 0; jj < JPW; ++jj) {
            const int j = wave + jj * NJW;
            if (j < J) {
                double hitfac = -1.0;
                if (my_meta[jj] & 0x200) {
                    int k = 0;  // valid deception actions of lower-numbered jammers -> RNG slot R + k
                    for (int j2 = 0; j2 < j; ++j2) k += (s_meta[j2][lane] >> 9) & 1;
                    const int target = my_meta[jj] & 0xff;
                    const double Pn_t = tb->Pn[target];
                    double snr_f = (Pn_t > 1e-18) ? (tb->D[target] * my_prj[jj]) / Pn_t : 0.0;
                    snr_f = (snr_f > 0.0) ? snr_f : 0.0;
                    const double pd_f = det_prob(snr_f, pdk);
                    const double u = (DEC_ONE_BLOCK && !io.u) ? u32_mid(philox_word(dec_blk, (R + k) & 3))
                                                              : draw_uniform(io, e, episode, R + k, (uint32_t)step_before);
                    if (u <= pd_f) hitfac = 1.0 - (pd_f < 0.999999 ? pd_f : 0.999999);
                }
                s_hitfac[j][lane] = hitfac;
            }
        }
    } else {
        // radars: detections, FSM, r_d, r_j(suppression); environment.py:316-398
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = (wave - NJW) + rr * NRW;  // wave-uniform
            if (r < R) {
                double supp = 0.0;
                bool targeted = false;
#pragma unroll
                for (int j = 0; j < J; ++j) {  // jammer order, environment.py:299
                    const int meta = s_meta[j][lane];
                    const bool hit = (meta & 0x100) && ((meta & 0xff) == r);
                    supp += hit ? s_prj[j][lane] : 0.0;
                    targeted |= hit;
                }
                const double Pn = tb->Pn[r];
                const double den = tb->D[r] * supp + Pn;
                const double snr_with = (den > 1e-18) ? tb->GaPs[r] / den : 0.0;
                const double pd = det_prob(snr_with, pdk);
                const bool tracking = (u_radar[rr] <= pd);  // next FSM state == detected (radar.py:102-117)
                const double red = tb->pd_no[r] - pd;
                s_rd[r][lane] = tracking ? tb->rd_pen[r] : 0.0;
                s_rjs[r][lane] = (targeted && red > 0.0) ? red : 0.0;
                if (active) {
                    const double snr_rep = (snr_with > 0.0) ? snr_with : 0.0;
                    io.track[e * io.k_se + (int64_t)r * io.k_sx] = tracking ? 1 : 0;
                    if (io.pd) io.pd[e * io.pd_se + (int64_t)r * io.pd_sx] = (float)pd;
                    if (io.snr_with) io.snr_with[e * io.sw_se + (int64_t)r * io.sw_sx] = (float)snr_rep;
                    if (io.pd64) io.pd64[e * R + r] = pd;
                    if (io.snr64) io.snr64[e * R + r] = snr_rep;
                }
            }
        }
    }
    __syncthreads();

    // ---------------- phase 3: per-radar deception product, environment.py:437-451 ----------------
    if (!jam_wave) {
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int r = (wave - NJW) + rr * NRW;
            if (r < R) {
                double prod = 1.0;
                bool any = false;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int meta = s_meta[j][lane];
                    const double hf = s_hitfac[j][lane];
                    const bool hit = (meta & 0x200) && ((meta & 0xff) == r) && (hf >= 0.0);
                    prod = hit ? prod * hf : prod;
                    any |= hit;
                }
                s_rjd[r][lane] = any ? (1.0 - prod) : 0.0;
            }
        }
    }
    __syncthreads();

    // ---------------- phase 4: ordered sums + per-env outputs, environment.py:353-460 ----------------
    if (wave == 0 && active) {
        double r_d = 0.0, r_p = 0.0, r_j = 0.0, r_j_dec = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) { r_d += s_rd[r][lane]; r_j += s_rjs[r][lane]; r_j_dec += s_rjd[r][lane]; }
#pragma unroll
        for (int j = 0; j < J; ++j) r_p += s_rpterm[j][lane];
        r_j += r_j_dec;
        const double reward = r_d + r_p + r_j;
        const int32_t step_count = step_before + 1;
        io.step[e] = step_count;
        if (io.terminated) io.terminated[e] = (step_count >= tb->episode_limit) ? 1 : 0;
        if (io.reward) io.reward[e] = (float)reward;
        if (io.r_dpj) {
            io.r_dpj[e * 3 + 0] = (float)r_d;
            io.r_dpj[e * 3 + 1] = (float)r_p;
            io.r_dpj[e * 3 + 2] = (float)r_j;
        }
        if (io.r_dpj_sum) {
            io.r_dpj_sum[e * 3 + 0] += (float)r_d;
            io.r_dpj_sum[e * 3 + 1] += (float)r_p;
            io.r_dpj_sum[e * 3 + 2] += (float)r_j;
        }
        if (io.out64) {
            io.out64[e * 4 + 0] = reward;
            io.out64[e * 4 + 1] = r_d;
            io.out64[e * 4 + 2] = r_p;
            io.out64[e * 4 + 3] = r_j;
        }
    }
}

__global__ void env_reset_kernel(int64_t n_envs, int R, uint8_t* track, int64_t k_se, int64_t k_sx, int32_t* step,
                                 const uint8_t* mask, int32_t* episode) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_envs;
         e += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[e]) continue;
        for (int r = 0; r < R; ++r) track[e * k_se + (int64_t)r * k_sx] = 0;  // radar.py:10 initial_state SEARCH
        step[e] = 0;                                                         // environment.py:203
        if (episode) episode[e] += 1;   // a new episode draws fresh Monte-Carlo values (environment.py:341,430)
    }
}

// beam part of a reset (macjd_env_reset_scan): azimuths back to az0, state columns to (float)az0
__global__ void env_reset_scan_kernel(const DevTables* __restrict__ tb, int64_t n_envs, int R, double* theta_a, int64_t a_se,
                                      int64_t a_sx, float* state, int64_t st_se, int32_t st_col0, int32_t st_col_step,
                                      const uint8_t* mask) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_envs;
         e += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[e]) continue;
        for (int r = 0; r < R; ++r) {
            const double a0 = tb->az0[r];
            theta_a[e * a_se + (int64_t)r * a_sx] = a0;
            if (state) state[e * st_se + st_col0 + (int64_t)r * st_col_step] = (float)a0;
        }
    }
}

// the same with az0 from each env's column of the per-env scan SoA (include/macjd.h, macjd_scan_pe_io)
__global__ void env_reset_scan_pe_kernel(int64_t n_envs, int R, int J, const double* __restrict__ sp_tables, int64_t sp_stride,
                                         int32_t pe_tile, double* theta_a, int64_t a_se, int64_t a_sx, float* state,
                                         int64_t st_se, int32_t st_col0, int32_t st_col_step, const uint8_t* mask) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_envs;
         e += (int64_t)gridDim.x * blockDim.x) {
        if (mask && !mask[e]) continue;
        const int64_t sps = pe_tile > 0 ? (int64_t)pe_tile : sp_stride;
        const int64_t tile = pe_tile > 0 ? e / pe_tile : 0;
        const double* sp = sp_tables + tile * (10 * R + J * R) * sps + (pe_tile > 0 ? e - tile * pe_tile : e);
        for (int r = 0; r < R; ++r) {
            const double a0 = sp[(int64_t)(3 * R + r) * sps];   // row block az0
            theta_a[e * a_se + (int64_t)r * a_sx] = a0;
            if (state) state[e * st_se + st_col0 + (int64_t)r * st_col_step] = (float)a0;
        }
    }
}

// second half of macjd_env_step_many: the step counters advance by T, the per-episode reward-component sums get the T
// steps' (r_d, r_p, r_j) added in step order (deterministic).  One thread per (env, component): for a given step the
// 3 E values are contiguous, so every load of a wave is one coalesced row piece (one thread per env walking its three
// columns through [T, E, 3] was 31 us at E = 4096, T = 100), eight steps' loads in flight.
__global__ void env_advance_kernel(int64_t n_envs, int32_t T, int32_t* step, const float* r_dpj, float* r_dpj_sum) {
    const int64_t n3 = n_envs * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n_envs) step[i] += T;
        if (r_dpj && r_dpj_sum) {
            float a = r_dpj_sum[i];
            int t = 0;
            for (; t + 8 <= T; t += 8) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = r_dpj[(int64_t)(t + k) * n3 + i];
#pragma unroll
                for (int k = 0; k < 8; ++k) a += v[k];
            }
            for (; t < T; ++t) a += r_dpj[(int64_t)t * n3 + i];
            r_dpj_sum[i] = a;
        }
    }
}

// One launch when a scenario is created: the derived tables of DevTables, computed with the device functions the step
// kernels use (a host-computed reciprocal could differ from rcp_refined's in the last bit).
__global__ void scenario_derive_kernel(DevTables* t) {
    const int J = t->J, R = t->R;
    for (int i = threadIdx.x; i < J * R; i += blockDim.x) {
        const double denom = t->denom[i];
        const uint8_t fl = t->flags[i];
        const bool live = denom > 1e-18;
        const double d = live ? ((fl & MACJD_JR_WEAK_DENOM) ? (double)(float)denom : denom) : 1.0;
        t->dsel[i] = d;
        t->rsel[i] = rcp_refined(d);
        t->rflags[i] = (uint8_t)(fl | (denom >= 0.0 ? JR_RECORDABLE : 0) | (live ? JR_LIVE : 0));
    }
    for (int r = threadIdx.x; r < R; r += blockDim.x) t->rPn[r] = rcp_refined(t->Pn[r] > 1e-18 ? t->Pn[r] : 1.0);
    for (int j = threadIdx.x; j < J; j += blockDim.x) {
        const double rf = (double)(float)(t->pmax[j] - t->pmin[j]);
        t->range_fd[j] = rf;
        t->r_range[j] = rcp_refined(rf > 0.0 ? rf : 1.0);
    }
}

}  // namespace macjd

using macjd::CompiledDim;
using macjd::DevTables;
using macjd::LanePlan;
using macjd::lane_plan;
using macjd::set_err;

// ---- host side of the env_step_kernel launches: each rule once (templates: outside the extern "C" block) ----

// Geometry of a lane-kernel launch: macjd::lane_plan (macjd_env_plan.h); the production variants run on its full grid
static dim3 full_grid(const LanePlan& p) { return dim3((unsigned)p.full_x, (unsigned)p.full_y); }

// Grid of the reset / counter-advance kernels (256 lanes per workgroup, grid-stride loop over n items)
static dim3 strided_grid_256(int64_t n) {
    const int64_t grid = (n + 255) / 256;
    return dim3((unsigned)(grid > 4096 ? 4096 : grid));
}

// set_err with the entry point's name and a second word (the wordings of two entry points that share a check)
static int set_err2(int code, const char* fmt, const char* who, const char* word) {
    char msg[384];
    snprintf(msg, sizeof(msg), fmt, who, word);
    return set_err(code, "%s", msg);
}

// Every byte offset of a strided per-env array ([n_envs] x items elements of `elem` bytes, + extra elements) below 2^32
static bool span_ok(int64_t n_envs, int64_t se, int64_t sx, int items, int64_t elem, int64_t extra = 0) {
    return se >= 0 && sx >= 0 && extra >= 0 && ((n_envs - 1) * se + (int64_t)(items - 1) * sx + extra + 1) * elem < (int64_t)1 << 32;
}

// Production configuration (FAST): Philox uniforms, float32 actions / power arithmetic, no float64 diagnostics, strides
// that fit int32 and every byte offset of the launch below 2^32 (the production variants form them in 32 bits).  A SCAN
// launch adds the spans of its own arrays.
static bool production_io(const macjd_step_io* io, int J, int R, int64_t blocks, int32_t many_T, int64_t t_stride) {
    const int64_t En = io->n_envs, E = En * (many_T > 0 ? many_T : 1);
    const int64_t act_extra = many_T > 0 ? (int64_t)(many_T - 1) * t_stride : 0;
    return !io->u && io->P32 && !(io->flags & MACJD_STEP_ARITH_F64) && !io->out64 && !io->pd64 && !io->snr64 && !io->prj64 &&
           blocks <= 0x7fffffff && span_ok(En, io->T_se, io->T_sx, J, 4, act_extra) &&
           span_ok(En, io->P_se, io->P_sx, J, 4, act_extra) && span_ok(En, io->k_se, io->k_sx, R, 1) &&
           (E * 3 + 3) * 4 < ((int64_t)1 << 32) && t_stride <= INT32_MAX && (!io->pd || span_ok(En, io->pd_se, io->pd_sx, R, 4)) &&
           (!io->snr_with || span_ok(En, io->sw_se, io->sw_sx, R, 4));
}

// The production variants' argument block from the caller's (per-env tables: launch_step adds them)
static void fill_fast(macjd::FastStepIO& f, const macjd_step_io* io, int32_t many_T, int64_t t_stride) {
    f.n_envs = io->n_envs; f.env_offset = io->env_offset; f.seed = io->seed;   // (n_envs: real envs, not work items)
    f.T = io->T; f.P32 = io->P32; f.episode = io->episode; f.track = io->track; f.step = io->step;
    f.reward = io->reward; f.r_dpj = io->r_dpj; f.terminated = io->terminated; f.pd = io->pd;
    f.snr_with = io->snr_with; f.r_dpj_sum = io->r_dpj_sum;
    f.T_se = (int32_t)io->T_se; f.T_sx = (int32_t)io->T_sx; f.P_se = (int32_t)io->P_se; f.P_sx = (int32_t)io->P_sx;
    f.k_se = (int32_t)io->k_se; f.k_sx = (int32_t)io->k_sx; f.pd_se = (int32_t)io->pd_se; f.pd_sx = (int32_t)io->pd_sx;
    f.sw_se = (int32_t)io->sw_se; f.sw_sx = (int32_t)io->sw_sx;
    f.many_T = many_T; f.t_stride = (int32_t)t_stride;
}

// A SCAN launch's own arrays: their spans for the production variants, and their members of the argument block
static bool scan_spans_ok(const macjd_scan_io* sc, int64_t E, int R) {
    const bool st_ok = !sc->state || (sc->st_col0 >= 0 && sc->st_col_step >= 0 &&
                                      span_ok(E, sc->st_se, 1, 1, 4, (int64_t)sc->st_col0 + (int64_t)(R - 1) * sc->st_col_step));
    return span_ok(E, sc->a_se, sc->a_sx, R, 8) && st_ok && (!sc->snr_no || span_ok(E, sc->sn_se, sc->sn_sx, R, 4));
}
template <class X>
static void fill_scan(X& x, const macjd_scan_io* sc) {
    x.theta_a = sc->theta_a; x.a_se = sc->a_se; x.a_sx = sc->a_sx;
    x.state = sc->state; x.st_se = sc->st_se; x.st_col0 = sc->st_col0; x.st_col_step = sc->st_col_step;
    x.snr_no = sc->snr_no; x.sn_se = sc->sn_se; x.sn_sx = sc->sn_sx;
}

// What a MOVING launch reads beyond the step's own block, in one shape for the four table modes: the motion block as its
// shared-frame form (a per-env block is converted once, motion_pe_as_motion) with the env tile (0: shared frames), and under
// scanning radars the beam block and the per-frame scan / pattern tables (a per-env block converted likewise)
struct MovingArgs {
    macjd_motion_io mo;
    int32_t tile;
    const macjd_scan_io* sc;
    macjd_motion_scan_io ms;
};

// ... and a MOVING launch's members of the argument block (include/macjd.h, macjd_motion_io, macjd_motion_scan_io).  The
// scanning blocks name the state rows mv_state (`state` is the beam block's) and have no snr_no output of their own.
template <bool SCAN, bool PAT, class X>
static void fill_moving(X& x, const MovingArgs& a) {
    const macjd_motion_io& mo = a.mo;
    x.frames = mo.frames; x.frame_flags = mo.frame_flags;
    x.positions = mo.positions; x.position_columns = mo.position_columns;
    x.mv_st_se = mo.st_se; x.n_frames = mo.n_frames; x.n_pos = mo.n_pos;
    if constexpr (SCAN) {
        fill_scan(x, a.sc);
        x.sp_tables = a.ms.scan_frames; x.sp_stride = 0;   // frame-major: the strides are not read
        x.mv_state = mo.state;
        if constexpr (PAT) { x.pp_tables = a.ms.pattern_frames; x.pp_stride = 0; x.pat_levels = a.ms.n_levels; }
    } else {
        x.frame_snr_no = mo.frame_snr_no; x.state = mo.state;
        x.mv_snr_no = mo.snr_no; x.mv_sn_se = mo.sn_se; x.mv_sn_sx = mo.sn_sx;
    }
    if constexpr (macjd::io_moves_pe<X>::value) x.mv_tile = a.tile;
}

template <int JT, int RT, bool PE, bool FAST, bool REG = false, bool PD32 = false, bool SCAN = false, bool PAT = false, class IO>
static void launch_lanes(dim3 grid, dim3 block, hipStream_t stream, const macjd_scenario* s, const IO& io) {
    hipLaunchKernelGGL((macjd::env_step_kernel<JT, RT, PE, FAST, IO, REG, PD32, SCAN, PAT>), grid, block, 0, stream, s->dev, io);
}

// The compiled (J, R) sizes of env_step_kernel; every other size runs the generic <0, 0> kernel.  fn(JT, RT) takes the
// size as two std::integral_constants (CompiledDim, macjd_env_step.h) and picks the variant.
template <class F>
static int with_compiled_size(int J, int R, F&& fn) {
    if (J == 3 && R == 4) return fn(CompiledDim<3>{}, CompiledDim<4>{});
    if (J == 6 && R == 8) return fn(CompiledDim<6>{}, CompiledDim<8>{});
    if (J == 12 && R == 16) return fn(CompiledDim<12>{}, CompiledDim<16>{});
    if (J == 2 && R == 2) return fn(CompiledDim<2>{}, CompiledDim<2>{});
    return fn(CompiledDim<0>{}, CompiledDim<0>{});
}

// Compiled (J, R) sizes that have per-env SCAN variants of env_step_kernel; the others run its generic-size kernel
constexpr bool scan_pe_compiled(int JT) { return JT != 0 && JT != 12; }

// Error check after a launch of entry point `who`
static int launch_status(const char* who) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return MACJD_OK;
    char msg[256];
    snprintf(msg, sizeof(msg), "%s launch: %s", who, hipGetErrorString(err));
    return set_err(MACJD_EDEVICE, "%s", msg);
}

// Argument block of a SCAN launch on per-env tables, with or without the pattern's rows
template <bool PAT, class Base>
using ScanPeIO = std::conditional_t<PAT, macjd::ScanPePatStepIO<Base>, macjd::ScanPeStepIO<Base>>;

// SCAN launches on per-env scenario tables, with (PAT) or without a stepped antenna pattern: the lane kernel, single step
// (include/macjd.h, macjd_env_step_scan_pe, macjd_env_step_scan_pe_pattern).  The production variant or the general one at
// the sizes scan_pe_compiled covers, the generic-size kernel for the others.  `pp` is NULL without a pattern.
template <bool PAT>
static int launch_step_scan_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* sc, const macjd_scan_pe_io* sp,
                               const macjd_scan_pe_pattern_io* pp, hipStream_t stream, const char* who) {
    const int64_t E = io->n_envs;
    const int J = s->host.J, R = s->host.R;
    const LanePlan lp = lane_plan(E, 0);
    const dim3 gf = full_grid(lp), g(lp.strided), b(lp.block);
    const bool fast = production_io(io, J, R, lp.blocks, 0, 0) && scan_spans_ok(sc, E, R);
    const auto fill_tables = [&](auto& x) {
        fill_scan(x, sc);
        x.sp_tables = sp->tables; x.sp_stride = sp->stride;
        if constexpr (PAT) { x.pp_tables = pp->tables; x.pp_stride = pp->stride; x.pat_levels = pp->n_levels; }
    };
    ScanPeIO<PAT, macjd::FastStepIO> f{};
    ScanPeIO<PAT, macjd_step_io> w{};
    static_cast<macjd_step_io&>(w) = *io;
    fill_tables(w);
    if (fast) {
        fill_fast(f, io, 0, 0);
        f.pe_tables = io->pe_tables; f.pe_flags = io->pe_flags; f.pe_stride = io->pe_stride; f.pe_tile = io->pe_tile;
        fill_tables(f);
    }
    // launch_lanes<JT, RT, PE = true, FAST, REG = false, PD32 = false, SCAN = true, PAT>
    with_compiled_size(J, R, [&](auto jt, auto rt) -> int {
        constexpr int JT = decltype(jt)::value, RT = decltype(rt)::value;
        if constexpr (!scan_pe_compiled(JT)) macjd::launch_scan_pe_generic(g, b, stream, s->dev, w);
        else if (fast) launch_lanes<JT, RT, true, true, false, false, true, PAT>(gf, b, stream, s, f);
        else launch_lanes<JT, RT, true, false, false, false, true, PAT>(g, b, stream, s, w);
        return MACJD_OK;
    });
    return launch_status(who);
}

// ---- moving scenarios: ONE dispatch path for the four table modes ("Moving env launches") ----

// The production form's 32-bit offsets into the motion arrays: every state element of a row (the position columns lie below
// the row stride; the caller's tables say which), the snr_no output
static bool motion_spans_ok(const macjd_motion_io* mo, int64_t E, int R) {
    return span_ok(E, mo->st_se, 1, 1, 4, mo->st_se - 1) && (!mo->snr_no || span_ok(E, mo->sn_se, mo->sn_sx, R, 4));
}

// Argument block of a MOVING launch: (per-env frames, scanning radars, stepped pattern, production or general base)
template <bool MVPE, bool SCAN, bool PAT, class Base>
using MovingIO = std::conditional_t<
    SCAN, std::conditional_t<MVPE, macjd::MotionScanPeStepIO<ScanPeIO<PAT, Base>>, macjd::MotionScanStepIO<ScanPeIO<PAT, Base>>>,
    std::conditional_t<MVPE, macjd::MotionPeStepIO<Base>, macjd::MotionStepIO<Base>>>;

// MOVING launches: always the lane kernel on the frame tables (include/macjd.h, macjd_env_step_moving and its _pe, _scan,
// _scan_pe and many-step forms).  The production variant at a compiled moving size in the production configuration whose
// 32-bit offsets fit; otherwise the general variant (the generic-size kernel at the other sizes), single steps only.
template <bool MVPE, bool SCAN, bool PAT>
static int launch_step_moving(const macjd_scenario* s, const macjd_step_io* io, const MovingArgs& a, hipStream_t stream,
                              int32_t many_T, int64_t t_stride, const char* who) {
    const int64_t E = io->n_envs;
    const int J = s->host.J, R = s->host.R;
    if (many_T > 65535) return set_err(MACJD_EINVAL, "%s: at most 65535 steps per launch", who);
    const LanePlan lp = lane_plan(E, many_T);
    bool fast = macjd::motion_size_compiled(J, R) && production_io(io, J, R, lp.blocks, many_T, t_stride) &&
                motion_spans_ok(&a.mo, E, R);
    if constexpr (SCAN) fast = fast && scan_spans_ok(a.sc, E, R);
    if constexpr (MVPE) fast = fast && E < ((int64_t)1 << 31);   // the env index and its tile arithmetic in 32 bits
    if (fast) {
        MovingIO<MVPE, SCAN, PAT, macjd::FastStepIO> f{};
        fill_fast(f, io, many_T, t_stride);
        fill_moving<SCAN, PAT>(f, a);
        (void)macjd::launch_motion(J, R, full_grid(lp), dim3(lp.block), stream, s->dev, f);
    } else {
        if (many_T > 0)
            return set_err(MACJD_EUNSUPPORTED, "%s: production configuration at a compiled size (2j/2r, 3j/4r, 6j/8r) only: Philox "
                           "uniforms, float32 actions, no float64 diagnostics, offsets below 2^32 bytes", who);
        MovingIO<MVPE, SCAN, PAT, macjd_step_io> w{};
        static_cast<macjd_step_io&>(w) = *io;
        fill_moving<SCAN, PAT>(w, a);
        (void)macjd::launch_motion(J, R, dim3(lp.strided), dim3(lp.block), stream, s->dev, w);
    }
    return launch_status(who);
}

extern "C" {

int macjd_abi_version(void) { return MACJD_ABI_VERSION; }
const char* macjd_last_error(void) { return macjd::g_err; }

void macjd_reload_options(void) { macjd::load_env_options(); }

int macjd_device_count(void) {
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(err));
    return n;
}

// REGULAR range of a table value (see macjd_scenario_create); a gain may also be zero
static bool reg_mag(double v) { return v >= 1e-30 && v <= 1e30; }
static bool reg_gain(double v) { return v == 0.0 || reg_mag(v); }

int macjd_scenario_create(const macjd_scenario_desc* d, macjd_scenario** out) {
    if (!d || !out) return set_err(MACJD_EINVAL, "macjd_scenario_create: NULL argument");
    const int R = d->n_radars, J = d->n_jammers;
    if (R < 1 || R > MACJD_MAX_RADARS || J < 1 || J > MACJD_MAX_JAMMERS)
        return set_err(MACJD_EINVAL, "macjd_scenario_create: n_radars / n_jammers out of range");
    if (!d->radar_GaPs || !d->radar_Pn || !d->radar_D || !d->radar_pd_no || !d->radar_rd_pen || !d->radar_gr ||
        !d->jam_pmin || !d->jam_pmax || !d->jam_gj || !d->jr_denom || !d->jr_flags)
        return set_err(MACJD_EINVAL, "macjd_scenario_create: NULL table pointer");
    macjd_scenario* s = new (std::nothrow) macjd_scenario();
    if (!s) return set_err(MACJD_ENOMEM, "macjd_scenario_create: host allocation failed");
    DevTables& t = s->host;
    memset(&t, 0, sizeof(t));
    t.R = R; t.J = J; t.episode_limit = d->episode_limit;
    t.rp_min = d->rp_min; t.rp_max = d->rp_max;
    t.pd_A = d->pd_A; t.pd_c1 = d->pd_c1; t.pd_denB = d->pd_denB;
    for (int r = 0; r < R; ++r) {
        t.GaPs[r] = d->radar_GaPs[r]; t.Pn[r] = d->radar_Pn[r]; t.D[r] = d->radar_D[r];
        t.pd_no[r] = d->radar_pd_no[r]; t.rd_pen[r] = d->radar_rd_pen[r]; t.gr[r] = d->radar_gr[r];
    }
    for (int j = 0; j < J; ++j) {
        t.pmin[j] = d->jam_pmin[j]; t.pmax[j] = d->jam_pmax[j]; t.gj[j] = d->jam_gj[j];
    }
    for (int i = 0; i < J * R; ++i) { t.denom[i] = d->jr_denom[i]; t.flags[i] = d->jr_flags[i]; }
    // REGULAR scenario (env_step_kernel, REG): every quantity a division of the step can meet lies far inside the range
    // where the hardware's IEEE division needs neither operand scaling nor special cases (magnitudes in [1e-30, 1e30]
    // give quotients and residuals within 1e-220 .. 1e100), the float32 numerator cannot overflow, the noise power is
    // positive (SNR denominators >= Pn > 1e-18, SNRs >= +0), and the probability formula's argument stays above -700.
    {
        bool ok = t.pd_denB >= 1e-9 && t.pd_denB <= 1e30 && fabs(t.pd_A) <= 1e30 && fabs(t.pd_c1) <= 1e30 &&
                  (10.0 * t.pd_c1 - t.pd_A) / t.pd_denB >= -700.0;
        double gr_max = 0.0, pg_max = 0.0;
        for (int r = 0; r < R && ok; ++r) {
            ok = reg_mag(t.GaPs[r]) && t.Pn[r] > 1e-18 && t.Pn[r] <= 1e30 && reg_gain(t.D[r]) && reg_gain(t.gr[r]);
            gr_max = t.gr[r] > gr_max ? t.gr[r] : gr_max;
        }
        for (int j = 0; j < J && ok; ++j) {
            const double range = t.pmax[j] - t.pmin[j], pm = fabs(t.pmin[j]) > fabs(t.pmax[j]) ? fabs(t.pmin[j]) : fabs(t.pmax[j]);
            ok = pm <= 1e30 && reg_gain(t.gj[j]) && (range <= 1e-6 || reg_mag(range));
            pg_max = pm * t.gj[j] > pg_max ? pm * t.gj[j] : pg_max;
        }
        for (int i = 0; i < J * R && ok; ++i) ok = !(t.denom[i] > 1e-18) || t.denom[i] <= 1e30;
        t.regular = (ok && pg_max * gr_max < 1e30) ? 1 : 0;
    }
    hipError_t err = hipGetDevice(&s->device);
    if (err == hipSuccess) err = hipMalloc((void**)&s->dev, sizeof(DevTables));
    if (err == hipSuccess) err = hipMemcpy(s->dev, &t, sizeof(DevTables), hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(macjd::scenario_derive_kernel, dim3(1), dim3(256), 0, (hipStream_t)0, s->dev);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    if (err != hipSuccess) {
        if (s->dev) (void)hipFree(s->dev);
        delete s;
        return set_err(MACJD_EDEVICE, "macjd_scenario_create: %s", hipGetErrorString(err));
    }
    *out = s;
    return MACJD_OK;
}

void macjd_scenario_destroy(macjd_scenario* s) {
    if (!s) return;
    if (s->dev) (void)hipFree(s->dev);
    delete s;
}

int macjd_scenario_dims(const macjd_scenario* s, int32_t* n_radars, int32_t* n_jammers, int32_t* episode_limit) {
    if (!s) return set_err(MACJD_EINVAL, "macjd_scenario_dims: NULL scenario");
    if (n_radars) *n_radars = s->host.R;
    if (n_jammers) *n_jammers = s->host.J;
    if (episode_limit) *episode_limit = s->host.episode_limit;
    return MACJD_OK;
}

int macjd_scenario_is_regular(const macjd_scenario* s) {
    if (!s) return set_err(MACJD_EINVAL, "macjd_scenario_is_regular: NULL scenario");
    return s->host.regular;
}

int macjd_env_reset(const macjd_scenario* s, int64_t n_envs, uint8_t* track, int64_t k_se, int64_t k_sx,
                    int32_t* step, const uint8_t* mask, int32_t* episode, void* hip_stream) {
    if (!s || !track || !step || n_envs < 0) return set_err(MACJD_EINVAL, "macjd_env_reset: bad argument");
    if (n_envs == 0) return MACJD_OK;
    hipLaunchKernelGGL(macjd::env_reset_kernel, strided_grid_256(n_envs), dim3(256), 0, (hipStream_t)hip_stream, n_envs,
                       s->host.R, track, k_se, k_sx, step, mask, episode);
    return launch_status("macjd_env_reset");
}

static int validate_io(const macjd_scenario* s, const macjd_step_io* io) {
    if (!s || !io) return set_err(MACJD_EINVAL, "macjd_env_step: NULL scenario / io");
    if (io->n_envs < 0) return set_err(MACJD_EINVAL, "macjd_env_step: n_envs < 0");
    if (!io->T || !io->track || !io->step) return set_err(MACJD_EINVAL, "macjd_env_step: T / track / step is NULL");
    if ((io->P32 == nullptr) == (io->P64 == nullptr))
        return set_err(MACJD_EINVAL, "macjd_env_step: exactly one of P32 / P64 must be given");
    if ((io->pd && (io->pd_se == 0 && io->pd_sx == 0)) || (io->snr_with && (io->sw_se == 0 && io->sw_sx == 0)))
        return set_err(MACJD_EINVAL, "macjd_env_step: output strides are zero");
    if (io->k_se == 0 && io->k_sx == 0) return set_err(MACJD_EINVAL, "macjd_env_step: track strides are zero");
    if (io->pe_tables && (!io->pe_flags || io->pe_tile < 0 || (io->pe_tile == 0 && io->pe_stride < io->n_envs)))
        return set_err(MACJD_EINVAL, "macjd_env_step: per-env tables need pe_flags and pe_stride >= n_envs (or pe_tile > 0)");
    return MACJD_OK;
}

static int launch_step(const macjd_scenario* s, const macjd_step_io* io, hipStream_t stream, int32_t many_T = 0,
                       int64_t t_stride = 0) {
    const int64_t E = io->n_envs * (many_T > 0 ? many_T : 1);   // work items of the launch
    const int J = s->host.J, R = s->host.R;
    const bool has_slot_kernel = (J == 3 && R == 4) || (J == 6 && R == 8) || (J == 12 && R == 16) || (J == 2 && R == 2);
    // measured crossover on MI355X (3j/4r, round 2): slot kernel 3.9 / 4.2 / 7.3 / 21.8 us vs lane kernel 5.6 / 5.7 /
    // 7.5 / 13.5 us at E = 2^12 / 2^14 / 2^16 / 2^18
    bool slot_kernel = has_slot_kernel && E < (1 << 16);
    if (io->flags & MACJD_STEP_LANE_KERNEL) slot_kernel = false;
    if ((io->flags & MACJD_STEP_SLOT_KERNEL) && has_slot_kernel) slot_kernel = true;
    const bool per_env = io->pe_tables != nullptr;
    if (per_env) slot_kernel = false;   // per-env tables: lane-per-env kernel (each lane streams its own SoA column)
    if (many_T > 0) slot_kernel = false;
    if (slot_kernel) {  // one workgroup per 64 envs
        const dim3 g((unsigned)((E + 63) / 64));
#define MACJD_SLOTS(JT, RT, NJW, NRW) \
    hipLaunchKernelGGL((macjd::env_step_slots_kernel<JT, RT, NJW, NRW>), g, dim3(64 * (NJW + NRW)), 0, stream, s->dev, *io)
        if (J == 3) MACJD_SLOTS(3, 4, 3, 4);
        else if (J == 6) MACJD_SLOTS(6, 8, 6, 8);
        else if (J == 12) MACJD_SLOTS(12, 16, 4, 8);
        else MACJD_SLOTS(2, 2, 2, 2);
#undef MACJD_SLOTS
        return launch_status("macjd_env_step");
    }
    // generic sizes (and the A/B hook): one lane per env
    if (many_T > 65535) return set_err(MACJD_EINVAL, "%s", "macjd_env_step_many: at most 65535 steps per launch");
    const LanePlan lp = lane_plan(io->n_envs, many_T);
    const dim3 gf = full_grid(lp), g(lp.strided), b(lp.block);
    const bool fast = production_io(io, J, R, lp.blocks, many_T, t_stride);
    macjd::FastStepIO f{};
    if (fast) {
        fill_fast(f, io, many_T, t_stride);
        f.pe_tables = io->pe_tables; f.pe_flags = io->pe_flags; f.pe_stride = io->pe_stride; f.pe_tile = io->pe_tile;
    } else if (many_T > 0) {
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_env_step_many: production configuration only (Philox uniforms, "
                       "float32 actions, no float64 diagnostics, offsets below 2^32 bytes)");
    }
    const bool reg = s->host.regular && macjd::env_options().regular;   // MACJD_ENV_REGULAR=0: keep IEEE divisions + all guards
    const bool pd32 = macjd::env_options().pd32;                         // MACJD_ENV_PD32=0: all-float64 detection probabilities
    // launch_lanes<JT, RT, PE, FAST, REG, PD32> (SCAN = PAT = false)
    const int rc = with_compiled_size(J, R, [&](auto jt, auto rt) -> int {
        constexpr int JT = decltype(jt)::value, RT = decltype(rt)::value;
        if constexpr (JT == 0) {   // generic sizes: one (non-FAST) variant per table mode
            if (many_T > 0)
                return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_env_step_many: scenario size without a compiled production variant");
            if (per_env) launch_lanes<0, 0, true, false>(g, b, stream, s, *io);
            else launch_lanes<0, 0, false, false>(g, b, stream, s, *io);
        } else if (per_env && fast) launch_lanes<JT, RT, true, true>(gf, b, stream, s, f);
        else if (per_env) launch_lanes<JT, RT, true, false>(g, b, stream, s, *io);
        else if (fast && reg && pd32) launch_lanes<JT, RT, false, true, true, true>(gf, b, stream, s, f);
        else if (fast && reg) launch_lanes<JT, RT, false, true, true>(gf, b, stream, s, f);
        else if (fast) launch_lanes<JT, RT, false, true>(gf, b, stream, s, f);
        else launch_lanes<JT, RT, false, false>(g, b, stream, s, *io);
        return MACJD_OK;
    });
    return rc != MACJD_OK ? rc : launch_status("macjd_env_step");
}

// SCAN launches: always the lane kernel, shared tables, single step (include/macjd.h, macjd_env_step_scan)
static int launch_step_scan(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* sc, hipStream_t stream) {
    const int64_t E = io->n_envs;
    const int J = s->host.J, R = s->host.R;
    const LanePlan lp = lane_plan(E, 0);
    const dim3 gf = full_grid(lp), g(lp.strided), b(lp.block);
    const bool fast = production_io(io, J, R, lp.blocks, 0, 0) && scan_spans_ok(sc, E, R);
    macjd::ScanStepIO<macjd::FastStepIO> f{};
    macjd::ScanStepIO<macjd_step_io> w{};
    static_cast<macjd_step_io&>(w) = *io;
    fill_scan(w, sc);
    if (fast) {
        fill_fast(f, io, 0, 0);
        fill_scan(f, sc);
    }
    const bool reg = s->host.regular && s->host.scan_regular && macjd::env_options().regular;
    const bool pd32 = macjd::env_options().pd32;
    const bool pat = s->host.pat_levels > 0;   // stepped antenna pattern (macjd_scenario_set_scan_pattern)
    // launch_lanes<JT, RT, PE = false, FAST, REG, PD32, SCAN = true, PAT>
    with_compiled_size(J, R, [&](auto jt, auto rt) -> int {
        constexpr int JT = decltype(jt)::value, RT = decltype(rt)::value;
        if constexpr (JT == 0) {   // generic sizes: the general variant
            if (pat) launch_lanes<0, 0, false, false, false, false, true, true>(g, b, stream, s, w);
            else launch_lanes<0, 0, false, false, false, false, true>(g, b, stream, s, w);
        } else if (pat) {
            // the production variant (fast + REG + PD32) or the general all-float64 one, which serves every other switch
            // combination (same integers; rewards within the PD32 bound of each other)
            if (fast && reg && pd32) launch_lanes<JT, RT, false, true, true, true, true, true>(gf, b, stream, s, f);
            // 12j/16r outside the production configuration: its compiled general form needs all 512 registers and 8 more
            // (12 B of scratch per lane); the generic-size kernel computes the same bits without any
            else if constexpr (JT == 12) launch_lanes<0, 0, false, false, false, false, true, true>(g, b, stream, s, w);
            else launch_lanes<JT, RT, false, false, false, false, true, true>(g, b, stream, s, w);
        } else if (fast && reg && pd32) launch_lanes<JT, RT, false, true, true, true, true>(gf, b, stream, s, f);
        else if (fast && reg) launch_lanes<JT, RT, false, true, true, false, true>(gf, b, stream, s, f);
        else if (fast) launch_lanes<JT, RT, false, true, false, false, true>(gf, b, stream, s, f);
        else launch_lanes<JT, RT, false, false, false, false, true>(g, b, stream, s, w);
        return MACJD_OK;
    });
    return launch_status("macjd_env_step_scan");
}

static int validate_scan(const macjd_scenario* s, const macjd_scan_io* sc, const char* what) {
    if (!sc || !sc->theta_a) return set_err(MACJD_EINVAL, "%s: NULL scan io / theta_a", what);
    if (!s->host.scanning) return set_err(MACJD_EINVAL, "%s: the scenario has no scanning tables (macjd_scenario_set_scan)", what);
    if (sc->a_se == 0 && sc->a_sx == 0) return set_err(MACJD_EINVAL, "%s: theta_a strides are zero", what);
    if (sc->state && (sc->st_col0 < 0 || sc->st_col_step < 0)) return set_err(MACJD_EINVAL, "%s: bad state columns", what);
    if (sc->snr_no && sc->sn_se == 0 && sc->sn_sx == 0) return set_err(MACJD_EINVAL, "%s: snr_no strides are zero", what);
    return MACJD_OK;
}

// The scanning tail of the tables (everything from DevTables.scanning on) to the device
static hipError_t upload_scan_tables(macjd_scenario* s) {
    const size_t off = offsetof(DevTables, scanning);
    return hipMemcpy(reinterpret_cast<char*>(s->dev) + off, reinterpret_cast<const char*>(&s->host) + off,
                     sizeof(DevTables) - off, hipMemcpyHostToDevice);
}

int macjd_scenario_set_scan(macjd_scenario* s, const macjd_scan_desc* d) {
    if (!s || !d) return set_err(MACJD_EINVAL, "%s", "macjd_scenario_set_scan: NULL argument");
    DevTables& t = s->host;
    const int R = t.R, J = t.J;
    if (d->n_radars != R || d->n_jammers != J)
        return set_err(MACJD_EINVAL, "%s", "macjd_scenario_set_scan: n_radars / n_jammers differ from the scenario's");
    if (!d->half_beam || !d->sweep || !d->sweep_mod || !d->full || !d->az0 || !d->bear_tgt || !d->bear_jam || !d->GaPs_side ||
        !d->snr_no || !d->snr_no_side || !d->pd_no_side || !d->gr_side)
        return set_err(MACJD_EINVAL, "%s", "macjd_scenario_set_scan: NULL table pointer");
    for (int r = 0; r < R; ++r) {
        t.half[r] = d->half_beam[r]; t.h2[r] = 2.0 * d->half_beam[r]; t.sweep[r] = d->sweep[r]; t.swm[r] = d->sweep_mod[r];
        t.full[r] = d->full[r] ? 1 : 0; t.az0[r] = d->az0[r]; t.bt[r] = d->bear_tgt[r];
        t.GaPs_side[r] = d->GaPs_side[r]; t.snr_no[r] = d->snr_no[r]; t.snr_no_side[r] = d->snr_no_side[r];
        t.pd_no_side[r] = d->pd_no_side[r]; t.gr_side[r] = d->gr_side[r];
    }
    for (int i = 0; i < J * R; ++i) t.bj[i] = d->bear_jam[i];
    // the short-division (REG) variant also needs the side-lobe values inside its range (see macjd_scenario_create)
    // (gr_side <= gr: the float32-numerator bound of the main tables holds)
    bool ok = true;
    for (int r = 0; r < R; ++r)
        ok = ok && reg_mag(t.GaPs_side[r]) && t.gr_side[r] <= t.gr[r] && reg_gain(t.gr_side[r]);
    t.scan_regular = ok ? 1 : 0;
    t.scanning = 1;
    t.pat_levels = 0;   // new scan tables: an earlier pattern's level 0 / L + 1 rows no longer match them
    const hipError_t err = upload_scan_tables(s);
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_scenario_set_scan: %s", hipGetErrorString(err));
    return MACJD_OK;
}

int macjd_scenario_set_scan_pattern(macjd_scenario* s, const macjd_scan_pattern_desc* d) {
    const char* me = "macjd_scenario_set_scan_pattern";
    if (!s || !d) return set_err(MACJD_EINVAL, "%s: NULL argument", me);
    DevTables& t = s->host;
    const int R = t.R, L = d->n_levels;
    if (!t.scanning) return set_err(MACJD_EINVAL, "%s: the scenario has no scanning tables (macjd_scenario_set_scan comes first)", me);
    if (d->n_radars != R) return set_err(MACJD_EINVAL, "%s: n_radars differs from the scenario's", me);
    if (L < 1 || L > MACJD_MAX_PATTERN_LEVELS) return set_err(MACJD_EINVAL, "%s: n_levels outside 1..MACJD_MAX_PATTERN_LEVELS", me);
    if (!d->inv_width || !d->GaPs_lvl || !d->snr_no_lvl || !d->pd_no_lvl || !d->gr_lvl)
        return set_err(MACJD_EINVAL, "%s: NULL table pointer", me);
    for (int r = 0; r < R; ++r)
        if (!(d->inv_width[r] > 0.0 && d->inv_width[r] <= 1e3))   // 1 / (level_width half_beam) with the product >= 1e-3
            return set_err(MACJD_EINVAL, "%s: inv_width must lie in (0, 1e3]", me);
    // rows 0 and L + 1 from the handle's main / side-lobe tables, rows 1..L from the caller
    bool ok = true;
    for (int r = 0; r < R; ++r) {
        t.pat_inv_width[r] = d->inv_width[r];
        t.lv_GaPs[r] = t.GaPs[r]; t.lv_pd_no[r] = t.pd_no[r]; t.lv_snr_no[r] = t.snr_no[r]; t.lv_gr[r] = t.gr[r];
        const int z = (L + 1) * R + r;
        t.lv_GaPs[z] = t.GaPs_side[r]; t.lv_pd_no[z] = t.pd_no_side[r]; t.lv_snr_no[z] = t.snr_no_side[r]; t.lv_gr[z] = t.gr_side[r];
        for (int k = 1; k <= L; ++k) {
            const int i = k * R + r, c = (k - 1) * R + r;
            t.lv_GaPs[i] = d->GaPs_lvl[c]; t.lv_pd_no[i] = d->pd_no_lvl[c]; t.lv_snr_no[i] = d->snr_no_lvl[c]; t.lv_gr[i] = d->gr_lvl[c];
            // the short-division (REG) variant needs every level's values inside its range (see macjd_scenario_set_scan)
            ok = ok && reg_mag(t.lv_GaPs[i]) && t.lv_gr[i] <= t.gr[r] && reg_gain(t.lv_gr[i]);
        }
    }
    t.scan_regular = (t.scan_regular && ok) ? 1 : 0;
    t.pat_levels = L;
    const hipError_t err = upload_scan_tables(s);
    if (err != hipSuccess) {
        t.pat_levels = 0;
        return set_err(MACJD_EDEVICE, "macjd_scenario_set_scan_pattern: %s", hipGetErrorString(err));
    }
    return MACJD_OK;
}

int macjd_env_step_scan(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan, void* hip_stream) {
    int rc = validate_io(s, io);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan(s, scan, "macjd_env_step_scan");
    if (rc != MACJD_OK) return rc;
    if (io->pe_tables)   // per-env scan tables travel in a block of their own: macjd_env_step_scan_pe
        return set_err(MACJD_EUNSUPPORTED, "%s", "macjd_env_step_scan: per-env scenario tables are not supported (macjd_env_step_scan_pe)");
    if (io->n_envs == 0) return MACJD_OK;
    return launch_step_scan(s, io, scan, (hipStream_t)hip_stream);
}

int macjd_env_reset_scan(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan, const uint8_t* mask, void* hip_stream) {
    if (!s || n_envs < 0) return set_err(MACJD_EINVAL, "%s", "macjd_env_reset_scan: bad argument");
    int rc = validate_scan(s, scan, "macjd_env_reset_scan");
    if (rc != MACJD_OK) return rc;
    if (n_envs == 0) return MACJD_OK;
    hipLaunchKernelGGL(macjd::env_reset_scan_kernel, strided_grid_256(n_envs), dim3(256), 0, (hipStream_t)hip_stream, s->dev, n_envs,
                       s->host.R, scan->theta_a, scan->a_se, scan->a_sx, scan->state, scan->st_se, scan->st_col0,
                       scan->st_col_step, mask);
    return launch_status("macjd_env_reset_scan");
}

// `pattern_ok`: the caller brings the pattern's levels per env (macjd_env_step_scan_pe_pattern); the handle's are not read
static int validate_scan_pe(const macjd_scenario* s, const macjd_scan_pe_io* sp, int64_t n_envs, int32_t pe_tile, const char* what,
                            bool pattern_ok = false) {
    if (!sp || !sp->tables) return set_err(MACJD_EINVAL, "%s: NULL per-env scan tables", what);
    if (pe_tile < 0 || (pe_tile == 0 && sp->stride < n_envs))
        return set_err(MACJD_EINVAL, "%s: per-env scan tables need stride >= n_envs (or pe_tile > 0)", what);
    if (s->host.pat_levels > 0 && !pattern_ok)
        return set_err(MACJD_EUNSUPPORTED, "%s: a stepped antenna pattern is not supported with per-env scan tables", what);
    return MACJD_OK;
}

static int validate_scan_pe_pattern(const macjd_scenario* s, const macjd_scan_pe_pattern_io* pp, int64_t n_envs, int32_t pe_tile,
                                    const char* what) {
    if (!pp || !pp->tables) return set_err(MACJD_EINVAL, "%s: NULL per-env pattern tables", what);
    if (pe_tile < 0 || (pe_tile == 0 && pp->stride < n_envs))
        return set_err(MACJD_EINVAL, "%s: per-env pattern tables need stride >= n_envs (or pe_tile > 0)", what);
    if (pp->n_levels < 1 || pp->n_levels > MACJD_MAX_PATTERN_LEVELS)
        return set_err(MACJD_EINVAL, "%s: n_levels outside 1..MACJD_MAX_PATTERN_LEVELS", what);
    if (s->host.pat_levels > 0 && s->host.pat_levels != pp->n_levels)
        return set_err(MACJD_EINVAL, "%s: n_levels differs from the pattern levels of the scenario handle", what);
    return MACJD_OK;
}

int macjd_env_step_scan_pe_pattern(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan,
                                   const macjd_scan_pe_io* scan_pe, const macjd_scan_pe_pattern_io* pattern, void* hip_stream) {
    const char* me = "macjd_env_step_scan_pe_pattern";
    int rc = validate_io(s, io);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan(s, scan, me);
    if (rc != MACJD_OK) return rc;
    if (!io->pe_tables) return set_err(MACJD_EINVAL, "%s: needs per-env scenario tables (io->pe_tables); macjd_env_step_scan takes the handle's", me);
    rc = validate_scan_pe(s, scan_pe, io->n_envs, io->pe_tile, me, true);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan_pe_pattern(s, pattern, io->n_envs, io->pe_tile, me);
    if (rc != MACJD_OK) return rc;
    if (io->flags & MACJD_STEP_SLOT_KERNEL)
        return set_err(MACJD_EUNSUPPORTED, "%s: the (env x slot) kernel has no per-env pattern variant (one lane per env only)", me);
    if (io->n_envs == 0) return MACJD_OK;
    return launch_step_scan_pe<true>(s, io, scan, scan_pe, pattern, (hipStream_t)hip_stream, me);
}

int macjd_env_step_scan_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan, const macjd_scan_pe_io* scan_pe,
                           void* hip_stream) {
    const char* me = "macjd_env_step_scan_pe";
    int rc = validate_io(s, io);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan(s, scan, me);
    if (rc != MACJD_OK) return rc;
    if (!io->pe_tables) return set_err(MACJD_EINVAL, "%s: needs per-env scenario tables (io->pe_tables); macjd_env_step_scan takes the handle's", me);
    rc = validate_scan_pe(s, scan_pe, io->n_envs, io->pe_tile, me);
    if (rc != MACJD_OK) return rc;
    if (io->n_envs == 0) return MACJD_OK;
    return launch_step_scan_pe<false>(s, io, scan, scan_pe, nullptr, (hipStream_t)hip_stream, me);
}

int macjd_env_reset_scan_pe(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan, const macjd_scan_pe_io* scan_pe,
                            int32_t pe_tile, const uint8_t* mask, void* hip_stream) {
    const char* me = "macjd_env_reset_scan_pe";
    if (!s || n_envs < 0) return set_err(MACJD_EINVAL, "%s: bad argument", me);
    int rc = validate_scan(s, scan, me);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan_pe(s, scan_pe, n_envs, pe_tile, me);
    if (rc != MACJD_OK) return rc;
    if (n_envs == 0) return MACJD_OK;
    hipLaunchKernelGGL(macjd::env_reset_scan_pe_kernel, strided_grid_256(n_envs), dim3(256), 0, (hipStream_t)hip_stream, n_envs,
                       s->host.R, s->host.J, scan_pe->tables, scan_pe->stride, pe_tile, scan->theta_a, scan->a_se, scan->a_sx,
                       scan->state, scan->st_se, scan->st_col0, scan->st_col_step, mask);
    return launch_status(me);
}

int macjd_env_step(const macjd_scenario* s, const macjd_step_io* io, void* hip_stream) {
    int rc = validate_io(s, io);
    if (rc != MACJD_OK) return rc;
    if (io->n_envs == 0) return MACJD_OK;
    return launch_step(s, io, (hipStream_t)hip_stream);
}

// The argument checks of a many-step entry point `me`.  `unwritten` names the per-step outputs such a launch does not write
// ("pd / snr_with", plus "snr_no" where the entry has a block that carries one: `also_unwritten`).
static int validate_many(const macjd_step_io* io, int32_t n_steps, int64_t t_stride, const void* also_unwritten,
                         const char* unwritten, const char* me) {
    if (n_steps < 1 || t_stride < 0) return set_err(MACJD_EINVAL, "%s: bad n_steps / t_stride", me);
    if (io->pd || io->snr_with || also_unwritten) return set_err2(MACJD_EINVAL, "%s: %s are not written (pass NULL)", me, unwritten);
    if (io->r_dpj_sum && !io->r_dpj) return set_err(MACJD_EINVAL, "%s: r_dpj_sum needs the per-step r_dpj buffer", me);
    return MACJD_OK;
}

// Second launch of a many-step entry point: the step counters and the reward-component sums (env_advance_kernel)
static int advance_after_many(const macjd_step_io* io, int32_t n_steps, hipStream_t stream, const char* me) {
    hipLaunchKernelGGL(macjd::env_advance_kernel, strided_grid_256(io->n_envs * 3), dim3(256), 0, stream, io->n_envs, n_steps,
                       io->step, io->r_dpj, io->r_dpj_sum);
    return launch_status(me);
}

int macjd_env_step_many(const macjd_scenario* s, const macjd_step_io* io, int32_t n_steps, int64_t t_stride, void* hip_stream) {
    const char* me = "macjd_env_step_many";
    int rc = validate_io(s, io);
    if (rc != MACJD_OK) return rc;
    rc = validate_many(io, n_steps, t_stride, nullptr, "pd / snr_with", me);
    if (rc != MACJD_OK) return rc;
    if (io->n_envs == 0) return MACJD_OK;
    rc = launch_step(s, io, (hipStream_t)hip_stream, n_steps, t_stride);
    if (rc != MACJD_OK) return rc;
    return advance_after_many(io, n_steps, (hipStream_t)hip_stream, me);
}

}  // extern "C"

// ---- moving scenarios (include/macjd.h, macjd_motion_io and its _pe, _scan, _scan_pe forms; kernels in macjd_env_motion*.hip,
// dispatch in launch_step_moving above): the checks the entry points share (templates among them: C++ linkage) ----

static int validate_motion(const macjd_scenario* s, const macjd_motion_io* mo, const char* what) {
    if (!s || !mo) return set_err(MACJD_EINVAL, "%s: NULL scenario / motion io", what);
    if (!mo->frames || !mo->frame_flags || !mo->positions || !mo->position_columns || !mo->state)
        return set_err(MACJD_EINVAL, "%s: frames / frame_flags / positions / position_columns / state is NULL", what);
    if (mo->n_frames < 1) return set_err(MACJD_EINVAL, "%s: n_frames < 1", what);
    if (mo->n_frames != s->host.episode_limit)
        return set_err(MACJD_EINVAL, "%s: n_frames must equal the scenario's episode_limit", what);
    if (mo->n_pos != 2 * s->host.R + 2 * s->host.J) return set_err(MACJD_EINVAL, "%s: n_pos must equal 2R + 2J", what);
    if (mo->st_se < mo->n_pos) return set_err(MACJD_EINVAL, "%s: state row stride smaller than the number of position columns", what);
    if (mo->snr_no && (!mo->frame_snr_no || mo->sn_se < 0 || mo->sn_sx < 0 || (mo->sn_se == 0 && mo->sn_sx == 0)))
        return set_err(MACJD_EINVAL, "%s: snr_no needs frame_snr_no and non-negative, non-zero strides", what);
    return MACJD_OK;
}

// A per-env motion block as the shared-frame block with the same members: validation, span checks and fill_moving serve both
static macjd_motion_io motion_pe_as_motion(const macjd_motion_pe_io* mp) {
    macjd_motion_io mo{};
    mo.frames = mp->frames; mo.frame_flags = mp->frame_flags; mo.frame_snr_no = mp->frame_snr_no;
    mo.positions = mp->positions; mo.position_columns = mp->position_columns;
    mo.n_frames = mp->n_frames; mo.n_pos = mp->n_pos;
    mo.state = mp->state; mo.st_se = mp->st_se;
    mo.snr_no = mp->snr_no; mo.sn_se = mp->sn_se; mo.sn_sx = mp->sn_sx;
    return mo;
}

// The motion block of either kind, checked, into a->mo / a->tile (tile 0: shared frames)
static int validate_motion_into(const macjd_scenario* s, const macjd_motion_io* mo, MovingArgs* a, const char* what) {
    const int rc = validate_motion(s, mo, what);
    if (rc == MACJD_OK) { a->mo = *mo; a->tile = 0; }
    return rc;
}
static int validate_motion_into(const macjd_scenario* s, const macjd_motion_pe_io* mp, MovingArgs* a, const char* what) {
    if (!s || !mp) return set_err(MACJD_EINVAL, "%s: NULL scenario / motion io", what);
    a->mo = motion_pe_as_motion(mp);
    a->tile = mp->tile;
    const int rc = validate_motion(s, &a->mo, what);
    if (rc != MACJD_OK) return rc;
    if (mp->tile < 1) return set_err(MACJD_EINVAL, "%s: tile < 1", what);
    return MACJD_OK;
}

// Common head of the moving step entry points: the step's own block, then the motion block
template <class Motion>
static int validate_moving_step(const macjd_scenario* s, const macjd_step_io* io, const Motion* motion, MovingArgs* a, const char* me) {
    const int rc = validate_io(s, io);
    return rc != MACJD_OK ? rc : validate_motion_into(s, motion, a, me);
}
static int refuse_pe_tables(const macjd_step_io* io, const char* me) {
    return io->pe_tables ? set_err(MACJD_EINVAL, "%s: io->pe_tables must be NULL (the frames are the tables)", me) : MACJD_OK;
}
static int refuse_slot_kernel(const macjd_step_io* io, const char* me) {
    return (io->flags & MACJD_STEP_SLOT_KERNEL)
               ? set_err(MACJD_EUNSUPPORTED, "%s: the (env x slot) kernel has no moving variant (one lane per env only)", me)
               : MACJD_OK;
}

// The single-step (n_steps = 0) and many-step entry points on shared (Motion = macjd_motion_io) and per-env frames
template <class Motion>
static int env_step_moving(const macjd_scenario* s, const macjd_step_io* io, const Motion* motion, int32_t n_steps, int64_t t_stride,
                           bool many, hipStream_t stream, const char* me) {
    constexpr bool MVPE = std::is_same<Motion, macjd_motion_pe_io>::value;
    MovingArgs a{};
    int rc = validate_moving_step(s, io, motion, &a, me);
    if (rc != MACJD_OK) return rc;
    rc = refuse_pe_tables(io, me);
    if (rc != MACJD_OK) return rc;
    rc = many ? validate_many(io, n_steps, t_stride, a.mo.snr_no, "pd / snr_with / snr_no", me) : refuse_slot_kernel(io, me);
    if (rc != MACJD_OK) return rc;
    if (io->n_envs == 0) return MACJD_OK;
    rc = launch_step_moving<MVPE, false, false>(s, io, a, stream, many ? n_steps : 0, many ? t_stride : 0, me);
    if (rc != MACJD_OK || !many) return rc;
    return advance_after_many(io, n_steps, stream, me);
}

// The scan / pattern frame tables of a moving scanning step or reset `me`
static int validate_motion_scan_levels(const macjd_scenario* s, const macjd_motion_scan_io& ms, const char* me) {
    if (ms.n_levels < 0 || ms.n_levels > MACJD_MAX_PATTERN_LEVELS)
        return set_err(MACJD_EINVAL, "%s: n_levels outside 0..MACJD_MAX_PATTERN_LEVELS", me);
    if (s->host.pat_levels > 0 && s->host.pat_levels != ms.n_levels)
        return set_err(MACJD_EINVAL, "%s: n_levels differs from the pattern levels of the scenario handle", me);
    if ((ms.pattern_frames != nullptr) != (ms.n_levels > 0))
        return set_err(MACJD_EINVAL, "%s: pattern_frames and n_levels > 0 go together (both or neither)", me);
    return MACJD_OK;
}
// `ms` NULL or without scan frames: refused; otherwise a->ms and the level checks
static int validate_motion_scan(const macjd_scenario* s, const macjd_motion_scan_io* ms, MovingArgs* a, const char* me) {
    if (!ms || !ms->scan_frames) return set_err(MACJD_EINVAL, "%s: NULL motion scan io / scan_frames", me);
    a->ms = *ms;
    return validate_motion_scan_levels(s, a->ms, me);
}
// A per-env block as the shared-frame block with the same members (NULL stays NULL)
static const macjd_motion_scan_io* motion_scan_pe_as_motion_scan(const macjd_motion_scan_pe_io* mp, macjd_motion_scan_io* ms) {
    if (!mp) return nullptr;
    ms->scan_frames = mp->scan_frames; ms->pattern_frames = mp->pattern_frames; ms->n_levels = mp->n_levels; ms->reserved = 0;
    return ms;
}

// What a moving scanning step refuses of its motion block (`word`: "motion" or "motion_pe", as the entry point names it)
static int refuse_motion_snr_no(const MovingArgs& a, const char* word, const char* me) {
    return a.mo.snr_no ? set_err2(MACJD_EINVAL, "%s: %s->snr_no must be NULL (the per-step value travels in scan->snr_no)", me, word)
                       : MACJD_OK;
}
static int validate_same_state_rows(const macjd_scan_io* scan, const MovingArgs& a, const char* word, const char* me) {
    if (scan->state && scan->state != a.mo.state)
        return set_err2(MACJD_EINVAL, "%s: scan->state and %s->state must be the same rows", me, word);
    if (scan->state && scan->st_se != a.mo.st_se)
        return set_err2(MACJD_EINVAL, "%s: scan->st_se and %s->st_se must be the same row stride", me, word);
    return MACJD_OK;
}

// Tail of the two moving scanning step entry points, after their block checks: the pattern-or-plain choice and the launch
template <bool MVPE>
static int env_step_moving_scan_tail(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan, MovingArgs& a,
                                     const char* word, hipStream_t stream, const char* me) {
    int rc = validate_same_state_rows(scan, a, word, me);
    if (rc != MACJD_OK) return rc;
    rc = refuse_slot_kernel(io, me);
    if (rc != MACJD_OK) return rc;
    if (io->n_envs == 0) return MACJD_OK;
    a.sc = scan;
    return a.ms.pattern_frames ? launch_step_moving<MVPE, true, true>(s, io, a, stream, 0, 0, me)
                               : launch_step_moving<MVPE, true, false>(s, io, a, stream, 0, 0, me);
}

extern "C" {

int macjd_env_step_moving(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion, void* hip_stream) {
    return env_step_moving(s, io, motion, 0, 0, false, (hipStream_t)hip_stream, "macjd_env_step_moving");
}

int macjd_env_step_many_moving(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion, int32_t n_steps,
                               int64_t t_stride, void* hip_stream) {
    return env_step_moving(s, io, motion, n_steps, t_stride, true, (hipStream_t)hip_stream, "macjd_env_step_many_moving");
}

int macjd_env_reset_moving(const macjd_scenario* s, int64_t n_envs, const macjd_motion_io* motion, const uint8_t* mask,
                           void* hip_stream) {
    const char* me = "macjd_env_reset_moving";
    if (n_envs < 0) return set_err(MACJD_EINVAL, "%s: bad argument", me);
    const int rc = validate_motion(s, motion, me);
    if (rc != MACJD_OK) return rc;
    if (n_envs == 0) return MACJD_OK;
    macjd::launch_motion_reset(strided_grid_256(n_envs), dim3(256), (hipStream_t)hip_stream, n_envs, motion->n_pos, motion->positions,
                               motion->position_columns, motion->state, motion->st_se, mask);
    return launch_status(me);
}

int macjd_env_step_moving_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_pe_io* motion_pe, void* hip_stream) {
    return env_step_moving(s, io, motion_pe, 0, 0, false, (hipStream_t)hip_stream, "macjd_env_step_moving_pe");
}

int macjd_env_step_many_moving_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_pe_io* motion_pe,
                                  int32_t n_steps, int64_t t_stride, void* hip_stream) {
    return env_step_moving(s, io, motion_pe, n_steps, t_stride, true, (hipStream_t)hip_stream, "macjd_env_step_many_moving_pe");
}

int macjd_env_reset_moving_pe(const macjd_scenario* s, int64_t n_envs, const macjd_motion_pe_io* motion_pe, const uint8_t* mask,
                              void* hip_stream) {
    const char* me = "macjd_env_reset_moving_pe";
    if (n_envs < 0) return set_err(MACJD_EINVAL, "%s: bad argument", me);
    MovingArgs a{};
    const int rc = validate_motion_into(s, motion_pe, &a, me);
    if (rc != MACJD_OK) return rc;
    if (n_envs == 0) return MACJD_OK;
    macjd::launch_motion_pe_reset(strided_grid_256(n_envs), dim3(256), (hipStream_t)hip_stream, n_envs, a.mo.n_pos, a.mo.n_frames,
                                  a.tile, a.mo.positions, a.mo.position_columns, a.mo.state, a.mo.st_se, mask);
    return launch_status(me);
}

int macjd_env_step_moving_scan(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion,
                               const macjd_scan_io* scan, const macjd_motion_scan_io* motion_scan, void* hip_stream) {
    const char* me = "macjd_env_step_moving_scan";
    MovingArgs a{};
    int rc = validate_moving_step(s, io, motion, &a, me);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan(s, scan, me);   // (refuses a handle that is not a scanning handle)
    if (rc != MACJD_OK) return rc;
    if (!motion_scan || !motion_scan->scan_frames) return set_err(MACJD_EINVAL, "%s: NULL motion scan io / scan_frames", me);
    a.ms = *motion_scan;
    rc = refuse_pe_tables(io, me);
    if (rc != MACJD_OK) return rc;
    rc = refuse_motion_snr_no(a, "motion", me);
    if (rc != MACJD_OK) return rc;
    rc = validate_motion_scan_levels(s, a.ms, me);   // (this entry point checks the levels after the two refusals)
    if (rc != MACJD_OK) return rc;
    return env_step_moving_scan_tail<false>(s, io, scan, a, "motion", (hipStream_t)hip_stream, me);
}

int macjd_env_step_moving_scan_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_pe_io* motion_pe,
                                  const macjd_scan_io* scan, const macjd_motion_scan_pe_io* motion_scan_pe, void* hip_stream) {
    const char* me = "macjd_env_step_moving_scan_pe";
    MovingArgs a{};
    macjd_motion_scan_io ms;
    int rc = validate_moving_step(s, io, motion_pe, &a, me);
    if (rc != MACJD_OK) return rc;
    rc = validate_scan(s, scan, me);   // (refuses a handle that is not a scanning handle)
    if (rc != MACJD_OK) return rc;
    rc = validate_motion_scan(s, motion_scan_pe_as_motion_scan(motion_scan_pe, &ms), &a, me);
    if (rc != MACJD_OK) return rc;
    rc = refuse_pe_tables(io, me);
    if (rc != MACJD_OK) return rc;
    rc = refuse_motion_snr_no(a, "motion_pe", me);
    if (rc != MACJD_OK) return rc;
    return env_step_moving_scan_tail<true>(s, io, scan, a, "motion_pe", (hipStream_t)hip_stream, me);
}

int macjd_env_reset_moving_scan_pe(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan,
                                   const macjd_motion_scan_pe_io* motion_scan_pe, int32_t n_frames, int32_t tile,
                                   const uint8_t* mask, void* hip_stream) {
    const char* me = "macjd_env_reset_moving_scan_pe";
    if (!s || n_envs < 0) return set_err(MACJD_EINVAL, "%s: bad argument", me);
    MovingArgs a{};
    macjd_motion_scan_io ms;
    int rc = validate_scan(s, scan, me);
    if (rc != MACJD_OK) return rc;
    rc = validate_motion_scan(s, motion_scan_pe_as_motion_scan(motion_scan_pe, &ms), &a, me);
    if (rc != MACJD_OK) return rc;
    if (n_frames < 1) return set_err(MACJD_EINVAL, "%s: n_frames < 1", me);
    if (tile < 1) return set_err(MACJD_EINVAL, "%s: tile < 1", me);
    if (n_envs == 0) return MACJD_OK;
    macjd::launch_motion_scan_pe_reset(strided_grid_256(n_envs), dim3(256), (hipStream_t)hip_stream, n_envs, s->host.R, s->host.J,
                                       n_frames, tile, a.ms.scan_frames, scan->theta_a, scan->a_se, scan->a_sx,
                                       scan->state, scan->st_se, scan->st_col0, scan->st_col_step, mask);
    return launch_status(me);
}

static int env_step_timed_impl(const macjd_scenario* s, const macjd_step_io* io, int iters, void* hip_stream,
                               float* ms_per_launch, int32_t many_T, int64_t t_stride);

int macjd_env_step_timed(const macjd_scenario* s, const macjd_step_io* io, int iters, void* hip_stream,
                         float* ms_per_launch) {
    return env_step_timed_impl(s, io, iters, hip_stream, ms_per_launch, 0, 0);
}

int macjd_env_step_many_timed(const macjd_scenario* s, const macjd_step_io* io, int32_t n_steps, int64_t t_stride, int iters,
                              void* hip_stream, float* ms_per_launch) {
    if (n_steps < 1 || t_stride < 0) return set_err(MACJD_EINVAL, "%s", "macjd_env_step_many_timed: bad n_steps / t_stride");
    return env_step_timed_impl(s, io, iters, hip_stream, ms_per_launch, n_steps, t_stride);
}

static int env_step_timed_impl(const macjd_scenario* s, const macjd_step_io* io, int iters, void* hip_stream,
                               float* ms_per_launch, int32_t many_T, int64_t t_stride) {
    int rc = validate_io(s, io);
    if (rc != MACJD_OK) return rc;
    if (iters < 1 || !ms_per_launch) return set_err(MACJD_EINVAL, "macjd_env_step_timed: bad iters / output");
    hipStream_t stream = (hipStream_t)hip_stream;
    hipEvent_t t0, t1;
    hipError_t err = hipEventCreate(&t0);
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "hipEventCreate: %s", hipGetErrorString(err));
    err = hipEventCreate(&t1);
    if (err != hipSuccess) { (void)hipEventDestroy(t0); return set_err(MACJD_EDEVICE, "hipEventCreate: %s", hipGetErrorString(err)); }
    // The launches are replayed from ONE HIP graph (as in the benchmark's rollout), so the figure is the kernel's
    // back-to-back launch duration on the GPU and not the host's enqueue rate (4 - 9 us per launch, box-dependent,
    // for a 4 us kernel).  If the capture is refused the launches are issued directly.
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t priv = nullptr;
    bool graphed = false;
    // capture + replay on a private stream (the caller's may be the null stream, which cannot be captured), after
    // the caller's earlier work has finished; the events are recorded on the stream the launches run on
    if (hipStreamSynchronize(stream) == hipSuccess && hipStreamCreateWithFlags(&priv, hipStreamNonBlocking) == hipSuccess) {
        if (hipStreamBeginCapture(priv, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            int crc = MACJD_OK;
            for (int i = 0; i < iters && crc == MACJD_OK; ++i) crc = launch_step(s, io, priv, many_T, t_stride);
            const hipError_t ce = hipStreamEndCapture(priv, &graph);
            if (ce == hipSuccess && crc == MACJD_OK && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess)
                graphed = hipGraphLaunch(exec, priv) == hipSuccess && hipStreamSynchronize(priv) == hipSuccess;   // warm
        }
        (void)hipGetLastError();
        if (graphed) stream = priv;
    }
    (void)hipEventRecord(t0, stream);
    if (graphed) {
        if (hipGraphLaunch(exec, stream) != hipSuccess) rc = set_err(MACJD_EDEVICE, "%s", "macjd_env_step_timed: graph launch failed");
    } else {
        for (int i = 0; i < iters && rc == MACJD_OK; ++i) rc = launch_step(s, io, stream, many_T, t_stride);
    }
    (void)hipEventRecord(t1, stream);
    err = hipEventSynchronize(t1);
    // the graph is destroyed with its stream drained (the runtime defers the release of a launched graph to the launch
    // stream's next synchronisation point; that stream is destroyed right below)
    if (priv) (void)hipStreamSynchronize(priv);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    if (priv) (void)hipStreamDestroy(priv);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, t0, t1);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (rc != MACJD_OK) return rc;
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_env_step_timed: %s", hipGetErrorString(err));
    *ms_per_launch = ms / (float)iters;
    return MACJD_OK;
}

}  // extern "C"
