// The one-lane-per-env step kernel (env_step_kernel) with its argument blocks: a header, so that a second translation unit
// (macjd_env_scan_pe.hip, macjd_env_motion.hip, macjd_env_motion_pe.hip, macjd_env_motion_scan.hip, macjd_env_motion_scan_pe.hip) can instantiate it with another unrolling directive on its size-bounded
// loops.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/macjd.h"
#include "macjd_env_dev.h"
#include "macjd_philox.h"

// Directive on env_step_kernel's loops over the radars / jammers that end early at a generic size's run-time R / J
// (N = the compile-time bound).  `#pragma unroll` asks for full unrolling and is dropped by the optimizer when the unrolled
// body passes its size threshold — the generic-size kernel on per-env tables: its loops stay loops and the per-lane arrays
// they index go to scratch (1040 B per lane).  macjd_env_scan_pe.hip unrolls by the explicit count N instead, which has no
// threshold.
#ifndef MACJD_ENV_UNROLL_SIZED
#define MACJD_ENV_UNROLL_SIZED(N) _Pragma("unroll")
#endif

namespace macjd {

// PD32 (production variant on regular scenarios): the detection probability in float32 on the transcendental unit —
// pd = 1 / (1 + 2^y), y = -log2(e) B = ky1 snr + ky0 (one fma, v_exp_f32, v_add, v_rcp_f32: 5 instructions instead of ~60
// float64 ones incl. a 13-term exp polynomial and two refined reciprocals) — used where a value within 1e-5 is all the
// consumer needs (the reward terms), and as a FILTER for the Monte-Carlo compares u <= pd.  The radars' SNR itself is a
// float32 quotient there (GaPs * v_rcp_f32(D supp + Pn), the sum still formed in float64): relative error <= 3.5e-7, i.e.
// |dy| <= |ky1| snr 3.5e-7 + (|y| + |ky0|) 1.8e-7 (the fma and the two constants); |dpd/dy| <= 0.173 pd (1 - pd), which is
// < 1e-3 wherever snr > 3 (B > 4.9): |dpd| <= 3e-7 from the argument; v_exp_f32 and v_rcp_f32 1 ulp each and the add's
// rounding add <= 3e-7: **|pd32 - pd| <= 6e-7**; the float32 image of u is within 1.2e-7.  A compare whose two sides differ
// by more than PD32_BOUND = 4e-6 therefore has the same outcome in float64; the others (~8e-6 of all compares) evaluate
// the exact float64 chain, SNR included.  FSM bits, hit decisions and therefore every integer output are those of the float64 kernel bit for bit; reward
// terms differ from it by <= (R + J) 6e-7 (tested: bitwise-equal track / terminated, rewards within 1e-5, on the 70 000-env
// edge batch).  MACJD_ENV_PD32=0 selects the all-float64 form.
constexpr float PD32_BOUND = 4e-6f;
struct Pd32Consts { float ky1, ky0; };
__device__ __forceinline__ Pd32Consts pd32_consts(double A, double c1, double denB) {
    const double l2e = 1.4426950408889634;
    return Pd32Consts{(float)(-l2e * 10.0 / denB), (float)(-l2e * (10.0 * c1 - A) / denB)};
}
__device__ __forceinline__ float det_prob32(float snr, const Pd32Consts& k) {
    const float y = __builtin_fmaf(snr, k.ky1, k.ky0);
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y));
}

// Uniform of (env e, slot) for the step that starts at `step_before` (include/macjd.h, macjd_step_io.u): supplied by the
// caller, or word (slot & 3) of the env's Philox block (slot >> 2).  This on-demand form generates a whole block per
// call; the kernels below generate each block they need ONCE per env-step and pick words out of it.
template <bool PHILOX_ONLY = false, class IO = macjd_step_io>
__device__ __forceinline__ double draw_uniform(const IO& io, int64_t e, uint32_t episode, int slot,
                                               uint32_t step_before) {
    if (!PHILOX_ONLY && io.u) return io.u[e * io.u_se + (int64_t)slot * io.u_sx];
    const Philox4 r = env_philox_block(io.seed, (uint64_t)(io.env_offset + e), episode, step_before, (uint32_t)(slot >> 2));
    return u32_mid(philox_word(r, slot & 3));
}

// Argument block of the production (FAST) variants: only what that configuration reads or writes, strides as int32.
// A kernel taking the full macjd_step_io keeps ~95 SGPRs of arguments live next to ~70 SGPRs of wave-uniform table
// constants and spills (88 SGPR spills = ~280 v_readlane / v_writelane VALU instructions per env-step at 3j/4r).
struct FastStepIO {
    int64_t n_envs, env_offset;
    uint64_t seed;
    const int32_t* T;
    const float* P32;
    const int32_t* episode;
    uint8_t* track;
    int32_t* step;
    float* reward;
    float* r_dpj;
    uint8_t* terminated;
    float* pd;
    float* snr_with;
    float* r_dpj_sum;
    const double* pe_tables;
    const uint8_t* pe_flags;
    int64_t pe_stride;
    int32_t T_se, T_sx, P_se, P_sx, k_se, k_sx, pd_se, pd_sx, sw_se, sw_sx, pe_tile;
    // macjd_env_step_many: many_T > 0 runs many_T steps of each of n_envs envs as many_T * n_envs work items (time-major:
    // item v = t * n_envs + e), actions of step t at + t * t_stride elements
    int32_t many_T, t_stride;
    // members of macjd_step_io this configuration never has (compile-time constants: the code paths fold away)
    static constexpr const double* u = nullptr;
    static constexpr int64_t u_se = 0, u_sx = 0;
    static constexpr const double* P64 = nullptr;
    static constexpr uint32_t flags = 0;
    static constexpr double* out64 = nullptr;
    static constexpr double* pd64 = nullptr;
    static constexpr double* snr64 = nullptr;
    static constexpr double* prj64 = nullptr;
};

// Argument block of a SCAN launch: the step's own block plus the beam state (include/macjd.h, macjd_scan_io).  A separate
// type, so the non-scanning instantiations keep their argument layout and code.
template <class Base>
struct ScanStepIO : Base {
    double* theta_a;
    int64_t a_se, a_sx;
    float* state;
    int64_t st_se;
    int32_t st_col0, st_col_step;
    float* snr_no;
    int64_t sn_se, sn_sx;
};
// ... of a SCAN launch on per-env scenario tables: plus the per-env scan SoA (include/macjd.h, macjd_scan_pe_io), laid out
// plain or tiled as the step's own pe_tables (pe_tile)
template <class Base>
struct ScanPeStepIO : ScanStepIO<Base> {
    const double* sp_tables;
    int64_t sp_stride;
};
// ... under a stepped antenna pattern: plus the per-env pattern SoA (include/macjd.h, macjd_scan_pe_pattern_io), laid out
// like the two above.  A separate type again: the pattern-free per-env instantiations keep their argument block and code.
template <class Base>
struct ScanPePatStepIO : ScanPeStepIO<Base> {
    const double* pp_tables;
    int64_t pp_stride;
    int32_t pat_levels, pp_reserved;
};

// Argument block of a MOVING launch (include/macjd.h, macjd_motion_io): the step's own block plus the per-step frame tables
// and the state rows whose position columns the step rewrites.  The type switches the kernel (io_moves): the other
// instantiations keep their argument block and code.  Offsets of the production form are 32-bit like FastStepIO's (the host
// checks the spans).
template <class Base>
struct MotionStepIO : Base {
    const double* frames;
    const uint8_t* frame_flags;
    const double* frame_snr_no;
    const float* positions;
    const int32_t* position_columns;
    float* state;
    float* mv_snr_no;
    int64_t mv_st_se, mv_sn_se, mv_sn_sx;
    int32_t n_frames, n_pos;
};
// Argument block of a MOVING SCANNING launch (include/macjd.h, macjd_motion_scan_io): ScanBase = ScanPeStepIO<...> or, under a
// stepped antenna pattern, ScanPePatStepIO<...>, whose sp_tables / pp_tables point at the per-frame scan / pattern tables
// (frame-major like `frames`; the strides are not read), plus the frame tables and positions of MotionStepIO.  The beam
// block's `state` (theta_a columns, optional) and `snr_no` keep their names; the rows whose position columns the step
// rewrites are `mv_state`, and the moving step's own snr_no output does not exist here (the scan block's carries the
// per-step value): compile-time constants, its code folds away.
template <class ScanBase>
struct MotionScanStepIO : ScanBase {
    const double* frames;
    const uint8_t* frame_flags;
    const float* positions;
    const int32_t* position_columns;
    float* mv_state;
    int64_t mv_st_se;
    int32_t n_frames, n_pos;
    static constexpr const double* frame_snr_no = nullptr;
    static constexpr float* mv_snr_no = nullptr;
    static constexpr int64_t mv_sn_se = 0, mv_sn_sx = 0;
};
// Argument block of a MOVING launch on PER-ENV frame tables (include/macjd.h, macjd_motion_pe_io): MotionStepIO's members with
// every table in the tiled per-env layout, the frame index between tile and row; mv_tile = envs per tile.  A type of its own:
// the shared-frame instantiations keep their argument block and code.
template <class Base>
struct MotionPeStepIO : MotionStepIO<Base> {
    int32_t mv_tile, mv_reserved;
};
// Argument block of a MOVING SCANNING launch on PER-ENV frame tables (include/macjd.h, macjd_motion_scan_pe_io):
// MotionScanStepIO's members with every table — frames, flags, positions, scan rows, pattern rows — in the tiled per-env
// layout, the frame index between tile and row; mv_tile = envs per tile.  A type of its own: the shared-frame moving-scanning
// instantiations keep their argument block and code (their scan / pattern column strides stay the constant 1).
template <class ScanBase>
struct MotionScanPeStepIO : MotionScanStepIO<ScanBase> {
    int32_t mv_tile, mv_reserved;
};
template <class IO> struct io_moves : std::false_type {};
template <class Base> struct io_moves<MotionStepIO<Base>> : std::true_type {};
template <class Base> struct io_moves<MotionPeStepIO<Base>> : std::true_type {};
template <class IO> struct io_moves_pe : std::false_type {};
template <class Base> struct io_moves_pe<MotionPeStepIO<Base>> : std::true_type {};
template <class ScanBase> struct io_moves<MotionScanStepIO<ScanBase>> : std::true_type {};
template <class ScanBase> struct io_moves<MotionScanPeStepIO<ScanBase>> : std::true_type {};
template <class ScanBase> struct io_moves_pe<MotionScanPeStepIO<ScanBase>> : std::true_type {};

// Per-lane pattern state of an env-step: the number of levels and the target's level at each radar, four bits per radar
// in 64-bit words (word r >> 4; shifts only, so the per-lane index of the PD32 re-evaluation loop — compiled sizes,
// R <= 16, one word — is no private-array index).  Empty without a pattern: those instantiations carry nothing.
template <bool PAT, int NR>
struct PatLanes {
    static constexpr int L = 0;
    __device__ __forceinline__ void set(int, int) {}
    __device__ __forceinline__ int lv(int) const { return 0; }
};
template <int NR>
struct PatLanes<true, NR> {
    int L;
    uint64_t w[(NR + 15) / 16];
    __device__ __forceinline__ void set(int r, int k) { w[NR > 16 ? (r >> 4) : 0] |= (uint64_t)k << ((r & 15) * 4); }
    __device__ __forceinline__ int lv(int r) const { return (int)((w[NR > 16 ? (r >> 4) : 0] >> ((r & 15) * 4)) & 15u); }
};

// PE = per-env scenario tables (io.pe_tables, SoA [row][env]): every table read becomes a load from this lane's
// column of the SoA (row index static for the per-jammer / per-radar loops, data-dependent for the reads gathered by
// the chosen target radar); the shared-table variant stages the gathered tables in LDS instead.
// FAST = the production configuration fixed at compile time: uniforms from Philox (io.u == NULL), float32 actions with
// the reference's float32 power arithmetic (io.P32, no MACJD_STEP_ARITH_F64), no float64 diagnostics.  At streaming
// sizes the kernel is VALU-issue bound (PMC: ~1670 VALU instructions per 64-env iteration, VALU busy 73 % of the
// kernel); the run-time mode tests cost ~50 uniform branches and, through the extra live pointers, ~400 SGPR spill
// instructions (v_writelane / v_readlane) per iteration.
// REG = FAST on the shared tables of a REGULAR scenario (DevTables.regular, decided by macjd_scenario_create): every
// division whose divisor is a table value — the received-power quotient (float64 or float32, chosen per (jammer, radar)
// pair), the false-target SNR, the power normalisation — multiplies by the divisor's refined reciprocal from the
// tables (3 instead of 13 / 10 instructions; a float32 quotient is the float64 one rounded once more, which is exact for
// a quotient of two float32 values: 53 >= 2 * 24 + 2 bits), the radars' SNR division drops the scaling wrapper, and
// the guards that a regular scenario can never trigger (non-positive or tiny noise power, SNR < 0, the probability
// formula's saturation selects) are not evaluated.  Same results bit for bit (tests: lane kernel vs (env x slot) kernel,
// which keeps IEEE division and every guard, and both vs the oracle); 1285 -> ~1050 VALU instructions per env-step at 3j/4r.
// SCAN = scanning beams (include/macjd.h, macjd_scan_desc; IO = ScanStepIO<...>): the env's azimuths live in registers for
// the step, the per-radar main-lobe test of the target selects the main or side-lobe (GaPs, pd_no), a jammer's test on
// its chosen radar selects gr or gr_side; the rest of the step is unchanged.  Single-step launches.
// SCAN && PE (IO = ScanPeStepIO<...>): every scan quantity comes from this env's column of the per-env scan SoA
// (MACJD_PE_SCAN_ROWS rows: half | sweep | sweep_mod | az0 | bear_tgt | GaPs_side | snr_no | snr_no_side | pd_no_side |
// gr_side | bear_jam[J*R]) instead of DevTables / its LDS copies, requested with the pe_tables rows (HOIST); h2 = 2 half and
// full = (sweep + h2 >= 360) are formed per lane (both exact restatements of the host's values).  Same arithmetic, order,
// RNG slots and stores as the shared-table SCAN kernel in its general all-float64 form: bit-identical results.
// PAT = SCAN under a stepped antenna pattern (include/macjd.h, macjd_scan_pattern_desc; the same ScanStepIO<...> block):
// the two-way selects become a level 0..L + 1 per object (beam_level) that indexes the [L + 2, R] level tables staged in
// LDS; the target's R levels of an env are packed four bits each into 64-bit words (shifts by compile-time amounts, never
// a register array indexed per lane).
// PAT && PE (IO = ScanPePatStepIO<...>): inv_width and the four level tables come from this env's column of the per-env
// pattern SoA (MACJD_PE_SCAN_PATTERN_ROWS rows: inv_width[R] | GaPs_lvl | snr_no_lvl | pd_no_lvl | gr_lvl, each [(L + 2) R]
// level-major with level 0 = the env's main-lobe values and level L + 1 its side-lobe ones), L from the argument block; the
// handle's level tables are never read and nothing is staged in LDS.  The level tables are NOT requested up front (32 R
// rows at L = 6): once an object's level is known, the one selected row per (table, radar) is loaded by address,
// as the pattern-free per-env kernel loads its snr_no row.  beam_level, arithmetic, order, RNG slots, beam advance and
// stores are those of the shared-table PAT kernel in its general all-float64 form: bit-identical results.
// (PAT was first switched by the type of the argument block, so that the kernel
// kept its template parameter list; the parameter changes only the kernels' names, profiles/r10_env_isa_check.txt.)
template <int JT, int RT, bool PE, bool FAST, class IO, bool REG = false, bool PD32 = false, bool SCAN = false, bool PAT = false>
__global__ void __launch_bounds__(256) env_step_kernel(const DevTables* __restrict__ tb, const IO io) {
    static_assert(!REG || (FAST && !PE && JT && RT), "REG: production variant on shared tables, compiled sizes");
    static_assert(!PD32 || REG, "PD32: float32 detection-probability filter of the regular production variant");
    static_assert(!PAT || SCAN, "PAT: stepped antenna pattern of the scanning beams");
    constexpr bool SPE = SCAN && PE;    // scanning beams on per-env tables
    constexpr bool SPP = PAT && PE;     // ... under a stepped pattern: level tables from the env's column
    constexpr bool PSH = PAT && !PE;    // the pattern's level tables of the handle (LDS copies)
    static_assert(!SPP || !FAST || (JT && RT), "PAT on per-env tables: production variant at compiled sizes only");
    constexpr bool SSH = SCAN && !PE;   // ... on the shared tables (LDS copies of the gathered ones)
    // MOV (IO = MotionStepIO<...>; include/macjd.h, macjd_motion_io): the per-env-table path with the table column chosen by
    // the env's step counter instead of by its index, plus the position columns of the env's state row, rewritten with the
    // next frame's positions.  Same arithmetic, order, RNG slots and stores as the PE kernel of the same form.
    constexpr bool MOV = io_moves<IO>::value;
    // MOV && SCAN (IO = MotionScanStepIO<...>; include/macjd.h, macjd_motion_scan_io): the scan rows, and under PAT the
    // pattern rows, come from frame f of per-frame tables in the same way; the tail writes the theta_a columns and the
    // position columns of the env's state row.
    static_assert(!MOV || PE, "MOV: the per-env-table path of the step");
    // MOV on per-env frame tables (IO = MotionPeStepIO<...>; include/macjd.h, macjd_motion_pe_io): the same path with MotionStepIO
    // generalised by an env tile — row stride = tile, tile index (e / tile) * F + f, column e % tile.  With SCAN
    // (IO = MotionScanPeStepIO<...>; macjd_motion_scan_pe_io) the scan and pattern rows take the same stride, tile and column.
    constexpr bool MVPE = io_moves_pe<IO>::value;
    constexpr int NJ = JT ? JT : MAXJ;
    constexpr int NR = RT ? RT : MAXR;
    const int J = JT ? JT : tb->J;
    const int R = RT ? RT : tb->R;

    // ---- LDS staging of the tables gathered by per-lane target index (shared-table variant) ----
    __shared__ double s_denom[PE ? 1 : NJ * NR];   // REG: the divisor as used (DevTables.dsel)
    __shared__ double s_rsel[REG ? NJ * NR : 1], s_rPn[REG ? NR : 1];
    // REG: the per-radar suppression sums and false-target products of a lane live in its own LDS column and a jammer
    // adds into the row of the radar it chose (one ds_read / ds_write pair on the LDS port) instead of J x R
    // compare / select / fma chains on the VALU, which is the unit this kernel is bound by; row NR takes the
    // contributions of jammers that have none.  Same operations in the same (jammer) order on the same values.
    // (also the per-env-table production variant: its lanes hold ~45 table values each, every register counts)
#ifndef MACJD_PE_SCAT
#define MACJD_PE_SCAT 1   // build knob for A/B runs: 0 keeps the per-env variant's accumulators in registers
#endif
    constexpr bool SCAT = REG || (MACJD_PE_SCAT && PE && FAST && JT && RT);
    constexpr int ACC_W = SCAT ? 256 : 1;
    __shared__ double s_supp[SCAT ? NR + 1 : 1][ACC_W], s_prod[SCAT ? NR + 1 : 1][ACC_W];
    __shared__ double s_D[PE ? 1 : NR], s_Pn[PE ? 1 : NR], s_gr[PE ? 1 : NR];
    __shared__ uint8_t s_flags[PE ? 1 : NJ * NR];
    // SCAN: tables gathered by a jammer's chosen radar
    __shared__ double s_half[SSH ? NR : 1], s_h2[SSH ? NR : 1], s_sweep[SSH ? NR : 1], s_grs[SSH ? NR : 1];
    __shared__ double s_bj[SSH ? NJ * NR : 1];
    __shared__ uint8_t s_full[SSH ? NR : 1];
    // PAT: level tables [L + 2, R] (row 0 main, 1..L the pattern's levels, L + 1 side lobe), indexed by the per-lane level
    __shared__ double s_lgr[PSH ? MAXLV * NR : 1], s_lGaPs[PSH ? MAXLV * NR : 1], s_lpdno[PSH ? MAXLV * NR : 1];
    __shared__ double s_lsnrno[PSH ? MAXLV * NR : 1], s_invw[PSH ? NR : 1];
    if constexpr (PSH) {
        const int pat_L = tb->pat_levels;
        for (int i = threadIdx.x; i < (pat_L + 2) * R; i += blockDim.x) {
            s_lgr[i] = tb->lv_gr[i];
            s_lGaPs[i] = tb->lv_GaPs[i];
            s_lpdno[i] = tb->lv_pd_no[i];
            s_lsnrno[i] = tb->lv_snr_no[i];
        }
        for (int i = threadIdx.x; i < R; i += blockDim.x) s_invw[i] = tb->pat_inv_width[i];
    }
    if constexpr (SSH) {
        for (int i = threadIdx.x; i < J * R; i += blockDim.x) s_bj[i] = tb->bj[i];
        for (int i = threadIdx.x; i < R; i += blockDim.x) {
            s_half[i] = tb->half[i];
            s_h2[i] = tb->h2[i];
            s_sweep[i] = tb->sweep[i];
            s_grs[i] = tb->gr_side[i];
            s_full[i] = tb->full[i];
        }
    }
    if (!PE) {
        for (int i = threadIdx.x; i < J * R; i += blockDim.x) {
            s_denom[i] = REG ? tb->dsel[i] : tb->denom[i];
            s_flags[i] = REG ? tb->rflags[i] : tb->flags[i];
            if (REG) s_rsel[i] = tb->rsel[i];
        }
        for (int i = threadIdx.x; i < R; i += blockDim.x) {
            s_D[i] = tb->D[i];
            s_Pn[i] = tb->Pn[i];
            s_gr[i] = tb->gr[i];
            if (REG) s_rPn[i] = tb->rPn[i];
        }
        __syncthreads();
    }

    const double rp_min = tb->rp_min, rp_max = tb->rp_max;
    const PdConsts pdk = pd_consts(tb->pd_A, tb->pd_c1, tb->pd_denB);
    const Pd32Consts pdk32 = pd32_consts(tb->pd_A, tb->pd_c1, tb->pd_denB);
    const int32_t episode_limit = tb->episode_limit;
    const bool arith32 = FAST ? true : ((io.P32 != nullptr) && !(io.flags & MACJD_STEP_ARITH_F64));

    auto env_step_one = [&](const int64_t e, const int32_t tt) {
        // many-step launches (production variant only, macjd_env_step_many): work item (step tt, env e), outputs of the
        // item at index tt * n_envs + e (the step is wave-uniform: a scalar multiply); single-step launches: tt = 0
        bool many = false, last_t = true;
        if constexpr (FAST) {
            if (io.many_T > 0) {   // grid = (envs / 256, steps): no division
                many = true;
                last_t = (tt == io.many_T - 1);
            }
        }
        const int64_t e_item = FAST ? (int64_t)((uint32_t)tt * (uint32_t)io.n_envs + (uint32_t)e) : e;
        int64_t act_extra = 0;   // element offset of step t's actions
        if constexpr (FAST) act_extra = (int64_t)tt * io.t_stride;
        // Element (env e, item k) of a caller-strided array.  Production variant: the BYTE offset is formed in 32 bits
        // (the host checks that every offset of the launch fits) and added to the wave-uniform base pointer, which is
        // the SGPR-base + 32-bit-VGPR-offset addressing form of global_load / global_store — no 64-bit VALU address
        // arithmetic per access (~50 instructions per env-step at 3j/4r).
        auto at = [&](auto* base, int64_t env, auto se, int k, auto sx, int64_t extra = 0) -> decltype(*base)& {
            using T_ = std::remove_reference_t<decltype(*base)>;
            if constexpr (FAST) {
                const uint32_t off = ((uint32_t)env * (uint32_t)se + (uint32_t)k * (uint32_t)sx + (uint32_t)extra) * (uint32_t)sizeof(T_);
                using C_ = std::conditional_t<std::is_const_v<T_>, const char, char>;
                return *reinterpret_cast<T_*>(reinterpret_cast<C_*>(base) + off);
            } else {
                return base[env * (int64_t)se + (int64_t)k * (int64_t)sx + extra];
            }
        };
        const int32_t step_before = at(io.step, e, 1, 0, 0) + tt;
        const int32_t step_count = step_before + 1;  // environment.py:235
        const uint32_t episode = io.episode ? (uint32_t)at(io.episode, e, 1, 0, 0) : 0u;
        // Monte-Carlo uniforms of this env-step (R radar slots, then one per valid deception action): every Philox
        // block is generated once (ceil((R + J) / 4) blocks: 2 at 3j/4r); the radar pass reads its words at
        // compile-time indices, a deception action selects word R + n_dec.
        constexpr bool PRE = JT && RT;   // generic sizes generate a block on demand instead
        constexpr int NBLK = PRE ? (NJ + NR + 3) / 4 : 1;
        uint32_t rw[NBLK * 4];
        const bool own_rng = FAST || !io.u;
        auto gen_blocks = [&](const int b0, const int b1) {
#pragma unroll
            for (int b = b0; b < b1; ++b) {
                const Philox4 blk = env_philox_block(io.seed, (uint64_t)(io.env_offset + e), episode,
                                                     (uint32_t)step_before, (uint32_t)b);
#pragma unroll
                for (int i = 0; i < 4; ++i) rw[b * 4 + i] = blk.v[i];
            }
        };
        if (PRE && own_rng) gen_blocks(0, NBLK);

        // table accessors: this env's SoA column (PE) or the shared tables
        // this env's column of the per-env tables: plain SoA (row stride pe_stride) or tiled (row stride = tile width)
        // MOV: the column is frame f = min(step_before, n_frames - 1) of the frame-major tables — the tiled layout at tile
        // width 1 with the frame index as the tile index (row stride 1: one contiguous block per env-step)
        int32_t mv_frame = 0;
        if constexpr (MOV) {
            mv_frame = step_before < io.n_frames - 1 ? step_before : io.n_frames - 1;
            mv_frame = mv_frame > 0 ? mv_frame : 0;
        }
        // MVPE: this env's tile and column of the per-env frame tables (production form: 32-bit division, the host checks
        // that every env index fits); the shared-frame form is tile width 1 with the frame as the tile: constants
        int64_t mv_ps = 1, mv_tile_idx = mv_frame, mv_col = 0, mv_env_tile = 0;
        if constexpr (MVPE) {
            if constexpr (FAST) mv_env_tile = (int64_t)((uint32_t)e / (uint32_t)io.mv_tile);
            else mv_env_tile = e / io.mv_tile;
            mv_ps = io.mv_tile;
            mv_col = e - mv_env_tile * io.mv_tile;
            mv_tile_idx = mv_env_tile * io.n_frames + mv_frame;
        }
        const int64_t ps = MOV ? mv_ps : (PE && io.pe_tile > 0) ? (int64_t)io.pe_tile : io.pe_stride;
        const int64_t pe_tile_idx = MOV ? mv_tile_idx : (PE && io.pe_tile > 0) ? e / io.pe_tile : 0;
        const int64_t pe_col = MOV ? mv_col : (PE && io.pe_tile > 0) ? e - pe_tile_idx * io.pe_tile : e;
        const double* pe_base = nullptr;
        const uint8_t* pf_base = nullptr;
        if constexpr (MOV) { pe_base = io.frames; pf_base = io.frame_flags; }
        else if constexpr (PE) { pe_base = io.pe_tables; pf_base = io.pe_flags; }
        const double* __restrict__ pe = PE ? pe_base + pe_tile_idx * (6 * R + 3 * J + J * R) * ps + pe_col : nullptr;
        const uint8_t* __restrict__ pf = PE ? pf_base + pe_tile_idx * (J * R) * ps + pe_col : nullptr;
        // PE, compile-time sizes: every table value this env-step can touch is requested up front so that all the
        // loads are in flight together — left at their use sites they sit behind branches and possibly-aliasing
        // stores and arrive one memory latency at a time.  Static-index rows (per radar / per jammer) directly; the
        // rows gathered by a jammer's chosen target radar after a pre-pass that decodes the J actions.
        constexpr bool HOIST = PE && JT && RT;
        double pv_r[HOIST ? 5 * NR : 1], pv_j[HOIST ? 3 * NJ : 1];
        double gv_denom[HOIST ? NJ : 1], gv_gr[HOIST ? NJ : 1], gv_Pn[HOIST ? NJ : 1], gv_D[HOIST ? NJ : 1];
        uint8_t gv_fl[HOIST ? NJ : 1];
        if (HOIST) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
#pragma unroll
                for (int r = 0; r < NR; ++r) pv_r[k * NR + r] = pe[(int64_t)(k * R + r) * ps];   // GaPs, Pn, D, pd_no, rd_pen
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < NJ; ++j) pv_j[k * NJ + j] = pe[(int64_t)(6 * R + k * J + j) * ps];   // pmin, pmax, gj
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int32_t Tj = at(io.T, e, io.T_se, j, io.T_sx, act_extra);
                const int tj = ((Tj >= 1) && (Tj <= 2 * R)) ? ((Tj + 1) / 2 - 1) : 0;
                gv_denom[j] = pe[(int64_t)(6 * R + 3 * J + j * R + tj) * ps];
                gv_gr[j] = pe[(int64_t)(5 * R + tj) * ps];
                gv_Pn[j] = pe[(int64_t)(R + tj) * ps];
                gv_D[j] = pe[(int64_t)(2 * R + tj) * ps];
                gv_fl[j] = pf[(int64_t)(j * R + tj) * ps];
            }
        }
        // SCAN on per-env tables: this env's column of the scan SoA, its rows requested with the ones above — the rows the
        // radar loops index statically (snr_no / snr_no_side: one of the two per radar, by address, once the main-lobe
        // test is known), and the four values gathered by a jammer's chosen target radar in a pre-pass of their own
        const double* __restrict__ sp = nullptr;
        int64_t sps = 0;
        if constexpr (SPE) {
            if constexpr (MVPE) sps = mv_ps;   // per-env frames: row stride = the env tile
            else if constexpr (MOV) sps = 1;   // frame-major: one contiguous block per frame
            else sps = io.pe_tile > 0 ? (int64_t)io.pe_tile : io.sp_stride;
            sp = io.sp_tables + pe_tile_idx * (10 * R + J * R) * sps + pe_col;
        }
        constexpr bool SHOIST = SPE && HOIST;
        enum { SP_HALF = 0, SP_SWEEP, SP_SWM, SP_AZ0, SP_BT, SP_GAPS_SIDE, SP_SNR_NO, SP_SNR_NO_SIDE, SP_PD_NO_SIDE, SP_GR_SIDE, SP_BJ };
        double sv_half[SHOIST ? NR : 1], sv_sweep[SHOIST ? NR : 1], sv_swm[SHOIST ? NR : 1], sv_bt[SHOIST ? NR : 1];
        double sv_GaPs_side[SHOIST ? NR : 1], sv_pdno_side[SHOIST ? NR : 1], sv_snrno[SHOIST ? NR : 1];
        double gs_half[SHOIST ? NJ : 1], gs_sweep[SHOIST ? NJ : 1], gs_grs[SHOIST ? NJ : 1], gs_bj[SHOIST ? NJ : 1];
        // PAT on per-env tables: this env's column of the pattern SoA — inv_width requested with the rows above (per radar,
        // and gathered by a jammer's chosen radar); of the level tables only the rows an object's level selects, later
        const double* __restrict__ pp = nullptr;
        int64_t pps = 0, pp_lv = 0;   // pp_lv = (L + 2) R: rows of one level table
        if constexpr (SPP) {
            if constexpr (MVPE) pps = mv_ps;
            else if constexpr (MOV) pps = 1;
            else pps = io.pe_tile > 0 ? (int64_t)io.pe_tile : io.pp_stride;
            pp_lv = (int64_t)(io.pat_levels + 2) * R;
            pp = io.pp_tables + pe_tile_idx * (R + 4 * pp_lv) * pps + pe_col;
        }
        constexpr bool PHOIST = SPP && HOIST;
        enum { PP_GAPS = 0, PP_SNR_NO, PP_PD_NO, PP_GR };   // level table k at rows R + k (L + 2) R
        double sv_invw[PHOIST ? NR : 1], gs_invw[PHOIST ? NJ : 1];
        double lv_GaPs[PHOIST ? NR : 1], lv_pdno[PHOIST ? NR : 1], lv_snrno[PHOIST ? NR : 1];
        if constexpr (SHOIST) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                sv_half[r] = sp[(int64_t)(SP_HALF * R + r) * sps];
                sv_sweep[r] = sp[(int64_t)(SP_SWEEP * R + r) * sps];
                sv_swm[r] = sp[(int64_t)(SP_SWM * R + r) * sps];
                sv_bt[r] = sp[(int64_t)(SP_BT * R + r) * sps];
                if constexpr (PHOIST) {
                    sv_invw[r] = pp[(int64_t)r * pps];
                } else {
                    sv_GaPs_side[r] = sp[(int64_t)(SP_GAPS_SIDE * R + r) * sps];
                    sv_pdno_side[r] = sp[(int64_t)(SP_PD_NO_SIDE * R + r) * sps];
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int32_t Tj = at(io.T, e, io.T_se, j, io.T_sx, act_extra);
                const int tj = ((Tj >= 1) && (Tj <= 2 * R)) ? ((Tj + 1) / 2 - 1) : 0;
                gs_half[j] = sp[(int64_t)(SP_HALF * R + tj) * sps];
                gs_sweep[j] = sp[(int64_t)(SP_SWEEP * R + tj) * sps];
                if constexpr (PHOIST) gs_invw[j] = pp[(int64_t)tj * pps];
                else gs_grs[j] = sp[(int64_t)(SP_GR_SIDE * R + tj) * sps];
                gs_bj[j] = sp[(int64_t)(SP_BJ * R + j * R + tj) * sps];
            }
        }
        // row of level k of radar r in level table `tab` of this env's pattern column
        auto pp_row = [&](int tab, int k, int r) -> double { return pp[((int64_t)R + tab * pp_lv + (int64_t)(k * R + r)) * pps]; };
        // scan tables of radar r (static index): the env's column or the handle's tables
        auto c_half = [&](int r) -> double {
            if constexpr (SHOIST) return sv_half[r]; else if constexpr (SPE) return sp[(int64_t)(SP_HALF * R + r) * sps]; else return tb->half[r];
        };
        auto c_sweep = [&](int r) -> double {
            if constexpr (SHOIST) return sv_sweep[r]; else if constexpr (SPE) return sp[(int64_t)(SP_SWEEP * R + r) * sps]; else return tb->sweep[r];
        };
        auto c_swm = [&](int r) -> double {
            if constexpr (SHOIST) return sv_swm[r]; else if constexpr (SPE) return sp[(int64_t)(SP_SWM * R + r) * sps]; else return tb->swm[r];
        };
        auto c_bt = [&](int r) -> double {
            if constexpr (SHOIST) return sv_bt[r]; else if constexpr (SPE) return sp[(int64_t)(SP_BT * R + r) * sps]; else return tb->bt[r];
        };
        auto c_h2 = [&](int r) -> double {
            if constexpr (SPE) return 2.0 * c_half(r); else return tb->h2[r];
        };
        auto c_full = [&](int r) -> bool {
            if constexpr (SPE) return c_sweep(r) + 2.0 * c_half(r) >= 360.0; else return tb->full[r] != 0;
        };
        auto t_GaPs = [&](int r) { return HOIST ? pv_r[0 * NR + r] : PE ? pe[(int64_t)(r) * ps] : tb->GaPs[r]; };
        auto t_Pn = [&](int r) { return HOIST ? pv_r[1 * NR + r] : PE ? pe[(int64_t)(R + r) * ps] : tb->Pn[r]; };
        auto t_D = [&](int r) { return HOIST ? pv_r[2 * NR + r] : PE ? pe[(int64_t)(2 * R + r) * ps] : tb->D[r]; };
        auto t_pdno = [&](int r) { return HOIST ? pv_r[3 * NR + r] : PE ? pe[(int64_t)(3 * R + r) * ps] : tb->pd_no[r]; };
        auto t_rdpen = [&](int r) { return HOIST ? pv_r[4 * NR + r] : PE ? pe[(int64_t)(4 * R + r) * ps] : tb->rd_pen[r]; };
        auto t_pmin = [&](int j) { return HOIST ? pv_j[0 * NJ + j] : PE ? pe[(int64_t)(6 * R + j) * ps] : tb->pmin[j]; };
        auto t_pmax = [&](int j) { return HOIST ? pv_j[1 * NJ + j] : PE ? pe[(int64_t)(6 * R + J + j) * ps] : tb->pmax[j]; };
        auto t_gj = [&](int j) { return HOIST ? pv_j[2 * NJ + j] : PE ? pe[(int64_t)(6 * R + 2 * J + j) * ps] : tb->gj[j]; };
        // gathered by jammer j's chosen target radar t
        auto g_gr = [&](int j, int t) { return HOIST ? gv_gr[j] : PE ? pe[(int64_t)(5 * R + t) * ps] : s_gr[t]; };
        auto g_Pn = [&](int j, int t) { return HOIST ? gv_Pn[j] : PE ? pe[(int64_t)(R + t) * ps] : s_Pn[t]; };
        auto g_D = [&](int j, int t) { return HOIST ? gv_D[j] : PE ? pe[(int64_t)(2 * R + t) * ps] : s_D[t]; };
        auto g_denom = [&](int j, int t) {
            return HOIST ? gv_denom[j] : PE ? pe[(int64_t)(6 * R + 3 * J + j * R + t) * ps] : s_denom[j * R + t];
        };
        auto g_flags = [&](int j, int t) {
            return HOIST ? gv_fl[j] : PE ? pf[(int64_t)(j * R + t) * ps] : s_flags[j * R + t];
        };

        // ---- SCAN: beam azimuths and FSM states at the start of the step, main-lobe test of the target per radar ----
        // (compiled sizes keep the azimuths in registers; generic sizes read them again from the env's row)
        constexpr int NS = (SCAN && PRE) ? NR : 1;
        double az[NS];
        uint32_t s_bits = 0, in_t = 0;   // bit r: radar r was TRACKing / sees the target in its main lobe
        PatLanes<PAT, NR> pl;
        if constexpr (PAT) {
            if constexpr (SPP) pl.L = io.pat_levels; else pl.L = tb->pat_levels;
#pragma unroll
            for (int i = 0; i < (NR + 15) / 16; ++i) pl.w[i] = 0;
        }
        if constexpr (SCAN) {
MACJD_ENV_UNROLL_SIZED(NR)
            for (int r = 0; r < NR; ++r) {
                if (!RT && r >= R) break;
                const double a = at(io.theta_a, e, io.a_se, r, io.a_sx);
                const bool s = at(io.track, e, io.k_se, r, io.k_sx) != 0;
                if (PRE) az[PRE ? r : 0] = a;
                s_bits |= s ? (1u << r) : 0u;
                const double lim = (s ? 0.0 : c_sweep(r)) + c_h2(r);
                if constexpr (SPP) {
                    const double iw = PHOIST ? sv_invw[PHOIST ? r : 0] : pp[(int64_t)r * pps];
                    const int k = beam_level(c_bt(r), a, c_half(r), lim, c_full(r), iw, pl.L);
                    pl.set(r, k);
                    in_t |= (k == 0) ? (1u << r) : 0u;
                    if constexpr (PHOIST) {   // the level's rows, by address (generic sizes load them where they are used)
                        lv_GaPs[r] = pp_row(PP_GAPS, k, r);
                        lv_pdno[r] = pp_row(PP_PD_NO, k, r);
                        if (io.snr_no) lv_snrno[r] = pp_row(PP_SNR_NO, k, r);
                    }
                } else if constexpr (PAT) {
                    const int k = beam_level(tb->bt[r], a, tb->half[r], lim, tb->full[r] != 0, tb->pat_inv_width[r], pl.L);
                    pl.set(r, k);
                    in_t |= (k == 0) ? (1u << r) : 0u;
                } else {
                    const bool in = in_main_lobe(c_bt(r), a, c_half(r), lim, c_full(r));
                    in_t |= in ? (1u << r) : 0u;
                    if constexpr (SHOIST)   // the SNR without jamming this step reports: main or side-lobe row, by address
                        if (io.snr_no) sv_snrno[r] = sp[(int64_t)((in ? SP_SNR_NO : SP_SNR_NO_SIDE) * R + r) * sps];
                }
            }
        }
        // receive gain of jammer j's action on radar t: main or side lobe by the jammer's bearing (SCAN)
        auto scan_gr = [&](int j, int t) -> double {
            if constexpr (SCAN) {
                // the chosen radar's azimuth from the env's row (cache-hot: loaded above); a select chain over az[] is
                // turned into a dynamically indexed private array by hipcc (scratch)
                const double a_t = at(io.theta_a, e, io.a_se, t, io.a_sx);
                if constexpr (SPE) {   // the chosen radar's rows of this env's column (compiled sizes: requested up front)
                    const double half_t = SHOIST ? gs_half[SHOIST ? j : 0] : sp[(int64_t)(SP_HALF * R + t) * sps];
                    const double sweep_t = SHOIST ? gs_sweep[SHOIST ? j : 0] : sp[(int64_t)(SP_SWEEP * R + t) * sps];
                    // (PAT reads no side-lobe row: its level L + 1 holds it.  The load keeps its place among the others:
                    // moved behind them, the pattern-free generic-size kernel compiles to other code)
                    const double grs_t = SPP ? 0.0 : SHOIST ? gs_grs[SHOIST ? j : 0] : sp[(int64_t)(SP_GR_SIDE * R + t) * sps];
                    const double bj_t = SHOIST ? gs_bj[SHOIST ? j : 0] : sp[(int64_t)(SP_BJ * R + j * R + t) * sps];
                    const double h2_t = 2.0 * half_t;
                    const double lim_t = (((s_bits >> t) & 1u) ? 0.0 : sweep_t) + h2_t;
                    if constexpr (SPP) {   // the jammer's level at its chosen radar selects the gr row, loaded here
                        const double iw_t = PHOIST ? gs_invw[PHOIST ? j : 0] : pp[(int64_t)t * pps];
                        return pp_row(PP_GR, beam_level(bj_t, a_t, half_t, lim_t, sweep_t + h2_t >= 360.0, iw_t, pl.L), t);
                    }
                    return in_main_lobe(bj_t, a_t, half_t, lim_t, sweep_t + h2_t >= 360.0) ? g_gr(j, t) : grs_t;
                }
                const double lim = (((s_bits >> t) & 1u) ? 0.0 : s_sweep[t]) + s_h2[t];
                if constexpr (PAT)
                    return s_lgr[beam_level(s_bj[j * R + t], a_t, s_half[t], lim, s_full[t] != 0, s_invw[t], pl.L) * R + t];
                return in_main_lobe(s_bj[j * R + t], a_t, s_half[t], lim, s_full[t] != 0) ? s_gr[t] : s_grs[t];
            } else {
                return 0.0;
            }
        };
        // target-path tables of radar r: main or side lobe (SCAN)
        auto r_GaPs = [&](int r) -> double {
            if constexpr (SPP) return PHOIST ? lv_GaPs[PHOIST ? r : 0] : pp_row(PP_GAPS, pl.lv(r), r);
            else if constexpr (PAT) return s_lGaPs[pl.lv(r) * R + r];
            else if constexpr (SPE)
                return ((in_t >> r) & 1u) ? t_GaPs(r) : (SHOIST ? sv_GaPs_side[SHOIST ? r : 0] : sp[(int64_t)(SP_GAPS_SIDE * R + r) * sps]);
            else if constexpr (SCAN) return ((in_t >> r) & 1u) ? tb->GaPs[r] : tb->GaPs_side[r];
            else return t_GaPs(r);
        };
        auto r_pdno = [&](int r) -> double {
            if constexpr (SPP) return PHOIST ? lv_pdno[PHOIST ? r : 0] : pp_row(PP_PD_NO, pl.lv(r), r);
            else if constexpr (PAT) return s_lpdno[pl.lv(r) * R + r];
            else if constexpr (SPE)
                return ((in_t >> r) & 1u) ? t_pdno(r) : (SHOIST ? sv_pdno_side[SHOIST ? r : 0] : sp[(int64_t)(SP_PD_NO_SIDE * R + r) * sps]);
            else if constexpr (SCAN) return ((in_t >> r) & 1u) ? tb->pd_no[r] : tb->pd_no_side[r];
            else return t_pdno(r);
        };

        // The step runs as straight-line passes over the (compile-time unrolled) jammers and radars: (1) decode, power,
        // received power, suppression sums; (2) SNR per radar; (3) ALL R + J detection probabilities side by side
        // (det_prob_batch); (4) the deception draws in jammer order; (5) detection draws, FSM, reward terms in radar
        // order.  Same arithmetic, operation order and RNG slots as the reference's interleaved loops; the deception
        // quantities of a jammer that is not deceiving are computed on zeros and never used.
        constexpr int NP = PRE ? NR + NJ : 1;
        double supp[NR];   // environment.py:241
        double prod[NR];   // environment.py:443-447
#pragma unroll
        for (int r = 0; r < NR; ++r) { supp[r] = 0.0; prod[r] = 1.0; }
        const int col = SCAT ? (int)threadIdx.x : 0;
        if (SCAT) {
#pragma unroll
            for (int r = 0; r < NR; ++r) { s_supp[r][col] = 0.0; s_prod[r][col] = 1.0; }
        }
        uint32_t supp_mask = 0;  // environment.py:391-394 (set of suppressed radars)
        uint32_t hit_mask = 0;   // radars with >= 1 detected false target
        int n_dec = 0;           // valid deception actions so far (RNG slot R + k)
        double r_p = 0.0;        // environment.py:371-378
        double snr_all[NP], pd_all[NP];   // [0, NR): radars, [NR, NR + NJ): false targets of deceiving jammers
        int dec_tgt[NJ];                  // target radar of jammer j's valid deception action, -1 = none

MACJD_ENV_UNROLL_SIZED(NJ)
        for (int j = 0; j < NJ; ++j) {
            if (!JT && j >= J) break;
            // ---- action decode, environment.py:249-268 ----
            const int32_t T = at(io.T, e, io.T_se, j, io.T_sx, act_extra);
            const bool is_jamming = (T >= 1) && (T <= 2 * R);
            const int target = is_jamming ? ((T + 1) / 2 - 1) : 0;
            const int jtype = T % 2;  // 1 = suppression, 0 = deception (only read when is_jamming)

            // ---- power scale + r_p term, environment.py:271-277 ----
            const double pmin = t_pmin(j), pmax = t_pmax(j);
            const double power_range = pmax - pmin;
            double actual_d, norm;
            float actual_f = 0.0f;
            if (arith32) {
                float Pc = at(io.P32, e, io.P_se, j, io.P_sx, act_extra);
                Pc = Pc < 0.0f ? 0.0f : (Pc > 1.0f ? 1.0f : Pc);  // np.clip, NaN propagates
                actual_f = (float)pmin + Pc * (float)power_range;
                actual_d = (double)actual_f;
                if (REG)
                    norm = (power_range > 1e-6) ? (double)(float)div_by_refined((double)(actual_f - (float)pmin), tb->range_fd[j],
                                                                                tb->r_range[j]) : 0.0;
                else
                    norm = (power_range > 1e-6) ? (double)((actual_f - (float)pmin) / (float)power_range) : 0.0;
            } else {
                double Pc = io.P64 ? io.P64[e * io.P_se + (int64_t)j * io.P_sx]
                                   : (double)at(io.P32, e, io.P_se, j, io.P_sx, act_extra);
                Pc = Pc < 0.0 ? 0.0 : (Pc > 1.0 ? 1.0 : Pc);
                actual_d = pmin + Pc * power_range;
                norm = (power_range > 1e-6) ? (actual_d - pmin) / power_range : 0.0;
            }
            r_p += rp_max + (rp_min - rp_max) * norm;  // environment.py:377-378

            // ---- received jamming power, environment.py:280-302, jammer.py:56-98 ----
            const double denom = g_denom(j, target);
            const bool recorded = REG ? (is_jamming && (actual_d > 0.0) && (g_flags(j, target) & JR_RECORDABLE))
                                      : (is_jamming && (actual_d > 0.0) && (denom >= 0.0));
            double prj = 0.0;
            if (REG) {
                // `denom` is the divisor as the reference uses it here (1.0 where it does not divide)
                const uint8_t fl = g_flags(j, target);
                const bool live = recorded && (fl & JR_LIVE);
                const float num = (actual_f * (float)t_gj(j)) * (float)(SCAN ? scan_gr(j, target) : g_gr(j, target));
                const double q64 = div_by_refined((double)num, denom, s_rsel[j * R + target]);
                const double q = (fl & MACJD_JR_WEAK_DENOM) ? (double)(float)q64 : q64;
                prj = (live && q > 0.0) ? q : 0.0;  // Python max(0.0, x)
            } else if (PRE) {
                // branch-free: the quotient is evaluated on a harmless divisor where the reference does not divide
                const bool live = recorded && denom > 1e-18;
                const double dsafe = live ? denom : 1.0;
                const double grj = SCAN ? scan_gr(j, target) : g_gr(j, target);
                double q;
                if (arith32) {
                    const float num = (actual_f * (float)t_gj(j)) * (float)grj;
                    q = (g_flags(j, target) & MACJD_JR_WEAK_DENOM) ? (double)(num / (float)dsafe) : (double)num / dsafe;
                } else {
                    q = (actual_d * t_gj(j) * grj) / dsafe;
                }
                prj = (live && q > 0.0) ? q : 0.0;  // Python max(0.0, x)
            } else if (recorded && denom > 1e-18) {
                const double grj = SCAN ? scan_gr(j, target) : g_gr(j, target);
                if (arith32) {
                    const float num = (actual_f * (float)t_gj(j)) * (float)grj;
                    prj = (g_flags(j, target) & MACJD_JR_WEAK_DENOM) ? (double)(num / (float)denom)
                                                                         : (double)num / denom;
                } else {
                    prj = (actual_d * t_gj(j) * grj) / denom;
                }
                prj = (prj > 0.0) ? prj : 0.0;  // Python max(0.0, x)
            }
            if (!FAST && io.prj64) io.prj64[e * J + j] = recorded ? prj : -1.0;

            const bool is_sup = recorded && (jtype == 1);
            const bool is_dec = recorded && (jtype == 0);
            supp_mask |= is_sup ? (1u << target) : 0u;
            if (SCAT) {                    // environment.py:299
                const int row = is_sup ? target : NR;
                s_supp[row][col] = s_supp[row][col] + prj;
            } else {
#pragma unroll
                for (int r = 0; r < NR; ++r)   // fma(prj, 1 or 0, supp) == supp + prj or supp, bit for bit
                    supp[r] = PRE ? __builtin_fma(prj, (is_sup && target == r) ? 1.0 : 0.0, supp[r])
                                  : supp[r] + ((is_sup && target == r) ? prj : 0.0);
            }
            dec_tgt[j] = is_dec ? target : -1;

            // ---- deception: SNR of the false target, environment.py:410-422 ----
            if (REG) {
                const double snr_f = div_by_refined(g_D(j, target) * prj, g_Pn(j, target), s_rPn[target]);
                snr_all[NR + j] = (is_dec && snr_f > 0.0) ? snr_f : 0.0;
            } else if (PRE) {
                const double Pn_t = g_Pn(j, target);
                const bool live = is_dec && Pn_t > 1e-18;
                const double snr_f = (g_D(j, target) * prj) / (live ? Pn_t : 1.0);
                snr_all[NR + j] = (live && snr_f > 0.0) ? snr_f : 0.0;
            } else if (is_dec) {   // generic sizes: one evaluation at a time, only where needed
                const double Pn_t = g_Pn(j, target);
                double snr_f = (Pn_t > 1e-18) ? (g_D(j, target) * prj) / Pn_t : 0.0;
                snr_f = (snr_f > 0.0) ? snr_f : 0.0;
                const double pd_f = det_prob(snr_f, pdk);
                const double u = draw_uniform<FAST>(io, e, episode, R + n_dec, (uint32_t)step_before);
                ++n_dec;
                if (u <= pd_f) {
                    const double safe = pd_f < 0.999999 ? pd_f : 0.999999;  // environment.py:446
                    hit_mask |= (1u << target);
#pragma unroll
                    for (int r = 0; r < NR; ++r) prod[r] = (target == r) ? prod[r] * (1.0 - safe) : prod[r];
                }
            }
        }

        // ---- SNR with jamming, environment.py:316-333 ----
        double snr_w[NR];
        float snr32r[PD32 ? NR : 1];
MACJD_ENV_UNROLL_SIZED(NR)
        for (int r = 0; r < NR; ++r) {
            if (!RT && r >= R) break;
            const double Pn = t_Pn(r);
            const double den = t_D(r) * (SCAT ? s_supp[r][col] : supp[r]) + Pn;   // :331
            if (PD32) {                                                      // float32 quotient (see det_prob32)
                snr32r[PD32 ? r : 0] = (float)r_GaPs(r) * __builtin_amdgcn_rcpf((float)den);
                snr_w[r] = 0.0;   // (not formed; the outputs below take the float32 value)
            } else if (REG) {                                                // den >= Pn > 1e-18
                snr_w[r] = div_by_refined(r_GaPs(r), den, rcp_refined(den));
                snr_all[r] = snr_w[r];
            } else if (PRE) {
                const bool live = den > 1e-18;
                const double q = r_GaPs(r) / (live ? den : 1.0);
                snr_w[r] = live ? q : 0.0;                                   // :332
                snr_all[r] = snr_w[r];
            } else {
                snr_w[r] = (den > 1e-18) ? r_GaPs(r) / den : 0.0;            // :332
            }
        }
        // PD32: all R + J compares u <= pd decided here — by the float32 value where the two sides are further apart than
        // its error bound, by ONE shared copy of the exact float64 chain (a rarely taken loop) for the others
        uint32_t le_bits = 0;
        float pd32f[PD32 ? NP : 1];   // (kept as float32 until used: 7 registers instead of 14)
        auto pd_at = [&](int i) -> double { return PD32 ? (double)pd32f[PD32 ? i : 0] : pd_all[i]; };
        if constexpr (PD32) {
            uint32_t w_all[NP];
#pragma unroll
            for (int r = 0; r < NR; ++r) w_all[r] = rw[r];
            {
                int nd = 0;   // RNG slot of jammer j's valid deception action: R + (valid deception actions before it)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    uint32_t w = rw[NR];
#pragma unroll
                    for (int k = 1; k < NJ; ++k) w = (nd == k) ? rw[NR + k] : w;
                    w_all[NR + j] = w;
                    nd += (dec_tgt[j] >= 0) ? 1 : 0;
                }
            }
            uint32_t close_bits = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const float p32 = det_prob32(i < NR ? snr32r[PD32 && i < NR ? i : 0] : (float)snr_all[i], pdk32);
                pd32f[i] = p32;
                const float d = __builtin_fmaf((float)w_all[i], 0x1p-32f, 0x1p-33f) - p32;
                const bool need = (i < NR) || (dec_tgt[i < NR ? 0 : i - NR] >= 0);
                le_bits |= (d <= 0.0f) ? (1u << i) : 0u;
                close_bits |= (need && fabsf(d) <= PD32_BOUND) ? (1u << i) : 0u;
            }
            if (close_bits) {
#pragma unroll 1
                for (int i = 0; i < NP; ++i) {
                    if (!((close_bits >> i) & 1u)) continue;
                    double snr_i = snr_all[NR];
                    uint32_t w_i = w_all[0];
#pragma unroll
                    for (int k = 1; k < NP; ++k) {
                        if (k > NR) snr_i = (i == k) ? snr_all[k] : snr_i;
                        w_i = (i == k) ? w_all[k] : w_i;
                    }
                    if (i < NR) {   // a radar: the exact SNR from the suppression sum (still in this lane's LDS column)
                        const double den_i = tb->D[i] * s_supp[SCAT ? i : 0][col] + tb->Pn[i];
                        const double gaps_i = PAT ? s_lGaPs[pl.lv(i) * R + i]
                                                  : SCAN ? (((in_t >> i) & 1u) ? tb->GaPs[i] : tb->GaPs_side[i]) : tb->GaPs[i];
                        snr_i = div_by_refined(gaps_i, den_i, rcp_refined(den_i));
                    }
                    double p;
                    det_prob_batch_regular<1>(&snr_i, &p, pdk);
                    le_bits = (u32_mid(w_i) <= p) ? (le_bits | (1u << i)) : (le_bits & ~(1u << i));
                }
            }
        } else if (REG) det_prob_batch_regular<NP>(snr_all, pd_all, pdk);    // :337, :425
        else if (PRE) det_prob_batch<NP>(snr_all, pd_all, pdk);

        // ---- deception: Monte-Carlo detection of the false targets in jammer order, environment.py:425-447 ----
        if (PRE) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const bool is_dec = dec_tgt[j] >= 0;
                double u = 2.0;
                uint32_t w = 0;
                if (own_rng) {
                    w = rw[NR];
#pragma unroll
                    for (int k = 1; k < NJ; ++k) w = (n_dec == k) ? rw[NR + k] : w;
                    if (!PD32) u = u32_mid(w);
                } else {
                    u = is_dec ? io.u[e * io.u_se + (int64_t)(R + n_dec) * io.u_sx] : 2.0;
                }
                n_dec += is_dec ? 1 : 0;
                const double pd_f = pd_at(NR + j);
                const bool hit = PD32 ? (is_dec && ((le_bits >> (NR + j)) & 1u))
                                      : (is_dec && (u <= pd_f));             // :430-434
                const double safe = pd_f < 0.999999 ? pd_f : 0.999999;      // :446
                hit_mask |= hit ? (1u << dec_tgt[j]) : 0u;
                if (SCAT) {
                    const int row = hit ? dec_tgt[j] : NR;
                    s_prod[row][col] = s_prod[row][col] * (1.0 - safe);
                } else {
#pragma unroll
                    for (int r = 0; r < NR; ++r) prod[r] = (hit && dec_tgt[j] == r) ? prod[r] * (1.0 - safe) : prod[r];
                }
            }
        }

        // ---- detections, FSM, r_d, r_j(suppression); environment.py:337-398 ----
        double r_d = 0.0, r_j = 0.0, r_j_dec = 0.0;
        double pd_r[NR];
        uint32_t track_bits = 0;
MACJD_ENV_UNROLL_SIZED(NR)
        for (int r = 0; r < NR; ++r) {
            if (!RT && r >= R) break;
            const double pd = PRE ? pd_at(r) : det_prob(snr_w[r], pdk);     // :337
            bool detected;
            if constexpr (PD32) {
                detected = (le_bits >> r) & 1u;                                // :341
            } else {
                const double u = (PRE && own_rng) ? u32_mid(rw[r]) : draw_uniform<FAST>(io, e, episode, r, (uint32_t)step_before);
                detected = (u <= pd);                                          // :341
            }
            // radar.py:102-117: SEARCH & detected -> TRACK, SEARCH & !detected -> SEARCH,
            // TRACK & !detected -> SEARCH, TRACK & detected -> TRACK.  The next state therefore
            // equals `detected` whatever the previous state was, so the previous state is never
            // read (saves R bytes of HBM reads per env-step); `track` is write-only here.
            const bool tracking = detected;
            track_bits |= tracking ? (1u << r) : 0u;
            r_d += tracking ? t_rdpen(r) : 0.0;                             // :359-366 (post-update state)
            const double red = r_pdno(r) - pd;                               // :396-398
            r_j += ((supp_mask & (1u << r)) && red > 0.0) ? red : 0.0;
            r_j_dec += (hit_mask & (1u << r)) ? 1.0 - (SCAT ? s_prod[r][col] : prod[r]) : 0.0;   // :438-451
            pd_r[r] = pd;
        }
        // per-radar outputs (the only conditional code of the pass: kept behind the arithmetic)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (!RT && r >= R) break;
            const double snr_rep = PD32 ? (double)snr32r[PD32 ? r : 0]
                                        : ((REG || snr_w[r] > 0.0) ? snr_w[r] : 0.0);  // :333 (regular: never negative)
            if (last_t) at(io.track, e, io.k_se, r, io.k_sx) = (track_bits >> r) & 1u;
            if (io.pd) at(io.pd, e, io.pd_se, r, io.pd_sx) = (float)pd_r[r];
            if (io.snr_with) at(io.snr_with, e, io.sw_se, r, io.sw_sx) = (float)snr_rep;
            if (!FAST && io.pd64) io.pd64[e * R + r] = pd_r[r];
            if (!FAST && io.snr64) io.snr64[e * R + r] = snr_rep;
            if constexpr (SCAN) {   // beam advance (include/macjd.h, macjd_scan_desc)
                const bool in = (in_t >> r) & 1u;
                if constexpr (SPP) {
                    if (io.snr_no)
                        at(io.snr_no, e, io.sn_se, r, io.sn_sx) =
                            (float)(PHOIST ? lv_snrno[PHOIST ? r : 0] : pp_row(PP_SNR_NO, pl.lv(r), r));
                } else if constexpr (PAT) {
                    if (io.snr_no) at(io.snr_no, e, io.sn_se, r, io.sn_sx) = (float)s_lsnrno[pl.lv(r) * R + r];
                } else if constexpr (SPE) {
                    if (io.snr_no)
                        at(io.snr_no, e, io.sn_se, r, io.sn_sx) =
                            (float)(SHOIST ? sv_snrno[SHOIST ? r : 0] : sp[(int64_t)((in ? SP_SNR_NO : SP_SNR_NO_SIDE) * R + r) * sps]);
                } else {
                    if (io.snr_no) at(io.snr_no, e, io.sn_se, r, io.sn_sx) = (float)(in ? tb->snr_no[r] : tb->snr_no_side[r]);
                }
                const double a = PRE ? az[PRE ? r : 0] : at(io.theta_a, e, io.a_se, r, io.a_sx);
                double x = a + (SPE ? c_swm(r) : tb->swm[r]);
                x = (x >= 360.0) ? x - 360.0 : x;
                const double a1 = ((track_bits >> r) & 1u) ? (SPE ? c_bt(r) : tb->bt[r]) : (((s_bits >> r) & 1u) ? a : x);
                at(io.theta_a, e, io.a_se, r, io.a_sx) = a1;
                if (io.state) at(io.state, e, io.st_se, io.st_col0 + r * io.st_col_step, 1) = (float)a1;
            }
        }
        r_j += r_j_dec;                          // :454
        const double reward = r_d + r_p + r_j;  // :457

        if (!many) at(io.step, e, 1, 0, 0) = step_count;   // many-step: advanced by env_advance_kernel afterwards
        if (io.terminated) at(io.terminated, e_item, 1, 0, 0) = (step_count >= episode_limit) ? 1 : 0;  // :460
        if (io.reward) at(io.reward, e_item, 1, 0, 0) = (float)reward;
        if (io.r_dpj) {
            at(io.r_dpj, e_item, 3, 0, 1) = (float)r_d;
            at(io.r_dpj, e_item, 3, 1, 1) = (float)r_p;
            at(io.r_dpj, e_item, 3, 2, 1) = (float)r_j;
        }
        if (io.r_dpj_sum && !many) {   // many-step: summed over the steps by env_advance_kernel
            at(io.r_dpj_sum, e, 3, 0, 1) += (float)r_d;
            at(io.r_dpj_sum, e, 3, 1, 1) += (float)r_p;
            at(io.r_dpj_sum, e, 3, 2, 1) += (float)r_j;
        }
        if (!FAST && io.out64) {
            io.out64[e * 4 + 0] = reward;
            io.out64[e * 4 + 1] = r_d;
            io.out64[e * 4 + 2] = r_p;
            io.out64[e * 4 + 3] = r_j;
        }
        if constexpr (MOV) {
            // the entities move: frame min(step_count, n_frames)'s positions into this env's state row (the last item of a
            // many-step launch only: rows end as after the last step); the columns are wave-uniform (scalar loads)
            if (last_t) {
                int32_t fn = step_count < io.n_frames ? step_count : io.n_frames;
                fn = fn > 0 ? fn : 0;
                const float* __restrict__ pos;
                if constexpr (MVPE) pos = io.positions + ((mv_env_tile * (io.n_frames + 1) + fn) * io.n_pos) * mv_ps + mv_col;
                else pos = io.positions + (int64_t)fn * io.n_pos;
                float* mv_rows;   // (a scanning launch's `state` is the beam block's: optional, theta_a columns)
                if constexpr (SCAN) mv_rows = io.mv_state; else mv_rows = io.state;
                constexpr int NPOS = 2 * (NR + NJ);
                if constexpr (PRE) {
#pragma unroll
                    for (int i = 0; i < NPOS; ++i) at(mv_rows, e, io.mv_st_se, io.position_columns[i], 1) = pos[MVPE ? i * mv_ps : i];
                } else {
                    for (int i = 0; i < io.n_pos; ++i) at(mv_rows, e, io.mv_st_se, io.position_columns[i], 1) = pos[MVPE ? i * mv_ps : i];
                }
            }
            if (io.mv_snr_no && !many) {
MACJD_ENV_UNROLL_SIZED(NR)
                for (int r = 0; r < NR; ++r) {
                    if (!RT && r >= R) break;
                    if constexpr (MVPE)
                        at(io.mv_snr_no, e, io.mv_sn_se, r, io.mv_sn_sx) = (float)io.frame_snr_no[(mv_tile_idx * R + r) * mv_ps + mv_col];
                    else
                        at(io.mv_snr_no, e, io.mv_sn_se, r, io.mv_sn_sx) = (float)io.frame_snr_no[(int64_t)mv_frame * R + r];
                }
            }
        }
    };
    if constexpr (FAST) {
        // one env per lane, no grid-stride loop: inside a loop every argument and table constant is loop-invariant,
        // gets hoisted and stays live for the whole body (SGPR spills); straight-line code loads them where used
        const uint32_t env = blockIdx.x * blockDim.x + threadIdx.x;   // (the host checks that every offset fits 32 bits)
        if ((int64_t)env < io.n_envs) env_step_one((int64_t)env, (int32_t)blockIdx.y);   // (blockIdx.y = step of a many-step launch)
    } else {
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < io.n_envs;
             e += (int64_t)gridDim.x * blockDim.x)
            env_step_one(e, 0);
    }
}

// macjd_env_scan_pe.hip: the generic-size SCAN kernel on per-env tables, env_step_kernel<0, 0, PE = true, FAST = false, ...,
// SCAN = true>, built there with its size-bounded loops unrolled by count (see MACJD_ENV_UNROLL_SIZED)
void launch_scan_pe_generic(dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const ScanPeStepIO<macjd_step_io>& io);
// ... and its PAT form (ScanPePatStepIO), built there with the same unrolling
void launch_scan_pe_generic(dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const ScanPePatStepIO<macjd_step_io>& io);

// The moving launches (MOV instantiations, IO = Motion*StepIO<...>) live in four translation units of their own:
// macjd_env_motion.hip (shared frames), macjd_env_motion_pe.hip (per-env frames), macjd_env_motion_scan.hip (shared frames
// under scanning radars, with and without PAT) and macjd_env_motion_scan_pe.hip (per-env frames under scanning radars).
// They share the launcher below and ONE list of compiled sizes.

// A compiled (J, R) size as two std::integral_constants: what the size switches hand to their callable
template <int N>
using CompiledDim = std::integral_constant<int, N>;

// The compiled moving sizes: fn(JT, RT) runs at the size's constants; false (fn not called) for every other size
template <class F>
static bool with_motion_size(int J, int R, F&& fn) {
    if (J == 3 && R == 4) fn(CompiledDim<3>{}, CompiledDim<4>{});
    else if (J == 6 && R == 8) fn(CompiledDim<6>{}, CompiledDim<8>{});
    else if (J == 2 && R == 2) fn(CompiledDim<2>{}, CompiledDim<2>{});
    else return false;
    return true;
}
inline bool motion_size_compiled(int J, int R) { return with_motion_size(J, R, [](auto, auto) {}); }

template <int JT, int RT, bool PE, bool FAST, bool SCAN, bool PAT, class IO>
static void launch(dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const IO& io) {
    hipLaunchKernelGGL((env_step_kernel<JT, RT, PE, FAST, IO, false, false, SCAN, PAT>), grid, block, 0, stream, dev, io);
}

// Body of a unit's launch_motion overloads: the kernel of the compiled size; at every other size the production forms
// (FAST) launch nothing and return false, the general forms run the generic-size kernel.  The instantiations belong to the
// unit that calls this (its MACJD_ENV_UNROLL_SIZED).
template <bool FAST, bool SCAN, bool PAT, class IO>
static bool launch_motion_sized(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const IO& io) {
    const bool sized = with_motion_size(J, R, [&](auto jt, auto rt) {
        launch<decltype(jt)::value, decltype(rt)::value, true, FAST, SCAN, PAT>(grid, block, stream, dev, io);
    });
    if constexpr (!FAST)
        if (!sized) launch<0, 0, true, false, SCAN, PAT>(grid, block, stream, dev, io);
    return sized || !FAST;
}

// One overload per argument-block type, each defined in the unit that holds the type's kernels.  Returns whether a launch
// was issued.  The macro is the signature, for the declarations here and the definitions there.
#define MACJD_LAUNCH_MOTION(IO) \
    bool launch_motion(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const IO& io)
MACJD_LAUNCH_MOTION(MotionStepIO<FastStepIO>);                                // macjd_env_motion.hip
MACJD_LAUNCH_MOTION(MotionStepIO<macjd_step_io>);
MACJD_LAUNCH_MOTION(MotionPeStepIO<FastStepIO>);                              // macjd_env_motion_pe.hip
MACJD_LAUNCH_MOTION(MotionPeStepIO<macjd_step_io>);
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPeStepIO<FastStepIO>>);              // macjd_env_motion_scan.hip
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPeStepIO<macjd_step_io>>);
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPePatStepIO<FastStepIO>>);
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPePatStepIO<macjd_step_io>>);
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPeStepIO<FastStepIO>>);            // macjd_env_motion_scan_pe.hip
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPeStepIO<macjd_step_io>>);
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPePatStepIO<FastStepIO>>);
MACJD_LAUNCH_MOTION(MotionScanPeStepIO<ScanPePatStepIO<macjd_step_io>>);

// the resets of the moving modes: the position part (shared / per-env frames) and the beam part on per-env beam frames
void launch_motion_reset(dim3 grid, dim3 block, hipStream_t stream, int64_t n_envs, int n_pos, const float* positions,
                         const int32_t* position_columns, float* state, int64_t st_se, const uint8_t* mask);
void launch_motion_pe_reset(dim3 grid, dim3 block, hipStream_t stream, int64_t n_envs, int n_pos, int n_frames, int tile,
                            const float* positions, const int32_t* position_columns, float* state, int64_t st_se,
                            const uint8_t* mask);
void launch_motion_scan_pe_reset(dim3 grid, dim3 block, hipStream_t stream, int64_t n_envs, int R, int J, int n_frames, int tile,
                                 const double* scan_frames, double* theta_a, int64_t a_se, int64_t a_sx, float* state,
                                 int64_t st_se, int32_t st_col0, int32_t st_col_step, const uint8_t* mask);

}  // namespace macjd
