// macjd_episode_scan.h — closed-loop episode launch for scanning radars (included by macjd_episode.hip; C-ABI:
// include/macjd_nets.h, macjd_agent_env_episode_scan_io): agent step, scanning env step and next observation for all T
// steps of 16 environments per workgroup, without leaving the kernel.
//
// With scanning beams the observation's theta_a columns change every step, and through the FSM they depend on what the
// agents did, so agent_episode_kernel's premise (nothing the agent computes depends on the env's outputs) is gone.  What
// still holds is that environments are independent of each other: the workgroup that owns 16 envs owns everything their
// episodes need.
//
// Mapping (J agents, R radars, H = 64, actor hidden 128, A actions; 256 threads = 4 waves, as agent_episode_kernel):
//   * resident MFMA B fragments per wave w: W_hh and W_ih rows of hidden units [16w, 16w+16) of all three gates (2 x 48
//     VGPRs) and the Q-head's h-columns (16); actor layer 2 (128 x 128) is staged in LDS once per launch and wave w reads
//     its output columns [32w, 32w+32) as fragments — nothing is fetched from global memory inside the step loop;
//   * every agent of an env sees the same state vector, so the observation-only work is ONE 16-row tile per workgroup,
//     shared by the J agent tiles: the 16 observation rows live in LDS (static columns filled once per launch, the R
//     theta_a columns rewritten by the env half), and fc1 / the actor's first layer are full S-column MFMA products in
//     mlp_forward_kernel's k order with resident fragments (3 x 12 VGPRs) — the incremental form (static part + sum_r
//     W[:, col_r] theta_a[r]) was tried first and moved h by 2e-5 against the step-by-step path (theta_a reaches 360, an
//     ulp of these sums is 1.5e-5), outside the project's 1e-5 bar;
//   * per step: (S1) theta_a columns of this step's staging rows; x = ReLU(fc1) and the actor's first layer -> LDS;
//     (S2) gi = W_ih x + b_ih and actor layer 2 on MFMA, then gh, gates, h_t exactly as agent_episode_kernel; (S3) actor
//     layer 3 + sigmoid (16 A dot products of 128 on the VALU) -> P in LDS, Q-head base on MFMA; (S4) all-action Q-head,
//     mask, arg-max, epsilon-greedy (wave = agent tile) -> chosen actions to the staging rows and to LDS; (S5) the
//     scanning env step of the 16 envs, one lane per env (lanes 0..15 of wave 0), general all-float64 expressions of
//     env_step_kernel<.., SCAN> with the shared device helpers of macjd_env_dev.h; azimuths (f64), FSM bits, step counter
//     and the reward-component sums stay in that lane's registers, the float32 azimuths go to LDS for step t + 1.
//   Five barriers per step.  The env's tables are copied into LDS once per launch (uniform ds_read instead of ~100 SGPRs
//   of loop-invariant scalars).
//
// Stepped antenna pattern (include/macjd.h, macjd_scan_pattern_desc): PAT, the kernel's last template parameter, selects
// the variant that is launched for a handle that carries pattern tables.  Its env half takes a level per object from
// beam_level and reads the [L + 2, R] level tables (GaPs, pd_no, gr) from a second LDS block; the target's levels of the
// last step are kept four bits per radar for the hand-over's snr_no.  (The two variants were first compiled from one text
// included twice under two names, so that the variant without a pattern kept its name; the parameter changes only the
// name: both variants compile to the same code either way, profiles/r10_episode_isa_check.txt.)
//
// Per-env scenario batches (include/macjd_nets.h, macjd_agent_env_episode_scan_pe_io): PE, the next template parameter,
// with the argument block EpScanPeIO — the same kernel with every table read taken from the env's own column (see the
// comment on the kernel).  Again only the names of the existing variants change, profiles/r18_episode_isa_check.txt.
//
// Moving scenarios under scanning radars (include/macjd_nets.h, macjd_agent_env_episode_moving_scan_io): the PE variant
// launched with the argument block EpScanMovIO (MOV below, deduced from the block's type so that the existing variants keep
// their names) — the env's column is frame f = min(step counter, F - 1) of the frame tables, staged again every step, and
// the observation's position columns follow positions[min(step counter, F)] (see the comment on the kernel).
//
// Per-env moving scenarios under scanning radars (include/macjd_nets.h, macjd_agent_env_episode_moving_scan_pe_io): the MOV
// variant launched with the argument block EpScanMovPeIO (MVP below, deduced from the block's type again) — every frame
// read is taken from the env's own column of the tiled per-env frame tables (include/macjd.h, macjd_motion_pe_io /
// macjd_motion_scan_pe_io).  The twelve earlier variants keep their names and code,
// profiles/episode_moving_scan_pe_isa_check.txt.
#pragma once

#include <type_traits>

#include "macjd_env_dev.h"

namespace macjd {

constexpr int ES_AH = 128;            // actor hidden width
constexpr int ES_ALD = ES_AH + 8;     // LDS pitch of the actor's activations (= 8 mod 16 floats)
constexpr int ES_AKQ = ES_AH / 16;    // quads of a K = 128 product

template <int J, int R>
struct EpScanTab {   // LDS copy of what the env half reads from the scenario handle
    double rp_min, rp_max, pd_A, pd_c1, pd_denB;
    double GaPs[R], GaPs_side[R], Pn[R], D[R], pd_no[R], pd_no_side[R], rd_pen[R], gr[R], gr_side[R];
    double half[R], h2[R], sweep[R], swm[R], bt[R], snr_no[R], snr_no_side[R];
    double pmin[J], pmax[J], gj[J];
    double denom[J * R], bj[J * R];
    int32_t episode_limit;
    uint8_t flags[J * R], full[R];
};

// PE: what the handle still supplies when every env brings its own tables
struct EpScanConsts {
    double rp_min, rp_max, pd_A, pd_c1, pd_denB;
    int32_t episode_limit;
};

// Argument block of the launch on per-env scenario tables (include/macjd_nets.h, macjd_agent_env_episode_scan_pe_io): the
// shared launch's block, whose pe_tables are the batch's scenario tables here, plus the flag bytes, the per-env scan SoA
// and, under a stepped pattern, the per-env level tables — all laid out by pe_tile (include/macjd.h, macjd_step_io).
struct EpScanPeIO : macjd_agent_env_episode_scan_io {
    const uint8_t* pe_flags;
    int64_t pe_stride;
    const double* sp_tables;
    int64_t sp_stride;
    const double* pp_tables;
    int64_t pp_stride;
    int32_t pe_tile, pat_levels;
};

// Argument block of the launch on a moving scanning scenario (include/macjd_nets.h, macjd_agent_env_episode_moving_scan_io):
// the shared launch's block plus the frame tables of macjd_motion_io / macjd_motion_scan_io (frame-major: the tiled per-env
// layout at tile width 1 with the frame index as the tile index).
struct EpScanMovIO : macjd_agent_env_episode_scan_io {
    const double* frames;
    const uint8_t* frame_flags;
    const double* scan_frames;
    const double* pattern_frames;
    const float* positions;
    const int32_t* position_columns;
    int32_t n_frames, pat_levels;
};

// Argument block of the launch on a per-env moving scanning scenario batch (include/macjd_nets.h,
// macjd_agent_env_episode_moving_scan_pe_io): EpScanMovIO's members, the tables in the tiled per-env frame layout of
// macjd_motion_pe_io / macjd_motion_scan_pe_io (row t of frame f of env e at
// table[(((e / tile) * F + f) * ROWS + t) * tile + e % tile]; positions with F + 1 frames per tile), and the tile width.
struct EpScanMovPeIO : macjd_agent_env_episode_scan_io {
    const double* frames;
    const uint8_t* frame_flags;
    const double* scan_frames;
    const double* pattern_frames;
    const float* positions;
    const int32_t* position_columns;
    int32_t n_frames, pat_levels, tile;
};

// Rows of the per-env LDS block [row][16] of the PE variants (lane er reads [row * 16 + er]): the env's pe_tables rows in
// their own order, then the scan rows the step reads, then (PAT) inv_width.
template <int J, int R>
struct EpScanPeRows {
    enum {
        GAPS = 0, PN = R, D = 2 * R, PD_NO = 3 * R, RD_PEN = 4 * R, GR = 5 * R, PMIN = 6 * R, PMAX = 6 * R + J, GJ = 6 * R + 2 * J,
        DENOM = 6 * R + 3 * J, NPE = 6 * R + 3 * J + J * R,
        HALF = NPE, SWEEP = NPE + R, SWM = NPE + 2 * R, BT = NPE + 3 * R, GAPS_SIDE = NPE + 4 * R, PD_NO_SIDE = NPE + 5 * R,
        GR_SIDE = NPE + 6 * R, BJ = NPE + 7 * R, NSCAN = 7 * R + J * R, INVW = NPE + NSCAN,
        NSP = 10 * R + J * R   // rows of macjd_scan_pe_io
    };
    // source row in macjd_scan_pe_io of staged scan row k: half | sweep | sweep_mod | (az0) | bear_tgt | GaPs_side | (snr_no) |
    // (snr_no_side) | pd_no_side | gr_side | bear_jam — the rows in brackets are not staged
    static __device__ __forceinline__ int sp_src(int k) {
        const int b = k / R;
        return k < 7 * R ? (b < 3 ? b : (b < 5 ? b + 1 : b + 3)) * R + (k - b * R) : 10 * R + (k - 7 * R);
    }
};

// PE (with IO = EpScanPeIO): every env reads its own tables.  The loop-invariant rows of the workgroup's 16 envs are staged
// once per launch into an LDS block [row][16] of float64 (13R + 3J + 2JR rows, + R under a pattern) and lane er of the env
// half reads column er — sixteen consecutive doubles, conflict-free also when the row is picked per lane by the chosen
// radar; h2 and full are formed per lane as env_step_kernel<.., SCAN && PE> does.  Under a pattern the level tables stay in
// HBM (96 rows at L = 6 do not fit beside the rest): the one row an object's level selects is loaded from the env's
// column by address, 2R + J loads per lane and step, as env_step_kernel<.., PAT && PE> does.  The handle supplies only the
// r_p bounds, the Pd constants and episode_limit.  The agent half (S1-S4), keying and barriers are the shared kernel's.
//
// MOV (IO = EpScanMovIO, PE = true): env e runs step t on frame f = min(step0[e] + t, F - 1), step0 = io.step[e] at entry, so
// one workgroup may hold envs on different frames.  The [row][16] block and the flag bytes are rewritten in place by all
// 256 threads at the top of every step (thread -> column tid & 15, whose step0 the thread holds already): the block is
// read only in S5 by wave 0, the barrier that closes S5 of step t - 1 precedes the writes and the barriers of S1 - S4
// precede the reads, so the step keeps its five barriers.  The level rows under a pattern and the hand-over's snr_no row
// are loaded by address from frame f's row of pattern_frames / scan_frames.  The observation's n_pos = 2R + 2J position
// columns: waves 1 - 3, idle during S5, copy positions[min(step0 + t + 1, F)] into the LDS observation tile for step t + 1
// (wave 0 writes the theta_a columns there: disjoint columns), S1 copies them from the tile into the staging rows next to
// the theta_a columns, and the env lane leaves positions[min(step0 + T, F)] in the env's state row at exit.
//
// MVP (IO = EpScanMovPeIO; MOV's code with other addresses): every frame table is per env in the tiled layout.  Thread tid
// owns env column tid & 15 in every role that reads a table (staging, position columns, env lane), so the tile arithmetic
// (e / tile, e % tile) is done once per launch: the thread keeps its env's tile index and its lane in the tile, and inside
// the loop only the frame index changes.  Any tile width >= 1: the 16 envs of a workgroup may span several tiles; rows past
// E use env E - 1's column, so the last tile's padding lanes are never read.  With tile % 16 == 0 the 16 envs of a row are
// 128 contiguous bytes.
template <int J, int R, int A, int SQ, bool PAT, bool PE = false, class IO = macjd_agent_env_episode_scan_io>
__global__ void __launch_bounds__(256) agent_env_episode_scan_kernel(const DevTables* __restrict__ tb, const IO io) {
    static_assert(J <= 4, "one wave per agent tile in the Q-head phase");
    constexpr bool MVP = std::is_same_v<IO, EpScanMovPeIO>;   // MOV on per-env frame tables
    constexpr bool MOV = std::is_same_v<IO, EpScanMovIO> || MVP;
    static_assert(PE == (std::is_same_v<IO, EpScanPeIO> || MOV), "PE: the argument block with the per-env tables");
    constexpr int NPOS = 2 * R + 2 * J;   // MOV: position columns of a state row
    static_assert(!PAT || R <= 8, "PAT: the target's levels are packed four bits per radar into 32 bits");
    static_assert(16 * A <= 256, "actor layer 3: one thread per (env, action)");
    constexpr int OLD = 16 * SQ + 8;   // LDS pitch of the observation tile (S <= 16 SQ columns, zero-padded)
    __shared__ __attribute__((aligned(16))) float Hl[2][J][16 * EP_LD];   // h_{t-1} / h_t, ping-pong
    __shared__ __attribute__((aligned(16))) float Bl[J][16 * EP_LD];      // Q-head base of the current step
    __shared__ float Wq[(A + 2) * EP_H];                                  // Q-head columns, as agent_episode_kernel
    __shared__ __attribute__((aligned(16))) float Ol[16 * OLD];           // the 16 envs' observation rows
    __shared__ __attribute__((aligned(16))) float Xl[16 * EP_LD];         // x = ReLU(fc1 obs)
    __shared__ __attribute__((aligned(16))) float A1l[16 * ES_ALD], A2l[16 * ES_ALD];   // actor layers 1, 2
    __shared__ __attribute__((aligned(16))) float W2l[ES_AH * ES_ALD];    // actor layer 2 weights [out][in], pitch ES_ALD
    __shared__ __attribute__((aligned(16))) float W3l[A * ES_AH];         // actor layer 3 weights
    __shared__ float Pl[16 * A];                                          // actor output P[row][a] of the current step
    __shared__ float thf[R][16];                                          // (float) theta_a of the current observation
    __shared__ double s_az[R][16];                                        // theta_a (gathered by a jammer's chosen radar)
    __shared__ int Tl[J][16];                                             // chosen actions of the current step
    __shared__ float Pcl[J][16];
    __shared__ std::conditional_t<PE, EpScanConsts, EpScanTab<J, R>> tab;
    // PE: the 16 envs' own table rows and flag bytes
    using PR = EpScanPeRows<J, R>;
    constexpr int PTN = PR::INVW + (PAT ? R : 0);
    __shared__ double pt[PE ? PTN * 16 : 1];
    __shared__ uint8_t pfl[PE ? J * R * 16 : 1];
    __shared__ int pcol[MOV ? NPOS : 1];   // MOV: the position columns' indices in a state row
    // PAT: level tables [L + 2, R] packed [k * R + r] (row 0 main, 1..L the pattern's levels, L + 1 side lobe), 1 / width
    constexpr int LVN = (PAT && !PE) ? MAXLV * R : 1;
    __shared__ double lv_GaPs[LVN], lv_pd_no[LVN], lv_gr[LVN], lv_invw[(PAT && !PE) ? R : 1];
    int pat_L = 0;
    if constexpr (PAT && PE) {
        pat_L = io.pat_levels;
    } else if constexpr (PAT) {
        pat_L = tb->pat_levels;
        if (threadIdx.x < (pat_L + 2) * R) {
            lv_GaPs[threadIdx.x] = tb->lv_GaPs[threadIdx.x];
            lv_pd_no[threadIdx.x] = tb->lv_pd_no[threadIdx.x];
            lv_gr[threadIdx.x] = tb->lv_gr[threadIdx.x];
        }
        if (threadIdx.x < R) lv_invw[threadIdx.x] = tb->pat_inv_width[threadIdx.x];
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int64_t e0 = (int64_t)blockIdx.x * 16;
    const int T = io.T, S = io.S;
    const int64_t E = io.n_envs;
    const int64_t N = E * J;
    const int col0 = io.scan.st_col0, colstep = io.scan.st_col_step;
    auto env_of = [&](int r, bool& live) -> int64_t {   // clamped: rows past the end are computed, never stored
        const int64_t e = e0 + r;
        live = e < E;
        return live ? e : E - 1;
    };

    // ---- launch constants: weight fragments (B operands) ----
    f32x4 Bh[3][EP_KQ], Bi[3][EP_KQ], Bq[EP_KQ];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int Q = 0; Q < EP_KQ; ++Q) {
            const int64_t off = (int64_t)(c * EP_H + 16 * wave + li) * EP_H + 16 * Q + 4 * g;
            Bh[c][Q] = *reinterpret_cast<const f32x4_u*>(io.w_hh + off);
            Bi[c][Q] = *reinterpret_cast<const f32x4_u*>(io.w_ih + off);
        }
#pragma unroll
    for (int Q = 0; Q < EP_KQ; ++Q)
        Bq[Q] = *reinterpret_cast<const f32x4_u*>(io.W1 + (int64_t)(16 * wave + li) * io.w1_ld + 16 * Q + 4 * g);
    // actor layer 2 (128 x 128) is staged in LDS once per launch: as resident fragments it is 64 more VGPRs per lane, which
    // pushed the 3j/4r variant past 512 registers into scratch; read as B fragments it is 16 ds_read_b128 per wave and step
    for (int idx = tid; idx < ES_AH * (ES_AH / 4); idx += 256) {
        const int n = idx / (ES_AH / 4), k4 = idx - n * (ES_AH / 4);
        *reinterpret_cast<f32x4*>(&W2l[n * ES_ALD + 4 * k4]) = *reinterpret_cast<const f32x4_u*>(io.a2_w + (int64_t)n * ES_AH + 4 * k4);
    }
    const int u = 16 * wave + li;          // this lane's hidden unit (gates) / Q-head unit (base) in the C layout
    float bhh[3], bih[3], b2a[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        bhh[c] = io.b_hh[c * EP_H + u];
        bih[c] = io.b_ih[c * EP_H + u];
    }
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) b2a[tl] = io.a2_b[16 * (2 * wave + tl) + li];
    const float b1u = io.b1[u];
    // ---- first layers (fc1, actor layer 1): B fragments over the S observation columns, zero beyond S; the same k order,
    // zero padding and bias-after-sum as mlp_forward_kernel, so x and the actor's first layer are the step-by-step path's
    // values bit for bit (theta_a reaches 360: a different summation order moves these sums by ~1e-5) ----
    f32x4 Bx[SQ], Ba[2][SQ];
    auto frag_s = [&](const float* w, int row, int Q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 16 * Q + 4 * g + i;
            const float x = w[(int64_t)row * S + (c < S ? c : S - 1)];   // clamped address + select: no load in a branch
            v[i] = c < S ? x : 0.0f;
        }
        return v;
    };
#pragma unroll
    for (int Q = 0; Q < SQ; ++Q) {
        Bx[Q] = frag_s(io.fc1_w, 16 * wave + li, Q);
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) Ba[tl][Q] = frag_s(io.a1_w, 16 * (2 * wave + tl) + li, Q);
    }
    const float bfx = io.fc1_b[u];
    float bfa[2];
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) bfa[tl] = io.a1_b[16 * (2 * wave + tl) + li];
    for (int idx = tid; idx < 16 * 16 * SQ; idx += 256) {   // observation rows: the env's own state row, zero pad columns
        const int row = idx / (16 * SQ), c = idx - row * (16 * SQ);
        bool live;
        const int64_t e = env_of(row, live);
        const float x = io.scan.state[e * io.scan.st_se + (c < S ? c : S - 1)];
        Ol[row * OLD + c] = c < S ? x : 0.0f;
    }
    // actor layer 3: thread -> (row = tid & 15, action = tid >> 4), clamped for the threads past 16 A
    const int r3 = tid & 15, a3 = (tid >> 4) < A ? (tid >> 4) : A - 1;
    const float b3 = io.a3_b[a3];
    for (int idx = tid; idx < A * ES_AH; idx += 256) W3l[idx] = io.a3_w[idx];
    for (int idx = tid; idx < (A + 2) * EP_H; idx += 256) {
        const int a = idx / EP_H, uu = idx - a * EP_H;
        Wq[idx] = (a <= A) ? io.W1[(int64_t)uu * io.w1_ld + EP_H + a] : io.w2[uu];
    }
    const float b2 = io.b2[0];
    // env tables -> LDS
    if constexpr (MOV) {   // (the frame's rows are staged at the top of every step)
        if (tid < NPOS) pcol[tid] = io.position_columns[tid];
        if (tid == 0) {
            tab.rp_min = tb->rp_min; tab.rp_max = tb->rp_max; tab.pd_A = tb->pd_A; tab.pd_c1 = tb->pd_c1;
            tab.pd_denB = tb->pd_denB; tab.episode_limit = tb->episode_limit;
        }
    } else if constexpr (PE) {
        // thread -> (column tid & 15 = env of the workgroup, rows tid >> 4, + 16, ...): one env column per thread, so the
        // tile arithmetic is done once; sixteen consecutive envs of a row are 128 contiguous bytes (a tile boundary aside)
        const int c = tid & 15;
        bool live;
        const int64_t e = env_of(c, live);
        const bool tiled = io.pe_tile > 0;
        const int64_t tl = tiled ? e / io.pe_tile : 0;
        const int64_t cl = tiled ? e - tl * io.pe_tile : e;
        const int64_t ps = tiled ? (int64_t)io.pe_tile : io.pe_stride, sps = tiled ? (int64_t)io.pe_tile : io.sp_stride;
        const double* __restrict__ pe = io.pe_tables + tl * PR::NPE * ps + cl;
        const uint8_t* __restrict__ pf = io.pe_flags + tl * (J * R) * ps + cl;
        const double* __restrict__ sp = io.sp_tables + tl * PR::NSP * sps + cl;
        for (int row = tid >> 4; row < PR::INVW; row += 16)
            pt[row * 16 + c] = row < PR::NPE ? pe[(int64_t)row * ps] : sp[(int64_t)PR::sp_src(row - PR::NPE) * sps];
        for (int row = tid >> 4; row < J * R; row += 16) pfl[row * 16 + c] = pf[(int64_t)row * ps];
        if constexpr (PAT) {   // inv_width: the first R rows of the env's pattern column
            const int64_t pps = tiled ? (int64_t)io.pe_tile : io.pp_stride;
            const double* __restrict__ pp = io.pp_tables + tl * (R + 4 * (int64_t)(pat_L + 2) * R) * pps + cl;
            if (tid < 16 * R) pt[(PR::INVW + (tid >> 4)) * 16 + c] = pp[(int64_t)(tid >> 4) * pps];
        }
        if (tid == 0) {
            tab.rp_min = tb->rp_min; tab.rp_max = tb->rp_max; tab.pd_A = tb->pd_A; tab.pd_c1 = tb->pd_c1;
            tab.pd_denB = tb->pd_denB; tab.episode_limit = tb->episode_limit;
        }
    } else {
    if (tid < R) {
        const int r = tid;
        tab.GaPs[r] = tb->GaPs[r]; tab.GaPs_side[r] = tb->GaPs_side[r]; tab.Pn[r] = tb->Pn[r]; tab.D[r] = tb->D[r];
        tab.pd_no[r] = tb->pd_no[r]; tab.pd_no_side[r] = tb->pd_no_side[r]; tab.rd_pen[r] = tb->rd_pen[r];
        tab.gr[r] = tb->gr[r]; tab.gr_side[r] = tb->gr_side[r]; tab.half[r] = tb->half[r]; tab.h2[r] = tb->h2[r];
        tab.sweep[r] = tb->sweep[r]; tab.swm[r] = tb->swm[r]; tab.bt[r] = tb->bt[r]; tab.full[r] = tb->full[r];
        tab.snr_no[r] = tb->snr_no[r]; tab.snr_no_side[r] = tb->snr_no_side[r];
    }
    if (tid < J) {
        tab.pmin[tid] = tb->pmin[tid]; tab.pmax[tid] = tb->pmax[tid]; tab.gj[tid] = tb->gj[tid];
    }
    if (tid < J * R) {
        tab.denom[tid] = tb->denom[tid]; tab.bj[tid] = tb->bj[tid]; tab.flags[tid] = tb->flags[tid];
    }
    if (tid == 0) {
        tab.rp_min = tb->rp_min; tab.rp_max = tb->rp_max; tab.pd_A = tb->pd_A; tab.pd_c1 = tb->pd_c1;
        tab.pd_denB = tb->pd_denB; tab.episode_limit = tb->episode_limit;
    }
    }
    // ---- hidden state ----
    float hreg[J][4];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            bool live;
            const int64_t n = env_of(4 * g + r, live) * J + j;
            hreg[j][r] = io.h0 ? io.h0[n * EP_H + u] : 0.0f;
            Hl[0][j][(4 * g + r) * EP_LD + u] = hreg[j][r];
        }
    // Q-head phase roles: wave = agent tile (waves >= J idle there), lane = (row qr, quarter qq)
    const int qr = lane & 15, qq = lane >> 4;
    const int jq = wave < J ? wave : 0;
    bool live_q;
    const int64_t eq = env_of(qr, live_q);
    const int64_t nq = eq * J + jq;
    uint64_t avail_bits = 0;
    int n_avail = 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        bool av = true;
        if (io.avail) {
            const int64_t off = eq * io.av_se + jq * io.av_sj + (int64_t)a * io.av_sa;
            av = (io.avail_elem_size == 8) ? (((const int64_t*)io.avail)[off] != 0) : (((const int32_t*)io.avail)[off] != 0);
        }
        avail_bits |= av ? (1ull << a) : 0ull;
        n_avail += av ? 1 : 0;
    }
    const uint64_t ctr_base = io.counter_base ? io.counter_base[0] : 0ull;
    // ---- env state of lane (lane & 15)'s env (used by wave 0; the other waves carry copies) ----
    const int er = lane & 15;
    bool live_e;
    const int64_t ee = env_of(er, live_e);
    const bool env_lane = (wave == 0) && (lane < 16);
    double az[R];
    uint32_t s_bits = 0, in_t_last = 0;
    uint32_t lv_last = 0;   // PAT: the target's level at radar r in the last step, bits [4r, 4r + 4)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        az[r] = io.scan.theta_a[ee * io.scan.a_se + (int64_t)r * io.scan.a_sx];
        s_bits |= (io.track[ee * io.k_se + (int64_t)r * io.k_sx] != 0) ? (1u << r) : 0u;
    }
    int32_t step_ctr = io.step[ee];
    const int32_t step0 = step_ctr;   // MOV: env (lane & 15)'s counter at entry, in every wave
    // MVP: env (lane & 15)'s place in the tiled tables — the only division of the launch; element offset of row 0 of frame f
    // of a table with `frames` frames per tile and `rows` rows per frame (consecutive rows are mv_w elements apart)
    int64_t mv_tl = 0, mv_w = 1;
    int mv_cl = 0;
    if constexpr (MVP) {
        mv_w = io.tile;
        mv_tl = ee / mv_w;
        mv_cl = (int)(ee - mv_tl * mv_w);
    }
    auto mv_off = [&](int64_t frames, int64_t f, int rows) -> int64_t { return ((mv_tl * frames + f) * rows) * mv_w + mv_cl; };
    const uint32_t episode = io.episode ? (uint32_t)io.episode[ee] : 0u;
    float rsum[3] = {0.0f, 0.0f, 0.0f};
    if (io.rdpj_sum) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rsum[k] = io.rdpj_sum[ee * 3 + k];
    }
    if (env_lane) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            thf[r][er] = (float)az[r];
            s_az[r][er] = az[r];
        }
    }
    __syncthreads();
    if constexpr (MOV) {   // the first step's position columns of the observation tile, from the table like every later step's
        const int k = step0 < io.n_frames ? step0 : io.n_frames;
        if constexpr (MVP) {
            const float* __restrict__ ps = io.positions + mv_off((int64_t)io.n_frames + 1, k, NPOS);
            for (int i = tid; i < 16 * NPOS; i += 256) Ol[er * OLD + pcol[i >> 4]] = ps[(int64_t)(i >> 4) * mv_w];
        } else {
        for (int i = tid; i < 16 * NPOS; i += 256) Ol[er * OLD + pcol[i >> 4]] = io.positions[(int64_t)k * NPOS + (i >> 4)];
        }
        __syncthreads();
    }
    const PdConsts pdk = pd_consts(tab.pd_A, tab.pd_c1, tab.pd_denB);
    // table reads of the env half: the shared LDS struct, or (PE) this lane's column er of the per-env block
#define ES_TAB(name, ROW, member)                                     \
    auto name = [&](int i) -> double {                                \
        if constexpr (PE) return pt[(PR::ROW + i) * 16 + er];         \
        else return tab.member[i];                                    \
    }
    ES_TAB(t_GaPs, GAPS, GaPs); ES_TAB(t_GaPs_side, GAPS_SIDE, GaPs_side); ES_TAB(t_Pn, PN, Pn); ES_TAB(t_D, D, D);
    ES_TAB(t_pd_no, PD_NO, pd_no); ES_TAB(t_pd_no_side, PD_NO_SIDE, pd_no_side); ES_TAB(t_rd_pen, RD_PEN, rd_pen);
    ES_TAB(t_gr, GR, gr); ES_TAB(t_gr_side, GR_SIDE, gr_side); ES_TAB(t_half, HALF, half); ES_TAB(t_sweep, SWEEP, sweep);
    ES_TAB(t_swm, SWM, swm); ES_TAB(t_bt, BT, bt); ES_TAB(t_pmin, PMIN, pmin); ES_TAB(t_pmax, PMAX, pmax); ES_TAB(t_gj, GJ, gj);
    ES_TAB(t_bj, BJ, bj);
#undef ES_TAB
    auto t_h2 = [&](int r) -> double {      // PE: 2 half and (sweep + 2 half >= 360) restate the host's values exactly
        if constexpr (PE) return 2.0 * t_half(r); else return tab.h2[r];
    };
    auto t_full = [&](int r) -> bool {
        if constexpr (PE) return t_sweep(r) + 2.0 * t_half(r) >= 360.0; else return tab.full[r] != 0;
    };
    auto t_flags = [&](int i) -> uint8_t {
        if constexpr (PE) return pfl[i * 16 + er]; else return tab.flags[i];
    };
    auto t_invw = [&](int r) -> double {
        if constexpr (PE) return pt[(PR::INVW + r) * 16 + er]; else return lv_invw[r];
    };
    // PAT on per-env tables: this lane's column of the pattern SoA (inv_width[R] | GaPs_lvl | snr_no_lvl | pd_no_lvl | gr_lvl,
    // each [(L + 2) R]); row of level k of radar r in level table `lt`
    enum { PP_GAPS = 0, PP_SNR_NO, PP_PD_NO, PP_GR };
    const double* __restrict__ pp_lane = nullptr;
    int64_t pps = 0;
    const double* mv_pp = nullptr;   // MOV: frame f's row of pattern_frames (set in S5)
    if constexpr (PAT && PE && !MOV) {
        const bool tiled = io.pe_tile > 0;
        const int64_t tl = tiled ? ee / io.pe_tile : 0;
        pps = tiled ? (int64_t)io.pe_tile : io.pp_stride;
        pp_lane = io.pp_tables + tl * (R + 4 * (int64_t)(pat_L + 2) * R) * pps + (tiled ? ee - tl * io.pe_tile : ee);
    }
    auto pp_row = [&](int lt, int k, int r) -> double {
        if constexpr (MVP) return mv_pp[(int64_t)(R + (lt * (pat_L + 2) + k) * R + r) * mv_w];
        else if constexpr (MOV) return mv_pp[R + (lt * (pat_L + 2) + k) * R + r];
        else return pp_lane[(int64_t)(R + (lt * (pat_L + 2) + k) * R + r) * pps];
    };

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        if constexpr (MVP) {
            // frame f of env (tid & 15)'s own column -> the [row][16] block and the flag bytes, in place (read next in S5)
            const int64_t f = (step0 + t < io.n_frames ? step0 + t : io.n_frames - 1);
            const double* __restrict__ pe = io.frames + mv_off(io.n_frames, f, PR::NPE);
            const double* __restrict__ sp = io.scan_frames + mv_off(io.n_frames, f, PR::NSP);
            for (int row = tid >> 4; row < PR::INVW; row += 16)
                pt[row * 16 + er] = row < PR::NPE ? pe[(int64_t)row * mv_w] : sp[(int64_t)PR::sp_src(row - PR::NPE) * mv_w];
            if ((tid >> 4) < J * R) pfl[(tid >> 4) * 16 + er] = io.frame_flags[mv_off(io.n_frames, f, J * R) + (int64_t)(tid >> 4) * mv_w];
            if constexpr (PAT) {   // inv_width: the first R rows of the env's pattern column of the frame
                if (tid < 16 * R)
                    pt[(PR::INVW + (tid >> 4)) * 16 + er] =
                        io.pattern_frames[mv_off(io.n_frames, f, R + 4 * (pat_L + 2) * R) + (int64_t)(tid >> 4) * mv_w];
            }
        } else if constexpr (MOV) {
            // frame f of env column (tid & 15) -> the [row][16] block and the flag bytes, in place (read next in S5)
            const int64_t f = (step0 + t < io.n_frames ? step0 + t : io.n_frames - 1);
            const double* __restrict__ pe = io.frames + f * PR::NPE;
            const double* __restrict__ sp = io.scan_frames + f * PR::NSP;
            for (int row = tid >> 4; row < PR::INVW; row += 16)
                pt[row * 16 + er] = row < PR::NPE ? pe[row] : sp[PR::sp_src(row - PR::NPE)];
            if ((tid >> 4) < J * R) pfl[(tid >> 4) * 16 + er] = io.frame_flags[f * (J * R) + (tid >> 4)];
            if constexpr (PAT) {   // inv_width: the first R rows of the frame's pattern row
                if (tid < 16 * R)
                    pt[(PR::INVW + (tid >> 4)) * 16 + er] = io.pattern_frames[f * (R + 4 * (int64_t)(pat_L + 2) * R) + (tid >> 4)];
            }
        }
        // ---- (S1) this step's observation: theta_a columns of the staging rows; first layers ----
        for (int i = tid; i < 16 * R * (J + 1); i += 256) {
            const int row = i & 15, rest = i >> 4;
            const int r = rest % R, jj = rest / R;      // jj == J: the state row
            bool live;
            const int64_t e = env_of(row, live);
            const float v = thf[r][row];
            const int c = col0 + r * colstep;
            if (live) {
                if (jj == J) io.st_state[((int64_t)t * E + e) * S + c] = v;
                else io.st_obs[(((int64_t)t * E + e) * J + jj) * S + c] = v;
            }
        }
        if constexpr (MOV) {   // position columns of this step's staging rows, from the observation tile
            for (int i = tid; i < 16 * NPOS * (J + 1); i += 256) {
                const int row = i & 15, rest = i >> 4;
                const int p = rest % NPOS, jj = rest / NPOS;      // jj == J: the state row
                bool live;
                const int64_t e = env_of(row, live);
                const int c = pcol[p];
                const float v = Ol[row * OLD + c];
                if (live) {
                    if (jj == J) io.st_state[((int64_t)t * E + e) * S + c] = v;
                    else io.st_obs[(((int64_t)t * E + e) * J + jj) * S + c] = v;
                }
            }
        }
        {
            f32x4 ax = f32x4{0.f, 0.f, 0.f, 0.f}, aa[2];
            aa[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            aa[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int Q = 0; Q < SQ; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&Ol[li * OLD + 16 * Q + 4 * g]);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    ax = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], Bx[Q][jj], ax, 0, 0, 0);
#pragma unroll
                    for (int tl = 0; tl < 2; ++tl) aa[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], Ba[tl][Q][jj], aa[tl], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Xl[(4 * g + r) * EP_LD + u] = fmaxf(ax[r] + bfx, 0.0f);
#pragma unroll
                for (int tl = 0; tl < 2; ++tl)
                    A1l[(4 * g + r) * ES_ALD + 16 * (2 * wave + tl) + li] = fmaxf(aa[tl][r] + bfa[tl], 0.0f);
            }
        }
        __syncthreads();
        // ---- (S2) gi = W_ih x + b_ih (one tile, shared by the agents); actor layer 2; gh; gates ----
        float giv[4][3];
        {
            f32x4 ai[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) ai[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int Q = 0; Q < EP_KQ; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&Xl[li * EP_LD + 16 * Q + 4 * g]);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int c = 0; c < 3; ++c) ai[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], Bi[c][Q][jj], ai[c], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) giv[r][c] = ai[c][r] + bih[c];
        }
        {
            f32x4 a2[2];
            a2[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            a2[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int Q = 0; Q < ES_AKQ; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&A1l[li * ES_ALD + 16 * Q + 4 * g]);
                f32x4 b[2];
#pragma unroll
                for (int tl = 0; tl < 2; ++tl)
                    b[tl] = *reinterpret_cast<const f32x4*>(&W2l[(16 * (2 * wave + tl) + li) * ES_ALD + 16 * Q + 4 * g]);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int tl = 0; tl < 2; ++tl) a2[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], b[tl][jj], a2[tl], 0, 0, 0);
            }
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    A2l[(4 * g + r) * ES_ALD + 16 * (2 * wave + tl) + li] = fmaxf(a2[tl][r] + b2a[tl], 0.0f);
        }
        f32x4 acc[J][3];
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[j][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int Q = 0; Q < EP_KQ; ++Q) {
            f32x4 a[J];
#pragma unroll
            for (int j = 0; j < J; ++j) a[j] = *reinterpret_cast<const f32x4*>(&Hl[cur][j][li * EP_LD + 16 * Q + 4 * g]);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int j = 0; j < J; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        acc[j][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][jj], Bh[c][Q][jj], acc[j][c], 0, 0, 0);
        }
        // gates (torch.nn.GRUCell, gate order r, z, n; expressions of gru_gates_kernel)
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float hr = acc[j][0][r] + bhh[0], hz = acc[j][1][r] + bhh[1], hn = acc[j][2][r] + bhh[2];
                const float rg = 1.0f / (1.0f + expf(-(giv[r][0] + hr)));
                const float zg = 1.0f / (1.0f + expf(-(giv[r][1] + hz)));
                const float nn = 1.0f - 2.0f / (expf(2.0f * (giv[r][2] + rg * hn)) + 1.0f);
                const float hnew = (hreg[j][r] - nn) * zg + nn;
                hreg[j][r] = hnew;
                const int row = 4 * g + r;
                Hl[nxt][j][row * EP_LD + u] = hnew;
                bool live;
                const int64_t n = env_of(row, live) * J + j;
                if (live) io.hidden[((int64_t)t * N + n) * EP_H + u] = hnew;   // staging row t: post-update h_t
            }
        __syncthreads();
        // ---- (S3) actor layer 3 + sigmoid -> P; Q-head base = W1[:, :H] h_t + b1 ----
        {
            float s = 0.0f;
            const float* arow = &A2l[r3 * ES_ALD];
            const float* wrow = &W3l[a3 * ES_AH];
#pragma unroll 4
            for (int k4 = 0; k4 < ES_AH / 4; ++k4) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 4 * k4);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wrow + 4 * k4);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) s = fmaf(av[kk], wv[kk], s);
            }
            s += b3;
            const float p = 1.0f / (1.0f + expf(-s));
            if (tid < 16 * A) Pl[r3 * A + a3] = p;
        }
        {
            f32x4 ab[J];
#pragma unroll
            for (int j = 0; j < J; ++j) ab[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int Q = 0; Q < EP_KQ; ++Q) {
                f32x4 a[J];
#pragma unroll
                for (int j = 0; j < J; ++j) a[j] = *reinterpret_cast<const f32x4*>(&Hl[nxt][j][li * EP_LD + 16 * Q + 4 * g]);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int j = 0; j < J; ++j) ab[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][jj], Bq[Q][jj], ab[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) Bl[j][(4 * g + r) * EP_LD + u] = ab[j][r] + b1u;
        }
        __syncthreads();
        // ---- (S4) all-action Q-head + selection: wave = agent tile ----
        const float epsilon = io.greedy_only ? 0.0f : io.eps[t];
        if (wave < J) {
            const int j = wave;
            float q[A], pv[A];
#pragma unroll
            for (int a = 0; a < A; ++a) {
                q[a] = 0.0f;
                pv[a] = Pl[qr * A + a];
            }
            const float* brow = &Bl[j][qr * EP_LD + 16 * qq];
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(brow + 4 * k4);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int uu = 16 * qq + 4 * k4 + kk;
                    const float wp = Wq[A * EP_H + uu], w2u = Wq[(A + 1) * EP_H + uu];
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        float v = b4[kk] + Wq[a * EP_H + uu];          // (W_h h + b1)[u] + W1[u, H + a]
                        v = fmaf(pv[a], wp, v);                        // + W1[u, H + A] * P_a
                        v = fmaxf(v, 0.0f);                            // ReLU
                        q[a] = fmaf(v, w2u, q[a]);                     // second layer
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < A; ++a) {
                q[a] += __shfl_xor(q[a], 16, 64);
                q[a] += __shfl_xor(q[a], 32, 64);
                q[a] += b2;
            }
            if (qq == 0) {
                // mask, first arg-max, epsilon-greedy: as agent_episode_kernel / qhead_select_kernel
                int best = 0;
                float bestq = -INFINITY;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    const float qa = ((avail_bits >> a) & 1ull) ? q[a] : -INFINITY;
                    if (qa > bestq) { bestq = qa; best = a; }
                }
                int chosen = best;
                if (epsilon > 0.0f) {
                    const uint64_t counter = ctr_base + (uint64_t)(t + 1);
                    const Philox4 rr = philox4x32_10((uint32_t)nq, (uint32_t)((uint64_t)nq >> 32), (uint32_t)counter,
                                                     (uint32_t)(counter >> 32), (uint32_t)io.seed, (uint32_t)(io.seed >> 32));
                    const float u_pick = (float)(rr.v[0] >> 8) * (1.0f / 16777216.0f);
                    if (u_pick < epsilon) {
                        const int pool = n_avail > 0 ? n_avail : A;
                        int k = (int)(((uint64_t)rr.v[1] * (uint64_t)pool) >> 32);
                        chosen = 0;
#pragma unroll
                        for (int a = 0; a < A; ++a) {
                            const bool av = (n_avail > 0) ? ((avail_bits >> a) & 1ull) : true;
                            if (av) { if (k == 0) chosen = a; --k; }
                        }
                    }
                }
                float pc = 0.0f;
#pragma unroll
                for (int a = 0; a < A; ++a) pc = (a == chosen) ? pv[a] : pc;
                Tl[j][qr] = chosen;
                Pcl[j][qr] = pc;
                if (live_q) {
                    const int64_t o = (int64_t)t * N + nq;
                    io.T_out[o] = chosen;
                    io.P_out[o] = pc;
                }
            }
        }
        __syncthreads();
        // ---- (S5) scanning env step, one lane per env (wave 0; its lanes >= 16 repeat lanes 0..15 and store nothing) ----
        if (wave == 0) {
            constexpr int NP = R + J, NBLK = (NP + 3) / 4;
            const uint32_t step_before = (uint32_t)step_ctr;
            if constexpr (MVP && PAT)   // the level rows of this step's frame in the env's own column
                mv_pp = io.pattern_frames + mv_off(io.n_frames, step_ctr < io.n_frames ? step_ctr : io.n_frames - 1, R + 4 * (pat_L + 2) * R);
            else if constexpr (MOV && PAT)   // the level rows of this step's frame (wave 0's counter is step0 + t here)
                mv_pp = io.pattern_frames + (int64_t)(step_ctr < io.n_frames ? step_ctr : io.n_frames - 1) * (R + 4 * (int64_t)(pat_L + 2) * R);
            uint32_t rw[NBLK * 4];
#pragma unroll
            for (int b = 0; b < NBLK; ++b) {
                const Philox4 blk = env_philox_block(io.env_seed, (uint64_t)(io.env_offset + ee), episode, step_before, (uint32_t)b);
#pragma unroll
                for (int i = 0; i < 4; ++i) rw[b * 4 + i] = blk.v[i];
            }
            uint32_t in_t = 0;   // bit r: radar r sees the target in its main lobe (start-of-step azimuth and FSM state)
            uint32_t lv_t = 0;   // PAT: the target's level at radar r, bits [4r, 4r + 4)
            double pl_GaPs[(PAT && PE) ? R : 1], pl_pd_no[(PAT && PE) ? R : 1];   // the target's level rows of the env's column
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double lim = (((s_bits >> r) & 1u) ? 0.0 : t_sweep(r)) + t_h2(r);
                if constexpr (PAT) {
                    const int k = beam_level(t_bt(r), az[r], t_half(r), lim, t_full(r), t_invw(r), pat_L);
                    lv_t |= (uint32_t)k << (4 * r);
                    if constexpr (PE) {   // requested here, by address, so that they are in flight over the jammer pass
                        pl_GaPs[r] = pp_row(PP_GAPS, k, r);
                        pl_pd_no[r] = pp_row(PP_PD_NO, k, r);
                    }
                } else {
                    in_t |= in_main_lobe(t_bt(r), az[r], t_half(r), lim, t_full(r)) ? (1u << r) : 0u;
                }
            }
            double supp[R], prod[R], snr_all[NP], pd_all[NP];
#pragma unroll
            for (int r = 0; r < R; ++r) { supp[r] = 0.0; prod[r] = 1.0; }
            uint32_t supp_mask = 0, hit_mask = 0;
            int dec_tgt[J];
            double r_p = 0.0;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                // action decode, power scale, r_p term (environment.py:249-277)
                const int32_t Tj = Tl[j][er];
                const bool is_jamming = (Tj >= 1) && (Tj <= 2 * R);
                const int target = is_jamming ? ((Tj + 1) / 2 - 1) : 0;
                const int jtype = Tj % 2;
                const double pmin = t_pmin(j), pmax = t_pmax(j);
                const double power_range = pmax - pmin;
                float Pc = Pcl[j][er];
                Pc = Pc < 0.0f ? 0.0f : (Pc > 1.0f ? 1.0f : Pc);
                const float actual_f = (float)pmin + Pc * (float)power_range;
                const double actual_d = (double)actual_f;
                const double norm = (power_range > 1e-6) ? (double)((actual_f - (float)pmin) / (float)power_range) : 0.0;
                r_p += tab.rp_max + (tab.rp_min - tab.rp_max) * norm;
                // received jamming power (environment.py:280-302), receive gain by the jammer's bearing
                double denom;   // (read in place: through an accessor the shared kernels' `live` mask is formed with swapped operands)
                if constexpr (PE) denom = pt[(PR::DENOM + j * R + target) * 16 + er]; else denom = tab.denom[j * R + target];
                const uint8_t fl = t_flags(j * R + target);
                const bool recorded = is_jamming && (actual_d > 0.0) && (denom >= 0.0);
                const bool live = recorded && denom > 1e-18;
                const double dsafe = live ? denom : 1.0;
                const double lim = (((s_bits >> target) & 1u) ? 0.0 : t_sweep(target)) + t_h2(target);
                double grj;
                if constexpr (PAT && PE)
                    grj = pp_row(PP_GR, beam_level(t_bj(j * R + target), s_az[target][er], t_half(target), lim, t_full(target),
                                                   t_invw(target), pat_L), target);
                else if constexpr (PAT)
                    grj = lv_gr[beam_level(t_bj(j * R + target), s_az[target][er], t_half(target), lim, t_full(target),
                                           t_invw(target), pat_L) * R + target];
                else
                    grj = in_main_lobe(t_bj(j * R + target), s_az[target][er], t_half(target), lim, t_full(target))
                              ? t_gr(target) : t_gr_side(target);
                const float num = (actual_f * (float)t_gj(j)) * (float)grj;
                const double q = (fl & MACJD_JR_WEAK_DENOM) ? (double)(num / (float)dsafe) : (double)num / dsafe;
                const double prj = (live && q > 0.0) ? q : 0.0;
                const bool is_sup = recorded && (jtype == 1);
                const bool is_dec = recorded && (jtype == 0);
                supp_mask |= is_sup ? (1u << target) : 0u;
#pragma unroll
                for (int r = 0; r < R; ++r) supp[r] = __builtin_fma(prj, (is_sup && target == r) ? 1.0 : 0.0, supp[r]);
                dec_tgt[j] = is_dec ? target : -1;
                // SNR of the false target (environment.py:410-422)
                const double Pn_t = t_Pn(target);
                const bool live_f = is_dec && Pn_t > 1e-18;
                const double snr_f = (t_D(target) * prj) / (live_f ? Pn_t : 1.0);
                snr_all[R + j] = (live_f && snr_f > 0.0) ? snr_f : 0.0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {   // SNR with jamming (environment.py:316-333)
                const double den = t_D(r) * supp[r] + t_Pn(r);
                const bool live = den > 1e-18;
                double gaps;
                if constexpr (PAT && PE) gaps = pl_GaPs[r];
                else if constexpr (PAT) gaps = lv_GaPs[(int)((lv_t >> (4 * r)) & 15u) * R + r];
                else gaps = ((in_t >> r) & 1u) ? t_GaPs(r) : t_GaPs_side(r);
                const double q = gaps / (live ? den : 1.0);
                snr_all[r] = live ? q : 0.0;
            }
            det_prob_batch<NP>(snr_all, pd_all, pdk);
            int n_dec = 0;
#pragma unroll
            for (int j = 0; j < J; ++j) {   // Monte-Carlo detection of the false targets in jammer order
                const bool is_dec = dec_tgt[j] >= 0;
                uint32_t w = rw[R];
#pragma unroll
                for (int k = 1; k < J; ++k) w = (n_dec == k) ? rw[R + k] : w;
                const double uu = u32_mid(w);
                n_dec += is_dec ? 1 : 0;
                const double pd_f = pd_all[R + j];
                const bool hit = is_dec && (uu <= pd_f);
                const double safe = pd_f < 0.999999 ? pd_f : 0.999999;
                hit_mask |= hit ? (1u << (dec_tgt[j] & 31)) : 0u;
#pragma unroll
                for (int r = 0; r < R; ++r) prod[r] = (hit && dec_tgt[j] == r) ? prod[r] * (1.0 - safe) : prod[r];
            }
            double r_d = 0.0, r_j = 0.0, r_j_dec = 0.0;
            uint32_t track_bits = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {   // detections, FSM, reward terms, beam advance
                const double pd = pd_all[r];
                const bool detected = u32_mid(rw[r]) <= pd;
                track_bits |= detected ? (1u << r) : 0u;
                r_d += detected ? t_rd_pen(r) : 0.0;
                double pd_no_r;
                if constexpr (PAT && PE) pd_no_r = pl_pd_no[r];
                else if constexpr (PAT) pd_no_r = lv_pd_no[(int)((lv_t >> (4 * r)) & 15u) * R + r];
                else pd_no_r = ((in_t >> r) & 1u) ? t_pd_no(r) : t_pd_no_side(r);
                const double red = pd_no_r - pd;
                r_j += ((supp_mask & (1u << r)) && red > 0.0) ? red : 0.0;
                r_j_dec += (hit_mask & (1u << r)) ? 1.0 - prod[r] : 0.0;
                double x = az[r] + t_swm(r);
                x = (x >= 360.0) ? x - 360.0 : x;
                az[r] = detected ? t_bt(r) : (((s_bits >> r) & 1u) ? az[r] : x);
            }
            r_j += r_j_dec;
            const double reward = r_d + r_p + r_j;
            s_bits = track_bits;
            in_t_last = in_t;
            lv_last = lv_t;
            step_ctr += 1;
            rsum[0] += (float)r_d;
            rsum[1] += (float)r_p;
            rsum[2] += (float)r_j;
            if (lane < 16) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    thf[r][er] = (float)az[r];
                    s_az[r][er] = az[r];
                    Ol[er * OLD + col0 + r * colstep] = (float)az[r];
                }
                if (live_e) {
                    io.reward[(int64_t)t * E + ee] = (float)reward;
                    io.terminated[(int64_t)t * E + ee] = (step_ctr >= tab.episode_limit) ? 1 : 0;
                }
            }
        } else if constexpr (MOV) {
            // waves 1 - 3: the position columns of step t + 1's observation (row = tid & 15: the env whose step0 the thread holds)
            const int k = step0 + t + 1 < io.n_frames ? step0 + t + 1 : io.n_frames;
            if constexpr (MVP) {
                const float* __restrict__ ps = io.positions + mv_off((int64_t)io.n_frames + 1, k, NPOS);
                for (int i = tid - 64; i < 16 * NPOS; i += 192) Ol[er * OLD + pcol[i >> 4]] = ps[(int64_t)(i >> 4) * mv_w];
            } else
            for (int i = tid - 64; i < 16 * NPOS; i += 192) Ol[er * OLD + pcol[i >> 4]] = io.positions[(int64_t)k * NPOS + (i >> 4)];
        }
        __syncthreads();
    }
    // ---- hand-over: what a step-by-step rollout leaves in the environment and the controller ----
    if (env_lane && live_e) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            io.scan.theta_a[ee * io.scan.a_se + (int64_t)r * io.scan.a_sx] = az[r];
            io.track[ee * io.k_se + (int64_t)r * io.k_sx] = (s_bits >> r) & 1u;
            io.scan.state[ee * io.scan.st_se + col0 + r * colstep] = (float)az[r];
            if constexpr (PE) {   // the env's own snr_no_lvl row of the last level / snr_no or snr_no_side row, by address
                if (io.scan.snr_no) {
                    double v;
                    if constexpr (PAT) {
                        v = pp_row(PP_SNR_NO, (int)((lv_last >> (4 * r)) & 15u), r);
                    } else if constexpr (MOV) {   // the last step's frame: its snr_no | snr_no_side row
                        const int64_t fl = step_ctr - 1 < io.n_frames ? step_ctr - 1 : io.n_frames - 1;
                        if constexpr (MVP)
                            v = io.scan_frames[mv_off(io.n_frames, fl, PR::NSP) + (int64_t)((((in_t_last >> r) & 1u) ? 6 : 7) * R + r) * mv_w];
                        else
                        v = io.scan_frames[fl * PR::NSP + (((in_t_last >> r) & 1u) ? 6 : 7) * R + r];
                    } else {
                        const bool tiled = io.pe_tile > 0;
                        const int64_t tl = tiled ? ee / io.pe_tile : 0;
                        const int64_t sps = tiled ? (int64_t)io.pe_tile : io.sp_stride;
                        const double* sp = io.sp_tables + tl * PR::NSP * sps + (tiled ? ee - tl * io.pe_tile : ee);
                        v = sp[(int64_t)((((in_t_last >> r) & 1u) ? 6 : 7) * R + r) * sps];   // snr_no | snr_no_side
                    }
                    io.scan.snr_no[ee * io.scan.sn_se + (int64_t)r * io.scan.sn_sx] = (float)v;
                }
            } else if constexpr (PAT) {
                if (io.scan.snr_no)
                    io.scan.snr_no[ee * io.scan.sn_se + (int64_t)r * io.scan.sn_sx] =
                        (float)tb->lv_snr_no[(int)((lv_last >> (4 * r)) & 15u) * R + r];
            } else {
                if (io.scan.snr_no)
                    io.scan.snr_no[ee * io.scan.sn_se + (int64_t)r * io.scan.sn_sx] =
                        (float)(((in_t_last >> r) & 1u) ? tab.snr_no[r] : tab.snr_no_side[r]);
            }
        }
        if constexpr (MOV) {   // the positions the next step's agents see
            const int k = step_ctr < io.n_frames ? step_ctr : io.n_frames;
            if constexpr (MVP) {
                const float* __restrict__ ps = io.positions + mv_off((int64_t)io.n_frames + 1, k, NPOS);
#pragma unroll
                for (int p = 0; p < NPOS; ++p) io.scan.state[ee * io.scan.st_se + pcol[p]] = ps[(int64_t)p * mv_w];
            } else
#pragma unroll
            for (int p = 0; p < NPOS; ++p) io.scan.state[ee * io.scan.st_se + pcol[p]] = io.positions[(int64_t)k * NPOS + p];
        }
        io.step[ee] = step_ctr;
        if (io.rdpj_sum) {
#pragma unroll
            for (int k = 0; k < 3; ++k) io.rdpj_sum[ee * 3 + k] = rsum[k];
        }
    }
    if (io.h_final) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool live;
                const int64_t n = env_of(4 * g + r, live) * J + j;
                if (live) io.h_final[n * EP_H + u] = hreg[j][r];
            }
    }
}

}  // namespace macjd

extern "C" int macjd_agent_env_episode_scan_supported(int32_t J, int32_t R, int32_t H, int32_t A) {
    return (H == macjd::EP_H && ((J == 3 && R == 4 && A == 9) || (J == 2 && R == 2 && A == 5))) ? 1 : 0;
}

// The argument checks both closed-loop entry points share (everything but the per-env blocks); `pe`: the caller is the
// launch on per-env scenario tables, which needs io->pe_tables where the shared launch refuses them
static int episode_scan_check(const macjd_scenario* s, const macjd_agent_env_episode_scan_io* io, const char* me, bool pe) {
    using namespace macjd;
    if (!s || !io) return set_err(MACJD_EINVAL, "%s: NULL scenario / io", me);
    if (!macjd_agent_env_episode_scan_supported(io->J, io->R, io->H, io->A) || io->actor_hidden != ES_AH)
        return set_err(MACJD_EUNSUPPORTED, "%s: unsupported J / R / H / A / actor width (see include/macjd_nets.h)", me);
    if (!pe && io->pe_tables) return set_err(MACJD_EUNSUPPORTED, "%s: per-env scenario tables are not supported", me);
    if (pe && !io->pe_tables)
        return set_err(MACJD_EINVAL, "%s: needs per-env scenario tables (base.pe_tables); macjd_agent_env_episode_scan takes the handle's", me);
    if (s->host.J != io->J || s->host.R != io->R) return set_err(MACJD_EINVAL, "%s: J / R differ from the scenario's", me);
    if (!s->host.scanning) return set_err(MACJD_EINVAL, "%s: the scenario has no scanning tables (macjd_scenario_set_scan)", me);
    if (io->S > 48) return set_err(MACJD_EUNSUPPORTED, "%s: state vectors wider than 48 are not supported", me);
    if (io->n_envs < 0 || io->T < 1 || io->S < 1 || !io->fc1_w || !io->fc1_b || !io->w_ih || !io->b_ih || !io->w_hh || !io->b_hh ||
        !io->a1_w || !io->a1_b || !io->a2_w || !io->a2_b || !io->a3_w || !io->a3_b || !io->W1 || !io->b1 || !io->w2 || !io->b2 ||
        !io->hidden || !io->T_out || !io->P_out || !io->st_state || !io->st_obs || !io->reward || !io->terminated || !io->track ||
        !io->step || (!io->greedy_only && !io->eps))
        return set_err(MACJD_EINVAL, "%s: bad n_envs / T / S or NULL pointer", me);
    if (!io->scan.theta_a || !io->scan.state || (io->scan.a_se == 0 && io->scan.a_sx == 0) || io->scan.st_se < io->S ||
        io->scan.st_col0 < 0 || io->scan.st_col_step < 1 || io->scan.st_col0 + (int64_t)(io->R - 1) * io->scan.st_col_step >= io->S ||
        (io->scan.snr_no && io->scan.sn_se == 0 && io->scan.sn_sx == 0) || (io->k_se == 0 && io->k_sx == 0))
        return set_err(MACJD_EINVAL, "%s: bad scan io (theta_a / state rows / columns / strides)", me);
    if (io->w1_ld < io->H + io->A + 1) return set_err(MACJD_EINVAL, "%s: row stride smaller than the row", me);
    if (io->avail && io->avail_elem_size != 4 && io->avail_elem_size != 8)
        return set_err(MACJD_EINVAL, "%s: avail_elem_size must be 4 or 8", me);
    if ((io->n_envs + 15) / 16 > 0x7fffffff) return set_err(MACJD_EINVAL, "%s: too many envs for one launch", me);
    return MACJD_OK;
}

extern "C" int macjd_agent_env_episode_scan(const macjd_scenario* s, const macjd_agent_env_episode_scan_io* io, void* hip_stream) {
    using namespace macjd;
    const char* me = "macjd_agent_env_episode_scan";
    const int rc = episode_scan_check(s, io, me, false);
    if (rc != MACJD_OK) return rc;
    if (io->n_envs == 0) return MACJD_OK;
    const dim3 grid((unsigned)((io->n_envs + 15) / 16)), block(256);
    hipStream_t st = (hipStream_t)hip_stream;
    if (s->host.pat_levels > 0) {   // stepped antenna pattern (macjd_scenario_set_scan_pattern)
        if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, true>), grid, block, 0, st, s->dev, *io);
        else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, true>), grid, block, 0, st, s->dev, *io);
    } else if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, false>), grid, block, 0, st, s->dev, *io);
    else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, false>), grid, block, 0, st, s->dev, *io);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_agent_env_episode_scan: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_agent_env_episode_scan_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A) {
    return macjd_agent_env_episode_scan_supported(J, R, H, A);
}

// The closed-loop launch on per-env scenario tables (include/macjd_nets.h, macjd_agent_env_episode_scan_pe_io); its argument
// errors mirror macjd_env_step_scan_pe(_pattern)'s, and all of them return before any launch
extern "C" int macjd_agent_env_episode_scan_pe(const macjd_scenario* s, const macjd_agent_env_episode_scan_pe_io* pio, void* hip_stream) {
    using namespace macjd;
    const char* me = "macjd_agent_env_episode_scan_pe";
    const int rc = episode_scan_check(s, pio ? &pio->base : nullptr, me, true);
    if (rc != MACJD_OK) return rc;
    const macjd_agent_env_episode_scan_io* io = &pio->base;
    const bool pat = pio->pattern.tables != nullptr;
    if (!pio->pe_flags) return set_err(MACJD_EINVAL, "%s: NULL pe_flags", me);
    if (!pio->scan_pe.tables) return set_err(MACJD_EINVAL, "%s: NULL per-env scan tables (scan_pe.tables)", me);
    if (pio->pe_tile < 0) return set_err(MACJD_EINVAL, "%s: pe_tile must be >= 0", me);
    if (pio->pe_tile == 0 && pio->pe_stride < io->n_envs) return set_err(MACJD_EINVAL, "%s: pe_stride must be >= n_envs (or pe_tile > 0)", me);
    if (pio->pe_tile == 0 && pio->scan_pe.stride < io->n_envs)
        return set_err(MACJD_EINVAL, "%s: scan_pe.stride must be >= n_envs (or pe_tile > 0)", me);
    if (pat && pio->pe_tile == 0 && pio->pattern.stride < io->n_envs)
        return set_err(MACJD_EINVAL, "%s: pattern.stride must be >= n_envs (or pe_tile > 0)", me);
    if (pat && (pio->pattern.n_levels < 1 || pio->pattern.n_levels > MACJD_MAX_PATTERN_LEVELS))
        return set_err(MACJD_EINVAL, "%s: pattern.n_levels outside 1..MACJD_MAX_PATTERN_LEVELS", me);
    if (s->host.pat_levels > 0 && (!pat || s->host.pat_levels != pio->pattern.n_levels))
        return set_err(MACJD_EUNSUPPORTED, "%s: the scenario handle carries pattern levels: accepted only with pattern.tables of the same n_levels", me);
    if (io->n_envs == 0) return MACJD_OK;
    EpScanPeIO k{};
    static_cast<macjd_agent_env_episode_scan_io&>(k) = *io;
    k.pe_flags = pio->pe_flags; k.pe_stride = pio->pe_stride; k.pe_tile = pio->pe_tile;
    k.sp_tables = pio->scan_pe.tables; k.sp_stride = pio->scan_pe.stride;
    k.pp_tables = pio->pattern.tables; k.pp_stride = pio->pattern.stride; k.pat_levels = pat ? pio->pattern.n_levels : 0;
    const dim3 grid((unsigned)((io->n_envs + 15) / 16)), block(256);
    hipStream_t st = (hipStream_t)hip_stream;
    if (pat) {
        if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, true, true, EpScanPeIO>), grid, block, 0, st, s->dev, k);
        else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, true, true, EpScanPeIO>), grid, block, 0, st, s->dev, k);
    } else if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, false, true, EpScanPeIO>), grid, block, 0, st, s->dev, k);
    else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, false, true, EpScanPeIO>), grid, block, 0, st, s->dev, k);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_agent_env_episode_scan_pe: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_agent_env_episode_moving_scan_supported(int32_t J, int32_t R, int32_t H, int32_t A) {
    return macjd_agent_env_episode_scan_supported(J, R, H, A);
}

// The closed-loop launch on a moving scanning scenario's frame tables (include/macjd_nets.h,
// macjd_agent_env_episode_moving_scan_io); its argument errors mirror macjd_env_step_moving_scan's, and all of them return
// before any launch
extern "C" int macjd_agent_env_episode_moving_scan(const macjd_scenario* s, const macjd_agent_env_episode_moving_scan_io* mio,
                                                   void* hip_stream) {
    using namespace macjd;
    const char* me = "macjd_agent_env_episode_moving_scan";
    if (mio && mio->base.pe_tables) return set_err(MACJD_EINVAL, "%s: base.pe_tables must be NULL (the frames are the tables)", me);
    const int rc = episode_scan_check(s, mio ? &mio->base : nullptr, me, false);
    if (rc != MACJD_OK) return rc;
    const macjd_agent_env_episode_scan_io* io = &mio->base;
    const macjd_motion_io* mo = &mio->motion;
    const macjd_motion_scan_io* ms = &mio->motion_scan;
    if (!mo->frames || !mo->frame_flags || !mo->positions || !mo->position_columns || !mo->state)
        return set_err(MACJD_EINVAL, "%s: frames / frame_flags / positions / position_columns / state is NULL", me);
    if (!ms->scan_frames) return set_err(MACJD_EINVAL, "%s: NULL scan_frames", me);
    if (mo->n_frames < 1) return set_err(MACJD_EINVAL, "%s: n_frames < 1", me);
    if (mo->n_frames != s->host.episode_limit) return set_err(MACJD_EINVAL, "%s: n_frames must equal the scenario's episode_limit", me);
    if (mo->n_pos != 2 * io->R + 2 * io->J) return set_err(MACJD_EINVAL, "%s: n_pos must equal 2R + 2J", me);
    if (mo->snr_no) return set_err(MACJD_EINVAL, "%s: motion.snr_no must be NULL (the per-step value travels in base.scan.snr_no)", me);
    if (mo->state != io->scan.state || mo->st_se != io->scan.st_se)
        return set_err(MACJD_EINVAL, "%s: base.scan.state and motion.state must be the same rows with the same row stride", me);
    if (ms->n_levels < 0 || ms->n_levels > MACJD_MAX_PATTERN_LEVELS)
        return set_err(MACJD_EINVAL, "%s: n_levels outside 0..MACJD_MAX_PATTERN_LEVELS", me);
    if (s->host.pat_levels > 0 && s->host.pat_levels != ms->n_levels)
        return set_err(MACJD_EINVAL, "%s: n_levels differs from the pattern levels of the scenario handle", me);
    if ((ms->pattern_frames != nullptr) != (ms->n_levels > 0))
        return set_err(MACJD_EINVAL, "%s: pattern_frames and n_levels > 0 go together (both or neither)", me);
    if (io->n_envs == 0) return MACJD_OK;
    const bool pat = ms->pattern_frames != nullptr;
    EpScanMovIO k{};
    static_cast<macjd_agent_env_episode_scan_io&>(k) = *io;
    k.frames = mo->frames; k.frame_flags = mo->frame_flags; k.scan_frames = ms->scan_frames; k.pattern_frames = ms->pattern_frames;
    k.positions = mo->positions; k.position_columns = mo->position_columns;
    k.n_frames = mo->n_frames; k.pat_levels = pat ? ms->n_levels : 0;
    const dim3 grid((unsigned)((io->n_envs + 15) / 16)), block(256);
    hipStream_t st = (hipStream_t)hip_stream;
    if (pat) {
        if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, true, true, EpScanMovIO>), grid, block, 0, st, s->dev, k);
        else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, true, true, EpScanMovIO>), grid, block, 0, st, s->dev, k);
    } else if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, false, true, EpScanMovIO>), grid, block, 0, st, s->dev, k);
    else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, false, true, EpScanMovIO>), grid, block, 0, st, s->dev, k);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_agent_env_episode_moving_scan: %s", hipGetErrorString(err));
    return MACJD_OK;
}

extern "C" int macjd_agent_env_episode_moving_scan_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A) {
    return macjd_agent_env_episode_scan_supported(J, R, H, A);
}

// The closed-loop launch on a per-env moving scanning scenario batch's tiled frame tables (include/macjd_nets.h,
// macjd_agent_env_episode_moving_scan_pe_io); its argument errors mirror macjd_env_step_moving_scan_pe's and
// macjd_agent_env_episode_moving_scan's, and all of them return before any launch
extern "C" int macjd_agent_env_episode_moving_scan_pe(const macjd_scenario* s, const macjd_agent_env_episode_moving_scan_pe_io* mio,
                                                      void* hip_stream) {
    using namespace macjd;
    const char* me = "macjd_agent_env_episode_moving_scan_pe";
    if (mio && mio->base.pe_tables) return set_err(MACJD_EINVAL, "%s: base.pe_tables must be NULL (the frames are the tables)", me);
    const int rc = episode_scan_check(s, mio ? &mio->base : nullptr, me, false);
    if (rc != MACJD_OK) return rc;
    const macjd_agent_env_episode_scan_io* io = &mio->base;
    const macjd_motion_pe_io* mo = &mio->motion_pe;
    const macjd_motion_scan_pe_io* ms = &mio->motion_scan_pe;
    if (!mo->frames || !mo->frame_flags || !mo->positions || !mo->position_columns || !mo->state)
        return set_err(MACJD_EINVAL, "%s: frames / frame_flags / positions / position_columns / state is NULL", me);
    if (!ms->scan_frames) return set_err(MACJD_EINVAL, "%s: NULL scan_frames", me);
    if (mo->n_frames < 1) return set_err(MACJD_EINVAL, "%s: n_frames < 1", me);
    if (mo->n_frames != s->host.episode_limit) return set_err(MACJD_EINVAL, "%s: n_frames must equal the scenario's episode_limit", me);
    if (mo->n_pos != 2 * io->R + 2 * io->J) return set_err(MACJD_EINVAL, "%s: n_pos must equal 2R + 2J", me);
    if (mo->tile < 1) return set_err(MACJD_EINVAL, "%s: tile must be >= 1", me);
    if (mo->snr_no) return set_err(MACJD_EINVAL, "%s: motion_pe.snr_no must be NULL (the per-step value travels in base.scan.snr_no)", me);
    if (mo->state != io->scan.state || mo->st_se != io->scan.st_se)
        return set_err(MACJD_EINVAL, "%s: base.scan.state and motion_pe.state must be the same rows with the same row stride", me);
    if (ms->n_levels < 0 || ms->n_levels > MACJD_MAX_PATTERN_LEVELS)
        return set_err(MACJD_EINVAL, "%s: n_levels outside 0..MACJD_MAX_PATTERN_LEVELS", me);
    if (s->host.pat_levels > 0 && s->host.pat_levels != ms->n_levels)
        return set_err(MACJD_EINVAL, "%s: n_levels differs from the pattern levels of the scenario handle", me);
    if ((ms->pattern_frames != nullptr) != (ms->n_levels > 0))
        return set_err(MACJD_EINVAL, "%s: pattern_frames and n_levels > 0 go together (both or neither)", me);
    if (io->n_envs == 0) return MACJD_OK;
    const bool pat = ms->pattern_frames != nullptr;
    EpScanMovPeIO k{};
    static_cast<macjd_agent_env_episode_scan_io&>(k) = *io;
    k.frames = mo->frames; k.frame_flags = mo->frame_flags; k.scan_frames = ms->scan_frames; k.pattern_frames = ms->pattern_frames;
    k.positions = mo->positions; k.position_columns = mo->position_columns;
    k.n_frames = mo->n_frames; k.pat_levels = pat ? ms->n_levels : 0; k.tile = mo->tile;
    const dim3 grid((unsigned)((io->n_envs + 15) / 16)), block(256);
    hipStream_t st = (hipStream_t)hip_stream;
    if (pat) {
        if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, true, true, EpScanMovPeIO>), grid, block, 0, st, s->dev, k);
        else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, true, true, EpScanMovPeIO>), grid, block, 0, st, s->dev, k);
    } else if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3, false, true, EpScanMovPeIO>), grid, block, 0, st, s->dev, k);
    else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3, false, true, EpScanMovPeIO>), grid, block, 0, st, s->dev, k);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_agent_env_episode_moving_scan_pe: %s", hipGetErrorString(err));
    return MACJD_OK;
}
