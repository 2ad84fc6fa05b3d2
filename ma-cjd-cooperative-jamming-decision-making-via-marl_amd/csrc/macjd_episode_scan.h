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
// Stepped antenna pattern (include/macjd.h, macjd_scan_pattern_desc): the kernel's text lives in
// macjd_episode_scan_kernel.h and is compiled twice, as agent_env_episode_scan_kernel (PAT = false) and as
// agent_env_episode_scan_pat_kernel (PAT = true), which is launched for a handle that carries pattern tables.  Its env
// half takes a level per object from beam_level and reads the [L + 2, R] level tables (GaPs, pd_no, gr) from a second LDS
// block; the target's levels of the last step are kept four bits per radar for the hand-over's snr_no.
#pragma once

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

}  // namespace macjd

#define MACJD_EPSCAN_KERNEL agent_env_episode_scan_kernel
#define MACJD_EPSCAN_PAT 0
namespace macjd {
#include "macjd_episode_scan_kernel.h"
}  // namespace macjd
#undef MACJD_EPSCAN_KERNEL
#undef MACJD_EPSCAN_PAT
#define MACJD_EPSCAN_KERNEL agent_env_episode_scan_pat_kernel
#define MACJD_EPSCAN_PAT 1
namespace macjd {
#include "macjd_episode_scan_kernel.h"
}  // namespace macjd
#undef MACJD_EPSCAN_KERNEL
#undef MACJD_EPSCAN_PAT

extern "C" int macjd_agent_env_episode_scan_supported(int32_t J, int32_t R, int32_t H, int32_t A) {
    return (H == macjd::EP_H && ((J == 3 && R == 4 && A == 9) || (J == 2 && R == 2 && A == 5))) ? 1 : 0;
}

extern "C" int macjd_agent_env_episode_scan(const macjd_scenario* s, const macjd_agent_env_episode_scan_io* io, void* hip_stream) {
    using namespace macjd;
    const char* me = "macjd_agent_env_episode_scan";
    if (!s || !io) return set_err(MACJD_EINVAL, "%s: NULL scenario / io", me);
    if (!macjd_agent_env_episode_scan_supported(io->J, io->R, io->H, io->A) || io->actor_hidden != ES_AH)
        return set_err(MACJD_EUNSUPPORTED, "%s: unsupported J / R / H / A / actor width (see include/macjd_nets.h)", me);
    if (io->pe_tables) return set_err(MACJD_EUNSUPPORTED, "%s: per-env scenario tables are not supported", me);
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
    if (io->n_envs == 0) return MACJD_OK;
    const int64_t wgs = (io->n_envs + 15) / 16;
    if (wgs > 0x7fffffff) return set_err(MACJD_EINVAL, "%s: too many envs for one launch", me);
    const dim3 grid((unsigned)wgs), block(256);
    hipStream_t st = (hipStream_t)hip_stream;
    if (s->host.pat_levels > 0) {   // stepped antenna pattern (macjd_scenario_set_scan_pattern)
        if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_pat_kernel<3, 4, 9, 3>), grid, block, 0, st, s->dev, *io);
        else hipLaunchKernelGGL((agent_env_episode_scan_pat_kernel<2, 2, 5, 3>), grid, block, 0, st, s->dev, *io);
    } else if (io->J == 3) hipLaunchKernelGGL((agent_env_episode_scan_kernel<3, 4, 9, 3>), grid, block, 0, st, s->dev, *io);
    else hipLaunchKernelGGL((agent_env_episode_scan_kernel<2, 2, 5, 3>), grid, block, 0, st, s->dev, *io);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_agent_env_episode_scan: %s", hipGetErrorString(err));
    return MACJD_OK;
}
