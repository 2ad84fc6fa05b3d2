// Device-side pieces of the environment step shared by macjd_env.hip and the closed-loop episode kernel
// (macjd_episode_scan.h): the scenario handle's table block, the detection-probability chain with its refined
// divisions, the main-lobe test and the Philox word pick.  One copy, so both kernels compute the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/macjd.h"
#include "macjd_philox.h"

namespace macjd {

constexpr int MAXR = MACJD_MAX_RADARS;
constexpr int MAXJ = MACJD_MAX_JAMMERS;
constexpr int MAXLV = MACJD_MAX_PATTERN_LEVELS + 2;   // main, the pattern's levels, side lobe

// Device-resident scenario tables (one per scenario handle).
struct DevTables {
    int32_t R, J, episode_limit, pad;
    double rp_min, rp_max, pd_A, pd_c1, pd_denB;
    double GaPs[MAXR], Pn[MAXR], D[MAXR], pd_no[MAXR], rd_pen[MAXR], gr[MAXR];
    double pmin[MAXJ], pmax[MAXJ], gj[MAXJ];
    double denom[MAXJ * MAXR];   // packed [j*R + r]; negative = jammer sits on the radar (ignored)
    uint8_t flags[MAXJ * MAXR];  // packed [j*R + r]
    // ---- derived ON THE DEVICE when the scenario is created (scenario_derive_kernel, with the very device functions the
    // step kernels divide with), read by the REGULAR production variant (see env_step_kernel, REG) ----
    int32_t regular, pad2;       // host verdict: every table value in the range where the short division is IEEE division
    double rPn[MAXR];            // refined reciprocal of Pn
    double range_fd[MAXJ], r_range[MAXJ];      // (double)(float)(pmax - pmin) and its refined reciprocal
    double dsel[MAXJ * MAXR], rsel[MAXJ * MAXR];   // divisor of the received-power quotient as the step uses it (1.0 where
                                                   // it does not divide; the float32-rounded value where the division is
                                                   // float32) and its refined reciprocal
    uint8_t rflags[MAXJ * MAXR]; // flags | JR_RECORDABLE (denom >= 0) | JR_LIVE (denom > 1e-18)
    // ---- scanning beams (macjd_scenario_set_scan; include/macjd.h, macjd_scan_desc), read by the SCAN variants only ----
    int32_t scanning, scan_regular;   // tables set; side-lobe tables also pass the REGULAR range checks
    double half[MAXR], h2[MAXR], sweep[MAXR], swm[MAXR], az0[MAXR], bt[MAXR];   // h2 = 2 half (exact)
    double bj[MAXJ * MAXR];           // packed [j*R + r]
    double GaPs_side[MAXR], pd_no_side[MAXR], gr_side[MAXR], snr_no[MAXR], snr_no_side[MAXR];
    uint8_t full[MAXR];
    // ---- stepped antenna pattern (macjd_scenario_set_scan_pattern; include/macjd.h, macjd_scan_pattern_desc), read by the
    // pattern variants only.  Level tables [L + 2, R] packed [k * R + r]: level 0 = the main tables, 1..L the pattern's,
    // L + 1 the side lobe's, so a kernel stages (L + 2) R consecutive values and indexes them by the per-lane level ----
    int32_t pat_levels, pad3;         // L, 0 = no pattern
    double pat_inv_width[MAXR];
    double lv_GaPs[MAXLV * MAXR], lv_pd_no[MAXLV * MAXR], lv_snr_no[MAXLV * MAXR], lv_gr[MAXLV * MAXR];
};
constexpr uint8_t JR_RECORDABLE = 0x40, JR_LIVE = 0x80;

// ---- detection probability, core/radar.py:67-82 (constants A, c1, denB precomputed on the host) -------------------
// The two divisions of the formula are done with the hardware's own IEEE division algorithm MINUS its scaling /
// special-case wrapper (v_div_scale x2, v_div_fmas' scale step, v_div_fixup): refined reciprocal r of the divisor (v_rcp +
// two Newton steps), q = n r, q + r (n - d q).  That is bit-for-bit what `/` compiles to whenever no operand scaling
// is needed, which holds here by construction: the divisor of B is the scenario constant denB (|denB| >= 1e-9, else
// the function returns 0 like the reference), its numerator is bounded through Z <= 1e300 (any Z that large gives
// B > 700 -> pd = 1 either way); the divisor of 1 / (1 + exp(-B)) lies in [1, e^709] and every result computed from
// B outside [-700, 700] is replaced by the reference's own saturation values.  Both refined reciprocals of a constant
// divisor are shared by all the evaluations of an env-step (3 instead of 11 instructions per division).
struct PdConsts {
    double A, c1, denB, r_denB;
    bool degenerate;   // |denB| < 1e-9 -> pd = 0 (radar.py:75-76)
};
__device__ __forceinline__ double rcp_refined(double d) {
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    return __builtin_fma(r, e, r);
}
__device__ __forceinline__ double div_by_refined(double n, double d, double r) {
    const double q = n * r;
    return __builtin_fma(__builtin_fma(-d, q, n), r, q);
}
__device__ __forceinline__ PdConsts pd_consts(double A, double c1, double denB) {
    PdConsts k;
    k.A = A; k.c1 = c1; k.denB = denB;
    k.degenerate = fabs(denB) < 1e-9;
    k.r_denB = rcp_refined(k.degenerate ? 1.0 : denB);
    return k;
}
// N independent evaluations side by side: straight-line code, the exp polynomial's constants are materialised once
// and the N dependency chains interleave (the one-at-a-time form spent ~150 v_mov on constants per env-step and ran
// each chain alone)
template <int N>
__device__ __forceinline__ void det_prob_batch(const double* snr, double* pd, const PdConsts& k) {
    double B[N], den[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = (0.0 > snr[i]) ? 0.0 : snr[i];  // Python max(snr, 0.0)
        double Z = s + k.c1;
        Z = (Z < 1e300) ? Z : 1e300;
        B[i] = div_by_refined(10.0 * Z - k.A, k.denB, k.r_denB);
        den[i] = 1.0 + exp(-B[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double r = rcp_refined(den[i]);
        double p = div_by_refined(1.0, den[i], r);
        p = (B[i] > 700.0) ? 1.0 : p;
        p = (B[i] < -700.0) ? 0.0 : p;
        pd[i] = k.degenerate ? 0.0 : p;
    }
}
// REGULAR scenarios (host-checked, see macjd_scenario_create): denB > 0 and not degenerate, every SNR the step can form is
// finite, >= +0 and < 1e100, and B >= (10 c1 - A) / denB >= -700 for every SNR >= 0 — so max(snr, 0), the 1e300 cap and
// the B < -700 / degenerate selects of the general form never act; B > 700 needs no select at all: exp(-B) < 2^-53
// there (0 below -745), 1 + exp(-B) rounds to 1.0 and the quotient is exactly the reference's 1.0.
template <int N>
__device__ __forceinline__ void det_prob_batch_regular(const double* snr, double* pd, const PdConsts& k) {
    double den[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double Z = snr[i] + k.c1;
        const double B = div_by_refined(10.0 * Z - k.A, k.denB, k.r_denB);
        den[i] = 1.0 + exp(-B);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) pd[i] = div_by_refined(1.0, den[i], rcp_refined(den[i]));
}
__device__ __forceinline__ double det_prob(double snr, const PdConsts& k) {
    double p;
    det_prob_batch<1>(&snr, &p, k);
    return p;
}

// Main-lobe test of a scanning beam (include/macjd.h, macjd_scan_desc): azimuth a, half beam h, lim = w + 2h; plain IEEE
// float64 in the specified order (the TU is built with -ffp-contract=off), so the host restatement agrees bit for bit.
__device__ __forceinline__ bool in_main_lobe(double beta, double a, double h, double lim, bool full) {
    double off = (beta - a) + h;
    if (off < 0.0) off += 360.0;
    if (off >= 360.0) off -= 360.0;
    return full || off <= lim;
}

// Level of an object under a stepped antenna pattern (include/macjd.h, macjd_scan_pattern_desc): 0 = main lobe (the very
// test of in_main_lobe), 1..L by the distance x to the nearer edge of the covered sector in units of 1 / inv_w, L + 1 beyond
// the last level.  Plain IEEE float64 in the specified order, no division; the conversion acts on min(q, L) (q >= 0 outside
// the main lobe, < 3.6e5 by the host's validation), so q >= L gives 1 + L and no lane converts an out-of-range value.
__device__ __forceinline__ int beam_level(double beta, double a, double h, double lim, bool full, double inv_w, int L) {
    double off = (beta - a) + h;
    if (off < 0.0) off += 360.0;
    if (off >= 360.0) off -= 360.0;
    const double lead = off - lim, trail = 360.0 - off;
    const double x = lead < trail ? lead : trail;
    const double q = x * inv_w;
    const double Ld = (double)L;
    const double qc = (q >= Ld) ? Ld : ((q > 0.0) ? q : 0.0);
    const int k = 1 + (int)qc;
    return (full || off <= lim) ? 0 : k;
}

// Word w (0..3, possibly different per lane) of a block, as shifts on 64-bit pairs.  NOT b.v[w] and not a chain of
// selects on w either: hipcc turns both into a dynamically indexed private array, promotes that array to LDS and, to
// find its slice of it, reads the workgroup size from the dispatch packet — an uncached load from the AQL queue that
// cost the slot kernel 5 - 10 us per launch (3.9 -> 13.6 us at E = 4096; `.amdhsa_user_sgpr_dispatch_ptr 1` in the
// kernel descriptor is the tell-tale).
__device__ __forceinline__ uint32_t philox_word(const Philox4& b, int w) {
    const uint64_t lo = ((uint64_t)b.v[1] << 32) | b.v[0], hi = ((uint64_t)b.v[3] << 32) | b.v[2];
    const uint64_t pair = (w & 2) ? hi : lo;
    return (uint32_t)(pair >> ((w & 1) * 32));
}

}  // namespace macjd

struct macjd_scenario {
    macjd::DevTables host;
    macjd::DevTables* dev;
    int device;
};
