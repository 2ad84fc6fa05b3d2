/*
 * macjd.h — C-ABI of libmacjd_hip.so, the MI355X (gfx950) native library behind the
 * batched radar-jamming environment step.
 *
 * The reference (mfathulkr/MA-CJD-Cooperative-Jamming-Decision-Making-via-MARL) is pure Python
 * and has no FFI layer; its boundary for this path is the object protocol that main.py drives
 * (main.py:137-162,193).  Each entry point below names the reference interface it replaces.
 * Everything is `extern "C"`, plain pointers and sizes; no torch / HIP types in the signatures
 * (streams travel as `void*` holding a hipStream_t).
 *
 * Conventions
 *   - all data buffers are caller-owned DEVICE pointers (e.g. torch tensors' data_ptr());
 *   - entry points never allocate, free or synchronise on the hot path (graph-capture safe),
 *     they enqueue on the given stream and return;
 *   - return 0 on success, a negative MACJD_E* code otherwise; the message is available from
 *     macjd_last_error() (thread-local);
 *   - env arrays are addressed with explicit ELEMENT strides so the caller picks the HBM layout:
 *     env-major [E,J] (se=J, sx=1) as the reference's runner produces it, or agent-major [J,E]
 *     (se=1, sx=E), which is the coalesced layout the batched runner uses.
 */
#ifndef MACJD_H
#define MACJD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MACJD_ABI_VERSION 12
#define MACJD_PE_ROWS(R, J) (6 * (R) + 3 * (J) + (J) * (R))
#define MACJD_PE_SCAN_ROWS(R, J) (10 * (R) + (J) * (R))
#define MACJD_PE_SCAN_PATTERN_ROWS(R, L) ((R) + 4 * ((L) + 2) * (R))

#define MACJD_OK          0
#define MACJD_EINVAL     -1  /* bad argument (shape, NULL, stride)            */
#define MACJD_ENOMEM     -2  /* device / host allocation failed               */
#define MACJD_EDEVICE    -3  /* HIP runtime error (no device, launch failure) */
#define MACJD_EUNSUPPORTED -4

#define MACJD_MAX_RADARS  32
#define MACJD_MAX_JAMMERS 32
#define MACJD_MAX_PATTERN_LEVELS 6

/* jr_flags bits */
#define MACJD_JR_WEAK_DENOM 1u /* denominator was a Python float (d^2 <= 1e-9 branch of
                                  jammer.py:83): NumPy-2 weak promotion keeps the division in
                                  float32 when the power is float32 */

/* macjd_step_io.flags bits */
#define MACJD_STEP_ARITH_F64 1u /* P32 given, but do the power arithmetic in float64
                                   (NumPy-1.x value-based casting / python-float actions) */
/* Kernel choice (results are bit-identical).  Default: the (env x slot) kernel for the templated scenario
   sizes when n_envs < 2^17 (latency regime: shortest critical path), the one-lane-per-env kernel otherwise
   (throughput regime: fewest instructions per env).  These two bits force one variant (A/B + tests). */
#define MACJD_STEP_LANE_KERNEL 2u
#define MACJD_STEP_SLOT_KERNEL 4u

/*
 * Host-side description of one scenario: the static tables the scenario compiler derives from
 * the sim-config YAML.  Replaces the per-step recomputation inside
 * ElectromagneticEnvironment.step (simulation/environment.py:316-333: echo power, SNR without
 * jamming; core/radar.py:35-60; utils/math_utils.py:40-42 distances) — all of it is static
 * because nothing in step() moves an entity (environment.py:237-238 is a TODO).  (Opt-in motion, macjd_motion_io below:
 * one such set of tables per step of an episode; this handle then holds frame 0.)
 * All pointers are HOST pointers, copied by macjd_scenario_create.
 */
typedef struct macjd_scenario_desc {
    int32_t n_radars;       /* R, 1..MACJD_MAX_RADARS  */
    int32_t n_jammers;      /* J, 1..MACJD_MAX_JAMMERS */
    int32_t episode_limit;  /* environment.py:84,460   */
    int32_t reserved;
    double rp_min, rp_max;  /* environment.py:72-73,377 */
    /* Albersheim-style Pd constants, core/radar.py:67-82, evaluated on the host with the
       reference's own expressions so they are bit-identical: A = ln(0.62/prfa),
       c1 = 5 log10(m) / (6.2 + 4.54/sqrt(m) + 0.44), denB = 1.7 + 0.12 A */
    double pd_A, pd_c1, pd_denB;
    const double* radar_GaPs;   /* [R] Ga*Ps               environment.py:320-326, radar.py:35-60 */
    const double* radar_Pn;     /* [R] pn_watts            radar.py:19                            */
    const double* radar_D;      /* [R] anti_jamming_factor radar.py:28                            */
    const double* radar_pd_no;  /* [R] pd(snr_no_jam)      environment.py:385                     */
    const double* radar_snr_no; /* [R] max(0,Ga*Ps/Pn)     environment.py:326-327                 */
    const double* radar_rd_pen; /* [R] clip(-threat, rd_min, rd_max)  environment.py:362-365     */
    const double* radar_gr;     /* [R] receive gain (linear) = get_antenna_gain, radar.py:84-85  */
    const double* jam_pmin;     /* [J] power_min           environment.py:185                     */
    const double* jam_pmax;     /* [J] power_max           environment.py:184                     */
    const double* jam_gj;       /* [J] gain (linear)       jammer.py:44                           */
    const double* jr_denom;     /* [J*R] max(1e-9,d^2)*loss*latm*max(1e-9,bj), jammer.py:83-88;
                                   NEGATIVE when d <= 1e-6 (action ignored, environment.py:284)  */
    const uint8_t* jr_flags;    /* [J*R] MACJD_JR_* */
} macjd_scenario_desc;

typedef struct macjd_scenario macjd_scenario; /* opaque, owns the device copy of the tables */

/*
 * One env-step call.  Replaces ElectromagneticEnvironment.step (simulation/environment.py:221-477)
 * for E environments at once.  Device pointers; NULL where marked optional.
 */
typedef struct macjd_step_io {
    int64_t n_envs;      /* E */
    int64_t env_offset;  /* global index of env 0 (rank shard offset); keys the in-kernel RNG */
    uint64_t seed;       /* Philox key when u == NULL */
    uint32_t flags;      /* MACJD_STEP_* */
    uint32_t reserved;

    /* actions: T = discrete index (environment.py:249-268), P = normalised power (:251,271) */
    const int32_t* T;    int64_t T_se, T_sx;   /* [E,J] element strides (env, agent) */
    const float*   P32;  /* exactly one of P32 / P64 is non-NULL */
    const double*  P64;  int64_t P_se, P_sx;

    /* uniforms replacing np.random.rand() (environment.py:341,430): slot r<R = radar r's
       detection draw, slot R+k = k-th valid deception action (jammer order).  NULL → generated
       in-kernel by Philox4x32-10: one block serves FOUR slots,
         key     = (seed[31:0], seed[63:32] ^ genv[63:32]),            genv = env_offset + e
         counter = (genv[31:0], episode[e], step_before, slot >> 2),
         u       = (word[slot & 3] + 0.5) * 2^-32   (never 0, never 1),
       so every (env, episode, step, slot) has its own value whatever the batch size, the sharding
       over GPUs or the launch geometry. */
    const double* u;     int64_t u_se, u_sx;   /* [E,R+J] */
    /* [E] episode index of each env, optional (NULL = 0): the reference draws fresh np.random.rand()
       values in every episode; macjd_env_reset advances this counter (device memory, so a replayed
       HIP graph advances it too) and the in-kernel generator keys on it.  Unused when u != NULL. */
    const int32_t* episode;

    /* state, read-modify-write */
    uint8_t* track;      int64_t k_se, k_sx;   /* [E,R] 1 = TRACK, 0 = SEARCH (radar.py:90-119) */
    int32_t* step;       /* [E] _step_count (environment.py:235) */

    /* outputs */
    float*   reward;     /* [E]   r_d + r_p + r_j (environment.py:457), may be NULL */
    float*   r_dpj;      /* [E,3] contiguous (r_d, r_p, r_j), may be NULL            */
    uint8_t* terminated; /* [E]   step >= episode_limit (environment.py:460), may be NULL */
    float*   pd;         int64_t pd_se, pd_sx; /* [E,R] info['radar_pds'], may be NULL       */
    float*   snr_with;   int64_t sw_se, sw_sx; /* [E,R] info['snr_with_jamming'], may be NULL */
    /* optional float64 diagnostics (single-env facade + parity tests) */
    double*  out64;      /* [E,4] contiguous (reward, r_d, r_p, r_j) in float64, may be NULL  */
    double*  pd64;       /* [E,R] contiguous, may be NULL */
    double*  snr64;      /* [E,R] contiguous, may be NULL */
    double*  prj64;      /* [E,J] contiguous: received jamming power of jammer j's action if it
                            was recorded in info['jammer_actions'] (environment.py:288-295),
                            else -1; may be NULL */
    /* Per-env scenario tables, optional (radar / jammer positions, threat levels ... randomised per
       env — the mode in which the static scenario parameters carry real HBM bytes).  pe_tables is float64
       [MACJD_PE_ROWS(R,J), pe_stride] row-major: row t of env e at pe_tables[t * pe_stride + e] (consecutive envs are
       consecutive lanes: coalesced).  Row order, same quantities as macjd_scenario_desc:
         GaPs[R] | Pn[R] | D[R] | pd_no[R] | rd_pen[R] | gr[R] | pmin[J] | pmax[J] | gj[J] | denom[J*R] (j-major)
       pe_flags is uint8 [J*R, pe_stride] (MACJD_JR_*).  NULL = every env uses the scenario handle's tables; the
       handle still supplies R, J, episode_limit, the r_p bounds and the Pd constants. */
    const double*  pe_tables;
    const uint8_t* pe_flags;
    int64_t        pe_stride;   /* >= n_envs */
    /* pe_tile > 0 selects the tiled (AoSoA) form of the same tables instead: envs are grouped in tiles of pe_tile
       consecutive envs and a tile's rows are contiguous — row t of env e at
       pe_tables[((e / pe_tile) * MACJD_PE_ROWS + t) * pe_tile + e % pe_tile] (flags alike with J*R rows) — so a
       workgroup that handles pe_tile consecutive envs reads ONE contiguous block per step instead of 6R+3J+JR
       streams pe_stride apart.  pe_stride is ignored then; the last tile is padded. */
    int32_t        pe_tile;
    int32_t        reserved_pe;
    float*   r_dpj_sum;  /* [E,3] contiguous, optional: (r_d, r_p, r_j) of this step are ADDED to it — the
                            per-episode sums behind run_info['avg_r_d'|'avg_r_p'|'avg_r_j']
                            (runners/episode_runner.py:88-90,141-143) without a separate launch */
} macjd_step_io;

/*
 * Scanning radars (opt-in, sim-config `environment_params.radar_scan`): every radar's beam has an azimuth theta_a that
 * the step advances, and the target / a jammer outside the main lobe is seen with the side-lobe gain.  Host-derived
 * float64 tables per radar r (dt = step_seconds, rho = 10^(sidelobe_db / 10), wrap(x) = x - 360 floor(x / 360)):
 *   half_beam = theta_m / 2, sweep = 360 dt / t_s, sweep_mod = fmod(sweep, 360), full = (sweep + 2 half_beam >= 360),
 *   az0 = wrap(theta_a), bear_tgt = wrap(deg(atan2(ty - ry, tx - rx))), bear_jam[j*R + r] likewise for jammer j,
 *   GaPs_side = GaPs rho^2 (two-way), gr_side = gr rho, snr_no / pd_no of GaPs_side by the host expressions of the
 *   main tables.  Per step, with a = theta_a[e,r] and s = track[e,r] at its start, an object at bearing b is in the
 *   main lobe iff  full || off <= w + 2 half_beam,  w = s ? 0 : sweep,  off = (b - a) + half_beam wrapped once into
 *   [0, 360) by +-360 (plain IEEE float64, no division: host and device agree bit for bit).  The target path takes the
 *   main or the _side (GaPs, snr_no, pd_no); a jammer acting on radar r takes gr or gr_side by its own bearing.  The
 *   beam then moves: detected -> a' = bear_tgt; TRACK before -> a' = a; else a' = a + sweep_mod, minus 360 if >= 360.
 *   Everything else is macjd_env_step's arithmetic, RNG slots and Philox keying.  The outcome now depends on the past
 *   through theta_a and track: macjd_env_step_many does not apply.
 */
typedef struct macjd_scan_desc {
    int32_t n_radars, n_jammers;   /* must equal the scenario's */
    const double* half_beam;       /* [R] */
    const double* sweep;           /* [R] */
    const double* sweep_mod;       /* [R] */
    const uint8_t* full;           /* [R] 0 / 1 */
    const double* az0;             /* [R] wrap(theta_a)                                                   */
    const double* bear_tgt;        /* [R] wrap(...): [0, 360], 360 only from a tiny negative angle's rounding */
    const double* bear_jam;        /* [J*R] j-major, likewise                                             */
    const double* GaPs_side;       /* [R] */
    const double* snr_no;          /* [R] main-lobe SNR without jamming (= macjd_scenario_desc.radar_snr_no) */
    const double* snr_no_side;     /* [R] */
    const double* pd_no_side;      /* [R] */
    const double* gr_side;         /* [R] */
} macjd_scan_desc;

/*
 * Stepped antenna pattern of a scanning radar (opt-in, sim-config `radar_scan.pattern`): between the main lobe and the
 * far side lobe lie L = 1..MACJD_MAX_PATTERN_LEVELS levels, each `level_width` half beam widths wide, with their own
 * one-way gains.  With off, lim = w + 2 half_beam, full as in macjd_scan_desc, an object's level at radar r is
 *   0 (main)            if  full || off <= lim;  otherwise, with
 *   lead = off - lim,  trail = 360.0 - off,  x = lead < trail ? lead : trail   (distance to the nearer edge of the covered
 *   sector),  q = x * inv_width[r],   inv_width[r] = 1.0 / (level_width * half_beam[r])  (host, float64),
 *   k = (q >= (double)L) ? L + 1 : 1 + (int)q.
 * Plain IEEE float64 in this order, no division and no transcendental on the device: host and device agree bit for bit.
 * Levels 1..L have the one-way gain rho_k = 10^(gain_db[k-1] / 10); their tables come from the host expressions of the
 * side-lobe tables (gr_k = gr rho_k, GaPs_k = GaPs rho_k^2, snr_no_k / pd_no_k of GaPs_k); level L + 1 is the side lobe of
 * macjd_scan_desc.  The target path of radar r takes the level-k (GaPs, snr_no, pd_no); a jammer acting on radar r takes
 * gr_k by its own bearing.  Beam advance, RNG slots, Philox keying and everything else are unchanged; without pattern
 * tables (L = 0) the model is macjd_scan_desc's.  Host pointers; the level tables are level-major: level k (1..L) of
 * radar r at [(k - 1) * R + r].
 */
typedef struct macjd_scan_pattern_desc {
    int32_t n_radars;              /* must equal the scenario's */
    int32_t n_levels;              /* L, 1..MACJD_MAX_PATTERN_LEVELS */
    const double* inv_width;       /* [R] finite, > 0 */
    const double* GaPs_lvl;        /* [L*R] */
    const double* snr_no_lvl;      /* [L*R] */
    const double* pd_no_lvl;       /* [L*R] */
    const double* gr_lvl;          /* [L*R] */
} macjd_scan_pattern_desc;

/* Per-call state of a scanning step / reset.  Device pointers. */
typedef struct macjd_scan_io {
    double* theta_a;  int64_t a_se, a_sx;   /* [E,R] beam azimuth in degrees, read-modify-write */
    float*  state;    int64_t st_se;        /* optional [E,S] state rows: column st_col0 + r * st_col_step gets  */
    int32_t st_col0, st_col_step;           /* (float)theta_a[e,r] after the step (reset: (float)az0[r])          */
    float*  snr_no;   int64_t sn_se, sn_sx; /* optional [E,R] per-step SNR without jamming (main or side lobe)     */
} macjd_scan_io;

/*
 * Per-env scanning tables of a step / reset on per-env scenario tables (macjd_step_io.pe_tables): every env has its own
 * macjd_scan_desc quantities.  `tables` is a float64 device array of MACJD_PE_SCAN_ROWS(R, J) rows in the order
 *   half_beam[R] | sweep[R] | sweep_mod[R] | az0[R] | bear_tgt[R] | GaPs_side[R] | snr_no[R] | snr_no_side[R] |
 *   pd_no_side[R] | gr_side[R] | bear_jam[J*R] (j-major)
 * laid out like the step's own pe_tables: plain (pe_tile == 0), row t of env e at tables[t * stride + e]; tiled
 * (pe_tile > 0), at tables[((e / pe_tile) * MACJD_PE_SCAN_ROWS + t) * pe_tile + e % pe_tile], the last tile padded, stride
 * ignored.  `full` is not carried: it equals (sweep + 2 half_beam >= 360.0) in float64 (2 half_beam is exact), which the
 * device recomputes with the same bits.  The main-lobe GaPs / pd_no / gr are those of pe_tables.
 */
typedef struct macjd_scan_pe_io {
    const double* tables;
    int64_t stride;   /* >= n_envs when pe_tile == 0 */
} macjd_scan_pe_io;

/*
 * Per-env stepped antenna pattern of a scanning step on per-env scenario tables (macjd_env_step_scan_pe_pattern): every env
 * has its own macjd_scan_pattern_desc quantities; L = n_levels is shared by the batch.  `tables` is a float64 device array of
 * MACJD_PE_SCAN_PATTERN_ROWS(R, L) rows in the order
 *   inv_width[R] | GaPs_lvl[(L+2)*R] | snr_no_lvl[(L+2)*R] | pd_no_lvl[(L+2)*R] | gr_lvl[(L+2)*R]
 * each level table level-major, level k of radar r at row k * R + r of its block: level 0 holds the env's main-lobe values
 * (the bits of its pe_tables GaPs / pd_no / gr rows and of macjd_scan_pe_io's snr_no row), levels 1..L the pattern's
 * (macjd_scan_pattern_desc), level L + 1 its side-lobe values (the bits of macjd_scan_pe_io's _side rows) — so the device
 * picks an object's level with one address-selected load per table.  Laid out like the step's own pe_tables: plain
 * (pe_tile == 0), row t of env e at tables[t * stride + e]; tiled (pe_tile > 0), at
 * tables[((e / pe_tile) * MACJD_PE_SCAN_PATTERN_ROWS + t) * pe_tile + e % pe_tile], the last tile padded, stride ignored.
 */
typedef struct macjd_scan_pe_pattern_io {
    const double* tables;
    int64_t stride;     /* >= n_envs when pe_tile == 0 */
    int32_t n_levels;   /* L, 1..MACJD_MAX_PATTERN_LEVELS */
    int32_t reserved;
} macjd_scan_pe_pattern_io;

/*
 * Moving entities (opt-in, sim-config `environment_params.motion`): target, radars and jammers move with constant
 * velocities that do not depend on the actions, so every distance-dependent table is a pure function of the step counter.
 * The host compiles one FRAME per step of an episode: frame k is the static scenario whose positions are, per axis,
 * p0 + k (v dt) in float64 (dt = step_seconds), compiled like any other scenario (macjd_scenario_desc).  Device arrays:
 *   frames       float64 [n_frames, MACJD_PE_ROWS(R,J)], frame-major: row t of frame f at frames[f * MACJD_PE_ROWS + t], rows
 *                in the order of macjd_step_io.pe_tables (GaPs | Pn | D | pd_no | rd_pen | gr | pmin | pmax | gj | denom) —
 *                the tiled per-env layout at tile width 1 with the frame index as the tile index: one env-step reads one
 *                contiguous block;
 *   frame_flags  uint8 [n_frames, J*R] (MACJD_JR_*), flag i of frame f at frame_flags[f * J*R + i];
 *   frame_snr_no float64 [n_frames, R], optional (needed for snr_no): max(0, GaPs / Pn) of each frame as the host formed it;
 *   positions    float32 [n_frames + 1, n_pos], n_pos = 2R + 2J: the position entries of frame k's state vector in state
 *                order (per radar x, y; then per jammer x, y);
 *   position_columns int32 [n_pos]: their columns in a state row.
 * A step whose counter is k before it (for item t of a many-step launch: step[e] + t) runs macjd_env_step's arithmetic,
 * order, RNG slots, Philox keying and stores on frame f = min(k, n_frames - 1) — the positions the agents saw when they
 * chose the action.  The entities then move: the same launch copies positions[min(k + 1, n_frames)] into the env's state
 * row at position_columns (plain stores; every other column is left alone) and, when snr_no is given, writes
 * (float)frame_snr_no[f] to it.  Results are bit-identical to macjd_env_step on per-env tables (pe_tables) whose column for
 * env e holds frame f_e, in the same (production or general all-float64) form.  The target is not part of the state
 * vector: its motion acts through the tables only.  A step's outcome still depends on the past through the step counter
 * alone, so the many-step launch stays legal (macjd_env_step_many_moving).  n_frames = the scenario's episode_limit.
 */
typedef struct macjd_motion_io {
    const double*  frames;
    const uint8_t* frame_flags;
    const double*  frame_snr_no;      /* optional unless snr_no is given */
    const float*   positions;
    const int32_t* position_columns;
    int32_t n_frames;                 /* F >= 1 */
    int32_t n_pos;                    /* must equal 2R + 2J */
    float*  state;    int64_t st_se;  /* [E,S] state rows, row stride in elements.  position_columns lives on the device, so
                                         the library cannot check it: the CALLER guarantees 0 <= column < st_se for all
                                         n_pos entries (a column outside the row is written out of bounds) */
    float*  snr_no;   int64_t sn_se, sn_sx;   /* optional [E,R] SNR without jamming of the frame used; single steps only */
} macjd_motion_io;

/*
 * Moving entities WITH scanning beams (sim-config `environment_params.motion` and `radar_scan` on one clock: both
 * `step_seconds` equal, one env step is one dt for the beams and for the entities).  Frame k is the static SCANNING scenario
 * at positions p0 + k (v dt), so the beams' tables are per-step frames too.  Device arrays:
 *   scan_frames    float64 [n_frames, MACJD_PE_SCAN_ROWS(R,J)], frame-major, rows in the order of macjd_scan_pe_io.tables;
 *   pattern_frames float64 [n_frames, MACJD_PE_SCAN_PATTERN_ROWS(R,L)], frame-major, rows in the order of
 *                  macjd_scan_pe_pattern_io.tables; given exactly when n_levels > 0 (a stepped antenna pattern).
 * Row f of each holds the bits of the per-env column of frame f's compiled scenario.  n_frames is macjd_motion_io's.
 */
typedef struct macjd_motion_scan_io {
    const double* scan_frames;      /* [n_frames, MACJD_PE_SCAN_ROWS(R,J)], frame-major */
    const double* pattern_frames;   /* optional [n_frames, MACJD_PE_SCAN_PATTERN_ROWS(R,L)] */
    int32_t n_levels, reserved;     /* L, 0 without pattern_frames */
} macjd_motion_scan_io;

/*
 * PER-ENV moving scenarios (opt-in): macjd_motion_io with every table per env — each env has its own trajectory, so its
 * frame f is its own static scenario at p0_e + f (v_e dt).  The tables are the per-env tiled layout (macjd_step_io.pe_tile)
 * with the frame index between tile and row; envs are grouped in tiles of `tile` consecutive envs, the last tile padded:
 *   frames       float64 [n_tiles, F, MACJD_PE_ROWS(R,J), tile]: row t of frame f of env e at
 *                frames[(((e / tile) * F + f) * MACJD_PE_ROWS + t) * tile + e % tile], rows in the order of pe_tables;
 *   frame_flags  uint8   [n_tiles, F, J*R, tile]   (MACJD_JR_*), likewise;
 *   frame_snr_no float64 [n_tiles, F, R, tile], optional (needed for snr_no), likewise;
 *   positions    float32 [n_tiles, F + 1, n_pos, tile], likewise with F + 1 frames per tile.
 * A wave whose envs are on one frame reads whole contiguous row pieces; envs on different frames (after individual resets)
 * still read their own columns.  position_columns, n_frames, n_pos, state / st_se, snr_no and the clamps are macjd_motion_io's:
 * the step runs on frame min(k, F - 1), positions come from frame min(k + 1, F).
 */
typedef struct macjd_motion_pe_io {
    const double*  frames;
    const uint8_t* frame_flags;
    const double*  frame_snr_no;      /* optional unless snr_no is given */
    const float*   positions;
    const int32_t* position_columns;  /* int32 [n_pos], shared by the batch */
    int32_t n_frames;                 /* F >= 1 */
    int32_t n_pos;                    /* must equal 2R + 2J */
    int32_t tile;                     /* >= 1: envs per tile */
    int32_t reserved;
    float*  state;    int64_t st_se;  /* as macjd_motion_io: the CALLER guarantees 0 <= column < st_se */
    float*  snr_no;   int64_t sn_se, sn_sx;   /* optional [E,R]; single steps only */
} macjd_motion_pe_io;

/*
 * The device frame compiler of per-env moving scenarios (macjd_motion_pe_compile): ONE launch, item (e, f) for f in 0..F
 * writes frame f of env e into the four tables of macjd_motion_pe_io (f = F: the positions only).  Its input is one column
 * per env, float64 [n_tiles, MACJD_MOTION_PE_IN_ROWS(R,J), tile] in the same tiled layout (row t of env e at
 * in_tables[((e / tile) * MACJD_MOTION_PE_IN_ROWS + t) * tile + e % tile]), rows in the order
 *   Pn[R] | D[R] | rd_pen[R] | gr[R] | echo_num[R] | r_loss[R] | r_latm[R] | Ga[R] |
 *   pmin[J] | pmax[J] | gj[J] | j_loss[J] | j_latm[J] | bj_eff[J] |
 *   tgt_p0[2] | tgt_vdt[2] | radar_p0[2R] | radar_vdt[2R] | jam_p0[2J] | jam_vdt[2J]      (x, y per entity)
 * Pn, D, rd_pen, gr, pmin, pmax, gj are the env's distance-independent pe_tables rows and are copied through unchanged;
 * echo_num = pt gt gr lambda^2 rcs as the host's scenario compiler forms it, r_loss / r_latm / Ga the radar's linear loss
 * factors and pulse-compression gain; j_loss / j_latm the jammer's, bj_eff = max(1e-9, bj); p0 the float64 position at frame
 * 0 and vdt the host's float(v[a]) * dt per axis.  in_weak is uint8 [n_tiles, J, tile]: 1 when the product
 * 1e-9 * j_loss * j_latm * bj_eff is a Python float on the host (MACJD_JR_WEAK_DENOM's rule, which then depends on the
 * distance only).  Arithmetic of an item, plain IEEE float64 in this order (no fused multiply-add), fd = (double)f:
 *   position per axis  p = p0 + fd * vdt;  the positions table gets (float)p in state order (radars, then jammers);
 *   radar r:  dx, dy to the target;  d = sqrt(dx*dx + dy*dy);  sd = max(d, 1e-6);  d4 = (sd*sd)*(sd*sd);
 *             den = ((c0*d4)*r_loss)*r_latm, c0 = four_pi_cubed;  Ps = den <= 1e-18 ? 0 : echo_num/den;  GaPs = Ga*Ps;
 *             snr_no = max(0, Pn > 1e-18 ? GaPs/Pn : 0);  pd_no = the all-float64 detection probability of the step
 *             kernels (|denB| < 1e-9 -> 0, B > 700 -> 1, B < -700 -> 0 included);
 *   jammer j, radar r:  d likewise;  !(d > 1e-6): denom = -1.0, flag = 0;  otherwise d2 = d*d, dsq = d2 > 1e-9 ? d2 : 1e-9,
 *             denom = ((dsq*j_loss)*j_latm)*bj_eff, flag bit 0 = !(d2 > 1e-9) && in_weak[j].
 * Lanes of the last tile's padding and bytes outside the tables are not written.
 */
#define MACJD_MOTION_PE_IN_ROWS(R, J) (12 * (R) + 10 * (J) + 4)
typedef struct macjd_motion_pe_compile_desc {
    int64_t n_envs;                /* E */
    int32_t n_radars, n_jammers;   /* R, J */
    int32_t n_frames;              /* F, 1..65534 */
    int32_t tile;                  /* >= 1 */
    double  four_pi_cubed;         /* (4 pi)^3 as the host evaluates it */
    double  pd_A, pd_c1, pd_denB;  /* the Pd constants of macjd_scenario_desc */
    const double*  in_tables;
    const uint8_t* in_weak;
    double*  frames;
    uint8_t* frame_flags;
    double*  frame_snr_no;         /* optional */
    float*   positions;
} macjd_motion_pe_compile_desc;

/*
 * PER-ENV moving scenarios under SCANNING radars (opt-in): the beam tables of macjd_motion_scan_io in the tiled per-env layout
 * of macjd_motion_pe_io, the frame index between tile and row (tile = macjd_motion_pe_io.tile, F = its n_frames):
 *   scan_frames    float64 [n_tiles, F, MACJD_PE_SCAN_ROWS(R,J), tile], rows in the order of macjd_scan_pe_io.tables;
 *   pattern_frames float64 [n_tiles, F, MACJD_PE_SCAN_PATTERN_ROWS(R,L), tile], rows in the order of
 *                  macjd_scan_pe_pattern_io.tables; given exactly when n_levels > 0.
 * Row t of frame f of env e at table[(((e / tile) * F + f) * ROWS + t) * tile + e % tile]; the last tile is padded.
 */
typedef struct macjd_motion_scan_pe_io {
    const double* scan_frames;
    const double* pattern_frames;   /* optional */
    int32_t n_levels, reserved;     /* L, 0 without pattern_frames */
} macjd_motion_scan_pe_io;

/*
 * The device compiler of the beam frames (macjd_motion_scan_pe_compile): ONE launch, item (e, f) for f in 0..F-1 writes the
 * scan rows (and, L > 0, the level rows) of frame f of env e.  It runs AFTER macjd_motion_pe_compile on the same stream and
 * reads that compiler's outputs — the GaPs, Pn, pd_no and gr rows of `frames` and `frame_snr_no` (required here) — its
 * input `in_tables` (the float64 start positions and v dt rows), and one more column per env, scan_in, float64
 * [n_tiles, MACJD_MOTION_SCAN_PE_IN_ROWS(R,L), tile] in the same tiled layout, rows in the order
 *   half_beam[R] | sweep[R] | sweep_mod[R] | az0[R] | rho | inv_width[R] | rho_lvl[L]      (the last two blocks only when L > 0)
 * with rho = 10^(sidelobe_db / 10), rho_lvl[k] = 10^(gain_db[k] / 10) and inv_width as the host's scan compiler forms them.
 * Arithmetic of an item, plain IEEE float64 in this order (no fused multiply-add), fd = (double)f:
 *   position per axis  p = p0 + fd * vdt   (macjd_motion_pe_compile's expression: the same bits);
 *   bearing of object o from radar r:  a = atan2(oy - ry, ox - rx);  d = a * deg_per_rad;  b = d - 360.0 * floor(d / 360.0);
 *             bear_tgt[r] takes the target, bear_jam[j * R + r] jammer j;
 *   side lobe: gr_side = gr * rho;  GaPs_side = GaPs * (rho * rho);  snr_no_side = max(0, Pn > 1e-18 ? GaPs_side / Pn : 0);
 *             pd_no_side = the all-float64 detection probability of the step kernels;
 *   levels k = 1..L: the same four expressions with rho_lvl[k - 1];
 *   copies, bits unchanged: level 0 = the main rows (GaPs, frame_snr_no, pd_no, gr), level L + 1 = the side rows; half_beam,
 *             sweep, sweep_mod, az0 and inv_width copied through; the snr_no row = the frame's frame_snr_no.
 * The device library's atan2 is the only step IEEE 754 does not pin: bearings agree with the host within rounding, every
 * other row but the pd_no rows bit for bit.  Lanes of the last tile's padding and bytes outside the tables are not written.
 */
#define MACJD_MOTION_SCAN_PE_IN_ROWS(R, L) (4 * (R) + 1 + ((L) > 0 ? (R) + (L) : 0))
typedef struct macjd_motion_scan_pe_compile_desc {
    int64_t n_envs;                /* E */
    int32_t n_radars, n_jammers;   /* R, J */
    int32_t n_frames;              /* F, 1..65534 */
    int32_t tile;                  /* >= 1 */
    int32_t n_levels, reserved;    /* L, 0..MACJD_MAX_PATTERN_LEVELS */
    double  deg_per_rad;           /* 180 / pi as the host evaluates it */
    double  pd_A, pd_c1, pd_denB;  /* the Pd constants of macjd_scenario_desc */
    const double* in_tables;       /* macjd_motion_pe_compile_desc.in_tables */
    const double* scan_in;
    const double* frames;          /* written by macjd_motion_pe_compile */
    const double* frame_snr_no;    /* likewise; required */
    double* scan_frames;
    double* pattern_frames;        /* exactly when n_levels > 0 */
} macjd_motion_scan_pe_compile_desc;

/* library / device */
int         macjd_abi_version(void);
const char* macjd_last_error(void);
/* The library reads its MACJD_* environment switches (MACJD_ENV_REGULAR, MACJD_ENV_PD32, MACJD_GRU_SCAN) once, at the first
 * launch; call this after changing one of them inside a running process (tests, A/B timing). */
void        macjd_reload_options(void);
int         macjd_device_count(void);   /* number of HIP devices, <0 on error */

/* scenario handle: replaces ElectromagneticEnvironment.__init__/_initialize_entities
   (environment.py:35-206) as far as the device is concerned */
int  macjd_scenario_create(const macjd_scenario_desc* host_desc, macjd_scenario** out);
void macjd_scenario_destroy(macjd_scenario* s);
int  macjd_scenario_dims(const macjd_scenario* s, int32_t* n_radars, int32_t* n_jammers,
                         int32_t* episode_limit);
/* 1 when the scenario's tables are REGULAR: every value a division of the step can meet lies in [1e-30, 1e30] (or is an
   exact zero where that is harmless), noise powers are positive, the detection-probability argument cannot fall below
   -700.  The production lane kernel then divides by table values through reciprocals refined on the device when the
   scenario was created and drops the guards that cannot trigger — bit-identical results (tests), ~16 % fewer
   instructions.  Irregular scenarios run the IEEE-division form of the same kernel; MACJD_ENV_REGULAR=0 forces it. */
int  macjd_scenario_is_regular(const macjd_scenario* s);

/* replaces ElectromagneticEnvironment.reset (environment.py:208-219): all radars SEARCH,
   step counter 0.  mask (optional, [E] uint8) restricts the reset to envs with mask != 0.
   episode (optional, [E] int32): the reset envs' episode index is incremented (see
   macjd_step_io.episode). */
int macjd_env_reset(const macjd_scenario* s, int64_t n_envs, uint8_t* track, int64_t k_se,
                    int64_t k_sx, int32_t* step, const uint8_t* mask, int32_t* episode,
                    void* hip_stream);

/* replaces ElectromagneticEnvironment.step (environment.py:221-477) */
int macjd_env_step(const macjd_scenario* s, const macjd_step_io* io, void* hip_stream);

/* copies the scanning tables into the handle (host call, synchronous; not for the hot path) */
int macjd_scenario_set_scan(macjd_scenario* s, const macjd_scan_desc* d);
/* adds the stepped antenna pattern's level tables to a scanning handle (host call, synchronous; after
   macjd_scenario_set_scan, which drops an earlier pattern).  macjd_env_step_scan and macjd_agent_env_episode_scan then
   launch their pattern variants: no other call changes. */
int macjd_scenario_set_scan_pattern(macjd_scenario* s, const macjd_scan_pattern_desc* d);
/* macjd_env_step with scanning beams (see macjd_scan_desc); needs macjd_scenario_set_scan first.  Always the one-lane-
   per-env kernel; per-env scenario tables (pe_tables) are refused here: macjd_env_step_scan_pe takes them.  (Likewise the
   closed-loop launch, include/macjd_nets.h: macjd_agent_env_episode_scan refuses pe_tables, macjd_agent_env_episode_scan_pe
   takes them; macjd_env_step_many and the whole-episode launches on a static observation do not apply to scanning beams.) */
int macjd_env_step_scan(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan, void* hip_stream);
/* beam part of a reset, issued next to macjd_env_reset with the same mask: theta_a[e,:] = az0 (and the state
   columns = (float)az0) for envs with mask != 0 (all when mask == NULL) */
int macjd_env_reset_scan(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan, const uint8_t* mask,
                         void* hip_stream);

/* macjd_env_step_scan on per-env scenario tables: needs io->pe_tables (with io->pe_tile choosing the layout of both table
   sets) and a scanning handle WITHOUT pattern levels; the handle supplies R, J, episode_limit, the r_p bounds and the Pd
   constants, every table value comes from the env's own columns.  Results are bit-identical to a single-scenario
   macjd_env_step_scan of the same env in its all-float64 form (MACJD_ENV_PD32=0). */
int macjd_env_step_scan_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan,
                           const macjd_scan_pe_io* scan_pe, void* hip_stream);
/* macjd_env_reset_scan with az0 from each env's column: theta_a[e,r] = az0_e[r], state columns = (float)az0_e[r] */
int macjd_env_reset_scan_pe(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan, const macjd_scan_pe_io* scan_pe,
                            int32_t pe_tile, const uint8_t* mask, void* hip_stream);

/* macjd_env_step_scan_pe under a stepped antenna pattern whose level tables differ per env: needs io->pe_tables and a
   scanning handle; the handle supplies only R, J, episode_limit, the r_p bounds and the Pd constants — every level value
   comes from the env's column of `pattern`, the handle's own level tables are never read (a handle that has pattern levels
   is accepted only if its L equals pattern->n_levels).  Results are bit-identical to a single-scenario macjd_env_step_scan
   of the same env with macjd_scenario_set_scan_pattern, in its all-float64 form (MACJD_ENV_PD32=0).  The reset is
   macjd_env_reset_scan_pe on a handle without pattern levels: az0 does not depend on the pattern. */
int macjd_env_step_scan_pe_pattern(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan,
                                   const macjd_scan_pe_io* scan_pe, const macjd_scan_pe_pattern_io* pattern, void* hip_stream);

/* T consecutive steps of all E environments in ONE launch, given the actions of all T steps (time-major: step t of
   env e at offset t * t_stride + e * se + k * sx of T / P32; outputs reward / terminated / r_dpj likewise at
   t * n_envs + e, pd / snr_with are not written).  Legal because a step's outcome depends on the environment's past
   only through the step counter: the FSM's next state equals `detected` whatever the previous state (core/radar.py:
   102-117), nothing else is carried over (environment.py:221-477).  So when the actions do not depend on the env's
   outputs — the observation is static, environment.py:479-522 — the T x E env-steps of an episode batch are
   independent work items: virtual env v = t * E + e runs (env e, step step[e] + t) in the streaming lane kernel.
   `track` and `step` end as after the last step; io->r_dpj_sum gets the sums over the T steps.  Production
   configuration only (Philox uniforms, float32 actions); io->u, P64 and the float64 diagnostics must be NULL. */
int macjd_env_step_many(const macjd_scenario* s, const macjd_step_io* io, int32_t n_steps, int64_t t_stride,
                        void* hip_stream);

/* macjd_env_step for a moving scenario (see macjd_motion_io): the table column is chosen by the env's step counter.
   io->pe_tables must be NULL; the handle supplies R, J, episode_limit, the r_p bounds and the Pd constants, every table
   value comes from the frame.  One lane per env; compiled sizes 2j/2r, 3j/4r, 6j/8r have production and general variants,
   every other size runs the generic-size kernel. */
int macjd_env_step_moving(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion, void* hip_stream);
/* macjd_env_step_many for a moving scenario: same contract and restrictions (production configuration, compiled sizes with
   a production variant); item (t, e) runs frame min(step[e] + t, n_frames - 1); state rows end as after the last step;
   motion->snr_no must be NULL. */
int macjd_env_step_many_moving(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion,
                               int32_t n_steps, int64_t t_stride, void* hip_stream);
/* position part of a reset, issued next to macjd_env_reset with the same mask: frame-0 positions into the state rows of
   the envs with mask != 0 (all when mask == NULL) */
int macjd_env_reset_moving(const macjd_scenario* s, int64_t n_envs, const macjd_motion_io* motion, const uint8_t* mask,
                           void* hip_stream);

/* macjd_env_step_moving on PER-ENV frame tables (see macjd_motion_pe_io): env e runs frame f_e = min(step[e], F - 1) of its
   OWN tables.  io->pe_tables must be NULL; the handle supplies R, J, episode_limit, the r_p bounds and the Pd constants.
   Bit-identical to macjd_env_step on pe_tables whose column for env e holds env e's frame f_e, in the same (production or
   general all-float64) form.  Sizes and variants as macjd_env_step_moving. */
int macjd_env_step_moving_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_pe_io* motion_pe,
                             void* hip_stream);
/* macjd_env_step_many_moving on per-env frame tables: same contract and restrictions; motion_pe->snr_no must be NULL. */
int macjd_env_step_many_moving_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_pe_io* motion_pe,
                                  int32_t n_steps, int64_t t_stride, void* hip_stream);
/* macjd_env_reset_moving on per-env frame tables: each masked env's own frame-0 positions into its state row */
int macjd_env_reset_moving_pe(const macjd_scenario* s, int64_t n_envs, const macjd_motion_pe_io* motion_pe, const uint8_t* mask,
                              void* hip_stream);
/* the device frame compiler of per-env moving scenarios (see macjd_motion_pe_compile_desc): one launch, no handle */
int macjd_motion_pe_compile(const macjd_motion_pe_compile_desc* desc, void* hip_stream);

/* The env step of a moving scenario with scanning beams (see macjd_motion_scan_io); needs a scanning handle
   (macjd_scenario_set_scan).  A step whose counter is k before it runs the arithmetic, order, RNG slots and Philox keying of
   macjd_env_step_scan_pe (macjd_env_step_scan_pe_pattern when pattern_frames is given) on frame f = min(k, n_frames - 1):
   the step's own rows from motion->frames / frame_flags, every scan row from scan_frames, the level rows from
   pattern_frames; the handle supplies R, J, episode_limit, the r_p bounds and the Pd constants (pattern levels of the handle
   are accepted only if their L equals n_levels, and are never read).  The beams advance as macjd_scan_desc says, with
   bear_tgt of frame f: a beam that keeps detecting follows a moving target one frame behind.  The same launch then writes
   (float)theta_a' into scan->state's theta_a columns (when given), positions[min(k + 1, n_frames)] into the position
   columns of motion->state, and the per-step SNR without jamming into scan->snr_no (when given).  io->pe_tables and
   motion->snr_no must be NULL; scan->state, when given, must equal motion->state.  Results are bit-identical to
   macjd_env_step_scan_pe(_pattern) on per-env tables whose column for env e holds frame f_e, in the same (production or
   general all-float64) form.  The outcome depends on the past through theta_a, so there is no many-step form; the reset is
   macjd_env_reset + macjd_env_reset_scan + macjd_env_reset_moving with one mask (az0 does not depend on the frame).
   One lane per env; sizes and variants as macjd_env_step_moving. */
int macjd_env_step_moving_scan(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion,
                               const macjd_scan_io* scan, const macjd_motion_scan_io* motion_scan, void* hip_stream);

/* macjd_env_step_moving_scan on PER-ENV frame tables (see macjd_motion_pe_io, macjd_motion_scan_pe_io): env e runs frame
   f_e = min(step[e], F - 1) of its OWN tables — the step's rows from motion_pe->frames / frame_flags, every scan row from
   scan_frames, the level rows from pattern_frames — with bear_tgt of that frame, and the same launch writes (float)theta_a'
   into scan->state's theta_a columns (when given), positions of frame min(step[e] + 1, F) into the position columns of
   motion_pe->state and the per-step SNR without jamming into scan->snr_no (when given).  io->pe_tables and
   motion_pe->snr_no must be NULL; scan->state, when given, must equal motion_pe->state; the handle must be a scanning handle
   (pattern levels of the handle are accepted only if their L equals n_levels, and are never read).  Results are bit-identical
   to macjd_env_step_scan_pe(_pattern) on per-env tables whose column for env e holds env e's frame f_e, in the same
   (production or general all-float64) form.  The outcome depends on the past through theta_a: there is no many-step form.
   One lane per env; sizes and variants as macjd_env_step_moving. */
int macjd_env_step_moving_scan_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_pe_io* motion_pe,
                                  const macjd_scan_io* scan, const macjd_motion_scan_pe_io* motion_scan_pe, void* hip_stream);
/* beam part of a reset on per-env beam frames, issued next to macjd_env_reset and macjd_env_reset_moving_pe with the same
   mask: theta_a[e,r] = the az0 row of env e's frame 0 (and the state columns = (float)az0) for envs with mask != 0 */
int macjd_env_reset_moving_scan_pe(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan,
                                   const macjd_motion_scan_pe_io* motion_scan_pe, int32_t n_frames, int32_t tile,
                                   const uint8_t* mask, void* hip_stream);
/* the device compiler of the beam frames (see macjd_motion_scan_pe_compile_desc): one launch after macjd_motion_pe_compile
   on the same stream, no handle */
int macjd_motion_scan_pe_compile(const macjd_motion_scan_pe_compile_desc* desc, void* hip_stream);

/* timing helper for bench.py: `iters` back-to-back env_step launches, replayed from one HIP graph on a private
   stream after the work queued on `hip_stream` has finished (as the benchmark's rollout replays them, so the
   host's enqueue rate does not enter; issued directly on `hip_stream` if the capture is refused), bracketed by
   HIP events recorded on the stream the launches run on; waits and returns the average milliseconds per
   launch in *ms_per_launch. */
int macjd_env_step_timed(const macjd_scenario* s, const macjd_step_io* io, int iters,
                         void* hip_stream, float* ms_per_launch);

/* the same for the main kernel of macjd_env_step_many (n_steps x n_envs work items per launch; the counter-advance
   launch is not part of the replayed graph, so every replay does identical work) */
int macjd_env_step_many_timed(const macjd_scenario* s, const macjd_step_io* io, int32_t n_steps, int64_t t_stride,
                              int iters, void* hip_stream, float* ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* MACJD_H */
