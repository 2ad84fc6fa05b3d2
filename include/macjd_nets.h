/*
 * macjd_nets.h — C-ABI of the fused agent-side kernels in libmacjd_hip.so (MI355X / gfx950).
 *
 * The reference has no native layer; the interfaces replaced here are Python call sites:
 *   macjd_qhead_select   BasicMAC.select_actions' multi-pass loop + mask + epsilon-greedy + gather
 *                        (reference core/mac.py:109-164, utils/action_selectors.py:15-62) and the
 *                        per-action loop of QMixLearner._get_all_action_q_values_and_params
 *                        (core/qmix.py:256-274), both built on RNNAgent.get_q_value_for_action
 *                        (core/networks.py:131-180);
 *   macjd_gru_sequence   the learner's `for t in range(max_seq_len)` GRU unroll
 *                        (core/qmix.py:241-253 -> core/networks.py:88-114);
 *   macjd_mixer_tail_*   QMixer.forward after the hyper-network GEMMs, and its backward
 *                        (core/networks.py:283-315);
 *   macjd_td_loss        TD target + masked MSE + its gradient + logged means (core/qmix.py:155,190-194,212-213).
 * Device pointers, element strides, no torch / HIP types; asynchronous on the given stream.
 */
#ifndef MACJD_NETS_H
#define MACJD_NETS_H

#include <stdint.h>

#include "macjd.h"   /* macjd_scenario, macjd_scan_io (macjd_agent_env_episode_scan) */

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Q(h, a, P[:,a]) for every discrete action a in one pass, optionally followed by availability
 * masking, epsilon-greedy choice and the gather of the chosen power.
 *
 * The Q-head's first layer is W1 [H, H+A+1] applied to cat([h, onehot(a), P_a]) (networks.py:75-79,
 * 171-174).  The caller supplies base = W1[:, :H] h + b1 (one GEMM, [N,H]); the kernel adds the
 * action column W1[:, H+a] and the rank-1 power term W1[:, H+A] * P_a, applies ReLU and the second
 * layer (w2, b2), for all a, without materialising [N, A, H].
 * Row n of base / P_all / Q is (env e, agent j) with n = e * n_agents + j.
 *
 * Selection of row n (T_out32 / T_out64 / P_out):
 *   greedy    the FIRST maximum of Q over the available actions (unavailable ones count as -inf; the lower index wins a
 *             tie).  A row with NO available action takes action 0.
 *   explore   unless greedy_only or epsilon <= 0: (v0, v1, ., .) = Philox4x32-10(counter words (n lo, n hi, c lo, c hi),
 *             key (seed lo, seed hi)) with c = counter + *counter_dev.  The row explores iff (v0 >> 8) 2^-24 < epsilon
 *             (compared in float32; the left side is exact).  Then pool = number of available actions, or A if none is
 *             available, k = (v1 * pool) >> 32, and the choice is the k-th available action in index order — with no
 *             available action the k-th of all A: uniform over all of them.
 *   P_out = P_all[n, chosen], bit for bit.
 * q_gather_out[n] is 0 for a gather_idx[n] outside [0, A).
 */
typedef struct macjd_qhead_io {
    int64_t n_rows;          /* N = E * n_agents */
    int32_t H, A, n_agents, greedy_only; /* greedy_only != 0: test_mode (argmax, no exploration) */
    const float* base;  int64_t base_ld;   /* [N,H] row stride in elements */
    const float* P_all; int64_t p_ld;      /* [N,A] actor output (networks.py:116-129) */
    const float* W1;    int64_t w1_ld;     /* fc2_q_head.0.weight [H, H+A+1], row stride */
    const float* w2;                       /* fc2_q_head.2.weight [H] */
    const float* b2;                       /* fc2_q_head.2.bias  [1] */
    float* Q;           int64_t q_ld;      /* optional out [N,A]: UNMASKED Q-values */
    /* ---- optional selection stage (T_out32 or T_out64 non-NULL) ---- */
    const void* avail;  int32_t avail_elem_size, reserved; /* optional mask, int32 (4) or int64 (8) elements */
    int64_t av_se, av_sj, av_sa;           /* avail element strides over (env, agent, action) */
    float epsilon;      float reserved2;   /* exploration probability (action_selectors.py:30-32) */
    uint64_t seed, counter;                /* Philox key / call counter for the exploration draws */
    /* optional device-side sources, for launches replayed from a captured HIP graph (kernel arguments
       are frozen at capture): *eps_dev replaces epsilon, *counter_dev is ADDED to counter */
    const float* eps_dev;
    const uint64_t* counter_dev;
    int32_t* T_out32;                      /* optional chosen action, int32 */
    int64_t* T_out64;                      /* optional chosen action, int64 */
    int64_t t32_se, t32_sj, t64_se, t64_sj;/* element strides over (env, agent) */
    float* P_out;       int64_t po_se, po_sj; /* optional chosen power = P_all[n, T] (mac.py:151-164) */
    /* ---- Double-DQN helpers of the learner (reference core/qmix.py:138-147), contiguous [N] ----
       argmax_out[n] = first arg-max of the UNMASKED Q-values (the reference applies no mask there);
       q_gather_out[n] = Q[n, gather_idx[n]] (the target network's value of the eval network's choice). */
    int64_t* argmax_out;
    const int64_t* gather_idx;
    float* q_gather_out;
} macjd_qhead_io;

int macjd_qhead_select(const macjd_qhead_io* io, void* hip_stream);

/*
 * All T steps of the GRU recurrence for B*J independent sequences, for up to two networks (eval and
 * target) in one launch.  Replaces the learner's `for t in range(max_seq_len): h = agent.forward(...)`
 * unroll (reference core/qmix.py:241-253 -> core/networks.py:88-114 -> torch.nn.GRUCell), inference
 * only (the reference never back-propagates through it, see SURVEY.md section 8a note 4).
 *
 * gi = W_ih x_t + b_ih is time-parallel and supplied by the caller for every step ([B,T,J,3H],
 * contiguous, gate order r,z,n); the kernel evaluates  gh = W_hh h + b_hh,  r = s(gi_r + gh_r),
 * z = s(gi_z + gh_z),  n = tanh(gi_n + r * gh_n),  h' = (h - n) z + n  and stores every h' ([B,T,J,H]).
 * H must be 64 or 128.
 */
typedef struct macjd_gru_io {
    int32_t n_nets, B, T, J, H, reserved;   /* n_nets = 1 or 2; reserved != 0 ("gi_static"): gi is [B,1,J,3H], the
                                               same input transform at every step (static observation) */
    const float* gi[2];    /* [B,T,J,3H] */
    const float* w_hh[2];  /* rnn.weight_hh [3H,H] row-major, 16-byte aligned (its rows are read as float4;
                              MACJD_EINVAL otherwise) */
    const float* b_hh[2];  /* rnn.bias_hh [3H] */
    const float* h0[2];    /* optional initial state [B,J,H]; NULL = zeros (mac.init_hidden) */
    float* h_out[2];       /* [B,T,J,H] */
    int64_t h0_sb[2];      /* element stride between batch entries of h0 (0 = J*H, contiguous): lets the caller pass
                              step 0 of a stored [B,T+1,J,H] hidden-state tensor without copying it.  0 never means
                              "one [J,H] block for every batch entry": such an h0 has to be materialised as [B,J,H] */
    /* Static observation, input transform computed IN the kernel (gi[] may then be NULL): sequence (b, j) reads its
       observation row obs + row(b) * obs_sb + j * obs_sj (row(b) = obs_index[b] if obs_index else b — e.g. the sampled
       episodes' step-0 rows straight out of the replay ring, no gather in front of the scan) and evaluates
       gi = W_ih ReLU(fc1 obs + b_fc1) + b_ih once (reference core/networks.py:96-100), used at every step. */
    const float* obs;      int64_t obs_sb, obs_sj;   int32_t S, reserved2;
    const int64_t* obs_index;                        /* optional [B] */
    const float* fc1_w[2]; const float* fc1_b[2];    /* fc1.weight [H,S], fc1.bias [H] */
    const float* w_ih[2];  const float* b_ih[2];     /* rnn.weight_ih [3H,H], rnn.bias_ih [3H] */
    /* optional, with obs: the frozen actor chain of the same observation row (core/networks.py:116-129),
       p_out[net][(b * J + j) * A + a] = sigmoid(L3 ReLU(L2 ReLU(L1 x))) — the continuous parameter of every action,
       one row per SEQUENCE (it is the same at every step).  Ah <= 256, A <= 64. */
    float* p_out[2];
    const float* act_w[2][3]; const float* act_b[2][3];   /* actor.{0,2,4}.{weight,bias}: [Ah,S], [Ah,Ah], [A,Ah] */
    int32_t Ah, A;
} macjd_gru_io;

int macjd_gru_sequence(const macjd_gru_io* io, void* hip_stream);

/*
 * QMixer.forward after the hyper-network GEMMs (reference core/networks.py:283-315), per row m:
 *   w1 = clamp(w1_raw, 0, 5) [J,Em]   b1 = clamp(b1_raw, -5, 5) [Em]   wf = clamp(wf_raw, 0, 5) [Em]
 *   v = clamp(v_raw, -5, 5)           hid = q . w1 + b1                y = ELU(hid) . wf + v
 * (torch.bmm([M,1,J],[M,J,Em]) / F.elu / torch.bmm([M,1,Em],[M,Em,1]) in the reference) and its backward
 * (clamp passes the gradient where min <= x <= max, like torch.clamp).  All tensors contiguous float32 (b1_raw may
 * have a row stride).
 * Forward needs q, w1_raw, b1_raw, wf_raw, v_raw, y.  Backward additionally gy and the five gradient outputs.
 */
typedef struct macjd_mixer_io {
    int64_t M;              /* rows = B * (T-1) */
    int32_t J, Em;          /* agents, mixing_embed_dim */
    const float* q;         /* [M,J]    */
    const float* w1_raw;    /* [M,J*Em] hyper_w_1 output   */
    const float* b1_raw;    /* [M,Em]   hyper_b_1 output   */
    const float* wf_raw;    /* [M,Em]   hyper_w_final output */
    const float* v_raw;     /* [M]      V output           */
    float* y;               /* [M]      Q_tot (forward out) */
    const float* gy;        /* [M]      dL/dy (backward in) */
    float* gq;              /* [M,J]    (backward outs)    */
    float* gw1_raw;         /* [M,J*Em] */
    float* gb1_raw;         /* [M,Em]   */
    float* gwf_raw;         /* [M,Em]   */
    float* gv_raw;          /* [M]      */
    int64_t b1_ld;          /* row stride of b1_raw in elements (0 = Em): b1_raw may be a column block of the merged
                               first-layer output */
} macjd_mixer_io;

int macjd_mixer_tail_forward(const macjd_mixer_io* io, void* hip_stream);
int macjd_mixer_tail_backward(const macjd_mixer_io* io, void* hip_stream);

/*
 * TD target + masked mean-squared TD error of QMixLearner.train (reference core/qmix.py:155,190-194):
 *   target = r + gamma (1 - terminated) tq ;  loss = sum((filled (y - target))^2) / sum(filled)
 * over M = B * Tm1 (batch, step) pairs, plus dL/dy = 2 filled (y - target) / sum(filled) and the two logged means
 * (eval_qtot_avg = mean(y), target_qtot_avg = mean(target), qmix.py:212-213).  One single-workgroup launch.
 * y / tq / reward / terminated / filled are addressed with batch (and step) element strides so that slices of
 * longer [B,T(+1),1] tensors need no copy; gy may be a full-length row with the unused tail zeroed.  terminated / filled are 1-byte bools.
 */
typedef struct macjd_tdloss_io {
    int32_t B, Tm1;
    float gamma, reserved;
    const float* y;            /* eval Q_tot:   element (b, t) at y[b * y_sb + t],  t < Tm1 */
    const float* tq;           /* target Q_tot: element (b, t) at tq[b * tq_sb + t]         */
    int64_t y_sb, tq_sb;       /* batch strides (Tm1 for contiguous [B*Tm1] tensors)        */
    int64_t gy_sb, gy_cols;    /* gy row pitch and row length: columns Tm1..gy_cols-1 are written as zeros */
    const float* reward;       int64_t r_sb, r_st;
    const uint8_t* terminated; int64_t t_sb, t_st;
    const uint8_t* filled;     int64_t f_sb, f_st;
    float* stats;              /* [4] out: loss, mean(y), mean(target), sum(filled) */
    float* gy;                 /* out: dL/dy, element (b, t) at gy[b * gy_sb + t]; NULL: the logged sums only — stats[0..2]
                                  are written, stats[3] is left alone, no gradient (macjd_mixer_fused_backward_td forms it) */
} macjd_tdloss_io;

int macjd_td_loss(const macjd_tdloss_io* io, void* hip_stream);
/* out[0] = sum of the loss mask (io->filled over B x Tm1; the other fields are not read): the only global quantity the
   gradient of the loss needs — see macjd_mixer_fused_backward_td. */
int macjd_td_mask_sum(const macjd_tdloss_io* io, float* out, void* hip_stream);

/*
 * TD(lambda) targets: the loss of macjd_td_loss against lambda-returns instead of the one-step target.  For a batch of B
 * episodes and Tm1 loss-carrying steps, with the inputs of macjd_td_loss (tq[b, t] = the target network's Q_tot of step
 * t + 1), per episode:
 *   boot[t] = gamma * (1 - terminated[t])
 *   cont[t] = (t + 1 < Tm1) and filled[t + 1] and not terminated[t]          -- a select, never a multiply
 *   lam[t]  = lambda if cont[t] else 0
 *   G[t]    = reward[t] + boot[t] * ((1 - lam[t]) * tq[t] + lam[t] * G[t + 1])          -- G[Tm1] is never read
 *   loss    = sum((filled (y - G))^2) / sum(filled)
 *   gy      = 2 filled (y - G) / sum(filled)
 *   stats   = loss, mean(y), mean(G) over all B * Tm1, sum(filled)
 * The chain stops on termination, at the last step and in front of an unfilled step; what sits behind a stop never
 * reaches a G in front of it (the select: not even as 0 * inf).  lambda = 0 is macjd_td_loss's target term for term;
 * lambda = 1 is the discounted reward-to-go with one bootstrap where the chain stops.  G[t] is defined at unfilled t by
 * the same recursion, so mean(G) keeps the meaning mean(target) has in macjd_td_loss.
 * One single-workgroup launch.  td: every field as in macjd_td_loss (strides, gy_cols, gy == NULL = the sums only:
 * stats[0..2] written, stats[3] left alone; ret is written either way).
 */
typedef struct macjd_tdlambda_io {
    macjd_tdloss_io td;
    float lambda;              /* 0 <= lambda <= 1 */
    float reserved;            /* the padding in front of ret made explicit (as in macjd_tdloss_io): not read, set 0 */
    float* ret;                /* out, required: G, element (b, t) at ret[b * ret_sb + t], t < Tm1 */
    int64_t ret_sb;            /* >= Tm1 */
} macjd_tdlambda_io;

int macjd_td_lambda_loss(const macjd_tdlambda_io* io, void* hip_stream);

/*
 * Gradient clipping + Adam over ONE flat parameter vector (reference core/qmix.py:199-200:
 * torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step()):
 *   total_norm = ||grad||_2 ; coef = min(1, max_norm / (total_norm + 1e-6)) ; g = coef * grad
 *   step += 1 ; m = m + (1 - b1)(g - m) ; v = b2 v + (1 - b2) g g
 *   param -= (lr / (1 - b1^step)) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 * param / grad / exp_avg / exp_avg_sq are contiguous float32 [n]; step is a float32 device scalar (torch's
 * capturable Adam keeps it on the device), read-modify-written by the kernel; grad_norm (out) = total_norm.
 * `partials` is caller-provided scratch of >= 256 floats.  Two launches.
 */
typedef struct macjd_adam_io {
    int64_t n;
    float lr, beta1, beta2, eps, max_norm, reserved;
    float* param; float* grad /* scaled in place by coef, like clip_grad_norm_ */; float* exp_avg; float* exp_avg_sq;
    float* step; float* grad_norm; float* partials;
} macjd_adam_io;

int macjd_clip_adam_step(const macjd_adam_io* io, void* hip_stream);

/*
 * Draw of the NEXT update's episodes on the device: idx_out[0..n) = n distinct indices, uniform over [0, *n_stored) —
 * what the reference's buffer does on the host with np.random.choice(current_size, batch, replace=False)
 * (utils/replay_buffer.py:89) — as the first n images of a keyed pseudo-random permutation of [0, *n_stored):
 * an 8-round Feistel network on the ceil(log2 N) bits of an index, cycle-walked back into [0, N), round keys =
 * Philox4x32-10(counter = *counter, key = seed).  *counter advances by one per draw, so a sequence of draws is a
 * function of (seed, first counter value) only.  A host-drawn batch needs an index upload between two updates, which
 * sits on the serial chain of the replayed graphs (~10 us of a ~190 us step); this draw rides at the end of the previous
 * update's last launch (macjd_clip_adam_step_sample), or stands alone (macjd_sample_episodes: first draw, redraw after
 * the population changed).  *n_stored < n: idx_out[i] = i mod *n_stored (callers fall back to the host path before).
 */
typedef struct macjd_sampler_io {
    int64_t* idx_out;          /* [n] */
    int32_t n, reserved;       /* reserved >= 0: counter offset — the draw of counter value *counter + reserved, which
                                  leaves *counter = that value + 1 (0: the plain draw; see macjd_prefetch_batch) */
    const int32_t* n_stored;   /* device scalar: stored episodes (the population) */
    int64_t* counter;          /* device scalar: draws made so far */
    uint64_t seed;
} macjd_sampler_io;

int macjd_sample_episodes(const macjd_sampler_io* io, void* hip_stream);
/* macjd_clip_adam_step followed, inside its last launch, by the draw of the next update's episodes (next may be NULL) */
int macjd_clip_adam_step_sample(const macjd_adam_io* io, const macjd_sampler_io* next, void* hip_stream);

/*
 * Weight and bias gradient of y = x W^T + b over K rows:  dW[M,N] = gout[K,M]^T x inp[K,N],  db[M] = sum_k gout[k,:]
 * (the backward of torch.nn.Linear for its parameters, core/qmix.py:198 loss.backward()).  On this path the outputs
 * are tiny (e.g. [192,128]) and K is 3e3..1e4 rows, so the reduction is split over K: every workgroup computes one
 * 64x64 output tile for one 64-row K-chunk on exact-f32 MFMA into `workspace`, a second launch sums the chunks in
 * fixed order (deterministic).  workspace >= macjd_linear_wgrad_workspace_floats(K, M, N) floats; the number of chunks is
 * what that size implies: chunks (Mp Np + Mp) floats with Mp / Np = M / N padded to 64.
 */
typedef struct macjd_wgrad_io {
    int64_t K;
    int32_t M, N;
    const float* gout; int64_t gout_ld;   /* [K,M] row stride (elements) */
    const float* inp;  int64_t inp_ld;    /* [K,N] */
    float* dW;         int64_t dw_ld;     /* [M,N] out */
    float* db;                            /* [M] out, optional */
    float* workspace;
    /* optional (both or neither): the [K,M] operand is not `gout` itself but formed while it is staged,
       element (k, m) = (gout[k, m] > 0) ? outer_vec[k] * outer_w[m] : 0 — the gradient behind ReLU -> one-output Linear
       (the MP-DQN Q-head, core/networks.py:75-79): `gout` then holds the ReLU's OUTPUT, outer_vec the gradient of the
       one output per row, outer_w that layer's weight row.  Saves the launch that would materialise the product. */
    const float* outer_vec;               /* [K] */
    const float* outer_w;                 /* [M] */
    /* optional, macjd_linear_wgrad_many_norm only (every other entry point returns MACJD_EUNSUPPORTED for kind != 0):
       where the REDUCE launch takes the problem's terms from.  A problem of kind != 0 has no work item in the
       partial-products launch; when no problem of a call has one, that launch is not issued.
         MACJD_WGRAD_EXT_SLOTS     `workspace` already holds `ext_chunks` slots in the partial launch's layout — slot c at
                                   workspace + c Mp Np (Mp / Np = M / N padded to 64, row stride Np), the bias rows behind
                                   them at workspace + ext_chunks Mp Np + c Mp — written by an earlier launch
                                   (macjd_mixer_wgrad_block).  gout / inp / K / outer_* are not read.  The contracted
                                   problem: `ext_chunks` slots of [2][N] floats.
         MACJD_WGRAD_ROW_PRODUCTS  no slots at all: output (m, n) = sum_k gout[k, m] * inp[k, n] and db[m] = sum_k gout[k, m]
                                   straight from the operands (fmaf per term, the rounds / waves / tree of the slot sums
                                   with term k in the place of slot k).  For short reductions (K of a few hundred rows).
                                   `workspace` is not read; no outer_vec; not the contracted problem. */
    int32_t kind, ext_chunks;
} macjd_wgrad_io;
#define MACJD_WGRAD_ORDINARY 0
#define MACJD_WGRAD_EXT_SLOTS 1
#define MACJD_WGRAD_ROW_PRODUCTS 2

int64_t macjd_linear_wgrad_workspace_floats(int64_t K, int32_t M, int32_t N);
int macjd_linear_wgrad(const macjd_wgrad_io* io, void* hip_stream);
/* Up to MACJD_WGRAD_MAX_BATCH independent problems in ONE launch pair (all their (tile, chunk) partial products,
   then all their chunk sums): same arithmetic and summation order as macjd_linear_wgrad per problem.  The learner's
   backward pass defers its six weight gradients to one such call (they only feed .grad; nothing downstream waits). */
#define MACJD_WGRAD_MAX_BATCH 8
int macjd_linear_wgrad_many(const macjd_wgrad_io* ios, int32_t n, void* hip_stream);

/*
 * macjd_linear_wgrad_many whose launch pair also leaves what the optimiser step needs of the gradients it writes, so
 * that macjd_clip_adam_step_reduced can follow as ONE launch (no squared-norm / LayerNorm launch in between):
 *   * problem `ln_problem` (-1: none) is LayerNorm-CONTRACTED: G = gout^T inp [M, N <= 64] is never written.  Its work
 *     item (row tile, chunk) multiplies its 64 x N accumulators by W[m, n] (rows past M count zero), sums over its rows
 *     in a fixed order (registers, across lanes, across the waves through LDS; no atomics) and stores two rows of N
 *     floats into slot [tile * n_chunks + chunk][2][N] of the problem's workspace:
 *         dgamma_part[n] = sum_m W[m, n] G_part[m, n]      dbeta_part[n] = sum_m W[m, n] gb_part[m]
 *     (gb_part = the chunk's column sums of gout).  The reduce launch sums the slots into dgamma[n] / dbeta[n]:
 *     macjd_lnparam_io's outputs with gb = the column sums of this problem's gout.  Its dW / db are ignored (db must be
 *     NULL); the workspace size is that of the ordinary problem.
 *   * every reduce workgroup w writes partials[w] = sum of the squares of the values it STORED (dW, db, dgamma, dbeta),
 *     w < macjd_linear_wgrad_many_norm_partials(...) <= 8192 <= partials_cap;
 *   * the reduce launch advances the optimiser's step counter (*step += 1), as the squared-norm launch of
 *     macjd_clip_adam_step does.
 * The ordinary problems' dW / db are bit-identical to macjd_linear_wgrad_many's.
 */
typedef struct macjd_wgrad_norm_io {
    int32_t ln_problem, partials_cap;
    const float* W; int64_t w_ld;          /* [M, N] of problem ln_problem: the Linear layer behind the LayerNorm */
    float* dgamma; float* dbeta;           /* [N] out */
    float* partials;                       /* [partials_cap] out */
    float* step;                           /* device scalar, read-modify-written */
} macjd_wgrad_norm_io;

int32_t macjd_linear_wgrad_many_norm_partials(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem);   /* < 0: bad argument */
int macjd_linear_wgrad_many_norm(const macjd_wgrad_io* ios, int32_t n, const macjd_wgrad_norm_io* norm, void* hip_stream);
/* The same call with flags.  ROW PRODUCTS problems: by default the reduce launch is the STAGED form — blocks of 256
   consecutive weight items (four 64-item groups, one thread per output) of one such problem with 37 <= N <= 128 form their
   sums from operand rows staged once per block into LDS; every other 64-item group (bias items, other kinds, heads and
   tails of a range, other N) is a block of the plain rows kernel's code.  Every output, partials[w] (still the squares of
   items [64 w, 64 w + 64)) and the step counter are bit-identical to the plain rows kernel for finite operands.
   MACJD_WGRAD_PLAIN_ROWS selects the plain rows kernel.  macjd_linear_wgrad_many_norm = flags 0. */
#define MACJD_WGRAD_PLAIN_ROWS 1u
int macjd_linear_wgrad_many_norm_ex(const macjd_wgrad_io* ios, int32_t n, const macjd_wgrad_norm_io* norm, uint32_t flags,
                                    void* hip_stream);
/* workgroups of that call's reduce launch (<= macjd_linear_wgrad_many_norm_partials: a staged block stands for four
   groups); < 0: bad argument */
int32_t macjd_linear_wgrad_many_norm_blocks(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem, uint32_t flags);
/* work items of that call's partial-products launch (0: the launch is not issued); < 0: bad argument */
int64_t macjd_linear_wgrad_many_norm_work_items(const macjd_wgrad_io* ios, int32_t n, int32_t ln_problem);
/* floats of `slots` external slots of an [M, N] problem with their bias rows (MACJD_WGRAD_EXT_SLOTS); < 0: bad argument */
int64_t macjd_wgrad_slot_floats(int32_t M, int32_t N, int64_t slots);

/* The optimiser step of macjd_clip_adam_step_sample as ONE launch behind macjd_linear_wgrad_many_norm: every workgroup sums
   io->partials[0 .. n_partials) itself (all 256 threads: loads first, then per thread in index order, across the wave,
   four waves as (p0 + p1) + (p2 + p3)), clips, applies Adam with the ALREADY advanced step counter, writes grad_norm and
   draws the next batch (next may be NULL).  Every element of io->grad that is not zero must be counted in the partials. */
int macjd_clip_adam_step_reduced(const macjd_adam_io* io, int32_t n_partials, const macjd_sampler_io* next, void* hip_stream);

/*
 * Gather `n_rows` whole rows (episodes) of up to 8 tensors in ONE launch: dst_k[i, :] = src_k[idx[i], :] as raw
 * bytes (row_bytes[k] each, multiples of 4).  Replaces the per-key index_select of
 * EpisodeReplayBuffer.sample (reference utils/replay_buffer.py:181-183).
 */
typedef struct macjd_gather_io {
    int32_t n_tensors, n_rows;
    const int64_t* idx;            /* [n_rows] device */
    const void* src[8]; void* dst[8]; int64_t row_bytes[8];
    int64_t dst_row_bytes[8];      /* destination row pitch (>= row_bytes, multiple of 4); 0 = row_bytes */
} macjd_gather_io;

int macjd_gather_rows(const macjd_gather_io* io, void* hip_stream);

/*
 * The whole prefetch of a LATER update's batch inside a captured group of updates as ONE launch: what
 * macjd_sample_episodes -> macjd_gather_rows -> macjd_td_mask_sum -> macjd_gru_sequence (static observation read from the
 * replay ring, in-kernel input transform, actor rows) do one behind the other, with the same device code on the same data
 * (bit-identical results).  The three short launches no longer stand in front of the latency-bound scan.
 *   gru      the scan's arguments: n_nets = 1, H = 64, obs = the ring's observation tensor, p_out[0] set.  obs_index is
 *            NOT read: sequence (b, j) reads ring row index(b).
 *   gather   the gather's arguments: n_rows = B; idx is NOT read, dst_k[b, :] = src_k[index(b), :].
 *   sampler  index(t) = element t of the draw of counter value *counter + reserved (reserved >= 0: the counter offset),
 *            evaluated by every workgroup for the indices it needs.  The launch only READS the counter; one workgroup
 *            stores idx_out[0..n) for later readers.  With *n_stored < 1 or no_draw != 0: index(t) = idx_out[t] as found.
 *   mask     B, Tm1, filled / f_sb / f_st of the RING's `filled` tensor (rows index(b)); tot_m[0] = sum over B x Tm1.
 * A group of K updates bakes offsets 0 .. K-2 into the prefetches of its updates 1 .. K-1 and closes with a draw of
 * offset K-1 (macjd_sampler_io.reserved of macjd_clip_adam_step_sample's `next`), which leaves the counter K further:
 * the counter values and the final counter of K sequential draws.
 * gather_blocks: workgroups that share the copy (0 = default).
 */
typedef struct macjd_prefetch_io {
    macjd_gru_io gru;
    macjd_gather_io gather;
    macjd_sampler_io sampler;
    macjd_tdloss_io mask;
    float* tot_m;
    int32_t no_draw, gather_blocks;
} macjd_prefetch_io;

int macjd_prefetch_batch_supported(int32_t n_nets, int32_t H, int32_t B);   /* 1 / 0 */
int macjd_prefetch_batch(const macjd_prefetch_io* io, void* hip_stream);

/*
 * The prefetches of n consecutive later updates (1 <= n <= MACJD_PREFETCH_MAX_BATCHES) as ONE launch: for every batch i
 * what macjd_prefetch_batch(&ios[i]) does, bit for bit, in one grid — the scan workgroups of every batch first, then the
 * actor rows, the gather workgroups (gather_blocks PER batch) and one mask-sum workgroup per batch.  A second batch is
 * another B * J sequences on compute units that the latency-bound scan of the first leaves idle, so the launch takes
 * little longer than a one-batch launch (inside the learner's update 71 us for two batches against 60 us for one), and
 * a group of updates that issues it two updates ahead takes the prefetch off its critical cycle.  macjd_prefetch_batch
 * is the case n = 1.
 * All batches share the ring tensors and the weights, B / J / T and the gather sources, the sampler's counter, n_stored
 * and seed, the mask geometry and gather_blocks: ios[i] must equal ios[0] in everything but
 *     sampler.reserved (the counter offset), no_draw, sampler.idx_out,
 *     gather.dst[] / gather.dst_row_bytes[], gru.h_out[0], gru.p_out[0], tot_m,
 * and no two batches may share one of these outputs (MACJD_EINVAL otherwise): the byte ranges that two batches write —
 * h_out [B,T,J,H], p_out [B,J,A], tot_m, idx_out [B] unless no_draw, dst[k] (B - 1 row pitches + one row) — must not
 * overlap, whichever outputs they belong to; an idx_out that is only read (no_draw) may be shared between such batches
 * but not overlap anything another batch writes.  The launch only reads the counter.
 */
#define MACJD_PREFETCH_MAX_BATCHES 4
int macjd_prefetch_batches_supported(int32_t n_nets, int32_t H, int32_t B, int32_t n);   /* 1 / 0 */
int macjd_prefetch_batches(const macjd_prefetch_io* ios, int32_t n, void* hip_stream);

/*
 * Input rows of the Q-head for the TAKEN action, out[n, :] = [h[n, 0..H-1], onehot_A(idx[n]), P[n]]  — the
 * F.one_hot / torch.cat sequence of RNNAgent.get_q_value_for_action (reference core/networks.py:160-174)
 * as one launch.  idx outside [0, A) gives an all-zero one-hot block (the caller validates indices when asked to).
 */
typedef struct macjd_qinput_io {
    int64_t n_rows;
    int32_t H, A;
    const float* h;   int64_t h_ld;      /* [n_rows, H] */
    const void* idx;  int32_t idx_elem_size, reserved;   /* [n_rows] int32 (4) or int64 (8), contiguous */
    const float* P;                      /* [n_rows] contiguous */
    float* out;       int64_t out_ld;    /* [n_rows, H + A + 1] */
} macjd_qinput_io;

int macjd_qhead_input(const macjd_qinput_io* io, void* hip_stream);

/*
 * Q-value of the TAKEN action for n rows — RNNAgent.get_q_value_for_action (reference core/networks.py:131-180: one_hot,
 * cat, Linear, ReLU, Linear), the only differentiable path of the learner's loss into the agent (core/qmix.py:161-184) —
 * as ONE launch instead of macjd_qhead_input + a library GEMM with bias / ReLU epilogue + macjd_rowdot:
 *   x[n, :]   = [h[n, 0..H-1], onehot_A(idx[n]), P[n]]                   (written: the backward's weight-gradient operand)
 *   act[n, u] = ReLU(sum_k W1[u, k] h[n, k] + b1[u] + W1[u, H + idx[n]] + W1[u, H + A] P[n])   (written: saved for backward)
 *   q[n]      = sum_u w2[u] act[n, u] + b2
 * The H x H product runs on exact-f32 MFMA (32 rows per workgroup, wave w owns hidden units [16w, 16w+16), W1's h-columns
 * as register fragments); the one-hot / power columns of W1 are a gather from LDS.  H = 64 (= rows of W1), A <= 64,
 * h rows 16-byte aligned.  idx outside [0, A): empty one-hot block.  Differs from the three-launch form by the summation
 * order of the first layer (~1e-7 relative).
 */
typedef struct macjd_qtaken_io {
    int64_t n_rows;
    int32_t H, A;
    const float* h;   int64_t h_ld;                       /* [n_rows, H] */
    const void* idx;  int32_t idx_elem_size, reserved;    /* [n_rows] int32 (4) or int64 (8), contiguous */
    const float* P;                                       /* [n_rows] contiguous */
    const float* W1;  int64_t w1_ld;                      /* fc2_q_head.0.weight [H, H + A + 1] */
    const float* b1;  const float* w2;  const float* b2;  /* [H], fc2_q_head.2.weight [H], .bias [1] or NULL */
    float* x;         int64_t x_ld;                       /* [n_rows, H + A + 1] out (may be NULL) */
    float* act;       int64_t act_ld;                     /* [n_rows, H] out */
    float* q;                                             /* [n_rows] out */
} macjd_qtaken_io;

int macjd_qhead_taken_supported(int32_t H, int32_t A);   /* 1 / 0 */
int macjd_qhead_taken(const macjd_qtaken_io* io, void* hip_stream);

/*
 * LayerNorm forward over the last dimension (QMixer.state_norm, reference core/networks.py:215,270):
 *   mean = sum(x)/S, var = sum((x-mean)^2)/S (biased, two-pass), rstd = rsqrt(var + eps), y = (x-mean) rstd gamma + beta.
 * mean / rstd [M] are saved for torch's native_layer_norm_backward.  S <= 1024.
 */
typedef struct macjd_layernorm_io {
    int64_t M;
    int32_t S, reserved;
    float eps, reserved2;
    const float* x;  int64_t x_ld;
    const float* gamma;   /* [S] or NULL (= 1) */
    const float* beta;    /* [S] or NULL (= 0) */
    float* y;        int64_t y_ld;
    float* mean;          /* [M], optional */
    float* rstd;          /* [M], optional */
    float* xhat;     int64_t xhat_ld;   /* optional [M, S]: the normalised input (x - mean) rstd, before gamma / beta */
} macjd_layernorm_io;

int macjd_layernorm_forward(const macjd_layernorm_io* io, void* hip_stream);

/*
 * Gradients of a LayerNorm's gamma / beta when the normalised tensor feeds ONE Linear layer y = s W^T + b,
 * s = xhat gamma + beta (QMixer.state_norm -> the merged first hyper-network layer), from quantities the weight-
 * gradient pass already has:  dbeta[k] = sum_c gb[c] W[c,k],  dgamma[k] = sum_c W[c,k] G[c,k]  with gb = column sums
 * of the layer's output gradient and G = gout^T xhat ([C, K], one more split-K problem).  Replaces the [M, K]
 * input-gradient GEMM + the two reduction launches of native_layer_norm_backward.
 */
typedef struct macjd_lnparam_io {
    int32_t C, K;                          /* Linear: C outputs, K inputs (= LayerNorm width) */
    const float* W;   int64_t w_ld;        /* [C, K] */
    const float* G;   int64_t g_ld;        /* [C, K] = gout^T xhat */
    const float* gb;                       /* [C] */
    float* dgamma;                         /* [K] */
    float* dbeta;                          /* [K] */
} macjd_lnparam_io;

int macjd_layernorm_param_grad(const macjd_lnparam_io* io, void* hip_stream);
/* macjd_clip_adam_step_sample whose FIRST launch also evaluates the LayerNorm parameter gradients (this struct) — they are
   part of the clipped vector, at elements gamma_off / beta_off of io->grad (ln->dgamma / ln->dbeta must point there), so
   the squared-norm launch computes them in K extra workgroups and counts their squares itself; the other workgroups skip
   those two ranges.  One launch less behind the weight-gradient reduce.  io->partials: >= 256 + ln->K floats.
   The two ranges [gamma_off, gamma_off + K) and [beta_off, beta_off + K) lie inside [0, io->n) and must not overlap
   (|gamma_off - beta_off| >= K; adjacent ranges are fine): MACJD_EINVAL before any launch otherwise.  ln->K <= 1024. */
int macjd_clip_adam_step_ln(const macjd_adam_io* io, const macjd_sampler_io* next, const macjd_lnparam_io* ln,
                            int64_t gamma_off, int64_t beta_off, void* hip_stream);

/*
 * Fused chain of up to three dense layers, y = act_n(W_n ... act_1(W_1 x + b_1) ... + b_n), float32 with
 * exact-f32 MFMA (v_mfma_f32_16x16x4_f32).  Replaces the separate Linear / activation launches of
 *   RNNAgent.actor            Linear-ReLU-Linear-ReLU-Linear-Sigmoid   (reference core/networks.py:54-61,127)
 *   fc1 + GRU input transform Linear-ReLU-Linear (W_ih x + b_ih)       (core/networks.py:100, GRUCell)
 * in the rollout (core/mac.py:168-187) and in the learner's time-parallel unroll (core/qmix.py:241-253).
 * W_l is torch.nn.Linear's [out, in] row-major weight.  Limits: dims[0] <= 256, hidden widths <= 128, last
 * width <= 384, ceil(width / 16) in {1,2,3,4,8,12,24}, one layer's LDS weight image (rows padded to a pitch of
 * 32 m + 2 floats) + the activation strips <= 160 KB of LDS; MACJD_EUNSUPPORTED otherwise.
 */
#define MACJD_ACT_NONE 0
#define MACJD_ACT_RELU 1
#define MACJD_ACT_SIGMOID 2
typedef struct macjd_mlp_io {
    int64_t n_rows;
    int32_t n_layers;        /* 1..3 */
    int32_t dims[4];         /* dims[0] = input width, dims[l+1] = output width of layer l */
    int32_t act[3];          /* MACJD_ACT_* per layer */
    const float* W[3];       /* [dims[l+1], dims[l]] contiguous */
    const float* b[3];       /* [dims[l+1]] */
    const float* x;  int64_t x_ld;   /* [n_rows, dims[0]], row stride in elements (0 = one row broadcast to all) */
    float* y;        int64_t y_ld;   /* [n_rows, dims[n_layers]] */
} macjd_mlp_io;

/* One launch, no workspace: the weights are read in torch's own [out, in] layout (LDS-DMA into padded LDS rows). */
int macjd_mlp_forward(const macjd_mlp_io* io, void* hip_stream);
/* Two independent chains in ONE launch (workgroups are split between them): the actor chain and the fc1 -> W_ih chain
   of the rollout step over the same observation rows, or the eval and target actors of the learner. */
int macjd_mlp_forward_pair(const macjd_mlp_io* io0, const macjd_mlp_io* io1, void* hip_stream);

/*
 * Backward of "ReLU on the first Cr columns of a [M, Cr + Cp] matrix, pass the last Cp columns through, hand the
 * result out as column blocks" (the merged first layer of the mixer's hyper-networks, reference
 * core/networks.py:283-299): gout[m, c] = g_k[m, c - start_k] * (act[m, c] > 0) for the ReLU blocks and
 * g_pass[m, c - Cr] for the pass-through block, written in ONE launch (autograd would run cat + threshold_backward
 * + cat).  Up to 4 ReLU blocks; a NULL block gradient counts as zero.
 */
typedef struct macjd_splitrelu_bwd_io {
    int64_t M;
    int32_t n_blocks, Cp;             /* ReLU blocks (1..4); pass-through width (may be 0) */
    int32_t width[4];                 /* widths of the ReLU blocks, sum = Cr */
    const float* g[4];  int64_t g_ld[4];     /* block gradients [M, width[k]] */
    const float* g_pass; int64_t gp_ld;      /* [M, Cp] */
    const float* act;   int64_t act_ld;      /* [M, Cr] ReLU output saved by the forward */
    float* gout;        int64_t gout_ld;     /* [M, Cr + Cp] */
    const float* outer_w[4];                 /* NULL, or [width[k]]: block k's gradient is g[k][m] * outer_w[k][c] */
} macjd_splitrelu_bwd_io;

int macjd_splitrelu_backward(const macjd_splitrelu_bwd_io* io, void* hip_stream);

/*
 * y[n] = x[n, :] . w + b for a Linear layer with ONE output feature (the Q-head's second layer and the mixer's V
 * head, reference core/networks.py:78,247): one launch instead of a bias-broadcast copy + a 16 x 256-tile GEMM.
 * K <= 1024, K % 4 == 0.
 */
typedef struct macjd_rowdot_io {
    int64_t n_rows;
    int32_t K, reserved;
    const float* x;  int64_t x_ld;   /* [n_rows, K] row stride in elements */
    const float* w;                  /* [K] */
    const float* b;                  /* [1] or NULL */
    float* y;                        /* [n_rows] contiguous */
} macjd_rowdot_io;

int macjd_rowdot(const macjd_rowdot_io* io, void* hip_stream);

/*
 * Gate arithmetic of one GRU cell step for N rows (torch.nn.GRUCell after its two GEMMs, reference
 * core/networks.py:100-113): given gi = W_ih x + b_ih and gh = W_hh h + b_hh ([N,3H], gate order r, z, n),
 *   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (h - n) z + n,
 * written to h_out and, optionally, to a second destination (the batched runner's staging row) in the same launch
 * (replaces the fused-cell launch + the copy).  H must be a multiple of 4; h_out may alias h.  gi_ld = 0 broadcasts
 * ONE gi row to all N rows (the observation of every env / agent is the same static vector, so its input transform
 * is computed once per episode batch).
 */
typedef struct macjd_grugates_io {
    int64_t n_rows;
    int32_t H, reserved;
    const float* gi;  int64_t gi_ld;
    const float* gh;  int64_t gh_ld;
    const float* h;   int64_t h_ld;
    float* h_out;     int64_t ho_ld;
    float* h_out2;    int64_t ho2_ld;   /* optional */
} macjd_grugates_io;

int macjd_gru_gates(const macjd_grugates_io* io, void* hip_stream);

/*
 * The whole QMix mixer as ONE launch each way (reference core/networks.py:250-315, QMixer.forward):
 *   s~ = LayerNorm(s)                                                                     networks.py:283
 *   [h_w1 | h_wf | h_V | b1_raw] = s~ W_first^T + b_first, ReLU on the first 2 Hh + Em columns   (first layers of
 *                                   hyper_w_1, hyper_w_final, V and the one-layer hyper_b_1, merged: 2 Hh + 2 Em rows)
 *   w1_raw = h_w1 W2^T + b2 [J Em]    wf_raw = h_wf Wf2^T + bf2 [Em]    v_raw = h_V . wV2 + bV2
 *   y = ELU(q . clamp(w1_raw,0,5) + clamp(b1_raw,-5,5)) . clamp(wf_raw,0,5) + clamp(v_raw,-5,5)
 * on the matrix cores in exact float32 (v_mfma_f32_16x16x4_f32).  A workgroup owns 16 rows; its four waves split the
 * OUTPUT columns of every layer (M = batch x steps is only a few thousand rows: 16-row workgroups fill the chip, and a
 * row's whole chain stays inside one workgroup).  Weights are read as MFMA operand fragments straight from L2 — every
 * fragment of the launch is requested before the first arithmetic instruction, so the chain pays one memory latency —
 * activations pass between the layers through LDS, and the hyper-network outputs w1_raw / wf_raw are consumed from the
 * accumulators: they are never written to memory (the unfused form materialises w1_raw [M, J Em] in HBM and
 * contracts it in a second kernel).  Replaces 7 launches of the mixer forward (LayerNorm, 3 library GEMMs, ReLU,
 * row-dot, tail) by one, for the eval and the target mixer alike.
 *
 * Training (save != 0): the forward also stores what the weight-gradient products need — s~, xhat = (s - mean) rstd
 * and the first-layer output `act` [M, 2 Hh + 2 Em] (post-ReLU blocks, then b1_raw).
 * Backward (macjd_mixer_fused_backward): re-derives w1_raw / wf_raw / v_raw from `act` (same instruction sequence,
 * bit-identical), then writes dL/dq [M,J], the output gradients of the second layers (g_w1raw [M,J Em], g_wfraw [M,Em],
 * g_v [M]) and — through the transposed second-layer weights and the ReLU masks — the output gradient of the merged
 * first layer `gout1` [M, 2 Hh + 2 Em].  No gradient flows to the state.  The weight / bias / LayerNorm-parameter
 * gradients are split-K products of these matrices (macjd_linear_wgrad_many, macjd_layernorm_param_grad).
 *
 * Operand type (operand_dtype; the five entry points below dispatch on it, the two mixers of a pair / training call must
 * agree, any other value returns MACJD_EINVAL).  0: the exact-f32 products above.  1: bf16 operands, i.e. round to
 * nearest even at exactly these points, every accumulation in f32 (v_mfma_f32_16x16x32_bf16):
 *   forward   LayerNorm f32; first layer bf16(s~) . bf16(W_first)^T, then + b_first in f32, then ReLU;
 *             w1_raw = bf16(h_w1) . bf16(W2)^T + b2, wf_raw = bf16(h_wf) . bf16(Wf2)^T + bf2; v_raw (row-dot), the clamps,
 *             the fmaf chain over the agents, ELU and the final products f32 as in the f32 kernels; sn / xhat / act are
 *             saved in f32, unrounded.
 *   backward  tail gradients (gq, g_w1raw, g_wfraw, g_v) f32; gout1[:, :Hh] = bf16(g_w1raw) . bf16(W2) and
 *             gout1[:, Hh:2Hh] = bf16(g_wfraw) . bf16(Wf2), each masked by its ReLU; the V and b1 blocks f32.  w1_raw /
 *             wf_raw are re-derived with the forward's bf16 instruction sequence (bit-identical: same clamp masks).
 *   The weight, bias and LayerNorm-parameter gradients stay the f32 split-K products of the f32 saved matrices.  The
 *   weights stay the f32 parameters: fragments are rounded in the kernel, so there is no bf16 copy to keep current.
 *
 * Supported: hyper_hidden_dim Hh = 128, mixing_embed_dim Em = 64 (the reference's sizes), n_agents J in {2, 3, 6, 12},
 * state_dim S <= 16 J (the shipped 2j/2r, 3j/4r, 6j/8r and 12j/16r scenarios; J = 12 runs both layers in passes); everything else returns
 * MACJD_EUNSUPPORTED and the caller keeps the unfused kernels.  Narrow states, S <= 16 (J - 1), run variants of the f32
 * kernels that guard every first-layer weight load; with bf16 operands S <= 16 (J - 1) (even J: 16 (J - 2)) is
 * unsupported (the entry points return MACJD_EUNSUPPORTED; macjd_mixer_fused_supported does not know the operand type).
 */
typedef struct macjd_mixerf_io {
    int64_t M;                 /* rows */
    int32_t J, S, Hh, Em;      /* agents, state_dim, hyper_hidden_dim, mixing_embed_dim */
    int32_t save;              /* forward: != 0 stores sn / xhat / act */
    int32_t operand_dtype;     /* 0: exact f32 products, 1: bf16 operands with f32 accumulation (see above); else MACJD_EINVAL */
    float ln_eps;  float reserved_f;
    const float* s;   int64_t s_ld;      /* [M,S] state rows */
    const float* q;            /* [M,J] agent Q-values (contiguous) */
    const float* ln_w; const float* ln_b;      /* state_norm.{weight,bias} [S] */
    const float* W1; const float* b1;          /* merged first layer [2Hh+2Em, S] row-major (row stride S), bias [2Hh+2Em]:
                                                  rows = hyper_w_1.0 | hyper_w_final.0 | V.0 | hyper_b_1 */
    const float* W2; const float* b2;          /* hyper_w_1.2     [J Em, Hh], [J Em] */
    const float* Wf2; const float* bf2;        /* hyper_w_final.2 [Em, Hh],  [Em]   */
    const float* wV2; const float* bV2;        /* V.2             [1, Em],   [1]    */
    float* y;                  /* [M] Q_tot (forward out) */
    float* sn; float* xhat;    /* [M,S] contiguous (forward out when save; sn unused by backward) */
    float* act;                /* [M, 2Hh+2Em] contiguous (forward out when save, backward in) */
    const float* gy;           /* [M] dL/dy (backward in) */
    float* gq;                 /* [M,J]        (backward outs) */
    float* gout1;              /* [M, 2Hh+2Em] */
    float* g_w1raw;            /* [M, J Em]    */
    float* g_wfraw;            /* [M, Em]      */
    float* g_v;                /* [M]          */
} macjd_mixerf_io;

int macjd_mixer_fused_supported(int32_t J, int32_t S, int32_t Hh, int32_t Em);   /* 1 / 0 */
int macjd_mixer_fused_forward(const macjd_mixerf_io* io, void* hip_stream);
/* The eval and the target mixer of one learner update (reference core/qmix.py:151 and :187: the same module class on
 * two parameter sets and two Q inputs, same states) as ONE grid: `saved` (save = 1: the eval mixer, whose activations the
 * backward needs) and `plain` (save = 0) must agree in J / S / M.  Results equal the two single launches bit for bit. */
int macjd_mixer_fused_forward_pair(const macjd_mixerf_io* saved, const macjd_mixerf_io* plain, void* hip_stream);
int macjd_mixer_fused_backward(const macjd_mixerf_io* io, void* hip_stream);
/* macjd_mixer_fused_backward that forms dL/dy itself from the TD loss's inputs (macjd_td_loss's expression; td->y = this
   mixer's forward output, td->tq the target values, rows = td->B x td->gy_cols) and tot_m[0] = the batch's mask sum
   (macjd_td_mask_sum): io->gy is not read, td->gy is not written.  Takes the loss launch off the update's serial chain;
   bit-identical gradients.  td->stats != NULL: one extra workgroup of the same grid computes the loss's logged sums
   (stats[0..2] = loss, mean(y), mean(target) — core/qmix.py:194, 212-213; stats[3] is left alone), so that they need neither
   a launch nor a stream of their own. */
int macjd_mixer_fused_backward_td(const macjd_mixerf_io* io, const macjd_tdloss_io* td, const float* tot_m, void* hip_stream);
/* The learner update's two mixers, the TD loss's gradient and the eval mixer's backward as ONE launch: `eval` (save = 1,
   with the backward's outputs gq / gout1 / g_w1raw / g_wfraw / g_v; gy is not read) and `target` (save = 0) as in
   macjd_mixer_fused_forward_pair, `td` and `tot_m` as in macjd_mixer_fused_backward_td with the rows the loss pairs up
   kept on chip: td->y = eval->y, td->tq = target->y + 1, y_sb = tq_sb = gy_cols > Tm1 (eval row (b, t) against target row
   (b, t + 1)).  Every output equals forward_pair + backward_td bit for bit, except target->y at row 0, which the loss
   never reads and this launch does not write.  td->stats is not read: the logged sums are the caller's (macjd_td_loss
   with td->gy = NULL after this launch).  J in {2, 3}; other J return MACJD_EINVAL. */
int macjd_mixer_fused_train(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                            const float* tot_m, void* hip_stream);
/* macjd_mixer_fused_train for episodes whose STATE does not change in time: every row (b, t) of `eval->s` that the loss
   reaches (t < Tm1) equals row (b, 0) — the caller's promise, not checked; rows t >= Tm1 get zero gradient, so what they
   hold does not matter (a full-length episode's row T is zeros).  The hyper-networks read only the state, so the `inp` operand of
   each of the mixer's five weight-gradient products (sn, xhat, three column blocks of act) repeats within an episode and
   dW = sum_m g[m]^T x[m] = sum_tiles (sum of the tile's rows of g)^T x[tile], provided no 16-row tile straddles two
   episodes.  Row mapping: T1 = td->gy_cols rows per episode, TPE = ceil(T1 / 16); workgroup b * TPE + k owns rows
   t = 16 k .. 16 k + 15 of episode b; rows t >= T1 are dead (loads clamped, nothing stored, gradient operands exact zeros).
   eval->y, target->y (rows >= 1) and eval->gq are written per row and equal macjd_mixer_fused_train bit for bit.  The
   operands of the weight-gradient products are written compact, n_tiles = B * TPE rows: sn / xhat / act hold the tile's
   row 0, the four *_sum buffers the sum over the tile's rows of what macjd_mixer_fused_train writes per row (fixed
   summation order, no atomics: deterministic; order in csrc/macjd_mixer.hip).  K = n_tiles in macjd_linear_wgrad_many.
   The per-row forms are NOT written: eval->sn / xhat / act / gout1 / g_w1raw / g_wfraw / g_v must be NULL (MACJD_EINVAL
   otherwise, as for M != B * gy_cols, J not in {2, 3}, differing operand types and a NULL compact pointer). */
typedef struct macjd_mixer_static_io {
    int64_t n_tiles;           /* B * ceil(gy_cols / 16) */
    float* sn; float* xhat;    /* [n_tiles, S] */
    float* act;                /* [n_tiles, 2Hh+2Em], 16-byte aligned */
    float* gout1_sum;          /* [n_tiles, 2Hh+2Em] */
    float* g_w1raw_sum;        /* [n_tiles, J Em]    */
    float* g_wfraw_sum;        /* [n_tiles, Em]      */
    float* g_v_sum;            /* [n_tiles]          */
} macjd_mixer_static_io;
int macjd_mixer_fused_train_static(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                   const float* tot_m, const macjd_mixer_static_io* st, void* hip_stream);
/* macjd_mixer_fused_train_static whose workgroups also leave, behind everything above (which stays bit-identical), what the
   weight-gradient REDUCE launch needs of the taken-action Q-head and of the LayerNorm — so that the update runs no
   partial-products launch (macjd_wgrad_io.kind).  Workgroup `tile` = (b, k) forms gq for the mixer rows t = 16 k .. 16 k + 15
   of episode b, i.e. for the 16 J agent rows n = (b T1 + 16 k) J .. of the Q-head grid (macjd_qhead_taken on M J rows):
     * slot `tile` of the Q-head's first-layer problem, ws1 (M = H, N = H + A + 1: the [H x N] part of the padded
       [Mp x Np] slot and the bias row, layout in macjd_wgrad_io.kind):
           dW1_part = g_hid^T x,  db1_part = column sums of g_hid,  g_hid[r][m] = (act_q[r][m] > 0) ? gq[r] w2[m] : 0,
           x[r] = [h[r], onehot(idx[r]), P[r]]  (an index outside [0, A) gives no one: macjd_qhead_taken's rule)
       on exact-f32 MFMA, rows ascending; rows with t >= T1 are read from clamped addresses and count exact zeros;
     * slot `tile` of its second-layer problem, ws2 (M = 1, N = H): dw2_part[m] = sum_r gq[r] act_q[r][m], db2_part = sum_r gq[r];
     * the tile's LayerNorm slot ln_slots[tile][2][S]: [0][k] = xhat[tile][k] u[k], [1][k] = u[k] with
       u[k] = sum_c W_first[c][k] gout1_sum[tile][c] (c ascending in eight runs of 48, combined as a fixed tree): the
       contracted problem's terms, dgamma = sum_tiles xhat u, dbeta = sum_tiles u.
   Fixed summation orders, no atomics; no workgroup reads what another one of the launch writes.  f32 operands only, H = 64,
   1 <= A <= 15.  MACJD_EINVAL: a NULL member, act_q / h not 16-byte aligned or a row stride that is not a multiple of 4
   or < H, idx_elem_size not 4 / 8, w_ld < S, a workspace smaller than n_tiles slots.  wg == NULL: the call above. */
typedef struct macjd_mixer_wgrad_block {
    const float* act_q; int64_t act_ld;    /* [M J, H] the Q-head's ReLU output (macjd_qtaken_io.act) */
    const float* h;     int64_t h_ld;      /* [M J, H] */
    const void* idx;    int32_t idx_elem_size, A;   /* [M J] int32 / int64 */
    const float* P;                        /* [M J] */
    const float* w2;                       /* [H] the Q-head's second layer */
    int32_t H, reserved;
    float* ws1; int64_t ws1_floats;        /* >= macjd_wgrad_slot_floats(H, H + A + 1, n_tiles) */
    float* ws2; int64_t ws2_floats;        /* >= macjd_wgrad_slot_floats(1, H, n_tiles) */
    float* ln_slots; int64_t ln_floats;    /* >= n_tiles * 2 * S */
    const float* W_first; int64_t w_ld;    /* [2Hh+2Em, S] the merged first layer (= eval->W1 with its row stride) */
} macjd_mixer_wgrad_block;
int macjd_mixer_fused_train_static_wgrad(const macjd_mixerf_io* eval, const macjd_mixerf_io* target, const macjd_tdloss_io* td,
                                         const float* tot_m, const macjd_mixer_static_io* st, const macjd_mixer_wgrad_block* wg,
                                         void* hip_stream);

/*
 * The agent side of a WHOLE episode batch in one launch: for t = 0 .. T-1 and every (env, agent) row
 *   h_t = GRUCell(x, h_{t-1})  with the input transform gi = W_ih ReLU(fc1 obs) + b_ih given (it does not change
 *         within an episode: the observation is static, reference simulation/environment.py:479-522),
 *   Q(h_t, a, P_a) for all a (MP-DQN multi-pass Q-head, core/networks.py:131-180), availability mask, epsilon-greedy
 *   choice and gather of the chosen power (core/mac.py:59-166, utils/action_selectors.py:15-62)
 * i.e. T x (macjd_gru_gates + two GEMMs + macjd_qhead_select) of the step-by-step rollout.  Nothing the agent
 * computes depends on the environment's outputs when the observation is static, so the T steps of the agent need no
 * env step in between (the env steps of the whole episode then run as ONE launch too: macjd_env_step_many).
 *
 * A workgroup owns 16 environments (16 J rows = J MFMA row tiles, tile j = agent j) for the whole episode: W_hh and
 * the Q-head's h-columns live in registers as MFMA operand fragments (wave w owns hidden units [16w, 16w+16) of all
 * three gates), h_t ping-pongs between two LDS tiles, two barriers per step, no global synchronisation at all —
 * environments are independent.  Exact float32 (v_mfma_f32_16x16x4_f32); gate and Q-head expressions and the Philox
 * exploration draws are those of macjd_gru_gates / macjd_qhead_select (same (row, counter) keying), so the episode equals
 * the step-by-step rollout up to the summation order of the two matrix products.
 * Supported:
 *   H = 64:  A in {5, 9, 17, 33}, any J >= 1 (J in {2, 3, 6} with A <= 17: one row tile per agent as described; every
 *            other size: four tiles of 16 consecutive rows n = env * J + agent per workgroup — the arithmetic per row is
 *            the same);
 *   H = 128: (J, A) in {2, 3} x {5, 9}, one row tile per agent only (eight waves, wave w = units [16w, 16w+16); the
 *            Q-head's h-columns are read from LDS instead of registers; same arithmetic per row).  No four-tile form and
 *            no A in {17, 33} at this size (they did not compile without scratch memory);
 *   MACJD_EUNSUPPORTED otherwise.  w_hh must be 16-byte aligned with contiguous rows of H floats.
 */
typedef struct macjd_agent_episode_io {
    int64_t n_envs;            /* E */
    int32_t T, J, H, A;        /* steps, agents, rnn_hidden_dim, n_actions */
    int32_t greedy_only, reserved;
    const float* gi;    int64_t gi_ld;   /* [E*J, 3H] input transform incl. b_ih; gi_ld = 0: one row for all */
    const float* P_all; int64_t p_ld;    /* [E*J, A] actor output; p_ld = 0: one row for all */
    const float* h0;                     /* [E*J, H] initial hidden state or NULL = zeros (mac.init_hidden) */
    const float* w_hh;  const float* b_hh;           /* rnn.weight_hh [3H,H], rnn.bias_hh [3H] */
    const float* W1;    int64_t w1_ld;               /* fc2_q_head.0.weight [H, H+A+1] */
    const float* b1;    const float* w2; const float* b2;   /* fc2_q_head.0.bias [H], .2.weight [H], .2.bias [1] */
    const void* avail;  int32_t avail_elem_size, reserved2;  /* optional mask (static), int32 / int64 elements */
    int64_t av_se, av_sj, av_sa;
    const float* eps;          /* [T] exploration probability of every step (device memory) */
    uint64_t seed;
    const uint64_t* counter_base;   /* device scalar: step t draws with counter = *counter_base + t + 1 */
    /* outputs, time-major staging rows of the batched runner */
    float*   hidden;    /* [T(+1), E, J, H] contiguous: row t = post-update h_t */
    int32_t* T_out;     /* [T, E, J] chosen discrete action */
    float*   P_out;     /* [T, E, J] chosen power */
    float*   h_final;   /* [E*J, H] optional: h_{T-1} (mac.hidden_states) */
} macjd_agent_episode_io;

int macjd_agent_episode_supported(int32_t J, int32_t H, int32_t A);
int macjd_agent_episode(const macjd_agent_episode_io* io, void* hip_stream);

/*
 * macjd_agent_episode with PER-STEP inputs: gi and P_all carry a leading time dimension and step t reads
 *   gi    + t * gi_lt + n * base.gi_ld + c * H + u      ([T, rows or 1, 3H])
 *   P_all + t * p_lt  + n * base.p_ld  + a              ([T, rows or 1, A])
 * For a MOVING scenario (macjd_motion_io): its observation shows frame min(k, F) for every env whatever the agents did,
 * so gi / P are functions of the step counter alone — one row per frame (base.gi_ld = base.p_ld = 0, gi_lt = 3H,
 * p_lt = A), computed by one launch for the whole episode — and, as in the static case, nothing the agent computes
 * depends on the environment's outputs (the env steps of the episode run as macjd_env_step_many_moving).
 * Everything else is macjd_agent_episode: step t of this launch computes what a T = 1 launch of macjd_agent_episode on
 * (gi[t], P_all[t], h0 = h_{t-1}, eps + t, *counter_base + t) computes, bit for bit.
 *   base.gi_ld / base.p_ld   as in macjd_agent_episode (0 = one row for all rows of a step)
 *   gi_lt >= 3H, p_lt >= A   time strides in elements; or 0: the step reads row block 0 (both 0: the launch equals
 *                            macjd_agent_episode).  MACJD_EINVAL for 0 < gi_lt < 3H or 0 < p_lt < A.
 * Supported: the one-tile-per-agent forms — H = 64 with (J, A) in {(2, 5), (3, 9), (6, 17)}, H = 128 with (J, A) in
 * {(2, 5), (3, 9)}; MACJD_EUNSUPPORTED otherwise (no four-tile form).
 */
typedef struct macjd_agent_episode_seq_io {
    macjd_agent_episode_io base;
    int64_t gi_lt, p_lt;
} macjd_agent_episode_seq_io;

int macjd_agent_episode_seq_supported(int32_t J, int32_t H, int32_t A);
int macjd_agent_episode_seq(const macjd_agent_episode_seq_io* io, void* hip_stream);

/*
 * Closed-loop episode launch for scanning radars (macjd_scan_desc): agent AND environment of a whole episode batch in
 * ONE launch.  With scanning beams the observation's theta_a columns change every step and depend, through the FSM, on
 * what the agents did, so macjd_agent_episode + macjd_env_step_many do not apply; environments are still independent of
 * each other, so the workgroup that owns 16 environments runs, for t = 0 .. T-1 and without leaving the kernel:
 *   observation-only work once per ENV (every agent sees the same state vector): x = ReLU(fc1 obs + b),
 *     gi = W_ih x + b_ih, actor P = sigma(L3 ReLU(L2 ReLU(L1 obs))); the first layers as (static columns, once per launch)
 *     + sum_r W[:, col_r] theta_a[r] — a different summation order than the GEMM, ~1e-7 relative;
 *   the agent step of macjd_agent_episode (same gate / Q-head expressions, same Philox draw (row, *counter_base + t + 1));
 *   the scanning env step of macjd_env_step_scan on the chosen actions (general all-float64 form, same Philox stream:
 *     counter = (global env, episode, step, slot / 4), key = env_seed): reward[t], terminated[t], r_dpj sums;
 *   (float) theta_a -> the theta_a columns of state[t + 1] / obs[t + 1, :, j, :] and the next agent step.
 * The kernel writes ONLY the theta_a columns (scan.st_col0 + r * scan.st_col_step) of the staging rows t < T; their
 * static columns are the caller's.  At exit theta_a, track, step, the theta_a columns of the env's state rows
 * (scan.state), scan.snr_no (last step's lobe), rdpj_sum and h_final hold what T single steps would have left.
 * Needs macjd_scenario_set_scan; shared scenario tables only (pe_tables must be NULL; macjd_agent_env_episode_scan_pe below
 * takes per-env tables).
 * Supported: H = 64, actor_hidden = 128, (J, R, A) in {(3, 4, 9), (2, 2, 5)}; MACJD_EUNSUPPORTED otherwise.
 */
typedef struct macjd_agent_env_episode_scan_io {
    int64_t n_envs;            /* E */
    int64_t env_offset;        /* global index of env 0 (keys the env's Philox stream) */
    int32_t T, J, R, H, A, S;  /* steps, agents, radars, rnn_hidden_dim, n_actions, state / observation width */
    int32_t actor_hidden, greedy_only;
    /* agent */
    const float* h0;                                  /* [E*J, H] initial hidden state or NULL = zeros */
    const float* fc1_w; const float* fc1_b;           /* fc1 [H, S], [H] */
    const float* w_ih;  const float* b_ih;            /* rnn.weight_ih [3H, H], rnn.bias_ih [3H] */
    const float* w_hh;  const float* b_hh;            /* rnn.weight_hh [3H, H], rnn.bias_hh [3H] */
    const float* a1_w;  const float* a1_b;            /* actor.0 [128, S] */
    const float* a2_w;  const float* a2_b;            /* actor.2 [128, 128] */
    const float* a3_w;  const float* a3_b;            /* actor.4 [A, 128] */
    const float* W1;    int64_t w1_ld;                /* fc2_q_head.0.weight [H, H+A+1] */
    const float* b1;    const float* w2; const float* b2;
    const void* avail;  int32_t avail_elem_size, reserved;   /* optional mask (static), int32 / int64 elements */
    int64_t av_se, av_sj, av_sa;
    const float* eps;          /* [T] exploration probability of every step (device memory) */
    uint64_t seed;             /* exploration draws */
    const uint64_t* counter_base;
    /* environment */
    uint64_t env_seed;         /* macjd_step_io.seed */
    const int32_t* episode;    /* [E] episode index, optional (NULL = 0) */
    uint8_t* track;     int64_t k_se, k_sx;           /* [E, R] read-modify-write */
    int32_t* step;                                    /* [E] read-modify-write */
    macjd_scan_io scan;        /* theta_a, the env's state rows and their theta_a columns, snr_no */
    const double* pe_tables;   /* must be NULL */
    /* outputs, time-major staging rows of the batched runner */
    float*   hidden;    /* [T(+1), E, J, H] row t = post-update h_t */
    int32_t* T_out;     /* [T, E, J] */
    float*   P_out;     /* [T, E, J] */
    float*   h_final;   /* [E*J, H] optional */
    float*   st_state;  /* [T(+1), E, S]: theta_a columns of rows t < T */
    float*   st_obs;    /* [T(+1), E, J, S]: likewise */
    float*   reward;    /* [T, E] */
    uint8_t* terminated;/* [T, E] */
    float*   rdpj_sum;  /* [E, 3] optional: the T steps' (r_d, r_p, r_j) are added in step order */
} macjd_agent_env_episode_scan_io;

int macjd_agent_env_episode_scan_supported(int32_t J, int32_t R, int32_t H, int32_t A);
int macjd_agent_env_episode_scan(const macjd_scenario* scenario, const macjd_agent_env_episode_scan_io* io, void* hip_stream);

/*
 * macjd_agent_env_episode_scan on per-env scenario tables (a scanning scenario batch, with or without a stepped antenna
 * pattern per env): the same launch, outputs and hand-over, with every table value read from the env's own columns.
 *   base       the shared call's block; base.pe_tables = the batch's scenario tables (macjd_step_io.pe_tables), non-NULL
 *   pe_flags, pe_stride, pe_tile   as macjd_step_io: pe_tile == 0 is the plain layout (every stride >= n_envs), pe_tile > 0
 *              the tiled one of ALL table sets (any width, also below the 16 envs of a workgroup; last tile padded)
 *   scan_pe    the per-env scan tables (macjd_scan_pe_io)
 *   pattern    tables == NULL: no pattern; else the per-env level tables (macjd_scan_pe_pattern_io), n_levels = L
 * The scenario handle is the batch's scanning handle: it supplies only J, R, episode_limit, the r_p bounds and the Pd
 * constants (macjd_env_step_scan_pe's rule).  A handle that carries pattern levels is accepted only with pattern.tables of
 * the same L (MACJD_EUNSUPPORTED otherwise).  MACJD_EINVAL: NULL base.pe_tables / pe_flags / scan_pe.tables, a stride below
 * n_envs in the plain layout, pe_tile < 0, L outside 1..MACJD_MAX_PATTERN_LEVELS, a handle without scan tables; every check
 * returns before any launch.  Results are bit-identical to T single macjd_env_step_scan_pe(_pattern) steps on the actions the
 * agent half chose; scan.snr_no ends as the last step's value from the env's own snr_no / snr_no_side row, or under a
 * pattern from its snr_no_lvl row of the last level.  Supported sizes: those of macjd_agent_env_episode_scan.
 */
typedef struct macjd_agent_env_episode_scan_pe_io {
    macjd_agent_env_episode_scan_io base;
    const uint8_t* pe_flags;
    int64_t pe_stride;
    int32_t pe_tile, reserved;
    macjd_scan_pe_io scan_pe;
    macjd_scan_pe_pattern_io pattern;
} macjd_agent_env_episode_scan_pe_io;

int macjd_agent_env_episode_scan_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A);
int macjd_agent_env_episode_scan_pe(const macjd_scenario* scenario, const macjd_agent_env_episode_scan_pe_io* io, void* hip_stream);

/*
 * macjd_agent_env_episode_scan for a MOVING scenario under scanning radars (macjd_motion_io + macjd_motion_scan_io, with
 * or without a stepped antenna pattern): the same launch and outputs, with the env's tables taken from the frame of the
 * step.  Env e runs step t on frame f = min(step0[e] + t, n_frames - 1), step0[e] = base.step[e] at entry (step counters
 * are per env: one workgroup may hold envs on different frames): the step's own rows from motion.frames[f] /
 * frame_flags[f], every scan row from motion_scan.scan_frames[f], under a pattern inv_width and the level rows from
 * motion_scan.pattern_frames[f].
 *   base         the shared call's block; base.pe_tables must be NULL (the frames are the tables)
 *   motion       frames, frame_flags, positions, position_columns, n_frames, n_pos and state (= base.scan.state) are
 *                read; snr_no must be NULL (the per-step value travels in base.scan.snr_no); frame_snr_no is not read
 *   motion_scan  scan_frames; pattern_frames together with n_levels = L, or neither
 * The observation of step t shows positions[min(step0[e] + t, n_frames)] at position_columns: besides the theta_a columns
 * the kernel writes these n_pos = 2R + 2J columns of the staging rows t < T (st_state, st_obs); every other column is the
 * caller's.  At exit theta_a, track, step, rdpj_sum, h_final, the theta_a columns and the position columns
 * (positions[min(step0[e] + T, n_frames)]) of the env's state rows hold what T single macjd_env_step_moving_scan steps
 * would have left, and scan.snr_no the last step's value of its frame: the snr_no / snr_no_side row of scan_frames, or
 * under a pattern the snr_no_lvl row of the last level in pattern_frames.  The env half is bit-identical to T single
 * macjd_env_step_moving_scan steps in their general all-float64 form on the actions the agent half chose.
 * The handle is the scenario's scanning handle (R, J, episode_limit, the r_p bounds, the Pd constants).  MACJD_EINVAL: NULL
 * frames / frame_flags / positions / position_columns / scan_frames, n_frames < 1 or not the handle's episode_limit,
 * n_pos != 2R + 2J, motion.snr_no != NULL, motion.state != base.scan.state (or another row stride), pattern_frames without
 * n_levels in 1..MACJD_MAX_PATTERN_LEVELS or n_levels without pattern_frames, a handle whose pattern L differs from
 * n_levels, a handle without scan tables, base.pe_tables != NULL; MACJD_EUNSUPPORTED: sizes other than those of
 * macjd_agent_env_episode_scan.  Every check returns before any launch.
 */
typedef struct macjd_agent_env_episode_moving_scan_io {
    macjd_agent_env_episode_scan_io base;   /* base.pe_tables must be NULL */
    macjd_motion_io       motion;
    macjd_motion_scan_io  motion_scan;
} macjd_agent_env_episode_moving_scan_io;

int macjd_agent_env_episode_moving_scan_supported(int32_t J, int32_t R, int32_t H, int32_t A);
int macjd_agent_env_episode_moving_scan(const macjd_scenario* scenario, const macjd_agent_env_episode_moving_scan_io* io,
                                        void* hip_stream);

/*
 * macjd_agent_env_episode_moving_scan on a PER-ENV moving scanning scenario batch (macjd_motion_pe_io +
 * macjd_motion_scan_pe_io, with or without a stepped antenna pattern per env): the same launch, outputs and hand-over, with
 * every frame read taken from the env's own column of the tiled per-env frame tables.  Env e runs step t on its own frame
 * f = min(step0[e] + t, n_frames - 1), step0[e] = base.step[e] at entry: row k of a table with ROWS rows per frame at
 * table[(((e / tile) * n_frames + f) * ROWS + k) * tile + e % tile] — the step's own rows from motion_pe.frames /
 * frame_flags, every scan row from motion_scan_pe.scan_frames, under a pattern inv_width and the level rows from
 * motion_scan_pe.pattern_frames.  Any tile width >= 1 (also below the 16 envs of a workgroup, and widths that do not
 * divide 16); the padded lanes of the last tile are never read.
 *   base            the shared call's block; base.pe_tables must be NULL (the frames are the tables)
 *   motion_pe       frames, frame_flags, positions, position_columns, n_frames, n_pos, tile and state (= base.scan.state)
 *                   are read; snr_no must be NULL (the per-step value travels in base.scan.snr_no); frame_snr_no is not read
 *   motion_scan_pe  scan_frames; pattern_frames together with n_levels = L, or neither
 * The observation of step t shows the env's positions of frame min(step0[e] + t, n_frames) (the positions table holds
 * n_frames + 1 frames per tile) at position_columns: besides the theta_a columns the kernel writes these n_pos = 2R + 2J
 * columns of the staging rows t < T (st_state, st_obs) and nothing else of them; every other column is the caller's.  At
 * exit theta_a, track, step, rdpj_sum, h_final, the theta_a columns and the position columns (frame
 * min(step0[e] + T, n_frames)) of the env's state rows hold what T single macjd_env_step_moving_scan_pe steps would have
 * left, and scan.snr_no the last step's value of the env's own frame: the snr_no / snr_no_side row of scan_frames, or under
 * a pattern the snr_no_lvl row of the last level in pattern_frames.  The env half is bit-identical to T single
 * macjd_env_step_moving_scan_pe steps in their general all-float64 form on the actions the agent half chose.
 * The handle is the batch's scanning handle (R, J, episode_limit, the r_p bounds, the Pd constants).  MACJD_EINVAL: NULL
 * frames / frame_flags / positions / position_columns / scan_frames / state, n_frames < 1 or not the handle's
 * episode_limit, n_pos != 2R + 2J, tile < 1, motion_pe.snr_no != NULL, motion_pe.state != base.scan.state (or another row
 * stride), pattern_frames without n_levels in 1..MACJD_MAX_PATTERN_LEVELS or n_levels without pattern_frames, a handle whose
 * pattern L is > 0 and differs from n_levels, a handle without scan tables, base.pe_tables != NULL; MACJD_EUNSUPPORTED:
 * sizes other than those of macjd_agent_env_episode_scan.  Every check returns before any launch.
 */
typedef struct macjd_agent_env_episode_moving_scan_pe_io {
    macjd_agent_env_episode_scan_io base;   /* base.pe_tables must be NULL */
    macjd_motion_pe_io       motion_pe;
    macjd_motion_scan_pe_io  motion_scan_pe;
} macjd_agent_env_episode_moving_scan_pe_io;

int macjd_agent_env_episode_moving_scan_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A);
int macjd_agent_env_episode_moving_scan_pe(const macjd_scenario* scenario, const macjd_agent_env_episode_moving_scan_pe_io* io,
                                           void* hip_stream);

/*
 * The agent side of a whole episode batch on PER-ENV moving frames (macjd_motion_pe_io) in ONE launch.  The observation
 * of env e at step t is its own state row with the position columns taken from its own frame min(step0[e] + t, F),
 * whatever the agents did, so — as for macjd_agent_episode_seq — nothing the agent computes depends on the environment's
 * outputs, and the env's T steps run as macjd_env_step_many_moving_pe.  Per-step gi / P rows would be [T, E J, 3H + A], so
 * the observation-only work is done in the kernel, once per ENV (every agent of an env sees the same observation), as in
 * macjd_agent_env_episode_scan.  Step t, row n = e J + j:
 *   obs = state[e, :S] with column position_columns[p] replaced by
 *         positions[(((e / tile) * (F + 1) + min(step0[e] + t, F)) * n_pos + p) * tile + e % tile],  p = 0 .. n_pos - 1,
 *         step0[e] = step[e] at entry (step == NULL: 0; read only); the padded lanes of the last tile are never read;
 *   x   = ReLU(fc1 obs + b),  gi = W_ih x + b_ih,  P = sigma(L3 ReLU(L2 ReLU(L1 obs)))  — the first layers as full
 *         S-column products in macjd_mlp_forward's k order with the bias after the sum;
 *   then exactly the step of macjd_agent_episode on (gi, P): the same gate and Q-head expressions, the same mask, first
 *   arg-max and epsilon-greedy rule, the same Philox keying (row n, *counter_base + t + 1).
 * A T-step launch equals T launches with T = 1 chained through h_final with step + t, eps + t and *counter_base + t, bit
 * for bit.  The kernel writes hidden, T_out, P_out and h_final only: no staging observation rows (they do not depend on
 * the actions: the caller fills them once) and nothing of the env.  Rows past n_envs in the last workgroup are computed
 * from clamped addresses and never stored.  The caller guarantees 0 <= position_columns[p] < S.
 * Supported: H = 64, actor_hidden = 128, (J, R, A) in {(3, 4, 9), (2, 2, 5)}; MACJD_EUNSUPPORTED otherwise.
 * MACJD_EINVAL, before any launch: a NULL required member (everything but h0, avail, step, counter_base, h_final, and eps
 * under greedy_only); T < 1; n_frames < 1; n_pos != 2R + 2J; tile < 1; st_se < S; S outside 1..48; avail_elem_size not 4 / 8
 * with a mask; w1_ld < H + A + 1; w_hh, w_ih or a2_w not 16-byte aligned (their rows are contiguous).
 */
typedef struct macjd_agent_episode_moving_pe_io {
    int64_t n_envs;            /* E */
    int32_t T, J, R, H, A, S;  /* steps, agents, radars, rnn_hidden_dim, n_actions, state / observation width */
    int32_t actor_hidden, greedy_only;
    /* agent */
    const float* h0;                                  /* [E*J, H] initial hidden state or NULL = zeros */
    const float* fc1_w; const float* fc1_b;           /* fc1 [H, S], [H] */
    const float* w_ih;  const float* b_ih;            /* rnn.weight_ih [3H, H], rnn.bias_ih [3H] */
    const float* w_hh;  const float* b_hh;            /* rnn.weight_hh [3H, H], rnn.bias_hh [3H] */
    const float* a1_w;  const float* a1_b;            /* actor.0 [128, S] */
    const float* a2_w;  const float* a2_b;            /* actor.2 [128, 128] */
    const float* a3_w;  const float* a3_b;            /* actor.4 [A, 128] */
    const float* W1;    int64_t w1_ld;                /* fc2_q_head.0.weight [H, H+A+1] */
    const float* b1;    const float* w2; const float* b2;
    const void* avail;  int32_t avail_elem_size, reserved;   /* optional mask (static), int32 / int64 elements */
    int64_t av_se, av_sj, av_sa;
    const float* eps;          /* [T] exploration probability of every step (device memory) */
    uint64_t seed;             /* exploration draws */
    const uint64_t* counter_base;
    /* observation */
    const float* state; int64_t st_se;      /* [E, S] every env's own state row, row stride st_se; position columns ignored */
    const int32_t* step;                    /* [E] step counters at entry, read only; NULL = zeros */
    const float* positions;                 /* [n_tiles, F + 1, n_pos, tile] (macjd_motion_pe_io) */
    const int32_t* position_columns;        /* int32 [n_pos] */
    int32_t n_frames, n_pos, tile, reserved2;   /* F >= 1, 2R + 2J, envs per tile >= 1 */
    /* outputs, time-major staging rows of the batched runner */
    float*   hidden;    /* [T(+1), E, J, H] row t = post-update h_t */
    int32_t* T_out;     /* [T, E, J] */
    float*   P_out;     /* [T, E, J] */
    float*   h_final;   /* [E*J, H] optional */
} macjd_agent_episode_moving_pe_io;

int macjd_agent_episode_moving_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A);
int macjd_agent_episode_moving_pe(const macjd_agent_episode_moving_pe_io* io, void* hip_stream);

/*
 * Double-DQN target values straight from the unrolled hidden states (reference core/qmix.py:138-147): for every row n
 *   a* = argmax_a Q_eval(h_e[n], a, P_e[n,a])   (no availability mask there, qmix.py:141-142)
 *   out[n] = Q_target(h_t[n], a*, P_t[n,a*])
 * in ONE launch: both Q-head base products W1[:, :H] h + b1 on the matrix cores (exact f32), both all-action Q-heads,
 * arg-max and gather.  Replaces two library GEMMs + two macjd_qhead_select launches behind the learner's scan.
 * h_e / h_t [n, H] (the same tensor when the agent body is shared), P_e / P_t [n, A].
 * Supported: H = 64 with A in {5, 9, 17, 33}; H = 128 with A in {5, 9, 17}; MACJD_EUNSUPPORTED otherwise.
 */
typedef struct macjd_doubleq_io {
    int64_t n_rows;
    int32_t H, A;
    const float* h_e; int64_t he_ld;  const float* h_t; int64_t ht_ld;
    const float* P_e; int64_t pe_ld;  const float* P_t; int64_t pt_ld;
    const float* W1_e; int64_t w1e_ld; const float* b1_e; const float* w2_e; const float* b2_e;   /* eval fc2_q_head */
    const float* W1_t; int64_t w1t_ld; const float* b1_t; const float* w2_t; const float* b2_t;   /* target fc2_q_head */
    float* out;              /* [n] */
    int64_t* argmax_out;     /* optional [n] */
    /* optional row map of P_e / P_t: p_group > 0 -> row n reads P row (n / p_group) * p_inner + n % p_inner (one actor
       row per SEQUENCE (b, j) for rows n = (b, t, j): p_group = T * J, p_inner = J).  p_group = 0: no map, p_inner is
       not read.  MACJD_EINVAL, before any launch, for p_group < 0 and for p_group > 0 with p_inner < 1 or
       p_inner > p_group (macjd_qhead_double_q and macjd_qheads_pair alike). */
    int64_t p_group, p_inner;
} macjd_doubleq_io;

int macjd_qhead_double_q_supported(int32_t H, int32_t A);
int macjd_qhead_double_q(const macjd_doubleq_io* io, void* hip_stream);
/* macjd_qhead_taken and macjd_qhead_double_q of one learner update (reference core/qmix.py:138-147 and :161-184: both read
 * the same unrolled hidden states, neither reads the other's result) as ONE grid; same A in both.  Results equal the two
 * single launches bit for bit.  H = 64 only (macjd_qhead_taken exists at H = 64 only): MACJD_EUNSUPPORTED at H = 128, where
 * the caller launches macjd_qhead_double_q on its own. */
int macjd_qheads_pair(const macjd_qtaken_io* taken, const macjd_doubleq_io* dq, void* hip_stream);

/*
 * Back-propagation through time of macjd_gru_sequence for ONE network: all T steps of the reverse chain for B*J
 * independent sequences in one launch (the training counterpart of the scan; the reference never trains through its
 * GRU unroll, so this has no line there).  The caller supplies the forward's inputs and outputs and the time-parallel
 * product gh = W_hh h_{t-1} + b_hh for every step; the kernel recomputes the gates with the forward kernels' own
 * sigmoid / tanh (so they are the gates that produced h_all) and walks t = T-1 ... 0.  With
 *   g      = dh_all[t] + carry          (carry = 0 at t = T-1)
 *   h_prev = h_all[t-1]                 (h0, or 0 when h0 is NULL, at t = 0)
 * per hidden unit:
 *   r = s(gi_r + gh_r)    z = s(gi_z + gh_z)    n = tanh(gi_n + r gh_n)
 *   da_n = g (1 - z)(1 - n^2)
 *   da_z = g (h_prev - n) z (1 - z)
 *   da_r = da_n gh_n r (1 - r)
 *   dgi[t] = (da_r, da_z, da_n)
 *   dgh[t] = (da_r, da_z, da_n r)
 *   carry  = g z + W_hh^T dgh[t]
 * and dh0 = the final carry.  dh_all[t] is the gradient that reaches h_t from everything that READ h_t other than the
 * recurrence itself.  The weight gradients are time-parallel and left to the caller:
 *   dW_hh = dgh^T h_prev, db_hh = column sums of dgh, dW_ih / db_ih / dx from dgi.
 * All tensors contiguous float32; every output element is written exactly once (deterministic, no atomics).
 * NULL pointers (dh0 and h0 are optional) and non-positive B / T / J return MACJD_EINVAL; H other than 64 / 128 returns
 * MACJD_EUNSUPPORTED.
 */
typedef struct macjd_gru_bwd_io {
    int32_t B, T, J, H;            /* H = 64 or 128 */
    const float* gi;      /* [B,T,J,3H]  W_ih x_t + b_ih, gate order r,z,n (as macjd_gru_io)            */
    const float* gh;      /* [B,T,J,3H]  W_hh h_{t-1} + b_hh for every t: the caller's time-parallel product */
    const float* h_all;   /* [B,T,J,H]   the forward scan's stored h_t                                   */
    const float* h0;  int64_t h0_sb;   /* optional initial state, as macjd_gru_io (NULL = zeros)          */
    const float* w_hh;    /* [3H,H] row-major                                                            */
    const float* dh_all;  /* [B,T,J,H]   dL/dh_t from everything that READ h_t (not the recurrence)       */
    float* dgi;           /* [B,T,J,3H]  out                                                             */
    float* dgh;           /* [B,T,J,3H]  out (= dgi except the n gate: da_n * r)                         */
    float* dh0;           /* [B,J,H]     out, optional                                                   */
} macjd_gru_bwd_io;
int macjd_gru_sequence_backward_supported(int32_t H);   /* 1 for 64 and 128, else 0 */
int macjd_gru_sequence_backward(const macjd_gru_bwd_io* io, void* hip_stream);

/*
 * Gradient of the MP-DQN actor objective (Bester et al.; the reference never trains its actor, so this has no line
 * there) down to the OUTPUT gradients of the three actor layers, for N independent rows in ONE launch.  Per row n, with
 * the Q-head a constant and nothing flowing into h (base = W1q[:, :H] h + b1q is the caller's GEMM, as for macjd_qhead_io):
 *   a1 = relu(W1a x + b1a)   a2 = relu(W2a a1 + b2a)   u = W3a a2 + b3a   P = sigmoid(u)        (core/networks.py:116-129)
 *   z_a = base + W1q[:, H + a] + W1q[:, H + A] P_a        Q_a = w2q . relu(z_a) + b2q            (core/networks.py:131-180)
 *   L = - sum_n m[n] sum_a Q_na
 *   s_a = sum_k w2q[k] W1q[k, H + A] [z_ak > 0]
 *   g3[n, a] = dL/du = - m[n] s_a P_a (1 - P_a)
 *   g2 = (g3 W3a) * [a2 > 0]        g1 = (g2 W2a) * [a1 > 0]        qsum[n] = sum_a Q_na
 * The weight gradients are time-parallel products left to the caller (macjd_linear_wgrad):
 *   dW3a = g3^T a2, dW2a = g2^T a1, dW1a = g1^T x, the bias gradients the column sums of g3 / g2 / g1.
 * Exact float32 (v_mfma_f32_16x16x4_f32 for the three layers and the two transposed products, the weights in torch's own
 * [out, in] layout both ways; the per-action term on VALU, [N, A, H] is never materialised); P comes from the forward
 * kernels' sigmoid.  Every output element is written exactly once (no atomics, no workspace); a row with m[n] == 0
 * gets exact zeros in g1 / g2 / g3 (a1, a2 and qsum are written all the same).  All outputs are contiguous.
 * Supported: the actor chain within macjd_mlp_forward's limits (S <= 256, Ha <= 128 with ceil(Ha / 16) in {1,2,3,4,8},
 * one layer's LDS image + the activation strips <= 160 KB), H = 64 or 128, A <= 33.  NULL required pointers, a
 * non-positive size or a row stride smaller than its row return MACJD_EINVAL; an unsupported shape returns
 * MACJD_EUNSUPPORTED with nothing launched.
 */
typedef struct macjd_actor_grad_io {
    int64_t n_rows;                    /* N */
    int32_t S, Ha, H, A;               /* observation width, actor hidden width, rnn_hidden_dim, n_actions */
    const float* x;     int64_t x_ld;      /* [N,S] observation rows, row stride in elements */
    const float* base;  int64_t base_ld;   /* [N,H] W1q[:, :H] h + b1q */
    const float* m;                        /* [N] row weights */
    const float* W1a; const float* b1a;    /* actor.0 [Ha,S], [Ha] */
    const float* W2a; const float* b2a;    /* actor.2 [Ha,Ha], [Ha] */
    const float* W3a; const float* b3a;    /* actor.4 [A,Ha], [A] */
    const float* W1q;   int64_t w1_ld;     /* fc2_q_head.0.weight [H, H+A+1], row stride */
    const float* w2q;                      /* fc2_q_head.2.weight [H] */
    const float* b2q;                      /* fc2_q_head.2.bias [1] or NULL (= 0): enters qsum only */
    float* a1; float* a2;                  /* out [N,Ha]: post-ReLU activations (weight-gradient operands) */
    float* g3;                             /* out [N,A] */
    float* g2; float* g1;                  /* out [N,Ha] */
    float* qsum;                           /* out [N], optional (NULL skips it) */
} macjd_actor_grad_io;
int macjd_actor_gradient_supported(int32_t S, int32_t Ha, int32_t H, int32_t A);   /* 1 / 0 */
int macjd_actor_gradient(const macjd_actor_grad_io* io, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MACJD_NETS_H */
