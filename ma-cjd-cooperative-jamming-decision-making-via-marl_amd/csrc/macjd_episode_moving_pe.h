// macjd_episode_moving_pe.h — the agent side of a whole episode batch on PER-ENV moving frames as one launch (included by
// macjd_episode.hip; C-ABI: include/macjd_nets.h, macjd_agent_episode_moving_pe_io).
//
// agent_episode_kernel's premise holds per env: the observation of env e at step t is its own state row with the position
// columns taken from its own frame min(step0[e] + t, F), whatever the agents did, so the agent's T steps need no env step
// in between (the env's T steps run as macjd_env_step_many_moving_pe).  What is gone is "one row per frame for the whole
// batch": per-step gi / P rows would be [T, E J, 3H + A] (about 1 GB at E = 4096, T = 100), so the observation-only work is
// done here, as in the closed-loop kernel (macjd_episode_scan.h, S1 - S4) whose agent half this kernel restates WITHOUT the
// env half, the env's tables and the staging-row writes.
//
// Mapping (J agents, R radars, H = 64, actor hidden 128, A actions; 256 threads = 4 waves, 16 envs per workgroup):
//   * resident MFMA B fragments per wave w: W_hh and W_ih rows of hidden units [16w, 16w+16) of all three gates, the Q-head's
//     h-columns, fc1 and the actor's first layer over the S observation columns; actor layer 2 is staged in LDS once per
//     launch — nothing but the position values is fetched from global memory inside the step loop;
//   * every agent of an env sees the same observation, so the observation-only work is ONE 16-row tile per workgroup: the 16
//     observation rows live in LDS (static columns from the env's state row once per launch; the n_pos = 2R + 2J position
//     columns rewritten every step), and fc1 / the actor's first layer are full S-column MFMA products in
//     mlp_forward_kernel's k order with the bias after the sum.  NOT the incremental form (static part + sum W[:, col] v):
//     position columns reach several hundred and that form moved h by 2e-5 in the closed-loop kernel;
//   * per step: (S1) x = ReLU(fc1 obs) and the actor's first layer -> LDS; (S2) position columns of step t + 1 -> the
//     observation tile (thread = (env row, column): the value was requested from the env's own column of the positions
//     table in front of S1); gi = W_ih x + b_ih and actor layer 2 on MFMA, gh, gates, h_t exactly as agent_episode_kernel;
//     (S3) actor layer 3 + sigmoid -> P in LDS, Q-head base on MFMA; (S4) all-action Q-head, mask, first arg-max,
//     epsilon-greedy with the Philox draw of (row n, *counter_base + t + 1) (wave = agent tile).
//   THREE barriers per step, behind S1, S2 and S3.  The closed-loop kernel's fourth, behind S4, separates the selection from
//   the env half that reads it; here nothing in LDS is written by S4, and what S4 reads (P, the base) is next written in
//   S3 of step t + 1, two barriers later.  The observation tile is read in S1 only and written in S2: the barriers behind
//   S2 and S3 lie between that write and the next read.
// Rows past n_envs in the last workgroup are computed from the clamped env index and never stored.
#pragma once

namespace macjd {

// the closed-loop kernel's actor constants under this kernel's own names (this header stands on its own beside that one)
constexpr int MP_AH = 128;            // actor hidden width
constexpr int MP_ALD = MP_AH + 8;     // LDS pitch of the actor's activations (= 8 mod 16 floats)
constexpr int MP_AKQ = MP_AH / 16;    // quads of a K = 128 product

template <int J, int R, int A, int SQ>
__global__ void __launch_bounds__(256) agent_episode_moving_pe_kernel(const macjd_agent_episode_moving_pe_io io) {
    static_assert(J <= 4, "one wave per agent tile in the Q-head phase");
    static_assert(16 * A <= 256, "actor layer 3: one thread per (env, action)");
    constexpr int NPOS = 2 * R + 2 * J;   // position columns of a state row
    static_assert(16 * NPOS <= 256, "position columns: one thread per (env, column)");
    constexpr int OLD = 16 * SQ + 8;      // LDS pitch of the observation tile (S <= 16 SQ columns, zero-padded)
    __shared__ __attribute__((aligned(16))) float Hl[2][J][16 * EP_LD];   // h_{t-1} / h_t, ping-pong
    __shared__ __attribute__((aligned(16))) float Bl[J][16 * EP_LD];      // Q-head base of the current step
    __shared__ float Wq[(A + 2) * EP_H];                                  // Q-head columns, as agent_episode_kernel
    __shared__ __attribute__((aligned(16))) float Ol[16 * OLD];           // the 16 envs' observation rows
    __shared__ __attribute__((aligned(16))) float Xl[16 * EP_LD];         // x = ReLU(fc1 obs)
    __shared__ __attribute__((aligned(16))) float A1l[16 * MP_ALD], A2l[16 * MP_ALD];   // actor layers 1, 2
    __shared__ __attribute__((aligned(16))) float W2l[MP_AH * MP_ALD];    // actor layer 2 weights [out][in], pitch MP_ALD
    __shared__ __attribute__((aligned(16))) float W3l[A * MP_AH];         // actor layer 3 weights
    __shared__ float Pl[16 * A];                                          // actor output P[row][a] of the current step

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const int64_t e0 = (int64_t)blockIdx.x * 16;
    const int T = io.T, S = io.S;
    const int64_t E = io.n_envs;
    const int64_t N = E * J;
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
            Bh[c][Q] = *reinterpret_cast<const f32x4*>(io.w_hh + off);   // 16-byte aligned (checked by the entry point)
            Bi[c][Q] = *reinterpret_cast<const f32x4*>(io.w_ih + off);
        }
#pragma unroll
    for (int Q = 0; Q < EP_KQ; ++Q)
        Bq[Q] = *reinterpret_cast<const f32x4_u*>(io.W1 + (int64_t)(16 * wave + li) * io.w1_ld + 16 * Q + 4 * g);
    // actor layer 2 (128 x 128) in LDS, read as B fragments: 16 ds_read_b128 per wave and step instead of 64 resident VGPRs
    for (int idx = tid; idx < MP_AH * (MP_AH / 4); idx += 256) {
        const int n = idx / (MP_AH / 4), k4 = idx - n * (MP_AH / 4);
        *reinterpret_cast<f32x4*>(&W2l[n * MP_ALD + 4 * k4]) = *reinterpret_cast<const f32x4*>(io.a2_w + (int64_t)n * MP_AH + 4 * k4);
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
    // zero padding and bias-after-sum as mlp_forward_kernel ----
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
        const float x = io.state[e * io.st_se + (c < S ? c : S - 1)];
        Ol[row * OLD + c] = c < S ? x : 0.0f;
    }
    // actor layer 3: thread -> (row = tid & 15, action = tid >> 4), clamped for the threads past 16 A
    const int r3 = tid & 15, a3 = (tid >> 4) < A ? (tid >> 4) : A - 1;
    const float b3 = io.a3_b[a3];
    for (int idx = tid; idx < A * MP_AH; idx += 256) W3l[idx] = io.a3_w[idx];
    for (int idx = tid; idx < (A + 2) * EP_H; idx += 256) {
        const int a = idx / EP_H, uu = idx - a * EP_H;
        Wq[idx] = (a <= A) ? io.W1[(int64_t)uu * io.w1_ld + EP_H + a] : io.w2[uu];
    }
    const float b2 = io.b2[0];
    // ---- position columns: thread -> (env row pr = tid & 15, column pp = tid >> 4), clamped for the threads past 16 NPOS.
    // Env e's value p of frame k is positions[(((e / tile) * (F + 1) + k) * NPOS + p) * tile + e % tile]: its own column, so
    // the padded lanes of the last tile are never read for a live env (a dead row reads env E - 1's) ----
    const int pr = tid & 15, pp = (tid >> 4) < NPOS ? (tid >> 4) : NPOS - 1;
    const bool pos_thread = tid < 16 * NPOS;
    const int F = io.n_frames;
    bool live_p;
    const int64_t ep = env_of(pr, live_p);
    const int64_t ptile = ep / io.tile;
    const float* __restrict__ pos_lane = io.positions + (ptile * (F + 1) * NPOS + pp) * (int64_t)io.tile + (ep - ptile * io.tile);
    const int64_t pos_fs = (int64_t)NPOS * io.tile;   // frame stride
    int pcolumn = io.position_columns[pp];            // in [0, S) by the caller's guarantee; clamped, so that a bad index
    pcolumn = pcolumn < 0 ? 0 : (pcolumn < S ? pcolumn : S - 1);   // can only misplace a value inside the tile
    int32_t pstep0 = io.step ? io.step[ep] : 0;
    pstep0 = pstep0 < 0 ? 0 : (pstep0 < F ? pstep0 : F);   // frame of step t: min(step0 + t, F); T + F stays far from 2^31
    auto pos_frame = [&](int t) -> int64_t { return pstep0 + t < F ? pstep0 + t : F; };
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
    const float pos0 = pos_lane[pos_frame(0) * pos_fs];
    __syncthreads();   // the state rows are in the tile: the first step's position columns go over them
    if (pos_thread) Ol[pr * OLD + pcolumn] = pos0;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        // the next step's position value of this thread's (env, column): requested here, stored behind S1's barrier
        const float pos_next = pos_lane[pos_frame(t + 1) * pos_fs];
        // ---- (S1) first layers on this step's observation tile ----
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
                    A1l[(4 * g + r) * MP_ALD + 16 * (2 * wave + tl) + li] = fmaxf(aa[tl][r] + bfa[tl], 0.0f);
            }
        }
        __syncthreads();
        // ---- (S2) position columns of step t + 1; gi = W_ih x + b_ih (one tile, shared by the agents); actor layer 2; gh;
        // gates ----
        if (pos_thread) Ol[pr * OLD + pcolumn] = pos_next;
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
            for (int Q = 0; Q < MP_AKQ; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&A1l[li * MP_ALD + 16 * Q + 4 * g]);
                f32x4 b[2];
#pragma unroll
                for (int tl = 0; tl < 2; ++tl)
                    b[tl] = *reinterpret_cast<const f32x4*>(&W2l[(16 * (2 * wave + tl) + li) * MP_ALD + 16 * Q + 4 * g]);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int tl = 0; tl < 2; ++tl) a2[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], b[tl][jj], a2[tl], 0, 0, 0);
            }
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    A2l[(4 * g + r) * MP_ALD + 16 * (2 * wave + tl) + li] = fmaxf(a2[tl][r] + b2a[tl], 0.0f);
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
            const float* arow = &A2l[r3 * MP_ALD];
            const float* wrow = &W3l[a3 * MP_AH];
#pragma unroll 4
            for (int k4 = 0; k4 < MP_AH / 4; ++k4) {
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
                if (live_q) {
                    const int64_t o = (int64_t)t * N + nq;
                    io.T_out[o] = chosen;
                    io.P_out[o] = pc;
                }
            }
        }
        // no barrier closes the step (see the header comment)
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

extern "C" int macjd_agent_episode_moving_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A) {
    return (H == macjd::EP_H && ((J == 3 && R == 4 && A == 9) || (J == 2 && R == 2 && A == 5))) ? 1 : 0;
}

// every check returns before any launch (include/macjd_nets.h lists them)
extern "C" int macjd_agent_episode_moving_pe(const macjd_agent_episode_moving_pe_io* io, void* hip_stream) {
    using namespace macjd;
    const char* me = "macjd_agent_episode_moving_pe";
    if (!io) return set_err(MACJD_EINVAL, "%s: NULL io", me);
    if (!macjd_agent_episode_moving_pe_supported(io->J, io->R, io->H, io->A) || io->actor_hidden != MP_AH)
        return set_err(MACJD_EUNSUPPORTED, "%s: unsupported J / R / H / A / actor width (see include/macjd_nets.h)", me);
    if (io->n_envs < 0 || io->T < 1 || !io->fc1_w || !io->fc1_b || !io->w_ih || !io->b_ih || !io->w_hh || !io->b_hh || !io->a1_w ||
        !io->a1_b || !io->a2_w || !io->a2_b || !io->a3_w || !io->a3_b || !io->W1 || !io->b1 || !io->w2 || !io->b2 || !io->hidden ||
        !io->T_out || !io->P_out || !io->state || !io->positions || !io->position_columns || (!io->greedy_only && !io->eps))
        return set_err(MACJD_EINVAL, "%s: bad n_envs / T or NULL pointer", me);
    if (io->S < 1 || io->S > 48) return set_err(MACJD_EINVAL, "%s: state width S outside 1..48", me);
    if (io->st_se < io->S) return set_err(MACJD_EINVAL, "%s: st_se smaller than S", me);
    if (io->n_frames < 1) return set_err(MACJD_EINVAL, "%s: n_frames < 1", me);
    if (io->n_pos != 2 * io->R + 2 * io->J) return set_err(MACJD_EINVAL, "%s: n_pos must equal 2R + 2J", me);
    if (io->tile < 1) return set_err(MACJD_EINVAL, "%s: tile < 1", me);
    if (io->w1_ld < io->H + io->A + 1) return set_err(MACJD_EINVAL, "%s: row stride smaller than the row", me);
    if (io->avail && io->avail_elem_size != 4 && io->avail_elem_size != 8)
        return set_err(MACJD_EINVAL, "%s: avail_elem_size must be 4 or 8", me);
    if ((((uintptr_t)io->w_hh) | ((uintptr_t)io->w_ih) | ((uintptr_t)io->a2_w)) & 15)
        return set_err(MACJD_EINVAL, "%s: w_hh, w_ih and a2_w must be 16-byte aligned", me);
    if ((io->n_envs + 15) / 16 > 0x7fffffff) return set_err(MACJD_EINVAL, "%s: too many envs for one launch", me);
    if (io->n_envs == 0) return MACJD_OK;
    const dim3 grid((unsigned)((io->n_envs + 15) / 16)), block(256);
    hipStream_t st = (hipStream_t)hip_stream;
    if (io->J == 3) hipLaunchKernelGGL((agent_episode_moving_pe_kernel<3, 4, 9, 3>), grid, block, 0, st, *io);
    else hipLaunchKernelGGL((agent_episode_moving_pe_kernel<2, 2, 5, 3>), grid, block, 0, st, *io);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_err(MACJD_EDEVICE, "macjd_agent_episode_moving_pe: %s", hipGetErrorString(err));
    return MACJD_OK;
}
