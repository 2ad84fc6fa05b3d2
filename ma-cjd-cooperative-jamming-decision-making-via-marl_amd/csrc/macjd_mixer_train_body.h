// The body of mixer_fused_train_kernel / mixer_fused_train_wgrad_kernel (macjd_mixer.hip includes this text into both, so
// that the kernels without the weight-gradient block stay the very code they were).  In scope where it is included:
// J, BF, NARROW, STATIC (compile-time), io, tio, td, tot_m; with MX_TRAIN_WG defined to 1 also wb (macjd_mixer_wgrad_block).
    constexpr int LDG = J * MX_EM + 8;
    constexpr int LDF = MX_EM + 8;
    constexpr int KQ1 = J * MX_EM / 16;
    constexpr int KQF = MX_EM / 16;
    __shared__ MixerTrainLds<J> L;
    const int lane = threadIdx.x & 63;
    const int wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = wave8 & 3;
    const bool eval_half = wave8 < 4;
    const int li = lane & 15, g = lane >> 4;
    // rows of this workgroup: [m0, m0 + 16) below Mev (eval) and [m0 + 1, m0 + 17) below Mtg (target)
    const int64_t tile = blockIdx.x;
    int64_t m0 = tile * 16, Mev = io.M, Mtg = io.M;
    if constexpr (STATIC) {   // tile k of episode b: rows t = 16 k .. 16 k + 15 of that episode only, the rest of the tile is dead
        const int T1 = (int)td.gy_cols, tpe = (T1 + 15) / 16;
        const int b = (int)blockIdx.x / tpe, k = (int)blockIdx.x - b * tpe;
        m0 = (int64_t)b * T1 + 16 * k;
        Mev = (int64_t)(b + 1) * T1;
        Mtg = Mev + 1 < io.M ? Mev + 1 : io.M;
    }
    const float* Hs = L.ev.Hs;   // the eval mixer's first-layer output of the tile = `act`

    // the loss inputs of this lane's rows (4 g + r, and li for the V head), requested before the forward's loads
    float rw[5], term[5], mk[5];
    bool live[5];
    if (eval_half) {
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int row = r < 4 ? 4 * g + r : li;
            const int64_t mc = (m0 + row < Mev) ? m0 + row : Mev - 1;
            const int cols = (int)td.gy_cols;
            const int b = (int)(mc / cols), t = (int)(mc - (int64_t)b * cols);
            const int tc = t < td.Tm1 ? t : td.Tm1 - 1;
            term[r] = td.terminated[b * td.t_sb + tc * td.t_st] ? 1.0f : 0.0f;
            mk[r] = td.filled[b * td.f_sb + tc * td.f_st] ? 1.0f : 0.0f;
            rw[r] = td.reward[b * td.r_sb + tc * td.r_st];
            live[r] = t < td.Tm1;
        }
    }

    MixerKeep<J> K;
    f32x4 D1[KQ1], Df[KQF];
    if (eval_half) {
        if constexpr (STATIC) {
            macjd_mixerf_io eio = io;
            eio.M = Mev;
            mixer_fused_forward_body<J, J, true, true, true, BF, NARROW, true>(eio, m0, wave, L.ev, &K, tile);
        } else {
            mixer_fused_forward_body<J, J, true, true, true, BF, NARROW>(io, m0, wave, L.ev, &K);
        }
        if (wave == 0 && g == 0) L.ys[li] = K.y;
    } else {
        MixerKeep<J> Kt;
        if constexpr (STATIC) {
            macjd_mixerf_io etio = tio;
            etio.M = Mtg;
            mixer_fused_forward_body<J, J, false, true, true, BF, NARROW>(etio, m0 + 1, wave, L.tg, &Kt);
        } else {
            mixer_fused_forward_body<J, J, false, true, true, BF, NARROW>(tio, m0 + 1, wave, L.tg, &Kt);
        }
        if (wave == 0 && g == 0) L.tqs[li] = Kt.y;
    }
    // transposed second-layer fragments of this wave's gout1 column tile n = 16 wave8 + li (B[k][n] = W2[k][n], k = 16 Q +
    // 4 g + jj), requested while the tail gradients run
    {
        const int n = 16 * wave8 + li;
#pragma unroll
        for (int Q = 0; Q < KQ1; ++Q)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) D1[Q][jj] = io.W2[(int64_t)(BF ? mx_kq<KQ1>(Q, g) + jj : 16 * Q + 4 * g + jj) * MX_HH + n];
#pragma unroll
        for (int Q = 0; Q < KQF; ++Q)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) Df[Q][jj] = io.Wf2[(int64_t)(BF ? mx_kq<KQF>(Q, g) + jj : 16 * Q + 4 * g + jj) * MX_HH + n];
    }
    float wvo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) wvo[i] = io.wV2[(threadIdx.x + 512 * i) & (MX_EM - 1)];
    __syncthreads();   // ys / tqs of the tile

    if (eval_half) {
        const float scale = 2.0f / tot_m[0];
        float gyv[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int row = r < 4 ? 4 * g + r : li;
            const float target = rw[r] + td.gamma * (1.0f - term[r]) * L.tqs[row];
            const float gv = scale * mk[r] * (L.ys[row] - target);
            gyv[r] = live[r] ? gv : 0.0f;
        }
        const int e = 16 * wave + li;
        float gb1_sum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * g + r;
            const int64_t m = m0 + row;
            const float b1r = Hs[row * MX_LDH + MX_RELU + e];
            float hid = mx_clamp(b1r, -5.0f, 5.0f);
            float w1r[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                w1r[j] = K.acc2[j][r] + K.b2e[j];
                hid = fmaf(K.qv[r][j], mx_clamp(w1r[j], 0.0f, 5.0f), hid);
            }
            const float h = hid > 0.0f ? hid : expm1f(hid);
            const float wfr = K.accf[r] + K.bfe;
            const float ghid = gyv[r] * mx_clamp(wfr, 0.0f, 5.0f) * (hid > 0.0f ? 1.0f : h + 1.0f);
            const float gwf = (wfr >= 0.0f && wfr <= 5.0f) ? gyv[r] * h : 0.0f;
            const float gb1 = (b1r >= -5.0f && b1r <= 5.0f) ? ghid : 0.0f;
            L.Gf[row * LDF + e] = gwf;
            if constexpr (STATIC) {
                gb1_sum = r == 0 ? gb1 : gb1_sum + gb1;
            } else if (m < Mev) {
                io.g_wfraw[m * MX_EM + e] = gwf;
                io.gout1[m * MX_N1 + MX_RELU + e] = gb1;
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float gw = (w1r[j] >= 0.0f && w1r[j] <= 5.0f) ? ghid * K.qv[r][j] : 0.0f;
                L.G1[row * LDG + j * MX_EM + e] = gw;
                if (!STATIC && m < Mev) io.g_w1raw[m * (J * MX_EM) + j * MX_EM + e] = gw;
                const float t = mx_sum16(ghid * mx_clamp(w1r[j], 0.0f, 5.0f));
                if (li == 0) L.gq_part[wave][row][j] = t;
            }
        }
        if constexpr (STATIC) {   // the b1 block of gout1: this lane's four rows above, then the four lane groups
            gb1_sum += __shfl_xor(gb1_sum, 16, 64);
            gb1_sum += __shfl_xor(gb1_sum, 32, 64);
            if (g == 0) io.gout1[tile * MX_N1 + MX_RELU + e] = gb1_sum;
#if MX_TRAIN_WG
            if (g == 0) reinterpret_cast<float*>(&L.tg)[WGB_GS + MX_RELU + e] = gb1_sum;
#endif
        }
        if (wave == 0 && g == 0) {   // v = clamp(v_raw, -5, 5): row li
            const int64_t m = m0 + li;
            const float gv = (K.v_raw >= -5.0f && K.v_raw <= 5.0f) ? gyv[4] : 0.0f;
            L.gv_s[li] = gv;
            if (!STATIC && m < Mev) io.g_v[m] = gv;
        }
    }
    __syncthreads();
#if MX_TRAIN_WG
    // the tile's agent rows of h and of the Q-head's ReLU output, requested here: in flight under the products below
    WgbLoads<J> wgl;
    wgb_load<J>(wb, m0 * J, Mev * J, wgl);
#endif
    // dL/dq: the four embed blocks' partial sums in fixed order
    if (threadIdx.x < 16 * J) {
        const int row = threadIdx.x / J, j = threadIdx.x - row * J;
        if (m0 + row < Mev)
            io.gq[(m0 + row) * J + j] = (L.gq_part[0][row][j] + L.gq_part[1][row][j]) + (L.gq_part[2][row][j] + L.gq_part[3][row][j]);
    }
    // input gradients of the second layers, masked by the first layer's ReLU: column tile n of [0, Hh) and of [Hh, 2 Hh)
    {
        f32x4 a1 = f32x4{0.f, 0.f, 0.f, 0.f}, af = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BF) {
#pragma unroll
            for (int P = 0; P < KQ1 / 2; ++P) a1 = mx_mfma_bf16(mx_a_bf16<KQ1>(L.G1 + li * LDG, P, g), mx_b_bf16<KQ1>(D1, P), a1);
#pragma unroll
            for (int P = 0; P < KQF / 2; ++P) af = mx_mfma_bf16(mx_a_bf16<KQF>(L.Gf + li * LDF, P, g), mx_b_bf16<KQF>(Df, P), af);
        } else {
            const float* gp = L.G1 + li * LDG + 4 * g;
            const float* fp = L.Gf + li * LDF + 4 * g;
#pragma unroll
            for (int Q = 0; Q < KQ1; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(gp + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], D1[Q][jj], a1, 0, 0, 0);
            }
#pragma unroll
            for (int Q = 0; Q < KQF; ++Q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(fp + 16 * Q);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) af = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], Df[Q][jj], af, 0, 0, 0);
            }
        }
        const int n = 16 * wave8 + li;
        float s1 = 0.0f, sf = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * g + r;
            const int64_t m = m0 + row;
            const float v1 = (Hs[row * MX_LDH + n] > 0.0f) ? a1[r] : 0.0f;
            const float vf = (Hs[row * MX_LDH + MX_HH + n] > 0.0f) ? af[r] : 0.0f;
            if constexpr (STATIC) {
                s1 = r == 0 ? v1 : s1 + v1;
                sf = r == 0 ? vf : sf + vf;
            } else if (m < Mev) {
                io.gout1[m * MX_N1 + n] = v1;
                io.gout1[m * MX_N1 + MX_HH + n] = vf;
            }
        }
        if constexpr (STATIC) {   // this lane's four rows above, then the four lane groups
            s1 += __shfl_xor(s1, 16, 64);
            s1 += __shfl_xor(s1, 32, 64);
            sf += __shfl_xor(sf, 16, 64);
            sf += __shfl_xor(sf, 32, 64);
            if (g == 0) {
                io.gout1[tile * MX_N1 + n] = s1;
                io.gout1[tile * MX_N1 + MX_HH + n] = sf;
#if MX_TRAIN_WG
                reinterpret_cast<float*>(&L.tg)[WGB_GS + n] = s1;
                reinterpret_cast<float*>(&L.tg)[WGB_GS + MX_HH + n] = sf;
#endif
            }
        }
    }
#if MX_TRAIN_WG
    wgb_load_row<J>(wb, m0 * J, Mev * J, wgl);   // (the second-layer fragments are dead: their registers are free)
#endif
    if constexpr (STATIC) {
        // column sums over the tile's LDS rows, row 0 first: g_w1raw / g_wfraw (threads 0 .. J Em + Em - 1), the V block of
        // gout1 (threads 256 .. 256 + Em - 1, each row under its own ReLU mask) and g_v (thread 256 + Em)
        const int c = threadIdx.x;
        if (c < J * MX_EM) {
            float s = L.G1[c];
#pragma unroll
            for (int row = 1; row < 16; ++row) s += L.G1[row * LDG + c];
            io.g_w1raw[tile * (J * MX_EM) + c] = s;
        } else if (c < J * MX_EM + MX_EM) {
            const int cf = c - J * MX_EM;
            float s = L.Gf[cf];
#pragma unroll
            for (int row = 1; row < 16; ++row) s += L.Gf[row * LDF + cf];
            io.g_wfraw[tile * MX_EM + cf] = s;
        } else if (c >= 256 && c < 256 + MX_EM) {
            const int k = c - 256;   // wvo[0] = wV2[k]
            float s = (Hs[2 * MX_HH + k] > 0.0f) ? L.gv_s[0] * wvo[0] : 0.0f;
#pragma unroll
            for (int row = 1; row < 16; ++row) s += (Hs[row * MX_LDH + 2 * MX_HH + k] > 0.0f) ? L.gv_s[row] * wvo[0] : 0.0f;
            io.gout1[tile * MX_N1 + 2 * MX_HH + k] = s;
#if MX_TRAIN_WG
            reinterpret_cast<float*>(&L.tg)[WGB_GS + 2 * MX_HH + k] = s;
#endif
        } else if (c == 256 + MX_EM) {
            float s = L.gv_s[0];
#pragma unroll
            for (int row = 1; row < 16; ++row) s += L.gv_s[row];
            io.g_v[tile] = s;
        }
#if MX_TRAIN_WG
        static_assert(STATIC && !BF, "the weight-gradient block rides in the static f32 training launch");
        static_assert(WGB_SX + 16 * J * WGB_PITCH + 64 <= (int)(sizeof(MixerFwdLds<J>) / 4), "L.tg too small");
        static_assert(16 * J * (WGB_PITCH + 64) <= (int)(sizeof(MixerFwdLds<J>) / 4), "L.ev too small");
        wgb_finish<J>(wb, wgl, io.xhat, io.S, tile, (int64_t)gridDim.x, L.gq_part, reinterpret_cast<float*>(&L.tg),
                      reinterpret_cast<float*>(&L.ev));
#endif
        return;
    }
    // the V head's one-output second layer: outer product g_v wV2, masked: columns [2 Hh, 2 Hh + Em)
#pragma unroll
    for (int i = 0; i < 16 * MX_EM / 512; ++i) {
        const int idx = threadIdx.x + 512 * i;
        const int row = idx / MX_EM, k = idx - row * MX_EM;
        if (m0 + row < Mev)
            io.gout1[(m0 + row) * MX_N1 + 2 * MX_HH + k] = (Hs[row * MX_LDH + 2 * MX_HH + k] > 0.0f) ? L.gv_s[row] * wvo[i] : 0.0f;
    }
