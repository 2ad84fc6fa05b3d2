"""Float64 NumPy restatement of the scanning-radar env step under a stepped antenna pattern (include/macjd.h,
macjd_scan_pattern_desc), written from the model's specification and independent of the HIP kernels and of the product's
table compiler: it derives its own bearings, side-lobe and per-level tables, keeps the beam state (azimuth, FSM) per env
and applies the step with a level 0..L + 1 per object.  Without ``radar_scan.pattern`` L = 0 and the model is
tests/scan_model.py's.  Vectorised over E.

Level of an object at bearing b for a radar with azimuth a, half beam h, lim = w + 2 h (w = 0 when tracking, else the
sweep): off = (b - a) + h wrapped once into [0, 360); level 0 iff full or off <= lim; otherwise lead = off - lim,
trail = 360 - off, x = min by (lead < trail), q = x * inv_width, level = L + 1 if q >= L else 1 + int(q).

Uniforms: as tests/scan_model.py (supplied [E, R + J] with the kernel's slot rules, or the facade's np.random order)."""
import numpy as np

from scan_model import bearing, det_prob, wrap


def derive(sc):
    """Scan and level tables from the scenario's parsed parameters (own derivation).  Level tables are [L + 2, R]: row 0
    main, rows 1..L the pattern's levels, row L + 1 the side lobe."""
    R, J = sc.num_radars, sc.num_jammers
    rs = sc.radar_scan
    dt = float(rs["step_seconds"])
    t = sc.tables
    pat = rs.get("pattern")
    gains = [float(g) for g in pat["gain_db"]] if pat else []
    L = len(gains)
    d = {"L": L}
    d["half"] = np.array([float(r["theta_m"]) / 2 for r in sc.radars])
    d["sweep"] = np.array([360.0 * dt / float(r["t_s"]) for r in sc.radars])
    d["swm"] = np.fmod(d["sweep"], 360.0)
    d["full"] = (d["sweep"] + 2 * d["half"]) >= 360.0
    d["az0"] = np.array([wrap(float(r["theta_a"])) for r in sc.radars])
    d["bt"] = np.array([bearing(r["position"], sc.target_position) for r in sc.radars])
    d["bj"] = np.array([[bearing(r["position"], q["position"]) for r in sc.radars] for q in sc.jammers]).reshape(J, R)
    d["inv_width"] = np.array([1.0 / (float(pat["level_width"]) * h) for h in d["half"]]) if pat else np.ones(R)
    rho = [1.0] + [10 ** (g / 10) for g in gains] + [10 ** (float(rs["sidelobe_db"]) / 10)]
    d["rho"] = np.array(rho)
    gr = np.zeros((L + 2, R)); GaPs = np.zeros((L + 2, R)); snr_no = np.zeros((L + 2, R)); pd_no = np.zeros((L + 2, R))
    for k, rk in enumerate(rho):
        for r in range(R):
            pn = t["radar_Pn"][r]
            if k == 0:
                gr[k, r], GaPs[k, r] = t["radar_gr"][r], t["radar_GaPs"][r]
            else:
                gr[k, r] = t["radar_gr"][r] * rk
                GaPs[k, r] = t["radar_GaPs"][r] * (rk * rk)
            s_no = GaPs[k, r] / pn if pn > 1e-18 else 0.0
            snr_no[k, r] = max(0.0, s_no)
            pd_no[k, r] = float(det_prob(snr_no[k, r], sc.pd_consts))
    d["gr"], d["GaPs"], d["snr_no"], d["pd_no"] = gr, GaPs, snr_no, pd_no
    return d


def level(beta, a, h, w, full, inv_width, L):
    off = (beta - a) + h
    off = np.where(off < 0.0, off + 360.0, off)
    off = np.where(off >= 360.0, off - 360.0, off)
    lim = w + 2 * h
    main = full | (off <= lim)
    lead = off - lim
    trail = 360.0 - off
    x = np.where(lead < trail, lead, trail)
    q = x * inv_width
    beyond = q >= float(L)
    k = np.where(beyond, L + 1, 1 + np.where(beyond | main, 0.0, q).astype(np.int64))
    return np.where(main, 0, k)


class ScanPatternModel:
    def __init__(self, sc, E):
        self.sc, self.E = sc, int(E)
        self.R, self.J = sc.num_radars, sc.num_jammers
        self.d = derive(sc)
        self.L = self.d["L"]
        self.track = np.zeros((self.E, self.R), dtype=bool)
        self.step_count = np.zeros(self.E, dtype=np.int64)
        self.theta_a = np.tile(self.d["az0"], (self.E, 1))
        # hits per level 0..L + 1: the target paths (every env, radar, step) and the recorded jammer actions
        self.count_target = np.zeros(self.L + 2, dtype=np.int64)
        self.count_jammer = np.zeros(self.L + 2, dtype=np.int64)

    def reset(self, mask=None):
        sel = np.ones(self.E, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.track[sel] = False
        self.step_count[sel] = 0
        self.theta_a[sel] = self.d["az0"]

    def n_deception_draws(self, T, P):
        sc, R = self.sc, self.R
        denom = sc.tables["jr_denom"].reshape(self.J, R)
        n = np.zeros(self.E, dtype=np.int64)
        for j in range(self.J):
            Tj = T[:, j].astype(np.int64)
            pmin, pmax = sc.jammers[j]["power_min"], sc.jammers[j]["power_max"]
            actual = pmin + np.clip(P[:, j], 0.0, 1.0) * (pmax - pmin)
            jam = (Tj >= 1) & (Tj <= 2 * R)
            tgt = np.where(jam, (Tj + 1) // 2 - 1, 0)
            n += (jam & (actual > 0) & (denom[j, tgt] >= 0.0) & (Tj % 2 == 0)).astype(np.int64)
        return n

    def draw_uniforms(self, T, P):
        """np.random draws in the facade's order (env by env): R radar draws, then one per valid deception action."""
        R, J = self.R, self.J
        nd = self.n_deception_draws(T, P)
        u = np.full((self.E, R + J), 2.0)
        for e in range(self.E):
            for k in range(R + int(nd[e])):
                u[e, k] = np.random.rand()
        return u

    def step(self, T, P, u, arith32=False):
        sc, d, t = self.sc, self.d, self.sc.tables
        E, R, J, L = self.E, self.R, self.J, self.L
        T = np.asarray(T).astype(np.int64)
        a = self.theta_a.copy()
        s = self.track.copy()
        w = np.where(s, 0.0, d["sweep"][None, :])
        cols = np.arange(R)[None, :]
        lv_t = level(d["bt"][None, :], a, d["half"][None, :], w, d["full"][None, :], d["inv_width"][None, :], L)
        self.count_target += np.bincount(lv_t.ravel(), minlength=L + 2)
        GaPs = d["GaPs"][lv_t, cols]
        pd_no = d["pd_no"][lv_t, cols]
        snr_no = d["snr_no"][lv_t, cols]
        denom_t = t["jr_denom"].reshape(J, R)
        weak = (t["jr_flags"].reshape(J, R) & 1) != 0
        rows = np.arange(E)

        supp = np.zeros((E, R))
        supp_mask = np.zeros((E, R), dtype=bool)
        r_p = np.zeros(E)
        prj_out = np.full((E, J), -1.0)
        dec_tgt = np.full((E, J), -1, dtype=np.int64)
        snr_f = np.zeros((E, J))
        lv_jam = np.full((E, J), -1, dtype=np.int64)
        for j in range(J):
            Tj = T[:, j]
            jam = (Tj >= 1) & (Tj <= 2 * R)
            tgt = np.where(jam, (Tj + 1) // 2 - 1, 0)
            jtype = Tj % 2
            pmin, pmax = float(sc.jammers[j]["power_min"]), float(sc.jammers[j]["power_max"])
            rng = pmax - pmin
            if arith32:
                Pc = np.clip(np.asarray(P[:, j], dtype=np.float32), np.float32(0), np.float32(1))
                act_f = np.float32(pmin) + Pc * np.float32(rng)
                actual = act_f.astype(np.float64)
                norm = ((act_f - np.float32(pmin)) / np.float32(rng)).astype(np.float64) if rng > 1e-6 else np.zeros(E)
            else:
                Pc = np.clip(np.asarray(P[:, j], dtype=np.float64), 0.0, 1.0)
                actual = pmin + Pc * rng
                norm = (actual - pmin) / rng if rng > 1e-6 else np.zeros(E)
            r_p = r_p + (sc.rp_max + (sc.rp_min - sc.rp_max) * norm)
            den = denom_t[j, tgt]
            recorded = jam & (actual > 0.0) & (den >= 0.0)
            # receive gain by the level of the jammer's bearing from the chosen radar
            lj = level(d["bj"][j, tgt], a[rows, tgt], d["half"][tgt], np.where(s[rows, tgt], 0.0, d["sweep"][tgt]),
                       d["full"][tgt], d["inv_width"][tgt], L)
            self.count_jammer += np.bincount(lj[recorded], minlength=L + 2)
            lv_jam[:, j] = np.where(recorded, lj, -1)
            grj = d["gr"][lj, tgt]
            live = recorded & (den > 1e-18)
            dsafe = np.where(live, den, 1.0)
            if arith32:
                num = (act_f * np.float32(t["jam_gj"][j])) * grj.astype(np.float32)
                q = np.where(weak[j, tgt], (num / dsafe.astype(np.float32)).astype(np.float64),
                             num.astype(np.float64) / dsafe)
            else:
                q = (actual * t["jam_gj"][j] * grj) / dsafe
            prj = np.where(live & (q > 0.0), q, 0.0)
            prj_out[:, j] = np.where(recorded, prj, -1.0)
            is_sup = recorded & (jtype == 1)
            is_dec = recorded & (jtype == 0)
            supp[rows[is_sup], tgt[is_sup]] += prj[is_sup]
            supp_mask[rows[is_sup], tgt[is_sup]] = True
            dec_tgt[:, j] = np.where(is_dec, tgt, -1)
            Pn_t = t["radar_Pn"][tgt]
            ok = is_dec & (Pn_t > 1e-18)
            sf = (t["radar_D"][tgt] * prj) / np.where(ok, Pn_t, 1.0)
            snr_f[:, j] = np.where(ok & (sf > 0.0), sf, 0.0)

        den = t["radar_D"][None, :] * supp + t["radar_Pn"][None, :]
        snr_w = np.where(den > 1e-18, GaPs / np.where(den > 1e-18, den, 1.0), 0.0)
        pd = det_prob(snr_w, sc.pd_consts)
        detected = u[:, :R] <= pd

        prod = np.ones((E, R))
        hit_mask = np.zeros((E, R), dtype=bool)
        n_dec = np.zeros(E, dtype=np.int64)
        for j in range(J):
            is_dec = dec_tgt[:, j] >= 0
            uj = u[rows, np.minimum(R + n_dec, R + J - 1)]
            n_dec += is_dec
            pd_f = det_prob(snr_f[:, j], sc.pd_consts)
            hit = is_dec & (uj <= pd_f)
            safe = np.minimum(pd_f, 0.999999)
            tg = dec_tgt[:, j]
            prod[rows[hit], tg[hit]] *= (1.0 - safe[hit])
            hit_mask[rows[hit], tg[hit]] = True

        r_d = np.zeros(E)
        r_j = np.zeros(E)
        r_j_dec = np.zeros(E)
        for r in range(R):
            r_d = r_d + np.where(detected[:, r], t["radar_rd_pen"][r], 0.0)
            red = pd_no[:, r] - pd[:, r]
            r_j = r_j + np.where(supp_mask[:, r] & (red > 0.0), red, 0.0)
            r_j_dec = r_j_dec + np.where(hit_mask[:, r], 1.0 - prod[:, r], 0.0)
        r_j = r_j + r_j_dec
        reward = r_d + r_p + r_j

        # beam advance
        x = a + d["swm"][None, :]
        x = np.where(x >= 360.0, x - 360.0, x)
        self.theta_a = np.where(detected, d["bt"][None, :], np.where(s, a, x))
        self.track = detected
        self.step_count = self.step_count + 1
        terminated = self.step_count >= sc.episode_limit
        return {"track": detected.copy(), "terminated": terminated, "theta_a": self.theta_a.copy(), "pd": pd,
                "snr": np.where(snr_w > 0.0, snr_w, 0.0), "snr_no": snr_no, "prj": prj_out,
                "out": np.stack([reward, r_d, r_p, r_j], axis=1), "level_target": lv_t, "level_jammer": lv_jam}
