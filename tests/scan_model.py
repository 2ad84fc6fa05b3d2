"""Float64 NumPy restatement of the scanning-radar env step (include/macjd.h, macjd_scan_desc), written from the model's
specification and independent of the HIP kernel: it derives its own tables and bearings (np.arctan2), keeps the beam
state (azimuth, FSM) per env and applies today's step with the main- / side-lobe selections.  Vectorised over E.

Uniforms are supplied [E, R + J] with the kernel's slot rules (slot r < R: radar r's detection draw; slot R + k: the k-th
valid deception action in jammer order), or drawn from the global np.random stream in the single-env facade's order
(R draws, then one per valid deception action).  ``arith32`` follows the float32 power arithmetic of float32 actions
(NumPy-2 weak promotion), as the production kernel does."""
import numpy as np


def wrap(x):
    x = np.asarray(x, dtype=np.float64)
    return x - 360.0 * np.floor(x / 360.0)


def bearing(frm, to):
    frm = np.asarray(frm, dtype=np.float64).reshape(-1)
    to = np.asarray(to, dtype=np.float64).reshape(-1)
    return wrap(np.degrees(np.arctan2(to[1] - frm[1], to[0] - frm[0])))


def det_prob(snr, consts):
    A, c1, den_b = consts
    s = np.maximum(np.asarray(snr, dtype=np.float64), 0.0)
    Z = s + c1
    if abs(den_b) < 1e-9:
        return np.zeros_like(Z)
    B = (10 * Z - A) / den_b
    with np.errstate(over="ignore"):
        p = 1 / (1 + np.exp(-B))
    return np.where(B > 700, 1.0, np.where(B < -700, 0.0, p))


def derive(sc):
    """The scan tables from the scenario's parsed parameters (own derivation)."""
    R, J = sc.num_radars, sc.num_jammers
    dt = float(sc.radar_scan["step_seconds"])
    rho = 10 ** (float(sc.radar_scan["sidelobe_db"]) / 10)
    t = sc.tables
    d = {}
    d["half"] = np.array([float(r["theta_m"]) / 2 for r in sc.radars])
    d["sweep"] = np.array([360.0 * dt / float(r["t_s"]) for r in sc.radars])
    d["swm"] = np.fmod(d["sweep"], 360.0)
    d["full"] = (d["sweep"] + 2 * d["half"]) >= 360.0
    d["az0"] = np.array([wrap(float(r["theta_a"])) for r in sc.radars])
    d["bt"] = np.array([bearing(r["position"], sc.target_position) for r in sc.radars])
    d["bj"] = np.array([[bearing(r["position"], q["position"]) for r in sc.radars] for q in sc.jammers]).reshape(J, R)
    d["rho"] = rho
    d["gr_side"] = t["radar_gr"] * rho
    d["GaPs_side"] = t["radar_GaPs"] * (rho * rho)
    snr_side = np.zeros(R)
    pd_side = np.zeros(R)
    for r in range(R):
        pn = t["radar_Pn"][r]
        s_no = d["GaPs_side"][r] / pn if pn > 1e-18 else 0.0
        snr_side[r] = max(0.0, s_no)
        pd_side[r] = float(det_prob(snr_side[r], sc.pd_consts))
    d["snr_no_side"], d["pd_no_side"] = snr_side, pd_side
    return d


def in_lobe(beta, a, h, w, full):
    off = (beta - a) + h
    off = np.where(off < 0.0, off + 360.0, off)
    off = np.where(off >= 360.0, off - 360.0, off)
    return full | (off <= w + 2 * h)


class ScanModel:
    def __init__(self, sc, E):
        self.sc, self.E = sc, int(E)
        self.R, self.J = sc.num_radars, sc.num_jammers
        self.d = derive(sc)
        self.track = np.zeros((self.E, self.R), dtype=bool)
        self.step_count = np.zeros(self.E, dtype=np.int64)
        self.theta_a = np.tile(self.d["az0"], (self.E, 1))
        # lobe counters: [main, side] for the target paths (every env, radar, step) and the recorded jammer actions
        self.count_target = np.zeros(2, dtype=np.int64)
        self.count_jammer = np.zeros(2, dtype=np.int64)

    def reset(self, mask=None):
        sel = np.ones(self.E, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.track[sel] = False
        self.step_count[sel] = 0
        self.theta_a[sel] = self.d["az0"]

    def n_deception_draws(self, T, P):
        """Valid deception actions per env (the facade's extra draws), as the host decode counts them."""
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
        E, R, J = self.E, self.R, self.J
        T = np.asarray(T).astype(np.int64)
        a = self.theta_a.copy()
        s = self.track.copy()
        w = np.where(s, 0.0, d["sweep"][None, :])
        in_t = in_lobe(d["bt"][None, :], a, d["half"][None, :], w, d["full"][None, :])
        self.count_target += [int(in_t.sum()), int((~in_t).sum())]
        GaPs = np.where(in_t, t["radar_GaPs"][None, :], d["GaPs_side"][None, :])
        pd_no = np.where(in_t, t["radar_pd_no"][None, :], d["pd_no_side"][None, :])
        snr_no = np.where(in_t, t["radar_snr_no"][None, :], d["snr_no_side"][None, :])
        denom_t = t["jr_denom"].reshape(J, R)
        weak = (t["jr_flags"].reshape(J, R) & 1) != 0
        rows = np.arange(E)

        supp = np.zeros((E, R))
        supp_mask = np.zeros((E, R), dtype=bool)
        r_p = np.zeros(E)
        prj_out = np.full((E, J), -1.0)
        dec_tgt = np.full((E, J), -1, dtype=np.int64)
        snr_f = np.zeros((E, J))
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
            # receive gain by the jammer's bearing from the chosen radar
            a_t, h_t = a[rows, tgt], d["half"][tgt]
            inj = in_lobe(d["bj"][j, tgt], a_t, h_t, np.where(s[rows, tgt], 0.0, d["sweep"][tgt]), d["full"][tgt])
            self.count_jammer += [int((recorded & inj).sum()), int((recorded & ~inj).sum())]
            grj = np.where(inj, t["radar_gr"][tgt], d["gr_side"][tgt])
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
                "out": np.stack([reward, r_d, r_p, r_j], axis=1), "in_target": in_t}
