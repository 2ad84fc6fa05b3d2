"""Float64 model of the moving scanning env step (include/macjd.h, macjd_env_step_moving_scan): the frame-oracle idea of
tests/motion_cases.py on the scanning restatements.  One ``scan_model.ScanModel`` (``scan_pattern_model.ScanPatternModel``
under a stepped pattern) per frame scenario, used unchanged; env e, whose step counter is k, runs on the model of frame
min(k, F - 1) with the beam azimuths, FSM bits and counters carried across frames.  A step runs every frame some env is in
on the whole batch and keeps each env's rows from its own frame; the envs of other frames get the no-op action there, so the
frame model's own jammer counters count each recorded action once.

The coverage record (what the CPU test asserts on the GPU cases): target paths and recorded jammer actions per lobe / level,
detections in a frame whose bear_tgt differs from frame 0's with the beam left on that bearing, and the smallest distance of
a consumed uniform from its detection probability."""
import numpy as np

from scan_model import ScanModel, det_prob
from scan_pattern_model import ScanPatternModel


class MovingScanModel:
    def __init__(self, frames, n_envs):
        self.frames = frames[:-1]            # frame F is only ever shown, never stepped on
        self.F = len(self.frames)
        self.E = int(n_envs)
        sc0 = frames[0]
        self.R, self.J = sc0.num_radars, sc0.num_jammers
        self.pattern = "pattern" in sc0.radar_scan
        self.L = len(sc0.radar_scan["pattern"]["gain_db"]) if self.pattern else 0
        self.models = {}
        self.az0 = self._model(0).d["az0"].copy()
        self.track = np.zeros((self.E, self.R), dtype=bool)
        self.step_count = np.zeros(self.E, dtype=np.int64)
        self.theta_a = np.tile(self.az0, (self.E, 1))
        n = self.L + 2
        self.count_target = np.zeros(n, dtype=np.int64)    # per level 0..L + 1 (without a pattern: [main, side])
        self.count_jammer = np.zeros(n, dtype=np.int64)
        self.followed = 0             # detections in a frame whose bear_tgt differs in bits from frame 0's, beam on it after
        self.min_margin = np.inf      # min |u - pd| over every consumed draw

    def _model(self, f):
        m = self.models.get(f)
        if m is None:
            m = self.models[f] = (ScanPatternModel if self.pattern else ScanModel)(self.frames[f], self.E)
        return m

    def reset(self, mask=None):
        sel = np.ones(self.E, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.track[sel] = False
        self.step_count[sel] = 0
        self.theta_a[sel] = self.az0   # az0 does not depend on the frame

    def frame_of(self):
        return np.minimum(self.step_count, self.F - 1)

    def positions_after(self, positions):
        """Rows of ``positions`` [F + 1, n_pos] the envs' state rows show now: frame min(counter, F)."""
        return positions[np.minimum(self.step_count, self.F)]

    def _margins(self, sc, T, u, out, sel):
        """|u - pd| of every draw the envs ``sel`` consumed: R radar draws, then one per valid deception action in jammer
        order (recorded <=> prj >= 0), whose false-target pd is re-derived from the reported received power."""
        R, J, t = self.R, self.J, sc.tables
        best = np.abs(u[sel, :R] - out["pd"][sel]).min()
        for e in np.flatnonzero(sel):
            k = 0
            for j in range(J):
                Tj = int(T[e, j])
                if out["prj"][e, j] >= 0.0 and Tj % 2 == 0:
                    tgt = (Tj + 1) // 2 - 1
                    pn = t["radar_Pn"][tgt]
                    sf = (t["radar_D"][tgt] * out["prj"][e, j]) / pn if pn > 1e-18 else 0.0
                    best = min(best, abs(u[e, R + k] - float(det_prob(max(sf, 0.0), sc.pd_consts))))
                    k += 1
        return best

    def step(self, T, P, u, arith32=False):
        T = np.asarray(T)
        fe = self.frame_of()
        out = None
        bt0 = self._model(0).d["bt"]
        for f in np.unique(fe):
            m = self._model(int(f))
            sel = fe == f
            m.theta_a, m.track, m.step_count = self.theta_a.copy(), self.track.copy(), self.step_count.copy()
            Tf = np.where(sel[:, None], T, 0)          # the other frames' envs do nothing here
            before = m.count_jammer.copy()
            res = m.step(Tf, P, u, arith32=arith32)
            jam = m.count_jammer - before
            self.count_jammer += jam
            if self.pattern:
                self.count_target += np.bincount(res["level_target"][sel].ravel(), minlength=self.L + 2)
            else:
                self.count_target += [int(res["in_target"][sel].sum()), int((~res["in_target"][sel]).sum())]
            moved = m.d["bt"].view(np.uint64) != bt0.view(np.uint64)
            self.followed += int((res["track"][sel] & moved[None, :] & (res["theta_a"][sel] == m.d["bt"][None, :])).sum())
            self.min_margin = min(self.min_margin, self._margins(self.frames[int(f)], T, u, res, sel))
            if out is None:
                out = {k: np.array(v, copy=True) for k, v in res.items()}
            else:
                for k, v in res.items():
                    out[k][sel] = v[sel]
        self.theta_a, self.track = out["theta_a"].copy(), out["track"].copy()
        self.step_count = self.step_count + 1
        out["terminated"] = self.step_count >= self.frames[0].episode_limit
        return out
