"""numpy float64 restatement of the device compiler of the beam frames of per-env moving scanning scenarios (include/macjd.h,
macjd_motion_scan_pe_compile_desc) in ITS operation order, composed of tests/motion_pe_model.py (the first compiler, whose
frames it reads), plus the case table shared by tests/test_moving_scan_pe_cpu.py and tests/test_moving_scan_pe_gpu.py.  Every
operation is one IEEE float64 operation on numpy arrays (numpy never fuses a multiply-add), so the model's bits are what a
correct device run must produce for everything but the pd_no rows (the device's exp is its own polynomial) and the bearing
rows (the device library's atan2 is its own)."""
import copy
import functools

import numpy as np

import motion_pe_model as mpe
import moving_scan_cases as msc
from scan_pattern_model import level as beam_level

from macjd_amd.scenario import (DEG_PER_RAD, MovingScanScenarioBatch, Scenario, motion_frame_dict, motion_scan_pe_in_rows,
                                pe_scan_pattern_rows, pe_scan_rows)

F_PE = mpe.F_PE            # episode limit (= frames) of every case
SIZES = [(2, 2), (3, 4), (6, 8), (3, 3)]   # three compiled sizes and a generic one
GAIN_DB = {0: None, 1: [-6.0], 4: [-3.0, -12.0, -17.0, -25.0], 6: [-2.0, -5.0, -9.0, -14.0, -20.0, -26.0]}
# the compiler cases: every size without and with the four-level pattern, 3j/4r also at one and six levels
CASES = [(J, R, L) for (J, R) in SIZES for L in (0, 4)] + [(3, 4, 1), (3, 4, 6)]
E0 = 19
N_SPECIAL = 6              # the four edge envs of motion_pe_model, the crosser and the seam env
config = mpe.config


def wrap(d):
    return d - 360.0 * np.floor(d / 360.0)


def circular(x, y):
    """Distance of two bearings in degrees on the circle: min(|x - y|, 360 - |x - y|)."""
    a = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64))
    return np.minimum(a, 360.0 - a)


def scan_slices(R, J):
    """Named row blocks of a scan column (include/macjd.h, macjd_scan_pe_io)."""
    names = ("half_beam", "sweep", "sweep_mod", "az0", "bear_tgt", "GaPs_side", "snr_no", "snr_no_side", "pd_no_side", "gr_side")
    s = {n: slice(i * R, (i + 1) * R) for i, n in enumerate(names)}
    s["bear_jam"] = slice(10 * R, 10 * R + J * R)
    return s


def pattern_slices(R, L):
    """Named row blocks of a pattern column (include/macjd.h, macjd_scan_pe_pattern_io)."""
    n = (L + 2) * R
    s = {"inv_width": slice(0, R)}
    for i, name in enumerate(("GaPs_lvl", "snr_no_lvl", "pd_no_lvl", "gr_lvl")):
        s[name] = slice(R + i * n, R + (i + 1) * n)
    return s


def scan_compile_model(column, scan_column, frames, snr_no, R, J, F, L, consts, deg_per_rad=DEG_PER_RAD):
    """One env: the first compiler's input column f64 [IN_ROWS] (its position rows), the beam compiler's input column f64
    [SCAN_IN_ROWS], the first compiler's outputs ``frames`` f64 [F, rows] and ``snr_no`` f64 [F, R] ->
    (scan_frames f64 [F, 10R + JR], pattern_frames f64 [F, R + 4(L+2)R] or None) in the operation order of include/macjd.h."""
    col = np.asarray(column, dtype=np.float64)
    si = np.asarray(scan_column, dtype=np.float64)
    assert si.shape == (motion_scan_pe_in_rows(R, L),)
    o = 8 * R + 6 * J
    tp0, tvdt = col[o:o + 2], col[o + 2:o + 4]
    o += 4
    rp0, rvdt = col[o:o + 2 * R].reshape(R, 2), col[o + 2 * R:o + 4 * R].reshape(R, 2)
    o += 4 * R
    jp0, jvdt = col[o:o + 2 * J].reshape(J, 2), col[o + 2 * J:o + 4 * J].reshape(J, 2)
    half, sweep, swm, az0 = (si[k * R:(k + 1) * R] for k in range(4))
    rho = si[4 * R]
    inv_width = si[4 * R + 1:5 * R + 1] if L else None
    rho_lvl = si[5 * R + 1:5 * R + 1 + L] if L else None
    dpr = np.float64(deg_per_rad)
    scan = np.zeros((F, pe_scan_rows(R, J)))
    pat = np.zeros((F, pe_scan_pattern_rows(R, L))) if L else None
    for f in range(F):
        fd = np.float64(f)
        t = tp0 + fd * tvdt
        rp = rp0 + fd * rvdt
        jp = jp0 + fd * jvdt
        bt = wrap(np.arctan2(t[1] - rp[:, 1], t[0] - rp[:, 0]) * dpr)
        bj = wrap(np.arctan2(jp[:, None, 1] - rp[None, :, 1], jp[:, None, 0] - rp[None, :, 0]) * dpr)   # [J, R]
        GaPs, Pn, pd_no, gr = (frames[f, k * R:(k + 1) * R] for k in (0, 1, 3, 5))

        def lobe(rho_k):
            gr_k = gr * rho_k
            GaPs_k = GaPs * (rho_k * rho_k)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(Pn > 1e-18, GaPs_k / Pn, 0.0)
            s_k = np.where(0.0 > q, 0.0, q)
            return GaPs_k, s_k, mpe.model_pd(s_k, consts), gr_k
        side = lobe(rho)
        scan[f] = np.concatenate([half, sweep, swm, az0, bt, side[0], snr_no[f], side[1], side[2], side[3], bj.reshape(-1)])
        if L:
            lv = [(GaPs, snr_no[f], pd_no, gr)] + [lobe(rho_lvl[k]) for k in range(L)] + [side]
            pat[f] = np.concatenate([inv_width] + [np.concatenate([x[tab] for x in lv]) for tab in range(4)])
    return scan, pat


def scan_compile_column(sc0):
    """The beam compiler's input column of a scanning scenario compiled at the start positions (the product's own)."""
    from macjd_amd.scenario import _scan_compile_inputs
    return _scan_compile_inputs(sc0)


def model_tables(scs, first="model"):
    """The two compilers' models on a list of moving scanning scenarios, stacked per env like MovingScanScenarioBatch's host
    arrays.  ``first="model"``: the beam compiler reads the first compiler's MODEL frames (what the device chain computes);
    ``first="host"``: it reads the scenario's host-compiled frames (the definition of a frame: the CPU proof)."""
    outs = []
    for sc in scs:
        R, J, F, L = sc.num_radars, sc.num_jammers, sc.episode_limit, sc.scan_pattern_levels
        ins = sc.motion_compile_inputs()
        if first == "model":
            o = mpe.compile_model(ins["column"], ins["weak"], R, J, F, sc.pd_consts)
        else:
            mt = sc.motion_tables
            o = {"frames": mt["frames"], "flags": mt["flags"], "snr_no": mt["snr_no"], "positions": mt["positions"]}
        o = dict(o)
        o["scan_frames"], pat = scan_compile_model(ins["column"], scan_compile_column(sc), o["frames"], o["snr_no"], R, J, F, L,
                                                   sc.pd_consts)
        if L:
            o["pattern_frames"] = pat
        outs.append(o)
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


# ---- the shared case table ------------------------------------------------------------------------------------------------
def _scanning(d, L, e=0):
    """``d`` with a ``radar_scan`` block on the motion clock (the per-radar t_s / theta_m cycle of tests/moving_scan_cases.py);
    env number ``e`` shifts ``sidelobe_db`` and every ``gain_db`` entry: they differ between the envs of a batch."""
    d = copy.deepcopy(d)
    rs = {"step_seconds": d["environment_params"]["motion"]["step_seconds"], "sidelobe_db": -30.0 - 0.5 * e}
    if L:
        rs["pattern"] = {"level_width": msc.PATTERN["level_width"], "gain_db": [g - 0.25 * e for g in GAIN_DB[L]]}
    d["environment_params"]["radar_scan"] = rs
    for i, r in enumerate(d["radars"]):
        r["t_s"], r["theta_m"] = msc.T_S[i % 4], msc.THETA_M[i % 4]
    return d


def _crosser(J, R):
    """The target and the last jammer fly past the resting radar 0 at close range: their bearings from it change by several
    degrees per frame, across the edge of the sector its beam covers from az0 = 355 degrees."""
    import motion_cases
    d = motion_cases.moving_ring_dict(J, R)
    r0 = d["radars"][0]["position"]
    d["radars"][0]["theta_a"] = 355.0
    d["protected_target"]["position"] = [r0[0] + 200.0, r0[1] - 40.0]
    d["jammers"][J - 1]["position"] = [r0[0] + 150.0, r0[1] + 40.0]
    mo = d["environment_params"]["motion"]
    mo["radar_velocity"][0] = [0.0, 0.0]
    mo["target_velocity"] = [0.0, 40.0]
    mo["jammer_velocity"][J - 1] = [0.0, -30.0]
    return d


def _seam(J, R):
    """The resting target lies due east of the resting radar 1, 1.7e-6 m to the south at 1000 m: a bearing about 1e-7 degrees
    below 360."""
    import motion_cases
    d = motion_cases.moving_ring_dict(J, R)
    t = d["protected_target"]["position"]
    d["radars"][1]["position"] = [float(t[0]) - 1000.0, float(t[1]) + 1.7e-6]
    mo = d["environment_params"]["motion"]
    mo["radar_velocity"][1] = [0.0, 0.0]
    mo["target_velocity"] = [0.0, 0.0]
    return d


@functools.lru_cache(maxsize=None)
def _case(J, R, L, E, limit):
    import motion_cases
    from macjd_amd.scenario import randomized_moving_scenario_dict
    base = motion_cases.moving_ring_dict(J, R)
    dicts = [_scanning(d, L, i) for i, d in enumerate(mpe._edge_dicts(J, R) + [_crosser(J, R), _seam(J, R)])]
    assert len(dicts) == N_SPECIAL
    e = 0
    while len(dicts) < E:   # the moving ring with per-env jitter (positions, powers, threat levels, velocities, azimuths)
        rng = np.random.default_rng([4343, e])
        d = randomized_moving_scenario_dict(base, rng, velocity_jitter=2.0, position_jitter=20.0)
        for r in d["radars"]:
            r["theta_a"] = float(r["theta_a"]) + float(rng.normal(0.0, 40.0))
        dicts.append(_scanning(d, L, len(dicts)))
        e += 1
    dicts = dicts[:E]
    return dicts, [Scenario.from_dict(d, config=config(limit)) for d in dicts]


def case(J, R, L, E=E0, limit=F_PE):
    """(sim-config dicts, their compiled moving scanning Scenarios) of the E-env case of a size and a number of pattern
    levels: the special envs first, then jittered moving rings.  Compiled once and shared."""
    return _case(J, R, L, E, limit)


def env_frames(d, limit=F_PE):
    """The static scanning Scenarios of frames 0..F of one env's sim-config (what ``MovingScanModel`` takes)."""
    return [Scenario.from_dict(motion_frame_dict(d, f), config=config(limit)) for f in range(limit + 1)]


def search_levels(scan_frames, pattern_frames, R, J, L):
    """Levels 0..L + 1 of the target [F, R] and of every jammer [F, J, R] at each radar in every frame of one env, with the
    beam resting at az0 in SEARCH (tests/scan_pattern_model.level; L = 0: 0 = main lobe, 1 = side lobe)."""
    s = scan_slices(R, J)
    half, sweep, az0 = (scan_frames[:, s[k]] for k in ("half_beam", "sweep", "az0"))
    full = sweep + 2 * half >= 360.0
    iw = pattern_frames[:, :R] if L else np.full_like(half, np.inf)
    bt = scan_frames[:, s["bear_tgt"]]
    bj = scan_frames[:, s["bear_jam"]].reshape(-1, J, R)
    with np.errstate(invalid="ignore"):
        lt = beam_level(bt, az0, half, sweep, full, iw, L)
        lj = beam_level(bj, az0[:, None], half[:, None], sweep[:, None], full[:, None], iw[:, None], L)
    return lt, lj


# ---- the step cases against MovingScanModel: one model per env ------------------------------------------------------------
STEP_MODEL_CASES = [(3, 4, 0), (3, 4, 4), (3, 3, 4)]
STEP_MODEL = dict(E=7, steps=F_PE + 2)


def step_model_inputs(J, R):
    """The actions and uniforms of the model run, step by step: (T int32 [E, J], P float64 [E, J], u float64 [E, R + J])."""
    from _harness import random_actions
    rng = np.random.default_rng(97 + 100 * J + R)
    for _ in range(STEP_MODEL["steps"]):
        T, P = random_actions(rng, STEP_MODEL["E"], J, R)
        yield T, P.astype(np.float64), rng.random((STEP_MODEL["E"], R + J))


@functools.lru_cache(maxsize=None)
def step_model_run(J, R, L):
    """``MovingScanModel`` (tests/moving_scan_model.py), one per env on that env's own frames, on the step inputs: a list of
    per-step dicts of [E, ...] arrays, and the models (their ``min_margin`` is the fairness record)."""
    from moving_scan_model import MovingScanModel
    E = STEP_MODEL["E"]
    dicts, _ = case(J, R, L, E=E)
    models = [MovingScanModel(env_frames(d), 1) for d in dicts]
    steps = []
    for T, P, u in step_model_inputs(J, R):
        outs = [m.step(T[e:e + 1], P[e:e + 1], u[e:e + 1]) for e, m in enumerate(models)]
        steps.append((T, P, u, {k: np.concatenate([np.atleast_1d(o[k]) for o in outs]) for k in outs[0]}))
    return steps, models


__all__ = ["CASES", "E0", "F_PE", "GAIN_DB", "MovingScanScenarioBatch", "N_SPECIAL", "SIZES", "case", "circular", "config",
           "env_frames", "model_tables", "pattern_slices", "scan_compile_model", "scan_slices", "search_levels", "wrap"]
