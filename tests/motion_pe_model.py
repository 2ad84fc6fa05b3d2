"""numpy float64 restatement of the device frame compiler of per-env moving scenarios (include/macjd.h,
macjd_motion_pe_compile_desc) in ITS operation order, plus the case table shared by tests/test_motion_pe_cpu.py and
tests/test_motion_pe_gpu.py.  Every operation is one IEEE float64 operation on numpy scalars / arrays (numpy never fuses a
multiply-add), so the model's bits are what a correct device run must produce for everything but pd_no (the device's exp is
its own polynomial)."""
import copy
import functools
import json
from types import SimpleNamespace

import numpy as np

import motion_cases as cases

from macjd_amd.scenario import (FOUR_PI_CUBED, MovingScenarioBatch, Scenario, motion_frame_dict, motion_pe_in_rows,
                                randomized_moving_scenario_dict)

F_PE = 5   # episode limit (= frames) of every case


def config(limit=F_PE):
    return SimpleNamespace(episode_limit=limit)


def pe_rows(R, J):
    return 6 * R + 3 * J + J * R


def model_pd(snr, consts):
    """scenario.detection_probability in the device's all-float64 form (csrc/macjd_env_dev.h, det_prob_batch): the same
    branches, elementwise."""
    A, c1, den_b = consts
    s = np.where(0.0 > snr, 0.0, snr)
    if abs(den_b) < 1e-9:
        return np.zeros_like(s)
    Z = np.minimum(s + c1, 1e300)
    B = (10.0 * Z - A) / den_b
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-B))
    p = np.where(B > 700.0, 1.0, p)
    return np.where(B < -700.0, 0.0, p)


def compile_model(column, weak, R, J, F, consts, c0=FOUR_PI_CUBED):
    """One env: input column f64 [IN_ROWS] + weak u8 [J] -> dict(frames f64 [F, rows], flags u8 [F, J*R], snr_no f64 [F, R],
    positions f32 [F + 1, 2R + 2J]) in the operation order of include/macjd.h."""
    col = np.asarray(column, dtype=np.float64)
    assert col.shape == (motion_pe_in_rows(R, J),)
    o = 0

    def take(n):
        nonlocal o
        a = col[o:o + n]
        o += n
        return a
    Pn, D, rd_pen, gr, num, rloss, rlatm, Ga = (take(R) for _ in range(8))
    pmin, pmax, gj, jloss, jlatm, bj = (take(J) for _ in range(6))
    tp0, tvdt = take(2), take(2)
    rp0, rvdt = take(2 * R).reshape(R, 2), take(2 * R).reshape(R, 2)
    jp0, jvdt = take(2 * J).reshape(J, 2), take(2 * J).reshape(J, 2)
    frames = np.zeros((F, pe_rows(R, J)))
    flags = np.zeros((F, J * R), dtype=np.uint8)
    snr_no = np.zeros((F, R))
    positions = np.zeros((F + 1, 2 * R + 2 * J), dtype=np.float32)
    c0 = np.float64(c0)
    for f in range(F + 1):
        fd = np.float64(f)
        t = tp0 + fd * tvdt
        rp = rp0 + fd * rvdt
        jp = jp0 + fd * jvdt
        positions[f] = np.concatenate([rp.reshape(-1), jp.reshape(-1)]).astype(np.float32)
        if f == F:
            break
        dx, dy = rp[:, 0] - t[0], rp[:, 1] - t[1]
        d = np.sqrt(dx * dx + dy * dy)
        sd = np.where(d > 1e-6, d, 1e-6)
        d4 = (sd * sd) * (sd * sd)
        den = ((c0 * d4) * rloss) * rlatm
        with np.errstate(divide="ignore", invalid="ignore"):
            Ps = np.where(den <= 1e-18, 0.0, num / den)
            GaPs = Ga * Ps
            q = np.where(Pn > 1e-18, GaPs / Pn, 0.0)
        s_no = np.where(0.0 > q, 0.0, q)
        dxj, dyj = jp[:, None, 0] - rp[None, :, 0], jp[:, None, 1] - rp[None, :, 1]
        dj = np.sqrt(dxj * dxj + dyj * dyj)
        d2 = dj * dj
        big = d2 > 1e-9
        dsq = np.where(big, d2, 1e-9)
        denom = ((dsq * jloss[:, None]) * jlatm[:, None]) * bj[:, None]
        live = dj > 1e-6
        denom = np.where(live, denom, -1.0)
        fl = (live & ~big & (np.asarray(weak)[:, None] != 0)).astype(np.uint8)
        frames[f] = np.concatenate([GaPs, Pn, D, model_pd(s_no, consts), rd_pen, gr, pmin, pmax, gj, denom.reshape(-1)])
        flags[f] = fl.reshape(-1)
        snr_no[f] = s_no
    return {"frames": frames, "flags": flags, "snr_no": snr_no, "positions": positions}


# ---- the shared case table ------------------------------------------------------------------------------------------------
def _edge_dicts(J, R):
    """The four hand-made envs of a size: all velocities zero; only the target moves; a jammer whose position equals a
    radar's bit for bit at frame 2 (denominator -1.0 there); a jammer 2e-5 m from a radar (d^2 <= 1e-9: the weak flag)."""
    base = cases.moving_ring_dict(J, R)
    out = []
    z = copy.deepcopy(base)
    z["environment_params"]["motion"] = dict(step_seconds=0.5)
    out.append(z)
    t = copy.deepcopy(base)
    t["environment_params"]["motion"] = dict(step_seconds=0.5, target_velocity=[30.0, -4.0])
    out.append(t)
    # jammer 0 starts 2 * (v dt) short of radar 0 with power-of-two offsets: p0 + 2.0 * (v dt) is exact, equal bit for bit
    c = copy.deepcopy(base)
    r0 = c["radars"][0]["position"]
    c["radars"][0]["position"] = [400.0, 0.0]
    c["jammers"][0]["position"] = [400.0 - 1.0, 0.0 - 0.5]
    mo = c["environment_params"]["motion"]
    mo["radar_velocity"][0] = [0.0, 0.0]
    mo["jammer_velocity"][0] = [1.0, 0.5]     # dt = 0.5: v dt = (0.5, 0.25); two steps = (1.0, 0.5)
    out.append(c)
    w = copy.deepcopy(base)
    r1 = w["radars"][1]["position"]
    w["jammers"][1]["position"] = [r1[0] + 2e-5, r1[1]]
    w["environment_params"]["motion"]["jammer_velocity"][1] = [0.0, 0.0]
    w["environment_params"]["motion"]["radar_velocity"][1] = [0.0, 0.0]
    out.append(w)
    del r0
    return out


@functools.lru_cache(maxsize=None)
def _case(J, R, E, limit):
    base = cases.moving_ring_dict(J, R)
    dicts = _edge_dicts(J, R)
    e = 0
    while len(dicts) < E:   # the moving ring with per-env jitter (positions, powers, threat levels and velocities)
        rng = np.random.default_rng([4242, e])
        dicts.append(randomized_moving_scenario_dict(base, rng, velocity_jitter=2.0, position_jitter=20.0))
        e += 1
    dicts = dicts[:E]
    scs = [Scenario.from_dict(d, config=config(limit)) for d in dicts]
    return dicts, scs


def case(J, R, E=19, limit=F_PE):
    """(sim-config dicts, their compiled moving Scenarios) of the E-env case of a size: the four edge envs first, then
    jittered moving rings.  Compiled once and shared."""
    dicts, scs = _case(J, R, E, limit)
    return dicts, scs


def model_tables(scs):
    """The model's tables of a list of moving scenarios, stacked per env like MovingScenarioBatch's host arrays."""
    outs = []
    for sc in scs:
        ins = sc.motion_compile_inputs()
        outs.append(compile_model(ins["column"], ins["weak"], sc.num_radars, sc.num_jammers, sc.episode_limit, sc.pd_consts))
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def row_slices(R, J):
    """Named row blocks of a frame column."""
    names = ("GaPs", "Pn", "D", "pd_no", "rd_pen", "gr")
    s = {n: slice(i * R, (i + 1) * R) for i, n in enumerate(names)}
    s.update(pmin=slice(6 * R, 6 * R + J), pmax=slice(6 * R + J, 6 * R + 2 * J), gj=slice(6 * R + 2 * J, 6 * R + 3 * J),
             denom=slice(6 * R + 3 * J, 6 * R + 3 * J + J * R))
    return s


__all__ = ["F_PE", "MovingScenarioBatch", "case", "compile_model", "config", "json", "model_pd", "model_tables",
           "motion_frame_dict", "pe_rows", "row_slices"]
