"""Inputs shared by tests/test_scan_pe_pattern_cpu.py and tests/test_scan_pe_pattern_gpu.py: per-env scanning scenario batches
under a stepped antenna pattern.  The construction is tests/scan_pe_cases.py's (``ring_scenario_dict`` + ``radar_scan {0.25,
-30}``, ``randomized_scenario_dict`` with its default jitters and an N(0, 45 degrees) azimuth jitter, keyed like
``ScenarioBatch.randomized``; env 1 sweeps a whole turn per step, env 2 has jammer 0 sitting on radar 0) plus the pattern
``{level_width: 1.5, gain_db: [-3, -12, -17, -25]}`` and the per-radar ``t_s`` / ``theta_m`` cycle of
tests/test_scan_pattern_cpu.py::pattern_dict, so that ``inv_width`` differs per radar.  The seeds below are the ones both
files use: the CPU file checks that the reference model (tests/scan_pattern_model.py) meets every level on both paths,
both FSM states and a deception draw on exactly the inputs the GPU file compares."""
import copy

import numpy as np

import scan_pe_cases as plain
from _harness import random_actions

from macjd_amd.scenario import Scenario, ScenarioBatch, randomized_scenario_dict, ring_scenario_dict

T_S = [7.3, 6.1, 9.7, 11.9]
THETA_M = [4, 3, 6, 5]
GAINS = {1: [-7.5], 4: [-3, -12, -17, -25], 6: [-3, -8, -12, -17, -21, -25]}
LEVEL_WIDTH = 1.5
AZIMUTH_JITTER = plain.AZIMUTH_JITTER
FULL_ENV, ON_RADAR_ENV = plain.FULL_ENV, plain.ON_RADAR_ENV
# test 1 (batch == single envs): size, envs, steps, scenario seed, env offset, env seed, action seed, masked reset step
SINGLES = dict(J=3, R=4, L=4, E=40, steps=30, seed=5, env_offset=100, env_seed=11, action_seed=21, reset_at=17)
# test 2 (against the model): envs, steps; (J, R, L) -> (scenario seed, action seed)
MODEL = dict(E=33, steps=12)
MODEL_CASES = [(3, 4, 4), (2, 2, 4), (6, 8, 4), (12, 16, 4), (5, 7, 4), (3, 4, 1), (3, 4, 6)]
MODEL_SEEDS = {c: (9, 31) for c in MODEL_CASES}


def pattern_base(J, R, L=4, gain_db=None, sidelobe_db=None, pattern=True):
    """The ring base with scanning beams, the t_s / theta_m cycle and (``pattern``) the pattern block."""
    d = ring_scenario_dict(J, R)
    rs = dict(plain.RADAR_SCAN)
    if sidelobe_db is not None:
        rs["sidelobe_db"] = float(sidelobe_db)
    if pattern:
        rs["pattern"] = {"level_width": LEVEL_WIDTH, "gain_db": list(GAINS[L] if gain_db is None else gain_db)}
    d["environment_params"]["radar_scan"] = rs
    for i, r in enumerate(d["radars"]):
        r["t_s"], r["theta_m"] = T_S[i % 4], THETA_M[i % 4]
    return d


def scenario_dicts(J, R, E, seed, env_offset=0, **base_kw):
    base = pattern_base(J, R, **base_kw)
    out = []
    for e in range(E):
        rng = np.random.default_rng([int(seed), int(env_offset) + e])
        d = randomized_scenario_dict(base, rng, azimuth_jitter=AZIMUTH_JITTER)
        if e == FULL_ENV:
            for r in d["radars"]:
                r["t_s"] = 0.25          # sweep = 360 degrees per step
        if e == ON_RADAR_ENV:
            d["jammers"][0]["position"] = list(copy.deepcopy(d["radars"][0]["position"]))
        out.append(d)
    return out


def scenarios(J, R, E, seed, env_offset=0, **base_kw):
    return [Scenario.from_dict(d, source=f"<scan_pe_pattern {seed}:{env_offset + e}>")
            for e, d in enumerate(scenario_dicts(J, R, E, seed, env_offset, **base_kw))]


def batch(J, R, E, seed, env_offset=0, **base_kw):
    scs = scenarios(J, R, E, seed, env_offset, **base_kw)
    return scs, ScenarioBatch(scs, scan=True, pattern=True)


def model_scenarios(J, R, L):
    return scenarios(J, R, MODEL["E"], MODEL_SEEDS[(J, R, L)][0], L=L)


def model_actions(J, R, L):
    """The actions and uniforms of test 2, step by step: (T int32 [E, J], P float64 [E, J], u float64 [E, R + J])."""
    rng = np.random.default_rng(MODEL_SEEDS[(J, R, L)][1] + 100 * J + R)
    for _ in range(MODEL["steps"]):
        T, P = random_actions(rng, MODEL["E"], J, R)
        yield T, P.astype(np.float64), rng.random((MODEL["E"], R + J))


def singles_actions():
    """The actions of test 1, step by step: out-of-range T (random_actions), P also below 0, above 1 and NaN."""
    c = SINGLES
    rng = np.random.default_rng(c["action_seed"])
    for _ in range(c["steps"]):
        T, P = random_actions(rng, c["E"], c["J"], c["R"])
        P = (P * 1.5 - 0.25).astype(np.float32)                 # [-0.25, 1.25): clipped by the step
        P[rng.random(P.shape) < 0.02] = np.float32("nan")       # NaN propagates into r_p and the reward
        yield T, P
