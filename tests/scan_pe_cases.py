"""Inputs shared by tests/test_scan_pe_cpu.py and tests/test_scan_pe_gpu.py: per-env scanning scenario batches built from
``ring_scenario_dict`` + ``radar_scan {0.25, -30}``, ``randomized_scenario_dict`` with its default jitters and an N(0, 45
degrees) azimuth jitter, keyed like ``ScenarioBatch.randomized`` (env e = variation ``env_offset + e`` of ``seed``'s stream).
Env 1 sweeps a whole turn per step (``full`` for every radar), env 2 has jammer 0 sitting on radar 0 (denom = -1: its
actions on that radar are ignored).  The seeds below are the ones both files use: the CPU file checks that the reference
model (tests/scan_model.py) meets every lobe path on exactly the inputs the GPU file compares."""
import copy

import numpy as np

from _harness import random_actions

from macjd_amd.scenario import Scenario, ScenarioBatch, randomized_scenario_dict, ring_scenario_dict

RADAR_SCAN = {"step_seconds": 0.25, "sidelobe_db": -30.0}
AZIMUTH_JITTER = 45.0
FULL_ENV, ON_RADAR_ENV = 1, 2
# test 1 (batch == single envs): size, envs, steps, scenario seed, env offset, env seed, action seed, masked reset step
SINGLES = dict(J=3, R=4, E=40, steps=30, seed=5, env_offset=100, env_seed=11, action_seed=21, reset_at=17)
# test 2 (against the model): envs, steps, scenario seed, action seed
MODEL = dict(E=33, steps=12, seed=9, action_seed=31)
MODEL_SIZES = [(3, 4), (2, 2), (6, 8), (12, 16), (5, 7)]


def scan_base(J, R):
    d = ring_scenario_dict(J, R)
    d["environment_params"]["radar_scan"] = dict(RADAR_SCAN)
    return d


def scenario_dicts(J, R, E, seed, env_offset=0):
    base = scan_base(J, R)
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


def scenarios(J, R, E, seed, env_offset=0):
    return [Scenario.from_dict(d, source=f"<scan_pe {seed}:{env_offset + e}>")
            for e, d in enumerate(scenario_dicts(J, R, E, seed, env_offset))]


def batch(J, R, E, seed, env_offset=0):
    scs = scenarios(J, R, E, seed, env_offset)
    return scs, ScenarioBatch(scs, scan=True)


def model_actions(J, R):
    """The actions and uniforms of test 2, step by step: (T int32 [E, J], P float64 [E, J], u float64 [E, R + J])."""
    rng = np.random.default_rng(MODEL["action_seed"] + 100 * J + R)
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
