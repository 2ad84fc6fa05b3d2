"""Inputs shared by tests/test_moving_scan_cpu.py and tests/test_moving_scan_gpu.py: moving scenarios with scanning radars
(``environment_params.motion`` and ``radar_scan`` on one clock).  The construction is ``motion_cases.moving_ring_dict`` (every
kind of entity moves, 0.5 s per step, 24 frames) plus ``radar_scan {step_seconds: 0.5, sidelobe_db: -30}``, the per-radar
``t_s`` / ``theta_m`` cycle of tests/scan_pe_pattern_cases.py and, with ``pattern``, its four-level pattern.  The model run
below is the one the GPU file compares against; the CPU file checks its coverage (both lobes / every level on both paths, a
beam that follows the moved target, uniforms that stay clear of every detection probability)."""
import copy
import functools
import json

import numpy as np

import motion_cases
from _harness import random_actions

from macjd_amd.scenario import Scenario, motion_frame_dict

F = motion_cases.F_SHORT
SIZES = [(2, 2), (3, 4), (6, 8), (3, 3)]   # three compiled sizes and a generic one
CASES = [(J, R, pattern) for (J, R) in SIZES for pattern in (False, True)]
STEP_SECONDS = 0.5
T_S = [7.3, 6.1, 9.7, 11.9]
THETA_M = [4, 3, 6, 5]
PATTERN = {"level_width": 1.5, "gain_db": [-3, -12, -17, -25]}
# the model run: envs, steps (the envs that are never reset pass F: the clamp), the step of the masked reset
MODEL = dict(E=33, steps=F + 4, reset_at=5)


def moving_scan_dict(J, R, pattern=False, step_seconds=STEP_SECONDS):
    d = motion_cases.moving_ring_dict(J, R)
    rs = {"step_seconds": step_seconds, "sidelobe_db": -30.0}
    if pattern:
        rs["pattern"] = copy.deepcopy(PATTERN)
    d["environment_params"]["radar_scan"] = rs
    for i, r in enumerate(d["radars"]):
        r["t_s"], r["theta_m"] = T_S[i % 4], THETA_M[i % 4]
    return d


def zero_velocity(cfg):
    """``cfg`` with a motion block on the same clock whose velocities are all zero."""
    d = copy.deepcopy(cfg)
    d["environment_params"]["motion"] = dict(step_seconds=d["environment_params"]["radar_scan"]["step_seconds"])
    return d


@functools.lru_cache(maxsize=None)
def _compiled(cfg_json, limit):
    cfg = json.loads(cfg_json)
    conf = motion_cases.config(limit)
    sc = Scenario.from_dict(cfg, config=conf)
    frames = [Scenario.from_dict(motion_frame_dict(cfg, f), config=conf) for f in range(sc.episode_limit + 1)]
    return sc, frames


def compiled(cfg, limit=F):
    """(moving scanning Scenario, [static scanning Scenario of frame 0 .. F]) — compiled once per (config, episode limit)."""
    return _compiled(json.dumps(cfg), limit)


def case(J, R, pattern):
    return compiled(moving_scan_dict(J, R, pattern))


def third(E):
    return np.arange(E) % 3 == 0


def model_inputs(J, R):
    """The actions and uniforms of the model run, step by step: (T int32 [E, J], P float64 [E, J], u float64 [E, R + J])."""
    rng = np.random.default_rng(41 + 100 * J + R)
    for _ in range(MODEL["steps"]):
        T, P = random_actions(rng, MODEL["E"], J, R)
        yield T, P.astype(np.float64), rng.random((MODEL["E"], R + J))


@functools.lru_cache(maxsize=None)
def model_run(J, R, pattern):
    """The model's outputs on the model inputs (every third env reset after ``reset_at`` steps, so one batch holds several
    frames), with its coverage record; computed once per case."""
    from moving_scan_model import MovingScanModel
    sc, frames = case(J, R, pattern)
    E = MODEL["E"]
    m = MovingScanModel(frames, E)
    steps = []
    for t, (T, P, u) in enumerate(model_inputs(J, R)):
        if t == MODEL["reset_at"]:
            m.reset(third(E))
        frame = m.frame_of().copy()
        steps.append((T, P, u, frame, m.step(T, P, u)))
    return steps, m
