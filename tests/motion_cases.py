"""Shared pieces of tests/test_motion_cpu.py and tests/test_motion_gpu.py: the moving scenarios, their per-frame static
scenarios (compiled once and cached) and the FRAME ORACLE — the C oracle of the static step run on the frame scenario each
env is in, with track / step counter / episode index carried across frames."""
import copy
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

from _harness import GOLDEN, OracleEnv

from macjd_amd.scenario import Scenario, motion_frame_dict, ring_scenario_dict

F_SHORT = 24   # episode limit of the GPU cases (the fixture's is 100)


def fixture():
    """(sim-config dict with the ``motion`` key, raw npz) of tests/golden/env_3j4r_moving.npz."""
    g = np.load(os.path.join(GOLDEN, "env_3j4r_moving.npz"))
    return json.loads(str(g["scenario_json"])), g


def moving_ring_dict(n_jammers, n_radars):
    """The ring scenario of that size with every kind of entity moving, 0.5 s per step: jammer 0 starts 5 m short of radar 0
    and closes 1 m per step (co-located, negative denominator, in frame 5 only); jammer 1 starts 2e-5 m from radar 1 (weak
    denominator in frame 0 only) and leaves; the other jammers drift; the target runs towards radar 0 at 15 m per step
    (its no-jamming detection probability sweeps most of (0, 1) within 24 frames); the last radar moves."""
    d = ring_scenario_dict(n_jammers, n_radars)
    r0, r1 = d["radars"][0]["position"], d["radars"][1]["position"]
    d["jammers"][0]["position"] = [r0[0] - 5.0, r0[1]]
    d["jammers"][1]["position"] = [r1[0] + 2e-5, r1[1]]
    jv = [[2.0, 0.0], [1.0, -3.0]] + [[0.5 * (j % 3) - 0.5, 0.25 * j] for j in range(2, n_jammers)]
    rv = [[0.0, 0.0] for _ in range(n_radars)]
    rv[-1] = [1.0, 0.5]
    d["environment_params"]["motion"] = dict(step_seconds=0.5, target_velocity=[30.0, 0.0], radar_velocity=rv,
                                             jammer_velocity=jv[:n_jammers])
    return d


def config(limit=F_SHORT):
    return SimpleNamespace(episode_limit=limit)


@functools.lru_cache(maxsize=None)
def _compiled(cfg_json, limit):
    cfg = json.loads(cfg_json)
    conf = None if limit is None else config(limit)
    sc = Scenario.from_dict(cfg, config=conf)
    frames = [Scenario.from_dict(motion_frame_dict(cfg, f), config=conf) for f in range(sc.episode_limit + 1)]
    return sc, frames


def compiled(cfg, limit=F_SHORT):
    """(moving Scenario, [static Scenario of frame 0 .. F]) — compiled once per (config, episode limit)."""
    return _compiled(json.dumps(cfg), limit)


def zero_velocity(cfg):
    """``cfg`` with a motion block whose velocities are all zero."""
    d = copy.deepcopy(cfg)
    d["environment_params"]["motion"] = dict(step_seconds=0.5)
    return d


class FrameOracle:
    """E envs of a moving scenario stepped by the C oracle: env e, whose step counter is k, runs on the static scenario of
    frame min(k, F - 1).  One OracleEnv per frame; a step runs every frame some env is in on the whole batch (so env
    indices, and with them the Philox keys, stay the batch's) and keeps each env's rows from its own frame."""

    def __init__(self, frames, n_envs):
        self.frames = frames[:-1]            # frame F is only ever shown, never stepped on
        self.F = len(self.frames)
        self.E = int(n_envs)
        self.oracles = {}
        R = frames[0].num_radars
        self.track = np.zeros((self.E, R), dtype=np.uint8)
        self.step_count = np.zeros(self.E, dtype=np.int32)
        self.episode = np.zeros(self.E, dtype=np.int32)

    def reset(self, mask=None):
        sel = slice(None) if mask is None else np.asarray(mask, dtype=bool)
        self.track[sel] = 0
        self.step_count[sel] = 0
        self.episode[sel] += 1

    def frame_of(self):
        return np.minimum(self.step_count, self.F - 1)

    def step(self, T, P, u=None, seed=0, env_offset=0, arith_f64=False):
        fe = self.frame_of()
        out = None
        for f in np.unique(fe):
            o = self.oracles.get(int(f))
            if o is None:
                o = self.oracles[int(f)] = OracleEnv(self.frames[int(f)], self.E)
            o.track[:] = self.track
            o.step_count[:] = self.step_count
            o.episode[:] = self.episode
            res = o.step(T, P, u=u, seed=seed, env_offset=env_offset, arith_f64=arith_f64)
            if out is None:
                out = {k: np.array(v, copy=True) for k, v in res.items()}
            else:
                sel = fe == f
                for k, v in res.items():
                    out[k][sel] = v[sel]
        self.track[:] = out["track"]
        self.step_count[:] = out["step"]
        return out
