#!/usr/bin/env python3
"""Generate the golden trace of the MOVING 3j/4r scenario by driving the REFERENCE implementation.

Run (build container only; the reference tree does not exist on the GPU box):

    python tests/golden/make_golden_motion.py

The reference's step() moves no entity, but it recomputes every distance-dependent quantity from ``radar.position``,
``jammer.position`` and ``protected_target_config['position']`` on every call (simulation/environment.py:282-286,313-327).
This script moves those three attributes between its step() calls: before step number k it assigns the positions of
``scenario.motion_frame_dict(cfg, k)`` — THE definition of a frame, shared with the scenario compiler and the tests — and
after the step those of frame k + 1, then records ``env.get_state()`` as ``obs_after``.  So every recorded number is the
reference's own physics on the frame's positions.

The scenario is the package's ``config/scenario_3j4r_moving.yaml``.  The reference's constructor is handed frame 0 (the
same file without the ``motion`` key: its schema has no such key).  Only DATA is written (inputs, the reference's outputs
and ``scenario_json`` including the ``motion`` key); no reference source or bytecode is copied.  Same generator environment
as make_golden.py (Python 3.10, numpy >= 2: the "f32" mode relies on NEP-50 promotion).
"""
import contextlib
import io
import json
import os
import sys
import tempfile
from types import SimpleNamespace

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import macjd_amd
from macjd_amd.scenario import motion_frame_dict
from make_golden import make_actions, reference_cwd   # the scripted actions and the reference import context

CONFIG = os.path.join(os.path.dirname(os.path.abspath(macjd_amd.__file__)), "config", "scenario_3j4r_moving.yaml")
N_STEPS = 100
SEED = 42


def assign_frame(env, cfg, k):
    """Positions of frame k onto the reference's entities (np.array, as its constructors store them)."""
    fr = motion_frame_dict(cfg, k)
    for r, radar in enumerate(env.radars):
        radar.position = np.array(fr["radars"][r]["position"])
    for j, jammer in enumerate(env.jammers):
        jammer.position = np.array(fr["jammers"][j]["position"])
    env.protected_target_config["position"] = np.array(fr["protected_target"]["position"])


def gen(out_dir):
    with open(CONFIG) as f:
        cfg = yaml.safe_load(f)
    with reference_cwd():
        from simulation.environment import ElectromagneticEnvironment
        path = os.path.join(tempfile.mkdtemp(prefix="macjd_golden_motion_"), "frame0.yaml")
        with open(path, "w") as f:
            yaml.safe_dump(motion_frame_dict(cfg, 0), f)
        with contextlib.redirect_stdout(io.StringIO()):
            env = ElectromagneticEnvironment(SimpleNamespace(), path)
        J, R = env.num_jammers, env.num_radars
        info0 = env.get_env_info()
        assert info0["episode_limit"] == N_STEPS
        rec = {"scenario_json": json.dumps(cfg), "env_info_json": json.dumps(info0)}
        for mode in ("f32", "f64"):
            rng = np.random.default_rng(1000 + SEED)
            np.random.seed(SEED)
            drawn = []
            orig_rand = np.random.rand

            def logged_rand(*a):
                v = orig_rand(*a)
                drawn.append(float(v))
                return v
            np.random.rand = logged_rand
            try:
                tr = {k: [] for k in ("T", "P", "u", "n_draws", "reward", "r_d", "r_p", "r_j", "pd", "snr_no", "snr_with",
                                      "track", "terminated", "prj", "obs_after")}
                with contextlib.redirect_stdout(io.StringIO()):
                    env.reset()
                    assign_frame(env, cfg, 0)
                    rec[f"{mode}_s{SEED}_obs_reset"] = np.array(env.get_state())
                    for step in range(N_STEPS):
                        T, P = make_actions(rng, step, J, R)
                        if mode == "f32":
                            P_in = P.astype(np.float32)
                            acts = [(T[i], P_in[i]) for i in range(J)]
                        else:
                            P_in = P.astype(np.float64)
                            acts = [(int(T[i]), float(P_in[i])) for i in range(J)]
                        assign_frame(env, cfg, step)
                        drawn.clear()
                        obs, reward, term, info = env.step(acts)
                        assign_frame(env, cfg, step + 1)
                        u = np.full(R + J, np.nan)
                        u[:len(drawn)] = drawn
                        prj = np.full(J, -1.0)
                        for a in info["jammer_actions"]:
                            prj[a["jammer_idx"]] = a["received_power"]
                        tr["T"].append(T.astype(np.int32)); tr["P"].append(P_in.astype(np.float64))
                        tr["u"].append(u); tr["n_draws"].append(len(drawn))
                        tr["reward"].append(float(reward)); tr["r_d"].append(float(info["r_d"]))
                        tr["r_p"].append(float(info["r_p"])); tr["r_j"].append(float(info["r_j"]))
                        tr["pd"].append(np.array(info["radar_pds"], dtype=np.float64))
                        tr["snr_no"].append(np.array(info["snr_no_jamming"], dtype=np.float64))
                        tr["snr_with"].append(np.array(info["snr_with_jamming"], dtype=np.float64))
                        tr["track"].append(np.array([s["is_tracking"] for s in info["radar_states"]], dtype=np.uint8))
                        tr["terminated"].append(bool(term)); tr["prj"].append(prj)
                        tr["obs_after"].append(np.array(env.get_state()))
            finally:
                np.random.rand = orig_rand
            for k, v in tr.items():
                rec[f"{mode}_s{SEED}_{k}"] = np.array(v)
        np.savez_compressed(os.path.join(out_dir, "env_3j4r_moving.npz"), **rec)
        print(f"env_3j4r_moving.npz  J={J} R={R} S={info0['state_shape']} steps={N_STEPS}")


if __name__ == "__main__":
    gen(HERE)
