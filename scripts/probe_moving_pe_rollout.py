"""Time one episode batch of the moving 3j/4r scenario with PER-ENV trajectories (config/scenario_3j4r_moving.yaml randomized
with velocity_jitter 1.0, frame tables compiled on the device, E = 4096, T = 100), graph-replayed, with HIP events on the
replay stream:

    step       the step-by-step rollout (BatchedEpisodeRunner.step x T captured as one graph; the switch off)
    moving_pe  the whole-episode launches (the agent's steps on every env's own frames, the env's steps:
               MACJD_MOVING_PE_EPISODE_ROLLOUT)

    python scripts/probe_moving_pe_rollout.py                    # alternates step / moving_pe three times, one process per run
    python scripts/probe_moving_pe_rollout.py --mode moving_pe   # one run in this process

Every run appends one JSON line to profiles/moving_pe_rollout_probe.jsonl: microseconds per episode batch as the mean over
``--reps`` replays after ``--warmup`` replays, and the fastest / slowest single replay.  No profiler is attached."""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "moving_pe_rollout_probe.jsonl")


def one_run(mode, E, T, reps, warmup, out):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import yaml
    import macjd_amd  # noqa: F401
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.scenario import MovingScenarioBatch
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    from test_nets_cpu import make_args, quiet
    pkg = os.path.dirname(os.path.abspath(sys.modules["macjd_amd"].__file__))
    with open(os.path.join(pkg, "config", "scenario_3j4r_moving.yaml")) as f:
        base = yaml.safe_load(f)
    mb = MovingScenarioBatch.randomized(base, E, seed=42, config=SimpleNamespace(episode_limit=T), velocity_jitter=1.0,
                                        compile="device")
    env = BatchedElectromagneticEnvironment(moving_batch=mb, device="cuda:0", seed=5)
    info = env.get_env_info()
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=E, epsilon_start=0.3,
                     epsilon_anneal_time=500)
    args.env_info = info
    torch.manual_seed(3)
    with quiet():
        mac = BasicMAC(info["obs_shape"], args)
        mac.cuda()
        buf = EpisodeReplayBuffer(args)
    r = BatchedEpisodeRunner(env, mac, buf, args)
    r.moving_pe_episode_rollout = mode == "moving_pe"
    assert r.moving_pe_rollout_available() and not r.moving_rollout_available() and not r.fused_rollout_available()
    r.enable_graph()
    for _ in range(warmup):
        r.rollout_graphed()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        r.rollout_graphed()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    line = {"probe": "moving_pe_rollout", "mode": mode, "E": E, "T": info["episode_limit"], "reps": reps, "warmup": warmup,
            "us_per_batch_mean": sum(us) / len(us), "us_per_batch_min": min(us), "us_per_batch_max": max(us),
            "table_bytes": env.table_bytes, "device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}
    r.release_graphs()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "moving_pe"])
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.mode:
        return one_run(a.mode, a.envs, a.steps, a.reps, a.warmup, a.out)
    for _ in range(a.alternations):
        for mode in ("step", "moving_pe"):     # a failing run ends the sequence: nothing more is started on the device
            subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(a.envs), "--steps", str(a.steps),
                            "--reps", str(a.reps), "--warmup", str(a.warmup), "--out", a.out], check=True, timeout=300)


if __name__ == "__main__":
    main()
