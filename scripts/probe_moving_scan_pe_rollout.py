"""Time one episode batch of the moving 3j/4r scenario under scanning radars with PER-ENV trajectories and beams
(config/scenario_3j4r_moving_scan.yaml, L = 4, randomized with velocity_jitter 1.0, frame tables compiled on the device,
E = 4096, T = 100), graph-replayed, with HIP events on the replay stream — both forms in ONE process on ONE environment:

    step            the step-by-step rollout (BatchedEpisodeRunner.step x T captured as one graph; the switch off)
    closed_loop_pe  the closed-loop launch on every env's own frame tables (MACJD_CLOSED_LOOP_MOVING_PE_ROLLOUT)

    python scripts/probe_moving_scan_pe_rollout.py
    MACJD_LIB=<another build> python scripts/probe_moving_scan_pe_rollout.py --label prefetch     # kernel A/B runs

Two runners (same agent weights) share the environment; each captures its graph, then ``--blocks`` blocks alternate between
the two, a block being ``--reps`` replays timed one by one.  One JSON line is appended to
profiles/moving_scan_pe_rollout_probe.jsonl: per form, milliseconds per episode batch as the mean over all blocks and the
smallest and largest block mean.  No profiler is attached."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "moving_scan_pe_rollout_probe.jsonl")
MODES = ("step", "closed_loop_pe")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="", help="free text kept in the line (which build of the library)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import yaml
    import macjd_amd  # noqa: F401
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.scenario import MovingScanScenarioBatch
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    from test_nets_cpu import make_args, quiet
    pkg = os.path.dirname(os.path.abspath(sys.modules["macjd_amd"].__file__))
    with open(os.path.join(pkg, "config", "scenario_3j4r_moving_scan.yaml")) as f:
        base = yaml.safe_load(f)
    E, T = a.envs, a.steps
    mb = MovingScanScenarioBatch.randomized(base, E, seed=42, config=SimpleNamespace(episode_limit=T), velocity_jitter=1.0,
                                            compile="device")
    env = BatchedElectromagneticEnvironment(moving_scan_batch=mb, device="cuda:0", seed=5)
    info = env.get_env_info()
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
    runners = {}
    for mode in MODES:
        args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=E, epsilon_start=0.3,
                         epsilon_anneal_time=500)
        args.env_info = info
        torch.manual_seed(3)
        with quiet():
            mac = BasicMAC(info["obs_shape"], args)
            mac.cuda()
            buf = EpisodeReplayBuffer(args)
        r = runners[mode] = BatchedEpisodeRunner(env, mac, buf, args)
        r.closed_loop_moving_pe_rollout = mode == "closed_loop_pe"
        assert r.closed_loop_moving_pe_available() and not r.closed_loop_moving_available() and not r.fused_rollout_available()
        r.enable_graph()
        for _ in range(a.warmup):
            r.rollout_graphed()
    torch.cuda.synchronize()
    blocks = {mode: [] for mode in MODES}
    for _ in range(a.blocks):
        for mode in MODES:
            r = runners[mode]
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for s, e in ev:
                s.record()
                r.rollout_graphed()
                e.record()
            torch.cuda.synchronize()
            blocks[mode].append(sum(s.elapsed_time(e) for s, e in ev) / a.reps)
    line = {"probe": "moving_scan_pe_rollout", "label": a.label, "E": E, "T": info["episode_limit"],
            "L": int(mb.scan_pattern_levels), "blocks": a.blocks, "reps": a.reps, "warmup": a.warmup}
    for mode in MODES:
        b = blocks[mode]
        line[mode] = {"ms_per_batch_mean": sum(b) / len(b), "ms_per_batch_min_block": min(b), "ms_per_batch_max_block": max(b)}
    line["step_over_closed_loop_pe"] = line["step"]["ms_per_batch_mean"] / line["closed_loop_pe"]["ms_per_batch_mean"]
    line.update(table_bytes=env.table_bytes, lib=os.environ.get("MACJD_LIB", ""), device=torch.cuda.get_device_name(0),
                time=time.strftime("%Y-%m-%dT%H:%M:%S"))
    for r in runners.values():
        r.release_graphs()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
