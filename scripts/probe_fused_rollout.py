#!/usr/bin/env python3
"""Times the pieces of the fused episode rollout at the benchmark's size (E = 4096, 3j/4r, H = 64, T = 100): the
agent-episode launch, the many-step env launch, the replay store, and the whole runner.run().

    python scripts/probe_fused_rollout.py [E] [--jammers J --radars R --hidden H]
    python scripts/probe_fused_rollout.py [E] ... --graph fused|step [--out FILE]

``--graph`` times ONE graph-replayed episode batch instead (HIP events around single replays, no profiler): ``fused`` the
whole-episode launches, ``step`` the step-by-step rollout (``fused_rollout = False``; also what a library without the
episode kernel at this size runs, e.g. another build selected with MACJD_LIB), and prints one JSON line (appended to
``--out``)."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as entry

if not os.environ.get("MACJD_LIB"):
    entry.build()
from macjd_amd import bench_rollout, ops
from macjd_amd.core.mac import BasicMAC
from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
from macjd_amd.scenario import Scenario, ring_scenario_dict
from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer

ap = argparse.ArgumentParser()
ap.add_argument("envs", nargs="?", type=int, default=4096)
ap.add_argument("--jammers", type=int, default=3)
ap.add_argument("--radars", type=int, default=4)
ap.add_argument("--hidden", type=int, default=64)
ap.add_argument("--graph", choices=["fused", "step"])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out")
cli = ap.parse_args()

dev = torch.device("cuda", 0)
E, H = cli.envs, cli.hidden
sc = Scenario.from_dict(ring_scenario_dict(cli.jammers, cli.radars))
args = bench_rollout.make_args(sc, H, dev, batch_envs=E)
env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=dev, seed=42)
with contextlib.redirect_stdout(io.StringIO()):
    mac = BasicMAC(args.obs_shape, args)
    mac.cuda()
    buf = EpisodeReplayBuffer(args, device=dev)
runner = BatchedEpisodeRunner(env, mac, buf, args)
if cli.graph:
    runner.fused_rollout = cli.graph == "fused"
    assert runner.fused_rollout_available() == (cli.graph == "fused")
    runner.enable_graph()
    for _ in range(cli.warmup):
        runner.rollout_graphed()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(cli.reps)]
    for e0, e1 in ev:
        e0.record()
        runner.rollout_graphed()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    line = {"probe": "fused_rollout", "mode": cli.graph, "jammers": cli.jammers, "radars": cli.radars, "H": H, "E": E,
            "T": runner.episode_limit, "reps": cli.reps, "warmup": cli.warmup, "lib": os.path.basename(os.environ.get("MACJD_LIB", "")),
            "ms_per_batch_mean": sum(ms) / len(ms), "ms_per_batch_min": min(ms), "ms_per_batch_max": max(ms),
            "device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}
    runner.release_graphs()
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
    sys.exit(0)
assert runner.fused_rollout_available()


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


runner.rollout_fused()
st, T, J = runner.stage, runner.episode_limit, runner.n_agents
a = mac.agent
l1, l2 = a.fc2_q_head[0], a.fc2_q_head[2]
params, gi = mac.static_inputs
us_agent = timed(lambda: ops.agent_episode(gi, params, None, a.rnn.weight_hh, a.rnn.bias_hh, l1.weight, l1.bias, l2.weight,
                                           l2.bias, E, J, T, runner._avail, runner._eps_sched, False, 1, runner._ctr_base,
                                           st["hidden_state"], st["actions_discrete"], st["actions_continuous"],
                                           h_final=mac.hidden_states))
us_env = timed(lambda: env.step_many(st["actions_discrete"], st["actions_continuous"], st["reward"], st["terminated"],
                                     runner._rdpj_steps, rdpj_sum=runner._rdpj_sum))
us_store = timed(lambda: runner.end_episodes())
us_roll = timed(lambda: runner.rollout_fused())
us_run = timed(lambda: runner.run(sync_stats=False))
flops = 2.0 * E * J * T * (H * 3 * H + H * H)
print(f"E={E} {cli.jammers}j/{cli.radars}r H={H}: agent_episode {us_agent:8.1f} us ({us_agent / T:5.2f} us/step, {flops / us_agent / 1e6:6.2f} TFLOP/s in the two products)"
      f"   env.step_many {us_env:7.1f} us   replay store {us_store:7.1f} us   rollout_fused {us_roll:8.1f} us   run() {us_run:8.1f} us")
