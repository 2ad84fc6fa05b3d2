"""Time one episode batch of the moving 3j/4r scenario under scanning radars with a four-level pattern
(config/scenario_3j4r_moving_scan.yaml, E = 4096, T = 100), graph-replayed, with HIP events on the replay stream:

    step    the step-by-step rollout (BatchedEpisodeRunner.step x T captured as one graph)
    closed  the closed-loop episode launch on the frame tables (MACJD_CLOSED_LOOP_MOVING_ROLLOUT)

    python scripts/probe_moving_scan_rollout.py                 # alternates step / closed three times, one process per run
    python scripts/probe_moving_scan_rollout.py --mode closed   # one run in this process

Every run appends one JSON line to profiles/moving_scan_rollout_probe.jsonl: microseconds per episode batch as the mean over
``--reps`` replays after ``--warmup`` replays, and the fastest / slowest single replay.  No profiler is attached."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "moving_scan_rollout_probe.jsonl")


def one_run(mode, E, reps, warmup, out):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import macjd_amd  # noqa: F401
    from macjd_amd.scenario import Scenario
    from test_moving_scan_gpu import PKG, _runner
    sc = Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_moving_scan.yaml"))
    r, _, _ = _runner(sc, E)
    r.closed_loop_moving_rollout = mode == "closed"
    assert r.closed_loop_moving_available() and not r.fused_rollout_available() and not r.moving_rollout_available()
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
    line = {"probe": "moving_scan_rollout", "mode": mode, "E": E, "T": sc.episode_limit, "reps": reps, "warmup": warmup,
            "us_per_batch_mean": sum(us) / len(us), "us_per_batch_min": min(us), "us_per_batch_max": max(us),
            "device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}
    r.release_graphs()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "closed"])
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.mode:
        return one_run(a.mode, a.envs, a.reps, a.warmup, a.out)
    for _ in range(a.alternations):
        for mode in ("step", "closed"):     # a failing run ends the sequence: nothing more is started on the device
            subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(a.envs), "--reps", str(a.reps),
                            "--warmup", str(a.warmup), "--out", a.out], check=True, timeout=300)


if __name__ == "__main__":
    main()
