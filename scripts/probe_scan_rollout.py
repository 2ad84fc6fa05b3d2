"""Time one episode batch of the scanning 3j/4r scenario (E = 4096, T = 100), graph-replayed, with HIP events:

    step    the step-by-step rollout (BatchedEpisodeRunner.step x T captured as one graph)
    closed  the closed-loop launch (agent and env in one kernel, MACJD_CLOSED_LOOP_ROLLOUT)

    python scripts/probe_scan_rollout.py                 # alternates step / closed three times, one process per run
    python scripts/probe_scan_rollout.py --mode closed   # one run in this process
    python scripts/probe_scan_rollout.py --compare-pattern   # closed-loop launch: two-level scanning / stepped antenna
                                                             # pattern (config/scenario_3j4r_scan_pattern.yaml without and
                                                             # with its pattern block), alternating, one process per run;
                                                             # lines go to profiles/r09_scan_pattern_rollout_probe.jsonl
    python scripts/probe_scan_rollout.py --per-env       # the same alternation on a per-env scanning scenario batch
                                                         # (ScenarioBatch.randomized on the shipped scanning base, azimuth
                                                         # jitter 30 degrees), then again on the pattern config; lines go to
                                                         # profiles/r18_scan_pe_rollout_probe.jsonl

Every run appends one JSON line to profiles/r07_scan_rollout_probe.jsonl: ms per episode batch as the mean over
``--reps`` replays after ``--warmup`` replays, and the fastest / slowest single replay.  No profiler is attached."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "r07_scan_rollout_probe.jsonl")
PATTERN_OUT = os.path.join(REPO, "profiles", "r09_scan_pattern_rollout_probe.jsonl")
PE_OUT = os.path.join(REPO, "profiles", "r18_scan_pe_rollout_probe.jsonl")


def one_run(mode, E, reps, warmup, out, scenario="shipped", per_env=False):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import macjd_amd  # noqa: F401
    from macjd_amd.scenario import Scenario
    from test_scan_gpu import PKG, _runner
    if per_env:   # every env its own variation of the shipped scanning scenario ("shipped") or of the pattern config
        import yaml
        from macjd_amd.scenario import ScenarioBatch
        from test_scan_pe_gpu import _runner as pe_runner
        name = "scenario_3j4r_scan.yaml" if scenario == "shipped" else "scenario_3j4r_scan_pattern.yaml"
        batch = ScenarioBatch.randomized(yaml.safe_load(open(os.path.join(PKG, "config", name))), E, seed=0, azimuth_jitter=30.0)
        sc = batch.base
        r, _, _ = pe_runner(batch)
        r.closed_loop_rollout = mode == "closed"
        assert r.closed_loop_pe_available() and not r.closed_loop_available() and not r.fused_rollout_available()
    elif scenario == "shipped":
        sc = Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_scan.yaml"))
    else:   # "pattern" / "two_level": the pattern scenario with / without its pattern block (same beams)
        import yaml
        d = yaml.safe_load(open(os.path.join(PKG, "config", "scenario_3j4r_scan_pattern.yaml")))
        if scenario == "two_level":
            del d["environment_params"]["radar_scan"]["pattern"]
        sc = Scenario.from_dict(d)
    if not per_env:
        r, _, _ = _runner(sc, E)
        r.closed_loop_rollout = mode == "closed"
        assert r.closed_loop_available() and not r.fused_rollout_available()
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
    ms = [a.elapsed_time(b) for a, b in ev]
    line = {"probe": "scan_pe_rollout" if per_env else "scan_rollout", "mode": mode, "scenario": scenario, "levels": sc.scan_pattern_levels, "E": E, "T": sc.episode_limit, "reps": reps, "warmup": warmup,
            "ms_per_batch_mean": sum(ms) / len(ms), "ms_per_batch_min": min(ms), "ms_per_batch_max": max(ms),
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
    ap.add_argument("--out")
    ap.add_argument("--scenario", choices=["shipped", "two_level", "pattern"], default="shipped")
    ap.add_argument("--compare-pattern", action="store_true")
    ap.add_argument("--per-env", action="store_true")
    a = ap.parse_args()
    a.out = a.out or (PE_OUT if a.per_env else PATTERN_OUT if a.compare_pattern or a.scenario != "shipped" else OUT)
    if a.mode:
        return one_run(a.mode, a.envs, a.reps, a.warmup, a.out, a.scenario, a.per_env)
    if a.per_env:
        for scenario in ("shipped", "pattern"):
            for _ in range(a.alternations):
                for mode in ("step", "closed"):     # a failing run ends the sequence: nothing more is started on the device
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--per-env", "--mode", mode, "--scenario", scenario,
                                    "--envs", str(a.envs), "--reps", str(a.reps), "--warmup", str(a.warmup), "--out", a.out],
                                   check=True, timeout=300)
        return
    if a.compare_pattern:
        for _ in range(a.alternations):
            for scenario in ("two_level", "pattern"):   # a failing run ends the sequence
                subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "closed", "--scenario", scenario, "--envs",
                                str(a.envs), "--reps", str(a.reps), "--warmup", str(a.warmup), "--out", a.out], check=True, timeout=300)
        return
    for _ in range(a.alternations):
        for mode in ("step", "closed"):     # a failing run ends the sequence: nothing more is started on the device
            subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(a.envs), "--reps", str(a.reps),
                            "--warmup", str(a.warmup), "--out", a.out], check=True, timeout=300)


if __name__ == "__main__":
    main()
