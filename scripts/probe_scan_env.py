"""Lane-kernel env step with and without scanning beams (environment_params.radar_scan), timed with HIP events.

For each size (3j/4r, 12j/16r ring scenarios; E = 4096 and 2^20) both environments take the one-lane-per-env kernel
(the scanning path's only kernel) in its production configuration (Philox uniforms, float32 actions, no info outputs),
`iters` steps are captured as one graph and replayed; the figure is the replay's event-timed milliseconds per step.
The scanning scenario is the same ring with 0.25 s steps, -30 dB side lobes and the shipped 2.0 / 1.8 degree beams.

    python scripts/probe_scan_env.py [--iters 200] [--reps 5]

Prints one JSON line per (size, E) with the median of `reps` replays of each and their ratio.

    python scripts/probe_scan_env.py --pattern [--out profiles/r09_scan_pattern_env_probe.jsonl]

compares two-level scanning with the stepped antenna pattern (radar_scan.pattern) instead: the shipped
config/scenario_3j4r_scan_pattern.yaml with and without its pattern block (same beams), 3j/4r at E = 4096 and 2^20, default
kernel choice, one process per run, the two alternating three times; every run appends one JSON line to --out.

    python scripts/probe_scan_env.py --eager static|scan|pattern [--E 4096] [--iters 2000] [--reps 5] [--label L] [--out FILE]

times the host side of the launch path instead: `iters` eager env.step calls (no graph) on that scenario, wall clock per
call up to the last call's return (enqueue) and up to the device's completion (total), median of `reps` repetitions.

    python scripts/probe_scan_env.py --per-env [--sizes 3x4,12x16] [--Es 4096,1048576] [--out FILE]

compares scanning on per-env scenario batches (macjd_env_step_scan_pe) with its two neighbours: shared-table scanning
(`scan_shared`), per-env static tables (`pe_static`) and per-env scanning (`pe_scan`; 25 randomised ring scenarios with a
45 degree azimuth jitter, tiled to E), production configuration, graph-replayed steps timed with HIP events, one process
per run, the three alternating `--alternations` times; every run appends one JSON line to --out.  `--tags pe_scan,pe_pattern`
alternates other variants of that list: `pe_pattern` is `pe_scan` under the stepped pattern {1.5, [-3, -12, -17, -25]}
(macjd_env_step_scan_pe_pattern; the same 25 geometries, the level tables per env)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import macjd_amd  # noqa: E402,F401
from macjd_amd import _native  # noqa: E402
from macjd_amd.scenario import Scenario, ScenarioBatch, ring_scenario_dict  # noqa: E402
from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment  # noqa: E402


def timed(env, T, P, iters, reps):
    out_r = torch.zeros(env.batch_envs, device="cuda")
    out_t = torch.zeros(env.batch_envs, dtype=torch.uint8, device="cuda")
    env.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):   # warm-up (and the lazy library options) outside the capture
            env.step(T, P, out_reward=out_r, out_terminated=out_t, want_info=False)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            env.step(T, P, out_reward=out_r, out_terminated=out_t, want_info=False)
    g.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    del g
    return statistics.median(ms)


PATTERN_OUT = os.path.join(REPO, "profiles", "r09_scan_pattern_env_probe.jsonl")


def pattern_env(tag, E):
    """The shipped pattern scenario as it is (pattern), without its pattern block (scan) or without scanning (static)."""
    import yaml
    path = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd", "config", "scenario_3j4r_scan_pattern.yaml")
    d = yaml.safe_load(open(path))
    if tag == "scan":
        del d["environment_params"]["radar_scan"]["pattern"]
    elif tag == "static":
        del d["environment_params"]["radar_scan"]
    sc = Scenario.from_dict(d)
    J, R = sc.num_jammers, sc.num_radars
    rng = np.random.default_rng(0)
    T = torch.from_numpy(rng.integers(0, 2 * R + 1, size=(J, E)).astype(np.int32)).cuda().t()   # agent-major
    P = torch.from_numpy(rng.random((J, E), dtype=np.float32)).cuda().t()
    return sc, T, P, BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device="cuda", seed=1)


def emit(line, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


def eager_run(tag, E, iters, reps, out, label):
    """Host cost of the launch path: eager env.step calls in this process."""
    sc, T, P, env = pattern_env(tag, E)
    out_r = torch.zeros(E, device="cuda")
    out_t = torch.zeros(E, dtype=torch.uint8, device="cuda")
    env.reset()
    enq, tot = [], []
    for rep in range(reps + 1):   # (the first repetition warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            env.step(T, P, out_reward=out_r, out_terminated=out_t, want_info=False)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            enq.append((t1 - t0) / iters * 1e6)
            tot.append((t2 - t0) / iters * 1e6)
    env.close()
    emit({"probe": "scan_env_eager", "variant": tag, "label": label,
          "E": E, "iters": iters, "reps": reps, "us_per_call_enqueue_median": round(statistics.median(enq), 3),
          "us_per_call_total_median": round(statistics.median(tot), 3), "us_per_call_total_all": [round(x, 3) for x in tot],
          "device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}, out)


def pattern_run(tag, E, iters, reps, out):
    """One (two-level | pattern, E) measurement in this process."""
    sc, T, P, env = pattern_env(tag, E)
    J, R = sc.num_jammers, sc.num_radars
    n = iters if E < (1 << 20) else max(20, iters // 10)
    ms = timed(env, T, P, n, reps)
    line = {"probe": "scan_pattern_env", "variant": tag, "levels": sc.scan_pattern_levels, "J": J, "R": R, "E": E, "iters": n,
            "reps": reps, "ms_per_step_median": round(ms, 6), "device": torch.cuda.get_device_name(0),
            "time": time.strftime("%Y-%m-%dT%H:%M:%S")}
    env.close()
    emit(line, out)


PER_ENV_TAGS = ("scan_shared", "pe_static", "pe_scan")
PER_ENV_ALL_TAGS = PER_ENV_TAGS + ("pe_pattern",)


def per_env_run(tag, J, R, E, iters, reps, out):
    """One (scan_shared | pe_static | pe_scan | pe_pattern, size, E) measurement in this process."""
    d = ring_scenario_dict(J, R)
    if tag != "pe_static":
        d["environment_params"] = dict(d["environment_params"], radar_scan={"step_seconds": 0.25, "sidelobe_db": -30.0})
    if tag == "pe_pattern":
        d["environment_params"]["radar_scan"]["pattern"] = {"level_width": 1.5, "gain_db": [-3, -12, -17, -25]}
    if tag == "scan_shared":
        env = BatchedElectromagneticEnvironment(scenario=Scenario.from_dict(d), batch_envs=E, device="cuda", seed=1)
    else:
        jitter = {"azimuth_jitter": 45.0} if tag != "pe_static" else {}
        batch = ScenarioBatch.randomized(d, 25, seed=9, **jitter).tile(E)
        env = BatchedElectromagneticEnvironment(scenario_batch=batch, device="cuda", seed=1)
        del batch
    rng = np.random.default_rng(0)
    T = torch.from_numpy(rng.integers(0, 2 * R + 1, size=(J, E)).astype(np.int32)).cuda().t()   # agent-major
    P = torch.from_numpy(rng.random((J, E), dtype=np.float32)).cuda().t()
    n = iters if E < (1 << 20) else max(20, iters // 10)
    ms = timed(env, T, P, n, reps)
    env.close()
    emit({"probe": "scan_pe_env", "variant": tag, "J": J, "R": R, "E": E, "iters": n, "reps": reps,
          "us_per_step_median": round(ms * 1e3, 3), "device": torch.cuda.get_device_name(0),
          "time": time.strftime("%Y-%m-%dT%H:%M:%S")}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None, help="default 200 (--eager: 2000)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pattern", action="store_true", help="two-level scanning vs the stepped pattern, one process per run")
    ap.add_argument("--one", nargs=2, metavar=("VARIANT", "E"), help="(internal) one run of --pattern in this process")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--eager", choices=["static", "scan", "pattern"], help="host cost of eager env.step calls on that scenario")
    ap.add_argument("--E", type=int, default=4096, help="batch size of --eager")
    ap.add_argument("--label", default="", help="copied into the line of --eager (A/B runs: MACJD_LIB names the library)")
    ap.add_argument("--per-env", action="store_true", help="shared-table scanning vs per-env static vs per-env scanning")
    ap.add_argument("--sizes", default="3x4,12x16", help="JxR sizes of --per-env")
    ap.add_argument("--Es", default="4096,1048576", help="batch sizes of --per-env")
    ap.add_argument("--tags", default=",".join(PER_ENV_TAGS), help=f"variants of --per-env, of {','.join(PER_ENV_ALL_TAGS)}")
    ap.add_argument("--one-per-env", nargs=4, metavar=("VARIANT", "J", "R", "E"), help="(internal) one run of --per-env")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.iters = a.iters or (2000 if a.eager else 200)
    if a.eager:
        return eager_run(a.eager, a.E, a.iters, a.reps, a.out, a.label)
    if a.one_per_env:
        tag, J, R, E = a.one_per_env
        return per_env_run(tag, int(J), int(R), int(E), a.iters, a.reps, a.out)
    if a.per_env:
        tags = a.tags.split(",")
        if not set(tags) <= set(PER_ENV_ALL_TAGS):
            ap.error(f"--tags: unknown variant in {tags}")
        for size in a.sizes.split(","):
            J, R = size.split("x")
            for E in a.Es.split(","):
                for _ in range(a.alternations):
                    for tag in tags:   # a failing run ends the sequence: nothing more is started on the device
                        subprocess.run([sys.executable, os.path.abspath(__file__), "--one-per-env", tag, J, R, E, "--iters",
                                        str(a.iters), "--reps", str(a.reps)] + (["--out", a.out] if a.out else []),
                                       check=True, timeout=600)
        return
    a.out = a.out or PATTERN_OUT
    if a.one:
        return pattern_run(a.one[0], int(a.one[1]), a.iters, a.reps, a.out)
    if a.pattern:
        for E in (4096, 1 << 20):
            for _ in range(a.alternations):
                for tag in ("scan", "pattern"):   # a failing run ends the sequence: nothing more is started on the device
                    subprocess.run([sys.executable, os.path.abspath(__file__), "--one", tag, str(E), "--iters", str(a.iters),
                                    "--reps", str(a.reps), "--out", a.out], check=True, timeout=300)
        return
    for J, R in ((3, 4), (12, 16)):
        d0 = ring_scenario_dict(J, R)
        ds = dict(d0)
        ds["environment_params"] = dict(d0["environment_params"], radar_scan={"step_seconds": 0.25, "sidelobe_db": -30.0})
        sc0, scs = Scenario.from_dict(d0), Scenario.from_dict(ds)
        for E in (4096, 1 << 20):
            rng = np.random.default_rng(0)
            T = torch.from_numpy(rng.integers(0, 2 * R + 1, size=(J, E)).astype(np.int32)).cuda().t()   # agent-major
            P = torch.from_numpy(rng.random((J, E), dtype=np.float32)).cuda().t()
            res = {}
            for tag, sc in (("static", sc0), ("scan", scs)):
                env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device="cuda", seed=1)
                env.kernel_flags = _native.STEP_LANE_KERNEL
                res[tag] = timed(env, T, P, a.iters if E < (1 << 20) else max(20, a.iters // 10), a.reps)
                env.close()
                del env
                torch.cuda.empty_cache()
            print(json.dumps({"J": J, "R": R, "E": E, "static_ms": round(res["static"], 5), "scan_ms": round(res["scan"], 5),
                              "ratio": round(res["scan"] / res["static"], 3)}), flush=True)


if __name__ == "__main__":
    main()
