#!/usr/bin/env python3
"""Measurements of the per-env moving scenarios under scanning radars (include/macjd.h, macjd_motion_scan_pe_io):
config/scenario_3j4r_moving_scan.yaml randomised with velocity_jitter 1.0 at E = 4096, F = 100.  HIP events, no profiler, one
fresh process per run; the three step paths alternate three times.

    step_pe_scan  microseconds per launch of macjd_env_step_moving_scan_pe (an episode of F launches replayed from one graph)
    step_shared   ... of the shared-frame moving-scanning step (macjd_env_step_moving_scan) on the base scenario
    step_pe       ... of the per-env moving step (macjd_env_step_moving_pe) on scenario_3j4r_moving.yaml
    step_pe_scan_nopattern   step_pe_scan with the pattern removed from the base (no level rows)
    step_pe_scan_lastframe   step_pe_scan with every counter at F before the episode: all launches read frame F - 1 (warm tables)
    compile       microseconds of the two compiler launches, and table_bytes
    host          seconds of MovingScanScenarioBatch.randomized(compile="host") for 64 envs, scaled linearly to E
    rollout       milliseconds per episode batch of the graph-replayed step-loop rollout

    python scripts/probe_moving_scan_pe.py                  # everything, one process per run
    python scripts/probe_moving_scan_pe.py --mode compile   # one run in this process
Every run appends one JSON line to profiles/moving_scan_pe_probe.jsonl (or --out)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "moving_scan_pe_probe.jsonl")
HOST_ENVS = 64
STEP_MODES = ("step_pe_scan", "step_shared", "step_pe")
SPLIT_MODES = ("step_pe_scan_nopattern", "step_pe_scan_lastframe")   # what the per-env scanning step's time is made of
MODES = STEP_MODES + SPLIT_MODES + ("compile", "host", "rollout")


def _base(name):
    import yaml
    pkg = os.path.dirname(os.path.abspath(sys.modules["macjd_amd"].__file__))
    with open(os.path.join(pkg, "config", name)) as f:
        return yaml.safe_load(f)


def _episode_us(env, T, P, F, dev, last_frame=False):
    """Microseconds per step launch: F steps replayed from one graph after an untimed reset (``last_frame``: and with every
    counter set to F, so that each launch runs the clamped frame F - 1), three runs."""
    import torch
    from macjd_amd import hipgraph
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        env.reset()
        for _ in range(3):
            env.step(T, P, want_info=False)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    env.reset()
    torch.cuda.synchronize(dev)
    with hipgraph.capture(graph):
        for _ in range(F):
            env.step(T, P, want_info=False)
    runs = []
    for _ in range(4):   # the first replay warms up
        env.reset()
        if last_frame:
            env.step_count.fill_(F)
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        hipgraph.replay(graph, dev)
        t1.record()
        t1.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / F)
    hipgraph.destroy([graph], dev)
    return runs[1:]


def one_run(mode, E, F, out):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import macjd_amd  # noqa: F401
    from macjd_amd import _native
    from macjd_amd.scenario import DEG_PER_RAD, FOUR_PI_CUBED, MovingScanScenarioBatch, MovingScenarioBatch, Scenario
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    dev = torch.device("cuda", 0)
    conf = SimpleNamespace(episode_limit=F)
    line = {"probe": "moving_scan_pe", "mode": mode, "E": E, "F": F}
    kw = dict(seed=42, config=conf, velocity_jitter=1.0)
    if mode in STEP_MODES + SPLIT_MODES:
        if mode.startswith("step_pe_scan"):
            base = _base("scenario_3j4r_moving_scan.yaml")
            if mode == "step_pe_scan_nopattern":
                base["environment_params"]["radar_scan"].pop("pattern", None)
            env = Env(moving_scan_batch=MovingScanScenarioBatch.randomized(base, E, compile="device", **kw), device=dev, seed=1)
        elif mode == "step_shared":
            env = Env(scenario=Scenario.from_dict(_base("scenario_3j4r_moving_scan.yaml"), config=conf), batch_envs=E, device=dev,
                      seed=1)
        else:
            env = Env(moving_batch=MovingScenarioBatch.randomized(_base("scenario_3j4r_moving.yaml"), E, compile="device", **kw),
                      device=dev, seed=1)
        J, R = env.num_jammers, env.num_radars
        gen = torch.Generator(device=dev).manual_seed(1)
        T = torch.randint(0, 2 * R + 1, (J, E), generator=gen, device=dev, dtype=torch.int32).t()
        P = torch.rand((J, E), generator=gen, device=dev).t()
        runs = _episode_us(env, T, P, F, dev, last_frame=mode == "step_pe_scan_lastframe")
        line.update(us_per_step_min_med_max=[min(runs), statistics.median(runs), max(runs)])
        env.close()
    elif mode == "compile":
        t0 = time.perf_counter()
        mb = MovingScanScenarioBatch.randomized(_base("scenario_3j4r_moving_scan.yaml"), E, compile="device", **kw)
        t_inputs = time.perf_counter() - t0
        env = Env(moving_scan_batch=mb, device=dev, seed=1)
        keep, sc, w = env._motion_keep, env.scenario, env._pe_tile
        R, J, L = env.num_radars, env.num_jammers, mb.scan_pattern_levels
        lib = _native.load()
        d = _native.MotionPeCompileDesc()
        d.n_envs, d.n_radars, d.n_jammers, d.n_frames, d.tile = E, R, J, F, w
        d.four_pi_cubed = FOUR_PI_CUBED
        d.pd_A, d.pd_c1, d.pd_denB = sc.pd_consts
        d.in_tables, d.in_weak = keep["in_tables"].data_ptr(), keep["in_weak"].data_ptr()
        d.frames, d.frame_flags = keep["frames"].data_ptr(), keep["flags"].data_ptr()
        d.frame_snr_no, d.positions = keep["snr_no"].data_ptr(), keep["positions"].data_ptr()
        s = _native.MotionScanPeCompileDesc()
        s.n_envs, s.n_radars, s.n_jammers, s.n_frames, s.tile, s.n_levels = E, R, J, F, w, L
        s.deg_per_rad = DEG_PER_RAD
        s.pd_A, s.pd_c1, s.pd_denB = sc.pd_consts
        s.in_tables, s.scan_in = keep["in_tables"].data_ptr(), keep["scan_in"].data_ptr()
        s.frames, s.frame_snr_no = keep["frames"].data_ptr(), keep["snr_no"].data_ptr()
        s.scan_frames = keep["scan_frames"].data_ptr()
        s.pattern_frames = keep["pattern_frames"].data_ptr() if L else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        first, second = [], []
        for _ in range(4):   # rewrites the same bits: the env stays valid
            torch.cuda.synchronize(dev)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            _native.check(lib.macjd_motion_pe_compile(ctypes.byref(d), stream), "macjd_motion_pe_compile")
            e1.record()
            _native.check(lib.macjd_motion_scan_pe_compile(ctypes.byref(s), stream), "macjd_motion_scan_pe_compile")
            e2.record()
            e2.synchronize()
            first.append(e0.elapsed_time(e1) * 1e3)
            second.append(e1.elapsed_time(e2) * 1e3)
        first, second = first[1:], second[1:]
        beam_bytes = sum(keep[k].numel() * 8 for k in ("scan_frames", "pattern_frames") if k in keep)
        line.update(tile=w, n_levels=L, table_bytes=env.table_bytes, beam_table_bytes=beam_bytes, device_path_host_inputs_s=t_inputs,
                    frame_compiler_us_min_med_max=[min(first), statistics.median(first), max(first)],
                    beam_compiler_us_min_med_max=[min(second), statistics.median(second), max(second)],
                    beam_table_write_GBps=beam_bytes / (statistics.median(second) * 1e-6) / 1e9)
        env.close()
    elif mode == "host":
        t0 = time.perf_counter()
        MovingScanScenarioBatch.randomized(_base("scenario_3j4r_moving_scan.yaml"), HOST_ENVS, compile="host", **kw)
        t_host = time.perf_counter() - t0
        line.update(host_path_envs_timed=HOST_ENVS, host_path_s_timed=t_host, host_path_s_scaled_to_E=t_host * E / HOST_ENVS)
    else:
        from macjd_amd.core.mac import BasicMAC
        from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
        from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
        from test_nets_cpu import make_args, quiet
        env = Env(moving_scan_batch=MovingScanScenarioBatch.randomized(_base("scenario_3j4r_moving_scan.yaml"), E, compile="device",
                                                                      **kw), device=dev, seed=5)
        info = env.get_env_info()
        dd = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
        args = make_args(dd, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=E, epsilon_start=0.3,
                         epsilon_anneal_time=500)
        args.env_info = info
        torch.manual_seed(3)
        with quiet():
            mac = BasicMAC(info["obs_shape"], args)
            mac.cuda()
            buf = EpisodeReplayBuffer(args)
        r = BatchedEpisodeRunner(env, mac, buf, args)
        r.enable_graph()
        for _ in range(3):
            r.rollout_graphed()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
        for a, b in ev:
            a.record()
            r.rollout_graphed()
            b.record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        line.update(ms_per_batch_mean=sum(ms) / len(ms), ms_per_batch_min=min(ms), ms_per_batch_max=max(ms), reps=len(ms))
        r.release_graphs()
    line.update(device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%dT%H:%M:%S"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=MODES)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.mode:
        return one_run(a.mode, a.envs, a.frames, a.out)
    sequence = [m for _ in range(a.alternations) for m in STEP_MODES] + list(SPLIT_MODES) + ["compile", "host", "rollout"]
    for mode in sequence:     # a failing run ends the sequence: nothing more is started on the device
        subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--envs", str(a.envs), "--frames", str(a.frames),
                        "--out", a.out], check=True, timeout=300)


if __name__ == "__main__":
    main()
