#!/usr/bin/env python3
"""Measurements of the per-env moving scenarios (include/macjd.h, macjd_motion_pe_io) at 3j/4r, E = 4096, F = 100; one JSON
line per figure into profiles/moving_pe_probe.jsonl (or the path given as the first argument):

  (a) the device frame compiler's launch (macjd_motion_pe_compile, HIP events, three runs) beside the host path's wall time
      for the same batch — the host path is timed on the first HOST_ENVS envs and scaled to E (it is linear in the envs);
  (b) microseconds per step launch and nanoseconds per item of the many-step launch of the per-env moving step beside the
      shared-frame moving step and the static per-env step, each one episode of F back-to-back launches replayed from one HIP
      graph after an untimed reset and bracketed by events on the replay stream (three runs: min / median / max);
  (c) the HBM traffic the per-env moving step achieves, at ~430 B per env-step, as a fraction of the device's peak.
MACJD_LIB selects another build of the library."""
import ctypes
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import yaml

import __graft_entry__ as entry

if not os.environ.get("MACJD_LIB"):
    entry.build()
from macjd_amd import _native, hipgraph
from macjd_amd.scenario import FOUR_PI_CUBED, MovingScenarioBatch, Scenario, ScenarioBatch, motion_frame_dict
from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment

J, R, E, F = 3, 4, 4096, 100
HOST_ENVS = 64
BYTES_PER_ENV_STEP = 430      # 45 float64 rows + 12 flag bytes of the frame, actions, FSM bits, outputs, 14 position floats
HBM_PEAK = 8.0e12             # MI355X: 8 TB/s
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "profiles", "moving_pe_probe.jsonl")
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1)
pkg = os.path.dirname(os.path.abspath(sys.modules["macjd_amd"].__file__))
with open(os.path.join(pkg, "config", "scenario_3j4r_moving.yaml")) as f:
    base = yaml.safe_load(f)
conf = SimpleNamespace(episode_limit=F)
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def episode_us(env, T, P):
    """Microseconds per step launch: F steps replayed from one graph, three runs -> (min, median, max)."""
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
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        hipgraph.replay(graph, dev)
        t1.record()
        t1.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / F)
    hipgraph.destroy([graph], dev)
    runs = runs[1:]
    return min(runs), statistics.median(runs), max(runs)


def many_ns(env, T, P):
    """Nanoseconds per item of one many-step launch of F steps (+ the counter advance), three runs."""
    Tn = T.contiguous().view(1, E, J).expand(F, -1, -1).contiguous()
    Pn = P.contiguous().view(1, E, J).expand(F, -1, -1).contiguous()
    rew = torch.zeros((F, E), device=dev)
    term = torch.zeros((F, E), dtype=torch.uint8, device=dev)
    rdpj = torch.zeros((F, E, 3), device=dev)
    runs = []
    for _ in range(4):
        env.reset()
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        env.step_many(Tn, Pn, rew, term, rdpj)
        t1.record()
        t1.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e6 / (F * E))
    runs = runs[1:]
    return min(runs), statistics.median(runs), max(runs)


# ---- (a) compile ----------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
dev_batch = MovingScenarioBatch.randomized(base, E, seed=42, config=conf, velocity_jitter=1.0, compile="device")
t_inputs = time.perf_counter() - t0
t0 = time.perf_counter()
MovingScenarioBatch.randomized(base, HOST_ENVS, seed=42, config=conf, velocity_jitter=1.0, compile="host")
t_host = time.perf_counter() - t0
pe_mv = BatchedElectromagneticEnvironment(moving_batch=dev_batch, device=dev, seed=1)
keep = pe_mv._motion_keep
d = _native.MotionPeCompileDesc()
d.n_envs, d.n_radars, d.n_jammers, d.n_frames, d.tile = E, R, J, F, pe_mv._pe_tile
d.four_pi_cubed = FOUR_PI_CUBED
d.pd_A, d.pd_c1, d.pd_denB = pe_mv.scenario.pd_consts
d.in_tables, d.in_weak = keep["in_tables"].data_ptr(), keep["in_weak"].data_ptr()
d.frames, d.frame_flags = keep["frames"].data_ptr(), keep["flags"].data_ptr()
d.frame_snr_no, d.positions = keep["snr_no"].data_ptr(), keep["positions"].data_ptr()
lib = _native.load()
runs = []
for _ in range(4):   # rewrites the same bits: the env stays valid
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _native.check(lib.macjd_motion_pe_compile(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream), "macjd_motion_pe_compile")
    e1.record()
    e1.synchronize()
    runs.append(e0.elapsed_time(e1) * 1e3)
runs = runs[1:]
emit(what="compile", size="3j/4r", E=E, F=F, tile=pe_mv._pe_tile, table_bytes=pe_mv.table_bytes,
     device_launch_us_min_med_max=[min(runs), statistics.median(runs), max(runs)],
     device_path_host_inputs_s=t_inputs, host_path_envs_timed=HOST_ENVS, host_path_s_timed=t_host,
     host_path_s_scaled_to_E=t_host * E / HOST_ENVS,
     table_write_GBps=pe_mv.table_bytes / (statistics.median(runs) * 1e-6) / 1e9)

# ---- (b) steps ------------------------------------------------------------------------------------------------------------
T = torch.randint(0, 2 * R + 1, (J, E), generator=gen, device=dev, dtype=torch.int32).t()
P = torch.rand((J, E), generator=gen, device=dev).t()
shared = BatchedElectromagneticEnvironment(scenario=Scenario.from_dict(base, config=conf), batch_envs=E, device=dev, seed=1)
static_pe = BatchedElectromagneticEnvironment(
    scenario_batch=ScenarioBatch.randomized(motion_frame_dict(base, 0), E, seed=42, config=conf), device=dev, seed=1)
res = {}
for name, env in (("per_env_moving", pe_mv), ("shared_frame_moving", shared), ("static_per_env", static_pe)):
    res[name] = episode_us(env, T, P)
    emit(what="step", path=name, E=E, F=F, us_per_step_min_med_max=list(res[name]))
for name, env in (("per_env_moving", pe_mv), ("shared_frame_moving", shared), ("static_per_env", static_pe)):
    lo, med, hi = many_ns(env, T, P)
    emit(what="step_many", path=name, E=E, F=F, ns_per_item_min_med_max=[lo, med, hi], us_per_step_equivalent=med * E * 1e-3)

# ---- (c) HBM fraction -----------------------------------------------------------------------------------------------------
med = res["per_env_moving"][1]
bps = E * BYTES_PER_ENV_STEP / (med * 1e-6)
emit(what="hbm", path="per_env_moving", bytes_per_env_step=BYTES_PER_ENV_STEP, achieved_GBps=bps / 1e9,
     fraction_of_peak=bps / HBM_PEAK, peak_GBps=HBM_PEAK / 1e9,
     step_ratio_vs_shared_frame=med / res["shared_frame_moving"][1], step_ratio_vs_static_per_env=med / res["static_per_env"][1])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    for ln in lines:
        f.write(json.dumps(ln) + "\n")
for env in (pe_mv, shared, static_pe):
    env.close()
