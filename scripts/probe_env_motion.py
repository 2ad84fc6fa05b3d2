#!/usr/bin/env python3
"""Times the moving env step (macjd_env_step_moving, frame-major tables) against the per-env-table step it is derived from
(macjd_env_step with tiled pe_tables) at 3j/4r.  Both are measured the same way: one episode of 100 back-to-back step
launches captured in a HIP graph, replayed after an untimed reset and bracketed by events on the replay stream; three
runs each, min / median / max reported.  Also: the moving step with the step counters desynchronised inside every wave
(every third env reset after 5 steps), and the many-step launch's time per env-step.
MACJD_LIB selects another build of the library."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as entry

if not os.environ.get("MACJD_LIB"):
    entry.build()
from macjd_amd import hipgraph
from macjd_amd.scenario import Scenario, ScenarioBatch, ring_scenario_dict
from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment

J, R, N = 3, 4, 100
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1)
pkg = os.path.dirname(os.path.abspath(sys.modules["macjd_amd"].__file__))
moving = Scenario.from_yaml(os.path.join(pkg, "config", "scenario_3j4r_moving.yaml"))
batch = ScenarioBatch.randomized(ring_scenario_dict(J, R), 4096, seed=42)


def episode_us(env, T, P, want_info, prepare):
    """Microseconds per step launch: N steps replayed from one graph, three runs -> (min, median, max)."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        prepare(env)
        for _ in range(3):
            env.step(T, P, want_info=want_info)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    prepare(env)
    torch.cuda.synchronize(dev)
    with hipgraph.capture(graph):
        for _ in range(N):
            env.step(T, P, want_info=want_info)
    runs = []
    for _ in range(4):   # the first replay warms up
        prepare(env)
        torch.cuda.synchronize(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        hipgraph.replay(graph, dev)
        t1.record()
        t1.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / N)
    hipgraph.destroy([graph], dev)
    runs = runs[1:]
    return min(runs), statistics.median(runs), max(runs)


def synced(env):
    env.reset()


def desynced(env):
    """Step counters 5 + (0 on every third env, else 5): neighbouring lanes read different frames from the first step on."""
    env.reset()
    env._step.fill_(5)
    env.reset(desynced.mask[env.batch_envs])


desynced.mask = {}

for logE in [int(a) for a in (sys.argv[1:] or ["12", "20"])]:
    E = 1 << logE
    T = torch.randint(0, 2 * R + 1, (J, E), generator=gen, device=dev, dtype=torch.int32).t()
    P = torch.rand((J, E), generator=gen, device=dev).t()
    desynced.mask[E] = (torch.arange(E, device=dev) % 3 == 0).to(torch.uint8)
    pe = BatchedElectromagneticEnvironment(scenario_batch=batch.tile(E) if E > 4096 else batch, device=dev, seed=1)
    mv = BatchedElectromagneticEnvironment(scenario=moving, batch_envs=E, device=dev, seed=1)
    # diagnostic twin of the moving env: the position columns written into dense [E, 2R + 2J] rows (columns 0..13, row
    # stride 14) instead of the [E, S] state rows (14 of 46 columns, row stride 184 B) — separates the cost of the scattered
    # partial-line stores from the cost of choosing the table column by the step counter
    dn = BatchedElectromagneticEnvironment(scenario=moving, batch_envs=E, device=dev, seed=1)
    n_pos = 2 * R + 2 * J
    dense_rows = torch.zeros((E, n_pos), device=dev)
    dense_cols = torch.arange(n_pos, dtype=torch.int32, device=dev)
    dn._motion_io.state, dn._motion_io.st_se = dense_rows.data_ptr(), n_pos
    dn._motion_io.position_columns = dense_cols.data_ptr()
    for want_info in (False, True):
        rows = [("per-env tables (tiled)", episode_us(pe, T, P, want_info, synced)),
                ("moving, counters in step", episode_us(mv, T, P, want_info, synced)),
                ("moving, counters desynchronised", episode_us(mv, T, P, want_info, desynced)),
                ("moving, dense position rows", episode_us(dn, T, P, want_info, synced))]
        for label, (lo, med, hi) in rows:
            print(f"E=2^{logE} want_info={int(want_info)} {label:34s} {med:9.2f} us/step  (min {lo:.2f}, max {hi:.2f})", flush=True)
    # the many-step launch: one episode (N steps) of all E envs, + the counter-advance launch
    if E * N * 3 * 4 < 2 ** 32:
        Tn = T.contiguous().view(1, E, J).expand(N, -1, -1).contiguous()
        Pn = P.contiguous().view(1, E, J).expand(N, -1, -1).contiguous()
        rew = torch.zeros((N, E), device=dev)
        term = torch.zeros((N, E), dtype=torch.uint8, device=dev)
        rdpj = torch.zeros((N, E, 3), device=dev)
        runs = []
        for _ in range(4):
            mv.reset()
            torch.cuda.synchronize(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            mv.step_many(Tn, Pn, rew, term, rdpj)
            t1.record()
            t1.synchronize()
            runs.append(t0.elapsed_time(t1) * 1e3)
        runs = runs[1:]
        print(f"E=2^{logE} many-step launch ({N} steps): {statistics.median(runs):10.1f} us  (min {min(runs):.1f}, max {max(runs):.1f})  "
              f"= {statistics.median(runs) * 1e3 / (N * E):.3f} ns per env-step", flush=True)
    else:
        print(f"E=2^{logE} many-step launch: skipped ({N} x E outputs pass the 32-bit offsets of one launch)", flush=True)
    pe.close()
    mv.close()
    dn.close()
