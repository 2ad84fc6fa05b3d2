#!/usr/bin/env python3
"""Times ONE of two env steps at 3j/4r, E = 4096, per process (run the two alternately in fresh processes):

    moving_scan   the moving scanning step (macjd_env_step_moving_scan) on config/scenario_3j4r_moving_scan.yaml
    scan_pe       the per-env scanning step under the same pattern (macjd_env_step_scan_pe_pattern) on gathered tables: env
                  e's columns hold frame e mod F of that scenario (tiled layout)

Both the way scripts/probe_env_motion.py measures: one episode of 100 back-to-back step launches captured in a HIP graph,
replayed after an untimed reset and bracketed by events on the replay stream; the first replay warms up, three are reported
(min / median / max).  ``desync`` as a third argument resets every third env after 5 steps, so that the lanes of a wave read
different frames (moving_scan only)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import yaml

import __graft_entry__ as entry

entry.build()
from macjd_amd import hipgraph
from macjd_amd.scenario import Scenario, ScenarioBatch, motion_frame_dict
from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment

which = sys.argv[1]
want_info = bool(int(sys.argv[2])) if len(sys.argv) > 2 else False
desync = len(sys.argv) > 3 and sys.argv[3] == "desync"
J, R, N, E = 3, 4, 100, 4096
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1)
pkg = os.path.dirname(os.path.abspath(sys.modules["macjd_amd"].__file__))
path = os.path.join(pkg, "config", "scenario_3j4r_moving_scan.yaml")
if which == "moving_scan":
    env = BatchedElectromagneticEnvironment(scenario=Scenario.from_yaml(path), batch_envs=E, device=dev, seed=1)
else:
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    frames = [Scenario.from_dict(motion_frame_dict(cfg, f)) for f in range(100)]
    env = BatchedElectromagneticEnvironment(scenario_batch=ScenarioBatch(frames, scan=True, pattern=True).tile(E), device=dev, seed=1)
T = torch.randint(0, 2 * R + 1, (J, E), generator=gen, device=dev, dtype=torch.int32).t()
P = torch.rand((J, E), generator=gen, device=dev).t()
mask = (torch.arange(E, device=dev) % 3 == 0).to(torch.uint8)


def prepare():
    env.reset()
    if desync:
        env._step.fill_(5)
        env.reset(mask)


side = torch.cuda.Stream(device=dev)
side.wait_stream(torch.cuda.current_stream(dev))
with torch.cuda.stream(side):
    prepare()
    for _ in range(3):
        env.step(T, P, want_info=want_info)
torch.cuda.current_stream(dev).wait_stream(side)
torch.cuda.synchronize(dev)
graph = torch.cuda.CUDAGraph()
prepare()
torch.cuda.synchronize(dev)
with hipgraph.capture(graph):
    for _ in range(N):
        env.step(T, P, want_info=want_info)
runs = []
for _ in range(4):
    prepare()
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    hipgraph.replay(graph, dev)
    t1.record()
    t1.synchronize()
    runs.append(t0.elapsed_time(t1) * 1e3 / N)
hipgraph.destroy([graph], dev)
runs = runs[1:]
print(f"E={E} 3j/4r L=4 want_info={int(want_info)} {which + (' desync' if desync else ''):20s} {statistics.median(runs):8.2f} us/step  "
      f"(min {min(runs):.2f}, max {max(runs):.2f})", flush=True)
env.close()
