#!/usr/bin/env python3
"""TD(lambda) loss launch (macjd_td_lambda_loss) at the learner's own shape, B = 32 episodes x Tm1 = 99 steps, operands that
are [:, :-1] / [:, 1:] slices of [B, 100, 1] tensors, against
  * macjd_td_loss on the same buffers (the one-step launch it stands beside: recorded, not judged — both are bound by the
    launch latency), and
  * ops.td_lambda_reference on the device (the stock-torch reverse loop it replaces: Tm1 x a handful of launches).
The three alternate inside one process with no profiler attached: per block, HIP events around many back-to-back replays
after a warm-up (C-ABI calls on prebuilt structs: no allocation in the timed region); the block means go to the .jsonl.  Every
block must show the launch ahead of the stock-torch loop.  Then the per-update time of eager ``train()`` at 3j/4r (batch 32,
100 steps, H = 64) with and without ``td_lambda = 0.8``.
    python scripts/probe_td_lambda.py [--out profiles/td_lambda_probe.jsonl] [--blocks 5]"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as entry  # noqa: E402


def events_us(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def launches(dev):
    """(new launch, one-step launch, stock-torch loop) as callables on one set of buffers, + what keeps them alive."""
    import torch
    from macjd_amd import _native, ops
    lib = _native.load()
    B, T, gamma, lam = 32, 100, 0.99, 0.8
    g = torch.Generator(device="cpu").manual_seed(0)
    y_full, tq_full = (3 * torch.randn(B, T, 1, generator=g)).to(dev), (3 * torch.randn(B, T, 1, generator=g)).to(dev)
    reward = torch.randn(B, T, 1, generator=g).to(dev)
    length = torch.randint(T // 2, T + 1, (B, 1, 1), generator=g)
    step = torch.arange(T).view(1, T, 1)
    filled, terminated = (step < length).to(dev), (step == length - 1).to(dev)
    y, tq, r, term, fill = y_full[:, :-1], tq_full[:, 1:], reward[:, :-1], terminated[:, :-1], filled[:, :-1]
    stats, gy, ret = torch.empty(4, device=dev), torch.empty(B, T - 1, 1, device=dev), torch.empty(B, T - 1, 1, device=dev)
    io_l = _native.TdLambdaIO()
    td = io_l.td
    td.B, td.Tm1, td.gamma = B, T - 1, gamma
    td.y, td.y_sb, td.tq, td.tq_sb = y.data_ptr(), T, tq.data_ptr(), T
    td.gy, td.gy_sb, td.gy_cols = gy.data_ptr(), T - 1, T - 1
    td.reward, td.r_sb, td.r_st = r.data_ptr(), T, 1
    td.terminated, td.t_sb, td.t_st = term.data_ptr(), T, 1
    td.filled, td.f_sb, td.f_st = fill.data_ptr(), T, 1
    td.stats = stats.data_ptr()
    io_l.lam, io_l.ret, io_l.ret_sb = lam, ret.data_ptr(), T - 1
    io_1 = _native.TdLossIO()
    ctypes.memmove(ctypes.byref(io_1), ctypes.byref(io_l.td), ctypes.sizeof(io_1))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def new():
        _native.check(lib.macjd_td_lambda_loss(ctypes.byref(io_l), stream), "macjd_td_lambda_loss")

    def one_step():
        _native.check(lib.macjd_td_loss(ctypes.byref(io_1), stream), "macjd_td_loss")

    def stock():
        return ops.td_lambda_reference(y, tq, r, term, fill, gamma, lam)

    new()
    want = stock()
    torch.cuda.synchronize()
    got = (stats[0].item(), stats[1].item(), stats[2].item())
    for a, b in zip(got, want):
        assert abs(a - b.item()) <= 1e-4 * max(1.0, abs(b.item())), (got, [w.item() for w in want])
    return new, one_step, stock, (y_full, tq_full, reward, filled, terminated, stats, gy, ret)


def train_us(td_lambda, updates, reps):
    """Eager train() on sampled batches of the benchmark's 3j/4r configuration: microseconds per update, per repetition."""
    import time
    import torch
    from macjd_amd import bench_rollout
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.scenario import Scenario, ring_scenario_dict
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    dev = torch.device("cuda", 0)
    sc = Scenario.from_dict(ring_scenario_dict(3, 4))
    env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=256, device=dev, seed=1)
    args = bench_rollout.make_args(sc, 64, dev, batch_envs=256)
    if td_lambda is not None:
        args.td_lambda = td_lambda
    torch.manual_seed(42)
    with contextlib.redirect_stdout(io.StringIO()):
        mac = BasicMAC(args.obs_shape, args)
        buf = EpisodeReplayBuffer(args, device=dev)
        learner = QMixLearner(mac, args)
    BatchedEpisodeRunner(env, mac, buf, args).run(sync_stats=False)
    batch = buf.sample(args.batch_size)
    for _ in range(20):
        learner.train(batch, None, sync_stats=False)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(updates):
            learner.train(batch, None, sync_stats=False)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / updates * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "td_lambda_probe.jsonl"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    entry.build()
    import torch
    dev = torch.device("cuda", 0)
    new, one_step, stock, keep = launches(dev)
    rows = []
    for block in range(a.blocks):
        row = {"block": block, "shape": [32, 99],
               "td_lambda_launch_us": events_us(new, 2000, 200),
               "td_loss_launch_us": events_us(one_step, 2000, 200),
               "stock_torch_loop_us": events_us(stock, 20, 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if not a.no_train:
        for name, lam in (("eager_train_us_per_update", None), ("eager_train_td_lambda_0.8_us_per_update", 0.8)):
            row = {name: [round(x, 1) for x in train_us(lam, 200, 4)]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    assert all(r["td_lambda_launch_us"] < r["stock_torch_loop_us"] for r in rows if "block" in r), \
        "the launch must be ahead of the stock-torch loop in every block"


if __name__ == "__main__":
    main()
