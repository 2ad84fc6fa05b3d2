#!/usr/bin/env python3
"""Reverse-time GRU launch (ops.gru_sequence_train's backward) at the learner's shapes: 96 sequences x 101 steps at H = 64
(the 3j/4r update) and 64 x 101 at H = 128.  Per shape, by HIP events after warm-up, median of several rounds:
  whole backward   gh product + reverse-time launch + weight gradients, through autograd     (eager)
  stock autograd   backward of ops.gru_sequence_reference on the device: ~T x a dozen launches (eager)
  backward launch  macjd_gru_sequence_backward alone                                           (eager, and graph replay)
  forward scan     ops.gru_sequence                                                            (graph replay)
Graph replay times the GPU work alone; an eager figure is what a caller of train() waits for and includes the host's
share of issuing the launches.  (The autograd engine runs a backward on the stream of its forward, so a backward is
only captured together with its forward: the two autograd rows are eager.)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from bench_kernels import timeit  # noqa: E402


def eager_us(fn, iters, warmup=3):
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


def med(fn, rounds=5):
    return statistics.median(fn() for _ in range(rounds))


def main():
    entry.build()
    from macjd_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for (B, J, H) in ((32, 3, 64), (32, 2, 128)):
        T = 101
        gi = torch.randn(B, T, J, 3 * H, device=dev, requires_grad=True)
        w = (torch.randn(3 * H, H, device=dev) / H ** 0.5).requires_grad_(True)
        bb = (0.1 * torch.randn(3 * H, device=dev)).requires_grad_(True)
        dh = torch.randn(B, T, J, H, device=dev)
        with torch.no_grad():
            h_all = ops.gru_sequence(gi, w, bb)
            h_prev = torch.cat([torch.zeros_like(h_all[:, :1]), h_all[:, :-1]], dim=1)
            gh = torch.nn.functional.linear(h_prev.reshape(-1, H), w, bb).view(B, T, J, 3 * H)

        def fwd():
            with torch.no_grad():
                ops.gru_sequence(gi, w, bb)

        def launch():
            ops.gru_sequence_backward(gi, gh, h_all, w, dh)

        h_k = ops.gru_sequence_train(gi, w, bb)
        h_s = ops.gru_sequence_reference(gi, w, bb)

        def whole():
            torch.autograd.grad(h_k, (gi, w, bb), dh, retain_graph=True)

        def stock():
            torch.autograd.grad(h_s, (gi, w, bb), dh, retain_graph=True)

        gk = torch.autograd.grad(h_k, (gi, w, bb), dh, retain_graph=True)
        gs = torch.autograd.grad(h_s, (gi, w, bb), dh, retain_graph=True)
        errs = [float((a - b_).abs().max() / b_.abs().max()) for a, b_ in zip(gk, gs)]
        print(f"{B * J} sequences x {T} steps, H = {H}:  max rel |kernel - stock| dgi / dW_hh / db_hh = "
              + " / ".join(f"{e:.2e}" for e in errs), flush=True)
        for name, fn in (("whole backward (eager)", lambda: med(lambda: eager_us(whole, 50))),
                         ("stock autograd (eager)", lambda: med(lambda: eager_us(stock, 5), rounds=3)),
                         ("backward launch (eager)", lambda: med(lambda: eager_us(launch, 200))),
                         ("forward scan (graph)", lambda: med(lambda: timeit(fwd))),
                         ("backward launch (graph)", lambda: med(lambda: timeit(launch)))):
            print(f"    {name:26s} {fn():10.1f} us", flush=True)


if __name__ == "__main__":
    main()
