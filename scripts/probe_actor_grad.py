#!/usr/bin/env python3
"""One-launch actor gradient (ops.actor_gradient) against its stock-torch form under autograd
(ops.actor_gradient_reference: ~25 launches, materialises [N, A, H]) at the learner's row counts: 32 episodes x 99 steps x
3 agents at 3j/4r (the C2 update) and 32 x 99 x 12 at 12j/16r.  Per shape, by HIP events after warm-up, median of several
rounds of eager calls (what a caller of train() waits for, output allocations included); then the maximal relative
difference between the two on every output."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


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
    lin = lambda o, i: ((torch.rand(o, i, device=dev) * 2 - 1) / i ** 0.5, (torch.rand(o, device=dev) * 2 - 1) / i ** 0.5)
    for name, J, (S, Ha, H, A) in (("3j/4r", 3, (46, 128, 64, 9)), ("12j/16r", 12, (184, 128, 64, 33))):
        N = 32 * 99 * J
        layers = [lin(Ha, S), lin(Ha, Ha), lin(A, Ha)]
        W1q, b1q = lin(H, H + A + 1)
        w2q, b2q = lin(1, H)
        x = torch.randn(N, S, device=dev)
        base = torch.tanh(torch.randn(N, H, device=dev)) @ W1q[:, :H].t() + b1q
        m = torch.rand(N, device=dev) / N
        args = (x, base, m, layers, W1q, w2q, b2q, H, A)
        assert ops.actor_gradient_supported(x, S, Ha, H, A)
        got, ref = ops.actor_gradient(*args), ops.actor_gradient_reference(*args)
        torch.cuda.synchronize()
        errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref)]
        t_k = med(lambda: eager_us(lambda: ops.actor_gradient(*args), 200))
        t_r = med(lambda: eager_us(lambda: ops.actor_gradient_reference(*args), 20), rounds=3)
        print(f"{name}: {N} rows, (S, Ha, H, A) = {(S, Ha, H, A)}", flush=True)
        print(f"    ops.actor_gradient            {t_k:10.1f} us / call", flush=True)
        print(f"    ops.actor_gradient_reference  {t_r:10.1f} us / call   ratio {t_r / t_k:.1f}", flush=True)
        print("    max rel |kernel - stock| a1 / a2 / g3 / g2 / g1 / qsum (all rows, ReLU ties included) = "
              + " / ".join(f"{e:.2e}" for e in errs), flush=True)
        assert t_k < t_r, "the kernel path must be the faster of the two"


if __name__ == "__main__":
    main()
