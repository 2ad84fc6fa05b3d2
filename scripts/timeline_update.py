"""Kernel timeline of the replayed learner updates in a rocprofv3 --kernel-trace CSV (bench.py --mode train): one update =
the window from the end of an update's last kernel (adam_update_kernel / adam_update_reduced_kernel) to the end of the next one's; inside a replayed
group the next update's draw / gather / scan run on the side stream beside the current update's tail, so they show in
the window of the update BEFORE the one that consumes them.  Prints one window from the middle of the run, the median
period over all windows and the median duration of every kernel.  Usage:
  rocprofv3 --kernel-trace -d out -o p -f csv -- python3 bench.py --mode train --steps 300 --warmup 100 --no-cpu-baseline --no-other-modes
  python scripts/timeline_update.py out/**/p_kernel_trace.csv"""
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?")) for r in rows))
ends = [e[1] for e in ev if "adam_update_kernel" in e[2] or "adam_update_reduced_kernel" in e[2]]
if len(ends) < 8:
    sys.exit("fewer than 8 updates in the trace")
periods = [(b - a) / 1e3 for a, b in zip(ends[:-1], ends[1:])]
typical = [p for p in periods if p < 3 * statistics.median(periods)]      # (episode boundaries: rollout + store in between)
print(f"{len(ends)} updates; period between the ends of consecutive updates: median {statistics.median(periods):.1f} us, "
      f"mean of the {len(typical)} ordinary ones {statistics.mean(typical):.1f} us (the first update of a replayed group does its "
      f"draw / gather / scan itself, the others find them done)")
mid = len(periods) // 2
print("periods of 44 consecutive updates from the middle of the run (us; a replayed group shows as a repeating pattern): "
      + " ".join(f"{p:.0f}" for p in periods[mid - 22:mid + 22]))
# two consecutive windows whose mean period is the median one of all such pairs (windows with and without a prefetch launch
# take turns, so one window alone is either the short or the long kind; a pair at a group's boundary is far off the median)
pairs = [(a + b) / 2 for a, b in zip(periods[:-1], periods[1:])]
k = min(range(len(pairs) // 3, 2 * len(pairs) // 3), key=lambda i: abs(pairs[i] - statistics.median(pairs)))
# (every kernel that STARTS in a window: a side-stream launch that runs on into the next window — a later update's
# prefetch — is listed with its full duration; the idle / busy sums below count it up to the window's end.)  Two windows
# one behind the other: with the prefetch of two updates per launch (MACJD_PREFETCH_AHEAD=2) only every other one starts one.
names = []
for kk in (k, k + 1):
    if kk + 1 >= len(ends):
        break
    w0, w1 = ends[kk], ends[kk + 1]
    win = [(s, e, n, q) for s, e, n, q in ev if w0 - 100 <= s < w1]
    n_pre = sum(1 for s, _, n, _ in win if "prefetch_batch_kernel" in n and s >= w0)
    print(f"window of update {kk + 1} (t = 0 at the previous update's last kernel end; start us, duration us, queue, kernel); "
          f"prefetch launches started in it: {n_pre}:")
    for s, e, n, q in win:
        print(f"  {(s - w0) / 1e3:7.1f} {(e - s) / 1e3:6.1f}  q{q}  {n[:78]}")
    busy = sorted((s, e) for s, e, _, _ in win)
    idle, cur = 0, w0
    for s, e in busy:
        e = min(e, w1)
        if s > cur:
            idle += s - cur
        cur = max(cur, e)
    print(f"  no kernel running for {idle / 1e3:.1f} us of the window's {(w1 - w0) / 1e3:.1f} us; sum of kernel time "
          f"{sum(min(e, w1) - s for s, e, _, _ in win) / 1e3:.1f} us")
    for _, _, n, _ in win:
        if n not in names:
            names.append(n)
# how long the chain's first kernel (the Q-head pair) starts after the previous update's last kernel, over all ordinary windows,
# and how many windows start a prefetch launch
heads = [s for s, _, n, _ in ev if "qheads_pair_kernel" in n]
gaps, hi = [], 0
for a, b in zip(ends[:-1], ends[1:]):
    while hi < len(heads) and heads[hi] < a:
        hi += 1
    if hi < len(heads) and heads[hi] < b and (b - a) / 1e3 < 3 * statistics.median(periods):
        gaps.append((heads[hi] - a) / 1e3)
if gaps:
    print(f"qheads_pair_kernel starts a median {statistics.median(gaps):.1f} us after the previous update's last kernel ends "
          f"({len(gaps)} windows; 10th / 90th percentile {sorted(gaps)[len(gaps) // 10]:.1f} / {sorted(gaps)[9 * len(gaps) // 10]:.1f} us)")
n_launch = sum(1 for _, _, n, _ in ev if "prefetch_batch_kernel" in n)
print(f"prefetch_batch_kernel launches: {n_launch} for {len(ends)} updates")
# median duration per kernel name over the whole trace (update kernels only: those seen in the two windows)
print("median duration over the trace:")
for n in names:
    d = [(e - s) / 1e3 for s, e, nn, _ in ev if nn == n]
    print(f"  {statistics.median(d):6.1f} us x {len(d):5d}  {n[:78]}")
