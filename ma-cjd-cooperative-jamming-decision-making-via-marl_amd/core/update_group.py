"""K consecutive learner updates captured as ONE HIP graph (``QMixLearner.enable_graphs(updates_per_graph=K)``,
``train_from_buffer_many``): the schedule of a group as pure functions (``prefetch_plan``, ``group_schedule``) and the
object that captures it and owns every tensor whose address the captured launches bake (``UpdateGroup``)."""
from __future__ import annotations

import collections

import torch

from .. import hipgraph, ops, options

PrefetchLaunch = collections.namedtuple("PrefetchLaunch", "issue_at updates offsets sets")
GroupStep = collections.namedtuple("GroupStep", "reads prefetched issues draw")   # one update of a group (group_schedule)
# what a prefetched update waits for and takes over: the events behind the gather and the scan on the side stream (None: a
# wait earlier on the chain's stream covers it) and the batch's mask sum (``_forward_backward_full(prefetched=...)``)
Prefetched = collections.namedtuple("Prefetched", "gather_done scan_done tot_m")


def prefetch_plan(K: int, ahead: int):
    """The prefetches of a captured group of K pipelined updates: (launches, n_sets).  A launch is issued behind the Q-head
    grid of update ``issue_at`` and prefetches the batches of ``updates`` at the sampler's counter ``offsets`` into the
    staging ``sets``; update u reads set u % n_sets and its batch is the draw of offset u - 1 (update 0 runs on the batch
    drawn before the group; the group's closing draw has offset K - 1).
      ahead = 1  one launch per update 1 .. K-1, issued by the update before it; two staging sets.
      ahead = 2  one launch per PAIR (a, a + 1), a = 1, 3, 5, .., issued by update max(0, a - 2) — two updates before its
                 first consumer, so that in steady state a launch has two update periods to finish and no update waits for
                 its scan; a one-batch launch for the last update when K - 1 is odd; four staging sets: the launch for
                 (a, a + 1) is in flight beside the updates a - 2 and a - 1, which read the two other sets."""
    if ahead not in (1, 2):
        raise ValueError("prefetch_plan: ahead must be 1 or 2")
    n_sets = 2 * ahead
    launches = []
    for a in range(1, K, ahead):
        updates = tuple(range(a, min(a + ahead, K)))
        launches.append(PrefetchLaunch(max(0, a - ahead), updates, tuple(u - 1 for u in updates),
                                       tuple(u % n_sets for u in updates)))
    return launches, n_sets


def group_schedule(K: int, pipelined: bool, one_launch: bool = False, ahead: int = 1):
    """What each update u = 0 .. K-1 of a captured group does: ([GroupStep], n_sets) — the staging set it ``reads``, whether
    its batch was ``prefetched``, the PrefetchLaunch it ``issues`` behind its Q-head grid (or None), and the counter offset of
    the ``draw`` its optimiser launch makes (None: no draw).
      not pipelined  every update scans and gathers for itself (set 0) and its optimiser launch draws the next batch.
      pipelined      update 0 prepares its own batch; the batches of 1 .. K-1 are prefetched on the side stream by the
                     launches of ``prefetch_plan``, so only the LAST optimiser launch draws (the batch of the next group):
        one_launch     a prefetch is one launch of ``ahead`` batches that only READS the sampler's counter, at the offsets
                       0 .. K-2: the closing draw has offset K - 1 and leaves the counter K further, as K draws do.
        otherwise      draw, gather, mask sum and scan as four launches, one update ahead (the ``ahead`` = 1 plan with
                       another issue function); its draw advances the counter itself: the closing draw has offset 0."""
    if not pipelined:
        return [GroupStep(0, False, None, 0)] * K, 1
    launches, n_sets = prefetch_plan(K, ahead if one_launch else 1)
    issues = {l.issue_at: l for l in launches}
    closing = K - 1 if one_launch else 0
    return [GroupStep(u % n_sets, u > 0, issues.get(u), closing if u == K - 1 else None) for u in range(K)], n_sets


class UpdateGroup:
    """The graph of K updates of ``learner`` and everything it bakes addresses of: the staging sets, the index rows, every
    prefetched batch's outputs and the statistics rows.  Between two replayed graphs the stream pays a launch-to-launch
    hand-over (~20 us here) that an edge inside a graph does not."""

    def __init__(self, learner, K, stage, keys, srcs, body_a, pool):
        lr = self.learner = learner
        self.K, self.keys, self.srcs, self.graph, self.rows = K, keys, srcs, torch.cuda.CUDAGraph(), []
        self.sampler = (lr._g_idx, lr._g_n_stored, lr._g_draws, lr._sampler_seed())
        # Inside the group the updates are software-pipelined: everything of update k + 1 that depends on neither the
        # weights nor update k's results — the draw of its episodes, the gather into the OTHER staging set, the scan
        # launch (frozen body) — is issued on the side stream right behind update k's join and runs beside update k's
        # serial tail; update k + 1 then starts at its taken-action Q-head and finds the scan done at its join
        # (-17 us per pipelined update: the gather, its hand-over and the wait for the scan leave the chain).  Same
        # launches on the same data in an order that respects every dependence: same results (tested bitwise).
        self.pipelined = (lr._g_scan_from_ring and lr._g_actor_in_scan and options.get("UPDATE_STREAMS") != "1"
                          and options.on("PIPELINED_GROUP"))
        # The prefetch as ONE launch (ops.prefetch_batches: every workgroup evaluates the sampler's formula for the indices it
        # needs at a counter offset baked into the launch, so the draw, the gather and the mask sum run BESIDE the scan
        # instead of in front of it) — shared frozen body at hidden size 64; MACJD_PREFETCH_LAUNCH=0 and every other shape:
        # the four launches one behind the other.
        self.prefetch_launch = bool(self.pipelined and options.on("PREFETCH_LAUNCH") and "filled" in keys
                                    and ops.prefetch_batch_supported(lr._body_agents()[0], lr._g_B, srcs))
        # ... and TWO updates ahead (MACJD_PREFETCH_AHEAD): one launch prefetches the batches of a pair of updates and is
        # issued two updates before the first of them, so no Q-head grid waits for its scan — the prefetch leaves the cycle
        # that bounded the update.  "1": one launch per update, issued by the update before it.
        self.prefetch_ahead = 2 if (self.prefetch_launch and options.get("PREFETCH_AHEAD") != "1") else 1
        self.schedule, n_sets = group_schedule(K, self.pipelined, self.prefetch_launch, self.prefetch_ahead)
        # (the captured launches write and read the further staging sets through baked addresses: they have to live as long
        # as the graph.  Until round 3 nothing held the second set once enable_graphs returned — the freed blocks stayed
        # cached, so it went unnoticed until another capture's torch.cuda.empty_cache() unmapped them: a GPU memory fault
        # in the first replay of the group at 12j/16r.)  So do each set's index row (one-launch prefetches: _g_idx is then
        # written by the closing draw alone) and each prefetched batch's scan output, actor rows and mask sum.
        self.stages = [stage] + [{k: torch.zeros_like(v) for k, v in stage.items()} for _ in range(n_sets - 1)]
        self.idx_rows = torch.zeros(n_sets, lr._g_B, dtype=torch.int64, device=lr.device) if self.prefetch_launch else None
        self.batches = {}   # update -> (h [target, eval], P [target, eval], Prefetched) of its prefetched batch
        self.paired = self.pipelined and lr._paired_heads_ok(stage, lr._g_T)
        self._capture(body_a, pool)

    def _capture(self, body_a, pool):
        lr, T = self.learner, self.learner._g_T
        single_norm = lr._grad_norm
        issue = self._issue_one_launch if self.prefetch_launch else self._issue_four_launches
        with hipgraph.capture(self.graph, pool=pool):
            for u, step in enumerate(self.schedule):
                # (called by the update right behind its join / Q-head grid: _forward_backward_full(after_join=...))
                hook = (lambda fork=True, launch=step.issues: issue(launch, fork)) if step.issues is not None else None
                if step.prefetched:
                    h_pre, p_pre, pf = self.batches[u]
                    lr._forward_backward_full(self.stages[step.reads], T, pre_scan=h_pre, pre_actor=p_pre, prefetched=pf,
                                              after_join=hook)
                elif self.pipelined:
                    self._first_update(self.stages[step.reads], hook)
                else:
                    body_a()
                self.rows.append(lr._last_stats4)       # this update's (loss, mean Q_tot, mean target, grad norm)
                lr._grad_norm = self.rows[-1][3]
                if lr._g_graphed_ar:
                    lr._allreduce_grads(force=True)
                # the update's last launch draws the next batch — unless a prefetch has done or will do so (group_schedule)
                lr._clip_and_step(sample_next=None if step.draw is None else self.sampler + (step.draw,))
            if self.pipelined:
                torch.cuda.current_stream(lr.device).wait_stream(lr._update_stream())   # every fork rejoins
        lr._grad_norm = single_norm

    def _first_update(self, stage, hook):
        """Update 0 of a pipelined group: its own scan (side stream) and gather (this stream) on the batch in _g_idx."""
        lr, T = self.learner, self.learner._g_T
        pre = lr._scan_from_ring_early()
        ops.gather_rows(lr._g_idx, self.srcs, [stage[k] for k in self.keys])
        pf = None
        if self.paired:
            # the group's first update in the paired form too: its scan (side stream) and its gather + mask sum (this
            # stream) run beside each other, then the same chain as every other update — and the second update's prefetch
            # forks as early as everyone's (first two updates of a group: 169 + 134 -> 150 + 111 us)
            tot_m = ops.td_mask_sum(stage["filled"], T - 1)
            scan_done = torch.cuda.Event()
            scan_done.record(lr._update_stream())
            pf = Prefetched(gather_done=None, scan_done=scan_done, tot_m=tot_m)   # (the gather ran on this stream)
        lr._forward_backward_full(stage, T, pre_scan=pre[0], pre_actor=pre[1], prefetched=pf, after_join=hook)

    def _fork(self, fork):
        """The side stream, ordered behind the users of what a prefetch overwrites (index rows, a staging set).  ``fork`` is
        an Event recorded earlier on the origin stream; True: wait for the origin stream as it stands; False: no wait
        (those users ran earlier on the side stream itself)."""
        ts = self.learner._update_stream()
        if isinstance(fork, torch.cuda.Event):
            ts.wait_event(fork)
        elif fork:
            ts.wait_stream(torch.cuda.current_stream(self.learner.device))
        return ts

    def _issue_one_launch(self, launch, fork):
        """draw + gather + mask sum + scan of the later updates ``launch.updates`` as ONE launch on the side stream."""
        lr, ring = self.learner, self.learner._g_buffer.buffers
        ts = self._fork(fork)
        assert lr._body_is_shared()
        with torch.cuda.stream(ts), torch.no_grad():
            res = ops.prefetch_batches(
                ring["obs"], [lr.mac.agent], lr._g_B, lr.n_agents, lr._g_T + 1, self.sampler[1:], self.srcs,
                [(off, True, [self.stages[s][k] for k in self.keys], self.idx_rows[s])
                 for off, s in zip(launch.offsets, launch.sets)], ring["filled"], lr._g_T - 1)
            ev = torch.cuda.Event()   # one launch: the gathered batches and the scans are there together
            ev.record(ts)
        for i, (u, (h, p, tot_m)) in enumerate(zip(launch.updates, res)):
            # the first consumer waits for the launch; on the chain's stream that wait covers the later ones (the
            # paired update takes "no event"; the other forms wait where they always do, for an event long set)
            e = ev if (i == 0 or not self.paired) else None
            self.batches[u] = ([h, h], [p, p], Prefetched(e, e, tot_m))

    def _issue_four_launches(self, launch, fork):
        """draw, gather, mask sum and scan of the next update as four launches on the side stream, through _g_idx."""
        lr, ring = self.learner, self.learner._g_buffer.buffers
        (u,), dst = launch.updates, self.stages[launch.sets[0]]
        ts = self._fork(fork)
        agents, both = lr._body_agents()
        with torch.cuda.stream(ts), torch.no_grad():
            ops.sample_episodes(*self.sampler)
            ops.gather_rows(lr._g_idx, self.srcs, [dst[k] for k in self.keys])
            tot_m = ops.td_mask_sum(dst["filled"], lr._g_T - 1)     # the loss's only global sum the gradient needs
            gather_done = torch.cuda.Event()
            gather_done.record(ts)
            h, ps = ops.gru_sequence_from_obs(ring["obs"], lr._g_idx, agents, lr._g_B, lr.n_agents, lr._g_T + 1, with_actor=True)
            scan_done = torch.cuda.Event()
            scan_done.record(ts)
        self.batches[u] = (both(h), both(ps), Prefetched(gather_done, scan_done, tot_m))
