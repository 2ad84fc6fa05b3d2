"""The multi-batch prefetch launch (``macjd_prefetch_batches``, csrc/macjd_nets.hip ``prefetch_batch_kernel``) against the
single launches it stands for (``ops.prefetch_batch`` at the same counter offsets into separate destinations), and a
captured group of updates with MACJD_PREFETCH_AHEAD = 2 (pairs, two updates ahead, four staging sets) against = 1 (one
launch per update).  Everything bit for bit: the same device functions run on the same data, only their place in time moves.

Kernel cases: n in {1, 2, 3} batches, J in {3, 2}, B in {5, 1}, T + 1 = 4 scanned steps (mask sum over T - 1 = 2), a ring of
7 stored episodes (not a power of two: the permutation's cycle-walk runs), 3 stored < B (indices i mod 3), "no draw" on the
first batch only, and `filled` rows of different lengths (the batches' mask sums are checked against the rows their own
indices name).

Two shapes are the nearest ones that the launch under test accepts: the gather copies whole rows in 4-byte words
(``ops.gather_rows_supported``), and the bool rows `terminated` / `filled` hold one byte per stored step.  So the ring's rows
carry 4 steps, of which the scan runs T + 1 = 4 and the mask sum reads 2 (rows of T = 3 steps are 3 bytes: refused); and the
small learner's episode limit is 8, not 6 (at 6 the rows are 6 bytes, ``enable_graphs`` takes the index_select path and
captures no group at all, so neither arrangement would run)."""
import gc
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_nets_cpu import load, make_args, quiet  # noqa: E402
from tests_golden_helpers import sample_episodes_mirror  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED, C0, NB, TR, T = 0x5EED1234ABCD, 11, 7, 4, 3   # sampler seed, first counter value, ring slots, stored steps, T (T + 1 scanned)


def _ring(J, S, ragged, gen):
    r = lambda *shape: torch.randn(*shape, generator=gen, device=DEV)
    ring = {
        "obs": r(NB, TR + 1, J, S), "state": r(NB, TR + 1, 7), "hidden_state": r(NB, TR + 1, J, 4),
        "actions_discrete": torch.randint(0, 9, (NB, TR, J, 1), generator=gen, device=DEV, dtype=torch.int32),
        "actions_continuous": r(NB, TR, J, 1), "reward": r(NB, TR, 1),
        "terminated": torch.zeros(NB, TR, 1, dtype=torch.bool, device=DEV),
        "filled": torch.zeros(NB, TR, 1, dtype=torch.bool, device=DEV),
    }
    for e in range(NB):   # ragged: episode e carries 1 + e % 3 steps, so the first T - 1 = 2 hold one or two True
        n = 1 + e % 3 if ragged else TR
        ring["filled"][e, :n] = True
        ring["terminated"][e, n - 1] = True
    return ring


def _staging(ring, B, gen):
    """Staging tensors over raw byte buffers of random content (what a launch leaves untouched stays comparable): the
    action keys with one step more than stored, like the learner's."""
    raws, dsts = [], []
    for k, v in ring.items():
        shape = (B, TR + 1 if k.startswith("actions") else v.shape[1]) + tuple(v.shape[2:])
        nbytes = v.element_size() * int(torch.tensor(shape).prod())
        raw = torch.randint(0, 256, (nbytes,), generator=gen, device=DEV, dtype=torch.uint8)
        raws.append(raw)
        dsts.append(raw.view(v.dtype).view(shape))
    return raws, dsts


@pytest.fixture(scope="module")
def agent():
    from macjd_amd.core.networks import RNNAgent
    _, d = load("3j4r_h64")
    torch.manual_seed(4)
    with quiet():
        a = RNNAgent(d["S"], make_args(d, device="cuda", use_cuda=True)).to(DEV)
    return a, d["S"]


CASES = [  # n batches, B, J, N stored, first offset, first batch draws, ragged `filled`
    (1, 5, 3, 7, 0, True, False), (2, 5, 3, 7, 0, True, False), (3, 5, 3, 7, 2, True, False),
    (2, 1, 2, 7, 1, True, False), (3, 5, 2, 7, 0, True, False), (3, 1, 3, 7, 0, True, False),
    (2, 5, 3, 3, 0, True, False), (2, 5, 3, 7, 1, False, False), (3, 5, 3, 7, 0, True, True),
    (3, 5, 2, 7, 3, False, True),
]


@pytest.mark.parametrize("n,B,J,N,off,draw_first,ragged", CASES)
def test_one_launch_of_n_batches_equals_n_single_launches(agent, n, B, J, N, off, draw_first, ragged):
    from macjd_amd import ops
    a, S = agent
    gen = torch.Generator(device=DEV).manual_seed(1000 * n + 100 * B + 10 * J + N)
    ring = _ring(J, S, ragged, gen)
    keys = list(ring)
    srcs = [ring[k] for k in keys]
    assert ops.prefetch_batch_supported([a], B, srcs)
    n_stored = torch.tensor([N], dtype=torch.int32, device=DEV)
    preset = torch.tensor([(3 * t + 1) % N for t in range(B)], dtype=torch.int64, device=DEV)
    draws = [draw_first] + [True] * (n - 1)
    sides = []
    for multi in (False, True):
        counter = torch.tensor([C0], dtype=torch.int64, device=DEV)
        g2 = torch.Generator(device=DEV).manual_seed(77)
        stag = [_staging(ring, B, g2) for _ in range(n)]
        idxs = [preset.clone() for _ in range(n)]
        with torch.no_grad():
            if multi:
                res = ops.prefetch_batches(ring["obs"], [a], B, J, T + 1, (n_stored, counter, SEED), srcs,
                                           [(off + i, draws[i], stag[i][1], idxs[i]) for i in range(n)], ring["filled"], T - 1)
            else:
                res = []
                for i in range(n):
                    hs, ps, tot = ops.prefetch_batch(ring["obs"], [a], B, J, T + 1, (idxs[i], n_stored, counter, SEED), srcs,
                                                     stag[i][1], ring["filled"], T - 1, offset=off + i, draw=draws[i])
                    res.append((hs[0], ps[0], tot))
        torch.cuda.synchronize()
        assert int(counter) == C0                                   # the launches only read the counter
        sides.append(dict(res=res, idxs=idxs, raws=[s[0] for s in stag]))
    ref, got = sides
    outs = [t.data_ptr() for r_ in got["res"] for t in r_]
    assert len(set(outs)) == 3 * n                                  # every batch has its own h, P and mask sum
    for i in range(n):
        assert torch.equal(ref["idxs"][i], got["idxs"][i]), ("idx", i)
        for name, r_, g_ in zip(("h", "P", "tot_m"), ref["res"][i], got["res"][i]):
            assert r_.shape == g_.shape and torch.equal(r_, g_), (name, i)
        for k, r_, g_ in zip(keys, ref["raws"][i], got["raws"][i]):
            assert torch.equal(r_, g_), (k, i)
        # and the reference itself is what the case means to exercise
        if draws[i]:
            exp = [t % N for t in range(B)] if N < B else sample_episodes_mirror(B, N, C0 + off + i, SEED)
            assert ref["idxs"][i].tolist() == exp
        else:
            assert torch.equal(ref["idxs"][i], preset)
        masks = float(ring["filled"][ref["idxs"][i], :T - 1].sum())
        assert float(ref["res"][i][2]) == masks and (masks < B * (T - 1)) == ragged
        assert torch.isfinite(ref["res"][i][0]).all() and torch.isfinite(ref["res"][i][1]).all()
    if n > 1 and N >= B and N > 1 and B > 1:
        assert len({tuple(x.tolist()) for x in ref["idxs"]}) > 1    # the batches of a launch are different draws


def test_batches_that_do_not_share_what_a_launch_shares_are_refused(agent):
    """Two batches into the same destinations, and more batches than a launch takes: MACJD_EINVAL, nothing is launched."""
    from macjd_amd import _native, ops
    a, S = agent
    B, J = 2, 2
    gen = torch.Generator(device=DEV).manual_seed(5)
    ring = _ring(J, S, False, gen)
    srcs = list(ring.values())
    n_stored = torch.tensor([NB], dtype=torch.int32, device=DEV)
    counter = torch.tensor([C0], dtype=torch.int64, device=DEV)
    _, dsts = _staging(ring, B, gen)
    idx = [torch.zeros(B, dtype=torch.int64, device=DEV) for _ in range(5)]
    with pytest.raises(_native.NativeLibraryError):
        ops.prefetch_batches(ring["obs"], [a], B, J, T + 1, (n_stored, counter, SEED), srcs,
                             [(0, True, dsts, idx[0]), (1, True, dsts, idx[1])], ring["filled"], T - 1)
    with pytest.raises(_native.NativeLibraryError):
        ops.prefetch_batches(ring["obs"], [a], B, J, T + 1, (n_stored, counter, SEED), srcs,
                             [(i, True, _staging(ring, B, gen)[1], idx[i]) for i in range(5)], ring["filled"], T - 1)
    torch.cuda.synchronize()


def _learner(monkeypatch, ahead, K, Bsz, limit, E):
    """3j/4r learner, batches of Bsz of the E stored episodes of `limit` steps from the batched runner (static observations
    and states), captured in groups of K updates."""
    from macjd_amd import options
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.scenario import Scenario, ring_scenario_dict
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    monkeypatch.setenv("MACJD_PREFETCH_AHEAD", ahead)
    options.reload()
    sc = Scenario.from_dict(ring_scenario_dict(3, 4), config=SimpleNamespace(episode_limit=limit))
    env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=5)
    info = env.get_env_info()
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=2 * E, batch_size=Bsz,
                     lr=1e-3, epsilon_start=0.5, target_update_interval=100)
    args.env_info = info
    torch.manual_seed(3)
    with quiet():
        mac = BasicMAC(info["obs_shape"], args)
        buf = EpisodeReplayBuffer(args)
        learner = QMixLearner(mac, args)
    BatchedEpisodeRunner(env, mac, buf, args).run(sync_stats=False)
    assert buf.obs_static is True and buf.state_static is True and int(buf.current_size) == E
    learner.enable_graphs(buf, Bsz, updates_per_graph=K)
    gc.collect()
    torch.cuda.empty_cache()   # every address baked into the captured launches must belong to a live tensor
    return learner, buf


@pytest.mark.parametrize("K,Bsz,limit,E,paired", [(5, 4, 8, 16, False), (4, 4, 8, 16, False), (5, 16, 24, 32, True)])
def test_group_two_updates_ahead_equals_one_update_ahead(monkeypatch, K, Bsz, limit, E, paired):
    """Two replayed groups of K pipelined updates (K - 1 even and odd; the second group reuses the staging sets the first
    one filled) with the prefetch in pairs two updates ahead and one by one: trainable weights, Adam moments and step, the
    four statistics of every update, the drawn batch and the sampler's counter — all equal bit for bit.  The small learner
    (108 Q-head rows) takes the update with the target branch on the side stream; 16 episodes of 24 steps (1200 rows) take
    the paired update of the full-size learner, whose later consumer of a launch passes no event."""
    la, ba = _learner(monkeypatch, "2", K, Bsz, limit, E)
    lb, bb = _learner(monkeypatch, "1", K, Bsz, limit, E)
    assert la._paired_heads_ok(la._g_stages[0], la._g_T) is paired
    assert la._g_pipelined and lb._g_pipelined and la._g_multi[0] == lb._g_multi[0] == K
    assert la._g_prefetch_launch is True and lb._g_prefetch_launch is True
    assert la._g_prefetch_ahead == 2 and lb._g_prefetch_ahead == 1
    assert len(la._g_stages) == 4 and len(lb._g_stages) == 2
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k
    c0 = int(la._g_draws)
    seen = set()
    for group in (1, 2):
        sa, sb = torch.zeros(K, 4, device=DEV), torch.zeros(K, 4, device=DEV)
        la.train_from_buffer_many(K, stats_out=sa)
        lb.train_from_buffer_many(K, stats_out=sb)
        torch.cuda.synchronize()
        assert la.train_step == lb.train_step == group * K
        assert torch.equal(sa, sb) and bool(torch.isfinite(sa).all())
        for i, (pa, pb) in enumerate(zip(la.params, lb.params)):
            assert torch.equal(pa, pb), i
        for name in ("_flat_exp_avg", "_flat_exp_avg_sq", "_adam_step", "_g_idx", "_g_draws"):
            assert torch.equal(getattr(la, name), getattr(lb, name)), name
        seen |= {float(x) for x in sa[:, 0]}
    assert len(seen) == 2 * K                       # every update saw its own batch and weights
    assert int(la._g_draws) - c0 >= 2 * K           # (one draw per update; a stand-alone first draw where none was pending)
    la.release_graphs()
    lb.release_graphs()
    assert la._g_prefetch_held is None and la._g_stages is None


def test_recapture_that_changes_the_number_of_staging_sets_equals_one_capture(monkeypatch):
    """A group captured with MACJD_PREFETCH_AHEAD=1 (two staging sets and index rows), released, and captured again with
    the default (four), against a learner captured once with the default: two replayed groups of K = 5 after the cache was
    emptied — weights, Adam moments and step, every update's statistics, the drawn batch and the counter bit-equal.  What
    the first group held is gone by then: a launch of the second capture that baked an address of it would read freed
    memory."""
    from macjd_amd import options
    K, Bsz, limit, E = 5, 4, 8, 16
    assert options._DEFAULTS["PREFETCH_AHEAD"] == "2"
    la, ba = _learner(monkeypatch, "1", K, Bsz, limit, E)
    assert la._g_prefetch_ahead == 1 and len(la._g_stages) == 2 and la._g_prefetch_held[0].shape[0] == 2
    la.release_graphs()
    assert la._g_multi is None and la._g_stages is None and la._g_prefetch_held is None
    monkeypatch.delenv("MACJD_PREFETCH_AHEAD")
    options.reload()
    la.enable_graphs(ba, Bsz, updates_per_graph=K)
    gc.collect()
    torch.cuda.empty_cache()
    lb, bb = _learner(monkeypatch, "2", K, Bsz, limit, E)
    for l in (la, lb):
        assert l._g_pipelined and l._g_prefetch_launch is True and l._g_prefetch_ahead == 2 and l._g_multi[0] == K
        assert len(l._g_stages) == 4 and l._g_prefetch_held[0].shape[0] == 4
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k
    seen = set()
    for group in (1, 2):
        sa, sb = torch.zeros(K, 4, device=DEV), torch.zeros(K, 4, device=DEV)
        la.train_from_buffer_many(K, stats_out=sa)
        lb.train_from_buffer_many(K, stats_out=sb)
        torch.cuda.synchronize()
        assert la.train_step == lb.train_step == group * K
        assert torch.equal(sa, sb) and bool(torch.isfinite(sa).all())
        for i, (pa, pb) in enumerate(zip(la.params, lb.params)):
            assert torch.equal(pa, pb), i
        for name in ("_flat_exp_avg", "_flat_exp_avg_sq", "_adam_step", "_g_idx", "_g_draws"):
            assert torch.equal(getattr(la, name), getattr(lb, name)), name
        seen |= {float(x) for x in sa[:, 0]}
    assert len(seen) == 2 * K                       # every update saw its own batch and weights
    la.release_graphs()
    lb.release_graphs()
