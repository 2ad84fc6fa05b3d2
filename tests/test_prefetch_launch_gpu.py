"""The one-launch prefetch (``macjd_prefetch_batch``, csrc/macjd_nets.hip ``prefetch_batch_kernel``) against the four launches
it stands for — ``sample_episodes`` + ``gather_rows`` + ``td_mask_sum`` + ``gru_sequence_from_obs(with_actor=True)`` — on
copies of the same ring, and a captured group of updates with MACJD_PREFETCH_LAUNCH = 1 against = 0.  Everything bit for
bit: the new launch runs the same device functions on the same data.

Kernel cases: B in {2, 3}, J in {2, 3}, T in {4, 12} (T + 1 = 5 and 13: both remainders of the scan's unroll by three; bool
rows of 4 and 12 bytes on the 4-byte copy path, reward rows of 16 / 48 bytes on the 16-byte path, padded action rows), N
stored in {5, 8} (with and without cycle-walking) and N = 1 < n, counter offsets 0 and 2, "no draw", three gather workgroups
(a grid-stride loop of many passes) and the default; `filled` rows end before T - 1, so the mask sum is not B (T - 1)."""
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
SEED, C0, NB = 0x5EED1234ABCD, 11, 9   # sampler seed, first counter value, ring slots


def _ring(J, T, S, gen):
    r = lambda *shape: torch.randn(*shape, generator=gen, device=DEV)
    ring = {
        "obs": r(NB, T + 1, J, S), "state": r(NB, T + 1, 7), "hidden_state": r(NB, T + 1, J, 4),
        "actions_discrete": torch.randint(0, 9, (NB, T, J, 1), generator=gen, device=DEV, dtype=torch.int32),
        "actions_continuous": r(NB, T, J, 1), "reward": r(NB, T, 1),
        "terminated": torch.zeros(NB, T, 1, dtype=torch.bool, device=DEV),
        "filled": torch.zeros(NB, T, 1, dtype=torch.bool, device=DEV),
    }
    for e in range(NB):   # episode e carries 1 + e % (T - 2) <= T - 2 steps: every row has a False inside the first T - 1
        n = 1 + e % (T - 2)
        ring["filled"][e, :n] = True
        ring["terminated"][e, n - 1] = True
    return ring


def _staging(ring, B, T, gen):
    """Staging tensors over raw byte buffers of random content (what a launch leaves untouched stays comparable): the
    action keys with T + 1 steps, like the learner's."""
    raws, dsts = [], []
    for k, v in ring.items():
        shape = (B, T + 1 if k.startswith("actions") else v.shape[1]) + tuple(v.shape[2:])
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


CASES = [  # B, J, T, N stored, offset, draw, gather workgroups (0 = default)
    (2, 2, 4, 5, 0, True, 0), (3, 3, 12, 8, 2, True, 0), (3, 2, 12, 5, 2, True, 3), (2, 3, 4, 8, 0, True, 3),
    (2, 2, 12, 1, 0, True, 0), (3, 3, 4, 1, 2, True, 0), (3, 3, 12, 8, 0, False, 0), (2, 2, 4, 5, 2, False, 3),
]


@pytest.mark.parametrize("B,J,T,N,off,draw,gblocks", CASES)
def test_one_launch_equals_the_four_launches(agent, B, J, T, N, off, draw, gblocks):
    from macjd_amd import ops
    a, S = agent
    gen = torch.Generator(device=DEV).manual_seed(100 * B + 10 * J + T)
    ring = _ring(J, T, S, gen)
    keys = list(ring)
    srcs = [ring[k] for k in keys]
    assert ops.prefetch_batch_supported([a], B, srcs)
    n_stored = torch.tensor([N], dtype=torch.int32, device=DEV)
    preset = torch.tensor([(3 * t + 1) % N for t in range(B)], dtype=torch.int64, device=DEV)
    sides = []
    for fused in (False, True):
        g2 = torch.Generator(device=DEV).manual_seed(77)
        raws, dsts = _staging(ring, B, T, g2)
        idx, nxt, scratch = preset.clone(), preset.clone(), preset.clone()
        counter = torch.tensor([C0], dtype=torch.int64, device=DEV)
        sampler = (idx, n_stored, counter, SEED)
        with torch.no_grad():
            if fused:
                hs, ps, tot = ops.prefetch_batch(ring["obs"], [a], B, J, T + 1, sampler, srcs, dsts, ring["filled"], T - 1,
                                                 offset=off, draw=draw, gather_blocks=gblocks)
                assert int(counter) == C0                                    # the launch only reads the counter
                ops.sample_episodes(nxt, n_stored, counter, SEED, offset=(off + 1) if draw else off)   # the closing draw
            else:
                for _ in range(off):                                         # the draws of the earlier prefetches
                    ops.sample_episodes(scratch, n_stored, counter, SEED)
                if draw:
                    ops.sample_episodes(idx, n_stored, counter, SEED)
                ops.gather_rows(idx, srcs, dsts)
                tot = ops.td_mask_sum(dsts[keys.index("filled")], T - 1)
                hs, ps = ops.gru_sequence_from_obs(ring["obs"], idx, [a], B, J, T + 1, with_actor=True)
                ops.sample_episodes(nxt, n_stored, counter, SEED)
        torch.cuda.synchronize()
        sides.append(dict(idx=idx, nxt=nxt, counter=counter, tot=tot, h=hs[0], P=ps[0], raws=raws))
    ref, got = sides
    want = off + (2 if draw else 1)
    assert int(ref["counter"]) == int(got["counter"]) == C0 + want
    for k in ("idx", "nxt", "tot", "h", "P"):
        assert torch.equal(ref[k], got[k]), k
    for k, r_, g_ in zip(keys, ref["raws"], got["raws"]):
        assert torch.equal(r_, g_), k
    # and the reference itself is what the case means to exercise
    if draw:
        exp = [t % N for t in range(B)] if N < B else sample_episodes_mirror(B, N, C0 + off, SEED)
        assert ref["idx"].tolist() == exp
    else:
        assert torch.equal(ref["idx"], preset)
    masks = ring["filled"][ref["idx"], :T - 1].sum()
    assert float(ref["tot"]) == float(masks) and float(masks) < B * (T - 1)
    assert torch.isfinite(ref["h"]).all() and torch.isfinite(ref["P"]).all()


def _learner(monkeypatch, switch, K):
    """3j/4r learner, batch of 4 episodes of 12 steps from the batched runner (static observations and states)."""
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.scenario import Scenario, ring_scenario_dict
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    monkeypatch.setenv("MACJD_PREFETCH_LAUNCH", switch)
    E, Bsz = 16, 4
    sc = Scenario.from_dict(ring_scenario_dict(3, 4), config=SimpleNamespace(episode_limit=12))
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
    assert buf.obs_static is True and buf.state_static is True
    learner.enable_graphs(buf, Bsz, updates_per_graph=K)
    gc.collect()
    torch.cuda.empty_cache()   # every address baked into the captured launches must belong to a live tensor
    return learner, buf


def test_group_with_the_one_launch_prefetch_equals_the_four_launches(monkeypatch):
    """A replayed group of K = 4 pipelined updates, then two single updates (the remainder path), with the switch at 1 and
    at 0: trainable weights, Adam moments and step, the four statistics of every update, the drawn batch and the sampler's
    counter — all equal bit for bit."""
    K = 4
    la, ba = _learner(monkeypatch, "1", K)
    lb, bb = _learner(monkeypatch, "0", K)
    assert la._g_pipelined and lb._g_pipelined and la._g_multi[0] == lb._g_multi[0] == K
    assert la._g_prefetch_launch is True and lb._g_prefetch_launch is False
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k

    def same(n_updates, sa, sb):
        torch.cuda.synchronize()
        assert la.train_step == lb.train_step == n_updates
        assert torch.equal(sa, sb) and bool(torch.isfinite(sa).all())
        for i, (pa, pb) in enumerate(zip(la.params, lb.params)):
            assert torch.equal(pa, pb), i
        for name in ("_flat_exp_avg", "_flat_exp_avg_sq", "_adam_step", "_g_idx", "_g_draws"):
            assert torch.equal(getattr(la, name), getattr(lb, name)), name

    c0 = int(la._g_draws)
    sa, sb = torch.zeros(K, 4, device=DEV), torch.zeros(K, 4, device=DEV)
    la.train_from_buffer_many(K, stats_out=sa)
    lb.train_from_buffer_many(K, stats_out=sb)
    same(K, sa, sb)
    assert len({float(x) for x in sa[:, 0]}) == K
    sa2, sb2 = torch.zeros(2, 4, device=DEV), torch.zeros(2, 4, device=DEV)
    la.train_from_buffer_many(2, stats_out=sa2)
    lb.train_from_buffer_many(2, stats_out=sb2)
    same(K + 2, sa2, sb2)
    assert int(la._g_draws) - c0 >= K + 2   # (one draw per update; a stand-alone first draw where none was pending)
