"""The learner with MACJD_NORM_IN_REDUCE at 1 and at 0: one eager update and one captured group of four, 2 jammers / 2
radars, batch 4.

Two episode lengths, both multiples of 4 (the one-launch gather of the captured update copies whole 4-byte words of the bool
rows).  With 8 steps the taken-action Q-head has 72 rows, below the 1024 its one-launch form (and with it the split-K weight
gradients of the Q-head) needs: stock autograd produces those gradients, the grouped launch pair does NOT write every
gradient of the flat vector, and ``ops.norm_in_reduce_plan`` has to keep the three-launch tail — both switch positions then
run the same launches and agree bit for bit.  With 128 steps (4 x 129 x 2 = 1032 rows, the smallest batch-4 geometry on the
default path) the pair forms the LayerNorm gradients and the squared norm, and the runs differ in the summation order of
those 2 x S + 1 numbers only.

Measured on MI355X (lr 1e-3, weights up to 0.15, i.e. ulp 1.5e-8): 1.967e-08 after the eager update, 2.235e-08 after the group
(statistics: 3.9e-6 relative) — MEASURED below; asserted: FACTOR = 4 x measured."""
import gc
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_nets_cpu import make_args, quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K = 4
# worst |parameter difference| between the two switch positions after (one eager update, then a replayed group of four)
MEASURED = {8: (0.0, 0.0), 128: (1.967e-08, 2.235e-08)}
FACTOR = 4.0


def _learner(monkeypatch, switch, limit):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.scenario import Scenario, ring_scenario_dict
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    monkeypatch.setenv("MACJD_NORM_IN_REDUCE", switch)
    E, Bsz = 8, 4
    sc = Scenario.from_dict(ring_scenario_dict(2, 2), config=SimpleNamespace(episode_limit=limit))
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
    learner.enable_graphs(buf, Bsz, updates_per_graph=K)
    gc.collect()
    torch.cuda.empty_cache()   # every address baked into the captured launches must belong to a live tensor
    return learner, buf


@pytest.mark.parametrize("limit,taken", [(8, False), (128, True)])
def test_learner_update_with_the_switch_on_and_off(monkeypatch, limit, taken):
    from macjd_amd import ops
    from macjd_amd.core.qmix import QMixLearner
    plans = []
    plan = ops.norm_in_reduce_plan

    def spy(ios, lns, cover):
        q = plan(ios, lns, cover)
        plans.append((q, len(ios), len(lns), [(io.M, io.N, bool(io.db)) for io in ios]))
        return q

    monkeypatch.setattr(ops, "norm_in_reduce_plan", spy)
    la, ba = _learner(monkeypatch, "1", limit)
    assert la._norm_in_reduce() and (plans or not taken)
    asked = len(plans)
    lb, bb = _learner(monkeypatch, "0", limit)
    assert not lb._norm_in_reduce() and len(plans) == asked      # switch at 0: the question is not even asked
    assert all((q is not None) == taken for q, *_ in plans), plans
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k
    for pa, pb in zip(la.params, lb.params):
        assert torch.equal(pa, pb)

    def worst():
        torch.cuda.synchronize()
        return max(float((pa.detach().double() - pb.detach().double()).abs().max()) for pa, pb in zip(la.params, lb.params))

    # eager: the captured body and the optimiser step, issued directly
    for learner, switch in ((la, "1"), (lb, "0")):
        monkeypatch.setenv("MACJD_NORM_IN_REDUCE", switch)
        step0 = float(learner._adam_step)
        learner._graph_body_a()
        assert (learner._norm_partials is not None) == (taken and switch == "1")
        assert not (learner._norm_partials is not None and learner._held_ln)   # the LayerNorm launch: in the pair, not held as well
        learner._clip_and_step()
        torch.cuda.synchronize()
        assert float(learner._adam_step) == step0 + 1
        assert learner._norm_partials is None and learner._held_ln is None
    d_eager = worst()
    print(f"limit {limit}: eager update: worst parameter difference {d_eager:.3e}, "
          f"grad_norm {float(la._grad_norm)!r} vs {float(lb._grad_norm)!r}")
    sa, sb = torch.zeros(K, 4, device=DEV), torch.zeros(K, 4, device=DEV)
    la.train_from_buffer_many(K, stats_out=sa)
    lb.train_from_buffer_many(K, stats_out=sb)
    d_group = worst()
    rel = float(((sa - sb).abs() / sb.abs().clamp_min(1e-30)).max())
    print(f"limit {limit}: group of {K}: worst parameter difference {d_group:.3e}, worst relative statistics difference {rel:.3e}")
    assert la.train_step == lb.train_step == K
    assert bool(torch.isfinite(sa).all()) and float(la._adam_step) == float(lb._adam_step)
    assert la.grad_pack_launches == lb.grad_pack_launches and (la.grad_pack_launches == 0 or not taken)
    assert float(la.eval_qmix_net.state_norm.bias.detach().abs().max()) > 0      # the LayerNorm parameters did train
    if not taken:
        assert d_eager == d_group == 0.0 and torch.equal(sa, sb)
    else:
        assert la._g_multi[0] == lb._g_multi[0] == K
        for dval, m in zip((d_eager, d_group), MEASURED[limit]):
            assert dval <= FACTOR * m
        assert rel <= 4.5e-5   # what the statistics of an update were accepted at when the LayerNorm launch last moved
    # with ranks the all-reduce sits between the reduce and the norm: the old path is kept
    monkeypatch.setenv("MACJD_NORM_IN_REDUCE", "1")
    assert la._norm_in_reduce()
    monkeypatch.setattr(QMixLearner, "_world_size", staticmethod(lambda: 2))
    assert not la._norm_in_reduce()
