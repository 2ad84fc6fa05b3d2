"""The learner with MACJD_WGRAD_IN_TRAIN at 1 and at 0, in the form of tests/test_norm_in_reduce_learner_gpu.py: 2 jammers /
2 radars, batch 4, 128 steps (4 x 129 x 2 = 1032 agent rows, the smallest batch-4 geometry on the default path), the paired
form, ONE captured group of four updates.

Switch 0 is the parent's path: Q-head grid with input rows, static mixer training launch, partial-products launch, reduce,
optimiser.  Switch 1 drops the partial-products launch: the training launch leaves the Q-head's and the LayerNorm's slots per
16-row tile and the reduce forms the mixer's five products from the compact rows.  Same schedule, hence the same drawn
batches, counters and statistics rows; every gradient is the same sum in another order.

Measured on MI355X (lr 1e-3, weights up to 0.15, i.e. ulp 1.5e-8): worst |difference| between the two switch positions after the
group: parameters 5.960e-08 (four ulp of the largest weights), exp_avg 5.588e-09, exp_avg_sq 7.276e-12, statistics rows 2.184e-07
relative — MEASURED below; asserted: FACTOR = 4 x measured (that file's margin)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_norm_in_reduce_learner_gpu as base  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = base.DEV
K = base.K
# worst difference after the replayed group of four: (parameters, exp_avg, exp_avg_sq)
MEASURED = (5.960e-08, 5.588e-09, 7.276e-12)
FACTOR = 4.0


def _learner(monkeypatch, switch):
    monkeypatch.setenv("MACJD_WGRAD_IN_TRAIN", switch)
    return base._learner(monkeypatch, "1", 128)   # (MACJD_NORM_IN_REDUCE at 1 on both sides)


def test_group_of_four_with_the_switch_on_and_off(monkeypatch):
    from macjd_amd import ops
    from macjd_amd.core import update_group
    counts = []
    capture = update_group.UpdateGroup._capture

    def spy(self, body_a, pool):
        before = ops.wgrad_partial_launches
        capture(self, body_a, pool)
        counts.append(ops.wgrad_partial_launches - before)

    monkeypatch.setattr(update_group.UpdateGroup, "_capture", spy)
    la, ba = _learner(monkeypatch, "1")
    lb, bb = _learner(monkeypatch, "0")
    # one captured group of four updates each: no partial-products launch at 1, one per update at 0
    assert counts == [0, K], counts
    assert la._g_multi[0] == lb._g_multi[0] == K and la._g_pipelined and lb._g_pipelined
    assert la._g_mixer_static and lb._g_mixer_static and la._g_wgrad_in_train and not lb._g_wgrad_in_train
    assert la._norm_in_reduce() and lb._norm_in_reduce()
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k
    for pa, pb in zip(la.params, lb.params):
        assert torch.equal(pa, pb)
    sa, sb = torch.zeros(K, 4, device=DEV), torch.zeros(K, 4, device=DEV)
    la.train_from_buffer_many(K, stats_out=sa)
    lb.train_from_buffer_many(K, stats_out=sb)
    torch.cuda.synchronize()
    # the same schedule: drawn batches and counters
    assert torch.equal(la._g_idx, lb._g_idx) and torch.equal(la._g_draws, lb._g_draws)
    assert la.train_step == lb.train_step == K and float(la._adam_step) == float(lb._adam_step) == float(K)
    assert la.grad_pack_launches == lb.grad_pack_launches == 0
    assert bool(torch.isfinite(sa).all()) and bool(torch.isfinite(sb).all())
    rel = float(((sa - sb).abs() / sb.abs().clamp_min(1e-30)).max())
    diff = lambda a, b: float((a.detach().double() - b.detach().double()).abs().max())
    d = (diff(la._flat_param, lb._flat_param), diff(la._flat_exp_avg, lb._flat_exp_avg), diff(la._flat_exp_avg_sq, lb._flat_exp_avg_sq))
    print(f"group of {K}: worst difference parameters {d[0]:.3e}, exp_avg {d[1]:.3e}, exp_avg_sq {d[2]:.3e}; "
          f"statistics rows: worst relative difference {rel:.3e}")
    assert float(la.eval_qmix_net.state_norm.bias.detach().abs().max()) > 0      # the LayerNorm parameters did train
    for dval, m in zip(d, MEASURED):
        assert dval <= FACTOR * m, (d, MEASURED)
    assert rel <= 4.5e-5   # (the bar of tests/test_norm_in_reduce_learner_gpu.py for an update's statistics)
