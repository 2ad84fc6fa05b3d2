"""The learner with MACJD_ROWS_STAGED at 1 and at 0, in the form of tests/test_wgrad_in_train_learner_gpu.py: 2 jammers /
2 radars, batch 4, 128 steps, the paired form, ONE captured group of four updates.

Switch 0 is the plain rows kernel in the reduce launch, switch 1 the staged form (blocks of 256 outputs on LDS-staged operand
rows).  Every sum keeps its order, so nothing may differ at all: the same drawn batches and launch counts, weights, both
Adam moments and the statistics rows bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_norm_in_reduce_learner_gpu as base  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = base.DEV
K = base.K


def _learner(monkeypatch, switch):
    monkeypatch.setenv("MACJD_ROWS_STAGED", switch)
    return base._learner(monkeypatch, "1", 128)   # (MACJD_NORM_IN_REDUCE and MACJD_WGRAD_IN_TRAIN at 1 on both sides)


def test_group_of_four_with_the_switch_on_and_off(monkeypatch):
    from macjd_amd import _native, ops
    from macjd_amd.core import update_group
    lib = _native.load()
    counts, flags = [], []
    capture = update_group.UpdateGroup._capture
    entry = lib.macjd_linear_wgrad_many_norm_ex

    def spy(self, body_a, pool):
        before = ops.wgrad_partial_launches
        capture(self, body_a, pool)
        counts.append(ops.wgrad_partial_launches - before)

    class SpyLib:
        """The library with the grouped launch's flags recorded."""

        def __getattr__(self, name):
            return getattr(lib, name)

        def macjd_linear_wgrad_many_norm_ex(self, arr, n, nio, fl, stream):
            flags.append(int(fl))
            return entry(arr, n, nio, fl, stream)

    monkeypatch.setattr(update_group.UpdateGroup, "_capture", spy)
    monkeypatch.setattr(_native, "load", lambda: SpyLib())
    la, ba = _learner(monkeypatch, "1")
    n_a = len(flags)
    lb, bb = _learner(monkeypatch, "0")
    monkeypatch.setattr(_native, "load", lambda: lib)
    # the same launches on both sides: no partial-products launch, the reduce launch once per update, only its flag differs
    assert counts == [0, 0], counts
    assert n_a >= K and len(flags) == 2 * n_a and set(flags[:n_a]) == {0} and set(flags[n_a:]) == {_native.WGRAD_PLAIN_ROWS}
    assert la._g_multi[0] == lb._g_multi[0] == K and la._g_pipelined and lb._g_pipelined
    assert la._g_mixer_static and lb._g_mixer_static and la._g_wgrad_in_train and lb._g_wgrad_in_train
    assert la._norm_in_reduce() and lb._norm_in_reduce()
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k
    for pa, pb in zip(la.params, lb.params):
        assert torch.equal(pa, pb)
    sa, sb = torch.zeros(K, 4, device=DEV), torch.zeros(K, 4, device=DEV)
    la.train_from_buffer_many(K, stats_out=sa)
    lb.train_from_buffer_many(K, stats_out=sb)
    torch.cuda.synchronize()
    assert torch.equal(la._g_idx, lb._g_idx) and torch.equal(la._g_draws, lb._g_draws)
    assert la.train_step == lb.train_step == K and float(la._adam_step) == float(lb._adam_step) == float(K)
    assert la.grad_pack_launches == lb.grad_pack_launches == 0
    assert bool(torch.isfinite(sa).all()) and bool(torch.isfinite(la._flat_param).all())
    assert float(la.eval_qmix_net.state_norm.bias.detach().abs().max()) > 0      # the LayerNorm parameters did train
    assert torch.equal(la._flat_param, lb._flat_param)
    assert torch.equal(la._flat_exp_avg, lb._flat_exp_avg) and torch.equal(la._flat_exp_avg_sq, lb._flat_exp_avg_sq)
    assert torch.equal(sa, sb)
