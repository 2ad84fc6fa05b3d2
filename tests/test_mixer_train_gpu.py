"""The learner update's mixers as one launch (macjd_mixer_fused_train: eval forward, target forward, TD-loss gradient,
eval mixer backward) against the launches it replaces (macjd_mixer_fused_forward_pair + macjd_mixer_fused_backward_td):
every output bitwise equal, every parameter gradient after the grouped weight-gradient pass bitwise equal, grouped updates
with MACJD_MIXER_TRAIN=1 and =0 ending on the same weights."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO  # noqa: F401

sys.path.insert(0, os.path.dirname(__file__))
from test_nets_cpu import load, make_args, quiet, sd_from  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99


def _gpu_args(d, **kw):
    return make_args(d, device="cuda", use_cuda=True, **kw)


def _mixers(tag, weights):
    from macjd_amd.core.networks import QMixer
    g, d = load(tag)
    args = _gpu_args(d)
    torch.manual_seed(5)
    me, mt = QMixer(args).to(DEV), QMixer(args).to(DEV)
    with torch.no_grad():
        if weights == "g4_saturating":   # G4's weight set x 25: every clamp saturates on most rows
            me.load_state_dict(sd_from(g, "mixer."))
            mt.load_state_dict(sd_from(g, "mixer."))
            for p_e, p_t in zip(me.parameters(), mt.parameters()):
                p_e.mul_(25.0)
                p_t.mul_(0.9 * 25.0)
        else:                            # random, spread so that every clamp has rows on both sides
            for p in list(me.parameters()) + list(mt.parameters()):
                p.mul_(3.0)
    return d, args, me, mt


def _batch(d, args, B, T1, seed):
    rng = np.random.default_rng(seed)
    f = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=DEV)
    q_e, q_t = f(B, T1, d["J"]), f(B, T1, d["J"])
    state = 3.0 * f(B, T1, args.state_shape)
    reward = f(B, T1, 1)
    lens = torch.tensor(rng.integers(2, T1 + 1, B))
    steps = torch.arange(T1).view(1, T1, 1)
    filled = (steps < lens.view(B, 1, 1)).to(DEV)
    terminated = (steps >= (lens.view(B, 1, 1) - 1)).to(DEV)
    return q_e, q_t, state, reward, terminated, filled


def _params(m):
    from macjd_amd import ops
    ln, (w_cat, b_cat) = m.state_norm, m._first_layer_cat()
    return ops._mixerf_params(ln.weight, ln.bias, ln.eps, w_cat, b_cat, m.hyper_w_1[2].weight, m.hyper_w_1[2].bias,
                              m.hyper_w_final[2].weight, m.hyper_w_final[2].bias, m.V[2].weight, m.V[2].bias)


def _raw(train, me, mt, q_e, q_t, state, reward, terminated, filled, tot_m):
    """The launches through the C-ABI; every output pre-filled with NaN."""
    from macjd_amd import _native, ops
    lib = _native.load()
    B, T1, J = q_e.shape
    M, S = B * T1, state.shape[-1]
    qe, qt, s = q_e.reshape(M, J).contiguous(), q_t.reshape(M, J).contiguous(), state.reshape(M, S).contiguous()
    pe, pt = _params(me), _params(mt)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    out = {"y": nan(M), "tq": nan(M), "sn": nan(M, S), "xhat": nan(M, S), "act": nan(M, 384), "gq": nan(M, J),
           "gout1": nan(M, 384), "g_w1raw": nan(M, J * 64), "g_wfraw": nan(M, 64), "g_v": nan(M)}
    io = ops._mixerf_io(qe, s, pe)
    io.save = 1
    for k in ("y", "sn", "xhat", "act", "gq", "gout1", "g_w1raw", "g_wfraw", "g_v"):
        setattr(io, k, out[k].data_ptr())
    tio = ops._mixerf_io(qt, s, pt)
    tio.y = out["tq"].data_ptr()
    td = _native.TdLossIO()
    td.B, td.Tm1, td.gamma = B, T1 - 1, GAMMA
    td.y, td.y_sb = out["y"].data_ptr(), T1
    td.tq, td.tq_sb = out["tq"].data_ptr() + 4, T1
    td.gy, td.gy_sb, td.gy_cols = None, T1, T1
    td.reward, td.r_sb, td.r_st = reward.data_ptr(), reward.stride(0), reward.stride(1)
    td.terminated, td.t_sb, td.t_st = terminated.data_ptr(), terminated.stride(0), terminated.stride(1)
    td.filled, td.f_sb, td.f_st = filled.data_ptr(), filled.stride(0), filled.stride(1)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if train:
        _native.check(lib.macjd_mixer_fused_train(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                                  stream), "macjd_mixer_fused_train")
    else:
        _native.check(lib.macjd_mixer_fused_forward_pair(ctypes.byref(io), ctypes.byref(tio), stream),
                      "macjd_mixer_fused_forward_pair")
        _native.check(lib.macjd_mixer_fused_backward_td(ctypes.byref(io), ctypes.byref(td), tot_m.data_ptr(), stream),
                      "macjd_mixer_fused_backward_td")
    torch.cuda.synchronize()
    return out


def _autograd(train, me, mt, q_e, q_t, state, reward, terminated, filled, tot_m):
    """The update's path (ops / networks): gradients of q and of every eval-mixer parameter after the grouped pass."""
    from macjd_amd import ops
    B, T1, _ = q_e.shape
    q = q_e.clone().requires_grad_(True)
    params = [q] + list(me.parameters())
    for p in params:
        p.grad = None
    with torch.no_grad():
        if train:
            y_t, gy = mt.forward_paired_with_next_fused(q_t, state, td=dict(reward=reward, terminated=terminated, filled=filled,
                                                                             gamma=GAMMA, Tm1=T1 - 1, tot_m=tot_m))
        else:
            y_t = mt.forward_paired_with_next_fused(q_t, state)
    y_e = me(q, state)
    ops.assert_pairs_launched()
    if not train:
        gy = ops.td_grad_in_mixer_backward(y_e, y_t, reward, terminated, filled, GAMMA, T1 - 1, 1, tot_m)
    with ops.deferred_wgrad():
        y_e.backward(gy)
    torch.cuda.synchronize()
    return [y_e.detach().clone(), y_t.reshape(-1)[1:].clone()] + [p.grad.clone() for p in params]


@pytest.mark.parametrize("tag", ["3j4r_h64", "2j2r_h128"])
@pytest.mark.parametrize("B", [32, 3])
@pytest.mark.parametrize("weights", ["random", "g4_saturating"])
def test_mixer_train_launch_equals_pair_and_backward(tag, B, weights):
    from macjd_amd import ops
    d, args, me, mt = _mixers(tag, weights)
    T1 = 101                                   # M = 3232 rows at B = 32, a ragged 303 at B = 3
    batch = _batch(d, args, B, T1, seed=B)
    tot_m = ops.td_mask_sum(batch[5], T1 - 1)
    ref = _raw(False, me, mt, *batch, tot_m)
    got = _raw(True, me, mt, *batch, tot_m)
    for k in ref:
        a, b = ref[k], got[k]
        if k == "tq":                          # row 0 is no loss row's target: the training launch does not write it
            a, b = a[1:], b[1:]
        assert not torch.isnan(b).any(), k
        assert torch.equal(a, b), k
    if weights == "random":                    # (the clamps really go both ways: the gradients are not all zero)
        assert float(ref["g_w1raw"].abs().max()) > 0 and float(ref["gout1"].abs().max()) > 0
    g_ref = _autograd(False, me, mt, *batch, tot_m)
    g_got = _autograd(True, me, mt, *batch, tot_m)
    names = ["y", "tq"] + ["q"] + [n for n, _ in me.named_parameters()]
    for n, a, b in zip(names, g_ref, g_got):
        assert torch.equal(a, b), n


def test_mixer_train_argument_checks():
    from macjd_amd import _native, ops
    d, args, me, mt = _mixers("3j4r_h64", "random")
    B, T1 = 2, 11
    q_e, q_t, state, reward, terminated, filled = _batch(d, args, B, T1, seed=1)
    tot_m = ops.td_mask_sum(filled, T1 - 1)
    lib = _native.load()
    M = B * T1
    io = ops._mixerf_io(q_e.reshape(M, -1).contiguous(), state.reshape(M, -1).contiguous(), _params(me))
    tio = ops._mixerf_io(q_t.reshape(M, -1).contiguous(), state.reshape(M, -1).contiguous(), _params(mt))
    td = _native.TdLossIO()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    # nothing set up: refused, nothing launched
    assert lib.macjd_mixer_fused_train(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(), stream) != 0


def test_unconsumed_train_block_does_not_reach_the_next_launch():
    """A pending training block whose forward raised is dropped (the update clears it in a finally; a forward that fails
    inside the launch has taken it already): the next differentiable mixer forward is the plain one."""
    from macjd_amd import ops
    d, args, me, mt = _mixers("3j4r_h64", "random")
    B, T1 = 3, 101
    q_e, q_t, state, reward, terminated, filled = _batch(d, args, B, T1, seed=4)
    tot_m = ops.td_mask_sum(filled, T1 - 1)
    td = dict(reward=reward, terminated=terminated, filled=filled, gamma=GAMMA, Tm1=T1 - 1, tot_m=tot_m)

    def plain():
        q = q_e.clone().requires_grad_(True)
        y = me(q, state)
        assert ops._PAIRED_TRAIN is None
        y.backward(torch.ones_like(y))
        return y.detach().clone(), q.grad.clone()

    y0, g0 = plain()
    # (1) the caller's forward raises before the eval mixer runs
    with pytest.raises(RuntimeError, match="eval head failed"):
        try:
            with torch.no_grad():
                mt.forward_paired_with_next_fused(q_t, state, td=td)
            raise RuntimeError("eval head failed")
        finally:
            ops.clear_pending_pairs()
    assert ops._PAIRED_TRAIN is None
    y1, g1 = plain()
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    # (2) the eval forward itself fails (rows differ from the block's): the block is gone with it
    with torch.no_grad():
        mt.forward_paired_with_next_fused(q_t, state, td=td)
    with pytest.raises(AssertionError, match="differ in rows"):
        me(q_e[:2].clone().requires_grad_(True), state[:2])
    assert ops._PAIRED_TRAIN is None
    y2, g2 = plain()
    assert torch.equal(y0, y2) and torch.equal(g0, g2)
    ops.assert_pairs_launched()


def test_grouped_updates_with_the_training_launch_equal_the_pair(monkeypatch):
    """Grouped, graph-replayed updates (pipelined, paired) with MACJD_MIXER_TRAIN=1 and =0 from the same state: the same
    weights bit for bit, the logged statistics within the TD-loss tolerance; the training launch is really taken."""
    from macjd_amd import ops, options
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    from tests_golden_helpers import synthetic_batch
    g, d = load("3j4r_h64")
    T, N, B, K, n = 100, 48, 32, 3, 6
    launched = []
    real = ops._mixer_train
    monkeypatch.setattr(ops, "_mixer_train", lambda *a: launched.append(1) or real(*a))

    def build(flag):
        monkeypatch.setenv("MACJD_MIXER_TRAIN", flag)
        options.reload()
        args = _gpu_args(d, episode_limit=T, buffer_size=N, batch_size=B, target_update_interval=200, lr=1e-3)
        with quiet():
            mac = BasicMAC(d["S"], args)
            mac.load_state(sd_from(g, "g5_agent0."))
            learner = QMixLearner(mac, args)
            buf = EpisodeReplayBuffer(args)
        learner.eval_qmix_net.load_state_dict(sd_from(g, "g5_mixer0."))
        learner._update_targets()
        full = synthetic_batch(np.random.default_rng(9), args, N, T)
        for kk, v in buf.buffers.items():
            v.copy_(torch.as_tensor(full[kk]).to(v.dtype))
        buf.current_size, buf.current_index = N, 0
        buf.episode_lengths[:] = T
        obs = buf.buffers["obs"]          # static observations (as the batched runner stores them): the pipelined, paired
        obs.copy_(obs[:, :1].expand_as(obs).clone())   # update is the one the training launch belongs to
        buf.obs_static = True
        learner.enable_graphs(buf, B, updates_per_graph=K)
        assert learner._g_pipelined
        return mac, learner

    try:
        mac0, old = build("0")
        assert not launched
        mac1, new = build("1")
        assert launched, "the grouped update did not take the training launch"
        rows = {}
        for name, lrn in (("old", old), ("new", new)):
            rows[name] = []
            for _ in range(n // K):
                rows[name] += [r.clone() for r in lrn.train_from_buffer_many(K)]
        a, b = torch.stack(rows["old"]), torch.stack(rows["new"])
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=2e-6, atol=1e-7)
        assert old.train_step == new.train_step == n
        for (k_, x), y in zip(mac0.agent.state_dict().items(), mac1.agent.state_dict().values()):
            assert torch.equal(x, y), k_
        for (k_, x), y in zip(old.eval_qmix_net.state_dict().items(), new.eval_qmix_net.state_dict().values()):
            assert torch.equal(x, y), k_
    finally:
        monkeypatch.delenv("MACJD_MIXER_TRAIN", raising=False)
        options.reload()
