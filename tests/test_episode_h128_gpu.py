"""Whole-episode agent launch (agent_episode_kernel<128, J, A>) and one-launch Double-DQN (qhead_double_q_kernel<128, A>) at
the reference's default GRU hidden size 128: the kernel alone against stock torch ops, the runner's fused rollout
against its step-by-step rollout, the Double-DQN launch against the NumPy oracle, and the MACJD_QHEAD_DOUBLE_Q switch.

Measured on an MI355X (the bars below are the H = 64 tests' bars; K doubles here): max |hidden - GRUCell| 2.4e-7 over all
cases of the kernel test (bar 2e-5), every greedy choice the masked maximum; fused against step-by-step rollout 2.4e-7 on
the hidden states with all actions equal; Double-DQN values within 1.2e-7 of the oracle."""
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO, load_scenario

sys.path.insert(0, os.path.join(REPO, "oracle"))
import nets_oracle  # noqa: E402

from test_nets_cpu import load, make_args, quiet, sd_from  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"
H = 128


def _gpu_args(d, **kw):
    return make_args(d, device="cuda", use_cuda=True, **kw)


def _agent(J, A, S=24, seed=0):
    from macjd_amd.core.networks import RNNAgent
    torch.manual_seed(seed)
    with quiet():
        a = RNNAgent(S, _gpu_args(dict(J=J, A=A, S=S, H=H))).to(DEV)
    with torch.no_grad():   # spread the Q-values: fewer near-ties between the two summation orders
        for p_ in a.fc2_q_head.parameters():
            p_.mul_(3.0)
    return a


@pytest.mark.parametrize("E", [1, 37])
@pytest.mark.parametrize("J,A", [(2, 5), (3, 9)])
def test_agent_episode_kernel_h128_vs_torch(J, A, E):
    """ops.agent_episode alone (per-row gi and P, non-zero h0, a mask with actions off; E = 1: fewer rows than a tile,
    E = 37: three workgroups, the last one ragged) against torch.nn.GRUCell and the RNNAgent Q-head expressions along the
    stored trajectory; exploration draws against ops.qhead_select for the same (row, counter) pairs."""
    from macjd_amd import ops
    assert ops.agent_episode_supported(J, H, A)
    T, N = 5, E * J
    a = _agent(J, A)
    l1, l2 = a.fc2_q_head[0], a.fc2_q_head[2]
    gen = torch.Generator().manual_seed(100 * E + A)
    x = torch.randn(N, H, generator=gen).to(DEV)                       # the GRU cell's input rows (fc1's output)
    P_all = torch.rand(N, A, generator=gen).to(DEV)
    h0 = (0.5 * torch.randn(N, H, generator=gen)).to(DEV)
    avail = (torch.rand(E, J, A, generator=gen) < 0.7).to(torch.int64)
    avail[..., 1] |= (avail.sum(-1) == 0).to(torch.int64)
    avail = avail.to(DEV)
    assert int(avail.sum()) < avail.numel()
    with torch.no_grad():
        gi = torch.nn.functional.linear(x, a.rnn.weight_ih, a.rnn.bias_ih)
    assert gi.stride(0) == 3 * H and P_all.stride(0) == A
    eps = torch.ones(T, dtype=torch.float32, device=DEV)
    ctr = torch.tensor([1000], dtype=torch.int64, device=DEV)
    seed = 77

    def launch(greedy):
        hid = torch.full((T, E, J, H), float("nan"), device=DEV)
        T_out = torch.full((T, E, J), -1, dtype=torch.int32, device=DEV)
        P_out = torch.full((T, E, J), float("nan"), device=DEV)
        h_fin = torch.full((N, H), float("nan"), device=DEV)
        ops.agent_episode(gi, P_all, h0, a.rnn.weight_hh, a.rnn.bias_hh, l1.weight, l1.bias, l2.weight, l2.bias, E, J, T,
                          avail, eps, greedy, seed, ctr, hid, T_out, P_out, h_final=h_fin)
        torch.cuda.synchronize()
        return hid, T_out, P_out, h_fin

    def q_all(h):   # RNNAgent's Q-head for every action, stock torch ops: w2 . ReLU(W1 [h, onehot(a), P_a] + b1) + b2
        W1 = l1.weight
        pre = (torch.nn.functional.linear(h, W1[:, :H], l1.bias)[:, None, :] + W1[:, H:H + A].t()[None]
               + P_all[:, :, None] * W1[:, H + A][None, None, :])
        return torch.relu(pre) @ l2.weight.view(-1) + l2.bias

    av = avail.view(N, A) != 0
    rows = torch.arange(N, device=DEV)
    # ---- greedy ----
    hid, T_out, P_out, h_fin = launch(True)
    worst_h, worst_gap = 0.0, 0.0
    with torch.no_grad():
        h = h0
        for t in range(T):
            h_ref = a.rnn(x, h)
            got = hid[t].reshape(N, H)
            worst_h = max(worst_h, float((got - h_ref).abs().max()))
            h = got                                                     # follow the stored trajectory
            q = q_all(h)
            ch = T_out[t].reshape(N).long()
            assert bool(((ch >= 0) & (ch < A)).all()) and bool(av[rows, ch].all())
            qm = q.masked_fill(~av, float("-inf"))
            gap = qm.max(dim=1).values - qm[rows, ch]
            bar = 1e-5 * max(1.0, float(q.abs().max()))
            worst_gap = max(worst_gap, float(gap.max()) / bar)
            assert torch.equal(P_out[t].reshape(N), P_all[rows, ch])   # bit for bit
    print(f"[h128 episode J={J} A={A} E={E}] max |hidden - GRUCell| = {worst_h:.3e}, worst gap / bar = {worst_gap:.3f}")
    assert worst_h <= 2e-5, worst_h
    assert worst_gap <= 1.0, worst_gap
    assert torch.equal(h_fin, hid[T - 1].reshape(N, H))
    # ---- exploration (eps = 1: every row draws) ----
    hid_x, T_x, P_x, h_fin_x = launch(False)
    assert torch.equal(hid_x, hid) and torch.equal(h_fin_x, h_fin)     # the hidden trajectory does not depend on the actions
    with torch.no_grad():
        for t in range(T):
            base = torch.nn.functional.linear(hid_x[t].reshape(N, H), l1.weight[:, :H], l1.bias)
            T64, P_sel, _, _ = ops.qhead_select(base, P_all, l1.weight, l2.weight, l2.bias, H, A, J, avail, epsilon=1.0,
                                                greedy_only=False, seed=seed, counter=1000 + t + 1)
            ch = T_x[t].reshape(N).long()
            assert torch.equal(ch, T64.reshape(N)), t
            assert bool(av[rows, ch].all())
            assert torch.equal(P_x[t].reshape(N), P_all[rows, ch])
    assert not torch.equal(T_x, T_out)


def test_fused_rollout_h128_vs_step_by_step():
    """The runner at the reference's default size (2j/2r shipped scenario, H = 128): the fused rollout is available, and
    two episode batches equal the step-by-step rollout's as at H = 64 (test_fused_episode_rollout_vs_step_by_step); a
    graph-replayed batch equals the eager fused batch bit for bit."""
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    sc, _ = load_scenario("2j2r_shipped")
    E = 200   # not a multiple of 16: the last workgroup is ragged

    def build(fused):
        env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=5)
        info = env.get_env_info()
        d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=H)
        args = _gpu_args(d, episode_limit=info["episode_limit"], buffer_size=2 * E, epsilon_start=0.3, epsilon_anneal_time=500)
        args.env_info = info
        torch.manual_seed(3)
        with quiet():
            mac = BasicMAC(info["obs_shape"], args)
            with torch.no_grad():
                for p_ in mac.agent.fc2_q_head.parameters():
                    p_.mul_(3.0)
            mac.cuda()
            buf = EpisodeReplayBuffer(args)
        r = BatchedEpisodeRunner(env, mac, buf, args)
        r.fused_rollout = fused
        assert r.fused_rollout_available() == fused
        return r, buf, mac

    rf, bf, mf = build(True)
    rs, bs, ms = build(False)
    rg, bg, mg = build(True)
    rg.enable_graph()
    keys = ("hidden_state", "actions_discrete", "actions_continuous", "reward", "terminated")
    first = None
    for ep in range(2):
        rf.run(sync_stats=True)
        rs.run(sync_stats=True)
        if ep == 0:
            first = {k: rf.stage[k].clone() for k in keys}
    rg.run(sync_stats=True)
    for k in keys:
        assert torch.equal(rg.stage[k], first[k]), k
    assert rf.t_env == rs.t_env == 200 and mf.action_selector.epsilon == pytest.approx(ms.action_selector.epsilon)
    B = {k: (bf.buffers[k], bs.buffers[k]) for k in bf.buffers}
    dh = float((B["hidden_state"][0] - B["hidden_state"][1]).abs().max())
    same = (B["actions_discrete"][0] == B["actions_discrete"][1])                    # [N, T, J, 1]
    print(f"[h128 rollout] max |hidden fused - stepwise| = {dh:.3e}, action agreement = {float(same.float().mean()):.5f}")
    assert dh <= 2e-5, dh
    assert float(same.float().mean()) > 0.995
    agree = same.all(dim=2).squeeze(-1)                                              # [N, T]: all agents agree
    pa, pb = B["actions_continuous"]
    assert torch.equal(pa[same], pb[same])
    assert float((B["reward"][0].squeeze(-1)[agree] - B["reward"][1].squeeze(-1)[agree]).abs().max()) <= 1e-5
    assert torch.equal(B["terminated"][0], B["terminated"][1]) and torch.equal(B["filled"][0], B["filled"][1])
    for k in ("state", "obs", "avail_actions"):
        assert torch.equal(*B[k]), k
    assert torch.allclose(mf.hidden_states, ms.hidden_states, atol=2e-5)


@pytest.fixture
def dq_h128_on(monkeypatch):
    """The one-launch Double-DQN form at H = 128 is behind a default-off switch (slower inside the update)."""
    from macjd_amd import options
    monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q", raising=False)
    monkeypatch.setenv("MACJD_QHEAD_DOUBLE_Q_H128", "1")
    options.reload()
    yield
    monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q_H128", raising=False)
    options.reload()


@pytest.mark.parametrize("N", [37, 1030])
def test_double_q_from_hidden_states_kernel_h128(N, dq_h128_on):
    """qhead_double_q_kernel<128, 5> against the NumPy oracle's per-action loop: the assertions of
    test_double_q_from_hidden_states_kernel at the 2j2r_h128 fixture's weights."""
    from macjd_amd import ops
    from macjd_amd.core.networks import RNNAgent
    g, d = load("2j2r_h128")
    assert d["H"] == H and d["A"] == 5
    A = d["A"]
    args = _gpu_args(d)
    torch.manual_seed(1)
    with quiet():
        ae, at = RNNAgent(d["S"], args).to(DEV), RNNAgent(d["S"], args).to(DEV)
    ae.load_state_dict(sd_from(g, "agent."))
    rng = np.random.default_rng(N)
    h_e = torch.tensor(0.7 * rng.standard_normal((N, H)), dtype=torch.float32, device=DEV)
    h_t = torch.tensor(0.7 * rng.standard_normal((N, H)), dtype=torch.float32, device=DEV)
    P_e = torch.tensor(rng.random((N, A)), dtype=torch.float32, device=DEV)
    P_t = torch.tensor(rng.random((N, A)), dtype=torch.float32, device=DEV)
    heads = [(a.fc2_q_head[0].weight, a.fc2_q_head[0].bias, a.fc2_q_head[2].weight, a.fc2_q_head[2].bias) for a in (ae, at)]
    assert ops.qhead_double_q_fused_supported(h_e, H, A)
    with torch.no_grad():
        out, am = ops.qhead_double_q_from_h(h_e, P_e, heads[0], h_t, P_t, heads[1], H, A, want_argmax=True)
        same, am2 = ops.qhead_double_q_from_h(h_e, P_e, heads[0], h_e, P_e, heads[0], H, A, want_argmax=True)   # shared inputs
    sd_e = {k: v.cpu().numpy() for k, v in ae.state_dict().items()}
    sd_t = {k: v.cpu().numpy() for k, v in at.state_dict().items()}
    q_e = nets_oracle.q_all_actions(sd_e, h_e.cpu().numpy(), P_e.cpu().numpy())
    q_t = nets_oracle.q_all_actions(sd_t, h_t.cpu().numpy(), P_t.cpu().numpy())
    am_ref = q_e.argmax(axis=1)
    am_np = am.cpu().numpy()
    assert ((am_np >= 0) & (am_np < A)).all()
    tie = np.take_along_axis(q_e, am_ref[:, None], 1)[:, 0] - np.take_along_axis(q_e, am_np[:, None], 1)[:, 0]
    err = float(np.abs(out.cpu().numpy() - np.take_along_axis(q_t, am_np[:, None], 1)[:, 0]).max())
    print(f"[h128 double-q N={N}] max value error = {err:.3e}, max tie = {float(tie.max()):.3e}, "
          f"arg-max agreement = {(am_np == am_ref).mean():.5f}")
    assert (tie <= 1e-5).all()
    if N >= 1000:
        assert (am_np == am_ref).mean() > 0.999
    np.testing.assert_allclose(out.cpu().numpy(), np.take_along_axis(q_t, am_np[:, None], 1)[:, 0], atol=TOL, rtol=0)
    np.testing.assert_allclose(same.cpu().numpy(), q_e.max(axis=1), atol=TOL, rtol=0)
    assert torch.equal(am2, am)
    # one actor row per sequence (static observation): row n = (b, t, j) reads P[b, j]
    J, T1 = d["J"], 5
    Bn = N // (T1 * J)
    if Bn:
        n = Bn * T1 * J
        Pe_s, Pt_s = P_e[:Bn * J].contiguous(), P_t[:Bn * J].contiguous()
        ex = lambda p_: p_.view(Bn, 1, J, A).expand(Bn, T1, J, A).reshape(n, A).contiguous()
        with torch.no_grad():
            a_map = ops.qhead_double_q_from_h(h_e[:n], Pe_s, heads[0], h_t[:n], Pt_s, heads[1], H, A, p_row_map=(T1 * J, J))
            a_exp = ops.qhead_double_q_from_h(h_e[:n], ex(Pe_s), heads[0], h_t[:n], ex(Pt_s), heads[1], H, A)
        assert torch.equal(a_map, a_exp)


def test_double_q_switch_selects_the_two_launch_form(monkeypatch):
    """MACJD_QHEAD_DOUBLE_Q=0: the one-launch form is off at both hidden sizes, and a learner update at 2j2r_h128
    (B = 4, T = 12: the G5 batch) on library bases + two Q-head launches gives the statistics and the flat gradient of the
    one-launch form at the G5 tolerances of test_other_baseline_configs_end_to_end.  (At H = 128 "on" also needs
    MACJD_QHEAD_DOUBLE_Q_H128=1: by default that size keeps the two-launch form, which measured faster inside the update.)"""
    from macjd_amd import ops, options
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    g, d = load("2j2r_h128")
    batch = {k[len("g5_b0_"):]: g[k] for k in g.files if k.startswith("g5_b0_")}
    batch["max_seq_len"] = int(batch["max_seq_len"])
    probe = torch.zeros(4, d["S"], device=DEV)

    def update():
        with quiet():
            mac = BasicMAC(d["S"], _gpu_args(d))
            mac.load_state(sd_from(g, "g5_agent0."))
            learner = QMixLearner(mac, _gpu_args(d))
        learner.eval_qmix_net.load_state_dict(sd_from(g, "g5_mixer0."))
        learner._update_targets()
        st = learner.train(dict(batch), {})
        return st, learner._flat_grad.clone()

    monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q", raising=False)
    monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q_H128", raising=False)
    options.reload()
    try:
        assert not ops.qhead_double_q_fused_supported(probe, 128, 5) and ops.qhead_double_q_fused_supported(probe, 64, 9)
        monkeypatch.setenv("MACJD_QHEAD_DOUBLE_Q_H128", "1")
        options.reload()
        assert ops.qhead_double_q_fused_supported(probe, 128, 5) and ops.qhead_double_q_fused_supported(probe, 64, 9)
        st_on, g_on = update()
        monkeypatch.setenv("MACJD_QHEAD_DOUBLE_Q", "0")
        options.reload()
        assert not ops.qhead_double_q_fused_supported(probe, 128, 5)
        assert not ops.qhead_double_q_fused_supported(probe, 64, 9)
        st_off, g_off = update()
    finally:
        monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q", raising=False)
        monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q_H128", raising=False)
        options.reload()
    assert ops.qhead_double_q_fused_supported(probe, 64, 9) and not ops.qhead_double_q_fused_supported(probe, 128, 5)
    for k in ("loss", "grad_norm", "eval_qtot_avg", "target_qtot_avg"):
        assert st_off[k] == pytest.approx(st_on[k], rel=1e-4, abs=TOL), k
    scale = float(g_on.abs().max())
    assert scale > 0.0
    np.testing.assert_allclose(g_off.cpu().numpy(), g_on.cpu().numpy(), rtol=1e-4, atol=2e-5 * max(scale, 1e-12))
