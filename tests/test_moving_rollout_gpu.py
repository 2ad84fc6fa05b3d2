"""Whole-episode rollout of moving scenarios on the GPU: the episode kernel with per-step inputs
(macjd_agent_episode_seq) bit for bit against the static launch run one step at a time, its degenerate strides and
refusals, and the runner's three-launch path (BatchedEpisodeRunner.rollout_moving) against the step loop, eagerly and
from a HIP graph.

Measured on an MI355X: the kernel cases are bit-equal (no tolerance applies); runner against step loop max |hidden
difference| 0.0 (bar 2e-5; max |h| 1.0, mean 0.52: most gates of this scenario sit saturated), all actions equal (bar
99.5 %)."""
import os

import pytest
import torch

import motion_cases as cases
from _harness import REPO
from test_nets_cpu import make_args, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
SEED = 77
CTR = 1000


def _weights(J, A, H, seed=0):
    from macjd_amd.core.networks import RNNAgent
    torch.manual_seed(seed)
    with quiet():
        a = RNNAgent(24, make_args(dict(J=J, A=A, S=24, H=H), device="cuda", use_cuda=True)).to(DEV)
    with torch.no_grad():
        for p_ in a.fc2_q_head.parameters():
            p_.mul_(3.0)
    l1, l2 = a.fc2_q_head[0], a.fc2_q_head[2]
    return (a.rnn.weight_hh, a.rnn.bias_hh, l1.weight, l1.bias, l2.weight, l2.bias)


class _Out:
    """The four outputs of an episode launch inside NaN / -1 filled buffers with a margin of one row on either side."""

    def __init__(self, T, E, J, H):
        N = E * J
        self.bufs = (torch.full(((T * N + 2), H), float("nan"), device=DEV), torch.full((T * N + 2,), -1, dtype=torch.int32, device=DEV),
                     torch.full((T * N + 2,), float("nan"), device=DEV), torch.full((N + 2, H), float("nan"), device=DEV))
        hb, tb, pb, fb = self.bufs
        self.hidden, self.T_out, self.P_out = hb[1:-1].view(T, E, J, H), tb[1:-1].view(T, E, J), pb[1:-1].view(T, E, J)
        self.h_final = fb[1:-1]

    def tensors(self):
        return self.hidden, self.T_out, self.P_out, self.h_final

    def margins_untouched(self):
        hb, tb, pb, fb = self.bufs
        return (bool(torch.isnan(hb[0]).all()) and bool(torch.isnan(hb[-1]).all()) and int(tb[0]) == -1 and int(tb[-1]) == -1
                and bool(torch.isnan(pb[0])) and bool(torch.isnan(pb[-1])) and bool(torch.isnan(fb[0]).all())
                and bool(torch.isnan(fb[-1]).all()))

    def all_untouched(self):
        hb, tb, pb, fb = self.bufs
        return bool(torch.isnan(hb).all()) and bool((tb == -1).all()) and bool(torch.isnan(pb).all()) and bool(torch.isnan(fb).all())


def _mask(E, J, A, gen):
    avail = (torch.rand(E, J, A, generator=gen) < 0.7).to(torch.int64)
    avail[..., 1] |= (avail.sum(-1) == 0).to(torch.int64)
    assert int(avail.sum()) < avail.numel()
    return avail.to(DEV)


def _inputs(T, rows, H, A, pad, gen):
    """gi [T, rows, 3H] and P_all [T, rows, A], different at every row and step; ``pad``: row and time strides larger than
    the row / the row block (views of wider storage)."""
    if pad:
        gi = torch.randn(T, rows + 2, 3 * H + 8, generator=gen).to(DEV)[:, :rows, :3 * H]
        P = torch.rand(T, rows + 3, A + 3, generator=gen).to(DEV)[:, :rows, :A]
        assert gi.stride() == ((rows + 2) * (3 * H + 8), 3 * H + 8, 1) and P.stride() == ((rows + 3) * (A + 3), A + 3, 1)
    else:
        gi = torch.randn(T, rows, 3 * H, generator=gen).to(DEV)
        P = torch.rand(T, rows, A, generator=gen).to(DEV)
        assert gi.stride() == (rows * 3 * H, 3 * H, 1) and P.stride() == (rows * A, A, 1)
    return gi, P


def _step_by_step(ops, gi, P, h0, W, E, J, T, avail, eps, greedy, ctr):
    """The reference of the issue: T launches of the static macjd_agent_episode with T = 1 — launch t on gi[t], P_all[t],
    h0 = the previous launch's h_final, eps pointing at element t, counter_base + t."""
    N, H = E * J, W[0].shape[1]
    hid, To, Po = [], [], []
    h = h0
    for t in range(T):
        g_t, p_t = gi[t], P[t]
        if g_t.shape[0] == 1:      # the shared form: one row for all rows (row stride 0)
            g_t, p_t = g_t.expand(N, -1), p_t.expand(N, -1)
        o = _Out(1, E, J, H)
        ops.agent_episode(g_t, p_t, h, *W, E, J, 1, avail, eps[t:t + 1], greedy, SEED, ctr + t, *o.tensors())
        assert o.margins_untouched()
        h = o.h_final
        hid.append(o.hidden[0]); To.append(o.T_out[0]); Po.append(o.P_out[0])
    return torch.stack(hid), torch.stack(To), torch.stack(Po), h


@pytest.mark.parametrize("E", [1, 17, 33])
@pytest.mark.parametrize("J,A,H", [(3, 9, 64), (2, 5, 64), (6, 17, 64), (3, 9, 128)])
def test_seq_kernel_equals_static_kernel_step_by_step_bitwise(J, A, H, E):
    """Per step the launch with per-step inputs runs the static kernel's code on the same values, so hidden, T_out, P_out
    and h_final are torch.equal to T single-step static launches: no tolerance.  E = 1: one ragged tile; 17: two
    workgroups; 33: three, the last ragged.  Per-row and shared inputs, contiguous and padded strides, eps = 0.3 and
    greedy_only, a mask with actions off, NaN margins around every output."""
    from macjd_amd import ops
    assert ops.agent_episode_seq_supported(J, H, A)
    N = E * J
    W = _weights(J, A, H)
    gen = torch.Generator().manual_seed(1000 * E + 10 * A + H)
    avail = _mask(E, J, A, gen)
    h0 = (0.5 * torch.randn(N, H, generator=gen)).to(DEV)
    ctr = torch.tensor([CTR], dtype=torch.int64, device=DEV)
    explored = 0
    for T in (1, 2, 5):
        eps = torch.full((T,), 0.3, dtype=torch.float32, device=DEV)
        for rows in (N, 1):
            for pad in (False, True):
                gi, P = _inputs(T, rows, H, A, pad, gen)
                for greedy in (False, True):
                    o = _Out(T, E, J, H)
                    ops.agent_episode_seq(gi, P, h0, *W, E, J, T, avail, eps, greedy, SEED, ctr, *o.tensors())
                    torch.cuda.synchronize()
                    assert o.margins_untouched(), (T, rows, pad, greedy)
                    ref = _step_by_step(ops, gi, P, h0, W, E, J, T, avail, eps, greedy, ctr)
                    for name, got, want in zip(("hidden", "T_out", "P_out", "h_final"), o.tensors(), ref):
                        assert torch.equal(got, want), (name, T, rows, pad, greedy)
                    ch = o.T_out.reshape(T, N).long()
                    assert bool((avail.view(1, N, A).expand(T, -1, -1).gather(2, ch.unsqueeze(-1)) != 0).all())
                    if not greedy and rows == N and not pad:
                        g = _Out(T, E, J, H)
                        ops.agent_episode_seq(gi, P, h0, *W, E, J, T, avail, eps, True, SEED, ctr, *g.tensors())
                        explored += int((g.T_out != o.T_out).sum())
    if E > 1:
        assert explored > 0   # eps = 0.3 did draw: the exploration branch ran


def test_zero_time_strides_equal_the_static_launch():
    """gi_lt = p_lt = 0 (the same row block at every step) is defined to equal macjd_agent_episode: bit for bit."""
    from macjd_amd import ops
    J, A, H, E, T = 3, 9, 64, 33, 5
    N = E * J
    W = _weights(J, A, H)
    gen = torch.Generator().manual_seed(5)
    avail = _mask(E, J, A, gen)
    h0 = (0.5 * torch.randn(N, H, generator=gen)).to(DEV)
    gi, P = _inputs(1, N, H, A, False, gen)
    eps = torch.full((T,), 0.3, dtype=torch.float32, device=DEV)
    ctr = torch.tensor([CTR], dtype=torch.int64, device=DEV)
    gi_seq, P_seq = gi.expand(T, -1, -1), P.expand(T, -1, -1)
    assert gi_seq.stride(0) == 0 and P_seq.stride(0) == 0
    for greedy in (False, True):
        a, b = _Out(T, E, J, H), _Out(T, E, J, H)
        ops.agent_episode_seq(gi_seq, P_seq, h0, *W, E, J, T, avail, eps, greedy, SEED, ctr, *a.tensors())
        ops.agent_episode(gi[0], P[0], h0, *W, E, J, T, avail, eps, greedy, SEED, ctr, *b.tensors())
        torch.cuda.synchronize()
        for x, y in zip(a.tensors(), b.tensors()):
            assert torch.equal(x, y)
        assert a.margins_untouched() and b.margins_untouched()


def test_refusals_launch_nothing():
    """A time stride between 1 and the row width, and an unsupported size, return their error code with a message and
    leave the outputs as they were."""
    from macjd_amd import _native, ops
    J, A, H, E, T = 3, 9, 64, 4, 3
    N = E * J
    W = _weights(J, A, H)
    gen = torch.Generator().manual_seed(9)
    gi, P = _inputs(T, N, H, A, False, gen)
    eps = torch.full((T,), 0.3, dtype=torch.float32, device=DEV)
    ctr = torch.tensor([CTR], dtype=torch.int64, device=DEV)

    def refused(gi_, P_, W_, J_, code, text):
        o = _Out(T, E, J_, H)
        with pytest.raises(_native.NativeLibraryError, match=rf"macjd_agent_episode_seq failed \({code}\): .*{text}"):
            ops.agent_episode_seq(gi_, P_, None, *W_, E, J_, T, None, eps, False, SEED, ctr, *o.tensors())
        torch.cuda.synchronize()
        assert o.all_untouched()

    for lt in (1, 3 * H // 2, 3 * H - 1):     # the shared form, so that the overlapping view stays inside the storage
        refused(gi.as_strided((T, 1, 3 * H), (lt, 3 * H, 1)), P[:, :1], W, J, -1, "time stride")
    for lt in (1, A // 2, A - 1):
        refused(gi[:, :1], P.as_strided((T, 1, A), (lt, A, 1)), W, J, -1, "time stride")
    # (2, 9) at H = 64 is a size of the static launch, not of this one; so is the four-tile form of 4 agents
    for J_ in (2, 4):
        assert ops.agent_episode_supported(J_, H, A) and not ops.agent_episode_seq_supported(J_, H, A)
        refused(gi[:, :1], P[:, :1], W, J_, -4, "unsupported")


# ---------------------------------------------------------------------------------------------------------------
# the runner
E_RUN, T_RUN = 40, 12


def _runner(sc, E=E_RUN, seed=5, H=64, mac_on_gpu=True):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=seed)
    info = env.get_env_info()
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=H)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=2 * E,
                     epsilon_start=0.3, epsilon_anneal_time=500)
    args.env_info = info
    torch.manual_seed(3)
    with quiet():
        mac = BasicMAC(info["obs_shape"], args)
        with torch.no_grad():   # spread the Q-values: fewer near-ties between the two summation orders
            for p_ in mac.agent.fc2_q_head.parameters():
                p_.mul_(3.0)
        if mac_on_gpu:
            mac.cuda()
        buf = EpisodeReplayBuffer(args)
    return BatchedEpisodeRunner(env, mac, buf, args), buf, mac


def _moving_scenario():
    return cases.compiled(cases.moving_ring_dict(3, 4), T_RUN)[0]


def test_moving_rollout_vs_step_by_step():
    """Three launches against the step loop with the same weights, seeds and exploration counters, two episode batches.
    The observation rows are the same bits; the hidden states do not depend on the actions here and differ by the
    summation order of the recurrent product only; a chosen action may differ on a near-tie of the Q-values."""
    sc = _moving_scenario()
    E, T = E_RUN, T_RUN
    rm, bm, mm = _runner(sc)
    rs, bs, ms = _runner(sc)
    rm.moving_episode_rollout = True
    assert rm.moving_rollout_available() and rs.moving_rollout_available() and not rs.moving_episode_rollout
    assert not rm.fused_rollout_available() and not rm._static
    calls = []
    orig = rm.rollout_moving
    rm.rollout_moving = lambda **kw: (calls.append(kw), orig(**kw))[1]
    for _ in range(2):
        rm.run(sync_stats=True)
        rs.run(sync_stats=True)
    assert len(calls) == 2 and rm.t_env == rs.t_env == 2 * T
    assert mm.action_selector.epsilon == pytest.approx(ms.action_selector.epsilon)
    assert bm.obs_static is False and bs.obs_static is False
    B = {k: (bm.buffers[k][:2 * E], bs.buffers[k][:2 * E]) for k in bm.buffers}
    for k in ("state", "obs", "avail_actions", "terminated", "filled"):
        assert torch.equal(*B[k]), k
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(DEV)
    assert torch.equal(B["state"][0][:, :T][:, :, sc.position_columns], pos[:T].expand(2 * E, -1, -1))
    assert bool(B["terminated"][0][:, T - 1].all())
    dh = float((B["hidden_state"][0] - B["hidden_state"][1]).abs().max())
    same = B["actions_discrete"][0] == B["actions_discrete"][1]                      # [N, T, J, 1]
    frac = float(same.float().mean())
    hm = B["hidden_state"][0][:, :T]
    step_change = float((hm[:, 1:] - hm[:, :-1]).abs().max())
    print(f"[moving rollout] max |hidden - step loop| = {dh:.3e}, equal actions {frac:.5f}, "
          f"max |h| = {float(hm.abs().max()):.4f}, mean |h| = {float(hm.abs().mean()):.4f}, max |h_t+1 - h_t| = {step_change:.3e}, "
          f"distinct actions {int(B['actions_discrete'][0].unique().numel())}")
    assert step_change > 0.0 and bool(torch.isfinite(hm).all())      # a trajectory, not a fixed point
    assert dh <= 2e-5
    assert frac >= 0.995
    pa, pb = B["actions_continuous"]
    assert torch.equal(pa[same], pb[same])
    agree = same.all(dim=2).squeeze(-1)                                              # [N, T]: all agents agree
    assert float((B["reward"][0].squeeze(-1)[agree] - B["reward"][1].squeeze(-1)[agree]).abs().max()) <= 1e-5
    # every differing row is a near-tie, by stock torch ops on the stored hidden state
    a = mm.agent
    diff = (~same).squeeze(-1).nonzero()                                             # rows (n, t, j)
    if diff.numel():
        with torch.no_grad():
            n_, t_, j_ = diff.unbind(1)
            h = B["hidden_state"][0][n_, t_, j_]
            P = a.actor(B["obs"][0][n_, t_, j_])
            q = a.q_values_all_actions(h, P)
            qa = q.gather(1, B["actions_discrete"][0][n_, t_, j_].long())
            qb = q.gather(1, B["actions_discrete"][1][n_, t_, j_].long())
            assert float((qa - qb).abs().max()) <= 1e-5 * max(1.0, float(q.abs().max()))
    assert float((mm.hidden_states - ms.hidden_states).abs().max()) <= 2e-5
    # step t ran on frame t: the stored trajectory of the last batch against torch.nn.GRUCell on the stored observations
    with torch.no_grad():
        st, H = rm.stage, 64
        h = torch.zeros(E * rm.n_agents, H, device=DEV)
        for t in range(T):
            assert torch.equal(st["obs"][t], rm.env.frame_states()[t].expand(E, rm.n_agents, -1))
            h_ref = a.rnn(torch.relu(a.fc1(st["obs"][t].reshape(E * rm.n_agents, -1))), h)
            h = st["hidden_state"][t].reshape(E * rm.n_agents, H)
            assert float((h - h_ref).abs().max()) <= 2e-5, t
        assert torch.equal(mm.hidden_states, h)
    assert torch.equal(rm.env.step_count, rs.env.step_count) and int(rm.env.step_count[0]) == T
    assert torch.equal(rm.env.positions, rs.env.positions)
    assert torch.equal(rm.env.get_state()[:, sc.position_columns], rs.env.get_state()[:, sc.position_columns])
    assert torch.equal(rm.env.positions, pos[T].expand(E, -1))


def test_cut_batch_leaves_later_staging_rows_untouched():
    sc = _moving_scenario()
    r, _, _ = _runner(sc)
    r.moving_episode_rollout = True
    n = 5
    before = {}
    for k, v in r.stage.items():
        v[n:] = (float("nan") if v.dtype.is_floating_point else (True if v.dtype == torch.bool else -7))
        before[k] = v[n:].clone()
    r.rollout_moving(n_steps=n)
    torch.cuda.synchronize()
    for k, v in r.stage.items():
        eq = (torch.isnan(v[n:]).all() if v.dtype.is_floating_point else torch.equal(v[n:], before[k]))
        assert bool(eq), k
        if v.dtype.is_floating_point:
            assert not bool(torch.isnan(v[:n]).any()), k
    frames = r.env.frame_states()
    assert torch.equal(r.stage["state"][:n], frames[:n].unsqueeze(1).expand(-1, E_RUN, -1))
    assert torch.equal(r.stage["obs"][:n], frames[:n].view(n, 1, 1, -1).expand(-1, E_RUN, r.n_agents, -1))
    assert bool((r.stage["avail_actions"][:n] == 1).all())
    assert r.t_env == n and int(r.env.step_count[0]) == n
    assert torch.equal(r.env.positions, frames[n][sc.position_columns].expand(E_RUN, -1))
    # a longer batch afterwards fills the rows the cut one left out
    r.rollout_moving()
    assert torch.equal(r.stage["state"][:T_RUN], frames[:T_RUN].unsqueeze(1).expand(-1, E_RUN, -1))
    assert not bool(torch.isnan(r.stage["hidden_state"][:T_RUN]).any())


KEYS = ("hidden_state", "actions_discrete", "actions_continuous", "reward", "terminated")


def test_graph_replay_equals_eager_with_the_switch_on():
    sc = _moving_scenario()
    r_e, _, m_e = _runner(sc)
    r_g, _, m_g = _runner(sc)
    r_e.moving_episode_rollout = r_g.moving_episode_rollout = True
    r_g.enable_graph()
    for _ in range(2):
        r_e.rollout_moving()
        r_g.run(sync_stats=True)
        for k in KEYS + ("state", "obs", "avail_actions"):
            assert torch.equal(r_e.stage[k], r_g.stage[k]), k
        assert torch.equal(m_e.hidden_states, m_g.hidden_states)
        assert torch.equal(r_e.env.positions, r_g.env.positions) and torch.equal(r_e.env.step_count, r_g.env.step_count)
    assert r_e.t_env == r_g.t_env == 2 * T_RUN
    r_g.release_graphs()


def test_switch_off_keeps_the_step_loop(monkeypatch):
    from macjd_amd import options
    monkeypatch.delenv("MACJD_MOVING_EPISODE_ROLLOUT", raising=False)
    options.reload()
    sc = _moving_scenario()
    r_a, b_a, _ = _runner(sc)
    r_b, b_b, _ = _runner(sc)
    assert r_a.moving_rollout_available() and not r_a.moving_episode_rollout

    def never(*a, **kw):
        raise AssertionError("the moving whole-episode path ran with the switch off")
    r_a.rollout_moving = r_a._moving_launches = never
    for _ in range(2):
        r_a.run(sync_stats=True)
        r_b.begin_episodes()            # the step loop, spelled out
        for t in range(T_RUN):
            r_b.step(t)
        r_b.end_episodes()
    for k in b_a.buffers:
        assert torch.equal(b_a.buffers[k], b_b.buffers[k]), k
    r_a.enable_graph()                  # ... and the captured rollout is the step loop too
    r_a.run(sync_stats=True)
    r_b.begin_episodes()
    for t in range(T_RUN):
        r_b.step(t)
    for k in KEYS:
        assert torch.equal(r_a.stage[k], r_b.stage[k]), k
    r_a.release_graphs()


def test_availability_is_false_elsewhere():
    from macjd_amd.scenario import Scenario, ring_scenario_dict
    static = _runner(Scenario.from_dict(ring_scenario_dict(3, 4)))[0]
    scan = _runner(Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_scan.yaml")), E=16)[0]
    host_mac = _runner(_moving_scenario(), mac_on_gpu=False)[0]
    generic = _runner(cases.compiled(cases.moving_ring_dict(3, 3), T_RUN)[0])[0]     # no many-step launch at this size
    for r in (static, scan, host_mac, generic):
        r.moving_episode_rollout = True
        assert not r.moving_rollout_available()
        with pytest.raises(RuntimeError, match="not available"):
            r.rollout_moving()
    flagged = _runner(_moving_scenario())[0]
    assert flagged.moving_rollout_available()
    flagged.env.kernel_flags = 2
    assert not flagged.moving_rollout_available()
    with pytest.raises(AttributeError, match="does not move"):
        static.env.frame_states()
