"""Closed-loop episode launch for scanning radars on the GPU (include/macjd_nets.h, macjd_agent_env_episode_scan): the
env half teacher-forced against ``env.step`` and against the NumPy restatement, the agent half teacher-forced per step
against the step-by-step agent path, the hand-over to single steps, graph replay, the driver and the guard rails.

Tolerances are the issue's: integer outputs / azimuths bit-equal, reward 1e-5 (project bar), rdpj sums 1e-5 T, hidden
state and power 1e-5, arg-max within 2e-5 of the recomputed maximum (two Q-values each inside the 1e-5 bar)."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scan_model
from _harness import oracle_lib, random_actions
from test_scan_gpu import DEV, PKG, SCN, _base, _env, _runner, _sc, _scan_dict

pytestmark = pytest.mark.gpu


def _yaml_sc():
    from macjd_amd.scenario import Scenario
    return Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_scan.yaml"))


def _sc_2j2r():
    return _sc(_scan_dict(_base("2j2r_shipped"), 0.25, -30.0))


def _closed(sc, E, test_mode, n_steps=None, seed=5):
    r, buf, args = _runner(sc, E, seed=seed)
    r.closed_loop_rollout = True
    assert r.closed_loop_available() and not r.fused_rollout_available()
    r.rollout_closed_loop(test_mode=test_mode, n_steps=n_steps)
    torch.cuda.synchronize()
    return r, buf, args


def _check_env_half_and_hand_over(sc, E, test_mode):
    """Items 1 and 4: a second env with the same seed / episode index, stepped on the stored actions."""
    T, R, J = sc.episode_limit, sc.num_radars, sc.num_jammers
    cols = sc.theta_a_columns
    other = [c for c in range(sc.state_dim) if c not in cols]
    r, _, _ = _closed(sc, E, test_mode)
    st = r.stage
    env2 = _env(sc, E, seed=5)
    env2.reset()
    assert torch.equal(env2.episode_index, r.env.episode_index)
    sum2 = torch.zeros((E, 3), dtype=torch.float32, device=DEV)
    static = torch.from_numpy(sc.state_vector()).to(DEV)
    worst = 0.0
    for t in range(T):
        s2 = env2.get_state()
        assert torch.equal(st["state"][t][:, cols], s2[:, cols]), t
        assert torch.equal(st["obs"][t][:, :, cols], s2[:, cols].unsqueeze(1).expand(-1, J, -1)), t
        assert torch.equal(st["state"][t][:, other], static[other].expand(E, -1)), t
        rew, term, _ = env2.step(st["actions_discrete"][t], st["actions_continuous"][t], want_info=False, rdpj_sum=sum2)
        assert torch.equal(st["terminated"][t].view(E), term), t
        worst = max(worst, (st["reward"][t].view(E) - rew).abs().max().item())
    print(f"E={E} test_mode={test_mode}: max |reward - env.step| = {worst:.3e}, "
          f"max |rdpj_sum diff| = {(r._rdpj_sum - sum2).abs().max().item():.3e}")
    assert worst <= 1e-5
    assert (r._rdpj_sum - sum2).abs().max().item() <= 1e-5 * T
    assert not st["state"][T].any() and not st["obs"][T].any()                    # row T stays zero
    assert np.unique(st["state"][:T, :, cols[0]].cpu().numpy()).size > 5          # the loop really is closed
    assert torch.unique(st["actions_discrete"]).numel() >= 5
    # hand-over: the env is where T single steps leave it
    env1 = r.env
    assert torch.equal(env1.track, env2.track)
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(env1.get_state(), env2.get_state())
    assert torch.equal(env1.step_count, env2.step_count) and torch.equal(env1.episode_index, env2.episode_index)
    assert torch.equal(r.mac.hidden_states.view(E, J, -1), st["hidden_state"][T - 1])
    rng = np.random.default_rng(E)
    Tn, Pn = random_actions(rng, E, J, R)
    Td, Pd = torch.from_numpy(Tn).to(DEV), torch.from_numpy(Pn).to(DEV)
    r1, t1, i1 = env1.step(Td, Pd)
    r2, t2, i2 = env2.step(Td, Pd)
    assert torch.equal(i1["radar_tracking"], i2["radar_tracking"]) and torch.equal(t1, t2)
    assert torch.equal(i1["step_count"], i2["step_count"]) and torch.equal(i1["snr_no_jamming"], i2["snr_no_jamming"])
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(r1, r2)   # same kernel, same inputs
    return r


def _check_agent_half(r, sc, E, test_mode, ep=0):
    """Item 3: per step, the step-by-step agent path on the stored obs[t] and hidden_state[t - 1]."""
    from macjd_amd import ops
    T, J = sc.episode_limit, sc.num_jammers
    st, mac = r.stage, r.mac
    agent = mac.agent
    H, A = agent.rnn_hidden_dim, agent.n_actions
    l1, l2 = agent.fc2_q_head[0], agent.fc2_q_head[2]
    eps = r._eps_sched.cpu().numpy()
    avail = r.env.get_avail_actions()
    worst_h = worst_p = worst_q = 0.0
    n_flip = 0
    with torch.no_grad():
        for t in range(T):
            obs = st["obs"][t].reshape(E * J, -1)
            h_prev = torch.zeros(E * J, H, device=DEV) if t == 0 else st["hidden_state"][t - 1].reshape(E * J, H)
            h_ref, P_ref = agent.step_forward(obs, h_prev)
            Q_ref = agent.q_values_all_actions(h_ref, P_ref)
            a = st["actions_discrete"][t].reshape(E * J).long()
            assert int(a.min()) >= 0 and int(a.max()) < A and bool(avail.reshape(E * J, A).gather(1, a.view(-1, 1)).all())
            worst_h = max(worst_h, (st["hidden_state"][t].reshape(E * J, H) - h_ref).abs().max().item())
            worst_p = max(worst_p, (st["actions_continuous"][t].reshape(E * J) - P_ref.gather(1, a.view(-1, 1)).view(-1)).abs().max().item())
            gap = Q_ref.max(dim=1).values - Q_ref.gather(1, a.view(-1, 1)).view(-1)
            if test_mode:
                worst_q = max(worst_q, gap.max().item())
            else:
                base = F.linear(h_ref, l1.weight[:, :H], l1.bias)
                _, _, T32, _ = ops.qhead_select(base, P_ref, l1.weight, l2.weight, l2.bias, H, A, J, avail, epsilon=float(eps[t]),
                                                greedy_only=False, seed=mac.select_seed, counter=ep * (T + 1) + t + 1, want_q=False)
                sel = T32.reshape(E * J).long()
                differ = sel != a
                if bool(differ.any()):    # only a near-tie of the greedy branch may differ: both within 2e-5 of the maximum
                    gap_sel = Q_ref.max(dim=1).values - Q_ref.gather(1, sel.view(-1, 1)).view(-1)
                    n_flip += int(differ.sum())
                    worst_q = max(worst_q, gap[differ].max().item(), gap_sel[differ].max().item())
    print(f"E={E} test_mode={test_mode}: max |h - h_ref| = {worst_h:.3e}, max |P - P_ref| = {worst_p:.3e}, "
          f"max Q gap = {worst_q:.3e}, differing choices = {n_flip}")
    assert worst_h <= 1e-5
    assert worst_p <= 1e-5
    assert worst_q <= 2e-5


@pytest.mark.parametrize("E", [16, 257, 4096])
@pytest.mark.parametrize("test_mode", [False, True])
def test_closed_loop_env_half_agent_half_and_hand_over(E, test_mode):
    sc = _yaml_sc()
    r = _check_env_half_and_hand_over(sc, E, test_mode)
    _check_agent_half(r, sc, E, test_mode)


def test_closed_loop_2j2r():
    sc = _sc_2j2r()
    r = _check_env_half_and_hand_over(sc, 300, False)
    _check_agent_half(r, sc, 300, False)


def test_env_half_vs_restatement():
    """Item 2: the NumPy restatement driven with the stored actions and the oracle's Philox uniforms."""
    sc = _sc(SCN["3j4r"])
    R, J, E, n = sc.num_radars, sc.num_jammers, 65, 60
    cols = sc.theta_a_columns
    lib = oracle_lib()
    r, _, _ = _closed(sc, E, False, n_steps=n, seed=123)
    st = r.stage
    m = scan_model.ScanModel(sc, E)
    ep = r.env.episode_index.cpu().numpy()
    o = None
    for t in range(n):
        np.testing.assert_array_equal(st["state"][t][:, cols].cpu().numpy(), m.theta_a.astype(np.float32))
        u = np.array([[lib.macjd_oracle_uniform(123, e, int(ep[e]), t, k) for k in range(R + J)] for e in range(E)])
        Tt = st["actions_discrete"][t].view(E, J).cpu().numpy()
        Pt = st["actions_continuous"][t].view(E, J).cpu().numpy()
        o = m.step(Tt, Pt, u, arith32=True)
        np.testing.assert_array_equal(st["terminated"][t].view(E).cpu().numpy(), o["terminated"])
        np.testing.assert_allclose(st["reward"][t].view(E).cpu().numpy(), o["out"][:, 0], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(r.env.track.cpu().numpy().astype(bool), o["track"])
    assert r.env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
    np.testing.assert_array_equal(r.env.get_state()[:, cols].cpu().numpy(), o["theta_a"].astype(np.float32))
    assert int(r.env.step_count[0]) == n


def test_graph_replay_equals_eager_closed_loop():
    sc = _yaml_sc()
    E = 256
    r_e, b_e, _ = _runner(sc, E)
    r_g, b_g, _ = _runner(sc, E)
    r_e.closed_loop_rollout = r_g.closed_loop_rollout = True
    r_g.enable_graph()
    try:
        for _ in range(2):
            s_e = r_e.run(sync_stats=True)
            s_g = r_g.run(sync_stats=True)
            assert s_e["episode_return"] == s_g["episode_return"]
        for k in b_e.buffers:
            assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(r_e.mac.hidden_states, r_g.mac.hidden_states)
        assert r_e.t_env == r_g.t_env == 2 * sc.episode_limit
    finally:
        r_g.release_graphs()


def test_switch_off_takes_the_step_by_step_path(monkeypatch):
    from macjd_amd import ops
    sc = _yaml_sc()
    r, _, _ = _runner(sc, 32)
    assert r.closed_loop_rollout is False and r.closed_loop_available()

    def boom(*a, **k):
        raise AssertionError("closed-loop launch with the switch off")
    monkeypatch.setattr(ops, "agent_env_episode_scan", boom)
    r.run(sync_stats=True)
    assert r.t_env == sc.episode_limit


def test_driver_trains_with_the_closed_loop_rollout(tmp_path, monkeypatch):
    from macjd_amd import ops, options
    from macjd_amd.main import load_config, run
    calls = []
    real = ops.agent_env_episode_scan
    monkeypatch.setattr(ops, "agent_env_episode_scan", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("MACJD_CLOSED_LOOP_ROLLOUT", "1")
    options.reload()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cfg = load_config("default", os.path.join(PKG, "config"))
        E = 64
        cfg.device_request = "cuda"
        cfg.sim_config_path = os.path.join(PKG, "config", "scenario_3j4r_scan.yaml")
        cfg.save_model_dir, cfg.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
        cfg.log_interval_seconds = 0
        cfg.gemm_tuning = False
        cfg.resume = None
        for k, v in dict(batch_envs=E, buffer_size=4 * E, total_env_steps=2 * E * 100, start_training_steps=0,
                         save_interval=10 ** 9, test_interval=10 ** 9, test_nepisodes=E, batch_size=16, lr=1e-4).items():
            setattr(cfg, k, v)
        with contextlib.redirect_stdout(io.StringIO()) as out:
            res = run(cfg)
    finally:
        monkeypatch.delenv("MACJD_CLOSED_LOOP_ROLLOUT", raising=False)
        options.reload()
    assert res["total_steps"] == 2 * E * 100 and res["episodes"] == 2 * E and res["train_steps"] > 0
    assert "Training finished." in out.getvalue()
    assert calls, "the driver never issued the closed-loop launch"


def test_guard_rails():
    from macjd_amd import _native, ops
    # unsupported sizes: 6j/8r, H = 128
    r6, _, _ = _runner(_sc(SCN["6j8r"]), 32)
    r6.closed_loop_rollout = True
    assert not r6.closed_loop_available()
    with pytest.raises(RuntimeError, match="not available"):
        r6.rollout_closed_loop()
    assert not ops.agent_env_episode_scan_supported(6, 8, 64, 17) and not ops.agent_env_episode_scan_supported(3, 4, 128, 9)
    # a non-scanning scenario
    r0, _, _ = _runner(_sc(_base("3j4r")), 32)
    r0.closed_loop_rollout = True
    assert not r0.closed_loop_available()
    with pytest.raises(RuntimeError, match="do not scan"):
        r0.env.episode_scan_args()
    # the C call itself
    lib = _native.load()
    env = _env(_yaml_sc(), 16)
    cio = _native.AgentEnvEpisodeScanIO()
    cio.n_envs, cio.T, cio.J, cio.R, cio.H, cio.A, cio.S, cio.actor_hidden = 16, 1, 6, 8, 64, 17, 46, 128
    assert lib.macjd_agent_env_episode_scan(env._handle.ptr, ctypes.byref(cio), None) == -4     # MACJD_EUNSUPPORTED
    cio.J, cio.R, cio.A, cio.H = 3, 4, 9, 128
    assert lib.macjd_agent_env_episode_scan(env._handle.ptr, ctypes.byref(cio), None) == -4
    cio.H = 64
    cio.pe_tables = env._theta_a.data_ptr()                                                       # per-env tables: refused
    assert lib.macjd_agent_env_episode_scan(env._handle.ptr, ctypes.byref(cio), None) == -4
    assert b"per-env" in lib.macjd_last_error()
    cio.pe_tables = None
    assert lib.macjd_agent_env_episode_scan(env._handle.ptr, ctypes.byref(cio), None) == -1     # NULL pointers: MACJD_EINVAL
    e0 = _env(_sc(_base("3j4r")), 16)                                                            # handle without scan tables
    assert lib.macjd_agent_env_episode_scan(e0._handle.ptr, ctypes.byref(cio), None) == -1
    assert b"scanning" in lib.macjd_last_error()
    # step_many keeps refusing scanning
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="scanning"):
        env.step_many(z(4, 16, 3, dt=torch.int32), z(4, 16, 3), z(4, 16), z(4, 16, dt=torch.uint8), z(4, 16, 3))
