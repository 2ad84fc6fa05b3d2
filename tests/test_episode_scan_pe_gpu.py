"""Closed-loop episode launch on per-env scanning scenario batches on the GPU (include/macjd_nets.h,
macjd_agent_env_episode_scan_pe), with and without a stepped antenna pattern per env: the env half and the hand-over
teacher-forced against ``env.step`` on the same batch in every table layout, against the NumPy restatements per env, the
agent half per step against the step-by-step agent path, graph replay, the switch and the old names, the driver, and the
entry point's refusals.  Inputs: tests/scan_pe_cases.py and tests/scan_pe_pattern_cases.py (env 1 sweeps a full turn per
step, env 2 has a jammer on a radar).

Tolerances: integer outputs / azimuths / theta_a columns bit-equal, reward 1e-5 (project bar), rdpj sums 1e-5 T, hidden
state and power 1e-5, arg-max within 2e-5 of the recomputed maximum (two Q-values each inside the 1e-5 bar)."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import scan_model
import scan_pattern_model
import scan_pe_cases as cases
import scan_pe_pattern_cases as pcases
from _harness import oracle_lib, random_actions
from test_episode_scan_gpu import _check_agent_half
from test_scan_pe_gpu import DEV, PKG, _pe_env, _runner

pytestmark = pytest.mark.gpu
SEED, OFF = 5, 100     # env seed and global index of env 0 (scenario variation and Monte-Carlo stream alike)


def _batch(J, R, E, L, seed=5):
    """(scenarios, batch): per-env scanning scenarios, under the L-level pattern when L > 0."""
    return pcases.batch(J, R, E, seed, OFF, L=L) if L else cases.batch(J, R, E, seed, OFF)


def _layout(monkeypatch, layout):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    if layout == "tiled8":
        monkeypatch.setattr(Env, "PE_TILE", 8)
    monkeypatch.setattr(Env, "pe_tiled", layout != "plain")
    return {"tiled8": 8, "tile256": 256, "plain": 0}[layout]


def _closed_pe(batch, test_mode=False, n_steps=None, seed=SEED):
    r, _, _ = _runner(batch, seed=seed)
    r.env.env_offset = OFF
    r.closed_loop_rollout = True
    assert r.closed_loop_pe_available() and not r.closed_loop_available() and not r.fused_rollout_available()
    r.rollout_closed_loop_pe(test_mode=test_mode, n_steps=n_steps)
    torch.cuda.synchronize()
    return r


def _check_env_half_and_hand_over(r, batch):
    """A second per-env environment with the same batch, seed, env offset and episode index, stepped on the stored actions."""
    sc = batch.base
    E, T, R, J = batch.n_envs, sc.episode_limit, sc.num_radars, sc.num_jammers
    cols = sc.theta_a_columns
    other = [c for c in range(sc.state_dim) if c not in cols]
    st = r.stage
    env2 = _pe_env(batch, seed=SEED, env_offset=OFF)
    env2.reset()
    assert torch.equal(env2.episode_index, r.env.episode_index)
    sum2 = torch.zeros((E, 3), dtype=torch.float32, device=DEV)
    own = torch.from_numpy(batch.state_vectors).to(DEV)
    worst, distinct = 0.0, 0
    for t in range(T):
        s2 = env2.get_state()
        assert torch.equal(st["state"][t][:, cols], s2[:, cols]), t
        assert torch.equal(st["obs"][t][:, :, cols], s2[:, cols].unsqueeze(1).expand(-1, J, -1)), t
        assert torch.equal(st["state"][t][:, other], own[:, other]), t
        assert torch.equal(st["obs"][t][:, :, other], own[:, None, other].expand(-1, J, -1)), t
        rew, term, _ = env2.step(st["actions_discrete"][t], st["actions_continuous"][t], want_info=False, rdpj_sum=sum2)
        assert torch.equal(st["terminated"][t].view(E), term), t
        worst = max(worst, (st["reward"][t].view(E) - rew).abs().max().item())
        distinct = max(distinct, torch.unique(st["reward"][t]).numel())
    sum_err = (r._rdpj_sum - sum2).abs().max().item()
    print(f"E={E}: max |reward - env.step| = {worst:.3e}, max |rdpj_sum diff| = {sum_err:.3e}, "
          f"most distinct rewards in a step = {distinct}")
    assert worst <= 1e-5
    assert sum_err <= 1e-5 * T
    assert distinct > E // 2                                                      # the envs really read different tables
    assert not st["state"][T].any() and not st["obs"][T].any()                    # row T stays zero
    assert torch.unique(st["actions_discrete"]).numel() >= 5
    # hand-over: the env is where T single steps leave it
    env1 = r.env
    assert torch.equal(env1.track, env2.track)
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(env1.get_state(), env2.get_state())
    assert torch.equal(env1.step_count, env2.step_count) and torch.equal(env1.episode_index, env2.episode_index)
    assert torch.equal(env1._snr_no_step, env2._snr_no_step)                      # the last step's value, each env's own row
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


# ---------------------------------------------------------------------------------------------------------------
# 1 + 2. env half, hand-over and agent half, teacher-forced, in every table layout
LAYOUT_CASES = [(lay, L) for lay in ("tiled8", "tile256", "plain") for L in (0, 4)] + [("tiled8", 1), ("tiled8", 6)]


@pytest.mark.parametrize("layout,L", LAYOUT_CASES)
def test_closed_loop_pe_env_half_agent_half_and_hand_over(layout, L, monkeypatch):
    """3j/4r, E = 40: two full workgroups and half of one; with tiles of 8 a workgroup spans two tiles and the last tile is
    padded."""
    tile = _layout(monkeypatch, layout)
    _, batch = _batch(3, 4, 40, L)
    r = _closed_pe(batch)
    assert r.env._pe_tile == tile and (r.env._scan_pe_pattern_io is not None) == (L > 0)
    _check_env_half_and_hand_over(r, batch)
    _check_agent_half(r, batch.base, 40, False)


def test_closed_loop_pe_last_workgroup_in_a_second_tile():
    """E = 257 with the default tile of 256: the last workgroup has one live env, in the second tile."""
    _, batch = _batch(3, 4, 257, 0)
    r = _closed_pe(batch)
    assert r.env._pe_tile == 256
    _check_env_half_and_hand_over(r, batch)
    _check_agent_half(r, batch.base, 257, False)


def test_closed_loop_pe_test_mode(monkeypatch):
    _layout(monkeypatch, "tiled8")
    _, batch = _batch(3, 4, 40, 4)
    r = _closed_pe(batch, test_mode=True)
    _check_env_half_and_hand_over(r, batch)
    _check_agent_half(r, batch.base, 40, True)


# ---------------------------------------------------------------------------------------------------------------
# 3. env half against the NumPy restatements, one model per env
@pytest.mark.parametrize("L", [0, 4])
def test_env_half_vs_restatement_per_env(L, monkeypatch):
    _layout(monkeypatch, "tiled8")
    J, R, E, n, seed = 3, 4, 33, 12, 123
    scs, batch = _batch(J, R, E, L, seed=9)
    cols = batch.base.theta_a_columns
    lib = oracle_lib()
    r = _closed_pe(batch, n_steps=n, seed=seed)
    st = r.stage
    models = [scan_pattern_model.ScanPatternModel(sc, 1) if L else scan_model.ScanModel(sc, 1) for sc in scs]
    ep = r.env.episode_index.cpu().numpy()
    worst = 0.0
    outs = None
    for t in range(n):
        theta = np.concatenate([m.theta_a for m in models])
        np.testing.assert_array_equal(st["state"][t][:, cols].cpu().numpy(), theta.astype(np.float32))
        u = np.array([[lib.macjd_oracle_uniform(seed, OFF + e, int(ep[e]), t, k) for k in range(R + J)] for e in range(E)])
        Tt = st["actions_discrete"][t].view(E, J).cpu().numpy()
        Pt = st["actions_continuous"][t].view(E, J).cpu().numpy()
        outs = [m.step(Tt[e:e + 1], Pt[e:e + 1], u[e:e + 1], arith32=True) for e, m in enumerate(models)]
        cat = lambda k: np.concatenate([np.asarray(o[k]) for o in outs])
        np.testing.assert_array_equal(st["terminated"][t].view(E).cpu().numpy(), cat("terminated"))
        worst = max(worst, np.abs(st["reward"][t].view(E).cpu().numpy() - cat("out")[:, 0]).max())
    print(f"L={L}: max |reward - restatement| = {worst:.3e}")
    assert worst <= 1e-5
    cat = lambda k: np.concatenate([np.asarray(o[k]) for o in outs])
    np.testing.assert_array_equal(r.env.track.cpu().numpy().astype(bool), cat("track"))
    assert r.env.beam_azimuth.cpu().numpy().tobytes() == np.ascontiguousarray(cat("theta_a")).tobytes()
    np.testing.assert_array_equal(r.env.get_state()[:, cols].cpu().numpy(), cat("theta_a").astype(np.float32))
    assert int(r.env.step_count[0]) == n


# ---------------------------------------------------------------------------------------------------------------
# 4. the small size
@pytest.mark.parametrize("L", [0, 4])
def test_closed_loop_pe_2j2r(L, monkeypatch):
    _layout(monkeypatch, "tiled8")
    _, batch = _batch(2, 2, 40, L)
    r = _closed_pe(batch)
    _check_env_half_and_hand_over(r, batch)
    _check_agent_half(r, batch.base, 40, False)


# ---------------------------------------------------------------------------------------------------------------
# 5. graph replay
@pytest.mark.parametrize("L", [0, 4])
def test_graph_replay_equals_eager_closed_loop_pe(L):
    from macjd_amd.scenario import ScenarioBatch
    E = 64
    base = pcases.pattern_base(3, 4, L=L) if L else cases.scan_base(3, 4)
    batch = ScenarioBatch.randomized(base, E, seed=2, azimuth_jitter=cases.AZIMUTH_JITTER)
    r_e, b_e, _ = _runner(batch)
    r_g, b_g, _ = _runner(batch)
    r_e.closed_loop_rollout = r_g.closed_loop_rollout = True
    assert r_g.closed_loop_pe_available()
    r_g.enable_graph()
    try:
        for _ in range(2):
            s_e = r_e.run(sync_stats=True)
            s_g = r_g.run(sync_stats=True)
            assert s_e["episode_return"] == s_g["episode_return"]
        for k in b_e.buffers:
            assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(r_e.mac.hidden_states, r_g.mac.hidden_states)
        assert r_e.t_env == r_g.t_env == 2 * batch.base.episode_limit
    finally:
        r_g.release_graphs()


# ---------------------------------------------------------------------------------------------------------------
# 6. the switch and the old names
def test_switch_and_old_names(monkeypatch):
    from macjd_amd import ops
    _, batch = _batch(3, 4, 32, 0)
    r, _, _ = _runner(batch)
    assert r.closed_loop_rollout is False and r.closed_loop_pe_available()
    calls = []
    real = ops.agent_env_episode_scan_pe

    def boom(*a, **k):
        raise AssertionError("per-env closed-loop launch with the switch off")
    monkeypatch.setattr(ops, "agent_env_episode_scan_pe", boom)
    r.run(sync_stats=True)
    assert r.t_env == batch.base.episode_limit
    monkeypatch.setattr(ops, "agent_env_episode_scan_pe", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    r.closed_loop_rollout = True
    r.run(sync_stats=True)
    assert calls == [1] and r.t_env == 2 * batch.base.episode_limit
    # the old names keep their answers on a batch
    assert not r.closed_loop_available()
    with pytest.raises(RuntimeError, match="closed_loop_available"):
        r.rollout_closed_loop()
    with pytest.raises(RuntimeError, match="per-env scenario tables"):
        r.env.episode_scan_args()
    # kernel_flags != 0
    from macjd_amd import _native
    r.env.kernel_flags = _native.STEP_LANE_KERNEL
    assert not r.closed_loop_pe_available()
    with pytest.raises(RuntimeError, match="closed_loop_pe_available"):
        r.rollout_closed_loop_pe()
    r.env.kernel_flags = 0
    assert r.closed_loop_pe_available()
    # a 6j/8r batch: no closed-loop kernel of that size
    _, b6 = _batch(6, 8, 16, 0)
    r6, _, _ = _runner(b6)
    r6.closed_loop_rollout = True
    assert not r6.closed_loop_pe_available() and not ops.agent_env_episode_scan_pe_supported(6, 8, 64, 17)
    with pytest.raises(RuntimeError, match="closed_loop_pe_available"):
        r6.rollout_closed_loop_pe()
    # a shared-table scanning runner: the shared launch's, not this one
    from test_scan_gpu import _runner as shared_runner
    from macjd_amd.scenario import Scenario
    rs, _, _ = shared_runner(Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_scan.yaml")), 16)
    assert rs.closed_loop_available() and not rs.closed_loop_pe_available()
    with pytest.raises(RuntimeError, match="closed_loop_pe_available"):
        rs.rollout_closed_loop_pe()
    with pytest.raises(RuntimeError, match="per-env scanning scenario batch"):
        rs.env.episode_scan_pe_args()


# ---------------------------------------------------------------------------------------------------------------
# 7. the driver
def test_driver_trains_with_the_per_env_closed_loop_rollout(tmp_path, monkeypatch):
    from macjd_amd import ops, options
    from macjd_amd.main import load_config, run
    calls = []
    real = ops.agent_env_episode_scan_pe
    monkeypatch.setattr(ops, "agent_env_episode_scan_pe", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("MACJD_CLOSED_LOOP_ROLLOUT", "1")
    options.reload()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cfg = load_config("default", os.path.join(PKG, "config"))
        E = 64
        cfg.device_request = "cuda"
        cfg.sim_config_path = os.path.join(PKG, "config", "scenario_3j4r_scan_pattern.yaml")
        cfg.save_model_dir, cfg.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
        cfg.log_interval_seconds = 0
        cfg.gemm_tuning = False
        cfg.resume = None
        cfg.randomize_scenarios = True
        cfg.randomize_azimuth_jitter = 30.0
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
    assert calls, "the driver never issued the per-env closed-loop launch"


# ---------------------------------------------------------------------------------------------------------------
# 8. the entry point's refusals: each returns its code and names the argument, before any launch
def test_entry_point_refusals(monkeypatch):
    from macjd_amd import _native, ops
    from macjd_amd.scenario import Scenario
    _layout(monkeypatch, "plain")                      # plain layout: the strides are checked
    J, R, E = 3, 4, 16
    _, batch = _batch(J, R, E, 4)
    r, _, _ = _runner(batch)
    r.env.env_offset = OFF
    r.closed_loop_rollout = True
    captured = {}
    lib = _native.load()
    real = lib.macjd_agent_env_episode_scan_pe

    class Spy:   # keeps a copy of the argument block of a valid call
        def __getattr__(self, name):
            return getattr(lib, name)

        def macjd_agent_env_episode_scan_pe(self, h, ref, stream):
            captured["io"] = _native.AgentEnvEpisodeScanPeIO.from_buffer_copy(ref._obj)
            captured["h"], captured["stream"] = h, stream
            return real(h, ref, stream)
    real_load = _native.load
    monkeypatch.setattr(_native, "load", lambda: Spy())
    r.rollout_closed_loop_pe(n_steps=2)
    torch.cuda.synchronize()
    monkeypatch.setattr(_native, "load", real_load)
    good, h, stream = captured["io"], captured["h"], captured["stream"]
    err = lambda: lib.macjd_last_error().decode()
    before = {k: v.clone() for k, v in r.stage.items()}
    step0 = r.env.step_count.clone()

    def call(handle=h, **changes):
        io_ = _native.AgentEnvEpisodeScanPeIO.from_buffer_copy(good)
        for path, v in changes.items():
            obj, parts = io_, path.split("__")
            for p in parts[:-1]:
                obj = getattr(obj, p)
            setattr(obj, parts[-1], v)
        return lib.macjd_agent_env_episode_scan_pe(handle, ctypes.byref(io_), stream)

    assert call(base__pe_tables=None) == -1 and "pe_tables" in err()
    assert call(pe_flags=None) == -1 and "pe_flags" in err()
    assert call(scan_pe__tables=None) == -1 and "scan_pe.tables" in err()
    assert call(pe_stride=E - 1) == -1 and "pe_stride" in err()
    assert call(scan_pe__stride=E - 1) == -1 and "scan_pe.stride" in err()
    assert call(pattern__stride=E - 1) == -1 and "pattern.stride" in err()
    assert call(pe_tile=-1) == -1 and "pe_tile" in err()
    assert call(pattern__n_levels=0) == -1 and "n_levels" in err()
    assert call(pattern__n_levels=7) == -1 and "n_levels" in err()
    assert call(base__J=6, base__R=8, base__A=17) == -4 and "unsupported" in err()
    assert call(base__H=128) == -4 and "unsupported" in err()
    assert lib.macjd_agent_env_episode_scan_pe(h, None, stream) == -1 and "NULL" in err()
    with torch.cuda.device(DEV):
        static = _native.ScenarioHandle(Scenario.from_dict(cases.ring_scenario_dict(J, R)))
        pat4 = _native.ScenarioHandle(batch.base)                                # a handle that carries 4 pattern levels
    assert call(handle=static.ptr) == -1 and "no scanning tables" in err()
    assert call(handle=pat4.ptr) == 0                                            # equal L: accepted
    assert call(handle=pat4.ptr, pattern__n_levels=3) == -4 and "pattern levels" in err()
    assert call(handle=pat4.ptr, pattern__tables=None) == -4 and "pattern levels" in err()
    # the shared entry point keeps refusing per-env tables
    assert lib.macjd_agent_env_episode_scan(h, ctypes.byref(good.base), stream) == -4 and "per-env" in err()
    # none of the refused calls launched: the one accepted call above advanced the counters by its two steps, nothing else moved
    torch.cuda.synchronize()
    assert torch.equal(r.env.step_count, step0 + 2)
    for k in ("state", "obs"):
        assert torch.equal(r.stage[k][2:], before[k][2:]), k
    assert ops.agent_env_episode_scan_pe_supported(3, 4, 64, 9) and not ops.agent_env_episode_scan_pe_supported(3, 4, 128, 9)
