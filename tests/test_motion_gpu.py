"""Moving jammers, radars and target on the GPU (include/macjd.h, macjd_env_step_moving): the reference-generated fixture,
bitwise equality with the per-env-table step on the gathered frames, the frame oracle (tests/motion_cases.py), the
many-step launch, the state rows, the zero-velocity reduction, the runner and the single-env facade."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import motion_cases as cases
from _harness import REPO, random_actions
from test_env_gpu import TOL_REWARD, _cmp
from test_nets_cpu import make_args, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
F = cases.F_SHORT
SIZES = [(2, 2), (3, 4), (6, 8), (3, 3)]   # three compiled sizes and a generic one


def _env(sc, E, seed=11, **kw):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=seed, **kw)


def _diag(E, R, J):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    return {"out64": z(E, 4), "pd64": z(E, R), "snr64": z(E, R), "prj64": z(E, J)}


def _cuda(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _third(E):
    return torch.from_numpy((np.arange(E) % 3 == 0).astype(np.uint8)).to(DEV)


@contextlib.contextmanager
def _options(monkeypatch, **kv):
    from macjd_amd import _native
    for k, v in kv.items():
        monkeypatch.setenv(k, v)
    _native.reload_options()
    try:
        yield
    finally:
        for k in kv:
            monkeypatch.delenv(k, raising=False)
        _native.reload_options()


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's own trace
@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_fixture_trace_single_env(mode):
    """tests/golden/env_3j4r_moving.npz (the reference stepped on moved positions) through the moving step at E = 1: the
    assertions and tolerances of test_env_gpu.py::test_golden_trace_single_env, plus the state rows, exactly."""
    cfg, g = cases.fixture()
    sc, _ = cases.compiled(cfg, None)
    R, J = sc.num_radars, sc.num_jammers
    env = _env(sc, 1)
    diag = _diag(1, R, J)
    pre = f"{mode}_s42_"
    T, P, U = g[pre + "T"], g[pre + "P"], g[pre + "u"]
    Td = torch.from_numpy(T).cuda()
    Pd = torch.from_numpy(P.astype(np.float32) if mode == "f32" else P).cuda()
    Ud = torch.from_numpy(np.nan_to_num(U, nan=2.0)).cuda()
    got = {k: [] for k in ("out", "pd", "snr", "prj", "track", "term", "state", "snr_no")}
    env.reset()
    assert env.get_state().cpu().numpy().tobytes() == g[pre + "obs_reset"][None].tobytes()
    for t in range(T.shape[0]):
        _, term, info = env.step(Td[t:t + 1], Pd[t:t + 1], Ud[t:t + 1], diag=diag)
        got["out"].append(diag["out64"].clone()); got["pd"].append(diag["pd64"].clone())
        got["snr"].append(diag["snr64"].clone()); got["prj"].append(diag["prj64"].clone())
        got["track"].append(info["radar_tracking"].clone()); got["term"].append(term.clone())
        got["state"].append(env.get_state().clone()); got["snr_no"].append(info["snr_no_jamming"].clone())
    cat = lambda k: torch.cat(got[k]).cpu().numpy()
    np.testing.assert_array_equal(cat("track"), g[pre + "track"])            # bit-exact FSM
    np.testing.assert_array_equal(cat("term"), g[pre + "terminated"])
    ref = np.stack([g[pre + "reward"], g[pre + "r_d"], g[pre + "r_p"], g[pre + "r_j"]], axis=1)
    np.testing.assert_allclose(cat("out"), ref, rtol=0, atol=TOL_REWARD)
    np.testing.assert_allclose(cat("out"), ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(cat("pd"), g[pre + "pd"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(cat("snr"), g[pre + "snr_with"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(cat("prj"), g[pre + "prj"], rtol=1e-14, atol=0)
    assert cat("state").tobytes() == g[pre + "obs_after"].astype(np.float32).tobytes()
    np.testing.assert_array_equal(cat("snr_no"), g[pre + "snr_no"].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
# 2. bitwise against the per-env-table step on the gathered frames
def _gathered_reference(sc, frames, E, **kw):
    """An env of the static frame-0 scenario (same R, J, episode limit, r_p bounds and Pd constants in the handle) that steps
    through macjd_env_step on per-env tables; ``load(mv)`` makes env e's column the frame env e of ``mv`` is in (tile width
    1: [E, rows]) and copies ``mv``'s FSM bits, step counters and episode indices."""
    ref = _env(frames[0], E, **kw)
    mt = sc.motion_tables
    fr, fl = _cuda(mt["frames"], mt["flags"])

    def load(mv):
        f_e = torch.clamp(mv._step.to(torch.int64), max=fr.shape[0] - 1)
        ref._pe_tables, ref._pe_flags, ref._pe_tile = fr[f_e].contiguous(), fl[f_e].contiguous(), 1
        ref._track.copy_(mv._track); ref._step.copy_(mv._step); ref._episode.copy_(mv._episode)
        return f_e
    return ref, load


@pytest.mark.parametrize("mode", ["philox", "philox_diag", "uniforms_diag"])
@pytest.mark.parametrize("E", [1, 65, 257])
@pytest.mark.parametrize("J,R", SIZES)
def test_bitwise_equal_to_the_per_env_step_on_gathered_frames(J, R, E, mode):
    sc, frames = cases.compiled(cases.moving_ring_dict(J, R))
    mv = _env(sc, E, seed=77, env_offset=1000)
    ref, load = _gathered_reference(sc, frames, E, seed=77, env_offset=1000)
    mv.reset()
    rng = np.random.default_rng(E * 31 + R)
    d_mv, d_ref = (_diag(E, R, J), _diag(E, R, J)) if mode != "philox" else (None, None)
    rsum_mv, rsum_ref = (torch.zeros((E, 3), device=DEV) for _ in range(2))
    seen_frames = set()
    for t in range(F + 6):   # the envs that are never reset pass F: the clamp
        if t == 5:
            mv.reset(_third(E))
        f_e = load(mv)
        seen_frames.update(f_e.cpu().tolist())
        Tn, Pn = random_actions(rng, E, J, R)
        u = torch.from_numpy(rng.random((E, R + J))).to(DEV) if mode == "uniforms_diag" else None
        if mode != "philox" and t % 2 == 0:
            Pn = Pn.astype(np.float64)   # the float64 action path on every other step of the general form
        Td, Pd = _cuda(Tn, Pn)
        rew, term, info = mv.step(Td, Pd, u, diag=d_mv, rdpj_sum=rsum_mv)
        rew_r, term_r, info_r = ref.step(Td, Pd, u, diag=d_ref, rdpj_sum=rsum_ref)
        assert torch.equal(rew, rew_r) and torch.equal(term, term_r), t
        assert torch.equal(mv._r_dpj, ref._r_dpj) and torch.equal(rsum_mv, rsum_ref), t
        assert torch.equal(mv._track, ref._track) and torch.equal(mv._step, ref._step), t
        assert torch.equal(info["radar_pds"], info_r["radar_pds"]), t
        assert torch.equal(info["snr_with_jamming"], info_r["snr_with_jamming"]), t
        if d_mv is not None:
            for k in d_mv:
                assert torch.equal(d_mv[k], d_ref[k]), (t, k)
    # every third env was reset after 5 steps, the others never: both kinds end past F
    want = np.where(np.arange(E) % 3 == 0, F + 1, F + 6)
    np.testing.assert_array_equal(mv.step_count.cpu().numpy(), want)
    assert seen_frames == set(range(F))


# ---------------------------------------------------------------------------------------------------------------
# 3. against the frame oracle, in-kernel Philox
@pytest.mark.parametrize("J,R", SIZES)
def test_philox_mode_vs_frame_oracle(J, R):
    sc, frames = cases.compiled(cases.moving_ring_dict(J, R))
    E = 257
    env = _env(sc, E, seed=1234, env_offset=5000)
    ora = cases.FrameOracle(frames, E)
    env.reset(); ora.reset()
    rng = np.random.default_rng(R)
    for t in range(F + 3):
        if t == 5:
            m = _third(E)
            env.reset(m); ora.reset(m.cpu().numpy())
        Tn, Pn = random_actions(rng, E, J, R)
        o = ora.step(Tn, Pn, seed=1234, env_offset=5000)
        rew, term, info = env.step(*_cuda(Tn, Pn))
        _cmp(o, rew, term, info)
        np.testing.assert_array_equal(env.episode_index.cpu().numpy(), ora.episode)


# ---------------------------------------------------------------------------------------------------------------
# 4. the many-step launch
@pytest.mark.parametrize("J,R", [(3, 4), (6, 8)])
@pytest.mark.parametrize("n,mixed", [(F, False), (7, True)])
def test_step_many_equals_single_moving_steps(J, R, n, mixed):
    sc, _ = cases.compiled(cases.moving_ring_dict(J, R))
    E = 257
    a, b = _env(sc, E, seed=9), _env(sc, E, seed=9)
    a.reset(); b.reset()
    rng = np.random.default_rng(n)
    if mixed:   # counters 3 (every third env: reset after 5 steps) and 8: the 7 steps run frames 3..9 and 8..14 side by side
        for t in range(8):
            if t == 5:
                a.reset(_third(E)); b.reset(_third(E))
            Td, Pd = _cuda(*random_actions(rng, E, J, R))
            a.step(Td, Pd); b.step(Td, Pd)
        assert sorted(set(a.step_count.cpu().tolist())) == [3, 8]
    Tn = rng.integers(-1, 2 * R + 3, size=(n, E, J)).astype(np.int32)
    Pn = rng.random((n, E, J)).astype(np.float32)
    Td, Pd = _cuda(Tn, Pn)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    rew_s, term_s, rdpj_s, sum_s = z(n, E), z(n, E, dt=torch.uint8), z(n, E, 3), z(E, 3)
    for t in range(n):
        a.step(Td[t], Pd[t], out_reward=rew_s[t], out_terminated=term_s[t], want_info=False, rdpj_sum=sum_s)
        rdpj_s[t] = a._r_dpj
    rew_m, term_m, rdpj_m, sum_m = z(n, E), z(n, E, dt=torch.uint8), z(n, E, 3), z(E, 3)
    b.step_many(Td, Pd, rew_m, term_m, rdpj_m, rdpj_sum=sum_m)
    assert torch.equal(rew_s, rew_m) and torch.equal(term_s, term_m) and torch.equal(rdpj_s, rdpj_m)
    assert torch.equal(sum_s, sum_m)
    assert torch.equal(a.track, b.track) and torch.equal(a.step_count, b.step_count)
    assert torch.equal(a.get_state(), b.get_state())
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(DEV)
    assert torch.equal(b.positions, pos[torch.clamp(b.step_count.to(torch.int64), max=F)])
    if not mixed:
        assert term_m[-1].all() and not term_m[:-1].any()


def test_step_many_refusals():
    sc, _ = cases.compiled(cases.moving_ring_dict(3, 3))   # generic size: no production variant
    E, J = 8, 3
    env = _env(sc, E)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(Exception, match="production configuration at a compiled size"):
        env.step_many(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3))
    for call in (lambda: env.time_step_kernel(z(E, J, dt=torch.int32), z(E, J), 2),
                 lambda: env.time_step_many_kernel(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8),
                                                   z(4, E, 3), 2)):
        with pytest.raises(RuntimeError, match="not available with a moving scenario"):
            call()
    assert torch.equal(env.step_count, torch.zeros(E, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------
# 5. state rows
@pytest.mark.parametrize("J,R", [(3, 4), (3, 3)])
def test_state_rows_carry_the_next_frames_positions_and_nothing_else_is_touched(J, R):
    sc, _ = cases.compiled(cases.moving_ring_dict(J, R))
    E, S = 130, sc.state_dim
    env = _env(sc, E)
    assert env.observation_is_static is False
    # the state rows inside a NaN-filled buffer: margins of one row before and after
    big = torch.full(((E + 2) * S,), float("nan"), device=DEV)
    rows = big[S:S + E * S].view(E, S)
    rows.copy_(env._state_dyn)
    env._state_dyn = rows
    env._motion_io.state = rows.data_ptr()
    cols = sc.position_columns
    other = [c for c in range(S) if c not in cols]
    static = torch.from_numpy(sc.state_vector()).to(DEV)
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(DEV)

    def check():
        k = torch.clamp(env.step_count.to(torch.int64), max=F)
        assert torch.equal(env.get_state()[:, cols], pos[k]) and torch.equal(env.positions, pos[k])
        assert torch.equal(env.get_state()[:, other], static[other].expand(E, -1))
        assert torch.isnan(big[:S]).all() and torch.isnan(big[S + E * S:]).all()
        assert env.get_state().data_ptr() == rows.data_ptr()
        o = env.get_obs()
        assert tuple(o.shape) == (E, J, S) and torch.equal(o, rows.unsqueeze(1).expand(-1, J, -1))
    env.reset()
    check()
    rng = np.random.default_rng(2)
    for t in range(F + 3):
        if t == 5:
            before = env.get_state().clone()
            m = _third(E)
            env.reset(m)
            keep = ~m.bool()
            assert torch.equal(env.get_state()[keep], before[keep])            # a masked reset rewrites only the masked envs
            assert torch.equal(env.get_state()[m.bool()][:, cols], pos[0].expand(int(m.sum()), -1))
            check()
        env.step(*_cuda(*random_actions(rng, E, J, R)), want_info=bool(t % 2))
        check()
    assert env.step_count.max().item() == F + 3
    with pytest.raises(AttributeError):
        _env(cases.compiled(cases.moving_ring_dict(J, R))[1][0], 4).positions


# ---------------------------------------------------------------------------------------------------------------
# 6. zero velocities: the static scenario
@pytest.mark.parametrize("name", ["3j4r", "6j8r", "3j3r_edge"])
def test_zero_velocity_scenario_equals_the_static_one(name, monkeypatch):
    import json
    from _harness import GOLDEN
    from macjd_amd.scenario import Scenario
    base = json.loads(str(np.load(os.path.join(GOLDEN, f"env_{name}.npz"))["scenario_json"]))
    static = Scenario.from_dict(base, config=cases.config())
    moving = Scenario.from_dict(cases.zero_velocity(base), config=cases.config())
    E, R, J = 257, static.num_radars, static.num_jammers
    with _options(monkeypatch, MACJD_ENV_PD32="0"):
        a, b = _env(static, E, seed=3), _env(moving, E, seed=3)
        a.reset(); b.reset()
        rng = np.random.default_rng(4)
        for t in range(8):
            Td, Pd = _cuda(*random_actions(rng, E, J, R))
            ra, ta, ia = a.step(Td, Pd)
            rb, tb, ib = b.step(Td, Pd)
            assert torch.equal(ta, tb) and torch.equal(a.track, b.track) and torch.equal(a.step_count, b.step_count)
            assert torch.equal(ra, rb) and torch.equal(a._r_dpj, b._r_dpj)
            assert torch.equal(ia["radar_pds"], ib["radar_pds"]) and torch.equal(ia["snr_with_jamming"], ib["snr_with_jamming"])
            assert torch.equal(ib["snr_no_jamming"], ia["snr_no_jamming"].to(torch.float32).expand(E, -1))
            assert torch.equal(b.get_state(), a.get_state())


# ---------------------------------------------------------------------------------------------------------------
# 7. runner, learner, driver
def _runner(sc, E, seed=5):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    env = _env(sc, E, seed=seed)
    info = env.get_env_info()
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=2 * E,
                     epsilon_start=0.6, epsilon_anneal_time=300)
    args.env_info = info
    torch.manual_seed(3)
    with quiet():
        mac = BasicMAC(info["obs_shape"], args)
        mac.cuda()
        buf = EpisodeReplayBuffer(args)
    return BatchedEpisodeRunner(env, mac, buf, args), buf, args


def test_graph_replayed_rollout_equals_eager_stores_the_positions_and_the_learner_trains():
    from macjd_amd.core.qmix import QMixLearner
    cfg, _ = cases.fixture()
    sc, _ = cases.compiled(cfg)
    E = 16
    r_e, b_e, args = _runner(sc, E)
    r_g, b_g, _ = _runner(sc, E)
    # what observation_is_static = False selects: the step loop, no whole-episode launch, no closed-loop launch
    assert not r_e._static and not r_e.hoist_static_obs and not r_e.fused_rollout_available()
    assert not r_e.closed_loop_available() and not r_e.closed_loop_pe_available()
    r_g.enable_graph()
    for _ in range(2):
        r_e.run(sync_stats=True)
        r_g.run(sync_stats=True)
    assert b_e.obs_static is False and b_g.obs_static is False
    for k in b_e.buffers:
        assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
    cols = sc.position_columns
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(b_e.buffers["state"].device)
    for name in ("state", "obs"):
        st = b_e.buffers[name][:2 * E]                       # [2E, T + 1, (J,) S]
        st = st if name == "state" else st[:, :, 0]
        assert torch.equal(st[:, :F][:, :, cols], pos[:F].expand(2 * E, -1, -1)), name
    assert b_e.buffers["terminated"][:2 * E, F - 1].all()
    with quiet():
        learner = QMixLearner(r_e.mac, args)
    stats = learner.train(b_e.sample(8), {})
    assert np.isfinite(float(stats["loss"])) and np.isfinite(float(stats["grad_norm"]))


def test_driver_trains_on_the_moving_scenario(tmp_path):
    from macjd_amd.main import load_config, run
    with contextlib.redirect_stdout(io.StringIO()):
        cfg = load_config("default", os.path.join(PKG, "config"))
    E = 32
    cfg.device_request = "cuda"
    cfg.env_config = "scenario_3j4r_moving"
    cfg.sim_config_path = os.path.join(PKG, "config", "scenario_3j4r_moving.yaml")
    cfg.save_model_dir, cfg.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
    cfg.log_interval_seconds = 0
    cfg.gemm_tuning = False
    cfg.resume = None
    for k, v in dict(batch_envs=E, buffer_size=2 * E, total_env_steps=2 * E * F, episode_limit=F, start_training_steps=0,
                     save_interval=10 ** 9, test_interval=10 ** 9, test_nepisodes=E, batch_size=8, lr=1e-4,
                     updates_per_rollout=4).items():
        setattr(cfg, k, v)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = run(cfg)
    assert res["total_steps"] == 2 * E * F and res["episodes"] == 2 * E and res["train_steps"] > 0
    assert "Training finished." in out.getvalue()
    cfg.randomize_scenarios = True
    with pytest.raises(ValueError, match="--randomize-scenarios is not supported with a moving scenario"):
        with contextlib.redirect_stdout(io.StringIO()):
            run(cfg)


# ---------------------------------------------------------------------------------------------------------------
# 8. the single-env facade
@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_facade_returns_the_moving_state_step_by_step(mode):
    from macjd_amd.simulation.environment import ElectromagneticEnvironment
    cfg, g = cases.fixture()
    path = os.path.join(PKG, "config", "scenario_3j4r_moving.yaml")
    with contextlib.redirect_stdout(io.StringIO()):
        env = ElectromagneticEnvironment(SimpleNamespace(), path)
    pre = f"{mode}_s42_"
    T, P = g[pre + "T"], g[pre + "P"]
    J = T.shape[1]
    np.random.seed(42)
    s0 = env.reset()
    assert s0.tobytes() == g[pre + "obs_reset"].tobytes()
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(T.shape[0]):
            if mode == "f32":
                acts = [(np.int64(T[k, i]), np.float32(P[k, i])) for i in range(J)]
            else:
                acts = [(int(T[k, i]), float(P[k, i])) for i in range(J)]
            obs, rew, term, info = env.step(acts)
            assert len(obs) == J and all(o.tobytes() == g[pre + "obs_after"][k].tobytes() for o in obs), k
            assert env.get_state().tobytes() == g[pre + "obs_after"][k].tobytes()
            assert [s["is_tracking"] for s in info["radar_states"]] == g[pre + "track"][k].astype(bool).tolist(), k
            assert term == bool(g[pre + "terminated"][k])
            assert rew == pytest.approx(g[pre + "reward"][k], rel=1e-9, abs=1e-12)
            np.testing.assert_array_equal(info["snr_no_jamming"], g[pre + "snr_no"][k])
            np.testing.assert_allclose(info["radar_pds"], g[pre + "pd"][k], rtol=1e-12, atol=0)
            prj = np.full(J, -1.0)
            for a in info["jammer_actions"]:
                prj[a["jammer_idx"]] = a["received_power"]
            np.testing.assert_allclose(prj, g[pre + "prj"][k], rtol=1e-14, atol=0)
