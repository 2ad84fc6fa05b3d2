"""Scanning radars on the GPU (include/macjd.h, macjd_env_step_scan): reduction to today's kernel where the model
reduces to it, the kernel against the NumPy restatement (tests/scan_model.py), the dynamic observation, the runner's
rollouts, the single-env facade and the guard rails."""
import contextlib
import copy
import io
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import scan_model
from _harness import GOLDEN, REPO, oracle_lib, random_actions
from test_nets_cpu import make_args, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")


def _base(name):
    return json.loads(str(np.load(os.path.join(GOLDEN, f"env_{name}.npz"))["scenario_json"]))


def _scan_dict(d, step_seconds=0.25, sidelobe_db=-30.0, **radar_kw):
    d = copy.deepcopy(d)
    d.setdefault("environment_params", {})["radar_scan"] = {"step_seconds": step_seconds, "sidelobe_db": sidelobe_db}
    for r in d["radars"]:
        r.update(radar_kw)
    return d


def _sc(d):
    from macjd_amd.scenario import Scenario
    return Scenario.from_dict(d)


def _env(sc, E, seed=11):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=seed)


def _diag(E, R, J):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    return {"out64": z(E, 4), "pd64": z(E, R), "snr64": z(E, R), "prj64": z(E, J)}


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


def _cuda(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


# ---------------------------------------------------------------------------------------------------------------
# 1. reduction to today's kernel
@pytest.mark.parametrize("name", ["2j2r_shipped", "3j4r", "12j16r", "3j3r_edge"])
@pytest.mark.parametrize("case", ["unit_sidelobe", "wide_beam"])
@pytest.mark.parametrize("uniforms", ["philox", "supplied"])
def test_reduces_bitwise_to_the_static_kernel(name, case, uniforms):
    base = _base(name)
    if case == "unit_sidelobe":
        d = _scan_dict(base, 0.25, 0.0, theta_m=3.0, t_s=5.0)
    else:   # sweep + 2 h >= 360: every radar always sees everything through its main lobe
        d = _scan_dict(base, 0.25, -30.0, theta_m=40.0, t_s=0.27)
    sc_s, sc_0 = _sc(d), _sc(base)
    if case == "wide_beam":
        assert sc_s.scan_tables["full"].all()
    E, R, J = 300, sc_0.num_radars, sc_0.num_jammers
    es, e0 = _env(sc_s, E), _env(sc_0, E)
    for env in (es, e0):
        env.kernel_flags = 2   # lane kernel for both
        env.reset()
    st = sc_s.scan_tables
    theta = np.tile(st["az0"], (E, 1))
    rng = np.random.default_rng(len(name))
    ds, d0 = _diag(E, R, J), _diag(E, R, J)
    for t in range(200):
        if t % 37 == 36:
            mask = rng.random(E) < 0.3
            for env in (es, e0):
                env.reset(torch.from_numpy(mask.astype(np.uint8)).to(DEV))
            theta[mask] = st["az0"]
        T, P = random_actions(rng, E, J, R)
        s_prev = es.track.cpu().numpy().astype(bool)
        if uniforms == "supplied":
            u = _cuda(rng.random((E, R + J)))[0]
            P64 = _cuda(P.astype(np.float64))[0]
            T_d, = _cuda(T)
            rs, ts, is_ = es.step(T_d, P64, u, diag=ds)
            r0, t0, i0 = e0.step(T_d, P64, u, diag=d0)
        else:
            T_d, P_d = _cuda(T, P)
            rs, ts, is_ = es.step(T_d, P_d)
            r0, t0, i0 = e0.step(T_d, P_d)
        assert torch.equal(is_["radar_tracking"], i0["radar_tracking"])
        assert torch.equal(ts, t0) and torch.equal(is_["step_count"], i0["step_count"])
        assert torch.equal(rs, r0)
        for k in ("r_d", "r_p", "r_j", "radar_pds", "snr_with_jamming"):
            assert torch.equal(is_[k], i0[k]), k
        if uniforms == "supplied":
            for k in ds:
                assert torch.equal(ds[k], d0[k]), k
        # closed-form beam advance
        det = is_["radar_tracking"].cpu().numpy().astype(bool)
        x = theta + st["sweep_mod"]
        x = np.where(x >= 360.0, x - 360.0, x)
        theta = np.where(det, st["bear_tgt"], np.where(s_prev, theta, x))
        assert es.beam_azimuth.cpu().numpy().tobytes() == theta.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 2. against the restatement
def _restatement_scenarios():
    out = {}
    for name in ("3j4r", "6j8r"):
        out[name] = _scan_dict(_base(name), 0.25, -30.0)
    # one jammer sitting inside radar 0's beam toward the target, one well outside it
    d = _scan_dict(_base("3j4r"), 0.25, -30.0)
    rx, ry = d["radars"][0]["position"]
    d["jammers"][0]["position"] = [rx * 0.5, ry * 0.5 + 1.0]     # on the radar -> target line (bearing ~ target's)
    d["jammers"][1]["position"] = [rx * 0.5, ry * 0.5 + 150.0]   # ~37 degrees off it
    out["3j4r_inline"] = d
    return out


SCN = _restatement_scenarios()


def _run_vs_model(sc, E, steps, P_f64, diag_tol, seed):
    R, J = sc.num_radars, sc.num_jammers
    env, m = _env(sc, E), scan_model.ScanModel(sc, E)
    env.reset()
    rng = np.random.default_rng(seed)
    dg = _diag(E, R, J)
    for t in range(steps):
        if t % 41 == 40:
            mask = rng.random(E) < 0.4
            env.reset(torch.from_numpy(mask.astype(np.uint8)).to(DEV))
            m.reset(mask)
        T, P = random_actions(rng, E, J, R)
        u = rng.random((E, R + J))
        P_use = P.astype(np.float64) if P_f64 else P
        T_d, P_d, u_d = _cuda(T, P_use, u)
        _, term, info = env.step(T_d, P_d, u_d, diag=dg)
        o = m.step(T, P_use, u, arith32=not P_f64)
        np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
        np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
        assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
        np.testing.assert_array_equal(info["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
        if diag_tol:
            np.testing.assert_allclose(dg["pd64"].cpu().numpy(), o["pd"], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(dg["snr64"].cpu().numpy(), o["snr"], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(dg["prj64"].cpu().numpy(), o["prj"], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(dg["out64"].cpu().numpy(), o["out"], rtol=0, atol=1e-9)
    return m


@pytest.mark.parametrize("name", sorted(SCN))
@pytest.mark.parametrize("E", [1, 257, 4096])
@pytest.mark.parametrize("regular", ["1", "0"])
def test_kernel_vs_restatement_supplied_uniforms(name, E, regular, monkeypatch):
    sc = _sc(SCN[name])
    with _options(monkeypatch, MACJD_ENV_PD32="0", MACJD_ENV_REGULAR=regular):
        m = _run_vs_model(sc, E, 300, True, True, seed=E + len(name))
    if E >= 257:
        assert m.count_target.min() > 0 and m.count_jammer.min() > 0, (m.count_target, m.count_jammer)


@pytest.mark.parametrize("name", ["3j4r", "6j8r", "3j4r_inline"])
def test_restatement_jammer_lobes_and_float32_actions(name):
    sc = _sc(SCN[name])
    m = _run_vs_model(sc, 257, 120, False, False, seed=7)
    assert m.count_target.min() > 0 and m.count_jammer.min() > 0
    if name == "3j4r_inline":
        # the jammer on radar 0's line of sight is in its main lobe whenever the target is
        d = scan_model.derive(sc)
        assert abs(d["bj"][0, 0] - d["bt"][0]) < sc.radars[0]["theta_m"] / 2
        assert abs(d["bj"][1, 0] - d["bt"][0]) > 20.0


def _production_vs_model(name, monkeypatch, **options):
    sc = _sc(SCN[name])
    R, J, E = sc.num_radars, sc.num_jammers, 65
    lib = oracle_lib()
    with _options(monkeypatch, **options):
        env, m = _env(sc, E, seed=123), scan_model.ScanModel(sc, E)
        env.reset()
        rng = np.random.default_rng(3)
        for t in range(60):
            T, P = random_actions(rng, E, J, R)
            ep = env.episode_index.cpu().numpy()
            u = np.array([[lib.macjd_oracle_uniform(123, e, int(ep[e]), t, k) for k in range(R + J)] for e in range(E)])
            T_d, P_d = _cuda(T, P)
            rew, term, info = env.step(T_d, P_d)
            o = m.step(T, P, u, arith32=True)
            np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
            np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
            assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
            np.testing.assert_allclose(rew.cpu().numpy(), o["out"][:, 0], rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", ["3j4r", "6j8r"])
@pytest.mark.parametrize("pd32", ["1", "0"])
def test_default_production_variants_vs_restatement(name, pd32, monkeypatch):
    """Philox uniforms and float32 actions (the production variants): the restatement is driven with the same Philox
    values (the oracle's generator); integer outputs bit-exact, rewards within 1e-5."""
    _production_vs_model(name, monkeypatch, MACJD_ENV_PD32=pd32)


def test_ieee_division_production_variant_vs_restatement(monkeypatch):
    """MACJD_ENV_REGULAR=0 under Philox uniforms and float32 actions: the production variant that keeps IEEE divisions and
    every guard (the other tests of that switch supply uniforms, which selects the general variant); same bars."""
    _production_vs_model("3j4r", monkeypatch, MACJD_ENV_REGULAR="0")


# ---------------------------------------------------------------------------------------------------------------
# 3. state and observation
def test_state_and_observation_follow_the_beams():
    sc = _sc(SCN["3j4r"])
    E, R, J = 128, sc.num_radars, sc.num_jammers
    env = _env(sc, E)
    assert env.observation_is_static is False
    st0 = env.reset()
    ptr = env.get_state().data_ptr()
    static = torch.from_numpy(sc.state_vector()).to(DEV)
    cols = sc.theta_a_columns
    other = [c for c in range(sc.state_dim) if c not in cols]
    rng = np.random.default_rng(1)
    seen = set()
    for t in range(50):
        T, P = random_actions(rng, E, J, R)
        env.step(*_cuda(T, P))
        s = env.get_state()
        assert s.data_ptr() == ptr and st0.data_ptr() == ptr
        assert torch.equal(s[:, cols], env.beam_azimuth.to(torch.float32))
        assert torch.equal(s[:, other], static[other].expand(E, -1))
        o = env.get_obs()
        assert tuple(o.shape) == (E, J, sc.state_dim) and torch.equal(o, s.unsqueeze(1).expand(-1, J, -1))
        seen.add(s[0, cols[0]].item())
    assert len(seen) > 5
    env.reset()
    assert torch.equal(env.get_state()[:, cols], torch.from_numpy(sc.scan_tables["az0"]).to(DEV, torch.float32).expand(E, -1))


# ---------------------------------------------------------------------------------------------------------------
# 4. rollouts
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


def test_graph_replayed_rollout_equals_eager_and_stores_the_moving_beams():
    from macjd_amd.scenario import Scenario
    sc = Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_scan.yaml"))
    E = 256
    r_e, b_e, _ = _runner(sc, E)
    r_g, b_g, _ = _runner(sc, E)
    assert not r_e.hoist_static_obs and not r_e.fused_rollout_available()
    r_g.enable_graph()
    for _ in range(2):
        r_e.run(sync_stats=True)
        r_g.run(sync_stats=True)
    assert b_e.obs_static is False and b_g.obs_static is False
    for k in b_e.buffers:
        assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
    # the stored theta_a columns move over t and replay the restatement driven by the stored actions
    cols = sc.theta_a_columns
    T = sc.episode_limit
    state = b_e.buffers["state"][:E].cpu().numpy()              # [E, T+1, S] of the first episode batch
    assert np.unique(state[:, :T, cols[0]]).size > 5
    np.testing.assert_array_equal(state[:, 0, cols], np.tile(sc.scan_tables["az0"].astype(np.float32), (E, 1)))
    # every stored step follows the beam rule: a' = bt (detected, or a tracking beam staying on the target), else the
    # sweep advance of the float64 azimuth
    d = scan_model.derive(sc)
    term = b_e.buffers["terminated"][:E].cpu().numpy()
    a64 = np.tile(d["az0"], (E, 1))
    n_bt = 0
    for t in range(T - 1):
        a_next = state[:, t + 1, cols]
        x = a64 + d["swm"]
        x = np.where(x >= 360.0, x - 360.0, x)
        on_t = a_next == d["bt"].astype(np.float32)
        np.testing.assert_array_equal(a_next[~on_t], x.astype(np.float32)[~on_t])
        a64 = np.where(on_t, d["bt"], x)
        n_bt += int(on_t.sum())
    assert n_bt > 0
    assert term[:, T - 1].all()


# ---------------------------------------------------------------------------------------------------------------
# 6. facade
def test_facade_matches_the_restatement_on_the_global_stream():
    from macjd_amd.scenario import Scenario
    from macjd_amd.simulation.environment import ElectromagneticEnvironment
    path = os.path.join(PKG, "config", "scenario_3j4r_scan.yaml")
    with contextlib.redirect_stdout(io.StringIO()):
        env = ElectromagneticEnvironment(SimpleNamespace(), path)
    sc = Scenario.from_yaml(path)
    R, J = sc.num_radars, sc.num_jammers
    m = scan_model.ScanModel(sc, 1)
    rng = np.random.default_rng(9)
    acts = [[(int(rng.integers(0, 2 * R + 1)), float(rng.random())) for _ in range(J)] for _ in range(100)]
    s0 = env.reset()
    np.testing.assert_array_equal(s0[sc.theta_a_columns], sc.scan_tables["az0"].astype(np.float32))
    np.random.seed(17)
    outs = []
    with contextlib.redirect_stdout(io.StringIO()):
        for a in acts:
            outs.append(env.step(a))
    np.random.seed(17)
    for a, (obs, rew, term, info) in zip(acts, outs):
        T = np.array([[x[0] for x in a]])
        P = np.array([[x[1] for x in a]], dtype=np.float64)
        o = m.step(T, P, m.draw_uniforms(T, P))
        assert [st["is_tracking"] for st in info["radar_states"]] == o["track"][0].tolist()
        assert info["radar_beam_azimuth"].tobytes() == o["theta_a"][0].tobytes()
        np.testing.assert_array_equal(obs[0][sc.theta_a_columns], o["theta_a"][0].astype(np.float32))
        np.testing.assert_array_equal(info["snr_no_jamming"], o["snr_no"][0])
        np.testing.assert_allclose(info["radar_pds"], o["pd"][0], rtol=1e-12)
        assert rew == pytest.approx(o["out"][0, 0], rel=0, abs=1e-9)
        assert term == bool(o["terminated"][0])
    assert set(outs[0][3]) >= {"radar_pds", "radar_states", "snr_no_jamming", "snr_with_jamming", "r_d", "r_p", "r_j",
                               "jammer_actions", "radar_beam_azimuth"}
    np.testing.assert_array_equal(env.get_state()[sc.theta_a_columns], m.theta_a[0].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
# 7. guard rails and the driver
def test_guard_rails():
    from macjd_amd.scenario import ScenarioBatch
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    sc = _sc(SCN["3j4r"])
    E, J = 64, sc.num_jammers
    env = _env(sc, E)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="scanning"):
        env.step_many(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3))
    with pytest.raises(ValueError):
        ScenarioBatch([sc])
    batch = copy.copy(ScenarioBatch([_sc(_base("3j4r"))] * 2))
    batch.base = sc   # a batch that slipped a scanning scenario past ScenarioBatch's own check
    with pytest.raises(ValueError, match="scanning"):
        BatchedElectromagneticEnvironment(batch_envs=2, device=DEV, scenario_batch=batch)
    with pytest.raises(AttributeError):
        _env(_sc(_base("3j4r")), 4).beam_azimuth


def test_driver_trains_on_the_scan_scenario(tmp_path):
    from macjd_amd.main import load_config, run
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
    assert res["total_steps"] == 2 * E * 100 and res["episodes"] == 2 * E and res["train_steps"] > 0
    assert "Training finished." in out.getvalue()
