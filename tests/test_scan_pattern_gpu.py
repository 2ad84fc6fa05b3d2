"""Stepped antenna pattern of scanning radars on the GPU (include/macjd.h, macjd_scan_pattern_desc): bitwise reduction to
the two-level and the static kernels where the model reduces to them, the one-step kernels and the closed-loop episode
kernel against the NumPy restatement (tests/scan_pattern_model.py), the single-env facade, the guard rails and the driver.

Bars: integer outputs and azimuth bytes exact, snr_no equal as float32, float64 diagnostics rtol 1e-12 (out64 atol 1e-9),
rewards of the production variants within 1e-5 — those of tests/test_scan_gpu.py and tests/test_episode_scan_gpu.py."""
import contextlib
import ctypes
import functools
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import scan_pattern_model as spm
from _harness import oracle_lib, random_actions
from test_episode_scan_gpu import _check_agent_half, _check_env_half_and_hand_over, _closed
from test_scan_gpu import DEV, PKG, _base, _cuda, _diag, _env, _options, _runner, _sc
from test_scan_pattern_cpu import GAINS4, GAINS6, pattern_dict

pytestmark = pytest.mark.gpu
YAML = os.path.join(PKG, "config", "scenario_3j4r_scan_pattern.yaml")


def _yaml_sc():
    from macjd_amd.scenario import Scenario
    return Scenario.from_yaml(YAML)


# ---------------------------------------------------------------------------------------------------------------
# (a) reductions
def _step_both(ea, eb, rng, E, R, J, uniforms, da, db):
    T, P = random_actions(rng, E, J, R)
    if uniforms == "supplied":
        T_d, P_d, u = _cuda(T, P.astype(np.float64), rng.random((E, R + J)))
        return ea.step(T_d, P_d, u, diag=da), eb.step(T_d, P_d, u, diag=db)
    T_d, P_d = _cuda(T, P)
    return ea.step(T_d, P_d), eb.step(T_d, P_d)


@pytest.mark.parametrize("name", ["2j2r_shipped", "3j4r", "12j16r", "3j3r_edge"])
@pytest.mark.parametrize("uniforms", ["philox", "supplied"])
def test_equal_gains_reduce_bitwise_to_the_two_level_kernel(name, uniforms):
    sc_p = _sc(pattern_dict(name, gain_db=[-30.0] * 3, sidelobe_db=-30.0))
    sc_0 = _sc(pattern_dict(name, pattern=False, sidelobe_db=-30.0))
    assert sc_p.scan_pattern_levels == 3 and sc_0.scan_pattern_levels == 0
    E, R, J = 300, sc_0.num_radars, sc_0.num_jammers
    ep, e0 = _env(sc_p, E), _env(sc_0, E)
    for env in (ep, e0):
        env.reset()
    rng = np.random.default_rng(len(name))
    dp, d0 = _diag(E, R, J), _diag(E, R, J)
    for t in range(100):
        if t % 37 == 36:
            mask = torch.from_numpy((rng.random(E) < 0.3).astype(np.uint8)).to(DEV)
            for env in (ep, e0):
                env.reset(mask)
        (rp, tp, ip), (r0, t0, i0) = _step_both(ep, e0, rng, E, R, J, uniforms, dp, d0)
        assert torch.equal(rp, r0) and torch.equal(tp, t0)
        for k in ("radar_tracking", "step_count", "r_d", "r_p", "r_j", "radar_pds", "snr_with_jamming", "snr_no_jamming"):
            assert torch.equal(ip[k], i0[k]), (k, t)
        assert torch.equal(ep.beam_azimuth, e0.beam_azimuth) and torch.equal(ep.get_state(), e0.get_state())
        if uniforms == "supplied":
            for k in dp:
                assert torch.equal(dp[k], d0[k]), (k, t)
    assert len(torch.unique(ep.beam_azimuth)) > 5


@pytest.mark.parametrize("name", ["2j2r_shipped", "3j4r", "12j16r", "3j3r_edge"])
@pytest.mark.parametrize("uniforms", ["philox", "supplied"])
def test_unit_gains_reduce_bitwise_to_the_static_kernel(name, uniforms):
    d = pattern_dict(name, gain_db=[0.0] * 3, sidelobe_db=0.0, cycle=False)
    for r in d["radars"]:
        r.update(theta_m=3.0, t_s=5.0)
    sc_p, sc_0 = _sc(d), _sc(_base(name))
    E, R, J = 300, sc_0.num_radars, sc_0.num_jammers
    ep, e0 = _env(sc_p, E), _env(sc_0, E)
    for env in (ep, e0):
        env.kernel_flags = 2   # lane kernel for both
        env.reset()
    rng = np.random.default_rng(len(name) + 1)
    dp, d0 = _diag(E, R, J), _diag(E, R, J)
    for t in range(100):
        if t % 37 == 36:
            mask = torch.from_numpy((rng.random(E) < 0.3).astype(np.uint8)).to(DEV)
            for env in (ep, e0):
                env.reset(mask)
        (rp, tp, ip), (r0, t0, i0) = _step_both(ep, e0, rng, E, R, J, uniforms, dp, d0)
        assert torch.equal(rp, r0) and torch.equal(tp, t0)
        for k in ("radar_tracking", "step_count", "r_d", "r_p", "r_j", "radar_pds", "snr_with_jamming"):
            assert torch.equal(ip[k], i0[k]), (k, t)
        if uniforms == "supplied":
            for k in dp:
                assert torch.equal(dp[k], d0[k]), (k, t)


# ---------------------------------------------------------------------------------------------------------------
# (b) against the restatement, supplied uniforms, float64 diagnostics
B_SCN = {"3j4r": ("3j4r", GAINS4), "6j8r": ("6j8r", GAINS6), "3j3r_edge": ("3j3r_edge", GAINS4)}


@functools.lru_cache(maxsize=None)
def _reference_run(name, E, steps=120):
    """One restatement run per (scenario, E), shared by the kernel variants: inputs and expected outputs per step."""
    sc = _sc(pattern_dict(*B_SCN[name]))
    R, J = sc.num_radars, sc.num_jammers
    m = spm.ScanPatternModel(sc, E)
    rng = np.random.default_rng(E + len(name))
    rec = []
    for t in range(steps):
        mask = None
        if t % 41 == 40:
            mask = rng.random(E) < 0.4
            m.reset(mask)
        T, P = random_actions(rng, E, J, R)
        P = P.astype(np.float64)
        u = rng.random((E, R + J))
        rec.append((mask, T, P, u, m.step(T, P, u)))
    return sc, rec, m.count_target.copy(), m.count_jammer.copy()


@pytest.mark.parametrize("name", sorted(B_SCN))
@pytest.mark.parametrize("E", [1, 257])
@pytest.mark.parametrize("regular", ["1", "0"])
def test_kernel_vs_restatement_supplied_uniforms(name, E, regular, monkeypatch):
    sc, rec, count_t, count_j = _reference_run(name, E)
    R, J = sc.num_radars, sc.num_jammers
    with _options(monkeypatch, MACJD_ENV_PD32="0", MACJD_ENV_REGULAR=regular):
        env = _env(sc, E)
        env.reset()
        dg = _diag(E, R, J)
        for mask, T, P, u, o in rec:
            if mask is not None:
                env.reset(torch.from_numpy(mask.astype(np.uint8)).to(DEV))
            _, term, info = env.step(*_cuda(T, P, u), diag=dg)
            np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
            np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
            assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
            np.testing.assert_array_equal(info["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
            np.testing.assert_allclose(dg["pd64"].cpu().numpy(), o["pd"], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(dg["snr64"].cpu().numpy(), o["snr"], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(dg["prj64"].cpu().numpy(), o["prj"], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(dg["out64"].cpu().numpy(), o["out"], rtol=0, atol=1e-9)
    if E == 257:
        print(f"{name}: level counts target {count_t.tolist()} jammer {count_j.tolist()}")
        assert count_t.min() > 0 and count_j.min() > 0, (count_t, count_j)


# ---------------------------------------------------------------------------------------------------------------
# (c) production variants
@pytest.mark.parametrize("name,gains", [("3j4r", GAINS4), ("6j8r", GAINS6), ("12j16r", GAINS4), ("2j2r_shipped", GAINS4)])
@pytest.mark.parametrize("pd32", ["1", "0"])
def test_production_variants_vs_restatement(name, gains, pd32, monkeypatch):
    """Philox uniforms and float32 actions: the restatement is driven with the same Philox values (the oracle's
    generator); integer outputs and azimuths bit-exact, rewards within 1e-5."""
    sc = _sc(pattern_dict(name, gains))
    R, J, E = sc.num_radars, sc.num_jammers, 65
    lib = oracle_lib()
    with _options(monkeypatch, MACJD_ENV_PD32=pd32):
        env, m = _env(sc, E, seed=123), spm.ScanPatternModel(sc, E)
        assert env.scenario_regular
        env.reset()
        rng = np.random.default_rng(3)
        for t in range(60):
            T, P = random_actions(rng, E, J, R)
            ep = env.episode_index.cpu().numpy()
            u = np.array([[lib.macjd_oracle_uniform(123, e, int(ep[e]), t, k) for k in range(R + J)] for e in range(E)])
            rew, term, info = env.step(*_cuda(T, P))
            o = m.step(T, P, u, arith32=True)
            np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
            np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
            assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
            np.testing.assert_array_equal(info["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
            np.testing.assert_allclose(rew.cpu().numpy(), o["out"][:, 0], rtol=0, atol=1e-5)
    assert np.count_nonzero(m.count_target) >= 3 and np.count_nonzero(m.count_jammer) >= 3


# ---------------------------------------------------------------------------------------------------------------
# (d) closed loop
@pytest.mark.parametrize("E", [16, 257])
def test_closed_loop_on_the_pattern_scenario(E):
    sc = _yaml_sc()
    r = _check_env_half_and_hand_over(sc, E, False)
    _check_agent_half(r, sc, E, False)


def test_closed_loop_2j2r_pattern():
    sc = _sc(pattern_dict("2j2r_shipped", GAINS4))
    r = _check_env_half_and_hand_over(sc, 300, False)
    _check_agent_half(r, sc, 300, False)


def test_closed_loop_env_half_vs_restatement():
    """The episode kernel's env half against the restatement, driven with the stored actions and the oracle's Philox
    uniforms; the hand-over's snr_no is the last step's level value."""
    sc = _sc(pattern_dict("3j4r", GAINS4))
    R, J, E, n = sc.num_radars, sc.num_jammers, 65, 60
    cols = sc.theta_a_columns
    lib = oracle_lib()
    r, _, _ = _closed(sc, E, False, n_steps=n, seed=123)
    st = r.stage
    m = spm.ScanPatternModel(sc, E)
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
    np.testing.assert_array_equal(r.env._snr_no_step.t().cpu().numpy(), o["snr_no"].astype(np.float32))
    assert np.count_nonzero(m.count_target) >= 3 and np.count_nonzero(m.count_jammer) >= 3


def test_graph_replay_equals_eager_closed_loop_on_the_pattern_scenario():
    sc = _yaml_sc()
    E = 256
    r_e, b_e, _ = _runner(sc, E)
    r_g, b_g, _ = _runner(sc, E)
    r_e.closed_loop_rollout = r_g.closed_loop_rollout = True
    assert r_e.closed_loop_available()
    r_g.enable_graph()
    try:
        s_e = r_e.run(sync_stats=True)
        s_g = r_g.run(sync_stats=True)
        assert s_e["episode_return"] == s_g["episode_return"]
        for k in b_e.buffers:
            assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(r_e.mac.hidden_states, r_g.mac.hidden_states)
    finally:
        r_g.release_graphs()


# ---------------------------------------------------------------------------------------------------------------
# (e) facade
def test_facade_matches_the_restatement_on_the_global_stream():
    from macjd_amd.simulation.environment import ElectromagneticEnvironment
    with contextlib.redirect_stdout(io.StringIO()):
        env = ElectromagneticEnvironment(SimpleNamespace(), YAML)
    sc = _yaml_sc()
    R, J = sc.num_radars, sc.num_jammers
    m = spm.ScanPatternModel(sc, 1)
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
    levels = set()
    for a, (obs, rew, term, info) in zip(acts, outs):
        T = np.array([[x[0] for x in a]])
        P = np.array([[x[1] for x in a]], dtype=np.float64)
        o = m.step(T, P, m.draw_uniforms(T, P))
        levels |= set(o["level_target"][0].tolist())
        assert [st["is_tracking"] for st in info["radar_states"]] == o["track"][0].tolist()
        assert info["radar_beam_azimuth"].tobytes() == o["theta_a"][0].tobytes()
        np.testing.assert_array_equal(obs[0][sc.theta_a_columns], o["theta_a"][0].astype(np.float32))
        assert info["snr_no_jamming"].dtype == np.float64
        np.testing.assert_array_equal(info["snr_no_jamming"], o["snr_no"][0])      # the level's float64 table value
        np.testing.assert_allclose(info["radar_pds"], o["pd"][0], rtol=1e-12)
        rec = [j for j in range(J) if o["prj"][0, j] >= 0.0]
        assert [ja["jammer_idx"] for ja in info["jammer_actions"]] == rec
        np.testing.assert_allclose([ja["received_power"] for ja in info["jammer_actions"]], o["prj"][0, rec], rtol=1e-12)
        assert rew == pytest.approx(o["out"][0, 0], rel=0, abs=1e-9)
        assert term == bool(o["terminated"][0])
    assert len(levels) >= 4, levels   # main, side and pattern levels all handed out
    np.testing.assert_array_equal(env.get_state()[sc.theta_a_columns], m.theta_a[0].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
# (f) guard rails
def test_setter_guard_rails():
    from macjd_amd import _native
    lib = _native.load()
    EINVAL = -1
    sc = _sc(pattern_dict())
    good, keep = sc.c_scan_pattern_desc()

    def call(handle, desc):
        return lib.macjd_scenario_set_scan_pattern(handle.ptr, ctypes.byref(desc))

    def variant(**kw):
        d = _native.ScanPatternDesc()
        for n, *_ in _native.ScanPatternDesc._fields_:
            setattr(d, n, getattr(good, n))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    with torch.cuda.device(DEV):
        h_static = _native.ScenarioHandle(_sc(_base("3j4r")))           # no scan tables yet
        assert call(h_static, good) == EINVAL and b"macjd_scenario_set_scan" in lib.macjd_last_error()
        h = _native.ScenarioHandle(_sc(pattern_dict(pattern=False)))    # scanning, no pattern
        for bad, word in ((variant(n_levels=0), b"n_levels"), (variant(n_levels=7), b"n_levels"),
                          (variant(n_radars=3), b"n_radars"), (variant(gr_lvl=None), b"NULL"),
                          (variant(inv_width=None), b"NULL"), (variant(GaPs_lvl=None), b"NULL")):
            assert call(h, bad) == EINVAL
            assert word in lib.macjd_last_error(), lib.macjd_last_error()
        assert lib.macjd_scenario_set_scan_pattern(None, ctypes.byref(good)) == EINVAL
        assert lib.macjd_scenario_set_scan_pattern(h.ptr, None) == EINVAL
        zero = np.zeros(sc.num_radars)
        assert call(h, variant(inv_width=zero.ctypes.data)) == EINVAL and b"inv_width" in lib.macjd_last_error()
        assert call(h, good) == 0
        h.close()
        h_static.close()
    del keep


def test_a_handle_without_pattern_tables_is_today_s_two_level_env():
    """No ``pattern`` key, and a handle whose setter call was refused: the two-level model (the restatement with L = 0);
    the pattern scenario on the same inputs differs from it."""
    from macjd_amd import _native
    lib = _native.load()
    sc_0, sc_p = _sc(pattern_dict(pattern=False)), _sc(pattern_dict())
    E, R, J = 257, sc_0.num_radars, sc_0.num_jammers
    e0, e_refused, ep = _env(sc_0, E), _env(sc_0, E), _env(sc_p, E)
    bad, keep = sc_p.c_scan_pattern_desc()
    bad.n_levels = 7
    assert lib.macjd_scenario_set_scan_pattern(e_refused._handle.ptr, ctypes.byref(bad)) == -1
    m = spm.ScanPatternModel(sc_0, E)
    assert m.L == 0
    for env in (e0, e_refused, ep):
        env.reset()
    rng = np.random.default_rng(4)
    differs = False
    for t in range(40):
        T, P = random_actions(rng, E, J, R)
        u = rng.random((E, R + J))
        args = _cuda(T, P.astype(np.float64), u)
        o = m.step(T, P.astype(np.float64), u)
        d0, d1 = _diag(E, R, J), _diag(E, R, J)
        _, _, i0 = e0.step(*args, diag=d0)
        _, _, i1 = e_refused.step(*args, diag=d1)
        np.testing.assert_array_equal(i0["radar_tracking"].cpu().numpy().astype(bool), o["track"])
        assert e0.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
        np.testing.assert_array_equal(i0["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
        np.testing.assert_allclose(d0["out64"].cpu().numpy(), o["out"], rtol=0, atol=1e-9)
        for k in d0:
            assert torch.equal(d0[k], d1[k]), k
        assert torch.equal(e0.beam_azimuth, e_refused.beam_azimuth)
        _, _, ip = ep.step(*args)   # (its own trajectory: the near levels show in the SNR without jamming)
        differs = differs or not torch.equal(ip["snr_no_jamming"], i0["snr_no_jamming"])
    assert differs
    del keep


# ---------------------------------------------------------------------------------------------------------------
# (g) the driver
def test_driver_trains_on_the_pattern_scenario(tmp_path):
    from macjd_amd.main import load_config, run
    with contextlib.redirect_stdout(io.StringIO()):
        cfg = load_config("default", os.path.join(PKG, "config"))
    E = 64
    cfg.device_request = "cuda"
    cfg.sim_config_path = YAML
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
