"""Stepped antenna pattern on per-env scanning scenario batches on the GPU (include/macjd.h, macjd_env_step_scan_pe_pattern):
the batch against 40 single-scenario pattern environments, against the NumPy restatement (tests/scan_pattern_model.py) per
env in both table layouts, the production variant against the general one, a degenerate pattern against the pattern-free
per-env kernel, the entry point's argument errors, and the runner / driver on a domain-randomised pattern batch.  Inputs:
tests/scan_pe_pattern_cases.py (the CPU file checks the model's coverage of every level on them)."""
import contextlib
import ctypes
import functools
import io
import os
import re

import numpy as np
import pytest
import torch
import yaml

import scan_pattern_model as spm
import scan_pe_pattern_cases as cases
from _harness import REPO, random_actions
from test_nets_cpu import make_args, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
INFO_KEYS = ("r_d", "r_p", "r_j", "radar_tracking", "radar_pds", "snr_with_jamming", "snr_no_jamming")


def _pe_env(batch, seed=11, env_offset=0):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return BatchedElectromagneticEnvironment(scenario_batch=batch, device=DEV, seed=seed, env_offset=env_offset)


def _cuda(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _diag(E, R, J):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    return {"out64": z(E, 4), "pd64": z(E, R), "snr64": z(E, R), "prj64": z(E, J)}


def _bits_equal(a, b):
    """Bitwise equality of two float tensors, NaNs equal to NaNs (a NaN power action propagates into r_p and the reward;
    its payload is not part of the model)."""
    a, b = a.contiguous(), b.contiguous()
    if not torch.equal(a.isnan(), b.isnan()):
        return False
    iv = torch.int32 if a.dtype == torch.float32 else torch.int64
    z = torch.zeros((), dtype=a.dtype, device=a.device)
    return torch.equal(torch.where(a.isnan(), z, a).view(iv), torch.where(b.isnan(), z, b).view(iv))


# ---------------------------------------------------------------------------------------------------------------
# 1. the batch equals single-scenario pattern environments
@pytest.mark.parametrize("pd32", ["0", None])
def test_batch_equals_single_scenario_pattern_environments(pd32, monkeypatch):
    """Env e of the batch == a single-scenario pattern environment of scenario e (shared-table PAT kernel, the handle's own
    level tables) with the same global env index.  MACJD_ENV_PD32=0: every output bitwise.  Default: the single envs run the
    PD32 production variant — integers, beams and state columns bitwise, rewards within (R + J) 6e-7, the PD32 bound of
    csrc/macjd_env_step.h."""
    from macjd_amd import _native
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    if pd32 is not None:
        monkeypatch.setenv("MACJD_ENV_PD32", pd32)
    _native.reload_options()
    c = cases.SINGLES
    J, R, E, off = c["J"], c["R"], c["E"], c["env_offset"]
    scs, batch = cases.batch(J, R, E, c["seed"], off, L=c["L"])
    env = _pe_env(batch, seed=c["env_seed"], env_offset=off)
    assert env._scan_pe_pattern_io is not None and env._scan_pe_pattern_io.n_levels == c["L"]
    singles = [BatchedElectromagneticEnvironment(scenario=scs[e], batch_envs=1, device=DEV, seed=c["env_seed"], env_offset=off + e)
               for e in range(E)]
    assert env.observation_is_static is False
    env.reset()
    for s in singles:
        s.reset()
    cols = scs[0].theta_a_columns
    other = [k for k in range(scs[0].state_dim) if k not in cols]
    static = torch.from_numpy(np.stack([sc.state_vector() for sc in scs])).to(DEV)
    az0 = torch.from_numpy(np.stack([sc.scan_tables["az0"] for sc in scs])).to(DEV)
    assert torch.equal(env.beam_azimuth, az0) and torch.equal(env.get_state()[:, cols], az0.to(torch.float32))
    mask = np.zeros(E, dtype=np.uint8)
    mask[::3] = 1
    exact = ("r_d", "r_p", "r_j", "radar_pds", "snr_with_jamming", "snr_no_jamming")
    distinct = 0
    for t, (T, P) in enumerate(cases.singles_actions()):
        if t == c["reset_at"]:
            env.reset(torch.from_numpy(mask).to(DEV))
            for e in range(0, E, 3):
                singles[e].reset()
        T_d, P_d = _cuda(T, P)
        rew, term, info = env.step(T_d, P_d)
        outs = [s.step(T_d[e:e + 1], P_d[e:e + 1]) for e, s in enumerate(singles)]
        cat = lambda f: torch.cat([f(o, s) for o, s in zip(outs, singles)])
        assert torch.equal(info["radar_tracking"], cat(lambda o, s: o[2]["radar_tracking"])), t
        assert torch.equal(term, cat(lambda o, s: o[1])), t
        assert torch.equal(info["step_count"], cat(lambda o, s: o[2]["step_count"])), t
        assert torch.equal(env.beam_azimuth, cat(lambda o, s: s.beam_azimuth)), t
        state = env.get_state()
        assert torch.equal(state[:, cols], cat(lambda o, s: s.get_state()[:, cols])), t
        assert torch.equal(state[:, cols], env.beam_azimuth.to(torch.float32)), t
        assert torch.equal(state[:, other], static[:, other]), t
        assert _bits_equal(info["snr_no_jamming"], cat(lambda o, s: o[2]["snr_no_jamming"])), t   # the level each radar saw
        r1 = cat(lambda o, s: o[0])
        if pd32 == "0":
            assert _bits_equal(rew, r1), t
            for k in exact:
                assert _bits_equal(info[k], cat(lambda o, s: o[2][k])), (k, t)
        else:
            assert torch.equal(rew.isnan(), r1.isnan()), t
            ok = ~rew.isnan()
            err = (rew[ok].double() - r1[ok].double()).abs().max().item()
            print(f"step {t}: max |reward - single| = {err:.3e}")
            assert err <= (R + J) * 6e-7, (t, err)
        distinct = max(distinct, torch.unique(rew[~rew.isnan()]).numel())
    assert distinct > E // 2          # the envs really run different scenarios


# ---------------------------------------------------------------------------------------------------------------
# 2. against the restatement, per env
@functools.lru_cache(maxsize=None)
def _model_run(J, R, L):
    """The restatement's outputs on the model inputs of (J, R, L), one ScanPatternModel per env, stacked over the envs;
    computed once per case and shared by the two table layouts."""
    from macjd_amd.scenario import ScenarioBatch
    scs = cases.model_scenarios(J, R, L)
    models = [spm.ScanPatternModel(sc, 1) for sc in scs]
    steps = []
    for T, P, u in cases.model_actions(J, R, L):
        outs = [m.step(T[e:e + 1], P[e:e + 1], u[e:e + 1]) for e, m in enumerate(models)]
        steps.append((T, P, u, {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in outs[0]}))
    return ScenarioBatch(scs, scan=True, pattern=True), steps


@pytest.mark.parametrize("layout", ["tiled8", "plain"])
@pytest.mark.parametrize("J,R,L", cases.MODEL_CASES)
def test_kernel_vs_restatement_per_env(J, R, L, layout, monkeypatch):
    """Supplied uniforms, float64 actions, float64 diagnostics: the general variants ((3,4), (2,2), (6,8)) and the
    generic-size kernel ((12,16), (5,7)) at L = 4, (3,4) also at L = 1 and 6; 33 envs = four full tiles of 8 and a padded
    one, or the plain SoA.  Tolerances of tests/test_scan_gpu.py::_run_vs_model."""
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    monkeypatch.setattr(Env, "PE_TILE", 8)
    monkeypatch.setattr(Env, "pe_tiled", layout == "tiled8")
    batch, steps = _model_run(J, R, L)
    E = cases.MODEL["E"]
    env = _pe_env(batch)
    rows = R + 4 * (L + 2) * R
    assert env._pe_tile == (8 if layout == "tiled8" else 0)
    assert tuple(env._scan_pe_pattern_tables.shape) == ((5, rows, 8) if layout == "tiled8" else (rows, E))
    env.reset()
    dg = _diag(E, R, J)
    for T, P, u, o in steps:
        _, term, info = env.step(*_cuda(T, P, u), diag=dg)
        np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
        np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
        assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes()
        np.testing.assert_array_equal(info["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
        np.testing.assert_allclose(dg["pd64"].cpu().numpy(), o["pd"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["snr64"].cpu().numpy(), o["snr"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["prj64"].cpu().numpy(), o["prj"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["out64"].cpu().numpy(), o["out"], rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------
# 3. production variant == general variant
@pytest.mark.parametrize("J,R", [(3, 4), (6, 8), (12, 16), (2, 2)])
def test_production_variant_equals_general_variant(J, R, monkeypatch):
    """The production (FAST) per-env pattern variant == the general one (selected by asking for the diagnostics), bitwise.
    (12j/16r has no compiled per-env scanning variant: both calls run the generic-size kernel.)"""
    from macjd_amd import _native
    from macjd_amd.scenario import ScenarioBatch
    monkeypatch.setenv("MACJD_ENV_PD32", "0")
    _native.reload_options()
    E = 300
    batch = ScenarioBatch.randomized(cases.pattern_base(J, R), 25, seed=9, azimuth_jitter=cases.AZIMUTH_JITTER).tile(E)
    assert batch.scan_pattern_levels == 4
    fast, general = _pe_env(batch, seed=5, env_offset=64), _pe_env(batch, seed=5, env_offset=64)
    fast.reset(); general.reset()
    rng = np.random.default_rng(R)
    diag = _diag(E, R, J)
    L, lv = 4, 6 * R
    # snr_no per (level, radar, env) as the kernel reports it; `middle` counts reports that are a level 1..L value and neither
    # the main nor the side-lobe one
    snr_lv = torch.from_numpy(batch.pattern_tables[R + lv:R + 2 * lv].reshape(L + 2, R, E)).to(DEV).to(torch.float32)
    middle = 0
    for t in range(5):
        T, P = random_actions(rng, E, J, R)
        Td, Pd = _cuda(T, P)
        r1, t1, i1 = fast.step(Td, Pd)
        r2, t2, i2 = general.step(Td, Pd, diag=diag)
        assert torch.equal(r1, r2) and torch.equal(t1, t2)
        for k in INFO_KEYS:
            assert torch.equal(i1[k], i2[k]), k
        assert torch.equal(fast.beam_azimuth, general.beam_azimuth) and torch.equal(fast.get_state(), general.get_state())
        rep = i1["snr_no_jamming"].t()                                            # [R, E]
        mid = torch.stack([rep == snr_lv[k] for k in range(1, L + 1)]).any(dim=0)
        middle += int((mid & (rep != snr_lv[0]) & (rep != snr_lv[L + 1])).sum())
    assert torch.unique(fast.beam_azimuth[:25, 0]).numel() > 20
    assert middle > 0                 # the pattern's own levels occurred


# ---------------------------------------------------------------------------------------------------------------
# 4. a pattern whose every level has the side lobe's gain is the pattern-free per-env kernel
@pytest.mark.parametrize("J,R", [(3, 4), (5, 7)])
@pytest.mark.parametrize("general", [False, True])
def test_degenerate_pattern_equals_plain_scanning_batch(J, R, general):
    """Every gain_db == sidelobe_db: levels 1..L + 1 hold the side-lobe values bit for bit, so the outputs equal those of the
    plain scanning batch of the same scenarios through macjd_env_step_scan_pe, bitwise (production variant, and the general
    / generic-size one selected by the diagnostics)."""
    from macjd_amd.scenario import ScenarioBatch
    E, seed = 40, 6
    _, pat = cases.batch(J, R, E, seed, gain_db=[-30.0] * 3, sidelobe_db=-30.0)
    plain = ScenarioBatch(cases.scenarios(J, R, E, seed, pattern=False), scan=True)
    assert pat.scan_tables.tobytes() == plain.scan_tables.tobytes() and pat.tables.tobytes() == plain.tables.tobytes()
    a, b = _pe_env(pat, seed=3), _pe_env(plain, seed=3)
    assert a._scan_pe_pattern_io is not None and b._scan_pe_pattern_io is None
    a.reset(); b.reset()
    rng = np.random.default_rng(J)
    da, db = (_diag(E, R, J), _diag(E, R, J)) if general else (None, None)
    sides = 0
    for t in range(8):
        T, P = random_actions(rng, E, J, R)
        Td, Pd = _cuda(T, P)
        r1, t1, i1 = a.step(Td, Pd, diag=da)
        r2, t2, i2 = b.step(Td, Pd, diag=db)
        assert torch.equal(r1, r2) and torch.equal(t1, t2), t
        for k in INFO_KEYS:
            assert torch.equal(i1[k], i2[k]), (k, t)
        assert torch.equal(a.beam_azimuth, b.beam_azimuth) and torch.equal(a.get_state(), b.get_state()), t
        if general:
            for k in da:
                assert torch.equal(da[k], db[k]), (k, t)
        sides += int((i1["snr_no_jamming"] != a._snr_no.to(torch.float32)).sum())
    assert sides > 0                  # side-lobe values were really taken


# ---------------------------------------------------------------------------------------------------------------
# 5. guard rails
def test_entry_point_argument_errors_and_refusals(monkeypatch):
    from macjd_amd import _native
    from macjd_amd.scenario import Scenario
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    monkeypatch.setattr(Env, "pe_tiled", False)      # plain layout: the strides are checked
    J, R, E = 3, 4, 8
    scs, batch = cases.batch(J, R, E, seed=3)
    env = _pe_env(batch)
    env.reset()
    rng = np.random.default_rng(0)
    T, P = random_actions(rng, E, J, R)
    env.step(*_cuda(T, P))                           # fills env._io with a valid call's arguments
    lib, stream = _native.load(), torch.cuda.current_stream().cuda_stream
    io_, si, sp, pp, h = env._io, env._scan_io, env._scan_pe_io, env._scan_pe_pattern_io, env._handle.ptr
    ref = lambda x: ctypes.byref(x) if x is not None else None
    step = lambda io=io_, si=si, sp=sp, pp=pp, h=h: lib.macjd_env_step_scan_pe_pattern(h, ctypes.byref(io), ref(si), ref(sp),
                                                                                      ref(pp), stream)
    err = lambda: lib.macjd_last_error().decode()
    assert step() == 0
    # the handle of such an environment carries no pattern: the per-env reset takes it
    assert lib.macjd_env_reset_scan_pe(h, E, ctypes.byref(si), ctypes.byref(sp), 0, None, stream) == 0

    def pattern_io(tables=pp.tables, stride=E, n_levels=4):
        x = _native.ScanPePatternIO()
        x.tables, x.stride, x.n_levels = tables, stride, n_levels
        return x
    assert step(pp=None) == -1 and "NULL per-env pattern tables" in err()
    assert step(pp=pattern_io(tables=None)) == -1 and "NULL per-env pattern tables" in err()
    assert step(pp=pattern_io(stride=E - 1)) == -1 and "stride >= n_envs" in err()
    for bad in (0, -1, 7):
        assert step(pp=pattern_io(n_levels=bad)) == -1 and "n_levels outside 1..MACJD_MAX_PATTERN_LEVELS" in err(), bad
    no_pe = _native.StepIO.from_buffer_copy(io_)
    no_pe.pe_tables = None
    assert step(io=no_pe) == -1 and "pe_tables" in err()
    null = _native.ScanPeIO()
    null.tables, null.stride = None, E
    assert step(sp=null) == -1 and "NULL per-env scan tables" in err()
    assert step(sp=None) == -1 and "NULL per-env scan tables" in err()
    short = _native.ScanPeIO()
    short.tables, short.stride = sp.tables, E - 1
    assert step(sp=short) == -1 and "stride >= n_envs" in err()
    assert step(si=None) == -1 and "NULL scan io" in err()
    slot = _native.StepIO.from_buffer_copy(io_)
    slot.flags = _native.STEP_SLOT_KERNEL
    assert step(io=slot) == -4 and "slot" in err()

    with torch.cuda.device(DEV):
        pat4 = _native.ScenarioHandle(scs[0])                              # L = 4 on the handle: accepted, never read
        pat2_d = cases.scenario_dicts(J, R, 1, seed=3, gain_db=[-3, -12])[0]
        pat2 = _native.ScenarioHandle(Scenario.from_dict(pat2_d))
        static = _native.ScenarioHandle(Scenario.from_dict(cases.ring_scenario_dict(J, R)))
    assert step(h=pat4.ptr) == 0
    assert step(h=pat2.ptr) == -1 and "n_levels differs" in err()
    assert step(h=static.ptr) == -1 and "no scanning tables" in err()
    # the pattern-free per-env calls still refuse a pattern handle
    assert lib.macjd_env_step_scan_pe(pat4.ptr, ctypes.byref(io_), ctypes.byref(si), ctypes.byref(sp), stream) == -4 and "pattern" in err()
    assert lib.macjd_env_reset_scan_pe(pat4.ptr, E, ctypes.byref(si), ctypes.byref(sp), 0, None, stream) == -4 and "pattern" in err()
    # ... and the shared-table entry point per-env tables
    assert lib.macjd_env_step_scan(h, ctypes.byref(io_), ctypes.byref(si), stream) == -4 and "macjd_env_step_scan_pe" in err()
    torch.cuda.synchronize()

    # the launches that stay out of scope keep refusing, and say why
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="per-env scenario tables"):
        env.episode_scan_args()
    with pytest.raises(RuntimeError, match="scanning"):
        env.step_many(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3))
    with pytest.raises(RuntimeError, match="scanning"):
        env.time_step_kernel(z(E, J, dt=torch.int32), z(E, J), 2)
    env.kernel_flags = _native.STEP_SLOT_KERNEL
    with pytest.raises(_native.NativeLibraryError, match="slot"):
        env.step(*_cuda(T, P))
    env.kernel_flags = 0
    runner, _, _ = _runner(batch)
    assert not runner.closed_loop_available() and not runner.fused_rollout_available()
    with pytest.raises(RuntimeError, match="closed_loop_available"):
        runner.rollout_closed_loop()


# ---------------------------------------------------------------------------------------------------------------
# 6. runner and driver
def _runner(batch, seed=5):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    env = _pe_env(batch, seed=seed)
    E = batch.n_envs
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


def _shipped_base():
    with open(os.path.join(PKG, "config", "scenario_3j4r_scan_pattern.yaml")) as f:
        return yaml.safe_load(f)


def test_runner_on_a_randomized_pattern_batch():
    """One episode batch of the runner on ``ScenarioBatch.randomized`` of the shipped pattern scenario: the stored theta_a
    columns follow a replay of the stored actions through the pattern kernel, rewards differ across envs and are finite."""
    from macjd_amd.scenario import ScenarioBatch
    E, J = 64, 3
    batch = ScenarioBatch.randomized(_shipped_base(), E, seed=2, azimuth_jitter=cases.AZIMUTH_JITTER)
    assert batch.scan_pattern_levels == 4
    runner, buf, _ = _runner(batch)
    assert runner.env._scan_pe_pattern_io is not None
    assert not runner.hoist_static_obs and not runner.fused_rollout_available() and not runner.closed_loop_available()
    runner.run(sync_stats=True)
    sc = batch.base
    T, cols = sc.episode_limit, sc.theta_a_columns
    state = buf.buffers["state"][:E]                              # [E, T + 1, S]
    reward = buf.buffers["reward"][:E].reshape(E, -1)[:, :T]
    assert torch.isfinite(reward).all() and torch.unique(reward.sum(dim=1)).numel() > E // 2
    replay = _pe_env(batch, seed=5)
    replay.reset()
    Td = buf.buffers["actions_discrete"][:E].to(DEV).reshape(E, -1, J).to(torch.int32)
    Pd = buf.buffers["actions_continuous"][:E].to(DEV).reshape(E, -1, J).to(torch.float32)
    for t in range(T):
        assert torch.equal(state[:, t, cols].to(DEV), replay.beam_azimuth.to(torch.float32)), t
        rew, _, _ = replay.step(Td[:, t].contiguous(), Pd[:, t].contiguous())
        assert torch.equal(rew, reward[:, t].to(DEV)), t
    assert torch.unique(state[:, :T, cols[0]]).numel() > E


def test_driver_trains_on_randomized_pattern_scenarios(tmp_path):
    """``main --env-config scenario_3j4r_scan_pattern --randomize-scenarios`` in short: two episode batches, updates, no
    further flag."""
    from macjd_amd.main import load_config, run
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
    assert res["total_steps"] == 2 * E * 100 and res["episodes"] == 2 * E and res["train_steps"] > 0
    text = out.getvalue()
    assert "Training finished." in text and not re.search(r"\b(nan|inf)\b", text.lower())   # finite logged statistics
