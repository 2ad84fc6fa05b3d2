"""Moving scenarios with scanning radars on the GPU (include/macjd.h, macjd_env_step_moving_scan): bitwise equality with the
per-env scanning step (macjd_env_step_scan_pe / _pattern) on the gathered frames, the float64 model (tests/
moving_scan_model.py), the production variant against the general one, the entry point's argument errors, the zero-velocity
reduction to the static scanning step, the runner (eager, graph-replayed, both rollout switches on), the learner, the driver
and the single-env facade.  Inputs: tests/moving_scan_cases.py (the CPU file checks the model run's coverage)."""
import contextlib
import ctypes
import io
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import moving_scan_cases as cases
from _harness import REPO, random_actions
from moving_scan_model import MovingScanModel
from test_nets_cpu import make_args, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
F = cases.F
INFO_KEYS = ("r_d", "r_p", "r_j", "radar_tracking", "radar_pds", "snr_with_jamming", "snr_no_jamming")


def _env(sc, E, seed=11, **kw):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=seed, **kw)


def _diag(E, R, J):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    return {"out64": z(E, 4), "pd64": z(E, R), "snr64": z(E, R), "prj64": z(E, J)}


def _cuda(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _third(E):
    return torch.from_numpy(cases.third(E).astype(np.uint8)).to(DEV)


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


def _state_checker(sc, env):
    """check(): the state rows carry (float)theta_a in the theta_a columns, frame min(counter, F)'s positions in the position
    columns, and the scenario's state vector everywhere else."""
    S, E = sc.state_dim, env.batch_envs
    tcols, pcols = sc.theta_a_columns, sc.position_columns
    other = [c for c in range(S) if c not in tcols and c not in pcols]
    static = torch.from_numpy(sc.state_vector()).to(DEV)
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(DEV)

    def check():
        st = env.get_state()
        k = torch.clamp(env.step_count.to(torch.int64), max=F)
        assert torch.equal(st[:, tcols], env.beam_azimuth.to(torch.float32))
        assert torch.equal(st[:, pcols], pos[k]) and torch.equal(env.positions, pos[k])
        assert torch.equal(st[:, other], static[other].expand(E, -1))
    return check


# ---------------------------------------------------------------------------------------------------------------
# 1. bitwise against the per-env scanning step on the gathered frames
def _gathered_reference(sc, frames, E, pattern, **kw):
    """A per-env scanning env of E copies of the static frame-0 scenario (same R, J, episode limit, r_p bounds and Pd constants
    in the handle) that steps through macjd_env_step_scan_pe(_pattern); ``load(mv)`` makes env e's columns the frame env e of
    ``mv`` is in (tile width 1: [E, rows]) and copies ``mv``'s beams, FSM bits, step counters and episode indices."""
    from macjd_amd.scenario import ScenarioBatch
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    batch = ScenarioBatch([frames[0]] * E, scan=True, pattern=pattern)
    ref = BatchedElectromagneticEnvironment(scenario_batch=batch, device=DEV, **kw)
    mt = sc.motion_tables
    fr, fl, sf = _cuda(mt["frames"], mt["flags"], mt["scan_frames"])
    pf = _cuda(mt["pattern_frames"])[0] if pattern else None

    def load(mv):
        f_e = torch.clamp(mv._step.to(torch.int64), max=fr.shape[0] - 1)
        ref._pe_tables, ref._pe_flags, ref._pe_tile = fr[f_e].contiguous(), fl[f_e].contiguous(), 1
        ref._scan_pe_tables = sf[f_e].contiguous()
        ref._scan_pe_io.tables = ref._scan_pe_tables.data_ptr()
        if pattern:
            ref._scan_pe_pattern_tables = pf[f_e].contiguous()
            ref._scan_pe_pattern_io.tables = ref._scan_pe_pattern_tables.data_ptr()
        ref._track.copy_(mv._track); ref._step.copy_(mv._step); ref._episode.copy_(mv._episode)
        ref._theta_a.copy_(mv._theta_a)
        return f_e
    return ref, load


@pytest.mark.parametrize("mode", ["philox", "philox_diag", "uniforms_diag"])
@pytest.mark.parametrize("E", [1, 65, 257])
@pytest.mark.parametrize("J,R,pattern", cases.CASES)
def test_bitwise_equal_to_the_per_env_scanning_step_on_gathered_frames(J, R, pattern, E, mode):
    sc, frames = cases.case(J, R, pattern)
    mv = _env(sc, E, seed=77, env_offset=1000)
    assert mv._motion_scan_io is not None and mv._motion_scan_io.n_levels == (4 if pattern else 0)
    assert mv.observation_is_static is False
    ref, load = _gathered_reference(sc, frames, E, pattern, seed=77, env_offset=1000)
    assert (ref._scan_pe_pattern_io is not None) == pattern
    mv.reset()
    check = _state_checker(sc, mv)
    check()
    tcols = sc.theta_a_columns
    rng = np.random.default_rng(E * 31 + R)
    d_mv, d_ref = (_diag(E, R, J), _diag(E, R, J)) if mode != "philox" else (None, None)
    rsum_mv, rsum_ref = (torch.zeros((E, 3), device=DEV) for _ in range(2))
    seen_frames = set()
    for t in range(F + 6):   # the envs that are never reset pass F: the clamp
        if t == 5:           # masked reset: one wave then holds two frames
            before = mv.get_state().clone()
            mv.reset(_third(E))
            keep = ~_third(E).bool()
            assert torch.equal(mv.get_state()[keep], before[keep])
            check()
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
        assert torch.equal(mv._theta_a, ref._theta_a), t
        for k in INFO_KEYS:
            assert torch.equal(info[k], info_r[k]), (t, k)
        assert torch.equal(mv.get_state()[:, tcols], ref.get_state()[:, tcols]), t
        check()
        if d_mv is not None:
            for k in d_mv:
                assert torch.equal(d_mv[k], d_ref[k]), (t, k)
    want = np.where(cases.third(E), F + 1, F + 6)
    np.testing.assert_array_equal(mv.step_count.cpu().numpy(), want)
    assert seen_frames == set(range(F))


# ---------------------------------------------------------------------------------------------------------------
# 2. against the model
@pytest.mark.parametrize("J,R,pattern", cases.CASES)
def test_kernel_vs_model(J, R, pattern):
    """Supplied uniforms, float64 actions, float64 diagnostics (the general variants, (3,3): the generic-size kernel) on the
    model run of tests/moving_scan_cases.py.  Tolerances of tests/test_scan_pe_gpu.py."""
    sc, frames = cases.case(J, R, pattern)
    steps, _ = cases.model_run(J, R, pattern)
    E = cases.MODEL["E"]
    env = _env(sc, E)
    env.reset()
    dg = _diag(E, R, J)
    pos = sc.motion_tables["positions"]
    counter = np.zeros(E, dtype=np.int64)
    for t, (T, P, u, frame, o) in enumerate(steps):
        if t == cases.MODEL["reset_at"]:
            env.reset(_third(E))
            counter[cases.third(E)] = 0
        np.testing.assert_array_equal(np.minimum(counter, F - 1), frame)
        _, term, info = env.step(*_cuda(T, P, u), diag=dg)
        counter += 1
        np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
        np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
        assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes(), t
        np.testing.assert_array_equal(info["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
        np.testing.assert_allclose(dg["pd64"].cpu().numpy(), o["pd"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["snr64"].cpu().numpy(), o["snr"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["prj64"].cpu().numpy(), o["prj"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["out64"].cpu().numpy(), o["out"], rtol=0, atol=1e-9)
        assert env.positions.cpu().numpy().tobytes() == pos[np.minimum(counter, F)].tobytes(), t
        assert env.get_state()[:, sc.theta_a_columns].cpu().numpy().tobytes() == o["theta_a"].astype(np.float32).tobytes(), t


# ---------------------------------------------------------------------------------------------------------------
# 3. production variant == general variant
@pytest.mark.parametrize("J,R,pattern", cases.CASES)
def test_production_variant_equals_general_variant(J, R, pattern):
    """The production (FAST) variant == the general one (selected by asking for the diagnostics), bitwise.  ((3,3) has no
    compiled variant: both calls run the generic-size kernel.)"""
    sc, _ = cases.case(J, R, pattern)
    E = 300
    fast, general = _env(sc, E, seed=5, env_offset=64), _env(sc, E, seed=5, env_offset=64)
    fast.reset(); general.reset()
    rng = np.random.default_rng(R)
    diag = _diag(E, R, J)
    for t in range(F + 2):
        if t == 5:
            fast.reset(_third(E)); general.reset(_third(E))
        Td, Pd = _cuda(*random_actions(rng, E, J, R))
        r1, t1, i1 = fast.step(Td, Pd)
        r2, t2, i2 = general.step(Td, Pd, diag=diag)
        assert torch.equal(r1, r2) and torch.equal(t1, t2), t
        for k in INFO_KEYS:
            assert torch.equal(i1[k], i2[k]), (t, k)
        assert torch.equal(fast.beam_azimuth, general.beam_azimuth) and torch.equal(fast.get_state(), general.get_state()), t
    assert torch.unique(fast.beam_azimuth[:, 1]).numel() > 4


# ---------------------------------------------------------------------------------------------------------------
# 4. argument errors
def test_entry_point_argument_errors_and_refusals():
    from macjd_amd import _native
    from macjd_amd.scenario import Scenario, ring_scenario_dict
    import motion_cases
    J, R, E = 3, 4, 8
    sc, frames = cases.case(J, R, True)
    env = _env(sc, E)
    env.reset()
    T, P = random_actions(np.random.default_rng(0), E, J, R)
    env.step(*_cuda(T, P))                           # fills env._io with a valid call's arguments
    lib, stream = _native.load(), torch.cuda.current_stream().cuda_stream
    io_, mo, si, ms, h = env._io, env._motion_io, env._scan_io, env._motion_scan_io, env._handle.ptr
    ref = lambda x: ctypes.byref(x) if x is not None else None
    step = lambda io=io_, mo=mo, si=si, ms=ms, h=h: lib.macjd_env_step_moving_scan(h, ctypes.byref(io), ref(mo), ref(si), ref(ms),
                                                                                 stream)
    err = lambda: lib.macjd_last_error().decode()
    copy_of = lambda x: type(x).from_buffer_copy(x)
    assert step() == 0

    with torch.cuda.device(DEV):
        static = _native.ScenarioHandle(Scenario.from_dict(motion_cases.moving_ring_dict(J, R), config=motion_cases.config()))
        pat2_d = cases.moving_scan_dict(J, R, True)
        pat2_d["environment_params"]["radar_scan"]["pattern"]["gain_db"] = [-3, -12]
        pat2 = _native.ScenarioHandle(Scenario.from_dict(pat2_d, config=motion_cases.config()))
        plain = _native.ScenarioHandle(cases.case(J, R, False)[0])
    assert step(h=static.ptr) == -1 and "no scanning tables" in err()                 # not a scanning handle
    with_pe = copy_of(io_)
    with_pe.pe_tables, with_pe.pe_flags, with_pe.pe_stride = mo.frames, mo.frame_flags, E
    assert step(io=with_pe) == -1 and "pe_tables must be NULL" in err()
    with_snr = copy_of(mo)
    with_snr.snr_no, with_snr.sn_se, with_snr.sn_sx = env._snr_no_step.data_ptr(), 1, E
    assert step(mo=with_snr) == -1 and "motion->snr_no must be NULL" in err()

    def scan_io(frames_=ms.scan_frames, pattern=ms.pattern_frames, n_levels=4):
        x = _native.MotionScanIO()
        x.scan_frames, x.pattern_frames, x.n_levels = frames_, pattern, n_levels
        return x
    for bad in (-1, 7):
        assert step(ms=scan_io(n_levels=bad)) == -1 and "n_levels outside 0..MACJD_MAX_PATTERN_LEVELS" in err(), bad
    assert step(h=pat2.ptr) == -1 and "n_levels differs" in err()                     # the handle's L = 2, the call's 4
    assert step(h=plain.ptr) == 0                                                     # a pattern-free handle: levels from the call
    assert step(ms=scan_io(n_levels=0)) == -1 and "n_levels differs" in err()          # (the env's handle has L = 4)
    assert step(h=plain.ptr, ms=scan_io(n_levels=0)) == -1 and "go together" in err()  # pattern_frames with n_levels == 0
    assert step(h=plain.ptr, ms=scan_io(pattern=None)) == -1 and "go together" in err()   # ... and the reverse
    assert step(h=plain.ptr, ms=scan_io(pattern=None, n_levels=0)) == 0               # the pattern-free step on the same frames
    other = torch.zeros_like(env._state_dyn)
    two_states = copy_of(si)
    two_states.state = other.data_ptr()
    assert step(si=two_states) == -1 and "scan->state and motion->state" in err()
    no_state = copy_of(si)
    no_state.state = None
    assert step(si=no_state) == 0                                                     # the theta_a columns are optional
    assert step(ms=None) == -1 and "scan_frames" in err()
    assert step(ms=scan_io(frames_=None)) == -1 and "scan_frames" in err()
    assert step(si=None) == -1 and "NULL scan io" in err()
    assert step(mo=None) == -1 and "NULL scenario / motion io" in err()
    slot = copy_of(io_)
    slot.flags = _native.STEP_SLOT_KERNEL
    assert step(io=slot) == -4 and "slot" in err()
    torch.cuda.synchronize()

    # the launches that rest on the step counter alone refuse, and say why
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="scanning"):
        env.step_many(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3))
    with pytest.raises(RuntimeError, match="frame_states: not available with scanning radars"):
        env.frame_states()
    with pytest.raises(RuntimeError, match="scanning"):
        env.time_step_kernel(z(E, J, dt=torch.int32), z(E, J), 2)
    with pytest.raises(RuntimeError, match="scanning"):
        env.time_step_many_kernel(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3), 2)
    with pytest.raises(RuntimeError, match="moving scenario"):
        env.episode_scan_args()
    assert tuple(env.positions.shape) == (E, 2 * R + 2 * J)


# ---------------------------------------------------------------------------------------------------------------
# 5. zero velocities: the static scanning scenario
@pytest.mark.parametrize("J,R,pattern", [(3, 4, False), (3, 4, True), (3, 3, True)])
def test_zero_velocity_scenario_equals_the_static_scanning_one(J, R, pattern, monkeypatch):
    import copy
    import motion_cases
    from macjd_amd.scenario import Scenario
    cfg = cases.zero_velocity(cases.moving_scan_dict(J, R, pattern))
    base = copy.deepcopy(cfg)
    del base["environment_params"]["motion"]
    static = Scenario.from_dict(base, config=motion_cases.config())
    moving = Scenario.from_dict(cfg, config=motion_cases.config())
    E = 257
    with _options(monkeypatch, MACJD_ENV_PD32="0"):
        a, b = _env(static, E, seed=3), _env(moving, E, seed=3)
        assert a._motion_io is None and b._motion_scan_io is not None
        a.reset(); b.reset()
        rng = np.random.default_rng(4)
        for t in range(10):
            if t == 4:
                a.reset(_third(E)); b.reset(_third(E))
            Td, Pd = _cuda(*random_actions(rng, E, J, R))
            ra, ta, ia = a.step(Td, Pd)
            rb, tb, ib = b.step(Td, Pd)
            assert torch.equal(ta, tb) and torch.equal(a.step_count, b.step_count), t
            assert torch.equal(ra, rb) and torch.equal(a._r_dpj, b._r_dpj), t
            for k in INFO_KEYS:
                assert torch.equal(ia[k], ib[k]), (t, k)
            assert torch.equal(a.beam_azimuth, b.beam_azimuth) and torch.equal(b.get_state(), a.get_state()), t
        assert a.track.any() and torch.unique(a.beam_azimuth[:, 1]).numel() > 2


# ---------------------------------------------------------------------------------------------------------------
# 6. runner, learner, driver
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


def test_graph_replayed_rollout_equals_eager_with_both_switches_on_and_the_learner_trains():
    from macjd_amd.core.qmix import QMixLearner
    sc, _ = cases.case(3, 4, True)
    E, J = 16, 3
    r_e, b_e, args = _runner(sc, E)
    r_g, b_g, _ = _runner(sc, E)
    r_s, b_s, _ = _runner(sc, E)
    r_s.closed_loop_rollout = r_s.moving_episode_rollout = True      # both switches on: still the step loop
    for r in (r_e, r_s):
        assert not r._static and not r.hoist_static_obs and not r.fused_rollout_available()
        assert not r.closed_loop_available() and not r.closed_loop_pe_available() and not r.moving_rollout_available()
    for name in ("rollout_closed_loop", "rollout_moving"):
        with pytest.raises(RuntimeError, match="not available"):
            getattr(r_s, name)()
    r_g.enable_graph()
    for _ in range(2):
        r_e.run(sync_stats=True)
        r_g.run(sync_stats=True)
        r_s.run(sync_stats=True)
    assert b_e.obs_static is False and b_g.obs_static is False
    for k in b_e.buffers:
        assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(b_e.buffers[k], b_s.buffers[k]), k
    # the stored observations carry the moved positions and the moved beams
    pcols, tcols = sc.position_columns, sc.theta_a_columns
    dev = b_e.buffers["state"].device
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(dev)
    for name in ("state", "obs"):
        st = b_e.buffers[name][:2 * E]                       # [2E, T + 1, (J,) S]
        st = st if name == "state" else st[:, :, 0]
        assert torch.equal(st[:, :F][:, :, pcols], pos[:F].expand(2 * E, -1, -1)), name
    assert b_e.buffers["terminated"][:2 * E, F - 1].all()
    state = b_e.buffers["state"][E:2 * E]                    # the second episode batch: replayed through a fresh env
    replay = _env(sc, E, seed=5)
    replay.reset(); replay.reset()                           # its episode index
    Td = b_e.buffers["actions_discrete"][E:2 * E].to(DEV).reshape(E, -1, J).to(torch.int32)
    Pd = b_e.buffers["actions_continuous"][E:2 * E].to(DEV).reshape(E, -1, J).to(torch.float32)
    reward = b_e.buffers["reward"][E:2 * E].reshape(E, -1)
    for t in range(F):
        assert torch.equal(state[:, t, tcols].to(DEV), replay.beam_azimuth.to(torch.float32)), t
        rew, _, _ = replay.step(Td[:, t].contiguous(), Pd[:, t].contiguous())
        assert torch.equal(rew, reward[:, t].to(DEV)), t
    assert torch.unique(state[:, :F, tcols[1]]).numel() > F // 2
    with quiet():
        learner = QMixLearner(r_e.mac, args)
    for _ in range(3):
        stats = learner.train(b_e.sample(8), {})
        assert np.isfinite(float(stats["loss"])) and np.isfinite(float(stats["grad_norm"]))


_DRIVER = r'''
import contextlib, io, os, sys
sys.path.insert(0, %(repo)r)
from macjd_amd.main import load_config, run
pkg = %(pkg)r
with contextlib.redirect_stdout(io.StringIO()):
    cfg = load_config("default", os.path.join(pkg, "config"))
E, F = 32, 24
cfg.device_request = "cuda"
cfg.env_config = "scenario_3j4r_moving_scan"
cfg.sim_config_path = os.path.join(pkg, "config", "scenario_3j4r_moving_scan.yaml")
cfg.save_model_dir, cfg.results_path = os.path.join(%(tmp)r, "models"), os.path.join(%(tmp)r, "logs")
cfg.log_interval_seconds = 0
cfg.gemm_tuning = False
cfg.resume = None
for k, v in dict(batch_envs=E, buffer_size=2 * E, total_env_steps=2 * E * F, episode_limit=F, start_training_steps=0,
                 save_interval=10 ** 9, test_interval=10 ** 9, test_nepisodes=E, batch_size=8, lr=1e-4,
                 updates_per_rollout=4).items():
    setattr(cfg, k, v)
with contextlib.redirect_stdout(io.StringIO()) as out:
    res = run(cfg)
print("RESULT", res["total_steps"], res["episodes"], res["train_steps"], int("Training finished." in out.getvalue()))
cfg.randomize_scenarios = True
try:
    with contextlib.redirect_stdout(io.StringIO()):
        run(cfg)
    print("RANDOMIZE accepted")
except ValueError as e:
    print("RANDOMIZE", e)
'''


def test_driver_trains_on_the_moving_scanning_scenario_in_a_fresh_process(tmp_path):
    out = subprocess.run([sys.executable, "-c", _DRIVER % {"repo": REPO, "pkg": PKG, "tmp": str(tmp_path)}],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    E = 32
    assert [int(x) for x in line[1:3]] == [2 * E * F, 2 * E] and int(line[3]) > 0 and line[4] == "1"
    assert "RANDOMIZE --randomize-scenarios is not supported with a moving scenario" in out.stdout


# ---------------------------------------------------------------------------------------------------------------
# 7. the single-env facade
@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_facade_returns_the_moving_scanning_state_step_by_step(mode):
    import yaml
    import motion_cases
    from macjd_amd.scenario import Scenario, motion_frame_dict
    from macjd_amd.simulation.environment import ElectromagneticEnvironment
    path = os.path.join(PKG, "config", "scenario_3j4r_moving_scan.yaml")
    n = 30
    with contextlib.redirect_stdout(io.StringIO()):
        env = ElectromagneticEnvironment(SimpleNamespace(), path)
    sc = env.scenario
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    frames = [Scenario.from_dict(motion_frame_dict(cfg, f)) for f in range(n + 2)]
    model = MovingScanModel(frames + [frames[-1]], 1)        # the first n + 2 frames: enough for n steps
    R, J = sc.num_radars, sc.num_jammers
    tcols, pcols = sc.theta_a_columns, sc.position_columns
    rng = np.random.default_rng(8)
    np.random.seed(42)
    s0 = env.reset()
    assert s0[tcols].tobytes() == model.theta_a[0].astype(np.float32).tobytes()
    assert s0[pcols].tobytes() == sc.motion_tables["positions"][0].tobytes()
    levels = set()
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n):
            T, P = random_actions(rng, 1, J, R)
            T = np.clip(T, 0, 2 * R)                         # (no invalid-action warnings: not what this test is about)
            if mode == "f32":
                acts = [(np.int64(T[0, i]), np.float32(P[0, i])) for i in range(J)]
                Pm = P.astype(np.float32)
            else:
                acts = [(int(T[0, i]), float(P[0, i])) for i in range(J)]
                Pm = P.astype(np.float64)
            rs = np.random.get_state()
            u = model._model(int(model.frame_of()[0])).draw_uniforms(T, Pm.astype(np.float64))
            np.random.set_state(rs)                          # the facade consumes the same draws
            o = model.step(T, Pm, u, arith32=(mode == "f32"))
            obs, rew, term, info = env.step(acts)
            st = env.get_state()
            assert len(obs) == J and all(x.tobytes() == st.tobytes() for x in obs), k
            assert st[tcols].tobytes() == o["theta_a"][0].astype(np.float32).tobytes(), k
            assert st[pcols].tobytes() == sc.motion_tables["positions"][k + 1].tobytes(), k
            assert info["radar_beam_azimuth"].tobytes() == o["theta_a"][0].tobytes(), k
            assert [s["is_tracking"] for s in info["radar_states"]] == o["track"][0].tolist(), k
            assert term == bool(o["terminated"][0])
            assert rew == pytest.approx(o["out"][0, 0], rel=1e-9, abs=1e-9)
            np.testing.assert_allclose(info["radar_pds"], o["pd"][0], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(info["snr_no_jamming"], o["snr_no"][0], rtol=1e-12, atol=0)
            levels.update(o["level_target"][0].tolist())
    assert len(levels) > 2                                   # the beams met the target through several levels
