"""Closed-loop episode launch for moving scenarios under scanning radars on the GPU (include/macjd_nets.h,
macjd_agent_env_episode_moving_scan), with and without a stepped antenna pattern: the env half and the hand-over
teacher-forced against ``env.step`` (macjd_env_step_moving_scan) on a second env, envs on different frames in one workgroup
and the clamp past the last frame, the float64 model (tests/moving_scan_model.py), the agent half per step against the
step-by-step agent path, graph replay, the switches, the entry point's refusals and the driver.  Inputs:
tests/moving_scan_cases.py (F = 24 frames).

Tolerances: integer outputs / azimuths / theta_a and position columns bit-equal, reward 1e-5 against the production step
(project bar) and bit-equal against the all-float64 step (MACJD_ENV_PD32=0), rdpj sums 1e-5 T, hidden state and power 1e-5,
arg-max within 2e-5 of the recomputed maximum (``_check_agent_half``)."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import moving_scan_cases as cases
from _harness import REPO, oracle_lib, random_actions
from moving_scan_model import MovingScanModel
from test_episode_scan_gpu import _check_agent_half
from test_moving_scan_gpu import DEV, PKG, _env, _runner, _third

pytestmark = pytest.mark.gpu
F = cases.F
SEED = 5          # _runner's env seed


@contextlib.contextmanager
def _pd32_off(monkeypatch, off):
    """MACJD_ENV_PD32=0: env.step runs its general all-float64 form, the closed-loop launch's own."""
    from macjd_amd import _native, options
    if off:
        monkeypatch.setenv("MACJD_ENV_PD32", "0")
        options.reload()
        _native.reload_options()
    try:
        yield
    finally:
        if off:
            monkeypatch.delenv("MACJD_ENV_PD32", raising=False)
            options.reload()
            _native.reload_options()


def _closed(sc, E, n_steps=None, test_mode=False):
    r, buf, args = _runner(sc, E, seed=SEED)
    r.closed_loop_moving_rollout = True
    assert r.closed_loop_moving_available()
    assert not r.closed_loop_available() and not r.closed_loop_pe_available() and not r.moving_rollout_available()
    assert not r.fused_rollout_available()
    r.rollout_closed_loop_moving(test_mode=test_mode, n_steps=n_steps)
    torch.cuda.synchronize()
    return r


def _teacher_forced(r, sc, env2, n, sum2, exact):
    """env2 stepped with ``env.step`` on the stored actions of staging rows 0 .. n - 1: theta_a and position columns of the
    rows, terminated, rewards (bit-equal when ``exact``)."""
    E, J = r.batch_envs, sc.num_jammers
    tcols, pcols = list(sc.theta_a_columns), list(sc.position_columns)
    dyn = tcols + pcols
    other = [c for c in range(sc.state_dim) if c not in dyn]
    static = torch.from_numpy(sc.state_vector()).to(DEV)
    st = r.stage
    worst = 0.0
    for t in range(n):
        s2 = env2.get_state()
        assert torch.equal(st["state"][t][:, dyn], s2[:, dyn]), t
        assert torch.equal(st["obs"][t][:, :, dyn], s2[:, dyn].unsqueeze(1).expand(-1, J, -1)), t
        assert torch.equal(st["state"][t][:, other], static[other].expand(E, -1)), t
        assert torch.equal(st["obs"][t][:, :, other], static[other].expand(E, J, -1)), t
        rew, term, _ = env2.step(st["actions_discrete"][t], st["actions_continuous"][t], rdpj_sum=sum2)
        assert torch.equal(st["terminated"][t].view(E), term), t
        if exact:
            assert torch.equal(st["reward"][t].view(E), rew), t
        worst = max(worst, (st["reward"][t].view(E) - rew).abs().max().item())
    return worst


def _hand_over(r, sc, env2):
    """The env is where single steps leave it, and one further common step agrees in every bit."""
    E, J, R = r.batch_envs, sc.num_jammers, sc.num_radars
    env1 = r.env
    assert torch.equal(env1.track, env2.track)
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(env1.get_state(), env2.get_state())
    pos = torch.from_numpy(sc.motion_tables["positions"]).to(DEV)
    k = torch.clamp(env1.step_count.to(torch.int64), max=F)
    assert torch.equal(env1.get_state()[:, list(sc.position_columns)], pos[k])
    assert torch.equal(env1.step_count, env2.step_count) and torch.equal(env1.episode_index, env2.episode_index)
    assert torch.equal(env1._snr_no_step, env2._snr_no_step)                      # the last step's value of its frame
    Tn, Pn = random_actions(np.random.default_rng(E), E, J, R)
    Td, Pd = torch.from_numpy(Tn).to(DEV), torch.from_numpy(Pn).to(DEV)
    r1, t1, i1 = env1.step(Td, Pd)
    r2, t2, i2 = env2.step(Td, Pd)
    assert torch.equal(i1["radar_tracking"], i2["radar_tracking"]) and torch.equal(t1, t2)
    assert torch.equal(i1["step_count"], i2["step_count"]) and torch.equal(i1["snr_no_jamming"], i2["snr_no_jamming"])
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(env1.get_state(), env2.get_state())
    assert torch.equal(r1, r2)   # same kernel, same inputs


def _check_episode(J, R, pattern, E, exact, monkeypatch):
    """A whole episode (T = F) from a reset: env half, hand-over and agent half."""
    sc, _ = cases.case(J, R, pattern)
    with _pd32_off(monkeypatch, exact):
        r = _closed(sc, E)
        assert (r.env._motion_scan_io.n_levels > 0) == pattern
        st = r.stage
        env2 = _env(sc, E, seed=SEED)
        env2.reset()
        assert torch.equal(env2.episode_index, r.env.episode_index)
        sum2 = torch.zeros((E, 3), dtype=torch.float32, device=DEV)
        worst = _teacher_forced(r, sc, env2, F, sum2, exact)
        sum_err = (r._rdpj_sum - sum2).abs().max().item()
        print(f"{J}j/{R}r pattern={pattern} E={E} exact={exact}: max |reward - env.step| = {worst:.3e}, "
              f"max |rdpj_sum diff| = {sum_err:.3e}")
        assert worst <= 1e-5
        assert sum_err <= 1e-5 * F
        assert not st["state"][F].any() and not st["obs"][F].any()                    # row T stays zero, as the step loop leaves it
        assert np.unique(st["state"][:F, :, sc.theta_a_columns[0]].cpu().numpy()).size > 5   # the loop really is closed
        assert torch.unique(st["actions_discrete"]).numel() >= 5
        assert st["terminated"][F - 1].all() and not st["terminated"][:F - 1].any()
        assert torch.equal(r.mac.hidden_states.view(E, J, -1), st["hidden_state"][F - 1])
        _hand_over(r, sc, env2)
    return r, sc


# ---------------------------------------------------------------------------------------------------------------
# 1. env half, hand-over and agent half: two full workgroups and half of one
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("pattern", [False, True])
def test_closed_loop_moving_env_half_agent_half_and_hand_over(pattern, exact, monkeypatch):
    r, sc = _check_episode(3, 4, pattern, 40, exact, monkeypatch)
    if not exact:
        _check_agent_half(r, sc, 40, False)


# ---------------------------------------------------------------------------------------------------------------
# 2. one workgroup holds envs on different frames; the envs that are not reset pass the last frame
@pytest.mark.parametrize("pattern", [False, True])
def test_mixed_frames_in_a_workgroup_and_the_clamp(pattern, monkeypatch):
    sc, _ = cases.case(3, 4, pattern)
    E, n0, n1 = 40, 5, F - 3
    with _pd32_off(monkeypatch, True):
        r = _closed(sc, E, n_steps=n0)
        env2 = _env(sc, E, seed=SEED)
        env2.reset()
        sum2 = torch.zeros((E, 3), dtype=torch.float32, device=DEV)
        _teacher_forced(r, sc, env2, n0, sum2, True)
        mask = _third(E)
        r.env.reset(mask)
        env2.reset(mask)
        assert torch.equal(r.env.get_state(), env2.get_state()) and torch.equal(r.env.episode_index, env2.episode_index)
        want0 = np.where(cases.third(E), 0, n0)
        np.testing.assert_array_equal(r.env.step_count.cpu().numpy(), want0)          # frames 0 and 5 in every workgroup
        r._upload_eps_schedule(r._eps_schedule(n1, False))
        r._closed_loop_launch(n1)                                                      # (no begin_episodes: the counters stay)
        torch.cuda.synchronize()
        worst = _teacher_forced(r, sc, env2, n1, sum2, True)
        assert worst == 0.0
        assert (r._rdpj_sum - sum2).abs().max().item() <= 1e-5 * (n0 + n1)
        np.testing.assert_array_equal(r.env.step_count.cpu().numpy(), want0 + n1)
        assert int(r.env.step_count.max()) == F + 2                                    # past F - 1 and positions[F]
        term = r.stage["terminated"][:n1].view(n1, E).cpu().numpy()
        np.testing.assert_array_equal(term, (want0[None, :] + np.arange(1, n1 + 1)[:, None]) >= F)
        _hand_over(r, sc, env2)


# ---------------------------------------------------------------------------------------------------------------
# 3. a one-env last workgroup
def test_closed_loop_moving_last_workgroup_with_one_env(monkeypatch):
    r, sc = _check_episode(3, 4, True, 17, True, monkeypatch)
    _check_agent_half(r, sc, 17, False)


# ---------------------------------------------------------------------------------------------------------------
# 4. the small size
@pytest.mark.parametrize("pattern", [False, True])
def test_closed_loop_moving_2j2r(pattern, monkeypatch):
    r, sc = _check_episode(2, 2, pattern, 40, True, monkeypatch)
    _check_agent_half(r, sc, 40, False)


# ---------------------------------------------------------------------------------------------------------------
# 5. env half against the float64 model
@pytest.mark.parametrize("pattern", [False, True])
def test_env_half_vs_moving_scan_model(pattern):
    J, R, E, n = 3, 4, 33, 12
    sc, frames = cases.case(J, R, pattern)
    tcols, pcols = list(sc.theta_a_columns), list(sc.position_columns)
    lib = oracle_lib()
    r = _closed(sc, E, n_steps=n)
    st = r.stage
    m = MovingScanModel(frames, E)
    ep = r.env.episode_index.cpu().numpy()
    off, seed = int(r.env.env_offset), int(r.env.seed)
    pos = sc.motion_tables["positions"]
    worst, tracks, o = 0.0, set(), None
    for t in range(n):
        np.testing.assert_array_equal(st["state"][t][:, tcols].cpu().numpy(), m.theta_a.astype(np.float32))
        assert st["state"][t][:, pcols].cpu().numpy().tobytes() == m.positions_after(pos).tobytes(), t
        u = np.array([[lib.macjd_oracle_uniform(seed, off + e, int(ep[e]), t, k) for k in range(R + J)] for e in range(E)])
        Tt = st["actions_discrete"][t].view(E, J).cpu().numpy()
        Pt = st["actions_continuous"][t].view(E, J).cpu().numpy()
        o = m.step(Tt, Pt, u, arith32=True)
        np.testing.assert_array_equal(st["terminated"][t].view(E).cpu().numpy(), o["terminated"])
        worst = max(worst, np.abs(st["reward"][t].view(E).cpu().numpy() - o["out"][:, 0]).max())
        tracks.update(np.unique(o["track"]).tolist())
    print(f"pattern={pattern}: max |reward - model| = {worst:.3e}, target paths per level {m.count_target.tolist()}, recorded "
          f"jammer actions per level {m.count_jammer.tolist()}, track values {sorted(tracks)}")
    assert worst <= 1e-5
    np.testing.assert_array_equal(r.env.track.cpu().numpy().astype(bool), o["track"])
    assert r.env.beam_azimuth.cpu().numpy().tobytes() == np.ascontiguousarray(o["theta_a"]).tobytes()
    np.testing.assert_array_equal(r.env.get_state()[:, tcols].cpu().numpy(), o["theta_a"].astype(np.float32))
    assert r.env.get_state()[:, pcols].cpu().numpy().tobytes() == m.positions_after(pos).tobytes()
    assert int(r.env.step_count[0]) == n
    # coverage, from the model's own record on the stored actions
    assert m.count_target[0] > 0 and m.count_target[-1] > 0          # the target through the main and the side lobe
    assert m.count_jammer[0] > 0 and m.count_jammer[-1] > 0          # a recorded jammer action in each
    if pattern:
        assert m.count_target[1:-1].sum() > 0 and m.count_jammer[1:-1].sum() > 0   # ... and through an intermediate level
    assert tracks == {False, True}


# ---------------------------------------------------------------------------------------------------------------
# 6. graph replay
def test_graph_replay_equals_eager_closed_loop_moving():
    sc, _ = cases.case(3, 4, True)
    E = 64
    r_e, b_e, _ = _runner(sc, E)
    r_g, b_g, _ = _runner(sc, E)
    r_e.closed_loop_moving_rollout = r_g.closed_loop_moving_rollout = True
    assert r_g.closed_loop_moving_available()
    r_g.enable_graph()
    try:
        for _ in range(2):
            s_e = r_e.run(sync_stats=True)
            s_g = r_g.run(sync_stats=True)
            assert s_e["episode_return"] == s_g["episode_return"]
        for k in b_e.buffers:
            assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(r_e.mac.hidden_states, r_g.mac.hidden_states)
        assert r_e.t_env == r_g.t_env == 2 * F
    finally:
        r_g.release_graphs()


# ---------------------------------------------------------------------------------------------------------------
# 7. the switches
def test_switches_and_refusing_rollouts(monkeypatch):
    import motion_cases
    from macjd_amd import ops
    from macjd_amd.scenario import Scenario
    sc, frames = cases.case(3, 4, True)
    r, _, _ = _runner(sc, 32)
    assert r.closed_loop_moving_rollout is False and r.closed_loop_moving_available()
    calls = []
    real = ops.agent_env_episode_moving_scan

    def boom(*a, **k):
        raise AssertionError("moving closed-loop launch without its switch")
    monkeypatch.setattr(ops, "agent_env_episode_moving_scan", boom)
    r.run(sync_stats=True)                                           # switch off: the step loop
    assert r.t_env == F
    r.closed_loop_rollout = r.moving_episode_rollout = True          # the two old switches alone do not select it
    r.run(sync_stats=True)
    assert r.t_env == 2 * F
    assert not r.closed_loop_available() and not r.closed_loop_pe_available() and not r.moving_rollout_available()
    with pytest.raises(RuntimeError, match="not available"):
        r.rollout_closed_loop()
    r.closed_loop_rollout = r.moving_episode_rollout = False
    monkeypatch.setattr(ops, "agent_env_episode_moving_scan", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    r.closed_loop_moving_rollout = True
    r.run(sync_stats=True)
    assert calls == [1] and r.t_env == 3 * F
    # kernel_flags != 0
    from macjd_amd import _native
    r.env.kernel_flags = _native.STEP_LANE_KERNEL
    assert not r.closed_loop_moving_available()
    with pytest.raises(RuntimeError, match="closed_loop_moving_available"):
        r.rollout_closed_loop_moving()
    r.env.kernel_flags = 0
    # a static scanning env and a moving non-scanning env: not this launch's
    r_static, _, _ = _runner(frames[0], 16)
    assert r_static.closed_loop_available() and not r_static.closed_loop_moving_available()
    with pytest.raises(RuntimeError, match="closed_loop_moving_available"):
        r_static.rollout_closed_loop_moving()
    with pytest.raises(RuntimeError, match="both moves and scans"):
        r_static.env.episode_moving_scan_args()
    moving = Scenario.from_dict(motion_cases.moving_ring_dict(3, 4), config=motion_cases.config())
    r_mov, _, _ = _runner(moving, 16)
    assert not r_mov.closed_loop_moving_available()
    with pytest.raises(RuntimeError, match="closed_loop_moving_available"):
        r_mov.rollout_closed_loop_moving()
    with pytest.raises(RuntimeError, match="both moves and scans"):
        r_mov.env.episode_moving_scan_args()
    with pytest.raises(RuntimeError, match="moving scenario"):
        r.env.episode_scan_args()


# ---------------------------------------------------------------------------------------------------------------
# 8. the entry point's refusals: each returns its code and names the argument, before any launch
def test_entry_point_refusals(monkeypatch):
    import motion_cases
    from macjd_amd import _native, ops
    from macjd_amd.scenario import Scenario
    J, R, E = 3, 4, 16
    sc, frames = cases.case(J, R, True)
    r, _, _ = _runner(sc, E)
    r.closed_loop_moving_rollout = True
    captured = {}
    lib = _native.load()
    real = lib.macjd_agent_env_episode_moving_scan
    IO = _native.AgentEnvEpisodeMovingScanIO

    class Spy:   # keeps a copy of the argument block of a valid call
        def __getattr__(self, name):
            return getattr(lib, name)

        def macjd_agent_env_episode_moving_scan(self, h, ref, stream):
            captured["io"] = IO.from_buffer_copy(ref._obj)
            captured["h"], captured["stream"] = h, stream
            return real(h, ref, stream)
    real_load = _native.load
    monkeypatch.setattr(_native, "load", lambda: Spy())
    r.rollout_closed_loop_moving(n_steps=2)
    torch.cuda.synchronize()
    monkeypatch.setattr(_native, "load", real_load)
    good, h, stream = captured["io"], captured["h"], captured["stream"]
    err = lambda: lib.macjd_last_error().decode()
    before = {k: v.clone() for k, v in r.stage.items()}
    state0, step0, az0 = r.env.get_state().clone(), r.env.step_count.clone(), r.env.beam_azimuth.clone()

    def call(handle=h, **changes):
        io_ = IO.from_buffer_copy(good)
        for path, v in changes.items():
            obj, parts = io_, path.split("__")
            for p in parts[:-1]:
                obj = getattr(obj, p)
            setattr(obj, parts[-1], v)
        return lib.macjd_agent_env_episode_moving_scan(handle, ctypes.byref(io_), stream)

    assert call(motion__frames=None) == -1 and "frames / frame_flags" in err()
    assert call(motion__frame_flags=None) == -1 and "frames / frame_flags" in err()
    assert call(motion__positions=None) == -1 and "positions" in err()
    assert call(motion__position_columns=None) == -1 and "position_columns" in err()
    assert call(motion_scan__scan_frames=None) == -1 and "scan_frames" in err()
    assert call(motion__n_frames=0) == -1 and "n_frames < 1" in err()
    assert call(motion__n_frames=F - 1) == -1 and "episode_limit" in err()
    assert call(motion__n_pos=2 * R + 2 * J - 1) == -1 and "n_pos" in err()
    assert call(motion__snr_no=r.env._snr_no_step.data_ptr()) == -1 and "motion.snr_no must be NULL" in err()
    other = torch.zeros_like(r.env._state_dyn)
    assert call(motion__state=other.data_ptr()) == -1 and "same rows" in err()
    assert call(motion__state=None) == -1 and "state is NULL" in err()
    assert call(motion_scan__n_levels=0) == -1 and "n_levels differs" in err()         # (the env's handle has L = 4)
    assert call(motion_scan__n_levels=7) == -1 and "n_levels outside" in err()
    assert call(motion_scan__n_levels=-1) == -1 and "n_levels outside" in err()
    assert call(base__pe_tables=good.motion.frames) == -1 and "pe_tables must be NULL" in err()
    assert call(base__J=6, base__R=8, base__A=17) == -4 and "unsupported" in err()
    assert call(base__H=128) == -4 and "unsupported" in err()
    assert lib.macjd_agent_env_episode_moving_scan(h, None, stream) == -1 and "NULL" in err()
    with torch.cuda.device(DEV):
        static = _native.ScenarioHandle(Scenario.from_dict(motion_cases.moving_ring_dict(J, R), config=motion_cases.config()))
        pat2_d = cases.moving_scan_dict(J, R, True)
        pat2_d["environment_params"]["radar_scan"]["pattern"]["gain_db"] = [-3, -12]
        pat2 = _native.ScenarioHandle(Scenario.from_dict(pat2_d, config=motion_cases.config()))
        plain = _native.ScenarioHandle(cases.case(J, R, False)[0])
    assert call(handle=static.ptr) == -1 and "no scanning tables" in err()
    assert call(handle=pat2.ptr) == -1 and "n_levels differs" in err()                 # the handle's L = 2, the call's 4
    assert call(handle=plain.ptr, motion_scan__n_levels=0) == -1 and "go together" in err()       # pattern_frames without levels
    assert call(handle=plain.ptr, motion_scan__pattern_frames=None) == -1 and "go together" in err()   # ... and the reverse
    # the two other closed-loop entry points keep their refusals on this block's base
    assert lib.macjd_agent_env_episode_scan_pe(h, ctypes.byref(_pe_block(_native, good)), stream) == -1 and "pe_tables" in err()
    # none of the refused calls launched
    torch.cuda.synchronize()
    assert torch.equal(r.env.step_count, step0) and torch.equal(r.env.get_state(), state0)
    assert torch.equal(r.env.beam_azimuth, az0)
    for k in r.stage:
        assert torch.equal(r.stage[k], before[k]), k
    assert ops.agent_env_episode_moving_scan_supported(3, 4, 64, 9) and ops.agent_env_episode_moving_scan_supported(2, 2, 64, 5)
    assert not ops.agent_env_episode_moving_scan_supported(3, 4, 128, 9)


def _pe_block(_native, good):
    pio = _native.AgentEnvEpisodeScanPeIO()
    ctypes.memmove(ctypes.addressof(pio), ctypes.addressof(good.base), ctypes.sizeof(_native.AgentEnvEpisodeScanIO))
    return pio


# ---------------------------------------------------------------------------------------------------------------
# 9. the driver, in a fresh process with the switch on
_DRIVER = r'''
import contextlib, io, math, os, sys
sys.path.insert(0, %(repo)r)
from macjd_amd import ops
calls = []
real = ops.agent_env_episode_moving_scan
ops.agent_env_episode_moving_scan = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
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
print("RESULT", res["total_steps"], res["episodes"], res["train_steps"], int("Training finished." in out.getvalue()), len(calls))
import re
print("LOSSES", " ".join(re.findall(r"Avg Loss: (\S+)", out.getvalue())))
'''


def test_driver_trains_with_the_moving_closed_loop_rollout_in_a_fresh_process(tmp_path):
    env = dict(os.environ, MACJD_CLOSED_LOOP_MOVING_ROLLOUT="1")
    out = subprocess.run([sys.executable, "-c", _DRIVER % {"repo": REPO, "pkg": PKG, "tmp": str(tmp_path)}],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    E = 32
    assert [int(x) for x in line[1:3]] == [2 * E * F, 2 * E] and int(line[3]) > 0 and line[4] == "1"
    assert int(line[5]) > 0, "the driver never issued the moving closed-loop launch"
    losses = [float(x) for x in [l for l in out.stdout.splitlines() if l.startswith("LOSSES")][-1].split()[1:]]
    assert losses and all(np.isfinite(x) for x in losses), losses
