"""Closed-loop episode launch on per-env moving scanning scenario batches on the GPU (include/macjd_nets.h,
macjd_agent_env_episode_moving_scan_pe), with and without a stepped antenna pattern: the env half and the hand-over
teacher-forced against ``env.step`` (macjd_env_step_moving_scan_pe) on a second env, copies of one scenario against the
shared-frame launch, tile widths that split a workgroup's envs over several tiles (padding lanes poisoned), envs on different
frames in one workgroup and the clamp past the last frame, the float64 model (tests/moving_scan_model.py, one per env), the
agent half per step against the step-by-step agent path, graph replay, the switch, the entry point's refusals and the driver.
Inputs: tests/moving_scan_pe_model.py (F_PE = 5 frames, the edge envs, the crosser and the seam env first).

Tolerances (the project's existing ones): integer outputs / azimuths / theta_a and position columns bit-equal, reward 1e-5
against the production step and bit-equal against the all-float64 step (MACJD_ENV_PD32=0), rdpj sums 1e-5 T, hidden state and
power 1e-5, arg-max within 2e-5 of the recomputed maximum (``_check_agent_half``)."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_cases
import moving_scan_cases as msc
import moving_scan_pe_model as spm
from _harness import REPO, oracle_lib, random_actions
from moving_scan_model import MovingScanModel
from test_episode_moving_scan_gpu import _pd32_off
from test_episode_scan_gpu import _check_agent_half
from test_moving_scan_pe_gpu import DEV, JITTER, PKG, _base, _batch, _env, _ms_env, _runner, _third
from test_nets_cpu import make_args, quiet
from tiled_frames import gather_frames

from macjd_amd.scenario import MovingScanScenarioBatch, MovingScenarioBatch, Scenario, ScenarioBatch, motion_frame_dict

pytestmark = pytest.mark.gpu
F = spm.F_PE
SEED = 5          # _runner's env seed
TILE_RUN = 256    # _runner's env tile
STAGE_KEYS = ("state", "obs", "hidden_state", "actions_discrete", "actions_continuous", "reward", "terminated")


def _runner_on(env):
    """``test_moving_scan_pe_gpu._runner`` around a given environment (same agent weights: torch.manual_seed(3))."""
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    info = env.get_env_info()
    E = env.batch_envs
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


def _positions_of(env, k):
    """f32 [E, n_pos]: env e's position columns of frame k[e], read from the device table by the index model."""
    tab = env._motion_keep["positions"].cpu().numpy()
    k = np.asarray(k, dtype=np.int64)
    return torch.from_numpy(gather_frames(tab, np.arange(env.batch_envs), k)).to(DEV)


def _closed(mb, tile=TILE_RUN, n_steps=None, test_mode=False):
    r, _, _ = _runner_on(_ms_env(mb, tile=tile, seed=SEED))
    r.closed_loop_moving_pe_rollout = True
    assert r.closed_loop_moving_pe_available()
    assert not r.closed_loop_available() and not r.closed_loop_pe_available() and not r.closed_loop_moving_available()
    assert not r.moving_rollout_available() and not r.moving_pe_rollout_available() and not r.fused_rollout_available()
    r.rollout_closed_loop_moving_pe(test_mode=test_mode, n_steps=n_steps)
    torch.cuda.synchronize()
    return r


def _teacher_forced(r, mb, env2, n, sum2, exact):
    """env2 stepped with ``env.step`` on the stored actions of staging rows 0 .. n - 1: theta_a and position columns of the
    rows (every other column: the env's own state row), terminated, rewards (bit-equal when ``exact``)."""
    sc = mb.base
    E, J = r.batch_envs, sc.num_jammers
    tcols, pcols = list(sc.theta_a_columns), list(sc.position_columns)
    dyn = tcols + pcols
    other = [c for c in range(sc.state_dim) if c not in dyn]
    static = torch.from_numpy(mb.state_vectors).to(DEV)     # [E, S]
    st = r.stage
    worst = 0.0
    for t in range(n):
        s2 = env2.get_state()
        assert torch.equal(st["state"][t][:, dyn], s2[:, dyn]), t
        assert torch.equal(st["obs"][t][:, :, dyn], s2[:, dyn].unsqueeze(1).expand(-1, J, -1)), t
        assert torch.equal(st["state"][t][:, other], static[:, other]), t
        assert torch.equal(st["obs"][t][:, :, other], static[:, other].unsqueeze(1).expand(-1, J, -1)), t
        rew, term, _ = env2.step(st["actions_discrete"][t], st["actions_continuous"][t], rdpj_sum=sum2)
        assert torch.equal(st["terminated"][t].view(E), term), t
        if exact:
            assert torch.equal(st["reward"][t].view(E), rew), t
        worst = max(worst, (st["reward"][t].view(E) - rew).abs().max().item())
    return worst


def _hand_over(r, mb, env2):
    """The env is where single steps leave it, and one further common step agrees in every bit."""
    sc = mb.base
    E, J, R = r.batch_envs, sc.num_jammers, sc.num_radars
    env1 = r.env
    assert torch.equal(env1.track, env2.track)
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(env1.get_state(), env2.get_state())
    k = np.minimum(env1.step_count.cpu().numpy(), F)
    assert torch.equal(env1.get_state()[:, list(sc.position_columns)], _positions_of(env1, k))
    assert torch.equal(env1.step_count, env2.step_count) and torch.equal(env1.episode_index, env2.episode_index)
    assert torch.equal(env1._snr_no_step, env2._snr_no_step)                      # the last step's value of the env's own frame
    Tn, Pn = random_actions(np.random.default_rng(E), E, J, R)
    Td, Pd = torch.from_numpy(Tn).to(DEV), torch.from_numpy(Pn).to(DEV)
    r1, t1, i1 = env1.step(Td, Pd)
    r2, t2, i2 = env2.step(Td, Pd)
    assert torch.equal(i1["radar_tracking"], i2["radar_tracking"]) and torch.equal(t1, t2)
    assert torch.equal(i1["step_count"], i2["step_count"]) and torch.equal(i1["snr_no_jamming"], i2["snr_no_jamming"])
    assert env1.beam_azimuth.cpu().numpy().tobytes() == env2.beam_azimuth.cpu().numpy().tobytes()
    assert torch.equal(env1.get_state(), env2.get_state())
    assert torch.equal(env1._snr_no_step, env2._snr_no_step)
    assert torch.equal(r1, r2)   # same kernel, same inputs


def _check_episode(J, R, L, E, compiled, exact, monkeypatch):
    """A whole episode (T = F) from a reset: env half and hand-over."""
    mb, _ = _batch(J, R, L, E, compiled)
    sc = mb.base
    with _pd32_off(monkeypatch, exact):
        r = _closed(mb)
        assert r.env._motion_scan_pe_io.n_levels == L and int(r.env._motion_pe_io.tile) == TILE_RUN
        st = r.stage
        env2 = _ms_env(mb, tile=TILE_RUN, seed=SEED)
        env2.reset()
        assert torch.equal(env2.episode_index, r.env.episode_index)
        sum2 = torch.zeros((E, 3), dtype=torch.float32, device=DEV)
        worst = _teacher_forced(r, mb, env2, F, sum2, exact)
        sum_err = (r._rdpj_sum - sum2).abs().max().item()
        print(f"{J}j/{R}r L={L} E={E} {compiled} exact={exact}: max |reward - env.step| = {worst:.3e}, "
              f"max |rdpj_sum diff| = {sum_err:.3e}")
        assert worst <= 1e-5
        assert sum_err <= 1e-5 * F
        assert not st["state"][F].any() and not st["obs"][F].any()                    # row T stays zero, as the step loop leaves it
        assert np.unique(st["state"][:F, :, sc.theta_a_columns[0]].cpu().numpy()).size > 5   # the loop really is closed
        assert torch.unique(st["actions_discrete"]).numel() >= 5
        assert st["terminated"][F - 1].all() and not st["terminated"][:F - 1].any()
        assert torch.equal(r.mac.hidden_states.view(E, J, -1), st["hidden_state"][F - 1])
        _hand_over(r, mb, env2)
    return r, mb


# ---------------------------------------------------------------------------------------------------------------
# 1. env half, hand-over and agent half: two full workgroups and half of one
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("compiled", ["host", "device"])
@pytest.mark.parametrize("L", [0, 4])
def test_closed_loop_moving_pe_env_half_agent_half_and_hand_over(L, compiled, exact, monkeypatch):
    r, mb = _check_episode(3, 4, L, 40, compiled, exact, monkeypatch)
    if not exact:
        _check_agent_half(r, mb.base, 40, False)


# ---------------------------------------------------------------------------------------------------------------
# 2. copies of one scenario: the shared-frame launch — same kernel, same values, other addresses
def _outputs(r):
    env = r.env
    out = {k: r.stage[k] for k in STAGE_KEYS}
    out.update(hidden=r.mac.hidden_states, rdpj=r._rdpj_sum, env_state=env.get_state(), theta_a=env.beam_azimuth, track=env.track,
               step=env.step_count, episode=env.episode_index, snr_no=env._snr_no_step)
    return out


@pytest.mark.parametrize("pattern", [False, True])
def test_copies_of_one_scenario_equal_the_shared_frame_launch(pattern):
    from test_moving_scan_gpu import _runner as shared_runner
    sc = Scenario.from_dict(msc.moving_scan_dict(3, 4, pattern), config=spm.config())
    E = 40
    a, _, _ = shared_runner(sc, E, seed=SEED)
    a.closed_loop_moving_rollout = True
    assert a.closed_loop_moving_available()
    a.rollout_closed_loop_moving()
    b = _closed(MovingScanScenarioBatch([sc] * E), tile=16)
    torch.cuda.synchronize()
    oa, ob = _outputs(a), _outputs(b)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    assert a.env.track.any() or torch.unique(oa["actions_discrete"]).numel() >= 5


# ---------------------------------------------------------------------------------------------------------------
# 3. tile widths: a workgroup's 16 envs over four unaligned tiles (5), over two (8), in one (16) and in a padded one (256)
def _poisoned(mb):
    """``mb`` whose device tables carry NaN (flag bytes: 0xFF) in the padding lanes of the last tile, edited before upload."""
    pb = copy.copy(mb)
    real = mb.tiled

    def tiled(w):
        out = {k: np.array(a, copy=True) for k, a in real(w).items()}
        pad = out["frames"].shape[0] * w - mb.n_envs
        if pad:
            for a in out.values():
                a[-1, ..., w - pad:] = 0xFF if a.dtype == np.uint8 else np.nan
        return out
    pb.tiled = tiled
    return pb


@pytest.mark.parametrize("E", [40, 17])
@pytest.mark.parametrize("L", [0, 4])
def test_tile_widths_agree_bit_for_bit_and_padding_lanes_are_never_read(L, E):
    mb, _ = _batch(3, 4, L, E, "host")
    pb = _poisoned(mb)
    ref = None
    for tile in (16, 5, 8, 256):
        r = _closed(pb, tile=tile)
        keep = r.env._motion_keep
        n_pad = keep["frames"].shape[0] * tile - E
        if n_pad:                                               # the poison is in place
            assert torch.isnan(keep["frames"][-1, ..., tile - n_pad:]).all()
            assert torch.isnan(keep["positions"][-1, ..., tile - n_pad:]).all()
            assert torch.isnan(keep["scan_frames"][-1, ..., tile - n_pad:]).all()
        out = {k: v.clone() for k, v in _outputs(r).items()}
        for k, v in out.items():
            if v.is_floating_point():
                assert torch.isfinite(v).all(), (tile, k)
        if ref is None:
            ref = out
            assert torch.unique(out["actions_discrete"]).numel() >= 5
            continue
        for k in ref:
            assert torch.equal(ref[k], out[k]), (tile, k)


# ---------------------------------------------------------------------------------------------------------------
# 4. one workgroup holds envs on different frames; every env passes the last frame
@pytest.mark.parametrize("L", [0, 4])
def test_mixed_frames_in_a_workgroup_and_the_clamp(L, monkeypatch):
    E, n0, n1 = 40, 2, F
    assert n0 + n1 > F
    mb, _ = _batch(3, 4, L, E, "host")
    sc = mb.base
    with _pd32_off(monkeypatch, True):
        r = _closed(mb, n_steps=n0)
        env2 = _ms_env(mb, tile=TILE_RUN, seed=SEED)
        env2.reset()
        sum2 = torch.zeros((E, 3), dtype=torch.float32, device=DEV)
        _teacher_forced(r, mb, env2, n0, sum2, True)
        mask = _third(E)
        r.env.reset(mask)
        env2.reset(mask)
        assert torch.equal(r.env.get_state(), env2.get_state()) and torch.equal(r.env.episode_index, env2.episode_index)
        want0 = np.where(np.arange(E) % 3 == 0, 0, n0)
        np.testing.assert_array_equal(r.env.step_count.cpu().numpy(), want0)          # frames 0 and n0 in every workgroup
        r._upload_eps_schedule(r._eps_schedule(n1, False))
        r._closed_loop_launch(n1)                                                      # (no begin_episodes: the counters stay)
        torch.cuda.synchronize()
        pcols = list(sc.position_columns)
        for t in range(n1):                                                            # positions of frame min(step0 + t, F)
            assert torch.equal(r.stage["state"][t][:, pcols], _positions_of(r.env, np.minimum(want0 + t, F))), t
        worst = _teacher_forced(r, mb, env2, n1, sum2, True)
        assert worst == 0.0
        assert (r._rdpj_sum - sum2).abs().max().item() <= 1e-5 * (n0 + n1)
        np.testing.assert_array_equal(r.env.step_count.cpu().numpy(), want0 + n1)
        assert int(r.env.step_count.max()) == F + n0 and int(r.env.step_count.min()) == F   # past F - 1 and positions[F]
        term = r.stage["terminated"][:n1].view(n1, E).cpu().numpy()
        np.testing.assert_array_equal(term, (want0[None, :] + np.arange(1, n1 + 1)[:, None]) >= F)
        assert torch.equal(r.env.get_state()[:, pcols], _positions_of(r.env, np.full(E, F)))
        _hand_over(r, mb, env2)


# ---------------------------------------------------------------------------------------------------------------
# 5. env half against the float64 model, one model per env on its own frames
MODEL_LIMIT = {0: F, 4: F}    # frames (= steps) of the model cases per L: raised (at most 24) where coverage needs it


@pytest.mark.parametrize("L", [0, 4])
def test_env_half_vs_moving_scan_model(L):
    J, R, E = 3, 4, spm.E0
    n = MODEL_LIMIT[L]
    assert F <= n <= 24
    dicts, scs = spm.case(J, R, L, E=E, limit=n)
    mb = MovingScanScenarioBatch(scs)
    sc = mb.base
    tcols, pcols = list(sc.theta_a_columns), list(sc.position_columns)
    lib = oracle_lib()
    r = _closed(mb)
    assert r.episode_limit == n
    st = r.stage
    models = [MovingScanModel(spm.env_frames(d, n), 1) for d in dicts]
    ep = r.env.episode_index.cpu().numpy()
    off, seed = int(r.env.env_offset), int(r.env.seed)
    ar = np.arange(E)
    worst, tracks, outs = 0.0, set(), None
    for t in range(n):
        theta = np.concatenate([m.theta_a for m in models])
        np.testing.assert_array_equal(st["state"][t][:, tcols].cpu().numpy(), theta.astype(np.float32))
        assert st["state"][t][:, pcols].cpu().numpy().tobytes() == mb.positions[ar, min(t, n)].tobytes(), t
        Tt = st["actions_discrete"][t].view(E, J).cpu().numpy()
        Pt = st["actions_continuous"][t].view(E, J).cpu().numpy()
        outs = []
        for e, m in enumerate(models):
            u = np.array([[lib.macjd_oracle_uniform(seed, off + e, int(ep[e]), t, k) for k in range(R + J)]])
            outs.append(m.step(Tt[e:e + 1], Pt[e:e + 1], u, arith32=True))
        rew = np.concatenate([o["out"][:, 0] for o in outs])
        np.testing.assert_array_equal(st["terminated"][t].view(E).cpu().numpy(), np.concatenate([o["terminated"] for o in outs]))
        worst = max(worst, np.abs(st["reward"][t].view(E).cpu().numpy() - rew).max())
        for o in outs:
            tracks.update(np.unique(o["track"]).tolist())
    count_target = sum(m.count_target for m in models)
    count_jammer = sum(m.count_jammer for m in models)
    print(f"L={L} steps={n}: max |reward - model| = {worst:.3e}, target paths per level {count_target.tolist()}, recorded "
          f"jammer actions per level {count_jammer.tolist()}, track values {sorted(tracks)}")
    assert worst <= 1e-5
    track = np.concatenate([o["track"] for o in outs])
    theta = np.concatenate([o["theta_a"] for o in outs])
    np.testing.assert_array_equal(r.env.track.cpu().numpy().astype(bool), track)
    assert r.env.beam_azimuth.cpu().numpy().tobytes() == np.ascontiguousarray(theta).tobytes()
    np.testing.assert_array_equal(r.env.get_state()[:, tcols].cpu().numpy(), theta.astype(np.float32))
    assert r.env.get_state()[:, pcols].cpu().numpy().tobytes() == mb.positions[ar, n].tobytes()
    assert int(r.env.step_count[0]) == n
    # coverage, from the models' own record on the stored actions
    assert count_target[0] > 0 and count_target[-1] > 0          # the target through the main and the side lobe
    assert count_jammer[0] > 0 and count_jammer[-1] > 0          # a recorded jammer action in each
    if L:
        assert count_target[1:-1].sum() > 0 and count_jammer[1:-1].sum() > 0   # ... and through an intermediate level
    assert tracks == {False, True}


# ---------------------------------------------------------------------------------------------------------------
# 6. the small size
@pytest.mark.parametrize("L", [0, 4])
def test_closed_loop_moving_pe_2j2r(L, monkeypatch):
    r, mb = _check_episode(2, 2, L, 40, "host", True, monkeypatch)
    _check_agent_half(r, mb.base, 40, False)


# ---------------------------------------------------------------------------------------------------------------
# 7. graph replay equals eager; the step loop beside them
def test_graph_replay_equals_eager_and_the_step_loop_agrees(monkeypatch):
    from macjd_amd import ops
    E = 40
    mb, _ = _batch(3, 4, 4, E, "device")
    sc = mb.base
    calls = []
    real = ops.agent_env_episode_moving_scan_pe
    monkeypatch.setattr(ops, "agent_env_episode_moving_scan_pe", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    r_e, b_e, _ = _runner(mb)
    r_g, b_g, _ = _runner(mb)
    r_l, b_l, _ = _runner(mb)
    r_e.closed_loop_moving_pe_rollout = r_g.closed_loop_moving_pe_rollout = True
    assert r_l.closed_loop_moving_pe_rollout is False and r_l.closed_loop_moving_pe_available()
    r_g.enable_graph()
    n_capture = len(calls)
    assert n_capture == 2                                       # warm-up and capture
    try:
        for i in range(2):
            s_e = r_e.run(sync_stats=True)
            assert len(calls) == n_capture + i + 1              # one launch per eager episode batch
            s_g = r_g.run(sync_stats=True)
            assert len(calls) == n_capture + i + 1              # the replay issues it from the graph
            r_l.run(sync_stats=True)
            assert len(calls) == n_capture + i + 1              # available, yet the step loop ran
            assert s_e["episode_return"] == s_g["episode_return"]
        for k in b_e.buffers:
            assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(r_e.mac.hidden_states, r_g.mac.hidden_states)
        assert r_e.t_env == r_g.t_env == r_l.t_env == 2 * F
    finally:
        r_g.release_graphs()
    # eager launch against the eager step loop: positions equal; rewards wherever the stored actions agree up to that step
    pcols = list(sc.position_columns)
    n = 2 * E
    assert torch.equal(b_e.buffers["state"][:n, :F][:, :, pcols], b_l.buffers["state"][:n, :F][:, :, pcols])
    a_e, a_l = b_e.buffers["actions_discrete"][:n, :F], b_l.buffers["actions_discrete"][:n, :F]
    same = (a_e == a_l).reshape(n, F, -1).all(dim=2)
    upto = torch.cumprod(same.to(torch.int64), dim=1).bool()                    # [n, F]
    rew_e, rew_l = b_e.buffers["reward"][:n, :F].reshape(n, F), b_l.buffers["reward"][:n, :F].reshape(n, F)
    assert float(upto.float().mean()) > 0.5, float(upto.float().mean())
    worst = float((rew_e - rew_l).abs()[upto].max())
    print(f"launch against step loop: stored actions agree up to the step on {float(upto.float().mean()):.4f} of the rows, "
          f"max |reward diff| there = {worst:.3e}")
    assert worst <= 1e-5


# ---------------------------------------------------------------------------------------------------------------
# 8. the switch and the names
EARLIER_PREDICATES = ("closed_loop_available", "closed_loop_pe_available", "closed_loop_moving_available", "moving_rollout_available",
                      "moving_pe_rollout_available", "fused_rollout_available")
EARLIER_ROLLOUTS = ("rollout_closed_loop", "rollout_closed_loop_pe", "rollout_closed_loop_moving", "rollout_moving",
                    "rollout_moving_pe")


def test_switch_and_refusing_rollouts(monkeypatch):
    from macjd_amd import _native, ops
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    E = 16
    mb, static = _batch(3, 4, 4, E, "host")
    r, _, _ = _runner(mb)
    assert r.closed_loop_moving_pe_rollout is False and r.closed_loop_moving_pe_available()
    for name in EARLIER_PREDICATES:
        assert getattr(r, name)() is False, name
    for name in EARLIER_ROLLOUTS:
        with pytest.raises(RuntimeError, match="not available"):
            getattr(r, name)()
    calls = []
    real = ops.agent_env_episode_moving_scan_pe
    monkeypatch.setattr(ops, "agent_env_episode_moving_scan_pe", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    r.run(sync_stats=True)                                           # switch off: the step loop
    assert calls == [] and r.t_env == F
    r.closed_loop_moving_pe_rollout = True
    r.run(sync_stats=True)
    r.run(sync_stats=True)
    assert calls == [1, 1] and r.t_env == 3 * F                     # once per episode batch
    for bad in (0, F + 1, -1):
        with pytest.raises(ValueError, match=r"rollout_closed_loop_moving_pe: n_steps must be in 1\.\."):
            r.rollout_closed_loop_moving_pe(n_steps=bad)
    r.env.kernel_flags = _native.STEP_LANE_KERNEL
    assert not r.closed_loop_moving_pe_available()
    with pytest.raises(RuntimeError, match="closed_loop_moving_pe_available"):
        r.rollout_closed_loop_moving_pe()
    r.env.kernel_flags = 0
    assert r.closed_loop_moving_pe_available()
    # the other env kinds: not this launch's
    shared = Scenario.from_dict(msc.moving_scan_dict(3, 4, True), config=spm.config())
    moving = Scenario.from_dict(motion_cases.moving_ring_dict(3, 4), config=spm.config())
    others = {"shared-frame moving scanning": _env(shared, E),
              "moving_batch": Env(moving_batch=MovingScenarioBatch([moving] * E), device=DEV),
              "static scanning batch": Env(scenario_batch=ScenarioBatch([static] * E, scan=True, pattern=True), device=DEV)}
    for kind, env in others.items():
        ro, _, _ = _runner_on(env)
        ro.closed_loop_moving_pe_rollout = True
        assert not ro.closed_loop_moving_pe_available(), kind
        with pytest.raises(RuntimeError, match="closed_loop_moving_pe_available"):
            ro.rollout_closed_loop_moving_pe()
        with pytest.raises(RuntimeError, match="episode_moving_scan_pe_args: needs a per-env moving scanning scenario batch"):
            env.episode_moving_scan_pe_args()
    assert calls == [1, 1]
    args = r.env.episode_moving_scan_pe_args()
    assert set(args) == {"handle", "scan_io", "motion_pe_io", "motion_scan_pe_io", "track", "step", "episode", "seed", "env_offset",
                         "n_radars", "pe_tables"}
    assert args["pe_tables"] is None and args["scan_io"].snr_no == r.env._snr_no_step.data_ptr()
    assert ops.agent_env_episode_moving_scan_pe_supported(3, 4, 64, 9) and ops.agent_env_episode_moving_scan_pe_supported(2, 2, 64, 5)
    assert not ops.agent_env_episode_moving_scan_pe_supported(3, 4, 128, 9)
    assert not ops.agent_env_episode_moving_scan_pe_supported(6, 8, 64, 17)


# ---------------------------------------------------------------------------------------------------------------
# 9. the entry point's refusals: each returns its code and names the argument, before any launch
def test_entry_point_refusals(monkeypatch):
    from macjd_amd import _native
    J, R, L, E = 3, 4, 4, 16
    mb, _ = _batch(J, R, L, E, "host")
    r, _, _ = _runner(mb)
    captured = {}
    lib = _native.load()
    real = lib.macjd_agent_env_episode_moving_scan_pe
    IO = _native.AgentEnvEpisodeMovingScanPeIO

    class Spy:   # keeps a copy of the argument block of a valid call
        def __getattr__(self, name):
            return getattr(lib, name)

        def macjd_agent_env_episode_moving_scan_pe(self, h, ref, stream):
            captured["io"] = IO.from_buffer_copy(ref._obj)
            captured["h"], captured["stream"] = h, stream
            return real(h, ref, stream)
    real_load = _native.load
    monkeypatch.setattr(_native, "load", lambda: Spy())
    r.rollout_closed_loop_moving_pe(n_steps=2)
    torch.cuda.synchronize()
    monkeypatch.setattr(_native, "load", real_load)
    good, h, stream = captured["io"], captured["h"], captured["stream"]
    assert good.motion_pe.tile == TILE_RUN and good.motion_pe.snr_no is None and good.motion_scan_pe.n_levels == L
    err = lambda: lib.macjd_last_error().decode()
    # every output of the launch at a sentinel
    env = r.env
    for k, v in r.stage.items():
        v.fill_(True if v.dtype == torch.bool else 77)
    r._rdpj_sum.fill_(77.0)
    r.mac.hidden_states.fill_(77.0)
    outs = lambda: [v for v in r.stage.values()] + [r._rdpj_sum, r.mac.hidden_states, env._theta_a, env._track, env._step,
                                                    env._state_dyn, env._snr_no_step]
    torch.cuda.synchronize()
    before = [t.clone() for t in outs()]

    def call(handle=h, **changes):
        io_ = IO.from_buffer_copy(good)
        for path, v in changes.items():
            obj, parts = io_, path.split("__")
            for p in parts[:-1]:
                obj = getattr(obj, p)
            setattr(obj, parts[-1], v)
        return lib.macjd_agent_env_episode_moving_scan_pe(handle, ctypes.byref(io_), stream)

    EINVAL, EUNSUPPORTED = -1, -4
    assert call(motion_pe__frames=None) == EINVAL and "frames / frame_flags" in err()
    assert call(motion_pe__frame_flags=None) == EINVAL and "frames / frame_flags" in err()
    assert call(motion_pe__positions=None) == EINVAL and "positions" in err()
    assert call(motion_pe__position_columns=None) == EINVAL and "position_columns" in err()
    assert call(motion_pe__state=None) == EINVAL and "state is NULL" in err()
    assert call(motion_scan_pe__scan_frames=None) == EINVAL and "scan_frames" in err()
    assert call(motion_pe__n_frames=0) == EINVAL and "n_frames < 1" in err()
    assert call(motion_pe__n_frames=F - 1) == EINVAL and "episode_limit" in err()
    assert call(motion_pe__n_pos=2 * R + 2 * J - 1) == EINVAL and "n_pos" in err()
    assert call(motion_pe__tile=0) == EINVAL and "tile must be >= 1" in err()
    assert call(motion_pe__tile=-16) == EINVAL and "tile must be >= 1" in err()
    assert call(motion_pe__snr_no=env._snr_no_step.data_ptr()) == EINVAL and "motion_pe.snr_no must be NULL" in err()
    other = torch.zeros_like(env._state_dyn)
    assert call(motion_pe__state=other.data_ptr()) == EINVAL and "same rows" in err()
    assert call(motion_pe__st_se=good.motion_pe.st_se + 1) == EINVAL and "same rows" in err()
    assert call(motion_scan_pe__n_levels=0) == EINVAL and "go together" in err()           # pattern_frames without levels
    assert call(motion_scan_pe__n_levels=7) == EINVAL and "n_levels outside" in err()
    assert call(motion_scan_pe__n_levels=-1) == EINVAL and "n_levels outside" in err()
    assert call(motion_scan_pe__pattern_frames=None) == EINVAL and "go together" in err()  # levels without pattern_frames
    assert call(base__pe_tables=good.motion_pe.frames) == EINVAL and "pe_tables must be NULL" in err()
    assert call(base__J=6, base__R=8, base__A=17) == EUNSUPPORTED and "unsupported" in err()
    assert call(base__H=128) == EUNSUPPORTED and "unsupported" in err()
    assert call(base__actor_hidden=64) == EUNSUPPORTED and "unsupported" in err()
    assert lib.macjd_agent_env_episode_moving_scan_pe(h, None, stream) == EINVAL and "NULL" in err()
    assert lib.macjd_agent_env_episode_moving_scan_pe(None, ctypes.byref(IO.from_buffer_copy(good)), stream) == EINVAL
    with torch.cuda.device(DEV):
        no_scan = _native.ScenarioHandle(Scenario.from_dict(motion_cases.moving_ring_dict(J, R), config=spm.config()))
        pat1 = _native.ScenarioHandle(Scenario.from_dict(motion_frame_dict(_base(J, R, 1), 0), config=spm.config()))
    assert call(handle=no_scan.ptr) == EINVAL and "no scanning tables" in err()
    assert call(handle=pat1.ptr) == EINVAL and "n_levels differs" in err()                 # the handle's L = 1, the call's 4
    # no envs: nothing to do, nothing touched (not even with a table pointer missing behind the checks' reach)
    assert call(base__n_envs=0) == 0
    # none of the calls above launched
    torch.cuda.synchronize()
    for a, b in zip(before, outs()):
        assert torch.equal(a, b)
    # ... and the block itself is still good
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(before[0], r.stage["state"])


# ---------------------------------------------------------------------------------------------------------------
# 10. the driver, in a fresh process with the switch on
def test_driver_trains_with_the_closed_loop_moving_pe_rollout_in_a_fresh_process(tmp_path):
    """``python -m macjd_amd.main --env-config scenario_3j4r_moving_scan --randomize-moving-scan-scenarios
    --randomize-velocity-jitter 1.0`` with MACJD_CLOSED_LOOP_MOVING_PE_ROLLOUT=1 in the child's environment and no further flag."""
    import shutil
    import yaml
    cfg_dir = tmp_path / "config"
    cfg_dir.mkdir()
    with open(os.path.join(PKG, "config", "default.yaml")) as f:
        cfg = yaml.safe_load(f)
    E, Fd = 16, 8
    cfg.update(batch_envs=E, buffer_size=2 * E, total_env_steps=2 * E * Fd, episode_limit=Fd, start_training_steps=0, batch_size=8,
               updates_per_rollout=2, updates_per_graph=2, save_interval=10 ** 9, test_interval=0, gemm_tuning=False,
               log_interval_seconds=0, save_model_dir=str(tmp_path / "models"), results_path=str(tmp_path / "logs"), lr=1e-4)
    with open(cfg_dir / "default.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    shutil.copy(os.path.join(PKG, "config", "scenario_3j4r_moving_scan.yaml"), cfg_dir / "scenario_3j4r_moving_scan.yaml")
    env = dict(os.environ, MACJD_CLOSED_LOOP_MOVING_PE_ROLLOUT="1")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-m", "macjd_amd.main", "--config-dir", str(cfg_dir), "--env-config",
                          "scenario_3j4r_moving_scan", "--randomize-moving-scan-scenarios", "--randomize-velocity-jitter", "1.0"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Training finished." in out.stdout
