"""Launch geometry of the env lane kernel above the batch sizes the other tests reach: the first 256-lane launch with a
one-env tail block (E = 2^16 + 1) and the general variants' grid-stride cap (first reached above 256 * 8 * 256 envs).

One step of the whole batch in one launch against the same batch stepped as consecutive launches of at most 65 535 envs
(64-lane workgroups, no cap), each with env_offset at its first env and the matching slices of actions, uniforms and
state.  The draws are keyed by env_offset + e and envs are independent: every output is equal bit for bit."""
import ctypes

import pytest
import torch

from test_scan_gpu import DEV, _base, _diag, _env, _sc, _scan_dict
from test_scan_pattern_cpu import GAINS4, pattern_dict

pytestmark = pytest.mark.gpu
SLICE = 65535
SCENARIOS = {"static": lambda: _base("3j4r"), "scan": lambda: _scan_dict(_base("3j4r"), 0.25, -30.0),
             "pattern": lambda: pattern_dict("3j4r", GAINS4)}


def _slice_of(block, ptrs, a):
    """Copy of an argument block whose per-env arrays start at env a: (pointer, elements per env or its stride, bytes)."""
    out = type(block)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(block), ctypes.sizeof(block))
    for name, se, elem in ptrs:
        p = getattr(block, name)
        if p:
            setattr(out, name, p + a * (getattr(block, se) if isinstance(se, str) else se) * elem)
    return out


def _step_ptrs(R, J):
    return (("T", "T_se", 4), ("P32", "P_se", 4), ("P64", "P_se", 8), ("u", "u_se", 8), ("episode", 1, 4),
            ("track", "k_se", 1), ("step", 1, 4), ("reward", 1, 4), ("r_dpj", 3, 4), ("terminated", 1, 1),
            ("pd", "pd_se", 4), ("snr_with", "sw_se", 4), ("out64", 4, 8), ("pd64", R, 8), ("snr64", R, 8), ("prj64", J, 8))


SCAN_PTRS = (("theta_a", "a_se", 8), ("state", "st_se", 4), ("snr_no", "sn_se", 4))


def _step_in_slices(env, T, P, u, diag):
    R, J, E = env.num_radars, env.num_jammers, env.batch_envs
    io = env._fill_io(T, P, u, False, None, None, True, diag)
    stream = torch.cuda.current_stream(env.device).cuda_stream
    with torch.cuda.device(env.device):
        for a in range(0, E, SLICE):
            sub = _slice_of(io, _step_ptrs(R, J), a)
            sub.n_envs, sub.env_offset = min(SLICE, E - a), env.env_offset + a
            if env._scan_io is not None:
                scan = _slice_of(env._scan_io, SCAN_PTRS, a)
                rc = env._lib.macjd_env_step_scan(env._handle.ptr, ctypes.byref(sub), ctypes.byref(scan), stream)
            else:
                rc = env._lib.macjd_env_step(env._handle.ptr, ctypes.byref(sub), stream)
            assert rc == 0, env._lib.macjd_last_error()


@pytest.mark.parametrize("scenario,E,uniforms", [
    ("scan", 65537, "philox"), ("scan", 65537, "supplied"), ("pattern", 65537, "philox"), ("pattern", 65537, "supplied"),
    ("static", 524288 + 257, "supplied"), ("scan", 524288 + 257, "supplied")])
def test_one_launch_equals_consecutive_launches_of_slices(scenario, E, uniforms):
    sc = _sc(SCENARIOS[scenario]())
    R, J = sc.num_radars, sc.num_jammers
    gen = torch.Generator(device=DEV).manual_seed(E + len(scenario))
    rand = lambda *s: torch.rand(*s, generator=gen, device=DEV, dtype=torch.float64)
    # a mid-episode state: FSM bits, step counters and beam azimuths of every env differ
    track, step, theta = (rand(R, E) < 0.5).to(torch.uint8), (rand(E) * 50).to(torch.int32), rand(R, E) * 360.0
    whole, sliced = _env(sc, E), _env(sc, E)
    for env in (whole, sliced):
        env.kernel_flags = 2   # lane kernel for the slices of the static scenario as well
        env.reset()
        env._track.copy_(track)
        env._step.copy_(step)
        if sc.scanning:
            env._theta_a.copy_(theta)
            env._state_dyn[:, torch.as_tensor(sc.theta_a_columns, device=DEV)] = theta.t().to(torch.float32)
    T = (rand(E, J) * (2 * R + 4)).to(torch.int32) - 1       # -1 .. 2R + 2: invalid indices on both sides
    P = rand(E, J).to(torch.float32)
    u = dw = ds = None
    if uniforms == "supplied":   # the general variant
        P, u, dw, ds = P.to(torch.float64), rand(E, R + J), _diag(E, R, J), _diag(E, R, J)
    whole.step(T, P, u, diag=dw)
    _step_in_slices(sliced, T, P, u, ds)
    names = ["_reward", "_terminated", "_r_dpj", "_track", "_step", "_pd", "_snr"]
    names += ["_theta_a", "_state_dyn", "_snr_no_step"] if sc.scanning else []
    for k in names:
        assert torch.equal(getattr(whole, k), getattr(sliced, k)), k
    for k in (dw or {}):
        assert torch.equal(dw[k], ds[k]), k
    # the step did something in the tail block: its envs differ among themselves, counters advanced
    assert whole._reward[-257:].unique().numel() > 16 and whole._track[:, -257:].unique().numel() == 2
    assert torch.equal(whole._step, step + 1)
