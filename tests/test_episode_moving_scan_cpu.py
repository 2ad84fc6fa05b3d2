"""Closed-loop episode launch for moving scenarios under scanning radars, host side: exported symbols and supported sizes,
the ctypes mirror of ``macjd_agent_env_episode_moving_scan_io`` against the header's layout, the runner's new switch and
``closed_loop_moving_available`` on stub objects."""
import ctypes
import os
import subprocess
import tempfile
from types import SimpleNamespace

import pytest

import __graft_entry__ as entry
from _harness import REPO

from macjd_amd import _native, options


@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_library_exports_the_moving_closed_loop_symbols(built):
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    for sym in ("macjd_agent_env_episode_moving_scan_supported", "macjd_agent_env_episode_moving_scan"):
        assert sym in _native.EXPORTS and f"{sym}(" in hdr
        assert hasattr(built, sym), sym
    f = built.macjd_agent_env_episode_moving_scan_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    assert f(3, 4, 64, 9) == 1 and f(2, 2, 64, 5) == 1
    for J, R, H, A in ((6, 8, 64, 17), (3, 4, 128, 9), (3, 4, 64, 5), (2, 2, 64, 9), (2, 2, 128, 5), (12, 16, 64, 33), (3, 3, 64, 7)):
        assert f(J, R, H, A) == 0, (J, R, H, A)
    abi = open(os.path.join(REPO, "include", "macjd.h")).read()
    assert "#define MACJD_ABI_VERSION 12" in abi and _native.ABI_VERSION == 12
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == 12


def test_episode_moving_scan_io_struct_layout_matches_header():
    IO = _native.AgentEnvEpisodeMovingScanIO
    fields = ["base", "motion", "motion_scan"]
    nested = [("motion.frames", IO.motion.offset + _native.MotionIO.frames.offset),
              ("motion.frame_flags", IO.motion.offset + _native.MotionIO.frame_flags.offset),
              ("motion.positions", IO.motion.offset + _native.MotionIO.positions.offset),
              ("motion.position_columns", IO.motion.offset + _native.MotionIO.position_columns.offset),
              ("motion.n_frames", IO.motion.offset + _native.MotionIO.n_frames.offset),
              ("motion.n_pos", IO.motion.offset + _native.MotionIO.n_pos.offset),
              ("motion.state", IO.motion.offset + _native.MotionIO.state.offset),
              ("motion.snr_no", IO.motion.offset + _native.MotionIO.snr_no.offset),
              ("motion_scan.scan_frames", IO.motion_scan.offset + _native.MotionScanIO.scan_frames.offset),
              ("motion_scan.pattern_frames", IO.motion_scan.offset + _native.MotionScanIO.pattern_frames.offset),
              ("motion_scan.n_levels", IO.motion_scan.offset + _native.MotionScanIO.n_levels.offset),
              ("base.pe_tables", IO.base.offset + _native.AgentEnvEpisodeScanIO.pe_tables.offset),
              ("base.scan", IO.base.offset + _native.AgentEnvEpisodeScanIO.scan.offset),
              ("base.rdpj_sum", IO.base.offset + _native.AgentEnvEpisodeScanIO.rdpj_sum.offset)]
    t = "macjd_agent_env_episode_moving_scan_io"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           f'int main(){{printf("%zu %zu %zu %zu", sizeof({t}), sizeof(macjd_agent_env_episode_scan_io), '
           'sizeof(macjd_motion_io), sizeof(macjd_motion_scan_io));\n'
           + "".join(f'printf(" %zu", offsetof({t}, {f}));\n' for f in fields + [n for n, _ in nested])
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO) and out[1] == ctypes.sizeof(_native.AgentEnvEpisodeScanIO)
    assert out[2] == ctypes.sizeof(_native.MotionIO) and out[3] == ctypes.sizeof(_native.MotionScanIO)
    offs = out[4:]
    for name, off in zip(fields, offs):
        assert getattr(IO, name).offset == off, name
    for (name, want), off in zip(nested, offs[len(fields):]):
        assert want == off, name
    assert IO.base.offset == 0
    assert [n for n, *_ in IO._fields_] == fields
    # the two existing closed-loop blocks are what they were
    assert [n for n, *_ in _native.AgentEnvEpisodeScanPeIO._fields_] == ["base", "pe_flags", "pe_stride", "pe_tile", "reserved",
                                                                        "scan_pe", "pattern"]


def test_new_switch_default_set_reset_and_documented(monkeypatch):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    name = "MACJD_CLOSED_LOOP_MOVING_ROLLOUT"
    monkeypatch.delenv(name, raising=False)
    options.reload()
    try:
        assert options.get("CLOSED_LOOP_MOVING_ROLLOUT") == "0"
        assert BatchedEpisodeRunner.closed_loop_moving_rollout is False
        r = BatchedEpisodeRunner.__new__(BatchedEpisodeRunner)     # (no device needed to read a switch)
        assert r.closed_loop_moving_rollout is False
        monkeypatch.setenv(name, "1")
        options.reload()
        assert options.get("CLOSED_LOOP_MOVING_ROLLOUT") == "1" and r.closed_loop_moving_rollout is True
        # the old switches do not follow it, and it does not follow them
        assert r.closed_loop_rollout is False and r.moving_episode_rollout is False
        monkeypatch.delenv(name)
        monkeypatch.setenv("MACJD_CLOSED_LOOP_ROLLOUT", "1")
        monkeypatch.setenv("MACJD_MOVING_EPISODE_ROLLOUT", "1")
        options.reload()
        assert r.closed_loop_moving_rollout is False and r.closed_loop_rollout is True and r.moving_episode_rollout is True
        r.closed_loop_moving_rollout = True                        # an instance can set it
        assert r.closed_loop_moving_rollout is True and BatchedEpisodeRunner.closed_loop_moving_rollout is False
    finally:
        for n in (name, "MACJD_CLOSED_LOOP_ROLLOUT", "MACJD_MOVING_EPISODE_ROLLOUT"):
            monkeypatch.delenv(n, raising=False)
        options.reload()
    assert options.get("CLOSED_LOOP_MOVING_ROLLOUT") == "0"
    assert name in options.__doc__
    assert callable(r.closed_loop_moving_available) and callable(r.rollout_closed_loop_moving)


class _Trap:
    @property
    def agent(self):
        raise LookupError("the agent was asked for")


def _stub_runner(moving, scanning, batch=None, kernel_flags=0, device="cuda"):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner as Runner
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    env = object.__new__(Env)
    env.scenario = SimpleNamespace(moving=moving, scanning=scanning)
    env.scenario_batch, env.kernel_flags = batch, kernel_flags
    stub = SimpleNamespace(env=env, device=SimpleNamespace(type=device), mac=SimpleNamespace(agent=None))
    stub._closed_loop_conditions = lambda per_env, moving=False: Runner._closed_loop_conditions(stub, per_env, moving)
    return Runner, stub


def test_closed_loop_moving_available_is_false_off_its_ground():
    """Each stub fails on the scenario's kind alone: the agent (None here) is looked at only after those conditions, so a
    condition that let one of these through would reach it and answer False for another reason — hence the last case, which
    shows that a moving scanning env gets as far as the agent."""
    for moving, scanning, batch in ((False, True, None), (True, False, None), (False, False, None), (True, True, object())):
        Runner, stub = _stub_runner(moving, scanning, batch)
        stub.mac = _Trap()                                         # touching the agent would raise
        assert Runner.closed_loop_moving_available(stub) is False, (moving, scanning, batch)
    Runner, stub = _stub_runner(True, True, kernel_flags=1)
    stub.mac = _Trap()
    assert Runner.closed_loop_moving_available(stub) is False
    Runner, stub = _stub_runner(True, True, device="cpu")
    stub.mac = _Trap()
    assert Runner.closed_loop_moving_available(stub) is False
    Runner, stub = _stub_runner(True, True)
    stub.mac = _Trap()
    with pytest.raises(LookupError):                            # past the scenario conditions: it asks for the agent
        Runner.closed_loop_moving_available(stub)
    # the old names keep their answers on a moving scanning env
    Runner, stub = _stub_runner(True, True)
    assert Runner.closed_loop_available(stub) is False and Runner.closed_loop_pe_available(stub) is False


def test_environment_hands_over_only_when_it_moves_and_scans():
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    for scan_io, motion_io, motion_scan_io in ((object(), None, None), (None, object(), None), (None, None, None)):
        env = object.__new__(Env)
        env._scan_io, env._motion_io, env._motion_scan_io, env._pe_tables = scan_io, motion_io, motion_scan_io, None
        with pytest.raises(RuntimeError, match="episode_moving_scan_args: needs a scenario that both moves and scans"):
            env.episode_moving_scan_args()
    env = object.__new__(Env)
    env._scan_io, env._motion_io, env._motion_scan_io, env._pe_tables = object(), object(), object(), None
    with pytest.raises(RuntimeError, match="episode_scan_args: not available with a moving scenario"):
        env.episode_scan_args()
