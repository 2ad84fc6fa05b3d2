"""Closed-loop episode launch on per-env moving scanning scenario batches, host side: the switch, the availability predicate
off a HIP device, the ctypes mirror against its parts and the header's layout, the exported symbols and supported sizes, and
the index model of the tiled per-env frame layout (tests/tiled_frames.py) that the GPU file builds its expected values with."""
import ctypes
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import __graft_entry__ as entry  # noqa: E402
from _harness import REPO  # noqa: E402
from tiled_frames import gather_frames, tiled_index  # noqa: E402

from macjd_amd import _native, options  # noqa: E402

SYMS = ("macjd_agent_env_episode_moving_scan_pe_supported", "macjd_agent_env_episode_moving_scan_pe")
SWITCH = "MACJD_CLOSED_LOOP_MOVING_PE_ROLLOUT"
OLD_SWITCHES = ("closed_loop_rollout", "moving_episode_rollout", "closed_loop_moving_rollout", "moving_pe_episode_rollout")


@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_switch_is_off_by_default_documented_and_independent(monkeypatch):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    monkeypatch.delenv(SWITCH, raising=False)
    options.reload()
    try:
        assert options._DEFAULTS["CLOSED_LOOP_MOVING_PE_ROLLOUT"] == "0" and options.get("CLOSED_LOOP_MOVING_PE_ROLLOUT") == "0"
        assert BatchedEpisodeRunner.closed_loop_moving_pe_rollout is False
        r = BatchedEpisodeRunner.__new__(BatchedEpisodeRunner)     # (no device needed to read a switch)
        assert r.closed_loop_moving_pe_rollout is False
        monkeypatch.setenv(SWITCH, "1")
        options.reload()
        assert options.get("CLOSED_LOOP_MOVING_PE_ROLLOUT") == "1"
        assert BatchedEpisodeRunner.closed_loop_moving_pe_rollout is True and r.closed_loop_moving_pe_rollout is True
        assert not any(getattr(r, n) for n in OLD_SWITCHES)
        monkeypatch.delenv(SWITCH)
        monkeypatch.setenv("MACJD_CLOSED_LOOP_MOVING_ROLLOUT", "1")     # the shared-frame switch keeps its meaning
        options.reload()
        assert r.closed_loop_moving_pe_rollout is False and r.closed_loop_moving_rollout is True
        r.closed_loop_moving_pe_rollout = True                          # an instance can set it
        assert r.closed_loop_moving_pe_rollout is True and BatchedEpisodeRunner.closed_loop_moving_pe_rollout is False
    finally:
        for n in (SWITCH, "MACJD_CLOSED_LOOP_MOVING_ROLLOUT"):
            monkeypatch.delenv(n, raising=False)
        options.reload()
    assert SWITCH in options.__doc__
    assert callable(r.closed_loop_moving_pe_available) and callable(r.rollout_closed_loop_moving_pe)


class _Trap:
    @property
    def agent(self):
        raise LookupError("the agent was asked for")


def _stub(moving_scan_batch, kernel_flags=0, device="cuda"):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner as Runner
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    env = object.__new__(Env)
    env.scenario = SimpleNamespace(moving=True, scanning=True)
    env.moving_scan_batch, env.moving_batch, env.scenario_batch, env.kernel_flags = moving_scan_batch, None, None, kernel_flags
    return Runner, SimpleNamespace(env=env, device=SimpleNamespace(type=device), mac=_Trap())


def test_closed_loop_moving_pe_available_is_false_off_its_ground():
    """Each stub fails on the device or the env's kind alone — touching the agent would raise — and the last one shows that a
    per-env moving scanning batch on a HIP device gets as far as the agent."""
    for kw in (dict(moving_scan_batch=object(), device="cpu"),         # not a HIP device
               dict(moving_scan_batch=None),                            # a shared-frame moving scanning env
               dict(moving_scan_batch=object(), kernel_flags=1)):
        Runner, stub = _stub(**kw)
        assert Runner.closed_loop_moving_pe_available(stub) is False, kw
    Runner, stub = _stub(moving_scan_batch=object())
    with pytest.raises(LookupError):
        Runner.closed_loop_moving_pe_available(stub)
    stub.closed_loop_moving_pe_available = lambda: False
    with pytest.raises(RuntimeError, match="rollout_closed_loop_moving_pe: not available"):
        Runner.rollout_closed_loop_moving_pe(stub)


def test_environment_hands_over_only_on_a_per_env_moving_scanning_batch():
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    env = object.__new__(Env)        # (the class defaults: no per-env moving scanning batch)
    env._motion_scan_pe_io = None
    with pytest.raises(RuntimeError, match="episode_moving_scan_pe_args: needs a per-env moving scanning scenario batch"):
        env.episode_moving_scan_pe_args()


def test_struct_is_base_then_the_two_per_env_motion_blocks():
    IO = _native.AgentEnvEpisodeMovingScanPeIO
    assert [(n, tp) for n, tp in IO._fields_] == [("base", _native.AgentEnvEpisodeScanIO), ("motion_pe", _native.MotionPeIO),
                                                  ("motion_scan_pe", _native.MotionScanPeIO)]
    sizes = [ctypes.sizeof(t) for t in (_native.AgentEnvEpisodeScanIO, _native.MotionPeIO, _native.MotionScanPeIO)]
    assert ctypes.sizeof(IO) == sum(sizes)
    assert [IO.base.offset, IO.motion_pe.offset, IO.motion_scan_pe.offset] == [0, sizes[0], sizes[0] + sizes[1]]
    # ... and the header's own layout
    t = "macjd_agent_env_episode_moving_scan_pe_io"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           f'int main(){{printf("%zu %zu %zu %zu\\n", sizeof({t}), offsetof({t}, base), offsetof({t}, motion_pe), '
           f'offsetof({t}, motion_scan_pe));return 0;}}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(IO), 0, IO.motion_pe.offset, IO.motion_scan_pe.offset]
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    assert "int macjd_agent_env_episode_moving_scan_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A);" in hdr


def test_library_exports_the_symbols_and_answers_the_supported_sizes(built):
    for sym in SYMS:
        assert sym in _native.EXPORTS and hasattr(built, sym), sym
    f = built.macjd_agent_env_episode_moving_scan_pe_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    assert f(3, 4, 64, 9) == 1 and f(2, 2, 64, 5) == 1
    for J, R, H, A in ((6, 8, 64, 17), (3, 4, 128, 9), (3, 4, 64, 5), (2, 2, 64, 9), (2, 2, 128, 5), (12, 16, 64, 33), (3, 3, 64, 7),
                       (3, 2, 64, 9), (2, 4, 64, 5)):
        assert f(J, R, H, A) == 0, (J, R, H, A)


# ------------------------------------------------------------------------------------------------- the index model
def _untile(t, E):
    """[n_tiles, F, rows, tile] -> [E, F, rows] (numpy): test_moving_scan_pe_gpu._untile_t's transposition."""
    return np.ascontiguousarray(np.transpose(t, (0, 3, 1, 2)).reshape(t.shape[0] * t.shape[3], t.shape[1], t.shape[2])[:E])


@pytest.mark.parametrize("E", [17, 40])
@pytest.mark.parametrize("tile", [1, 5, 8, 16, 256])
def test_tiled_index_against_transposing_gathers(tile, E):
    from macjd_amd.scenario import tile_envs
    F, rows = 5, 7
    rng = np.random.default_rng(tile * 100 + E)
    per_env = rng.random((E, F, rows))                      # [E, F, rows]: every element distinct
    table = tile_envs(per_env, tile)                        # [n_tiles, F, rows, tile], the last tile zero-padded
    n_tiles = (E + tile - 1) // tile
    assert table.shape == (n_tiles, F, rows, tile)
    np.testing.assert_array_equal(_untile(table, E), per_env)
    flat = table.reshape(-1)
    e, f, r = np.meshgrid(np.arange(E), np.arange(F), np.arange(rows), indexing="ij")
    idx = tiled_index(e, f, r, rows, F, tile)
    assert idx.min() >= 0 and idx.max() < flat.size and np.unique(idx).size == idx.size
    np.testing.assert_array_equal(flat[idx], per_env)
    # no address of a real env falls into a padding lane of the last tile
    pad = np.ones(table.shape, dtype=bool)
    pad.reshape(-1)[idx.reshape(-1)] = False
    assert int(pad.sum()) == (n_tiles * tile - E) * F * rows
    if n_tiles * tile > E:
        assert pad[-1, :, :, E - (n_tiles - 1) * tile:].all() and not pad[:-1].any()
    # envs on frames of their own, as after individual resets
    fe = rng.integers(0, F, size=E)
    np.testing.assert_array_equal(gather_frames(table, np.arange(E), fe), per_env[np.arange(E), fe])
    # the positions table has F + 1 frames per tile
    pos = tile_envs(rng.random((E, F + 1, rows)).astype(np.float32), tile)
    k = np.minimum(fe + 1, F)
    np.testing.assert_array_equal(gather_frames(pos, np.arange(E), k), _untile(pos, E)[np.arange(E), k])
