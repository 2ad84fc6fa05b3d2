"""Whole-episode rollout of moving scenarios, host side: the header's declarations, the ctypes mirror against the header's
layout, the exported symbols and the supported sizes, the frame state rows and the runner's switch."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import __graft_entry__ as entry
import motion_cases as cases
from _harness import REPO

from macjd_amd import _native, options
from macjd_amd.scenario import Scenario, motion_frame_dict, ring_scenario_dict

SYMS = ("macjd_agent_episode_seq_supported", "macjd_agent_episode_seq")
# (J, A) per H of include/macjd_nets.h, macjd_agent_episode_seq_io; no instantiation was dropped (none needs scratch)
SUPPORTED = {(2, 64, 5), (3, 64, 9), (6, 64, 17), (2, 128, 5), (3, 128, 9)}


@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_header_declares_the_struct_and_both_functions():
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    assert "typedef struct macjd_agent_episode_seq_io {" in hdr and "} macjd_agent_episode_seq_io;" in hdr
    assert "int macjd_agent_episode_seq_supported(int32_t J, int32_t H, int32_t A);" in hdr
    assert "int macjd_agent_episode_seq(const macjd_agent_episode_seq_io* io, void* hip_stream);" in hdr


def test_seq_io_struct_layout_matches_header():
    IO, Base = _native.AgentEpisodeSeqIO, _native.AgentEpisodeIO
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(macjd_agent_episode_seq_io), sizeof(macjd_agent_episode_io),\n'
           'offsetof(macjd_agent_episode_seq_io, base), offsetof(macjd_agent_episode_seq_io, gi_lt),\n'
           'offsetof(macjd_agent_episode_seq_io, p_lt));return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO) and out[1] == ctypes.sizeof(Base)
    assert [IO.base.offset, IO.gi_lt.offset, IO.p_lt.offset] == out[2:]
    # base first, then two int64: the static launch's block did not move
    assert [(n, t) for n, t in IO._fields_] == [("base", Base), ("gi_lt", ctypes.c_int64), ("p_lt", ctypes.c_int64)]
    assert IO.base.offset == 0 and IO.gi_lt.offset == ctypes.sizeof(Base) and IO.p_lt.offset == ctypes.sizeof(Base) + 8
    assert ctypes.sizeof(IO) == ctypes.sizeof(Base) + 16


def test_library_exports_both_symbols_and_answers_the_supported_sizes(built):
    for sym in SYMS:
        assert sym in _native.EXPORTS and hasattr(built, sym), sym
    f = built.macjd_agent_episode_seq_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 3
    for H in (32, 64, 128, 256):
        for J in (1, 2, 3, 4, 6, 12):
            for A in (5, 9, 17, 33):
                assert f(J, H, A) == (1 if (J, H, A) in SUPPORTED else 0), (J, H, A)
    assert f(6, 128, 17) == 0 and f(12, 64, 33) == 0 and f(3, 32, 9) == 0
    # a subset of the static launch's sizes
    g = built.macjd_agent_episode_supported
    g.restype, g.argtypes = ctypes.c_int, [ctypes.c_int32] * 3
    assert all(g(J, H, A) == 1 for J, H, A in SUPPORTED)


def test_abi_version_is_unchanged(built):
    assert _native.ABI_VERSION == 12
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == 12


@pytest.mark.parametrize("which", ["fixture", "ring_2j2r", "ring_6j8r"])
def test_frame_state_rows_are_the_frames_state_vectors(which):
    cfg = cases.fixture()[0] if which == "fixture" else cases.moving_ring_dict(*((2, 2) if which == "ring_2j2r" else (6, 8)))
    sc, frames = cases.compiled(cfg)
    F = sc.episode_limit
    rows = sc.frame_state_rows()
    assert rows.dtype == np.float32 and rows.shape == (F + 1, sc.state_dim) and rows.flags["C_CONTIGUOUS"]
    for k in (0, 1, F):
        ref = Scenario.from_dict(motion_frame_dict(cfg, k), config=cases.config()).state_vector()
        assert rows[k].tobytes() == ref.tobytes(), k
        assert rows[k].tobytes() == frames[k].state_vector().tobytes(), k
    # only the position columns differ from the scenario's own state vector, and they are the frame table's
    cols = sc.position_columns
    rest = np.setdiff1d(np.arange(sc.state_dim), cols)
    assert (rows[:, rest] == sc.state_vector()[rest]).all()
    assert rows[:, cols].tobytes() == np.ascontiguousarray(sc.motion_tables["positions"]).tobytes()
    assert not np.array_equal(rows[0], rows[F])


def test_frame_state_rows_refuse_a_scenario_that_does_not_move():
    with pytest.raises(AttributeError, match="does not move"):
        Scenario.from_dict(ring_scenario_dict(3, 4)).frame_state_rows()


def test_switch_is_off_by_default_and_follows_the_option(monkeypatch):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    monkeypatch.delenv("MACJD_MOVING_EPISODE_ROLLOUT", raising=False)
    options.reload()
    try:
        assert options.get("MOVING_EPISODE_ROLLOUT") == "0"
        assert BatchedEpisodeRunner.moving_episode_rollout is False
        r = BatchedEpisodeRunner.__new__(BatchedEpisodeRunner)     # (no device needed to read a switch)
        assert r.moving_episode_rollout is False
        monkeypatch.setenv("MACJD_MOVING_EPISODE_ROLLOUT", "1")
        options.reload()
        assert BatchedEpisodeRunner.moving_episode_rollout is True and r.moving_episode_rollout is True
        r.moving_episode_rollout = False                            # an instance can pin it
        assert r.moving_episode_rollout is False and BatchedEpisodeRunner.moving_episode_rollout is True
        monkeypatch.setenv("MACJD_MOVING_EPISODE_ROLLOUT", "0")
        options.reload()
        assert BatchedEpisodeRunner.moving_episode_rollout is False
    finally:
        monkeypatch.delenv("MACJD_MOVING_EPISODE_ROLLOUT", raising=False)
        options.reload()
    assert "MACJD_MOVING_EPISODE_ROLLOUT" in options.__doc__
