"""Closed-loop episode launch for scanning radars, host side: exported symbols, the ctypes mirror against the header's
layout, and the runner's switch."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import __graft_entry__ as entry
from _harness import REPO

from macjd_amd import _native, options


@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_library_exports_the_closed_loop_symbols(built):
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    for sym in ("macjd_agent_env_episode_scan_supported", "macjd_agent_env_episode_scan"):
        assert sym in _native.EXPORTS and f"{sym}(" in hdr
        assert hasattr(built, sym), sym
    f = built.macjd_agent_env_episode_scan_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    assert f(3, 4, 64, 9) == 1 and f(2, 2, 64, 5) == 1
    assert f(6, 8, 64, 17) == 0 and f(3, 4, 128, 9) == 0 and f(3, 4, 64, 5) == 0 and f(12, 16, 64, 33) == 0


def test_episode_scan_io_struct_layout_matches_header():
    IO = _native.AgentEnvEpisodeScanIO
    fields = ["n_envs", "T", "greedy_only", "h0", "W1", "w1_ld", "avail", "av_se", "eps", "seed", "counter_base", "env_seed",
              "episode", "track", "step", "scan", "pe_tables", "hidden", "st_state", "terminated", "rdpj_sum"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           'int main(){printf("%zu %zu", sizeof(macjd_agent_env_episode_scan_io), sizeof(macjd_scan_io));\n'
           + "".join(f'printf(" %zu", offsetof(macjd_agent_env_episode_scan_io, {f}));\n' for f in fields)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO) and out[1] == ctypes.sizeof(_native.ScanIO)
    for name, off in zip(fields, out[2:]):
        assert getattr(IO, name).offset == off, name
    assert [n for n, *_ in IO._fields_][-1] == "rdpj_sum"


def test_switch_is_off_by_default_and_follows_the_option(monkeypatch):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    monkeypatch.delenv("MACJD_CLOSED_LOOP_ROLLOUT", raising=False)
    options.reload()
    try:
        assert BatchedEpisodeRunner.closed_loop_rollout is False
        r = BatchedEpisodeRunner.__new__(BatchedEpisodeRunner)     # (no device needed to read a switch)
        assert r.closed_loop_rollout is False
        monkeypatch.setenv("MACJD_CLOSED_LOOP_ROLLOUT", "1")
        options.reload()
        assert BatchedEpisodeRunner.closed_loop_rollout is True and r.closed_loop_rollout is True
        r.closed_loop_rollout = False                               # an instance can pin it
        assert r.closed_loop_rollout is False and BatchedEpisodeRunner.closed_loop_rollout is True
        monkeypatch.setenv("MACJD_CLOSED_LOOP_ROLLOUT", "0")
        options.reload()
        assert BatchedEpisodeRunner.closed_loop_rollout is False
    finally:
        monkeypatch.delenv("MACJD_CLOSED_LOOP_ROLLOUT", raising=False)
        options.reload()
