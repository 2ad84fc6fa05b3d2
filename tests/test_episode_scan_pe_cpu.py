"""Closed-loop episode launch on per-env scanning scenario batches, host side: exported symbols and ABI version, the ctypes
mirror of ``macjd_agent_env_episode_scan_pe_io`` against the header's layout, and the runner's switch."""
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


def test_library_exports_the_per_env_closed_loop_symbols(built):
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    for sym in ("macjd_agent_env_episode_scan_pe_supported", "macjd_agent_env_episode_scan_pe"):
        assert sym in _native.EXPORTS and f"{sym}(" in hdr
        assert hasattr(built, sym), sym
    f = built.macjd_agent_env_episode_scan_pe_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    assert f(3, 4, 64, 9) == 1 and f(2, 2, 64, 5) == 1
    assert f(6, 8, 64, 17) == 0 and f(3, 4, 128, 9) == 0 and f(3, 4, 64, 5) == 0 and f(12, 16, 64, 33) == 0
    abi = open(os.path.join(REPO, "include", "macjd.h")).read()
    assert f"#define MACJD_ABI_VERSION {_native.ABI_VERSION}" in abi and _native.ABI_VERSION >= 11
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == _native.ABI_VERSION


def test_episode_scan_pe_io_struct_layout_matches_header():
    IO = _native.AgentEnvEpisodeScanPeIO
    fields = ["base", "pe_flags", "pe_stride", "pe_tile", "reserved", "scan_pe", "pattern"]
    nested = [("scan_pe.tables", IO.scan_pe.offset + _native.ScanPeIO.tables.offset),
              ("scan_pe.stride", IO.scan_pe.offset + _native.ScanPeIO.stride.offset),
              ("pattern.tables", IO.pattern.offset + _native.ScanPePatternIO.tables.offset),
              ("pattern.stride", IO.pattern.offset + _native.ScanPePatternIO.stride.offset),
              ("pattern.n_levels", IO.pattern.offset + _native.ScanPePatternIO.n_levels.offset),
              ("base.pe_tables", IO.base.offset + _native.AgentEnvEpisodeScanIO.pe_tables.offset),
              ("base.rdpj_sum", IO.base.offset + _native.AgentEnvEpisodeScanIO.rdpj_sum.offset)]
    t = "macjd_agent_env_episode_scan_pe_io"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           f'int main(){{printf("%zu %zu %zu %zu", sizeof({t}), sizeof(macjd_agent_env_episode_scan_io), '
           'sizeof(macjd_scan_pe_io), sizeof(macjd_scan_pe_pattern_io));\n'
           + "".join(f'printf(" %zu", offsetof({t}, {f}));\n' for f in fields + [n for n, _ in nested])
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO) and out[1] == ctypes.sizeof(_native.AgentEnvEpisodeScanIO)
    assert out[2] == ctypes.sizeof(_native.ScanPeIO) and out[3] == ctypes.sizeof(_native.ScanPePatternIO)
    offs = out[4:]
    for name, off in zip(fields, offs):
        assert getattr(IO, name).offset == off, name
    for (name, want), off in zip(nested, offs[len(fields):]):
        assert want == off, name
    assert IO.base.offset == 0
    assert [n for n, *_ in IO._fields_] == fields


def test_switch_is_still_off_by_default(monkeypatch):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    monkeypatch.delenv("MACJD_CLOSED_LOOP_ROLLOUT", raising=False)
    options.reload()
    assert BatchedEpisodeRunner.closed_loop_rollout is False
    r = BatchedEpisodeRunner.__new__(BatchedEpisodeRunner)     # (no device needed to read a switch)
    assert r.closed_loop_rollout is False
    assert callable(r.closed_loop_pe_available) and callable(r.rollout_closed_loop_pe)
