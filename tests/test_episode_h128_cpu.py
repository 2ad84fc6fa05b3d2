"""Whole-episode agent launch and one-launch Double-DQN at GRU hidden size 128, host side: what the library says it
supports (the reference's default `rnn_hidden_dim: 128` at 2j/2r and 3j/4r), and the package switch that selects the
two-launch Double-DQN form."""
import ctypes

import pytest

import __graft_entry__ as entry

from macjd_amd import _native, options


@pytest.fixture(scope="module")
def built():
    entry.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    lib.macjd_agent_episode_supported.restype = ctypes.c_int
    lib.macjd_agent_episode_supported.argtypes = [ctypes.c_int32] * 3        # (J, H, A)
    lib.macjd_qhead_double_q_supported.restype = ctypes.c_int
    lib.macjd_qhead_double_q_supported.argtypes = [ctypes.c_int32] * 2       # (H, A)
    lib.macjd_agent_env_episode_scan_supported.restype = ctypes.c_int
    lib.macjd_agent_env_episode_scan_supported.argtypes = [ctypes.c_int32] * 4   # (J, R, H, A)
    lib.macjd_qhead_taken_supported.restype = ctypes.c_int
    lib.macjd_qhead_taken_supported.argtypes = [ctypes.c_int32] * 2
    return lib


def test_episode_launch_supported_at_h128(built):
    ep = built.macjd_agent_episode_supported
    assert ep(2, 128, 5) == 1
    assert ep(3, 128, 9) == 1
    # H = 64: unchanged
    assert ep(3, 64, 9) == 1 and ep(2, 64, 5) == 1 and ep(6, 64, 17) == 1 and ep(12, 64, 33) == 1 and ep(5, 64, 9) == 1
    assert ep(3, 64, 7) == 0 and ep(0, 64, 9) == 0
    # the header's supported set at H = 128 is exact: per-agent tiles only, A in {5, 9}
    assert ep(6, 128, 17) == 0 and ep(12, 128, 33) == 0 and ep(4, 128, 9) == 0 and ep(3, 128, 17) == 0 and ep(3, 128, 33) == 0
    assert ep(2, 96, 5) == 0 and ep(3, 96, 9) == 0


def test_double_q_launch_supported_at_h128(built):
    dq = built.macjd_qhead_double_q_supported
    assert dq(128, 5) == 1
    assert dq(128, 9) == 1
    assert dq(128, 17) == 1 and dq(128, 33) == 0 and dq(128, 7) == 0
    assert dq(64, 5) == 1 and dq(64, 9) == 1 and dq(64, 17) == 1 and dq(64, 33) == 1 and dq(64, 7) == 0
    assert dq(96, 5) == 0 and dq(96, 9) == 0


def test_h128_refusals_that_stay(built):
    assert built.macjd_agent_env_episode_scan_supported(3, 4, 128, 9) == 0
    assert built.macjd_agent_env_episode_scan_supported(3, 4, 64, 9) == 1
    assert built.macjd_qhead_taken_supported(128, 5) == 0 and built.macjd_qhead_taken_supported(64, 5) == 1


def test_double_q_switch_defaults_on_and_follows_the_environment(monkeypatch):
    monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q", raising=False)
    monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q_H128", raising=False)
    options.reload()
    try:
        assert options.get("QHEAD_DOUBLE_Q") == "1" and options.on("QHEAD_DOUBLE_Q")
        assert options.get("QHEAD_DOUBLE_Q_H128") == "0"      # H = 128: the one-launch form measured slower in the update
        monkeypatch.setenv("MACJD_QHEAD_DOUBLE_Q", "0")
        options.reload()
        assert not options.on("QHEAD_DOUBLE_Q")
    finally:
        monkeypatch.delenv("MACJD_QHEAD_DOUBLE_Q", raising=False)
        options.reload()
    assert "MACJD_QHEAD_DOUBLE_Q " in options.__doc__ and "MACJD_QHEAD_DOUBLE_Q_H128" in options.__doc__
