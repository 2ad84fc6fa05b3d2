"""Launch plan of the env-step kernels (csrc/macjd_env_plan.h): the stand-alone host program tests/env_plan_check.cpp under
AddressSanitizer / UBSan in a child process, against the values the launch functions' own expressions gave."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))

from test_wgrad_rows_staged_cpu import _host_compiler, _sanitizer_flags  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def test_launch_plan_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags, reason = _sanitizer_flags(cxx, tmp_path)
    if flags is None:
        pytest.skip("no statically linked sanitizer runtime that starts here: " + reason)
    exe = str(tmp_path / "env_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags + ["-o", exe, os.path.join(HERE, "env_plan_check.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("ok: 9 rows") and "FAIL" not in run.stdout and "runtime error" not in run.stderr
