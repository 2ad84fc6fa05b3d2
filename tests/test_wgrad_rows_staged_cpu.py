"""Host side of the staged ROWS reduce (MACJD_ROWS_STAGED, csrc/macjd_wgrad_map.h): the switch and the exports, the
block counts of a few problem sets through the C-ABI (host tables only: nothing is launched), and the block-map
builder under AddressSanitizer / UBSan as a stand-alone program (tests/wgrad_map_check.cpp) in a child process."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))

from macjd_amd import _native, options  # noqa: E402
from test_norm_in_reduce_cpu import _io  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, EXT = _native.WGRAD_ROW_PRODUCTS, _native.WGRAD_EXT_SLOTS


def test_switch_and_exports():
    assert options._DEFAULTS["ROWS_STAGED"] == "1" and "MACJD_ROWS_STAGED" in options.__doc__
    hdr = open(os.path.join(HERE, "..", "include", "macjd_nets.h")).read()
    for name in ("macjd_linear_wgrad_many_norm_ex", "macjd_linear_wgrad_many_norm_blocks"):
        assert name in _native.EXPORTS and f"{name}(" in hdr
    assert "#define MACJD_WGRAD_PLAIN_ROWS 1u" in hdr and _native.WGRAD_PLAIN_ROWS == 1


def _rows(K, M, N, inp=0x510000, inp_ld=None):
    io = _io(K, M, N, 0x500000, inp, 0x800000, 0x900000)
    io.kind, io.workspace = ROWS, None
    if inp_ld is not None:
        io.inp_ld = inp_ld
    return io


def _blocks(ios, ln=-1, flags=0):
    lib = _native.load()
    arr = (_native.WgradIO * len(ios))(*ios)
    return int(lib.macjd_linear_wgrad_many_norm_blocks(arr, len(ios), ln, flags)), int(lib.macjd_linear_wgrad_many_norm_partials(arr, len(ios), ln))


def test_block_counts():
    """A fast block stands for four 64-item groups of weight items; bias items, heads, tails and N outside 37..128 stay
    one plain block per group.  ``partials`` is what it was."""
    # [224, 6] x [224, 128]: 768 weight items = 3 fast blocks, 6 bias items = 1 plain block
    blocks, partials = _blocks([_rows(224, 6, 128)])
    assert (blocks, partials) == (3 + 1, 13)
    assert _blocks([_rows(224, 6, 128)], flags=_native.WGRAD_PLAIN_ROWS) == (13, 13)
    # the default learner's largest problem, 384 x 46 + 384: 17 664 weight items = 69 fast blocks, the rest plain
    blocks, partials = _blocks([_rows(224, 384, 46)])
    assert partials == -(-(384 * 46 + 384) // 64) and blocks == 69 + (partials - 4 * 69)
    # N = 1 (256 gout columns per block), N = 36 and N = 129: refused to the plain path; 37 and 128: taken
    for M, N, fast in ((300, 1, 0), (40, 36, 0), (40, 37, 5), (2, 128, 1), (2, 129, 0), (1, 128, 0), (1, 129, 0)):
        blocks, partials = _blocks([_rows(9, M, N)])
        assert partials == -(-(M * N + M) // 64) and blocks == partials - 3 * fast, (M, N)
    # a second problem starts wherever the first ends: its fast blocks start on the next 64-item boundary
    ios = [_rows(9, 1, 64), _rows(9, 64, 70)]        # 65 items, then 4480 weight items from item 65
    blocks, partials = _blocks(ios)
    fast = (65 + 4480 - 128) // 256
    assert partials == -(-(65 + 4480 + 64) // 64) and blocks == partials - 3 * fast
    # no ROW PRODUCTS problem: the launch is the other kernel's
    io = _io(1, 64, 32, None, None, 0x800000, 0x900000)
    io.kind, io.ext_chunks, io.workspace = EXT, 9, 0xA00000
    assert _blocks([io]) == (33, 33)


def _host_compiler():
    for cand in ("c++", "g++", "clang++"):
        path = shutil.which(cand)
        if path:
            return path
    return None


def _sanitizer_flags(cxx, tmp_path):
    """Flags that build AND run a trivial program with the sanitizer runtimes linked statically (the child then starts in
    whatever environment it inherits), or None with the reason."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    reason = "no flag set tried"
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static
        exe = str(tmp_path / "probe")
        build = subprocess.run([cxx, "-std=c++17"] + flags + ["-o", exe, str(probe)], capture_output=True, text=True)
        if build.returncode != 0:
            reason = (build.stderr.strip().splitlines() or ["build failed"])[-1]
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if run.returncode == 0:
            return flags, None
        reason = (run.stderr.strip().splitlines() or [f"exit {run.returncode}"])[-1]
    return None, reason


def test_block_map_builder_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags, reason = _sanitizer_flags(cxx, tmp_path)
    if flags is None:
        pytest.skip("no statically linked sanitizer runtime that starts here: " + reason)
    exe = str(tmp_path / "wgrad_map_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags + ["-o", exe, os.path.join(HERE, "wgrad_map_check.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "4000"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: 4000 sets") and "runtime error" not in run.stderr
