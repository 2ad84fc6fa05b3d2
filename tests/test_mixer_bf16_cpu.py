"""The fused mixer's operand type (``macjd_mixerf_io.operand_dtype``, include/macjd_nets.h) on the host side: the ctypes
mirror against the header, and the argument checks of the five entry points, which refuse an unknown operand type — and
a pair / training call whose two mixers disagree in it — with MACJD_EINVAL before anything is launched.  Every call
below returns from the library's own validation, so no GPU is needed."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

import __graft_entry__ as entry
from _harness import REPO
from macjd_amd import _native

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _native.load()


def _header_fields():
    """Member names of macjd_mixerf_io in declaration order, read from the header."""
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    body = re.search(r"typedef struct macjd_mixerf_io \{(.*?)\} macjd_mixerf_io;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.findall(r"\w+", first)[-1])
        names += [re.findall(r"\w+", r)[-1] for r in rest]
    return names


def test_mixer_io_mirror_matches_header(lib):
    names = _header_fields()
    assert "operand_dtype" in names and "reserved" not in names
    assert names == [f[0] for f in _native.MixerFusedIO._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           'int main(){printf("%zu %zu %zu\\n", sizeof(macjd_mixerf_io), offsetof(macjd_mixerf_io, operand_dtype), '
           'offsetof(macjd_mixerf_io, ln_eps));return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")],
                   check=True)
    out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ctypes.sizeof(_native.MixerFusedIO), _native.MixerFusedIO.operand_dtype.offset,
                   _native.MixerFusedIO.ln_eps.offset]
    assert lib.macjd_abi_version() == _native.ABI_VERSION


def _io(operand_dtype, save, M=0):
    """A 3j/4r argument block whose pointers are never dereferenced (M = 0: a valid call returns before any launch)."""
    io = _native.MixerFusedIO()
    io.M, io.J, io.S, io.Hh, io.Em = M, 3, 46, 128, 64
    io.save, io.operand_dtype, io.ln_eps = save, operand_dtype, 1e-5
    addr = iter(range(0x10000, 0x10000 + 0x1000 * 64, 0x1000))
    for name, ctype in _native.MixerFusedIO._fields_:
        if ctype is ctypes.c_void_p:
            setattr(io, name, next(addr))
    io.s_ld = io.S
    return io


def _td(M):
    td = _native.TdLossIO()
    td.B, td.Tm1, td.gamma = 1, M - 1, 0.99
    td.y, td.tq, td.reward, td.terminated, td.filled = 0x90000, 0x90004, 0xA0000, 0xB0000, 0xC0000
    td.y_sb = td.tq_sb = td.gy_cols = M
    return td


def _err(lib):
    return lib.macjd_last_error().decode()


def test_operand_type_is_validated_before_any_launch(lib):
    by = ctypes.byref
    # valid operand types with M = 0: accepted (nothing to launch)
    for dt in (0, 1):
        assert lib.macjd_mixer_fused_forward(by(_io(dt, 0)), None) == 0
        assert lib.macjd_mixer_fused_backward(by(_io(dt, 0)), None) == 0
        assert lib.macjd_mixer_fused_forward_pair(by(_io(dt, 1)), by(_io(dt, 0)), None) == 0
    for bad in (2, -1, 7):
        assert lib.macjd_mixer_fused_forward(by(_io(bad, 0)), None) == EINVAL
        assert "operand_dtype" in _err(lib)
        assert lib.macjd_mixer_fused_backward(by(_io(bad, 0)), None) == EINVAL
        assert "operand_dtype" in _err(lib)
        assert lib.macjd_mixer_fused_forward_pair(by(_io(bad, 1)), by(_io(bad, 0)), None) == EINVAL
        assert "operand_dtype" in _err(lib)
        assert lib.macjd_mixer_fused_backward_td(by(_io(bad, 0, M=8)), by(_td(8)), ctypes.c_void_p(0xD0000), None) == EINVAL
        assert "operand_dtype" in _err(lib)
        ev, tg = _io(bad, 1, M=8), _io(bad, 0, M=8)
        td = _td(8)
        td.y, td.tq = ev.y, tg.y + 4
        assert lib.macjd_mixer_fused_train(by(ev), by(tg), by(td), ctypes.c_void_p(0xD0000), None) == EINVAL
        assert "operand_dtype" in _err(lib)
    # the two mixers of one grid must agree
    assert lib.macjd_mixer_fused_forward_pair(by(_io(1, 1)), by(_io(0, 0)), None) == EINVAL
    assert "differ in operand_dtype" in _err(lib)
    assert lib.macjd_mixer_fused_forward_pair(by(_io(0, 1)), by(_io(1, 0)), None) == EINVAL
    assert "differ in operand_dtype" in _err(lib)
    ev, tg = _io(1, 1, M=8), _io(0, 0, M=8)
    td = _td(8)
    td.y, td.tq = ev.y, tg.y + 4
    assert lib.macjd_mixer_fused_train(by(ev), by(tg), by(td), ctypes.c_void_p(0xD0000), None) == EINVAL
    assert "differ in operand_dtype" in _err(lib)
