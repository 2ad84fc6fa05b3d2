"""The one-launch prefetch (``macjd_prefetch_batch``, include/macjd_nets.h ``macjd_prefetch_io``) without a GPU: the
counter-offset rule of its draws on the host restatement of the sampler, its switch, and header / exports / ctypes layout."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

import __graft_entry__ as entry
from _harness import REPO

from macjd_amd import _native, options
from tests_golden_helpers import sample_episodes_mirror


def _draw(n, N, counter, seed):
    """idx_out of one draw at counter value ``counter``: the restatement, and the kernel's rule for N < n."""
    return [t % N for t in range(n)] if N < n else sample_episodes_mirror(n, N, counter, seed)


@pytest.mark.parametrize("N", [1, 5, 8, 33])
@pytest.mark.parametrize("n", [2, 4])
def test_read_only_draws_at_offsets_equal_sequential_draws(N, n):
    """K - 1 prefetch launches that READ the counter at offsets 0 .. K-2 and a closing draw of offset K-1 that leaves the
    counter offset + 1 further == K draws that each advance the counter by one: same indices, same counter afterwards."""
    seed = 0x1234ABCD5678
    for c0 in (0, 7, (1 << 32) - 2):
        for K in (1, 2, 4, 20):
            counter, seq = c0, []
            for _ in range(K):                       # sample_episodes_block, offset 0
                seq.append(_draw(n, N, counter, seed))
                counter += 1
            dev_counter, got = c0, []
            for off in range(K - 1):                 # prefetch_batch_kernel: reads, never writes
                got.append(_draw(n, N, dev_counter + off, seed))
            got.append(_draw(n, N, dev_counter + (K - 1), seed))   # sample_episodes_block, offset K - 1
            dev_counter = dev_counter + (K - 1) + 1
            assert got == seq and dev_counter == counter
            for d in seq:
                assert all(0 <= x < N for x in d) and (N < n or len(set(d)) == n)
    if N >= n and N > 1:
        assert len({tuple(_draw(n, N, c, seed)) for c in range(32)}) > 1   # the offsets do select different draws


def test_switch_is_declared_and_documented():
    assert options._DEFAULTS["PREFETCH_LAUNCH"] == "1"
    assert re.search(r"^\s+MACJD_PREFETCH_LAUNCH\s+1 \| 0\s", options.__doc__, flags=re.M)
    for name in options._DEFAULTS:
        assert "MACJD_" + name in options.__doc__, name


def test_prefetch_struct_layout_and_exports_match_header():
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("macjd_prefetch_batch", "macjd_prefetch_batch_supported"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, plain) and sym in _native.EXPORTS
    body = re.search(r"typedef struct macjd_prefetch_io \{(.*?)\} macjd_prefetch_io;", plain, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert names == [f[0] for f in _native.PrefetchIO._fields_]
    fields = ["gru", "gather", "sampler", "mask", "tot_m", "no_draw", "gather_blocks"]
    structs = [("macjd_prefetch_io", _native.PrefetchIO), ("macjd_gru_io", _native.GruIO), ("macjd_gather_io", _native.GatherIO),
               ("macjd_sampler_io", _native.SamplerIO), ("macjd_tdloss_io", _native.TdLossIO)]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\nint main(){printf("'
           + "%zu " * (len(structs) + len(fields) + 1) + '\\n"'
           + "".join(", sizeof(%s)" % s for s, _ in structs)
           + "".join(", offsetof(macjd_prefetch_io, %s)" % f for f in fields)
           + ", offsetof(macjd_sampler_io, reserved));return 0;}\n")
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:len(structs)] == [ctypes.sizeof(c) for _, c in structs]
    assert out[len(structs):-1] == [getattr(_native.PrefetchIO, f).offset for f in fields]
    assert out[-1] == _native.SamplerIO.reserved.offset
    assert ctypes.sizeof(_native.PrefetchIO) <= 4096   # passed to the kernel by value
    entry.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "macjd_prefetch_batch") and hasattr(lib, "macjd_prefetch_batch_supported")
