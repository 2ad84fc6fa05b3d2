"""The staged form of the ROWS reduce (``macjd_linear_wgrad_many_norm_ex``, csrc/macjd_wgrad.hip: blocks of 256 outputs, one
per thread, on operand rows staged into LDS in slices of RS_KS = 32 terms) against the plain rows kernel (flag
MACJD_WGRAD_PLAIN_ROWS) on the same problem sets: every output, ``partials`` and ``step`` bit for bit.

Buffers as in tests/test_norm_in_reduce_gpu.py: NaN margins and NaN row gaps, so a staged element read from a gap or behind
the last row, or an LDS word used without having been staged, shows as a NaN or as a difference.  The staged form is also
held to the float64 bound of tests/test_wgrad_kinds_gpu.py: chain ceil(K / 32) + 3 + 2 + 1 roundings x 2^-24 x sum |terms|.

K: a single term, around a round of eight, the workload's 224, and around the slice length (31, 32, 33, 65 = one term
into a third slice)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_norm_in_reduce_gpu import DEV, U, Buf, _stream, _wgrad_io  # noqa: E402

pytestmark = pytest.mark.gpu
KS = 32          # RS_KS
N_CAP = 128      # WGMAP_N_CAP
PLAIN = 1        # MACJD_WGRAD_PLAIN_ROWS


def _pad(v):
    return (v + 63) // 64 * 64


class Shifted:
    """Columns [1, cols] of a Buf of cols + 1 columns: the same NaN surroundings, the base one float off its alignment."""

    def __init__(self, rows, cols, values, ld):
        self.buf = Buf(rows, cols + 1, np.concatenate([np.zeros((rows, 1), np.float32), values], axis=1), ld=ld)
        self.rows, self.cols, self.ld = rows, cols, ld
        self.ptr = self.buf.ptr + 4

    def np(self):
        return self.buf.np()[:, 1:]


def _rows_problem(gout, inp, bias=True, dw_ld=None):
    return SimpleNamespace(kind=2, gout=gout, inp=inp, M=gout.cols, N=inp.cols, bias=bias, dw_ld=dw_ld)


def _ordinary_problem(gout, inp):
    return SimpleNamespace(kind=0, gout=gout, inp=inp, M=gout.cols, N=inp.cols, bias=False, dw_ld=None)


def _slots_problem(rng, M, N, slots, bias=True, dw_ld=None):
    """`slots` external slots in the partial launch's layout, NaN in every slot's padding."""
    Mp, Np = _pad(M), _pad(N)
    host = np.full(slots * Mp * Np + slots * Mp, np.nan, dtype=np.float32)
    host[:slots * Mp * Np].reshape(slots, Mp, Np)[:, :M, :N] = rng.standard_normal((slots, M, N))
    host[slots * Mp * Np:].reshape(slots, Mp)[:, :M] = rng.standard_normal((slots, M))
    return SimpleNamespace(kind=1, ws=Buf(1, host.size, host.reshape(1, -1)), M=M, N=N, bias=bias, dw_ld=dw_ld, slots=slots)


def _ln_problem(rng, N, slots):
    """The contracted [64 x N] problem as `slots` external slots of [2][N]."""
    host = rng.standard_normal((slots, 2, N)).astype(np.float32)
    return SimpleNamespace(kind=1, ws=Buf(1, host.size, host.reshape(1, -1)), M=64, N=N, bias=False, dw_ld=None, slots=slots, ln=True)


def _run(lib, _native, problems, flags):
    """One launch pair on fresh outputs; returns (outputs in item order [(name, Buf)], partials, step, blocks)."""
    ios, outs, keep = [], [], []
    ln_problem, dg, dbt = -1, None, None
    for q, p in enumerate(problems):
        io = _native.WgradIO()
        io.M, io.N, io.kind = p.M, p.N, p.kind
        if getattr(p, "ln", False):
            ln_problem, dg, dbt = q, Buf(1, p.N), Buf(1, p.N)
            io.K, io.ext_chunks, io.workspace = 1, p.slots, p.ws.ptr
            outs += [(f"dgamma{q}", dg), (f"dbeta{q}", dbt)]
            ios.append(io)
            continue
        dW = Buf(p.M, p.N, ld=p.dw_ld)
        db = Buf(1, p.M) if p.bias else None
        io.dW, io.dw_ld, io.db = dW.ptr, dW.ld, db.ptr if db is not None else None
        if p.kind == 1:
            io.K, io.ext_chunks, io.workspace = 1, p.slots, p.ws.ptr
        else:
            io.K = p.gout.rows
            io.gout, io.gout_ld, io.inp, io.inp_ld = p.gout.ptr, p.gout.ld, p.inp.ptr, p.inp.ld
            if p.kind == 0:
                ws = Buf(1, int(lib.macjd_linear_wgrad_workspace_floats(io.K, io.M, io.N)))
                io.workspace = ws.ptr
                keep.append(ws)
        outs += [(f"dW{q}", dW), (f"db{q}", db)]
        ios.append(io)
    arr = (_native.WgradIO * len(ios))(*ios)
    n_partials = int(lib.macjd_linear_wgrad_many_norm_partials(arr, len(ios), ln_problem))
    blocks = int(lib.macjd_linear_wgrad_many_norm_blocks(arr, len(ios), ln_problem, flags))
    assert n_partials >= 1 and 1 <= blocks <= n_partials
    partials = Buf(1, n_partials)
    step = torch.full((3,), float("nan"), device=DEV)
    step[1] = 7.0
    nio = _native.WgradNormIO()
    nio.ln_problem, nio.partials_cap = ln_problem, n_partials
    if ln_problem >= 0:
        nio.dgamma, nio.dbeta = dg.ptr, dbt.ptr
    nio.partials, nio.step = partials.ptr, step[1:].data_ptr()
    with torch.cuda.device(DEV):
        _native.check(lib.macjd_linear_wgrad_many_norm_ex(arr, len(ios), ctypes.byref(nio), flags, _stream()), "macjd_linear_wgrad_many_norm_ex")
    torch.cuda.synchronize()
    return outs, partials, step, blocks, n_partials


def _both(problems):
    """The problem set through the staged form and through the plain rows kernel: everything equal bit for bit, nothing
    written outside the outputs, all finite, the staged row products within the float64 bound, ``partials[w]`` the squares
    of items [64 w, 64 w + 64).  Returns (staged blocks, plain blocks, staged outputs)."""
    from macjd_amd import _native
    lib = _native.load()
    s_out, s_part, s_step, s_blocks, n_partials = _run(lib, _native, problems, 0)
    p_out, p_part, p_step, p_blocks, _ = _run(lib, _native, problems, PLAIN)
    assert p_blocks == n_partials
    for (name, a), (_, b) in zip(s_out, p_out):
        if a is None:
            continue
        assert torch.equal(a.view, b.view), name
        assert bool(torch.isfinite(a.view).all()), name
        assert a.untouched_outside() and b.untouched_outside(), name
    assert torch.equal(s_part.view, p_part.view) and bool(torch.isfinite(s_part.view).all())
    assert s_part.untouched_outside() and p_part.untouched_outside()
    for step in (s_step, p_step):
        assert step[1].item() == 8.0 and bool(torch.isnan(step[0])) and bool(torch.isnan(step[2]))
    assert torch.equal(s_step[1], p_step[1])
    # float64 bound of the staged form's row products
    outs = dict(s_out)
    for q, p in enumerate(problems):
        if p.kind != 2:
            continue
        K = p.gout.rows
        chain = -(-K // 32) + 3 + 2 + 1
        g64, x64 = p.gout.np(), p.inp.np()
        err_w = np.abs(outs[f"dW{q}"].np() - g64.T @ x64)
        bound = chain * U * (np.abs(g64).T @ np.abs(x64))
        print(f"K={K} [{p.M} x {p.N}]: staged dW err/bound {np.max(err_w / bound):.3f}")
        assert np.all(err_w <= bound)
        if p.bias:
            assert np.all(np.abs(outs[f"db{q}"].np()[0] - g64.sum(0)) <= chain * U * np.abs(g64).sum(0))
    # partials[w]: the layout tests/test_wgrad_kinds_gpu.py::_check_partials pins
    stored = []
    for q, p in enumerate(problems):
        if getattr(p, "ln", False):
            stored += [outs[f"dgamma{q}"].np().ravel(), outs[f"dbeta{q}"].np().ravel()]
        else:
            stored += [outs[f"dW{q}"].np().ravel(), outs[f"db{q}"].np().ravel() if p.bias else np.zeros(p.M)]
    stored = np.concatenate(stored)
    stored = np.concatenate([stored, np.zeros(64 * n_partials - stored.size)]).reshape(n_partials, 64)
    sq_ref = (stored ** 2).sum(axis=1)
    assert np.all(np.abs(s_part.np()[0] - sq_ref) <= (1 + 6) * U * sq_ref)
    return s_blocks, p_blocks, outs


def _r(rng):
    return lambda *s: rng.standard_normal(s).astype(np.float32)


@pytest.mark.parametrize("K", sorted({1, 7, 8, 9, 33, 224, KS - 1, KS, KS + 1, 2 * KS + 1}))
def test_problem_set_of_the_kinds_test(K):
    """[K, 1] x [K, 64] + bias with ld 3 / 68; [K, 64] x [K, 70] + bias with ld 66 / 71 (dword staging; it starts at flat
    item 65: fast blocks from item 128 on, a plain head and tail); an ordinary [70, 33] x [70, 67]."""
    rng = np.random.default_rng(K)
    r = _r(rng)
    problems = [_rows_problem(Buf(K, 1, r(K, 1), ld=3), Buf(K, 64, r(K, 64), ld=68)),
                _rows_problem(Buf(K, 64, r(K, 64), ld=66), Buf(K, 70, r(K, 70), ld=71), dw_ld=72),
                _ordinary_problem(Buf(70, 33, r(70, 33)), Buf(70, 67, r(70, 67)))]
    staged, plain, _ = _both(problems)
    assert staged == plain - 3 * ((65 + 64 * 70 - 128) // 256)


@pytest.mark.parametrize("K", [9, 224])
def test_aligned_operands_and_the_same_one_float_off(K):
    """[K, 6] x [K, 128], every ld and base a multiple of four floats: 16-byte staging loads, 768 weight items = three fast
    blocks; then the same `inp` values one float into an aligned buffer: dword loads, the same results."""
    rng = np.random.default_rng(300 + K)
    r = _r(rng)
    g, x = r(K, 6), r(K, 128)
    aligned = _rows_problem(Buf(K, 6, g, ld=8), Buf(K, 128, x, ld=132), dw_ld=128)
    assert aligned.inp.ptr % 16 == 0 and aligned.gout.ptr % 16 == 0
    staged, plain, out_a = _both([aligned])
    assert (staged, plain) == (3 + 1, 13)
    shifted = _rows_problem(Buf(K, 6, g, ld=8), Shifted(K, 128, x, ld=132), dw_ld=128)
    assert shifted.inp.ptr % 16 == 4
    staged, plain, out_s = _both([shifted])
    assert (staged, plain) == (3 + 1, 13)
    assert torch.equal(out_a["dW0"].view, out_s["dW0"].view) and torch.equal(out_a["db0"].view, out_s["db0"].view)
    assert shifted.inp.buf.untouched_outside()


@pytest.mark.parametrize("N", [40, 100])
def test_aligned_operands_narrower_than_the_cap(N):
    """[33, 8] x [33, N], aligned, N a multiple of four below 128: a row is N / 4 < 32 float4, so the upper lanes of each
    half-wave have no column of their own (they re-read the last one and store nothing), and rows wrap inside a wave."""
    K = KS + 1
    rng = np.random.default_rng(700 + N)
    r = _r(rng)
    p = _rows_problem(Buf(K, 8, r(K, 8), ld=8), Buf(K, N, r(K, N), ld=N + 4), dw_ld=N)
    assert p.inp.ptr % 16 == 0
    staged, plain, _ = _both([p])
    assert plain == -(-(8 * N + 8) // 64) and staged == plain - 3 * (8 * N // 256)


@pytest.mark.parametrize("K", [KS + 1, 224])
def test_wrapping_rows(K):
    """[K, 32] x [K, 46] (ld 46) + bias: a lane's n wraps inside a wave and a block's items span 6 - 7 gout columns."""
    rng = np.random.default_rng(400 + K)
    r = _r(rng)
    staged, plain, _ = _both([_rows_problem(Buf(K, 32, r(K, 32)), Buf(K, 46, r(K, 46), ld=46))])
    assert plain == -(-(32 * 46 + 32) // 64) and staged == plain - 3 * (32 * 46 // 256)


def test_degenerate_shapes():
    """K = 9.  One `inp` column (256 gout columns per block): refused to the plain path.  N at the cap and one past it with
    one output row (128 weight items: no room for a fast block) and with two (the cap: one fast block; past it: none)."""
    K = 9
    rng = np.random.default_rng(500)
    r = _r(rng)
    staged, plain, _ = _both([_rows_problem(Buf(K, 300, r(K, 300)), Buf(K, 1, r(K, 1)))])
    assert staged == plain == -(-600 // 64)
    for M, N, fast in ((1, N_CAP, 0), (1, N_CAP + 1, 0), (2, N_CAP, 1), (2, N_CAP + 1, 0)):
        staged, plain, _ = _both([_rows_problem(Buf(K, M, r(K, M)), Buf(K, N, r(K, N)))])
        assert plain == -(-(M * N + M) // 64) and staged == plain - 3 * fast, (M, N)


@pytest.mark.parametrize("order", ["rows_slots_ln", "slots_ln_rows"])
def test_all_kinds_in_one_launch(order):
    """A ROW PRODUCTS problem ([33, 64] x [33, 70] + bias), an EXTERNAL SLOTS problem of 9 slots ([1 x 64] + bias) and the
    contracted [64 x 46] problem as 9 external slots, in both orders."""
    rng = np.random.default_rng(600)
    r = _r(rng)
    rows = _rows_problem(Buf(33, 64, r(33, 64), ld=66), Buf(33, 70, r(33, 70), ld=71), dw_ld=72)
    slots = _slots_problem(rng, 1, 64, 9)
    ln = _ln_problem(rng, 46, 9)
    problems = [rows, slots, ln] if order == "rows_slots_ln" else [slots, ln, rows]
    staged, plain, _ = _both(problems)
    first = 0 if order == "rows_slots_ln" else 65 + 2 * 46
    g_lo = -(-first // 64)
    assert staged == plain - 3 * ((first + 64 * 70 - 64 * g_lo) // 256)
