"""The reduce launch of ``macjd_linear_wgrad_many_norm`` on problems that take no part in the partial-products launch
(``macjd_wgrad_io.kind``, csrc/macjd_wgrad.hip): ROW PRODUCTS, whose terms the reduce forms from the operands, and EXTERNAL
SLOTS, whose partial slots are in the workspace already — here written by the test in the partial launch's layout.

K in {1, 7, 8, 9, 33} rows resp. slots: a single term, one short of / exactly / one past a wave's round of eight, and a
second round for wave 0 (terms 32 ..).  Outputs [1 x 64] and [64 x 70] with a bias (two column tiles of padding in the
slot layout), [64 x 46] contracted (slots of [2][46]).  Buffers, bounds, ``partials[w]`` and ``step`` as in
tests/test_norm_in_reduce_gpu.py: NaN margins and NaN row gaps; against a float64 evaluation of the same float32 operands,
(additions on the longest chain of the output) x 2^-24 x sum |terms| with the reduce's chain ceil(K / 32) + 3 + 2 (one of a
wave's eight accumulators, their tree, the four waves) and one more rounding per term of a row product (the fused multiply-add
rounds once; counted as if it were two); partials within (1 + 6) x 2^-24 of the squares of what was stored."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_norm_in_reduce_gpu import DEV, U, Buf, _stream, _wgrad_io  # noqa: E402

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -4
KS = [1, 7, 8, 9, 33]


def _pad(v):
    return (v + 63) // 64 * 64


def _run(lib, _native, ios, ln_problem, dg=None, dbt=None, W=None):
    arr = (_native.WgradIO * len(ios))(*ios)
    n_partials = int(lib.macjd_linear_wgrad_many_norm_partials(arr, len(ios), ln_problem))
    assert n_partials >= 1
    partials = Buf(1, n_partials)
    step = torch.full((3,), float("nan"), device=DEV)
    step[1] = 7.0
    nio = _native.WgradNormIO()
    nio.ln_problem, nio.partials_cap = ln_problem, n_partials
    if ln_problem >= 0:
        nio.dgamma, nio.dbeta = dg.ptr, dbt.ptr
        if W is not None:
            nio.W, nio.w_ld = W.ptr, W.ld
    nio.partials, nio.step = partials.ptr, step[1:].data_ptr()
    with torch.cuda.device(DEV):
        _native.check(lib.macjd_linear_wgrad_many_norm(arr, len(ios), ctypes.byref(nio), _stream()), "macjd_linear_wgrad_many_norm")
    torch.cuda.synchronize()
    assert step[1].item() == 8.0 and bool(torch.isnan(step[0])) and bool(torch.isnan(step[2]))
    assert partials.untouched_outside()
    return arr, partials


def _check_partials(partials, stored):
    n_partials = partials.cols
    stored = np.concatenate([stored, np.zeros(64 * n_partials - stored.size)]).reshape(n_partials, 64)
    sq_ref = (stored ** 2).sum(axis=1)
    assert np.all(np.abs(partials.np()[0] - sq_ref) <= (1 + 6) * U * sq_ref)


@pytest.mark.parametrize("K", KS)
def test_row_products_beside_an_ordinary_problem(K):
    """[K, 1] x [K, 64] and [K, 64] x [K, 70], both with a bias and strided rows, as row products; an ordinary problem
    ([70, 33] x [70, 67], no bias) in the same call stays bit-identical to macjd_linear_wgrad_many, and is the only one
    with work items in the partial-products launch (two column tiles x two chunks)."""
    from macjd_amd import _native
    lib = _native.load()
    rng = np.random.default_rng(K)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    g1, x1 = Buf(K, 1, r(K, 1), ld=3), Buf(K, 64, r(K, 64), ld=68)
    g2, x2 = Buf(K, 64, r(K, 64), ld=66), Buf(K, 70, r(K, 70), ld=71)
    g3, x3 = Buf(70, 33, r(70, 33)), Buf(70, 67, r(70, 67))
    out = dict(dW1=Buf(1, 64), db1=Buf(1, 1), dW2=Buf(64, 70, ld=72), db2=Buf(1, 64), dW3=Buf(33, 67))
    ref3 = Buf(33, 67)
    keep, ios = [], []
    for gout, inp, dW, db, kind in ((g1, x1, out["dW1"], out["db1"], 2), (g2, x2, out["dW2"], out["db2"], 2), (g3, x3, out["dW3"], None, 0)):
        io, ws = _wgrad_io(lib, _native, gout, inp, dW, db)
        io.kind = kind
        if kind:
            io.workspace = None          # not read
        ios.append(io)
        keep.append(ws)
    io3, ws3 = _wgrad_io(lib, _native, g3, x3, ref3, None)
    with torch.cuda.device(DEV):
        _native.check(lib.macjd_linear_wgrad_many((_native.WgradIO * 1)(io3), 1, _stream()), "macjd_linear_wgrad_many")
    arr, partials = _run(lib, _native, ios, -1)
    assert int(lib.macjd_linear_wgrad_many_norm_work_items(arr, 3, -1)) == 2 * 1 * 2
    assert torch.equal(out["dW3"].view, ref3.view) and bool(torch.isfinite(ref3.view).all())
    for k, b in out.items():
        assert b.untouched_outside(), k
    chain = -(-K // 32) + 3 + 2 + 1
    for gout, inp, dW, db in ((g1, x1, out["dW1"], out["db1"]), (g2, x2, out["dW2"], out["db2"])):
        g64, x64 = gout.np(), inp.np()
        err_w = np.abs(dW.np() - g64.T @ x64)
        err_b = np.abs(db.np()[0] - g64.sum(0))
        print(f"K={K} [{gout.cols} x {inp.cols}]: dW err/bound {np.max(err_w / (chain * U * (np.abs(g64).T @ np.abs(x64)))):.3f}")
        assert np.all(err_w <= chain * U * (np.abs(g64).T @ np.abs(x64)))
        assert np.all(err_b <= chain * U * np.abs(g64).sum(0))
    stored = np.concatenate([out["dW1"].np().ravel(), out["db1"].np().ravel(), out["dW2"].np().ravel(), out["db2"].np().ravel(),
                             out["dW3"].np().ravel(), np.zeros(33)])
    _check_partials(partials, stored)
    # only row products: no work item at all, i.e. no partial-products launch
    assert int(lib.macjd_linear_wgrad_many_norm_work_items((_native.WgradIO * 2)(*ios[:2]), 2, -1)) == 0


@pytest.mark.parametrize("K", KS)
def test_external_slots_with_a_contracted_problem(K):
    """K slots of a [1 x 64] and of a [64 x 70] problem with their bias rows, and K slots of [2][46] of the contracted one,
    written by the test (NaN in the padding of every slot: the reduce reads [M x N] of [Mp x Np] only).  No operand is
    given; no partial-products launch."""
    from macjd_amd import _native
    lib = _native.load()
    rng = np.random.default_rng(100 + K)
    N_LN = 46
    out = dict(dW1=Buf(1, 64), db1=Buf(1, 1), dW2=Buf(64, 70, ld=72), db2=Buf(1, 64), dg=Buf(1, N_LN), dbt=Buf(1, N_LN))
    ios, refs, keep = [], [], []
    for M, N, dW, db in ((1, 64, out["dW1"], out["db1"]), (64, 70, out["dW2"], out["db2"])):
        Mp, Np = _pad(M), _pad(N)
        floats = int(lib.macjd_wgrad_slot_floats(M, N, K))
        assert floats == K * Mp * Np + K * Mp
        host = np.full(floats, np.nan, dtype=np.float32)
        slots = host[:K * Mp * Np].reshape(K, Mp, Np)
        bias = host[K * Mp * Np:].reshape(K, Mp)
        slots[:, :M, :N] = rng.standard_normal((K, M, N))
        bias[:, :M] = rng.standard_normal((K, M))
        ws = Buf(1, floats, host.reshape(1, -1))
        io = _native.WgradIO()
        io.K, io.M, io.N, io.kind, io.ext_chunks = 1, M, N, 1, K
        io.dW, io.dw_ld, io.db, io.workspace = dW.ptr, dW.ld, db.ptr, ws.ptr
        ios.append(io)
        keep.append(ws)
        refs.append((slots[:, :M, :N].astype(np.float64), bias[:, :M].astype(np.float64), dW, db))
    ln_host = rng.standard_normal((K, 2, N_LN)).astype(np.float32)
    ln_ws = Buf(1, K * 2 * N_LN, ln_host.reshape(1, -1))
    io = _native.WgradIO()
    io.K, io.M, io.N, io.kind, io.ext_chunks, io.workspace = 1, 64, N_LN, 1, K, ln_ws.ptr
    ios.insert(1, io)
    arr, partials = _run(lib, _native, ios, 1, dg=out["dg"], dbt=out["dbt"])
    assert int(lib.macjd_linear_wgrad_many_norm_work_items(arr, 3, 1)) == 0
    for k, b in out.items():
        assert b.untouched_outside() and bool(torch.isfinite(b.view).all()), k
    chain = -(-K // 32) + 3 + 2
    for s64, b64, dW, db in refs:
        assert np.all(np.abs(dW.np() - s64.sum(0)) <= chain * U * np.abs(s64).sum(0))
        assert np.all(np.abs(db.np()[0] - b64.sum(0)) <= chain * U * np.abs(b64).sum(0))
    l64 = ln_host.astype(np.float64)
    assert np.all(np.abs(out["dg"].np()[0] - l64[:, 0].sum(0)) <= chain * U * np.abs(l64[:, 0]).sum(0))
    assert np.all(np.abs(out["dbt"].np()[0] - l64[:, 1].sum(0)) <= chain * U * np.abs(l64[:, 1]).sum(0))
    stored = np.concatenate([out["dW1"].np().ravel(), out["db1"].np().ravel(), out["dg"].np().ravel(), out["dbt"].np().ravel(),
                             out["dW2"].np().ravel(), out["db2"].np().ravel()])
    _check_partials(partials, stored)


def test_other_entry_points_turn_the_kinds_away():
    """macjd_linear_wgrad and macjd_linear_wgrad_many know no kinds: MACJD_EUNSUPPORTED, nothing launched; the grouped
    pair refuses a contracted row-products problem and one with an outer operand the same way."""
    from macjd_amd import _native
    lib = _native.load()
    g, x, dW = Buf(8, 4, np.ones((8, 4))), Buf(8, 5, np.ones((8, 5))), Buf(4, 5)
    for kind in (1, 2):
        io, ws = _wgrad_io(lib, _native, g, x, dW, None)
        io.kind, io.ext_chunks = kind, 1
        with torch.cuda.device(DEV):
            assert lib.macjd_linear_wgrad(ctypes.byref(io), _stream()) == EUNSUPPORTED
            assert lib.macjd_linear_wgrad_many((_native.WgradIO * 1)(io), 1, _stream()) == EUNSUPPORTED
    io, ws = _wgrad_io(lib, _native, g, x, None, None)
    io.kind = 2
    assert int(lib.macjd_linear_wgrad_many_norm_partials((_native.WgradIO * 1)(io), 1, 0)) == -1
    io, ws = _wgrad_io(lib, _native, g, x, dW, None)
    io.kind, io.outer_vec, io.outer_w = 2, g.ptr, g.ptr
    assert int(lib.macjd_linear_wgrad_many_norm_partials((_native.WgradIO * 1)(io), 1, -1)) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW.raw).all())
