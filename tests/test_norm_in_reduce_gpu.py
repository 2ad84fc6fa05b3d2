"""The weight-gradient launch pair that also serves the optimiser step (``macjd_linear_wgrad_many_norm``: LayerNorm
contraction in the partial launch, squares and step counter in the reduce launch) and the one-launch optimiser step behind
it (``macjd_clip_adam_step_reduced``), at kernel, optimiser and learner level.

Error bounds are what the kernels' FIXED summation orders give against a float64 evaluation of the same float32 operands:
(additions on the longest chain of the output) x 2^-24 x sum |terms|.  The chains, from csrc/macjd_wgrad.hip and
csrc/macjd_nets.hip:

  dgamma[n]   a work item: its <= 64 reduction rows through the MFMA accumulator (counted as a product and an addition per
              row: 2 min(K, 64)), 8 fused multiply-adds over the lane's accumulator rows, 2 additions across the lane
              groups, 1 across the wave pair; the reduce: ceil(slots / 32) additions into one of a wave's 8 accumulators
              (slots = row tiles x chunks), 3 to combine the 8, 2 for the four waves.
  dbeta[n]    the same with the column sum of the staged chunk in place of the MFMA: min(K, 64) additions + 1.
  partials[w] one rounding per square (fused into the addition), 6 additions of the wave sum.
  grad_norm   ceil(n / 256) additions per thread, 6 of the wave sum, 2 for the four waves; the square root halves the
              relative error of the sum and adds at most one ulp of its own.
"""
import ctypes
import gc
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from test_nets_cpu import make_args, quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
MARGIN = 96


class Buf:
    """A [rows, cols] float32 matrix of row stride ld inside a NaN-filled allocation with NaN margins and NaN row gaps."""

    def __init__(self, rows, cols, values=None, ld=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.raw = torch.full((2 * MARGIN + rows * self.ld,), float("nan"), dtype=torch.float32, device=DEV)
        self.view = self.raw[MARGIN:MARGIN + rows * self.ld].view(rows, self.ld)[:, :cols]
        if values is not None:
            self.view.copy_(torch.as_tensor(values, dtype=torch.float32))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def np(self):
        return self.view.cpu().numpy().astype(np.float64)

    def untouched_outside(self):
        inside = torch.zeros_like(self.raw, dtype=torch.bool)
        inside[MARGIN:MARGIN + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = True
        return bool(torch.isnan(self.raw[~inside]).all())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _wgrad_io(lib, _native, gout, inp, dW, db):
    io = _native.WgradIO()
    io.K, io.M, io.N = gout.rows, gout.cols, inp.cols
    io.gout, io.gout_ld, io.inp, io.inp_ld = gout.ptr, gout.ld, inp.ptr, inp.ld
    if dW is not None:
        io.dW, io.dw_ld = dW.ptr, dW.ld
    io.db = db.ptr if db is not None else None
    ws = Buf(1, int(lib.macjd_linear_wgrad_workspace_floats(io.K, io.M, io.N)))
    io.workspace = ws.ptr
    return io, ws


@pytest.mark.parametrize("K", [1, 64, 65, 224])
@pytest.mark.parametrize("N", [5, 46])
def test_contracted_problem_beside_ordinary_ones(K, N):
    """Three problems in one launch pair — an ordinary one with a bias ([K, 70] x [K, N]), the LayerNorm-contracted one on
    the same [K, 70] operand (two row tiles, the second ragged) and an ordinary one without a bias ([K, 33] x [K, 67], two
    column tiles, padded output rows) — with NaN around and between the rows of every buffer: dW / db bitwise equal to
    macjd_linear_wgrad_many, dgamma / dbeta / partials within the bounds of the module docstring, the step counter advanced
    by one, nothing written outside the outputs."""
    from macjd_amd import _native
    lib = _native.load()
    M = 70
    rng = np.random.default_rng(1000 * K + N)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    ga, s_, xh, W = Buf(K, M, r(K, M), ld=M + 2), Buf(K, N, r(K, N)), Buf(K, N, r(K, N), ld=N + 3), Buf(M, N, r(M, N), ld=N + 1)
    gb_, ib = Buf(K, 33, r(K, 33)), Buf(K, 67, r(K, 67))

    def outputs():
        return dict(dW0=Buf(M, N), db0=Buf(1, M), G=Buf(M, N), dW2=Buf(33, 67, ld=70), dg=Buf(1, N), dbt=Buf(1, N))

    ref, got = outputs(), outputs()
    keep = []

    def problems(o, contracted):
        ios = []
        for gout, inp, dW, db in ((ga, s_, o["dW0"], o["db0"]), (ga, xh, None if contracted else o["G"], None), (gb_, ib, o["dW2"], None)):
            io, ws = _wgrad_io(lib, _native, gout, inp, dW, db)
            ios.append(io)
            keep.append(ws)
        return (_native.WgradIO * 3)(*ios)

    with torch.cuda.device(DEV):
        _native.check(lib.macjd_linear_wgrad_many(problems(ref, False), 3, _stream()), "macjd_linear_wgrad_many")
        arr = problems(got, True)
        n_partials = int(lib.macjd_linear_wgrad_many_norm_partials(arr, 3, 1))
        total_items = (M * N + M) + 2 * N + (33 * 67 + 33)
        assert n_partials == -(-total_items // 64)
        partials = Buf(1, n_partials)
        step = torch.full((3,), float("nan"), device=DEV)
        step[1] = 7.0
        nio = _native.WgradNormIO()
        nio.ln_problem, nio.partials_cap = 1, n_partials
        nio.W, nio.w_ld, nio.dgamma, nio.dbeta = W.ptr, W.ld, got["dg"].ptr, got["dbt"].ptr
        nio.partials, nio.step = partials.ptr, step[1:].data_ptr()
        _native.check(lib.macjd_linear_wgrad_many_norm(arr, 3, ctypes.byref(nio), _stream()), "macjd_linear_wgrad_many_norm")
    torch.cuda.synchronize()
    # ordinary problems: bit for bit; G is not written on this path
    for k in ("dW0", "db0", "dW2"):
        assert torch.equal(ref[k].view, got[k].view) and bool(torch.isfinite(got[k].view).all()), k
    assert bool(torch.isnan(got["G"].raw).all())
    for k, b in list(got.items()) + [("partials", partials)]:
        assert b.untouched_outside(), k
    assert step[1].item() == 8.0 and bool(torch.isnan(step[0])) and bool(torch.isnan(step[2]))
    # dgamma / dbeta against float64 of the same operands
    g64, x64, w64 = ga.np(), xh.np(), W.np()
    rows = min(K, 64)
    slots = 2 * -(-K // 64)
    reduce_chain = -(-slots // 32) + 3 + 2
    chain_g = 2 * rows + 8 + 2 + 1 + reduce_chain
    chain_b = rows + 1 + 8 + 2 + 1 + reduce_chain
    dg_ref = np.einsum("mn,km,kn->n", w64, g64, x64)
    dg_abs = np.einsum("mn,km,kn->n", np.abs(w64), np.abs(g64), np.abs(x64))
    db_ref = np.einsum("mn,km->n", w64, g64)
    db_abs = np.einsum("mn,km->n", np.abs(w64), np.abs(g64))
    err_g, err_b = np.abs(got["dg"].np()[0] - dg_ref), np.abs(got["dbt"].np()[0] - db_ref)
    print(f"K={K} N={N}: dgamma err/bound {np.max(err_g / (chain_g * U * dg_abs)):.3f} (chain {chain_g}), "
          f"dbeta {np.max(err_b / (chain_b * U * db_abs)):.3f} (chain {chain_b})")
    assert np.all(err_g <= chain_g * U * dg_abs)
    assert np.all(err_b <= chain_b * U * db_abs)
    # partial squares: what each reduce workgroup stored, in item order (the bias items of the bias-less problem count zero)
    stored = np.concatenate([got["dW0"].np().ravel(), got["db0"].np().ravel(), got["dg"].np().ravel(), got["dbt"].np().ravel(),
                             got["dW2"].np().ravel(), np.zeros(33)])
    assert stored.size == total_items
    stored = np.concatenate([stored, np.zeros(64 * n_partials - total_items)]).reshape(n_partials, 64)
    sq_ref = (stored ** 2).sum(axis=1)
    err_p = np.abs(partials.np()[0] - sq_ref)
    assert np.all(err_p <= (1 + 6) * U * sq_ref)


def _adam_io(_native, n, param, grad, m, v, step, norm, partials, max_norm):
    io = _native.AdamIO()
    io.n, io.lr, io.beta1, io.beta2, io.eps, io.max_norm = n, 1e-3, 0.9, 0.999, 1e-8, max_norm
    io.param, io.grad, io.exp_avg, io.exp_avg_sq = param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
    io.step, io.grad_norm, io.partials = step.data_ptr(), norm.data_ptr(), partials.data_ptr()
    return io


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("p", [1, 255, 256, 257, 1600])
def test_launch_pair_and_one_launch_step_equal_the_three_launches(p, clip):
    """One problem [2, p] x [2, 63] with a bias: p x 64 outputs = p reduce workgroups = p partials.  Its operands are small
    integers over 8, so every gradient, square and partial sum is exact in float32 in ANY order: the new pair + one-launch
    step and macjd_linear_wgrad_many + macjd_clip_adam_step see the same norm, hence the same clip coefficient, and must
    then agree bit for bit in parameters, moments, clipped gradients and norm.  The step counter advances exactly once."""
    from macjd_amd import _native
    lib = _native.load()
    rng = np.random.default_rng(p)
    gout_v, inp_v = rng.integers(-2, 3, (2, p)), rng.integers(-1, 2, (2, 63)) / 8.0
    gout_v[:, 0], inp_v[:, 0] = (2, 1), (0.125, 0.125)   # (p = 1: not all zero)
    gout, inp = Buf(2, p, gout_v), Buf(2, 63, inp_v)
    n = 64 * p
    init = [torch.tensor(rng.standard_normal(n), dtype=torch.float32, device=DEV) for _ in range(2)]
    init.append(torch.tensor(rng.random(n) * 1e-2, dtype=torch.float32, device=DEV))
    exact_sq = None
    sides = []
    for new in (False, True):
        grad = torch.full((n + 2 * MARGIN,), float("nan"), device=DEV)
        g = grad[MARGIN:MARGIN + n]
        dW, db = SimpleNamespace(ptr=g.data_ptr(), ld=63), SimpleNamespace(ptr=g[63 * p:].data_ptr())
        io, ws = _wgrad_io(lib, _native, gout, inp, dW, db)
        arr = (_native.WgradIO * 1)(io)
        param, m, v = [t.clone() for t in init]
        step, norm = torch.tensor([3.0], device=DEV), torch.zeros(1, device=DEV)
        partials = Buf(1, max(p, 256))
        with torch.cuda.device(DEV):
            if new:
                assert int(lib.macjd_linear_wgrad_many_norm_partials(arr, 1, -1)) == p
                nio = _native.WgradNormIO()
                nio.ln_problem, nio.partials_cap, nio.partials, nio.step = -1, p, partials.ptr, step.data_ptr()
                _native.check(lib.macjd_linear_wgrad_many_norm(arr, 1, ctypes.byref(nio), _stream()), "macjd_linear_wgrad_many_norm")
            else:
                _native.check(lib.macjd_linear_wgrad_many(arr, 1, _stream()), "macjd_linear_wgrad_many")
            torch.cuda.synchronize()
            if exact_sq is None:
                exact_sq = float((g.double() ** 2).sum())
                assert exact_sq * 64 == int(exact_sq * 64) < 2 ** 24 and exact_sq > 0
            max_norm = (0.5 * math.sqrt(exact_sq)) if clip else 1e9
            aio = _adam_io(_native, n, param, g, m, v, step, norm, partials.view, max_norm)
            if new:
                _native.check(lib.macjd_clip_adam_step_reduced(ctypes.byref(aio), p, None, _stream()), "macjd_clip_adam_step_reduced")
            else:
                _native.check(lib.macjd_clip_adam_step(ctypes.byref(aio), _stream()), "macjd_clip_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isnan(grad[:MARGIN]).all()) and bool(torch.isnan(grad[MARGIN + n:]).all())
        assert partials.untouched_outside()
        sides.append((param, m, v, g.clone(), norm, step))
    for i, (a, b) in enumerate(zip(*sides)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), i
    assert sides[1][5].item() == 4.0
    assert sides[1][4].item() == np.float32(math.sqrt(exact_sq))
    assert not torch.equal(sides[1][0], init[0])


@pytest.mark.parametrize("p", [1, 255, 256, 257, 1600, 2049])
def test_one_launch_step_sums_the_partials_in_its_fixed_order(p):
    """The step fed p arbitrary partials (NaN behind them): the norm against float64 within the bound of the module
    docstring (2049: a second round of loads), the step counter left alone — this launch reads it — and no other launch's
    output needed."""
    from macjd_amd import _native
    lib = _native.load()
    rng = np.random.default_rng(p)
    partials = Buf(1, p, rng.random((1, p)) * rng.choice([1e-3, 1.0, 50.0], (1, p)))
    n = 1000
    param, g, m, v = [torch.tensor(rng.standard_normal(n), dtype=torch.float32, device=DEV) for _ in range(3)] + [torch.ones(n, device=DEV)]
    step, norm = torch.tensor([5.0], device=DEV), torch.zeros(1, device=DEV)
    aio = _adam_io(_native, n, param, g, m, v, step, norm, partials.view, 1e9)
    with torch.cuda.device(DEV):
        _native.check(lib.macjd_clip_adam_step_reduced(ctypes.byref(aio), p, None, _stream()), "macjd_clip_adam_step_reduced")
    torch.cuda.synchronize()
    ref = math.sqrt(partials.np().sum())
    chain = -(-p // 256) + 6 + 2
    assert abs(norm.item() - ref) <= ref * (chain / 2 * U + 2 * U)
    assert step.item() == 5.0 and bool(torch.isfinite(param).all())


