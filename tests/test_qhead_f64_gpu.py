"""The update's Q-head launches — ``macjd_qhead_taken``, ``macjd_qhead_double_q``, ``macjd_qheads_pair``
(csrc/macjd_episode.hip) — and the Q-head's parameter gradients (``macjd_linear_wgrad`` / ``macjd_linear_wgrad_many`` with
``outer_vec``, csrc/macjd_wgrad.hip) against the float64 model of their contract (tests/qhead_f64_model.py, proved against
the reference's fixtures, the oracle and float64 torch in tests/test_qhead_f64_cpu.py), through the C-ABI, at the smallest
shapes at which these kernels can go wrong: row counts around the 16- and 32-row tiles, every supported action count, row
strides above their minimum, operands at odd float offsets, optional pointers NULL, out-of-range and non-int32 action
indices, the P row map, exact ties of the arg-max in every position relative to the split of the actions over two waves,
and reductions of K = 1 .. 129 rows around the 64-row chunk at the three load widths of the weight-gradient kernel.

Every output is pre-filled with NaN (the int64 arg-max with a sentinel), sits between NaN margins, has NaN gaps where the
row stride exceeds the row and NaN rows past n_rows: all must survive.  Every input sits between NaN margins and gaps (idx
between out-of-range values), so a read past an input shows up in the result.

Tolerances: act / q / out: min(ceiling, 8 Y) of qhead_f64_model (Y from the float32 oracle and the model alone); the arg-max
is the float64 first maximum on EVERY random row (tests/test_qhead_f64_cpu.py asserts that no row's top-two gap is inside
4 x tolerance); parameter gradients: gamma_(K+2) x sum |terms|, the any-order bound of a length-K float32 sum (the
outer_vec product is rounded once to float32 in the model itself).  Each test prints its worst |got - ref| / tolerance per
tensor.  Largest ratios on MI355X over all cases of this file (all must be <= 1):
    taken head     act 0.100   q 0.118                      (of min(ceiling, 8 Y); i.e. the kernel deviates from float64
    Double-DQN     out 0.088 (random cases)  0.121 (ties)    by about as much as the float32 oracle does: 8 x 0.12 ~ 1 Y)
    gradients      dW1 0.331   db1 0.025   dw2 0.272   db2 0.019   (of gamma_(K+2) sum|terms|; the largest at K = 1, where the
                   bound is three roundings of ONE term)
The arg-max equalled the float64 first maximum on all rows of all random cases; the smallest top-two gap of the inputs is
38 x (4 x tolerance).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import qhead_f64_model as qm  # noqa: E402
from test_mixer_f64_gpu import IN_MARGIN, _Guarded  # noqa: E402
from test_norm_in_reduce_gpu import Buf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, EUNSUPPORTED = 0, -1, -4     # include/macjd.h
EXTRA = 3                                # rows of every output past n_rows: must stay NaN
SENTINEL = -7777
H64 = 64
f32, f64 = np.float32, np.float64


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


class _In:
    """A float32 input [rows, cols] of row stride ``ld``, ``offset`` floats past a 16-byte boundary, NaN around and between
    the rows; ``extra_rows`` NaN rows behind the data."""

    def __init__(self, data, ld=None, offset=0, extra_rows=0):
        a = np.atleast_2d(np.asarray(data, dtype=f32))
        rows, cols = a.shape
        self.ld = ld or cols
        self.g = _Guarded((rows + extra_rows, self.ld), IN_MARGIN, offset=offset)
        self.g.t[:rows, :cols] = torch.as_tensor(a)
        self.ptr = self.g.buf.data_ptr() + 4 * self.g.lo
        assert (self.ptr // 4) % 4 == offset % 4


class _Idx:
    """Action indices (4 or 8 bytes) between out-of-range values."""

    def __init__(self, idx, size, A):
        dt = torch.int32 if size == 4 else torch.int64
        self.buf = torch.full((64 + len(idx),), A + 1000, dtype=dt, device=DEV)
        self.buf[32:32 + len(idx)] = torch.as_tensor(np.asarray(idx, dtype=np.int64)).to(dt)
        self.ptr = self.buf.data_ptr() + 32 * size


class _IntOut:
    """int64 output [n + EXTRA] pre-filled with a sentinel, sentinel margins."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((64 + n + EXTRA,), SENTINEL, dtype=torch.int64, device=DEV)
        self.ptr = self.buf.data_ptr() + 32 * 8

    def values(self):
        return self.buf[32:32 + self.n].cpu().numpy()

    def intact(self, n_written=None):
        n = self.n if n_written is None else n_written
        return bool((self.buf[:32] == SENTINEL).all()) and bool((self.buf[32 + n:] == SENTINEL).all())


def _rows_out(n, cols, ld=None):
    return Buf(n + EXTRA, cols, ld=ld)


def _intact(buf, n):
    """Margins, row gaps and the rows past n are still NaN."""
    return buf.untouched_outside() and bool(torch.isnan(buf.view[n:]).all())


def _all_nan(buf):
    return bool(torch.isnan(buf.raw).all())


def _ratio(err, tol):
    err, tol = np.asarray(err, f64), np.asarray(tol, f64)
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------- taken head
class _Taken:
    """Device operands, NaN-filled outputs and the argument block of one macjd_qhead_taken call."""

    def __init__(self, d, n, A, idx_size=8, h_ld=64, w1_pad=0, act_ld=64, x_pad=0, h_off=0, H=H64):
        _native, _ = _lib()
        W = H64 + A + 1
        self.n, self.A = n, A
        rows = max(n, 1)                                   # (n = 0: one row of operands behind valid pointers)
        self.h = _In(d["h"][:rows], ld=h_ld, offset=h_off)
        self.idx = _Idx(d["idx"][:rows], idx_size, A)
        self.P = _In(d["P"][:rows])
        self.W1 = _In(d["W1"], ld=W + w1_pad, offset=1)    # odd float offset: the fragment loads are declared unaligned
        self.b1, self.w2 = _In(d["b1"]), _In(d["w2"])
        self.b2 = _In(d["b2"]) if d["b2"] is not None else None
        self.x = _rows_out(n, W, ld=W + x_pad) if x_pad is not None else None
        self.act, self.q = _rows_out(n, H64, ld=act_ld), Buf(1, n + EXTRA)
        io = _native.QtakenIO()
        io.n_rows, io.H, io.A = n, H, A
        io.h, io.h_ld, io.idx, io.idx_elem_size, io.P = self.h.ptr, h_ld, self.idx.ptr, idx_size, self.P.ptr
        io.W1, io.w1_ld, io.b1, io.w2 = self.W1.ptr, W + w1_pad, self.b1.ptr, self.w2.ptr
        io.b2 = self.b2.ptr if self.b2 is not None else None
        if self.x is not None:
            io.x, io.x_ld = self.x.ptr, W + x_pad
        io.act, io.act_ld, io.q = self.act.ptr, act_ld, self.q.ptr
        self.io = io

    def outputs(self):
        return [b for b in (self.x, self.act, self.q) if b is not None]

    def launch(self):
        _, lib = _lib()
        rc = lib.macjd_qhead_taken(ctypes.byref(self.io), _stream())
        torch.cuda.synchronize()
        return rc

    def nothing_written(self):
        return all(_all_nan(b) for b in self.outputs())

    def intact(self):
        return (self.x is None or _intact(self.x, self.n)) and _intact(self.act, self.n) and \
            self.q.untouched_outside() and bool(torch.isnan(self.q.view[0, self.n:]).all())

    def got(self):
        n = self.n
        return (None if self.x is None else self.x.view[:n].cpu().numpy(), self.act.view[:n].cpu().numpy(), self.q.view[0, :n].cpu().numpy())


def _taken_of(case):
    return _Taken(qm.taken_inputs(case), case.n, case.A, case.idx_size, case.h_ld, case.w1_pad, case.act_ld, case.x_pad)


@pytest.mark.parametrize("case", qm.TAKEN_CASES, ids=lambda c: f"n{c.n}-A{c.A}-i{c.idx_size}")
def test_taken_head_matches_the_model(case):
    d = qm.taken_inputs(case)
    t = _taken_of(case)
    assert t.launch() == OK
    assert t.intact(), "margin, row gap or a row past n_rows written"
    x, act, q = t.got()
    x_ref, pre, act_ref, q_ref = qm.taken(d["h"], d["idx"], d["P"], d["W1"], d["b1"], d["w2"], d["b2"], case.A)
    if x is not None:
        assert np.array_equal(x.view(np.uint32), x_ref.view(np.uint32)), "x is not [h, onehot, P] bit for bit"
    assert not np.isnan(act).any() and not np.isnan(q).any(), "unwritten element, or NaN read from a margin"
    tol_a, tol_q = qm.tolerance(case, "act"), qm.tolerance(case, "q")
    err_a, err_q = np.abs(act - act_ref), np.abs(q - q_ref)
    print(f"{case}: act {_ratio(err_a, tol_a):.3f}  q {_ratio(err_q, tol_q):.3f}  (of the tolerance)")
    assert np.all(err_a <= tol_a) and np.all(err_q <= tol_q)
    clear = np.abs(pre) > tol_a
    assert np.array_equal((act > 0)[clear], (pre > 0)[clear]), "ReLU side differs from float64 outside the band"
    t2 = _taken_of(case)
    assert t2.launch() == OK
    for a, b in zip(t.got(), t2.got()):
        assert a is None or np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two runs differ"


def test_taken_head_argument_checks():
    """n_rows = 0: OK, nothing written.  h base 4 bytes off 16-byte alignment / h_ld = 66: MACJD_EINVAL; A = 65 / H = 128:
    MACJD_EUNSUPPORTED; nothing written in any of them."""
    case = qm.TAKEN_CASES[7]                               # n = 17, A = 5
    d = qm.taken_inputs(case)
    for kw, want in ((dict(n=0), OK), (dict(h_off=1), EINVAL), (dict(h_ld=66), EINVAL), (dict(H=128), EUNSUPPORTED)):
        t = _Taken(d, kw.pop("n", case.n), case.A, idx_size=4, **kw)
        assert t.launch() == want, kw
        assert t.nothing_written(), kw
    big = dict(d, W1=np.zeros((H64, H64 + 65 + 1), f32))
    t = _Taken(big, case.n, 65, idx_size=4)
    assert t.launch() == EUNSUPPORTED and t.nothing_written()


# ---------------------------------------------------------------------------------------------------- Double-DQN
class _DoubleQ:
    def __init__(self, d, H, A, n, h_pad=0, h_off=0, shared=False, p_pad=0, row_map=None, argmax=True):
        _native, _ = _lib()
        self.n = n
        rows = max(n, 1)
        W = H + A + 1
        self.h_e = _In(d["h_e"][:rows], ld=H + h_pad, offset=h_off)
        self.h_t = self.h_e if shared else _In(d["h_t"][:rows], ld=H + h_pad, offset=h_off)
        # (with a row map: NaN in the P rows behind those the map addresses)
        self.P_e = _In(d["P_e"], ld=A + p_pad, extra_rows=2 if row_map else 0)
        self.P_t = _In(d["P_t"], ld=A + p_pad, extra_rows=2 if row_map else 0)
        self.heads = []
        io = _native.DoubleQIO()
        io.n_rows, io.H, io.A = n, H, A
        io.h_e, io.he_ld, io.h_t, io.ht_ld = self.h_e.ptr, H + h_pad, self.h_t.ptr, H + h_pad
        io.P_e, io.pe_ld, io.P_t, io.pt_ld = self.P_e.ptr, A + p_pad, self.P_t.ptr, A + p_pad
        for tag, hd, pad in (("e", d["head_e"], 0), ("t", d["head_t"], 3)):      # w1e_ld != w1t_ld
            W1, b1, w2, b2 = _In(hd[0], ld=W + pad, offset=1), _In(hd[1]), _In(hd[2]), _In(hd[3])
            self.heads += [W1, b1, w2, b2]
            setattr(io, f"W1_{tag}", W1.ptr); setattr(io, f"w1{tag}_ld", W + pad)
            setattr(io, f"b1_{tag}", b1.ptr); setattr(io, f"w2_{tag}", w2.ptr); setattr(io, f"b2_{tag}", b2.ptr)
        self.out = Buf(1, n + EXTRA)
        self.am = _IntOut(n) if argmax else None
        io.out = self.out.ptr
        io.argmax_out = self.am.ptr if argmax else None
        if row_map:
            io.p_group, io.p_inner = row_map
        self.io = io

    def launch(self):
        _, lib = _lib()
        rc = lib.macjd_qhead_double_q(ctypes.byref(self.io), _stream())
        torch.cuda.synchronize()
        return rc

    def nothing_written(self):
        return _all_nan(self.out) and (self.am is None or self.am.intact(0))

    def intact(self):
        return self.out.untouched_outside() and bool(torch.isnan(self.out.view[0, self.n:]).all()) and (self.am is None or self.am.intact())

    def got(self):
        return self.out.view[0, :self.n].cpu().numpy(), (None if self.am is None else self.am.values())


def _dq_of(case, d):
    if isinstance(case, qm.TieCase):
        return _DoubleQ(d, case.H, case.A, case.n, h_pad=3, h_off=1, p_pad=2)
    return _DoubleQ(d, case.H, case.A, case.n, case.h_pad, case.h_off, case.shared, case.p_pad, case.row_map, case.argmax)


def _dq_id(c):
    return f"H{c.H}-A{c.A}-n{c.n}" + ("-map" if c.row_map else "") + ("-shared" if c.shared else "") + ("" if c.argmax else "-noargmax")


@pytest.mark.parametrize("case", qm.DQ_CASES, ids=_dq_id)
def test_double_q_matches_the_model(case):
    d = qm.dq_inputs(case)
    k = _dq_of(case, d)
    assert k.launch() == OK
    assert k.intact(), "margin or a row past n_rows written"
    out, am = k.got()
    q_e, q_t, am_ref, out_ref = qm.double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], case.A, case.row_map)
    if am is not None:
        assert np.array_equal(am, am_ref), f"arg-max differs from the float64 first maximum on rows {np.nonzero(am != am_ref)[0]}"
    assert not np.isnan(out).any(), "unwritten element, or NaN read from a margin / an unaddressed P row"
    tol = qm.tolerance(case, "out")[np.arange(case.n), am_ref]
    err = np.abs(out - out_ref)
    print(f"{case}: out {_ratio(err, tol):.3f} of the tolerance")
    assert np.all(err <= tol)
    k2 = _dq_of(case, d)
    assert k2.launch() == OK
    assert np.array_equal(out.view(np.uint32), k2.got()[0].view(np.uint32)), "two runs differ"


@pytest.mark.parametrize("case", qm.TIE_CASES, ids=lambda c: f"H{c.H}-A{c.A}-{c.cls}")
def test_double_q_takes_the_first_maximum_on_exact_ties(case):
    """Bit-identical eval values for a pair of actions (a) inside the first half, (b) across the split at AH = (A + 1) / 2,
    (c) inside the second half with its last real action (next to the padded slot), (d) all actions: where the pair is the
    maximum the arg-max is the LOWER index; out is the target head's value at the kernel's index on every row."""
    d = qm.tie_inputs(case)
    k = _dq_of(case, d)
    assert k.launch() == OK and k.intact()
    out, am = k.got()
    q_e, q_t, am_ref, _ = qm.double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], case.A)
    rows = qm.tie_rows(case)
    assert rows.size >= 2
    want = 0 if case.cls == "d" else d["pair"][0]
    assert np.array_equal(am[rows], np.full(rows.size, want)), f"pair {d['pair']}: arg-max {am[rows]} on the tied rows, not {want}"
    assert np.all((am >= 0) & (am < case.A)) and not np.isnan(out).any()
    # every other row: the kernel's index holds a value within the band of the float64 maximum
    r = np.arange(case.n)
    assert np.all(q_e.max(axis=1) - q_e[r, am] <= 2 * qm.tolerance(case, "q")[r, am])
    tol = qm.tolerance(case, "out")[r, am]
    err = np.abs(out - q_t[r, am])
    print(f"{case}: {rows.size} tied rows; out {_ratio(err, tol):.3f} of the tolerance")
    assert np.all(err <= tol)


def test_double_q_row_map_is_checked_on_the_host():
    """p_group > 0 with p_inner < 1 (a modulo by zero on the device) or p_inner > p_group, and p_group < 0: MACJD_EINVAL
    before any launch, from macjd_qhead_double_q and macjd_qheads_pair alike; outputs untouched."""
    _, lib = _lib()
    case = next(c for c in qm.DQ_CASES if c.row_map and c.H == 64 and c.A == 9)
    d = qm.dq_inputs(case)
    tcase = next(c for c in qm.TAKEN_CASES if c.A == 9)
    for group, inner in ((6, 0), (6, -1), (6, 7), (-6, 2), (-1, 0)):
        k = _dq_of(case, d)
        k.io.p_group, k.io.p_inner = group, inner
        assert k.launch() == EINVAL, (group, inner)
        assert k.nothing_written()
        t = _taken_of(tcase)
        assert lib.macjd_qheads_pair(ctypes.byref(t.io), ctypes.byref(k.io), _stream()) == EINVAL, (group, inner)
        torch.cuda.synchronize()
        assert k.nothing_written() and t.nothing_written()


# ---------------------------------------------------------------------------------------------------- pair
@pytest.mark.parametrize("n_taken,n_dq", qm.PAIR_CASES)
def test_pair_equals_the_two_single_launches(n_taken, n_dq):
    _, lib = _lib()
    A = 9
    td = qm.taken_inputs(qm.TakenCase(max(n_taken, 1), A, 8, 68, 3, 67, 2, True, 2))
    dd = qm.dq_inputs(qm.DqCase(64, A, max(n_dq, 1), 3, 1, False, 2, None, True, 2))
    mk_t = lambda: _Taken(td, n_taken, A, 8, 68, 3, 67, 2)
    mk_d = lambda: _DoubleQ(dd, 64, A, n_dq, 3, 1, False, 2, None, True)
    t1, k1, t2, k2 = mk_t(), mk_d(), mk_t(), mk_d()
    assert t1.launch() == OK and k1.launch() == OK
    assert lib.macjd_qheads_pair(ctypes.byref(t2.io), ctypes.byref(k2.io), _stream()) == OK
    torch.cuda.synchronize()
    assert t2.intact() and k2.intact(), "margin, row gap or a row past n_rows written"
    for a, b in zip(t1.got() + k1.got(), t2.got() + k2.got()):
        assert a.shape == b.shape and not np.isnan(np.asarray(b, f64)).any()
        assert np.array_equal(a, b), "the pair launch differs from the single launches"
    if n_taken == 0:
        assert t2.nothing_written()
    if n_dq == 0:
        assert k2.nothing_written()


def test_pair_argument_checks():
    _, lib = _lib()
    td = qm.taken_inputs(qm.TakenCase(17, 9, 8, 68, 3, 67, 2, True, 2))
    for H, A in ((64, 5), (128, 9)):                       # A differs: EINVAL; H = 128: EUNSUPPORTED
        dd = qm.dq_inputs(qm.DqCase(H, A, 17, 3, 1, False, 2, None, True, 2))
        t, k = _Taken(td, 17, 9), _DoubleQ(dd, H, A, 17)
        assert lib.macjd_qheads_pair(ctypes.byref(t.io), ctypes.byref(k.io), _stream()) == (EINVAL if H == 64 else EUNSUPPORTED)
        torch.cuda.synchronize()
        assert t.nothing_written() and k.nothing_written()


# ---------------------------------------------------------------------------------------------------- parameter gradients
def _wgrad_problems(case, t, gq, w2, outs):
    """(problem one: dW1 / db1 with the outer operand, problem two: dw2 / db2) on the taken launch's x and act."""
    _native, lib = _lib()
    K, N = case.K, H64 + case.A + 1
    one, two = _native.WgradIO(), _native.WgradIO()
    one.K, one.M, one.N = K, H64, N
    one.gout, one.gout_ld, one.inp, one.inp_ld = t.act.ptr, case.act_ld, t.x.ptr, case.x_ld
    one.outer_vec, one.outer_w = gq.ptr, w2.ptr
    one.dW, one.dw_ld, one.db = outs["dW1"].ptr, outs["dW1"].ld, outs["db1"].ptr
    two.K, two.M, two.N = K, 1, H64
    two.gout, two.gout_ld, two.inp, two.inp_ld = gq.ptr, 1, t.act.ptr, case.act_ld
    two.dW, two.dw_ld, two.db = outs["dw2"].ptr, H64, outs["db2"].ptr
    ws = []
    for io in (one, two):
        ws.append(Buf(1, int(lib.macjd_linear_wgrad_workspace_floats(io.K, io.M, io.N))))
        io.workspace = ws[-1].ptr
    return one, two, ws


@pytest.mark.parametrize("case", qm.WGRAD_CASES, ids=lambda c: f"K{c.K}-A{c.A}-x{c.x_ld}-act{c.act_ld}")
def test_qhead_parameter_gradients_match_the_model(case):
    _native, lib = _lib()
    d = qm.wgrad_inputs(case)
    K, A = case.K, case.A
    N = H64 + A + 1
    t = _Taken(d, K, A, 8, 64, 0, case.act_ld, case.x_ld - N)
    assert t.launch() == OK and t.intact()
    x, act, _ = t.got()
    gq, w2 = _In(d["gq"].reshape(K, 1)), _In(d["w2"])
    mk = lambda: dict(dW1=Buf(H64, N, ld=N + case.dw_pad), db1=Buf(1, H64), dw2=Buf(1, H64), db2=Buf(1, 1))
    single, many = mk(), mk()
    one, two, ws1 = _wgrad_problems(case, t, gq, w2, single)
    for io in (one, two):
        _native.check(lib.macjd_linear_wgrad(ctypes.byref(io), _stream()), "macjd_linear_wgrad")
    one, two, ws2 = _wgrad_problems(case, t, gq, w2, many)
    _native.check(lib.macjd_linear_wgrad_many((_native.WgradIO * 2)(one, two), 2, _stream()), "macjd_linear_wgrad_many")
    torch.cuda.synchronize()
    val, mag = qm.qhead_grads(x, act, d["gq"], d["w2"])
    ratios = {}
    for name in ("dW1", "db1", "dw2", "db2"):
        assert single[name].untouched_outside() and many[name].untouched_outside(), f"{name}: margin or row gap written"
        got = single[name].np()
        assert not np.isnan(got).any(), name
        assert torch.equal(single[name].view, many[name].view), f"{name}: macjd_linear_wgrad and macjd_linear_wgrad_many differ"
        err, bound = np.abs(got.reshape(np.shape(val[name])) - val[name]), qm.gamma(K + 2) * mag[name]
        ratios[name] = _ratio(err, bound)
        assert np.all(err <= bound), f"{name} beyond gamma_({K} + 2) sum|terms|: {ratios[name]:.3f} of the bound"
    print(f"{case}: " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + "  (of the bound)")
    assert all(w.untouched_outside() for w in ws1 + ws2), "a workspace margin was written"
    assert float(np.abs(val["dW1"]).max()) > 0 and float(np.abs(val["dw2"]).max()) > 0
