"""The tail of the update chain — ``macjd_td_loss`` / ``macjd_td_mask_sum`` and the four optimiser entry points
``macjd_clip_adam_step`` / ``_sample`` / ``_ln`` / ``_reduced`` (csrc/macjd_nets.hip) — against the float64 model of their
contract (tests/update_tail_model.py, proved against float64 torch in tests/test_update_tail_cpu.py), through the C-ABI, at
the smallest shapes at which these launches can go wrong: vector lengths around the wave, the workgroup and the 65536
elements of one grid-stride pass (plus the learner's own flat length), step counters 0 .. 99999, zero and non-zero
moments, a gradient of zeros, a gradient of the size of eps, clipping off / on / exactly on the boundary, LayerNorm ranges
at the ends of the vector, across index 256, adjacent, and in the second pass, K up to its limit of 1024, C around 256, TD
batches on either side of the 1024 threads of the loss's one workgroup with padded / strided operands.

Every buffer a launch may write is pre-filled with NaN where it is an output, sits between NaN margins and has NaN gaps
where a stride exceeds the row: all must survive, and every written value must be finite.

Tolerances: update_tail_model's — derived bounds for the norm, the TD sums and the elementwise outputs; for the updated
parameters (whose bias correction goes through powf) min(ceiling, 8 Y), at least one float32 ulp of the value.  Each test
prints its worst |got - model| / tolerance per output.  Largest ratios on MI355X over all cases of this file (all must
be <= 1):
    optimiser (all four entry points)   norm 0.189   clipped grad 0.239   m 0.791   v 0.981   param 0.590
    LayerNorm gradients                 dgamma 0.109   dbeta 0.110
    TD loss                             stats 0.169   gy 0.498
(m and v: the bound is the three to five roundings of the expression, and single elements come close to all of them; the
float32 restatement of the model reaches 0.791 / 0.979 of the same bounds on the CPU.)  The file runs in 15 .. 17 s.

macjd_clip_adam_step_ln needs two disjoint ranges, so the length test runs it at every length but 1, with ranges beside
elements 0 and n - 1 and large gradient elements at 0, n - 1 and 65536 as for the other entry points.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import update_tail_model as um  # noqa: E402
from test_nets_cpu import load, make_args, quiet  # noqa: E402
from test_norm_in_reduce_gpu import Buf  # noqa: E402
from tests_golden_helpers import sample_episodes_mirror  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL = 0, -1     # include/macjd.h
SENTINEL = -7777
SEED = 0x1234ABCD5678
f32, f64 = np.float32, np.float64
_WORST = {}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def _ratio(key, got, value, tol):
    """Asserts finite and |got - value| <= tol; -> worst err / tol (0 where both vanish); kept in _WORST[key]."""
    got = np.asarray(got, f64)
    assert np.isfinite(got).all(), key
    err = np.abs(got - value)
    bad = err > tol
    assert not np.any(bad), (key, float(np.max(err - tol)), int(np.argmax(err - tol)))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.max(np.where(tol > 0, err / tol, 0.0)))
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    return r


def _report(prefix):
    print(prefix, {k: round(v, 3) for k, v in sorted(_WORST.items()) if k.startswith(prefix)})


@functools.lru_cache(maxsize=None)
def _learner_length():
    """The learner's own flat vector length at 3j4r_h64, read from a QMixLearner on the device."""
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    g, d = load("3j4r_h64")
    args = make_args(d, device="cuda", use_cuda=True)
    with quiet():
        mac = BasicMAC(d["S"], args)
        learner = QMixLearner(mac, args)
    n = int(learner._flat_param.numel())
    assert n == um.flat_length(p.numel() for p in learner._trainable()) and n > 257
    return n


class _IdxOut:
    """int64 [n] pre-filled with a sentinel between sentinel margins."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((64 + n,), SENTINEL, dtype=torch.int64, device=DEV)
        self.ptr = self.buf.data_ptr() + 32 * 8

    def values(self):
        return self.buf[32:32 + self.n].cpu().tolist()

    def intact(self):
        return bool((self.buf[:32] == SENTINEL).all()) and bool((self.buf[32 + self.n:] == SENTINEL).all())


class _Sampler:
    def __init__(self, _native, n, N, counter, reserved):
        self.idx = _IdxOut(n)
        self.n_stored = torch.tensor([-1, N, -1], dtype=torch.int32, device=DEV)
        self.counter = torch.tensor([-1, counter, -1], dtype=torch.int64, device=DEV)
        self.io = _native.SamplerIO()
        self.io.idx_out, self.io.n, self.io.reserved = self.idx.ptr, n, reserved
        self.io.n_stored, self.io.counter, self.io.seed = self.n_stored[1:].data_ptr(), self.counter[1:].data_ptr(), SEED

    def check(self, n, N, counter, reserved):
        c = counter + reserved
        want = [t % N for t in range(n)] if N < n else sample_episodes_mirror(n, N, c, SEED)
        assert self.idx.values() == want and self.idx.intact()
        assert self.counter.cpu().tolist() == [-1, c + 1, -1] and self.n_stored.cpu().tolist() == [-1, N, -1]
        return want


class _Adam:
    """The buffers of one optimiser call, each between NaN margins; ``partials``: exactly ``n_partials`` floats."""

    def __init__(self, _native, d, n_partials, partial_values=None, step=None):
        n = d["param"].size
        self.n = n
        self.param, self.grad, self.m, self.v = (Buf(1, n, d[k].reshape(1, n)) for k in ("param", "grad", "m", "v"))
        self.step = Buf(1, 1, [[float(d["step"] if step is None else step)]])
        self.norm = Buf(1, 1)
        self.partials = Buf(1, n_partials, None if partial_values is None else np.asarray(partial_values).reshape(1, -1))
        io = _native.AdamIO()
        io.n, io.lr, io.beta1, io.beta2, io.eps, io.max_norm = n, d["lr"], d["b1"], d["b2"], d["eps"], float(d["max_norm"])
        io.param, io.grad, io.exp_avg, io.exp_avg_sq = self.param.ptr, self.grad.ptr, self.m.ptr, self.v.ptr
        io.step, io.grad_norm, io.partials = self.step.ptr, self.norm.ptr, self.partials.ptr
        self.io = io

    def bufs(self):
        return dict(param=self.param, grad=self.grad, m=self.m, v=self.v, step=self.step, norm=self.norm, partials=self.partials)

    def untouched_outside(self):
        return all(b.untouched_outside() for b in self.bufs().values())

    def outputs(self):
        torch.cuda.synchronize()
        return {k: self.bufs()[k].view.clone() for k in ("param", "grad", "m", "v", "step", "norm")}


def _check_adam(tag, a, exp, written_partials):
    """All outputs of an optimiser call against the model's expectation; -> the outputs (torch, for bitwise relations)."""
    out = a.outputs()
    assert a.untouched_outside(), tag
    for k in ("param", "grad", "m", "v"):
        _ratio(f"adam {k}", out[k].cpu().numpy().astype(f64)[0], *exp[k])
    _ratio("adam norm", out["norm"].cpu().numpy().astype(f64)[0], *exp["norm"])
    assert out["step"].item() == exp["step"], tag
    p = a.partials.view[0]
    if written_partials is not None:   # the squared-norm launch wrote its workgroups' partials and nothing behind them
        assert bool(torch.isfinite(p[:written_partials]).all()) and bool(torch.isnan(p[written_partials:]).all()), tag
    return out


def _lengths():
    return um.LENGTHS + ["learner"]


@pytest.mark.parametrize("n", _lengths())
def test_optimiser_entry_points_against_the_model(n):
    """Every state of update_tail_model.STATES at one length, through macjd_clip_adam_step, macjd_clip_adam_step_sample with
    next = NULL (bit for bit the former) and macjd_clip_adam_step_reduced behind host-made partials (which reads the ALREADY
    advanced counter and leaves it alone): parameters, clipped gradient, moments, norm and counter against the model."""
    _native, lib = _lib()
    n = _learner_length() if n == "learner" else n
    nb = um.blocks_of(n)
    with torch.cuda.device(DEV):
        for st in um.STATES:
            d = um.adam_inputs(n, st)
            exp = um.plain_expectation(d)
            a = _Adam(_native, d, 256)
            assert lib.macjd_clip_adam_step(ctypes.byref(a.io), _stream()) == OK
            out = _check_adam((n, st.name, "step"), a, exp, nb)
            b = _Adam(_native, d, 256)
            assert lib.macjd_clip_adam_step_sample(ctypes.byref(b.io), None, _stream()) == OK
            out_b = b.outputs()
            assert b.untouched_outside()
            for k in out:
                assert torch.equal(out[k], out_b[k]), (n, st.name, k)
            parts = um.chunk_partials(d["grad"])
            c = _Adam(_native, d, parts.size, parts, step=d["step"] + 1)
            assert lib.macjd_clip_adam_step_reduced(ctypes.byref(c.io), parts.size, None, _stream()) == OK
            out_c = _check_adam((n, st.name, "reduced"), c, um.reduced_expectation(d, parts), None)
            assert np.array_equal(c.partials.view.cpu().numpy()[0], parts)
            for o in (out, out_c):
                g = o["grad"][0].cpu().numpy()
                if st.grad == "zero":      # norm 0, coefficient clamped to 1: the gradient stays +0, the old momentum moves
                    assert o["norm"].item() == 0.0 and not g.any() and not np.signbit(g).any()
                    assert not torch.equal(o["param"].cpu(), torch.as_tensor(d["param"]).reshape(1, -1))
                if st.clip == "edge":      # exactly representable squared norm: the reported norm is its rounded root
                    assert o["norm"].item() == f32(np.sqrt(float((d["grad"].astype(f64) ** 2).sum())))
                if st.clip == "off":
                    assert np.array_equal(g, d["grad"])
        if n >= 4:     # macjd_clip_adam_step_ln needs two disjoint ranges: every length but 1
            case = um.ln_case_at_length(n)
            dl = um.ln_inputs(case, True)
            e, keep, lio = _ln_call_args(_native, case, dl)
            assert lib.macjd_clip_adam_step_ln(ctypes.byref(e.io), None, ctypes.byref(lio), case.gamma_off, case.beta_off, _stream()) == OK
            _check_adam((n, "ln"), e, um.ln_expectation(case, dl), nb + case.K)
    _report("adam")


@pytest.mark.parametrize("N", [33, 5])
@pytest.mark.parametrize("reserved", [0, 2])
def test_sampler_rides_in_every_entry_point(N, reserved):
    """n = 32 drawn from N = 33 (the permutation) and N = 5 (N < n: t mod N) at counter offsets 0 and 2, inside the last launch
    of _sample, _reduced and _ln: the indices of the host mirror, the counter advanced by 1 + reserved, the same indices from
    every entry point, and the optimiser outputs of _sample(next) bit for bit those of next = NULL."""
    _native, lib = _lib()
    n_draw, c0 = 32, 7
    st = um.STATES[2]
    d = um.adam_inputs(300, st)
    with torch.cuda.device(DEV):
        ref = _Adam(_native, d, 256)
        assert lib.macjd_clip_adam_step_sample(ctypes.byref(ref.io), None, _stream()) == OK
        out_ref = ref.outputs()
        a, sa = _Adam(_native, d, 256), _Sampler(_native, n_draw, N, c0, reserved)
        assert lib.macjd_clip_adam_step_sample(ctypes.byref(a.io), ctypes.byref(sa.io), _stream()) == OK
        out = a.outputs()
        for k in out:
            assert torch.equal(out[k], out_ref[k]), k
        assert a.untouched_outside()
        want = sa.check(n_draw, N, c0, reserved)
        parts = um.chunk_partials(d["grad"])
        b, sb = _Adam(_native, d, parts.size, parts, step=d["step"] + 1), _Sampler(_native, n_draw, N, c0, reserved)
        assert lib.macjd_clip_adam_step_reduced(ctypes.byref(b.io), parts.size, ctypes.byref(sb.io), _stream()) == OK
        b.outputs()
        assert sb.check(n_draw, N, c0, reserved) == want and b.untouched_outside()
        case = um.LN_CASES[3]
        dl = um.ln_inputs(case, True)
        c, keep, lio = _ln_call_args(_native, case, dl)
        sc = _Sampler(_native, n_draw, N, c0, reserved)
        assert lib.macjd_clip_adam_step_ln(ctypes.byref(c.io), ctypes.byref(sc.io), ctypes.byref(lio), case.gamma_off, case.beta_off,
                                           _stream()) == OK
        out_c = c.outputs()
        assert sc.check(n_draw, N, c0, reserved) == want and c.untouched_outside()
        c2, keep2, lio2 = _ln_call_args(_native, case, dl)
        assert lib.macjd_clip_adam_step_ln(ctypes.byref(c2.io), None, ctypes.byref(lio2), case.gamma_off, case.beta_off, _stream()) == OK
        out_c2 = c2.outputs()
        for k in out_c:
            assert torch.equal(out_c[k], out_c2[k]), k
    if N >= n_draw:
        assert len(set(want)) == n_draw and want != list(range(n_draw))


def _ln_call_args(_native, case, d):
    a = _Adam(_native, d, 256 + case.K)
    W = Buf(case.C, case.K, d["W"], ld=case.K + case.w_pad)
    G = Buf(case.C, case.K, d["G"], ld=case.K + case.g_pad)
    gb = Buf(1, case.C, d["gb"].reshape(1, -1))
    lio = _native.LnParamIO()
    lio.C, lio.K, lio.W, lio.w_ld, lio.G, lio.g_ld, lio.gb = case.C, case.K, W.ptr, W.ld, G.ptr, G.ld, gb.ptr
    lio.dgamma, lio.dbeta = a.grad.ptr + 4 * case.gamma_off, a.grad.ptr + 4 * case.beta_off
    return a, (W, G, gb), lio


@pytest.mark.parametrize("clip", [False, True], ids=["coef1", "clipped"])
@pytest.mark.parametrize("case", um.LN_CASES, ids=lambda c: c.name)
def test_layernorm_gradients_inside_the_squared_norm_launch(case, clip):
    """macjd_clip_adam_step_ln with NaN in the two ranges of the gradient vector on entry (the squared-norm workgroups must
    skip them): dgamma / dbeta as stored — recovered at coefficient 1 bit for bit, under clipping as coef x the stand-alone
    macjd_layernorm_param_grad's values within two roundings — and within the model's bound; norm (the LayerNorm gradients
    carry at least a quarter of its square: all blocks + K partials must be summed), parameters, moments, clipped gradient
    against the model; partials: exactly 256 + K floats, blocks + K of them written."""
    _native, lib = _lib()
    d = um.ln_inputs(case, clip)
    exp = um.ln_expectation(case, d)
    K = case.K
    with torch.cuda.device(DEV):
        a, keep, lio = _ln_call_args(_native, case, d)
        alone = _native.LnParamIO()
        ctypes.memmove(ctypes.byref(alone), ctypes.byref(lio), ctypes.sizeof(lio))
        dg, db = Buf(1, K), Buf(1, K)
        alone.dgamma, alone.dbeta = dg.ptr, db.ptr
        assert lib.macjd_layernorm_param_grad(ctypes.byref(alone), _stream()) == OK
        assert lib.macjd_clip_adam_step_ln(ctypes.byref(a.io), None, ctypes.byref(lio), case.gamma_off, case.beta_off, _stream()) == OK
        out = _check_adam((case.name, clip), a, exp, um.blocks_of(case.n) + K)
    assert dg.untouched_outside() and db.untouched_outside() and all(b.untouched_outside() for b in keep)
    dg_a, db_a = dg.np()[0], db.np()[0]
    _ratio("ln dgamma", dg_a, *exp["dgamma"])
    _ratio("ln dbeta", db_a, *exp["dbeta"])
    g = out["grad"][0].cpu().numpy()
    got_g, got_b = g[case.gamma_off:case.gamma_off + K], g[case.beta_off:case.beta_off + K]
    if not clip:
        assert np.array_equal(got_g, dg.view.cpu().numpy()[0]) and np.array_equal(got_b, db.view.cpu().numpy()[0])
    else:
        norm = f32(out["norm"].item())
        coef = f32(d["max_norm"]) / f32(norm + um.CLIP_EPS)
        assert coef < 1
        for got, alone_v in ((got_g, dg_a), (got_b, db_a)):
            assert np.all(np.abs(got.astype(f64) - float(coef) * alone_v) <= 2 * um.U * np.abs(got.astype(f64)))
    _report("adam")
    _report("ln")


def _bytes(values, st, sb, garbage):
    """uint8 [B, Tm1] at element strides (sb, st) inside a tensor of ``garbage`` bytes; -> (tensor, pointer)."""
    B, Tm1 = values.shape
    t = torch.full((64 + B * sb,), garbage, dtype=torch.uint8, device=DEV)
    t[32:32 + B * sb].view(B, sb)[:, 0:(Tm1 - 1) * st + 1:st] = torch.as_tensor(values).to(DEV)
    return t, t.data_ptr() + 32


@pytest.mark.parametrize("mask", um.TD_MASKS)
@pytest.mark.parametrize("B,Tm1", um.TD_SHAPES)
def test_td_loss_and_mask_sum_against_the_model(B, Tm1, mask):
    """macjd_td_loss with gy = NULL (stats[0..2] written, the NaN in stats[3] survives) and with gy rows of Tm1, Tm1 + 1 and
    Tm1 + 5 columns at a pitch above that (tail columns exactly +0, gaps still NaN); macjd_td_mask_sum through the same
    strides equals the count.  Mask "all": contiguous operands (r_st = 1); the others: padded y / tq rows, r_st = 2, strided
    1-byte terminated / filled with true bytes in between."""
    _native, lib = _lib()
    d = um.td_inputs(B, Tm1, mask)
    args = (d["y"], d["tq"], d["reward"], d["terminated"], d["filled"], um.TD_GAMMA)
    e_stats, e_gy = um.td_bounds(*args)
    padded = mask != "all"
    y = Buf(B, Tm1, d["y"], ld=Tm1 + (3 if padded else 0))
    tq = Buf(B, Tm1, d["tq"], ld=Tm1 + (1 if padded else 0))
    r_st = 2 if padded else 1
    rv = np.full((B, r_st * Tm1), np.nan, f32)
    rv[:, ::r_st] = d["reward"]
    reward = Buf(B, r_st * Tm1, rv, ld=r_st * Tm1 + (3 if padded else 0))
    t_st, t_sb = (3, 3 * Tm1 + 2) if padded else (1, Tm1)
    f_st, f_sb = (2, 2 * Tm1 + 5) if padded else (1, Tm1)
    term_t, term_p = _bytes(d["terminated"], t_st, t_sb, 1)
    fill_t, fill_p = _bytes(d["filled"], f_st, f_sb, 1)
    frozen = [b.raw.clone() for b in (y, tq, reward)] + [term_t.clone(), fill_t.clone()]

    def io_for(stats, gy, gy_cols):
        io = _native.TdLossIO()
        io.B, io.Tm1, io.gamma = B, Tm1, um.TD_GAMMA
        io.y, io.tq, io.y_sb, io.tq_sb = y.ptr, tq.ptr, y.ld, tq.ld
        io.reward, io.r_sb, io.r_st = reward.ptr, reward.ld, r_st
        io.terminated, io.t_sb, io.t_st, io.filled, io.f_sb, io.f_st = term_p, t_sb, t_st, fill_p, f_sb, f_st
        io.stats = stats.ptr
        if gy is not None:
            io.gy, io.gy_sb, io.gy_cols = gy.ptr, gy.ld, gy_cols
        return io

    with torch.cuda.device(DEV):
        stats0 = Buf(1, 4)
        assert lib.macjd_td_loss(ctypes.byref(io_for(stats0, None, 0)), _stream()) == OK
        out = Buf(1, 1)
        assert lib.macjd_td_mask_sum(ctypes.byref(io_for(stats0, None, 0)), out.ptr, _stream()) == OK
        runs = []
        for extra in um.GY_EXTRA:
            stats, gy = Buf(1, 4), Buf(B, Tm1 + extra, ld=Tm1 + extra + 2)
            assert lib.macjd_td_loss(ctypes.byref(io_for(stats, gy, Tm1 + extra)), _stream()) == OK
            runs.append((extra, stats, gy))
    torch.cuda.synchronize()
    count = float(d["filled"].sum())
    model_stats, _ = um.td_loss_model(*args)
    s0 = stats0.view.cpu().numpy()[0]
    assert np.isnan(s0[3]) and stats0.untouched_outside()
    _ratio("td stats", s0[:3], model_stats[:3], e_stats[:3])
    assert out.view.item() == count and out.untouched_outside()
    for extra, stats, gy in runs:
        m_stats, m_gy = um.td_loss_model(*args, gy_cols=Tm1 + extra)
        s = stats.view.cpu().numpy()[0]
        _ratio("td stats", s, m_stats, e_stats)
        assert s[3] == count and np.array_equal(s[:3], s0[:3])
        got = gy.view.cpu().numpy()
        _ratio("td gy", got[:, :Tm1], m_gy[:, :Tm1], e_gy)
        tail = got[:, Tm1:]
        assert not tail.any() and not np.signbit(tail).any()
        assert not got[:, :Tm1][d["filled"] == 0].any()
        assert stats.untouched_outside() and gy.untouched_outside()
    for b, was in zip((y.raw, tq.raw, reward.raw, term_t, fill_t), frozen):   # the inputs are inputs
        assert torch.equal(b.view(torch.uint8), was.view(torch.uint8))
    _report("td")


def _snapshot(bufs):
    return [b.clone().view(torch.uint8) for b in bufs]


def test_argument_errors_are_refused_before_any_launch():
    """Every rule the entry points check before their first launch: MACJD_EINVAL, and not a byte of any buffer changes
    (overlapping LayerNorm ranges included: different workgroups would store to the same elements in no defined order)."""
    _native, lib = _lib()
    case = um.LnCase("err", 300, 46, 5, 0, 0, 10, 100)
    d = dict(um.adam_inputs(300, um.STATES[2]))
    rng = np.random.default_rng(3)
    d.update(W=rng.standard_normal((5, 46)).astype(f32), G=rng.standard_normal((5, 46)).astype(f32), gb=rng.standard_normal(5).astype(f32))
    td = um.td_inputs(3, 2, "ragged")
    with torch.cuda.device(DEV):
        a, keep, lio = _ln_call_args(_native, case, d)
        sp = _Sampler(_native, 4, 9, 7, 0)
        y, tq, rew, stats, gy, out = Buf(3, 2, td["y"]), Buf(3, 2, td["tq"]), Buf(3, 2, td["reward"]), Buf(1, 4), Buf(3, 2), Buf(1, 1)
        term = torch.as_tensor(td["terminated"]).to(DEV)
        fill = torch.as_tensor(td["filled"]).to(DEV)
        everything = [b.raw for b in a.bufs().values()] + [b.raw for b in keep] + [sp.idx.buf, sp.n_stored, sp.counter] + \
                     [b.raw for b in (y, tq, rew, stats, gy, out)] + [term, fill]
        before = _snapshot(everything)
        s = _stream()
        calls = []

        def adam_with(**kw):
            io = _native.AdamIO()
            ctypes.memmove(ctypes.byref(io), ctypes.byref(a.io), ctypes.sizeof(io))
            for k, v in kw.items():
                setattr(io, k, v)
            return io

        def sampler_with(**kw):
            io = _native.SamplerIO()
            ctypes.memmove(ctypes.byref(io), ctypes.byref(sp.io), ctypes.sizeof(io))
            for k, v in kw.items():
                setattr(io, k, v)
            return io

        def ln_with(**kw):
            io = _native.LnParamIO()
            ctypes.memmove(ctypes.byref(io), ctypes.byref(lio), ctypes.sizeof(io))
            for k, v in kw.items():
                setattr(io, k, v)
            return io

        g0, b0 = case.gamma_off, case.beta_off
        bad_adam = [("n=0", dict(n=0)), ("n<0", dict(n=-5))] + \
                   [(f"{k}=NULL", {k: None}) for k in ("param", "grad", "exp_avg", "exp_avg_sq", "step", "grad_norm", "partials")]
        for name, kw in bad_adam:
            io = adam_with(**kw)
            calls += [(f"step {name}", lambda io=io: lib.macjd_clip_adam_step(ctypes.byref(io), s)),
                      (f"sample {name}", lambda io=io: lib.macjd_clip_adam_step_sample(ctypes.byref(io), ctypes.byref(sp.io), s)),
                      (f"reduced {name}", lambda io=io: lib.macjd_clip_adam_step_reduced(ctypes.byref(io), 4, ctypes.byref(sp.io), s)),
                      (f"ln {name}", lambda io=io: lib.macjd_clip_adam_step_ln(ctypes.byref(io), None, ctypes.byref(lio), g0, b0, s))]
        calls += [("step io=NULL", lambda: lib.macjd_clip_adam_step(None, s)),
                  ("sample io=NULL", lambda: lib.macjd_clip_adam_step_sample(None, None, s)),
                  ("reduced io=NULL", lambda: lib.macjd_clip_adam_step_reduced(None, 4, None, s)),
                  ("ln io=NULL", lambda: lib.macjd_clip_adam_step_ln(None, None, ctypes.byref(lio), g0, b0, s)),
                  ("ln ln=NULL", lambda: lib.macjd_clip_adam_step_ln(ctypes.byref(a.io), None, None, g0, b0, s))]
        for np_ in (0, -1):
            calls.append((f"reduced n_partials={np_}", lambda np_=np_: lib.macjd_clip_adam_step_reduced(ctypes.byref(a.io), np_, None, s)))
        for name, kw in [("idx_out=NULL", dict(idx_out=None)), ("n=0", dict(n=0)), ("n_stored=NULL", dict(n_stored=None)),
                         ("counter=NULL", dict(counter=None)), ("reserved<0", dict(reserved=-1))]:
            bad = sampler_with(**kw)
            calls += [(f"sample sampler {name}", lambda bad=bad: lib.macjd_clip_adam_step_sample(ctypes.byref(a.io), ctypes.byref(bad), s)),
                      (f"reduced sampler {name}", lambda bad=bad: lib.macjd_clip_adam_step_reduced(ctypes.byref(a.io), 4, ctypes.byref(bad), s)),
                      (f"ln sampler {name}", lambda bad=bad: lib.macjd_clip_adam_step_ln(ctypes.byref(a.io), ctypes.byref(bad), ctypes.byref(lio), g0, b0, s)),
                      (f"draw sampler {name}", lambda bad=bad: lib.macjd_sample_episodes(ctypes.byref(bad), s))]
        gp = a.grad.ptr
        for name, kw, go, bo in [("C=0", dict(C=0), g0, b0), ("K=0", dict(K=0), g0, b0), ("K=1025", dict(K=1025, w_ld=1025, g_ld=1025), g0, b0),
                                 ("W=NULL", dict(W=None), g0, b0), ("G=NULL", dict(G=None), g0, b0), ("gb=NULL", dict(gb=None), g0, b0),
                                 ("w_ld<K", dict(w_ld=45), g0, b0), ("g_ld<K", dict(g_ld=45), g0, b0),
                                 ("gamma_off<0", dict(dgamma=gp - 4), -1, b0), ("beta_off<0", dict(dbeta=gp - 4), g0, -1),
                                 ("gamma_off+K>n", dict(dgamma=gp + 4 * 255), 255, b0), ("beta_off+K>n", dict(dbeta=gp + 4 * 255), g0, 255),
                                 ("dgamma elsewhere", dict(dgamma=gp + 4 * (g0 + 1)), g0, b0), ("dbeta elsewhere", dict(dbeta=gp + 4 * (b0 + 1)), g0, b0),
                                 ("dgamma=NULL", dict(dgamma=None), g0, b0), ("dbeta=NULL", dict(dbeta=None), g0, b0),
                                 ("ranges equal", dict(dbeta=gp + 4 * g0), g0, g0),
                                 ("beta inside gamma", dict(dbeta=gp + 4 * (g0 + 45)), g0, g0 + 45),
                                 ("gamma inside beta", dict(dgamma=gp + 4 * (b0 + 1)), b0 + 1, b0)]:
            bad = ln_with(**kw)
            calls.append((f"ln {name}", lambda bad=bad, go=go, bo=bo: lib.macjd_clip_adam_step_ln(ctypes.byref(a.io), None, ctypes.byref(bad), go, bo, s)))

        def td_with(**kw):
            io = _native.TdLossIO()
            io.B, io.Tm1, io.gamma = 3, 2, um.TD_GAMMA
            io.y, io.tq, io.y_sb, io.tq_sb, io.reward, io.r_sb, io.r_st = y.ptr, tq.ptr, 2, 2, rew.ptr, 2, 1
            io.terminated, io.t_sb, io.t_st, io.filled, io.f_sb, io.f_st = term.data_ptr(), 2, 1, fill.data_ptr(), 2, 1
            io.stats, io.gy, io.gy_sb, io.gy_cols = stats.ptr, gy.ptr, 2, 2
            for k, v in kw.items():
                setattr(io, k, v)
            return io

        for name, kw in [("B=0", dict(B=0)), ("Tm1=0", dict(Tm1=0))] + [(f"{k}=NULL", {k: None}) for k in ("y", "tq", "reward", "terminated", "filled", "stats")] + \
                        [("y_sb<Tm1", dict(y_sb=1)), ("tq_sb<Tm1", dict(tq_sb=1)), ("gy_cols<Tm1", dict(gy_cols=1)), ("gy_sb<gy_cols", dict(gy_cols=3, gy_sb=2))]:
            bad = td_with(**kw)
            calls.append((f"td_loss {name}", lambda bad=bad: lib.macjd_td_loss(ctypes.byref(bad), s)))
        calls.append(("td_loss io=NULL", lambda: lib.macjd_td_loss(None, s)))
        for name, kw in [("B=0", dict(B=0)), ("Tm1=0", dict(Tm1=0)), ("filled=NULL", dict(filled=None))]:
            bad = td_with(**kw)
            calls.append((f"mask_sum {name}", lambda bad=bad: lib.macjd_td_mask_sum(ctypes.byref(bad), out.ptr, s)))
        ok_td = td_with()
        calls += [("mask_sum out=NULL", lambda: lib.macjd_td_mask_sum(ctypes.byref(ok_td), None, s)),
                  ("mask_sum io=NULL", lambda: lib.macjd_td_mask_sum(None, out.ptr, s))]
        for name, call in calls:
            assert call() == EINVAL, name
        torch.cuda.synchronize()
        for i, (buf, was) in enumerate(zip(everything, before)):
            assert torch.equal(buf.view(torch.uint8), was), i
        # and the unchanged arguments are accepted (adjacent ranges: beta_off = gamma_off + K)
        adj = ln_with(dbeta=gp + 4 * (g0 + 46))
        assert lib.macjd_clip_adam_step_ln(ctypes.byref(a.io), None, ctypes.byref(adj), g0, g0 + 46, s) == OK
        assert lib.macjd_td_loss(ctypes.byref(ok_td), s) == OK
        torch.cuda.synchronize()
