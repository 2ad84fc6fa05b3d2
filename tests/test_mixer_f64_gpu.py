"""The exact-f32 fused mixer launches (``macjd_mixerf_io.operand_dtype = 0``, csrc/macjd_mixer.hip) against the float64
model of their contract (tests/mixer_f64_model.py, proved against the reference's fixtures and float64 autograd in
tests/test_mixer_f64_cpu.py), through the C-ABI, at the smallest shapes at which these kernels can go wrong: every J,
M around the 16-row tile, S from 1 to 16 J, a strided state, parameters at odd float offsets of one flat vector,
degenerate LayerNorm rows, the in-kernel TD gradient with episode ends and the batch end at chosen places of a tile,
and the module path down to the weight / LayerNorm-parameter gradients.

Every output is pre-filled with NaN and sits between two margins of NaN that must survive the launch; every input sits
between NaN margins too, so a read past an input shows up in the result instead of depending on the allocator.

Mask decisions.  Gradients jump at a ReLU / clamp threshold.  Where the float64 pre-activation lies within the model's
band of a threshold the side is taken from the kernel's own outputs (``act > 0``; clamps: the gradient element is zero
or not, where the unmasked gradient is non-zero — elsewhere the side has no effect); everywhere else the float64 side
is binding, and the kernel's side must agree with it.  Decisions taken from the kernel are counted and held to the
0.5 % cap that tests/test_mixer_f64_cpu.py asserts from the model alone.

Tolerances.  y: the project's bar, atol 1e-5 max(1, max|ref|), rtol 1e-5.  Every other tensor: rtol 1e-4 and
atol = ATOL[name] x max|ref|.  ATOL is the smaller of the ceiling 3e-5, which test_bf16_kernels_match_the_contract derives
for f32 accumulation of up to 768 terms, and 4 x the worst deviation recorded in MEASURED over the whole parametrisation,
rounded up to one digit (rounding sums: ~sqrt(K) typical against K worst, hence the margin).  Each test prints its worst
|got - ref| / max|ref| per tensor.  Measured on MI355X over all cases (MEASURED) and the resulting atol factors:
    sn 1.84e-7 -> 8e-7    xhat 2.03e-7 -> 9e-7    act 6.79e-7 -> 3e-6    gq 8.42e-7 -> 4e-6    gout1 1.38e-6 -> 6e-6
    g_w1raw 2.26e-6 -> 1e-5    g_wfraw 7.49e-7 -> 3e-6    g_v 4.19e-7 -> 2e-6    parameter gradients 1.55e-6 -> 7e-6
(worst cases: J = 12 and J = 6, the longest sums); y and the target values deviate by at most 4.3e-7 / 8.0e-7 of
max(1, max|ref|) against their 1e-5 bar.  Every factor is below the 3e-5 ceiling."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO  # noqa: F401

sys.path.insert(0, os.path.dirname(__file__))
import mixer_f64_model as mm  # noqa: E402
from test_nets_cpu import load, make_args  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HH, EM, N1, NRELU = mm.HH, mm.EM, mm.N1, mm.NRELU
OUT_MARGIN, IN_MARGIN = 64, 256     # floats of NaN on either side (IN_MARGIN > 16 J: the widest first-layer fragment row)
CEILING = 3e-5
# worst |got - ref| / max|ref| on MI355X over all cases of this file, per tensor ("wgrad": the parameter gradients)
MEASURED = {"sn": 1.84e-7, "xhat": 2.03e-7, "act": 6.79e-7, "gq": 8.42e-7, "gout1": 1.38e-6, "g_w1raw": 2.26e-6,
            "g_wfraw": 7.49e-7, "g_v": 4.19e-7, "wgrad": 1.55e-6}
_TENSORS = ("sn", "xhat", "act", "gq", "gout1", "g_w1raw", "g_wfraw", "g_v", "wgrad")


def _one_digit_up(x):
    e = 10.0 ** np.floor(np.log10(x))
    return float(np.ceil(x / e - 1e-9) * e)


ATOL = {k: min(CEILING, _one_digit_up(4.0 * MEASURED[k])) if MEASURED.get(k, 0) > 0 else CEILING for k in _TENSORS}
BACKWARD = ("gq", "gout1", "g_w1raw", "g_wfraw", "g_v")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


class _Guarded:
    """A float32 tensor inside a larger allocation, NaN margins on both sides (margins are multiples of 4 floats, so
    the view keeps the allocation's 16-byte alignment)."""

    def __init__(self, shape, margin, data=None, offset=0):
        n = int(np.prod(shape))
        self.buf = torch.full((margin + offset + n + margin,), float("nan"), dtype=torch.float32, device=DEV)
        self.lo, self.hi = margin + offset, margin + offset + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if data is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(data), dtype=torch.float32))

    def margins_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi:]).all())


def _inp(a, offset=0):
    g = _Guarded(a.shape, IN_MARGIN, data=a, offset=offset)
    return g.t, g


def _device_params(p, layout="plain"):
    """The parameter dict of ops._mixerf_io on the device.  "flat": views at odd float offsets of ONE vector (NaN between
    them), as in a flat parameter vector; otherwise one guarded allocation each."""
    keep, out = [], {"eps": p["eps"], "bf16": False}
    if layout == "flat":
        sizes = [int(np.prod(p[k].shape)) for k in mm.PARAMS]
        flat = torch.full((IN_MARGIN + sum(sizes) + 4 * len(sizes) + IN_MARGIN,), float("nan"), dtype=torch.float32, device=DEV)
        off = IN_MARGIN + 1
        for k, n in zip(mm.PARAMS, sizes):
            off += 1 - (off & 1)                          # odd offset
            out[k] = flat[off:off + n].view(*p[k].shape)
            out[k].copy_(torch.as_tensor(p[k]))
            assert (out[k].data_ptr() // 4) & 1
            off += n + 1
        keep.append(flat)
    else:
        for k in mm.PARAMS:
            out[k], g = _inp(p[k])
            keep.append(g)
    out["_keep"] = keep
    return out


def _outputs(M, J, S, names):
    shapes = {"y": (M,), "tq": (M,), "sn": (M, S), "xhat": (M, S), "act": (M, N1), "gq": (M, J), "gout1": (M, N1),
              "g_w1raw": (M, J * EM), "g_wfraw": (M, EM), "g_v": (M,)}
    return {k: _Guarded(shapes[k], OUT_MARGIN) for k in names}


def _finish(out):
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.margins_intact(), f"{k}: a NaN margin was written"
    return {k: g.t for k, g in out.items()}


def _fwd_bwd(p, q, s, gy):
    """Saving forward + backward through the C-ABI at operand_dtype = 0 (as _fwd_bwd of test_mixer_bf16_gpu.py)."""
    from macjd_amd import _native, ops
    lib = _native.load()
    M, J = q.shape
    S = s.shape[1]
    out = _outputs(M, J, S, mm.OUTPUTS)
    io = ops._mixerf_io(q, s, p)
    assert io.S == S and io.s_ld == s.stride(0)
    io.operand_dtype, io.save = 0, 1
    for k in ("y", "sn", "xhat", "act"):
        setattr(io, k, out[k].t.data_ptr())
    _native.check(lib.macjd_mixer_fused_forward(ctypes.byref(io), _stream()), "macjd_mixer_fused_forward")
    bio = ops._mixerf_io(q, None, p)
    bio.operand_dtype = 0
    bio.act, bio.gy = out["act"].t.data_ptr(), gy.data_ptr()
    for k in BACKWARD:
        setattr(bio, k, out[k].t.data_ptr())
    _native.check(lib.macjd_mixer_fused_backward(ctypes.byref(bio), _stream()), "macjd_mixer_fused_backward")
    return _finish(out)


def _update(kind, pe, pt, q_e, q_t, state, reward, terminated, filled, tot_m, stats=None, tq=None):
    """One update's mixer launches through the C-ABI at operand_dtype = 0 (as _update of test_mixer_bf16_gpu.py):
    "single" = saving forward + plain forward + backward_td (with ``stats``), "pair" = forward_pair + backward_td,
    "train" = the one-launch form.  ``tq`` [B, T1] given ("single" only): the target values, no target mixer runs."""
    from macjd_amd import _native, ops
    lib = _native.load()
    B, T1, J = q_e.shape
    M, S = B * T1, state.shape[-1]
    qe, s = q_e.view(M, J), state.view(M, S)
    out = _outputs(M, J, S, mm.OUTPUTS + (("tq",) if tq is None else ()))
    tq_ptr = out["tq"].t.data_ptr() if tq is None else tq.data_ptr()
    io = ops._mixerf_io(qe, s, pe)
    io.save, io.operand_dtype = 1, 0
    for k in mm.OUTPUTS:
        setattr(io, k, out[k].t.data_ptr())
    if tq is None:
        tio = ops._mixerf_io(q_t.view(M, J), s, pt)
        tio.y, tio.operand_dtype = tq_ptr, 0
    else:
        assert kind == "single" and tq.is_contiguous() and tq.numel() == M
    td = _native.TdLossIO()
    td.B, td.Tm1, td.gamma = B, T1 - 1, mm.GAMMA
    td.y, td.y_sb = out["y"].t.data_ptr(), T1
    td.tq, td.tq_sb = tq_ptr + 4, T1
    td.gy, td.gy_sb, td.gy_cols = None, T1, T1
    td.reward, td.r_sb, td.r_st = reward.data_ptr(), reward.stride(0), reward.stride(1)
    td.terminated, td.t_sb, td.t_st = terminated.data_ptr(), terminated.stride(0), terminated.stride(1)
    td.filled, td.f_sb, td.f_st = filled.data_ptr(), filled.stride(0), filled.stride(1)
    st = _stream()
    if kind == "train":
        _native.check(lib.macjd_mixer_fused_train(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(), st),
                      "macjd_mixer_fused_train")
    else:
        if stats is not None:
            td.stats = stats.data_ptr()
        if kind == "pair":
            _native.check(lib.macjd_mixer_fused_forward_pair(ctypes.byref(io), ctypes.byref(tio), st), "macjd_mixer_fused_forward_pair")
        else:
            _native.check(lib.macjd_mixer_fused_forward(ctypes.byref(io), st), "macjd_mixer_fused_forward")
            if tq is None:
                _native.check(lib.macjd_mixer_fused_forward(ctypes.byref(tio), st), "macjd_mixer_fused_forward")
        _native.check(lib.macjd_mixer_fused_backward_td(ctypes.byref(io), ctypes.byref(td), tot_m.data_ptr(), st),
                      "macjd_mixer_fused_backward_td")
    return _finish(out)


def _kernel_decisions(first, got):
    """The sides the kernel took, read from its outputs, merged with the model's first pass: -> (decisions for the
    second pass, number of decisions taken from the kernel).  Asserts that outside the band the kernel's side is the
    float64 side wherever it can be read."""
    M = got["act"].shape[0]
    c = lambda t: t.detach().cpu()
    for k, g in got.items():
        if k != "tq":                                  # (the training launch leaves row 0 of the target values alone)
            assert not bool(torch.isnan(g).any()), f"{k} has NaN (an unwritten element, or NaN read from an input's margin)"
    ksides = {"relu": c(got["act"])[:, :NRELU] > 0,
              "w1_raw": c(got["g_w1raw"]).view(M, -1, EM) != 0, "wf_raw": c(got["g_wfraw"]) != 0,
              "v_raw": c(got["g_v"]) != 0, "b1_raw": c(got["gout1"])[:, NRELU:] != 0}
    decisions, taken = {}, 0
    for name in mm.DECISIONS:
        side, near = first["side"][name], first["near"][name]
        readable = first["readable"][name]
        kside = torch.where(readable, ksides[name], side)
        wrong = (kside != side) & ~near
        assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} decisions outside the band differ from float64"
        decisions[name] = kside
        taken += int((near & readable).sum())
    assert taken <= mm.CAP * first["n_decisions"], (taken, first["n_decisions"])
    assert first["n_blind"] == 0     # (every near-threshold side that matters shows in the outputs; asserted on the CPU too)
    return decisions, taken


def _compare(got, ref, names, what, atol_key=None):
    """Every tensor of ``names`` against the model at the bars of the module docstring; prints the worst deviations."""
    worst, bad = {}, []
    for k in names:
        r = ref[k]
        g = got[k].detach().cpu().double().reshape(r.shape)
        assert not bool(torch.isnan(g).any()), f"{what}: {k} has NaN (an unwritten element, or NaN read from a margin)"
        top = float(r.abs().max()) if r.numel() else 0.0
        err = float((g - r).abs().max()) if r.numel() else 0.0
        worst[k] = err / top if top > 0 else err
        if k == "y" or k == "tq":
            ok = np.allclose(g.numpy(), r.numpy(), rtol=1e-5, atol=1e-5 * max(1.0, top))
        else:
            ok = np.allclose(g.numpy(), r.numpy(), rtol=1e-4, atol=ATOL[atol_key or k] * top)
        if not ok:
            bad.append(k)
    print(f"{what}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert not bad, f"{what}: {bad} beyond the bar; worst |got - ref| / max|ref|: {worst}"
    return worst


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.mark.parametrize("J", mm.JS)
def test_forward_backward_match_the_model(J):
    """(a) y, sn, xhat, act, gq, gout1, g_w1raw, g_wfraw, g_v of the forward + backward launches: M in {1, 15, 16, 17,
    33}, S in {1, 5, 16 J - 1, 16 J, shipped}, once a state with s_ld > S, once all parameters at odd float offsets."""
    cases = [c for c in mm.fwd_bwd_cases() if c[0] == J]
    assert len(cases) == 27
    taken_all = 0
    for case in cases:
        _, S, M, layout = case
        p, q, s, gy = mm.fwd_bwd_inputs(*case)
        dp = _device_params(p, layout)
        dq, gq_ = _inp(q)
        dgy, ggy = _inp(gy)
        if layout == "s_ld":
            wide = np.full((M, S + 7), np.nan, dtype=np.float32)
            wide[:, 3:3 + S] = s
            dwide, gs = _inp(wide)
            ds = dwide[:, 3:3 + S]
            assert ds.stride(0) == S + 7
        else:
            ds, gs = _inp(s)
        got = _fwd_bwd(dp, dq, ds, dgy)
        first = mm.forward_backward(p, q, s, gy)
        decisions, taken = _kernel_decisions(first, got)
        taken_all += taken
        ref = mm.forward_backward(p, q, s, gy, decisions)
        _compare(got, ref, mm.OUTPUTS, f"fwd_bwd J={J} S={S} M={M} {layout}")
    print(f"J={J}: {taken_all} decisions taken from the kernel")


@pytest.mark.parametrize("J", mm.JS)
def test_degenerate_layernorm_rows(J):
    """(b) All-zero state rows (row T of a closed-loop stage buffer: variance 0, rstd = 1 / sqrt(eps)) and rows of one
    constant small integer: xhat is exactly 0 and sn equals ln_b bit for bit there, the rest of the chain matches the
    model; with S = 1 every row is such a row."""
    for S in (mm.SHIPPED_S[J], 1):
        p, q, s, gy, rows = mm.degenerate_inputs(J, S)
        dp = _device_params(p)
        (dq, k0), (ds, k1), (dgy, k2) = _inp(q), _inp(s), _inp(gy)
        got = _fwd_bwd(dp, dq, ds, dgy)
        rows = list(range(q.shape[0])) if S == 1 else rows
        xh, sn = got["xhat"].cpu()[rows], got["sn"].cpu()[rows]
        assert bool((xh == 0).all()), "xhat of a constant row is not exactly 0"
        assert torch.equal(sn, torch.as_tensor(p["ln_b"]).expand_as(sn)), "sn of a constant row is not ln_b bit for bit"
        first = mm.forward_backward(p, q, s, gy)
        decisions, _ = _kernel_decisions(first, got)
        _compare(got, mm.forward_backward(p, q, s, gy, decisions), mm.OUTPUTS, f"degenerate J={J} S={S}")


def _td_case(J, B, T1, S):
    pe, pt, q_e, q_t, state, reward, terminated, filled = mm.td_inputs(J, B, T1, S=S)
    dev = {"pe": _device_params(pe), "pt": _device_params(pt)}
    dev["q_e"], dev["k0"] = _inp(q_e)
    dev["q_t"], dev["k1"] = _inp(q_t)
    dev["state"], dev["k2"] = _inp(state)
    # [:, :-1] views of [B, T1, 1] tensors: batch strides T1, not T1 - 1
    dev["reward"] = _dev(reward)[:, :-1]
    dev["terminated"] = _dev(terminated, torch.bool)[:, :-1]
    dev["filled"] = _dev(filled, torch.bool)[:, :-1]
    assert dev["reward"].stride(0) == T1 and dev["filled"].stride(0) == T1
    return (pe, pt, q_e, q_t, state, reward, terminated, filled), dev


@pytest.mark.parametrize("J", mm.JS)
def test_in_kernel_td_gradient(J):
    """(c) macjd_mixer_fused_backward_td (every J; with td->stats; behind two single forwards and behind
    macjd_mixer_fused_forward_pair) and macjd_mixer_fused_train (J in {2, 3}) against the
    model run on the eval and the target parameter sets, the loss's formula and the model's backward: (B, T1) chosen so
    that episode ends fall on, before and after tile edges and the batch ends mid-tile; rows with t = T1 - 1 or
    filled = 0 hold exact zeros in every gradient; stats[0..2] at rel 1e-5, stats[3] untouched.  One batch runs at S = 5: the
    narrow-row variants of the pair and training kernels."""
    from macjd_amd import ops
    for B, T1, S in mm.td_cases(J):
        host, dev = _td_case(J, B, T1, S)
        pe, pt, q_e, q_t, state, reward, terminated, filled = host
        tot_m = ops.td_mask_sum(dev["filled"], T1 - 1)
        assert float(tot_m) == float(filled[:, :-1].sum()) > 0
        tq_ref = mm.target_values(pt, q_t, state)
        first, _ = mm.td_reference(pe, q_e, state, tq_ref, reward, terminated, filled, mm.GAMMA)
        dead = torch.as_tensor(~filled.reshape(B, T1))
        dead[:, -1] = True
        dead = dead.reshape(-1)
        for kind in ("single", "pair", "train") if J in (2, 3) else ("single", "pair"):
            stats = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV) if kind == "single" else None
            got = _update(kind, dev["pe"], dev["pt"], dev["q_e"], dev["q_t"], dev["state"], dev["reward"],
                          dev["terminated"], dev["filled"], tot_m, stats)
            decisions, _ = _kernel_decisions(first, got)
            ref, (loss, mean_y, mean_t) = mm.td_reference(pe, q_e, state, tq_ref, reward, terminated, filled, mm.GAMMA, decisions)
            what = f"td {kind} J={J} B={B} T1={T1} S={S}"
            _compare(got, ref, mm.OUTPUTS, what)
            # the target mixer's values: row 0 is no loss row's target, the training launch does not write it
            _compare({"tq": got["tq"][1:]}, {"tq": tq_ref.reshape(-1)[1:]}, ("tq",), what)
            for k in BACKWARD:
                g = got[k].cpu().reshape(B * T1, -1)[dead]
                assert bool((g == 0).all()), f"{what}: {k} is not exactly zero on a row without loss"
            if stats is not None:
                st = stats.cpu()
                for i, v in enumerate((loss, mean_y, mean_t)):
                    assert float(st[i]) == pytest.approx(float(v), rel=1e-5), (what, "stats", i)
                assert bool(torch.isnan(st[3])), "stats[3] was written"


@pytest.mark.parametrize("tag", ["2j2r_h128", "3j4r_h64", "6j8r_h64", "12j16r_h64"])
def test_module_gradients_match_the_model(tag):
    """(d) QMixer on the GPU (x3 weights), ``me(q, state)``, ``ops.td_grad_in_mixer_backward`` and ``backward`` inside
    ``ops.deferred_wgrad()``: q.grad and the gradient of every named parameter — LayerNorm weight and bias included —
    against the model, i.e. macjd_linear_wgrad_many and macjd_layernorm_param_grad fed by the fused launch's outputs."""
    from macjd_amd import ops
    from macjd_amd.core.networks import QMixer
    g, d = load(tag)
    J = d["J"]
    args = make_args(d, device="cuda", use_cuda=True)
    me = mm.x3_mixer(QMixer, args).to(DEV)
    B, T1 = mm.MODULE_BATCH
    q, tq, state, reward, terminated, filled = mm.module_inputs(J)
    p = mm.params_from_state_dict(me.state_dict(), me.state_norm.eps)
    dq, dtq, dstate = _dev(q).requires_grad_(True), _dev(tq), _dev(state)
    drew = _dev(reward)[:, :-1]
    dterm, dfill = _dev(terminated, torch.bool)[:, :-1], _dev(filled, torch.bool)[:, :-1]
    tot_m = ops.td_mask_sum(dfill, T1 - 1)
    assert me.fused_available(dq)
    y = me(dq, dstate)
    assert type(y.grad_fn).__name__ != "NoneType" and ops.fused_mixer_backward_will_run(y)
    placeholder = ops.td_grad_in_mixer_backward(y, dtq, drew, dterm, dfill, mm.GAMMA, T1 - 1, 1, tot_m)
    with ops.deferred_wgrad():
        y.backward(placeholder)
    torch.cuda.synchronize()
    # the sides this launch took: the same kernel through the C-ABI on the same inputs (bit-identical outputs)
    first, _ = mm.td_reference(p, q, state, tq, reward, terminated, filled, mm.GAMMA)
    ln, (w_cat, b_cat) = me.state_norm, me._first_layer_cat()
    dp = ops._mixerf_params(ln.weight, ln.bias, ln.eps, w_cat, b_cat, me.hyper_w_1[2].weight, me.hyper_w_1[2].bias,
                            me.hyper_w_final[2].weight, me.hyper_w_final[2].bias, me.V[2].weight, me.V[2].bias)
    M = B * T1
    got = _update("single", dp, None, dq.detach(), None, dstate, drew, dterm, dfill, tot_m, tq=dtq)
    assert torch.equal(got["y"], y.detach().reshape(M)) and torch.equal(got["gq"], dq.grad.reshape(M, J))
    decisions, _ = _kernel_decisions(first, got)
    ref, _ = mm.td_reference(p, q, state, tq, reward, terminated, filled, mm.GAMMA, decisions)
    _compare(got, ref, mm.OUTPUTS, f"module {tag} (launch)")
    want = mm.state_dict_grads(ref["grads"], d["S"])
    grads = {n: p_.grad for n, p_ in me.named_parameters()}
    assert sorted(grads) == sorted(want) and all(v is not None for v in grads.values())
    _compare(grads, want, sorted(want), f"module {tag} (parameters)", atol_key="wgrad")
    assert float(want["state_norm.weight"].abs().max()) > 0 and float(want["state_norm.bias"].abs().max()) > 0


_NXT = lambda x, to: np.nextafter(np.float32(x), np.float32(to))
# column -> exact pre-activation: on a bound (the gradient passes) or one float32 step outside it (blocked)
_W1_COLS = {0: 0.0, 1: 5.0, 2: _NXT(0.0, -1.0), 3: _NXT(5.0, 6.0)}
_WF_COLS = {4: 0.0, 5: 5.0, 6: _NXT(0.0, -1.0), 7: _NXT(5.0, 6.0)}
_B1_COLS = {8: -5.0, 9: 5.0, 10: _NXT(-5.0, -6.0), 11: _NXT(5.0, 6.0)}
_V_VALUES = (5.0, -5.0, _NXT(5.0, 6.0), _NXT(-5.0, -6.0))


def _bound_params(p, J, v_raw):
    """Zero weight rows with a bias of exactly the wanted value: 0 + bias is exact in float32 as in float64."""
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    for c, v in _W1_COLS.items():
        p["W2"][(J - 1) * EM + c], p["b2"][(J - 1) * EM + c] = 0.0, v
    for c, v in _WF_COLS.items():
        p["Wf2"][c], p["bf2"][c] = 0.0, v
    for c, v in _B1_COLS.items():
        p["W1"][NRELU + c], p["b1"][NRELU + c] = 0.0, v
    for c in list(_W1_COLS) + list(_B1_COLS):          # (clamp(wf_raw) = 2.5 in the columns whose gradient runs through it)
        p["Wf2"][c], p["bf2"][c] = 0.0, 2.5
    p["wV2"][:], p["bV2"][:] = 0.0, v_raw
    return p


def _assert_bound_sides(got, ref, J, v_raw, what):
    M = got["g_v"].shape[0]
    can = ref["readable"]
    checks = [("w1_raw", got["g_w1raw"].cpu().view(M, J, EM)[:, J - 1], can["w1_raw"][:, J - 1], _W1_COLS, (0.0, 5.0)),
              ("wf_raw", got["g_wfraw"].cpu(), can["wf_raw"], _WF_COLS, (0.0, 5.0)),
              ("b1_raw", got["gout1"].cpu()[:, NRELU:], can["b1_raw"], _B1_COLS, (-5.0, 5.0))]
    for name, g, readable, cols, (lo, hi) in checks:
        for c, v in cols.items():
            rows = readable[:, c]
            assert int(rows.sum()) >= 4, (what, name, c)
            passes = bool(lo <= float(v) <= hi)
            assert bool(((g[:, c] != 0) == passes)[rows].all()), \
                f"{what}: {name} = {float(v)!r}: gradient {'blocked' if passes else 'passed'}"
    rows = can["v_raw"]
    assert int(rows.sum()) >= 4, (what, "v_raw")
    passes = bool(-5.0 <= float(v_raw) <= 5.0)
    assert bool(((got["g_v"].cpu() != 0) == passes)[rows].all()), \
        f"{what}: v_raw = {float(v_raw)!r}: gradient {'blocked' if passes else 'passed'}"


@pytest.mark.parametrize("J", mm.JS)
def test_gradient_passes_exactly_at_a_clamp_bound(J):
    """torch's clamp rule at the bounds themselves (gradient passes where min <= x <= max): w1_raw / wf_raw / b1_raw /
    v_raw are made exactly 0, 5 or -5, and one float32 step outside, in float32 as in float64, so the side is not a
    rounding matter there.  No decision is taken from the kernel in this test: the kernel's gradient must be non-zero
    exactly where the bound admits it, wherever the unmasked gradient is.  Through macjd_mixer_fused_backward (every J:
    the 16-row and the wide kernel) and, at J in {2, 3}, through macjd_mixer_fused_train, which has clamp masks of its own.
    (wV2 = 0 puts v_raw on the bound and empties gout1's V block, which the other tests cover.)"""
    from macjd_amd import ops
    S, M = mm.SHIPPED_S[J], 33
    p0, q, s, gy = mm.fwd_bwd_inputs(J, S, M)
    (dq, k0), (ds, k1), (dgy, k2) = _inp(q), _inp(s), _inp(gy)
    for v_raw in _V_VALUES:
        p = _bound_params(p0, J, v_raw)
        got = _fwd_bwd(_device_params(p), dq, ds, dgy)
        ref = mm.forward_backward(p, q, s, gy)
        what = f"bounds J={J} v_raw={float(v_raw)!r}"
        _compare(got, ref, ("y", "sn", "xhat", "act", "gq"), what)      # (no mask decision in these)
        _assert_bound_sides(got, ref, J, v_raw, what)
    if J not in (2, 3):
        return
    B, T1 = 3, 17
    host, dev = _td_case(J, B, T1, S)
    pe0, pt, q_e, q_t, state, reward, terminated, filled = host
    tot_m = ops.td_mask_sum(dev["filled"], T1 - 1)
    tq_ref = mm.target_values(pt, q_t, state)
    for v_raw in _V_VALUES:
        pe = _bound_params(pe0, J, v_raw)
        got = _update("train", _device_params(pe), dev["pt"], dev["q_e"], dev["q_t"], dev["state"], dev["reward"],
                      dev["terminated"], dev["filled"], tot_m)
        ref, _ = mm.td_reference(pe, q_e, state, tq_ref, reward, terminated, filled, mm.GAMMA)
        what = f"bounds train J={J} v_raw={float(v_raw)!r}"
        _compare(got, ref, ("y", "sn", "xhat", "act", "gq"), what)
        _assert_bound_sides(got, ref, J, v_raw, what)


@pytest.mark.parametrize("J", [3, 6, 12])
def test_bf16_entry_points_turn_narrow_states_away(J):
    """operand_dtype = 1 at S = 5 (narrow at these J): MACJD_EUNSUPPORTED from the forward, nothing launched, no output
    written — the bf16 kernels load whole first-layer quads there and would read past W1."""
    from macjd_amd import _native, ops
    lib = _native.load()
    S, M = mm.NARROW_S, 17
    p, q, s, gy = mm.fwd_bwd_inputs(J, S, M)
    dp = _device_params(p)
    (dq, k0), (ds, k1) = _inp(q), _inp(s)
    out = _outputs(M, J, S, ("y", "sn", "xhat", "act"))
    io = ops._mixerf_io(dq, ds, dp)
    io.operand_dtype, io.save = 1, 1
    for k in out:
        setattr(io, k, out[k].t.data_ptr())
    assert lib.macjd_mixer_fused_forward(ctypes.byref(io), _stream()) == -4   # MACJD_EUNSUPPORTED (include/macjd.h)
    io.operand_dtype = 0
    assert not ops.mixer_fused_supported(J, S, HH, EM, bf16=True) and ops.mixer_fused_supported(J, S, HH, EM)
    torch.cuda.synchronize()
    for k, g in out.items():
        assert bool(torch.isnan(g.buf).all()), k
