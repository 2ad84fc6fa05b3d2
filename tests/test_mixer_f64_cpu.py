"""The float64 model of the fused mixer (tests/mixer_f64_model.py) is right, and the GPU file's cases are well posed,
without a GPU: the model's Q_tot equals the reference's G4 fixtures, its explicit backward equals float64 autograd through
the stock-torch QMixer (intermediate gradients included), its TD gradient equals autograd of ``ops.td_loss_reference``,
and for every parametrised case of tests/test_mixer_f64_gpu.py (same case table, same seeds) at most 0.5 % of the launch's
mask decisions lie within the band of a threshold — the condition under which the GPU tests may take those few sides
from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO  # noqa: F401

sys.path.insert(0, os.path.dirname(__file__))
import mixer_f64_model as mm  # noqa: E402
from test_nets_cpu import TAGS, load, make_args, sd_from  # noqa: E402

from macjd_amd import ops  # noqa: E402
from macjd_amd.core.networks import QMixer  # noqa: E402

HH, EM, NRELU = mm.HH, mm.EM, mm.NRELU


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_the_g4_fixtures(tag):
    """Q_tot of the model on the reference's G4 inputs, for the fixture's weights and for the x25 set that saturates
    every clamp, at the bar of test_mixer: atol 1e-5 max(1, max|ref|) (the fixtures are float32)."""
    g, d = load(tag)
    sd = sd_from(g, "mixer.")
    q, s = g["g4_q"], g["g4_s"]
    zeros = torch.zeros(q.shape[0])
    for scale, key in ((1.0, "g4_qtot"), (25.0, "g4_qtot_big")):
        p = mm.params_from_state_dict({k: v.double() * scale for k, v in sd.items()})
        y = mm.forward_backward(p, q, s, zeros)["y"].numpy()
        ref = g[key].astype(np.float64).reshape(-1)
        np.testing.assert_allclose(y, ref, rtol=0, atol=1e-5 * max(1.0, float(np.abs(ref).max())), err_msg=key)


def _x3(tag, M=50):
    g, d = load(tag)
    args = make_args(d)
    mixer = mm.x3_mixer(QMixer, args).double()
    rng = np.random.default_rng(d["J"])
    f = lambda *shape: torch.tensor(rng.standard_normal(shape))
    return d, mixer, f(M, d["J"]), 3.0 * f(M, d["S"]), f(M)


@pytest.mark.parametrize("tag", TAGS)
def test_model_backward_equals_float64_autograd(tag):
    """gq, every parameter gradient (LayerNorm's included) and the intermediate gout1 / g_w1raw of the explicit backward
    against float64 autograd through ``QMixer(...).double()`` on the CPU (the stock-torch path), x3 weights,
    ``y.backward(gy)``, rtol 1e-10.  The clamps go both ways and every block of gout1 is non-zero: the comparison is not
    vacuous."""
    d, mixer, q, s, gy = _x3(tag)
    kept = {}
    tail = mixer._hyper_tail

    def keeping_tail(out):
        out.retain_grad()
        raw = tail(out)
        raw[0].retain_grad()
        kept["out1"], kept["w1_raw"] = out, raw[0]
        return raw
    mixer._hyper_tail = keeping_tail
    qg = q.clone().requires_grad_(True)
    y = mixer(qg, s)
    assert y.dtype == torch.float64 and "out1" in kept
    y.backward(gy.view_as(y))
    r = mm.forward_backward(mm.params_from_state_dict(mixer.state_dict(), mixer.state_norm.eps), q, s, gy)
    close = lambda a, b, name: np.testing.assert_allclose(
        a.detach().numpy().reshape(b.shape), b.numpy(), rtol=1e-10, atol=1e-10 * float(b.abs().max()), err_msg=name)
    close(y, r["y"], "y")
    close(qg.grad, r["gq"], "gq")
    close(kept["out1"].grad, r["gout1"], "gout1")
    close(kept["w1_raw"].grad, r["g_w1raw"], "g_w1raw")
    want = mm.state_dict_grads(r["grads"], d["S"])
    names = [n for n, _ in mixer.named_parameters()]
    assert sorted(names) == sorted(want)
    for n, p in mixer.named_parameters():
        close(p.grad, want[n], n)
    assert _populated(r)


def _populated(r):
    """Both sides of every clamp have elements and every block of gout1 is non-zero."""
    ok = True
    for name in ("w1_raw", "wf_raw"):
        x = r["pre"][name]
        ok &= bool((x < 0).any()) and bool(((x >= 0) & (x <= 5)).any()) and bool((x > 5).any())
    for name in ("v_raw", "b1_raw"):
        x = r["pre"][name]
        ok &= bool((x.abs() > 5).any()) and bool((x.abs() <= 5).any())
    g1 = r["gout1"]
    for c0, c1 in ((0, HH), (HH, 2 * HH), (2 * HH, NRELU), (NRELU, mm.N1)):
        ok &= float(g1[:, c0:c1].abs().max()) > 0
    return ok


def test_td_gradient_equals_autograd_of_the_reference_loss():
    """(gamma = 63 / 64: the reference form casts its masks to float32, which would round 0.99 to float32 on the way.)"""
    rng = np.random.default_rng(4)
    gamma = 63.0 / 64.0
    for B, T1 in mm.TD_BATCHES:
        *_, reward, terminated, filled = mm.td_inputs(3, B, T1)
        y = torch.tensor(rng.standard_normal((B, T1, 1)), requires_grad=True)
        tq = torch.tensor(rng.standard_normal((B, T1, 1)))
        r, t, f = (torch.tensor(a) for a in (reward, terminated, filled))
        loss, mean_y, mean_t = ops.td_loss_reference(y[:, :-1], tq[:, 1:], r.double()[:, :-1], t[:, :-1], f[:, :-1], gamma)
        loss.backward()
        gy, loss_m, my_m, mt_m = mm.td_gradient(y.detach().view(B, T1), tq.view(B, T1), r.view(B, T1), t.view(B, T1),
                                                f.view(B, T1), gamma)
        np.testing.assert_allclose(gy.numpy(), y.grad.view(B, T1).numpy(), rtol=1e-12, atol=1e-15)
        assert bool((gy[:, -1] == 0).all())
        for a, b in ((loss_m, loss), (my_m, mean_y), (mt_m, mean_t)):
            assert float(a) == pytest.approx(float(b.detach()), rel=1e-12)
        # the episode structure the GPU test relies on
        f2, t2 = filled.reshape(B, T1), terminated.reshape(B, T1)
        assert f2[:, :-1].sum() > 0 and f2[0].sum() == 1 and t2[0, 0]
        if B > 1:
            assert f2[-1].all() and not t2[-1].any()


def _cap(r, what):
    assert r["n_near"] <= mm.CAP * r["n_decisions"], (what, r["n_near"], r["n_decisions"])
    assert r["n_blind"] == 0, (what, "a near-threshold clamp decision cannot be read off the kernel: change the seed")
    return r["n_near"], r["n_decisions"]


def test_near_threshold_decisions_stay_under_the_cap_in_every_gpu_case():
    """For every launch of tests/test_mixer_f64_gpu.py: decisions within the band of a threshold <= 0.5 % of all mask
    decisions of that launch (a condition: a case that exceeds it gets another seed, never a wider cap).  On at least one
    case per J both sides of every clamp are populated and every gout1 block is non-zero."""
    worst, populated = 0.0, set()
    for case in mm.fwd_bwd_cases():
        r = mm.forward_backward(*mm.fwd_bwd_inputs(*case))
        n, tot = _cap(r, case)
        worst = max(worst, n / tot)
        J, S, M, layout = case
        if _populated(r):
            populated.add(J)
    assert populated == set(mm.JS)
    for J in mm.JS:
        for S in (mm.SHIPPED_S[J], 1):
            p, q, s, gy, _ = mm.degenerate_inputs(J, S)
            n, tot = _cap(mm.forward_backward(p, q, s, gy), ("degenerate", J, S))
            worst = max(worst, n / tot)
        for B, T1, S in mm.td_cases(J):
            pe, pt, q_e, q_t, state, reward, terminated, filled = mm.td_inputs(J, B, T1, S=S)
            r, _ = mm.td_reference(pe, q_e, state, mm.target_values(pt, q_t, state), reward, terminated, filled, mm.GAMMA)
            n, tot = _cap(r, ("td", J, B, T1, S))
            worst = max(worst, n / tot)
    for tag in TAGS:
        g, d = load(tag)
        mixer = mm.x3_mixer(QMixer, make_args(d))
        q, tq, state, reward, terminated, filled = mm.module_inputs(d["J"])
        assert state.shape[-1] == d["S"]
        r, _ = mm.td_reference(mm.params_from_state_dict(mixer.state_dict(), mixer.state_norm.eps), q, state, tq, reward,
                               terminated, filled, mm.GAMMA)
        n, tot = _cap(r, ("module", tag))
        worst = max(worst, n / tot)
    print(f"worst near-threshold share over all GPU cases: {100 * worst:.3f} %")


def test_decisions_argument_overrides_near_elements_only():
    """With ``decisions`` given, the model takes the given side exactly on the near elements: flipping every side changes
    the masks there and nowhere else."""
    p, q, s, gy = mm.fwd_bwd_inputs(3, 46, 33)
    a = mm.forward_backward(p, q, s, gy)
    flipped = {k: ~v for k, v in a["side"].items()}
    b = mm.forward_backward(p, q, s, gy, decisions=flipped)
    near = a["near"]["relu"]
    assert torch.equal(b["side"]["relu"], torch.where(near, ~a["side"]["relu"], a["side"]["relu"]))
    same = mm.forward_backward(p, q, s, gy, decisions=a["side"])
    for k in mm.OUTPUTS:
        assert torch.equal(same[k], a[k]), k


def test_bf16_operands_are_not_offered_for_narrow_states():
    """With bf16 operands the fused kernels have no narrow-row variants (S <= 16 (J - 1), even J: 16 (J - 2)):
    ``ops.mixer_fused_supported(..., bf16=True)`` says no there and yes at the shipped widths; f32 covers both."""
    for J in mm.JS:
        limit = 16 * (J - (2 if J % 2 == 0 else 1))
        for S in sorted({1, mm.NARROW_S, limit, limit + 1, mm.SHIPPED_S[J], 16 * J}):
            if S < 1:
                continue
            assert ops.mixer_fused_supported(J, S, HH, EM) is True, (J, S)
            assert ops.mixer_fused_supported(J, S, HH, EM, bf16=True) is (S > limit), (J, S)
