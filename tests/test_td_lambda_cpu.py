"""TD(lambda) targets without a GPU: the float64 model (tests/td_lambda_model.py) against an independent forward view and
its two special cases, ``ops.td_lambda_reference`` against the model, the float32 restatements inside the model's bounds
(and exact where every partial result is representable), the case table's coverage, the tolerances under the project's bar,
and the ``td_lambda`` learner / ``--td-lambda`` driver option on the CPU."""
import copy
import os

import numpy as np
import pytest
import torch

import td_lambda_model as tm
from test_actor_grad_cpu import _bar, learner_for, make_learner_batch, named_params
from test_nets_cpu import load, quiet

from macjd_amd import ops

f32, f64 = np.float32, np.float64
IDS = [c.name for c in tm.CASES]


# --------------------------------------------------------------------------------------------- the model itself
def forward_view(tq, reward, terminated, filled, gamma_, lam):
    """G = (1 - lambda) sum_{n < N} lambda^(n-1) G^(n) + lambda^(N-1) G^(N), N = the steps to the chain's stop, G^(n) the
    n-step returns built directly (float64): discounted rewards of n steps plus the bootstrap of the n-th."""
    tq, r = np.asarray(tq, f32).astype(f64), np.asarray(reward, f32).astype(f64)
    term, fill = np.asarray(terminated) != 0, np.asarray(filled) != 0
    g_, l_ = float(f32(gamma_)), float(f32(lam))
    B, Tm1 = tq.shape
    G = np.zeros((B, Tm1))
    for b in range(B):
        for t in range(Tm1):
            N = 1
            while t + N < Tm1 and fill[b, t + N] and not term[b, t + N - 1]:
                N += 1
            boot = g_ * (1.0 - term[b, t:t + N])
            incl = np.cumprod(boot)                                  # prod of boot over the first n steps
            excl = np.concatenate([[1.0], incl[:-1]])
            n_step = np.cumsum(excl * r[b, t:t + N]) + incl * tq[b, t:t + N]      # G^(1) .. G^(N)
            w = (1.0 - l_) * np.power(l_, np.arange(N - 1))
            G[b, t] = (w * n_step[:N - 1]).sum() + np.power(l_, N - 1) * n_step[N - 1]
    return G


@pytest.mark.parametrize("case", tm.CASES, ids=IDS)
def test_model_equals_the_forward_view(case):
    args = tm.case_args(case)
    _, _, G = tm.td_lambda_model(*args)
    want = forward_view(*args[1:])
    scale = np.abs(args[1]).max() + np.abs(args[2]).max() * (case.Tm1 + 1)
    np.testing.assert_allclose(G, want, rtol=0, atol=1e-13 * scale)


@pytest.mark.parametrize("mask", ["all", "ragged", "term", "hole", "deadrow"])
def test_lambda_zero_is_the_one_step_target_and_lambda_one_the_reward_to_go(mask):
    d = tm.inputs(5, 70, mask, salt=3)
    a = (d["y"], d["tq"], d["reward"], d["terminated"], d["filled"])
    stats, gy, G = tm.td_lambda_model(*a, 0.99, 0.0, gy_cols=73)
    s0, gy0 = tm.td_loss_model(*a, 0.99, gy_cols=73)
    np.testing.assert_allclose(stats, s0, rtol=1e-14, atol=0)
    np.testing.assert_allclose(gy, gy0, rtol=1e-13, atol=1e-18)
    _, _, G1 = tm.td_lambda_model(*a, 0.99, 1.0)
    g_ = float(f32(0.99))
    tq, r = d["tq"].astype(f64), d["reward"].astype(f64)
    for b in range(5):
        for t in range(70):
            want, disc, k = 0.0, 1.0, t
            while True:                       # rewards to the stop, then the single bootstrap
                want += disc * r[b, k]
                stop = k + 1 >= 70 or not d["filled"][b, k + 1] or d["terminated"][b, k]
                disc *= g_
                if stop:
                    want += disc * (1.0 - d["terminated"][b, k]) * tq[b, k]
                    break
                k += 1
            assert abs(G1[b, t] - want) <= 1e-12 * (1 + abs(want)), (b, t)


def _t(a, dtype, shape3=True):
    x = torch.as_tensor(np.asarray(a)).to(dtype)
    return x.unsqueeze(-1) if shape3 else x


@pytest.mark.parametrize("case", tm.CASES[::3], ids=IDS[::3])
def test_reference_form_equals_the_model_in_float64(case):
    y_, tq_, r_, term_, fill_, g_, l_ = tm.case_args(case)
    g_, l_ = float(f32(g_)), float(f32(l_))
    y = _t(y_, torch.float64).requires_grad_(True)
    tq, r = _t(tq_, torch.float64), _t(r_, torch.float64)
    term, fill = _t(term_, torch.bool), _t(fill_, torch.bool)
    loss, my, mg = ops.td_lambda_reference(y, tq, r, term, fill, g_, l_)
    loss.backward()
    stats, gy, G = tm.td_lambda_model(y_, tq_, r_, term_, fill_, g_, l_)
    np.testing.assert_allclose([float(loss.detach()), float(my), float(mg)], stats[:3], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(y.grad.squeeze(-1).numpy(), gy, rtol=1e-12, atol=1e-16)
    got = ops.td_lambda_returns(tq, r, term, fill, g_, l_)
    np.testing.assert_allclose(got.squeeze(-1).numpy(), G, rtol=1e-12, atol=1e-13)
    # lambda = 0: the stock form of the one-step loss, in float32
    y32, tq32, r32 = _t(y_, torch.float32), _t(tq_, torch.float32), _t(r_, torch.float32)
    a = ops.td_lambda_reference(y32, tq32, r32, term, fill, 0.99, 0.0)
    b = ops.td_loss_reference(y32, tq32, r32, term, fill, 0.99)
    np.testing.assert_allclose([float(v) for v in a], [float(v) for v in b], rtol=1e-6, atol=0)


def test_reference_form_keeps_what_is_behind_a_stop_out():
    """The select: a NaN behind a stop reaches no return in front of it."""
    d = tm.inputs(3, 20, "term", salt=1)
    term = d["terminated"].copy()
    term[:, 9] = 1
    tq, r = d["tq"].copy(), d["reward"].copy()
    clean = ops.td_lambda_returns(_t(tq, torch.float32), _t(r, torch.float32), _t(term, torch.bool), _t(d["filled"], torch.bool), 0.99, 0.8)
    tq[:, 10:], r[:, 10:] = np.nan, np.inf
    dirty = ops.td_lambda_returns(_t(tq, torch.float32), _t(r, torch.float32), _t(term, torch.bool), _t(d["filled"], torch.bool), 0.99, 0.8)
    assert torch.equal(clean[:, :10], dirty[:, :10])


# --------------------------------------------------------------------------------------------- restatements and bounds
@pytest.mark.parametrize("case", tm.CASES, ids=IDS)
def test_restatements_sit_inside_the_bounds_and_the_tolerances_under_the_bar(case):
    exp = tm.expectation(case)
    (stats, tol_s), (gy, tol_gy), (G, tol_g) = exp["stats"], exp["gy"], exp["G"]
    r_stats, r_gy, r_G = exp["restated"]
    e_stats, e_gy, e_g = exp["ceilings"]
    T = case.Tm1
    args = tm.case_args(case)
    seq = tm.td_lambda_seq_f32(*args[1:])
    assert np.all(np.abs(r_G - G) <= e_g) and np.all(np.abs(seq - G) <= e_g)          # fairness: both orders
    assert np.all(np.abs(r_gy[:, :T] - gy[:, :T]) <= e_gy) and not r_gy[:, T:].any()
    assert np.all(np.abs(r_stats - stats) <= e_stats) and r_stats[3] == stats[3]
    # the asserted tolerances: under the project's bar relative to the case's max |G| (and, for the scalars, to themselves)
    top = np.abs(G).max()
    print(case.name, "tol G %.2e  gy %.2e  (x max|G|)" % (tol_g.max() / top, tol_gy.max() / top),
          "stats", [float("%.2e" % (t / max(abs(s), 1e-300))) for t, s in zip(tol_s[:3], stats[:3])])
    assert tol_g.max() <= tm.BAR * top and tol_gy.max() <= tm.BAR * top
    assert tol_s[1] <= tm.BAR * np.abs(args[0]).max() and tol_s[2] <= tm.BAR * top and tol_s[0] <= tm.BAR * max(stats[0], top * top)
    assert np.all(tol_g >= np.spacing(np.abs(G).astype(f32)))                          # never under one float32 ulp


@pytest.mark.parametrize("B,Tm1", tm.EXACT_SHAPES)
def test_exact_cases_are_exact_in_both_orders(B, Tm1):
    d = tm.inputs(B, Tm1, "exact")
    a = (d["y"], d["tq"], d["reward"], d["terminated"], d["filled"], 0.5, 0.5)
    for x in a[:3]:
        assert np.array_equal(x * 8, np.round(x * 8)) and np.abs(x).max() <= 4
    term, fill, cont = tm._stops(d["terminated"], d["filled"])
    run = np.zeros(B, np.int64)
    for t in range(Tm1):                       # a stop at most every 8 steps
        run = np.where(cont[:, t], run + 1, 0)
        assert run.max() < 8
    stats, gy, G = tm.td_lambda_model(*a)
    r_stats, r_gy, r_G = tm.td_lambda_f32(*a)
    assert np.array_equal(r_G.astype(f64), G) and np.array_equal(tm.td_lambda_seq_f32(*a[1:]).astype(f64), G)
    assert r_stats[3] == stats[3] == d["filled"].sum()
    want_gy = ((f32(2) / f32(stats[3])) * fill.astype(f32) * (d["y"].astype(f64) - G).astype(f32)).astype(f32)
    assert np.array_equal(r_gy, want_gy)


def test_case_table_reaches_every_corner_of_the_issue():
    C = tm.CASES
    assert {1, 2, 63, 64, 65, 128, 129, 200} <= {c.Tm1 for c in C}
    assert {1, 2, 16, 17, 33} <= {c.B for c in C}
    assert {0.0, 0.5, 0.8, 1.0} <= {c.lam for c in C} and {0.99, 1.0} <= {c.gamma for c in C}
    assert set(tm.MASKS) == {c.mask for c in C}
    assert {0, 1, 5} == {c.gy_extra for c in C} and {"dense", "sliced", "strided"} == {c.layout for c in C}
    assert sum(c.exact for c in C) >= 5 and all((c.gamma, c.lam) == (0.5, 0.5) for c in C if c.exact)
    for c in C:
        d = tm.inputs(c.B, c.Tm1, c.mask)
        fill, term = d["filled"] != 0, d["terminated"] != 0
        if c.mask == "ragged" and c.Tm1 > 2:
            assert (~fill[:, -1]).any() and fill[:, 0].any()
        if c.mask == "term":
            assert (term[:, :-1] & fill[:, 1:]).any() or c.Tm1 == 1
        if c.mask == "hole" and c.Tm1 > 2 and c.B > 1:
            assert (~fill[:, 1:-1] & fill[:, :-2] & fill[:, 2:]).any()
        if c.mask == "deadrow":
            assert not fill[c.B // 2].any() and fill.any()
    # a carry across two chunk boundaries: an unbroken chain from chunk 0 into chunk 2
    long = [c for c in C if c.Tm1 >= 129 and c.mask == "all" and c.lam > 0]
    assert long


# --------------------------------------------------------------------------------------------- learner
TAG, B_, T_ = "3j4r_h64", 4, 7


@pytest.fixture(scope="module")
def setting():
    g, d = load(TAG)
    return g, d, make_learner_batch(g, d, B_, T_, seed=5)


def test_learner_with_lambda_zero_is_the_learner_without_the_option(setting):
    g, d, batch = setting
    mac0, l0, _ = learner_for(g, d)
    mac1, l1, _ = learner_for(g, d, td_lambda=0.0)
    assert l0.td_lambda is None and l1.td_lambda == 0.0
    out0 = l0._forward_backward(copy.deepcopy(batch), T_)
    out1 = l1._forward_backward(copy.deepcopy(batch), T_)
    np.testing.assert_allclose([float(v) for v in out1], [float(v) for v in out0], rtol=1e-6)
    n0, n1 = named_params(mac0, l0), named_params(mac1, l1)
    assert {k for k, p in n0.items() if p.grad is None} == {k for k, p in n1.items() if p.grad is None}
    for k, p in n0.items():
        if p.grad is not None:
            _bar(n1[k].grad.numpy(), p.grad.numpy(), k)


def test_learner_loss_is_the_model_on_its_own_mixer_outputs(setting, monkeypatch):
    g, d, batch = setting
    mac, learner, _ = learner_for(g, d, td_lambda=0.8)
    seen = {}
    real = ops.td_lambda_loss

    def spy(y, tq, reward, terminated, filled, gamma, lam):
        seen.update(y=y.detach(), tq=tq.detach(), reward=reward, terminated=terminated, filled=filled, gamma=gamma, lam=lam)
        return real(y, tq, reward, terminated, filled, gamma, lam)

    monkeypatch.setattr(ops, "td_lambda_loss", spy)
    loss, ev, tg = learner._forward_backward(copy.deepcopy(batch), T_)
    assert seen["lam"] == 0.8 and seen["gamma"] == 0.99 and seen["y"].shape == (B_, T_ - 1, 1)
    sq = lambda k: seen[k].squeeze(-1).numpy()
    stats, _, G = tm.td_lambda_model(sq("y"), sq("tq"), sq("reward"), sq("terminated"), sq("filled"), 0.99, 0.8)
    np.testing.assert_allclose([float(loss), float(ev), float(tg)], stats[:3], rtol=1e-5)
    one_step, _ = tm.td_loss_model(sq("y"), sq("tq"), sq("reward"), sq("terminated"), sq("filled"), 0.99)
    assert abs(one_step[0] - stats[0]) > 1e-3 * stats[0]          # the option moves the target
    assert all(p.grad is not None for p in learner.eval_qmix_net.parameters())
    s = learner.train(copy.deepcopy(batch), {})
    assert list(s) == ["loss", "grad_norm", "eval_qtot_avg", "target_qtot_avg"] and all(np.isfinite(v) for v in s.values())


def test_learner_combines_with_the_other_options(setting):
    g, d, batch = setting
    mac, learner, _ = learner_for(g, d, td_lambda=0.8, train_actor=True, train_agent_body=True)
    s = learner.train(copy.deepcopy(batch), {})
    assert list(s) == ["loss", "grad_norm", "eval_qtot_avg", "target_qtot_avg", "actor_q_avg"]
    assert all(np.isfinite(v) for v in s.values())
    assert all(p.grad is not None for p in mac.agent.parameters())


def test_option_is_validated_by_the_constructor_and_the_driver(setting):
    g, d, _ = setting
    for ok in (0, 0.8, 1, 1.0):
        assert learner_for(g, d, td_lambda=ok)[1].td_lambda == float(ok)
    assert learner_for(g, d, td_lambda=None)[1].td_lambda is None
    for bad in (-0.1, 1.5, float("nan"), "much"):
        with pytest.raises(ValueError, match="td_lambda"):
            learner_for(g, d, td_lambda=bad)
    import macjd_amd.main as mm
    cdir = os.path.join(os.path.dirname(mm.__file__), "config")
    assert "td_lambda" not in open(os.path.join(cdir, "default.yaml")).read()
    seen = []
    orig = mm.run
    mm.run = lambda a: seen.append(getattr(a, "td_lambda", None))
    try:
        with quiet():
            mm.main(["--config-dir", cdir])
            for ok in ("0", "0.8", "1"):
                mm.main(["--config-dir", cdir, "--td-lambda", ok])
        assert seen == [None, 0.0, 0.8, 1.0]
        for bad in ("-0.1", "1.5", "nan"):
            with pytest.raises(SystemExit), quiet(), _quiet_err():
                mm.main(["--config-dir", cdir, "--td-lambda", bad])
        assert len(seen) == 4
    finally:
        mm.run = orig


def _quiet_err():
    import contextlib
    import io
    return contextlib.redirect_stderr(io.StringIO())
