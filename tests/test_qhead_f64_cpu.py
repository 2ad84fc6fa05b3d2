"""tests/qhead_f64_model.py is right, and the inputs of tests/test_qhead_f64_gpu.py are fair: the model against the
reference's own G3 fixtures and the float32 oracle (within the bound derived below), against float64 torch
(``RNNAgent.get_q_value_for_action``, ``torch.argmax`` + ``gather``) and float64 autograd of Linear-ReLU-Linear; the row map
against an expanded P; and, from the model alone, the three conditions that keep the GPU test from hiding a failure.

Bound for float32 data against the model: the fixtures and the oracle hold FLOAT32 evaluations of the same operands, so they
differ from the model by at most the model's own ceiling (E_q of qhead_f64_model: the componentwise worst case of any
float32 order) plus half an ulp for the stored result — nothing is set by eye, and the bound is ~1e-5 on these values."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import qhead_f64_model as qm  # noqa: E402
from test_nets_cpu import TAGS, load, make_args  # noqa: E402

nets_oracle = qm.nets_oracle
f32, f64 = np.float32, np.float64


def _head_of(g):
    return (g["agent.fc2_q_head.0.weight"], g["agent.fc2_q_head.0.bias"], g["agent.fc2_q_head.2.weight"].reshape(-1),
            g["agent.fc2_q_head.2.bias"])


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_the_reference_fixtures_and_the_oracle(tag):
    """g3_q_taken / g3_q_all (written by the reference in float32) and oracle q_value_for_action / q_all_actions."""
    g, d = load(tag)
    A = d["A"]
    W1, b1, w2, b2 = _head_of(g)
    h, idx, par, pall = g["g3_h_out"], g["g3_act"].reshape(-1), g["g3_par"].reshape(-1), g["g3_params_all"]
    assert W1.shape == (d["H"], d["H"] + A + 1) and h.dtype == np.float32
    _, _, _, q = qm.taken(h, idx, par, W1, b1, w2, b2, A)
    _, e_q = qm.ceiling_taken(h, idx, par, W1, b1, w2, b2, A)
    bound = e_q + qm.U * np.abs(q)
    sd = {k[len("agent."):]: g[k] for k in g.files if k.startswith("agent.")}
    for name, q32 in (("fixture", g["g3_q_taken"].reshape(-1)), ("oracle", nets_oracle.q_value_for_action(sd, h, idx, par)[:, 0])):
        err = np.abs(q32.astype(f64) - q)
        print(f"{tag} taken {name}: worst err / bound {np.max(err / bound):.3f} (bound <= {bound.max():.2e})")
        assert np.all(err <= bound), name
    qa = qm.all_actions(h, pall, W1, b1, w2, b2, A)
    bound = qm.ceiling_all(h, pall, W1, b1, w2, b2, A) + qm.U * np.abs(qa)
    for name, q32 in (("fixture", g["g3_q_all"]), ("oracle", nets_oracle.q_all_actions(sd, h, pall))):
        err = np.abs(q32.astype(f64) - qa)
        print(f"{tag} all {name}: worst err / bound {np.max(err / bound):.3f} (bound <= {bound.max():.2e})")
        assert np.all(err <= bound), name
    # the taken value is the all-action value at the taken action with its parameter
    rows = np.arange(h.shape[0])
    pall2 = pall.copy()
    pall2[rows, idx] = par
    np.testing.assert_allclose(qm.all_actions(h, pall2, W1, b1, w2, b2, A)[rows, idx], q, rtol=1e-13, atol=1e-13)


def _agent64(H, A, hd):
    from macjd_amd.core.networks import RNNAgent
    args = make_args(dict(J=2, A=A, S=7, H=H))
    agent = RNNAgent(7, args).double()
    W1, b1, w2, b2 = hd
    with torch.no_grad():
        agent.fc2_q_head[0].weight.copy_(torch.tensor(W1, dtype=torch.float64))
        agent.fc2_q_head[0].bias.copy_(torch.tensor(b1, dtype=torch.float64))
        agent.fc2_q_head[2].weight.copy_(torch.tensor(w2, dtype=torch.float64).view(1, -1))
        agent.fc2_q_head[2].bias.copy_(torch.tensor(np.zeros(1) if b2 is None else b2, dtype=torch.float64))
    return agent


def test_model_matches_float64_torch():
    """RNNAgent.get_q_value_for_action in float64 on valid indices (it raises on the others); out-of-range and non-int32
    indices: the model's one-hot block is empty, i.e. the value is that of the module with the one-hot columns removed."""
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    for case in qm.TAKEN_CASES:
        d = qm.taken_inputs(case)
        A = case.A
        x, pre, act, q = qm.taken(d["h"], d["idx"], d["P"], d["W1"], d["b1"], d["w2"], d["b2"], A)
        valid = (d["idx"] >= 0) & (d["idx"] < A)
        assert np.array_equal(x[:, :64], d["h"]) and np.array_equal(x[:, -1], d["P"]) and x.dtype == np.float32
        assert np.array_equal(x[:, 64:64 + A].sum(axis=1), valid.astype(f32))
        assert np.all(x[valid, 64 + d["idx"][valid]] == 1)
        if case.n >= 15:
            assert not valid[1] and not valid[case.n - 1] and not valid[case.n // 2] and (case.idx_size == 4 or not valid[3])
        agent = _agent64(64, A, (d["W1"], d["b1"], d["w2"], d["b2"]))
        with torch.no_grad():
            if valid.any():
                ref = agent.get_q_value_for_action(t64(d["h"][valid]), torch.tensor(d["idx"][valid]), t64(d["P"][valid]))
                np.testing.assert_allclose(q[valid], ref.numpy()[:, 0], rtol=1e-12, atol=1e-13)
            l1, l2 = agent.fc2_q_head[0], agent.fc2_q_head[2]
            xin = torch.cat([t64(d["h"]), t64(d["P"]).view(-1, 1)], dim=1)
            w = torch.cat([l1.weight[:, :64], l1.weight[:, -1:]], dim=1)
            bare = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(xin, w, l1.bias)), l2.weight, l2.bias)
        if (~valid).any():
            np.testing.assert_allclose(q[~valid], bare.numpy()[~valid, 0], rtol=1e-12, atol=1e-13)
        assert np.array_equal(act, np.maximum(pre, 0))


def test_double_q_matches_torch_argmax_and_gather():
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    for case in qm.DQ_CASES:
        d = qm.dq_inputs(case)
        A, n = case.A, case.n
        q_e, q_t, am, out = qm.double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], A, case.row_map)
        rows = qm.map_rows(n, case.row_map)
        for q, h, P, hd in ((q_e, d["h_e"], d["P_e"], d["head_e"]), (q_t, d["h_t"], d["P_t"], d["head_t"])):
            agent = _agent64(case.H, A, hd)
            with torch.no_grad():
                cols = [agent.get_q_value_for_action(t64(h), torch.full((n,), a), t64(P[rows, a])) for a in range(A)]
            np.testing.assert_allclose(q, torch.cat(cols, dim=1).numpy(), rtol=1e-12, atol=1e-13)
        tam = torch.argmax(t64(q_e), dim=1)
        assert np.array_equal(am, tam.numpy())
        assert np.array_equal(out, torch.gather(t64(q_t), 1, tam.view(-1, 1)).numpy()[:, 0])
    # first maximum on an exact tie
    q = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]])
    assert list(np.argmax(q, axis=1)) == [1, 0]


def test_qhead_grads_match_float64_autograd():
    """Linear-ReLU-Linear in float64 autograd on the float32 x, rows whose pre-activations are away from zero (|pre| > 1e-3:
    the float32 act's mask is then the float64 mask); the outer product's single float32 rounding bounds the difference."""
    for case in qm.WGRAD_CASES:
        d = qm.wgrad_inputs(case)
        x, pre, act, _ = qm.taken(d["h"], d["idx"], d["P"], d["W1"], d["b1"], d["w2"], d["b2"], case.A)
        keep = np.abs(pre).min(axis=1) > 1e-3
        if not keep.any():
            continue
        x, act32, gq = x[keep], act[keep].astype(f32), d["gq"][keep]
        assert np.array_equal(act32 > 0, pre[keep] > 0)
        val, mag = qm.qhead_grads(x, act32, gq, d["w2"])
        W1 = torch.tensor(d["W1"], dtype=torch.float64, requires_grad=True)
        b1 = torch.tensor(d["b1"], dtype=torch.float64, requires_grad=True)
        w2 = torch.tensor(d["w2"], dtype=torch.float64, requires_grad=True)
        b2 = torch.tensor(d["b2"], dtype=torch.float64, requires_grad=True)
        q = torch.relu(torch.tensor(x, dtype=torch.float64) @ W1.T + b1) @ w2 + b2
        q.backward(torch.tensor(gq, dtype=torch.float64))
        # dW1 / db1: every term carries one float32 rounding of gq w2 (relative u); dw2 uses float32(act) (relative u); db2 exact
        for name, ref, rel in (("dW1", W1.grad, qm.U), ("db1", b1.grad, qm.U), ("dw2", w2.grad, qm.U), ("db2", b2.grad, 0.0)):
            err = np.abs(val[name] - ref.numpy().reshape(np.shape(val[name])))
            assert np.all(err <= (rel + 1e-14) * mag[name] + 1e-300), (case, name, float(np.max(err)))
    assert sum(1 for c in qm.WGRAD_CASES if c.K >= 63) >= 8


def test_row_map_reads_the_expanded_rows():
    """p_group = T J, p_inner = J: row (b, t, j) reads the actor row of sequence (b, j) — P[b, j] repeated over t."""
    B, T, J, A = 3, 3, 2, 5
    n = 17                                              # (the last episode is cut short)
    P = np.random.default_rng(5).random((B * J, A)).astype(f32)
    expanded = np.broadcast_to(P.reshape(B, 1, J, A), (B, T, J, A)).reshape(B * T * J, A)[:n]
    rows = qm.map_rows(n, (T * J, J))
    assert (T * J, J) == qm.MAP and np.array_equal(P[rows], expanded) and sorted(set(rows)) == list(range(B * J))
    for case in (c for c in qm.DQ_CASES if c.row_map):
        d = qm.dq_inputs(case)
        rows = qm.map_rows(case.n, case.row_map)
        a = qm.double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], case.A, case.row_map)
        b = qm.double_q(d["h_e"], d["h_t"], d["P_e"][rows], d["P_t"][rows], d["head_e"], d["head_t"], case.A, None)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert sum(1 for c in qm.DQ_CASES if c.row_map and c.n == 17) >= 2


def test_case_lists_cover_what_the_kernels_branch_on():
    tk = qm.TAKEN_CASES
    assert {c.n for c in tk} == {1, 15, 16, 17, 31, 32, 33, 65} and {c.A for c in tk} == {1, 5, 9, 33, 64}
    assert all(len({c.A for c in tk if c.n == n}) >= 2 for n in {c.n for c in tk})
    assert {c.idx_size for c in tk} == {4, 8} and {c.h_ld for c in tk} == {64, 68} and {c.w1_pad for c in tk} == {0, 3}
    assert {c.act_ld for c in tk} == {64, 67} and {c.x_pad for c in tk} == {0, 2, None} and {c.b2 for c in tk} == {True, False}
    dq = qm.DQ_CASES
    assert {(c.H, c.A) for c in dq} == {(64, 5), (64, 9), (64, 17), (64, 33), (128, 5), (128, 9), (128, 17)}
    assert {c.n for c in dq} == {1, 15, 16, 17, 33} and {c.h_pad for c in dq} == {0, 3} and {c.p_pad for c in dq} == {0, 2}
    assert {c.shared for c in dq} == {True, False} and {c.argmax for c in dq} == {True, False} and {c.h_off for c in dq} == {0, 1}
    wg = qm.WGRAD_CASES
    assert {c.K for c in wg} == {1, 63, 64, 65, 129} and {c.A for c in wg} == {5, 9, 33} and {c.act_ld for c in wg} == {64, 67}
    assert {c.x_ld - (65 + c.A) for c in wg} == {0, 1, 2} and sum(1 for c in wg if c.dw_pad) == 1
    rows = [c.n for c in tk] + [c.n for c in dq] + [c.n for c in qm.TIE_CASES] + [c.K for c in wg] + [n for p in qm.PAIR_CASES for n in p]
    assert max(rows) == 129


# ---- the conditions that keep the GPU test from hiding a failure, from the model alone ----
def test_fair_no_random_row_has_a_top_two_gap_inside_the_band():
    """Cap ZERO: on every random row the float64 arg-max is binding on the GPU."""
    worst = np.inf
    for case in qm.DQ_CASES:
        d = qm.dq_inputs(case)
        q_e, _, _, _ = qm.double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], case.A, case.row_map)
        top = np.sort(q_e, axis=1)
        gap = top[:, -1] - top[:, -2]
        band = qm.GAP * qm.tolerance(case, "q").max(axis=1)
        worst = min(worst, float(np.min(gap / band)))
        assert np.all(gap >= band), (case, int((gap < band).sum()))
    print(f"smallest top-two gap / (4 x tolerance): {worst:.1f}")


def test_fair_every_tie_class_has_rows_where_the_pair_leads():
    for case in qm.TIE_CASES:
        d = qm.tie_inputs(case)
        a, a2 = d["pair"]
        W1 = d["head_e"][0]
        assert a < a2 and np.array_equal(W1[:, case.H + a].view(np.uint32), W1[:, case.H + a2].view(np.uint32))
        assert np.array_equal(d["P_e"][:, a], d["P_e"][:, a2])
        AH = (case.A + 1) // 2
        assert {"a": a2 < AH, "b": (a, a2) == (AH - 1, AH), "c": a >= AH and a2 == case.A - 1, "d": (a, a2) == (0, case.A - 1)}[case.cls]
        rows = qm.tie_rows(case)
        print(f"{case}: the pair leads on {rows.size} of {case.n} rows")
        assert rows.size >= 2, case
        q_e, _, am, _ = qm.double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], case.A)
        assert np.all(am[rows] == (0 if case.cls == "d" else a))       # the model's first maximum is the lower index
    assert {(c.H, c.A) for c in qm.TIE_CASES} == {(64, 5), (64, 33), (128, 9)}


def test_fair_the_relu_mask_is_exercised():
    for case in list(qm.TAKEN_CASES) + list(qm.WGRAD_CASES):
        d = qm.taken_inputs(case) if isinstance(case, qm.TakenCase) else qm.wgrad_inputs(case)
        _, _, act, _ = qm.taken(d["h"], d["idx"], d["P"], d["W1"], d["b1"], d["w2"], d["b2"], case.A)
        zero = float((act == 0).mean())
        assert 0.25 <= zero <= 0.75, (case, zero)


def test_tolerances_are_below_the_ceiling_and_positive():
    for case in list(qm.TAKEN_CASES) + list(qm.DQ_CASES) + list(qm.TIE_CASES):
        for tensor in (("act", "q") if isinstance(case, qm.TakenCase) else ("q", "out")):
            tol, ceil = qm.tolerance(case, tensor), qm.ceiling(case, tensor)
            assert tol.shape == ceil.shape and np.all(tol > 0) and np.all(tol <= ceil)
            assert qm.yardstick(case)[tensor] > 0
