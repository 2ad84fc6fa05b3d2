"""tests/gru_scan_model.py is what it claims to be: its float64 functions equal float64 torch (``torch.nn.GRUCell``, a
float64 copy of ``RNNAgent``'s fc1 / rnn / actor, ``ops.gru_sequence_reference``) to 1e-12 and the ``nets_*`` golden
fixtures to the fixtures' own float32 bar; the float32 restatement passes its own tolerance on every case of the GPU
tests, and every case is fair (the restatement deviates by at most cap / 8); the prefetch model is ``index_select`` plus
the models of its parts.  Also ``ops.gru_sequence_multi`` on host tensors with an ``h0`` expanded over the batch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import gru_scan_model as gm  # noqa: E402
from test_nets_cpu import TAGS, load, make_args, quiet, sd_from  # noqa: E402

f32, f64 = np.float32, np.float64
T64 = lambda a: torch.tensor(np.asarray(a, f64))   # noqa: E731


def _agent64(w, S, H, Ah, A):
    """float64 RNNAgent carrying the model's weights."""
    from macjd_amd.core.networks import RNNAgent
    d = dict(J=1, A=A, S=S, H=H)
    with quiet():
        a = RNNAgent(S, make_args(d, actor_hidden_dim=Ah)).double()
    with torch.no_grad():
        a.fc1.weight.copy_(T64(w["fc1_w"])); a.fc1.bias.copy_(T64(w["fc1_b"]))
        a.rnn.weight_ih.copy_(T64(w["w_ih"])); a.rnn.bias_ih.copy_(T64(w["b_ih"]))
        a.rnn.weight_hh.copy_(T64(w["w_hh"])); a.rnn.bias_hh.copy_(T64(w["b_hh"]))
        for l, (ww, bb) in zip((0, 2, 4), w["actor"]):
            a.actor[l].weight.copy_(T64(ww)); a.actor[l].bias.copy_(T64(bb))
    return a


@pytest.mark.parametrize("H", [4, 64, 128])
def test_step_and_gates_equal_float64_grucell(H):
    rng = gm._rng("cell", H)
    N = 7
    x, h = rng.standard_normal((N, H)), 0.5 * rng.standard_normal((N, H))
    cell = torch.nn.GRUCell(H, H).double()
    with torch.no_grad():
        want = cell(T64(x), T64(h)).numpy()
    p = {k: v.detach().numpy() for k, v in cell.named_parameters()}
    gi = gm.linear(x, p["weight_ih"], p["bias_ih"])
    gh = gm.linear(h, p["weight_hh"], p["bias_hh"])
    np.testing.assert_allclose(gm.gru_step(gi, gh, h), want, atol=1e-12, rtol=0)
    np.testing.assert_allclose(gm.gates(gi, gh, h), want, atol=1e-12, rtol=0)
    # gi_ld = 0: one row for all
    with torch.no_grad():
        want1 = cell(T64(x[:1]).expand(N, H), T64(h)).numpy()
    np.testing.assert_allclose(gm.gates(gi[:1], gh, h), want1, atol=1e-12, rtol=0)
    np.testing.assert_allclose(gm.gates(gi[0], gh, h), want1, atol=1e-12, rtol=0)


def test_saturating_forms_do_not_overflow():
    x = np.array([0.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4, 800.0, -800.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):   # (underflow to 0 is the saturated value)
        for dt in (f64, f32):
            s, t = gm.sigmoid(x.astype(dt)), gm.tanh(x.astype(dt))
            assert s.dtype == dt and t.dtype == dt
            np.testing.assert_allclose(s, torch.sigmoid(T64(x)).numpy(), atol=1e-7 if dt is f32 else 1e-15, rtol=0)
            np.testing.assert_allclose(t, torch.tanh(T64(x)).numpy(), atol=1e-7 if dt is f32 else 1e-15, rtol=0)
    assert gm.sigmoid(np.array([1e4]))[0] == 1.0 and gm.sigmoid(np.array([-1e4]))[0] == 0.0
    assert gm.tanh(np.array([1e4]))[0] == 1.0 and gm.tanh(np.array([-1e4]))[0] == -1.0


@pytest.mark.parametrize("S,H,Ah,A", [(5, 64, 7, 3), (65, 128, 129, 9)])
def test_model_equals_float64_agent(S, H, Ah, A):
    """The scan from observations (input transform, T cell steps, actor rows) against a float64 RNNAgent stepped by hand."""
    rng = gm._rng("agent", S, H)
    w = gm.agent_weights(rng, S, H, Ah, A)
    B, J, T, NR = 3, 2, 5, 4
    obs = rng.standard_normal((NR, T + 1, J, S))
    rows = [3, 0, 3]
    w["h0"] = 0.5 * rng.standard_normal((B, J, H))
    a = _agent64(w, S, H, Ah, A)
    x = T64(obs[rows, 0]).reshape(B * J, S)
    with torch.no_grad():
        h = T64(w["h0"]).reshape(B * J, H)
        want = []
        for _ in range(T):
            h = a.rnn(torch.relu(a.fc1(x)), h)
            want.append(h.view(B, J, H).numpy())
        want_p = a.actor(x).view(B, J, A).numpy()
        want_gi = torch.nn.functional.linear(torch.relu(a.fc1(x)), a.rnn.weight_ih, a.rnn.bias_ih).numpy()
    got_h, got_p = gm.scan_from_obs(obs, rows, w, T)
    np.testing.assert_allclose(got_h, np.stack(want, 1), atol=1e-12, rtol=0)
    np.testing.assert_allclose(got_p, want_p, atol=1e-12, rtol=0)
    np.testing.assert_allclose(gm.input_transform(obs[rows, 0].reshape(B * J, S), w["fc1_w"], w["fc1_b"], w["w_ih"], w["b_ih"]),
                               want_gi, atol=1e-12, rtol=0)


@pytest.mark.parametrize("static", [False, True])
def test_scan_equals_ops_reference_in_float64(static):
    from macjd_amd import ops
    rng = gm._rng("ref", int(static))
    B, T, J, H = 3, 7, 2, 64
    gi = rng.standard_normal((B, 1 if static else T, J, 3 * H))
    w = gm.recurrent_weights(rng, H)
    h0 = 0.5 * rng.standard_normal((B, J, H))
    for h in (None, h0):
        g_t = T64(gi).expand(B, T, J, 3 * H) if static else T64(gi)
        want = ops.gru_sequence_reference(g_t, T64(w["w_hh"]), T64(w["b_hh"]), None if h is None else T64(h))
        np.testing.assert_allclose(gm.gru_scan(gi, w["w_hh"], w["b_hh"], h, T, static), want.numpy(), atol=1e-12, rtol=0)


@pytest.mark.parametrize("tag", TAGS)
def test_model_equals_golden_agent_step(tag):
    """G3 of the nets fixtures: one agent step (input transform + cell) and the actor rows, recorded in float32."""
    g, d = load(tag)
    sd = {k: v.numpy() for k, v in sd_from(g, "agent.").items()}
    gi = gm.input_transform(g["g3_obs"], sd["fc1.weight"], sd["fc1.bias"], sd["rnn.weight_ih"], sd["rnn.bias_ih"])
    gh = gm.linear(g["g3_h"], sd["rnn.weight_hh"], sd["rnn.bias_hh"])
    np.testing.assert_allclose(gm.gru_step(gi, gh, g["g3_h"]), g["g3_h_out"], atol=1e-5, rtol=0)
    layers = [(sd[f"actor.{l}.weight"], sd[f"actor.{l}.bias"]) for l in (0, 2, 4)]
    np.testing.assert_allclose(gm.actor_rows(g["g3_obs"], layers), g["g3_params_all"], atol=1e-5, rtol=0)
    # the scan of T = 1 from these rows is that step
    N = g["g3_obs"].shape[0]
    h1 = gm.gru_scan(gi.reshape(N, 1, 1, -1), sd["rnn.weight_hh"], sd["rnn.bias_hh"], g["g3_h"].reshape(N, 1, -1), 1, True)
    np.testing.assert_allclose(h1.reshape(N, -1), g["g3_h_out"], atol=1e-5, rtol=0)


def _rule(kind, model, restate):
    """The restatement passes its own tolerance, and the case is fair; -> share of the cap."""
    tol, share = gm.tolerance(kind, model, restate)
    assert np.isfinite(restate).all() and np.isfinite(model).all()
    assert np.all(np.abs(np.asarray(restate, f64) - model) <= tol)
    assert np.all(tol <= (gm.CAP_H if kind == "h" else gm.cap_p(model))) and np.all(tol >= min(gm.FLOOR_H, gm.FLOOR_P))
    assert gm.fair(share), (kind, share)
    return share


def test_floor_and_caps():
    assert gm.FLOOR_H == 12.5 * 2.0 ** -23 and gm.FLOOR_H < gm.CAP_H / 6 and gm.FLOOR_P == 2.0 ** -22 < 1e-6
    tol, share = gm.tolerance("h", np.zeros(3), np.zeros(3))
    assert np.all(tol == gm.FLOOR_H) and share == 0.0
    tol, _ = gm.tolerance("h", np.zeros(3), np.full(3, 1e-3))       # never above the cap
    assert np.all(tol == gm.CAP_H)
    tol, _ = gm.tolerance("p", np.array([0.0, 1.0]), np.array([0.0, 1.0 + 1e-3]))
    np.testing.assert_allclose(tol, [1e-6, 1.1e-5], rtol=1e-12)


def test_scan_cases_restatement_and_fairness():
    worst = 0.0
    for case in gm.scan_cases():
        if case[0] == "ksplit" and case[1] == 64:
            continue    # the same data as the units form
        for model, restate in gm.scan_case_expect(case):
            assert model.shape == (case[2], case[4], case[3], case[1])
            worst = max(worst, _rule("h", model, restate))
    print("scan: restatement's largest deviation / cap", round(worst, 4))


def test_scan_cases_cover_the_edges():
    cases = gm.scan_cases()
    for form, H in gm.FORMS:
        mine = [c for c in cases if c[0] == form and c[1] == H]
        assert {c[4] for c in mine} >= {1, 2, 3, 4, 5, 7, 101}
        assert {(c[2], c[3]) for c in mine} == set(gm.BJS)
        assert any(c[5] for c in mine) and any(c[7] for c in mine) and any(len(c[6]) == 2 for c in mine)
        specs = {s for c in mine for s in c[6]}
        assert specs >= {None, "0", "JH", "T1JH", "JH4"}
        assert any(c[6][0] is None and c[6][1] is not None for c in mine if len(c[6]) == 2)
        assert any(c[6][0] is not None and c[6][1] is None for c in mine if len(c[6]) == 2)
    # different data per sequence and per step, different weights per net
    d = gm.scan_case_data(next(c for c in cases if c[4] == 7 and len(c[6]) == 2))
    gi = d[0]["gi"]
    assert len({gi[b, t, j, 7].item() for b in range(gi.shape[0]) for t in range(gi.shape[1]) for j in range(gi.shape[2])}) == gi[..., 7].size
    assert not np.array_equal(d[0]["w_hh"], d[1]["w_hh"])


def test_obs_cases_restatement_and_fairness():
    worst_h = worst_p = 0.0
    seen_un = set()
    for case in gm.obs_cases():
        form, H, S, Ah, A = case[:5]
        for (h64, h32), (p64, p32) in gm.obs_case_expect(case):
            worst_h = max(worst_h, _rule("h", h64, h32))
            worst_p = max(worst_p, _rule("p", p64, p32))
        for K, N in ((S, Ah), (Ah, Ah), (Ah, A)):
            un = 16 // {1: 1, 2: 2, 3: 4, 4: 4}[(K + 63) // 64]
            if N % un:
                seen_un.add(un)
        if case[10]:    # dead ReLUs: gi = b_ih
            d = gm.obs_case_data(case)
            for w in d["nets"]:
                x = d["obs"][:, 0].reshape(-1, S)
                np.testing.assert_array_equal(gm.input_transform(x, w["fc1_w"], w["fc1_b"], w["w_ih"], w["b_ih"]),
                                              np.broadcast_to(w["b_ih"].astype(f64), (x.shape[0], 3 * H)))
    assert seen_un == {16, 8, 4}
    assert {c[2] for c in gm.obs_cases()} >= {1, 64, 65, 129, 256} and {c[3] for c in gm.obs_cases()} >= {1, 63, 65, 129, 256}
    assert {c[4] for c in gm.obs_cases()} >= {1, 5, 9, 17, 64}
    assert {c[8] for c in gm.obs_cases()} >= {(True, False), (False, True), (True, True)}
    assert {c[9] for c in gm.obs_cases()} == {"none", "dup", "ends"}
    print("from obs: restatement's largest deviation / cap: h", round(worst_h, 4), "P", round(worst_p, 4))


def test_gates_cases_restatement_and_fairness():
    worst = 0.0
    for N in gm.GATE_NS:
        for H in gm.GATE_HS:
            for v in gm.GATE_VARIANTS:
                worst = max(worst, _rule("h", *gm.gates_expect(gm.gates_case_data(N, H, v))))
    print("gates: restatement's largest deviation / cap", round(worst, 4))


def test_prefetch_model_is_index_select_plus_its_parts():
    worst_h = worst_p = 0.0
    for case in gm.PREFETCH_CASES:
        key, n, B, J, T1, N, slots, G, tensors, (S, Ah, A) = case
        d = gm.prefetch_case_data(key)
        ring, w = d["ring"], d["w"]
        assert len(d["idx"]) == n == len(slots)
        for i, (off, nd) in enumerate(slots):
            idx = d["idx"][i]
            assert len(idx) == B and all(0 <= e < gm.PREFETCH_RING for e in idx)
            if not nd:
                assert all(e < N for e in idx)
                assert len(set(idx)) == B if N >= B else idx == [t % N for t in range(B)]
            m = gm.prefetch_model(ring, idx, w, T1, d["Tm1"])
            ti = torch.tensor(idx)
            x = torch.tensor(ring["obs"]).index_select(0, ti)[:, 0].numpy()
            gi = gm.input_transform(x, w["fc1_w"], w["fc1_b"], w["w_ih"], w["b_ih"])[:, None]
            np.testing.assert_array_equal(m["h"], gm.gru_scan(gi, w["w_hh"], w["b_hh"], None, T1, True))
            np.testing.assert_array_equal(m["P"], gm.actor_rows(x, w["actor"]))
            for s, r in zip(ring["srcs"], m["rows"]):
                assert r.dtype == np.uint8 and np.array_equal(r, torch.tensor(s).index_select(0, ti).numpy())
            want = int(torch.tensor(ring["filled"]).index_select(0, ti)[:, :d["Tm1"]].sum())
            assert isinstance(m["tot_m"], int) and m["tot_m"] == want
            if B <= 8:
                assert 0 < B * d["Tm1"] and m["tot_m"] <= B * d["Tm1"]
            r32 = gm.prefetch_model(ring, idx, w, T1, d["Tm1"], f32)
            worst_h = max(worst_h, _rule("h", m["h"], r32["h"]))
            worst_p = max(worst_p, _rule("p", m["P"], r32["P"]))
    assert any(gm.PREFETCH_RING - 1 in i for c in gm.PREFETCH_CASES for i in gm.prefetch_case_data(c[0])["idx"])
    print("prefetch: restatement's largest deviation / cap: h", round(worst_h, 4), "P", round(worst_p, 4))


def test_gru_sequence_multi_on_host_with_an_expanded_initial_state():
    """An h0 expanded over the batch (stride 0) means the same [J, H] block for every batch entry."""
    from macjd_amd import ops
    rng = gm._rng("expand")
    B, T, J, H = 3, 4, 2, 64
    gi = rng.standard_normal((B, T, J, 3 * H)).astype(f32)
    w = gm.recurrent_weights(rng, H)
    row = (0.5 * rng.standard_normal((1, J, H))).astype(f32)
    h0 = torch.tensor(row).expand(B, J, H)
    assert h0.stride(0) == 0
    got = ops.gru_sequence_multi([torch.tensor(gi)], [torch.tensor(w["w_hh"])], [torch.tensor(w["b_hh"])], [h0])[0]
    want = gm.gru_scan(gi, w["w_hh"], w["b_hh"], np.broadcast_to(row, (B, J, H)), T)
    assert np.all(np.abs(got.numpy() - want) <= gm.CAP_H)
