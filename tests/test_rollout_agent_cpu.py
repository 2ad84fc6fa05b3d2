"""tests/rollout_agent_model.py is right, and the tables of tests/test_mlp_f64_gpu.py, tests/test_qhead_select_f64_gpu.py and
tests/test_agent_episode_f64_gpu.py are fair and complete — without a GPU: the model against float64 torch (Linear chains,
GRUCell, RNNAgent) to 1e-12, against the reference's G3 fixtures and the float32 oracle within the model's own bound, the
selection rule against the reference's selector semantics, the draw's uniformity and the explore compare; and, from the
model alone for every case of every table, that the float32 restatement stays inside the asserted tolerance, that the
tolerance is at most the project's cap, that at most 0.5 % of a case's greedy rows are not binding, and that the tables
reach every item the GPU files promise."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import gru_scan_model as gm  # noqa: E402
import qhead_f64_model as qm  # noqa: E402
import rollout_agent_model as m  # noqa: E402
from _harness import REPO  # noqa: E402
from test_nets_cpu import TAGS, load, make_args  # noqa: E402

nets_oracle = qm.nets_oracle
f32, f64 = np.float32, np.float64
t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------- the model is right
def test_mlp_matches_float64_torch():
    acts = {m.ACT_NONE: torch.nn.Identity, m.ACT_RELU: torch.nn.ReLU, m.ACT_SIGMOID: torch.nn.Sigmoid}
    for name in ("rows17-resident", "rows17-staged", "act22", "act-sigmoid-3layers", "k255-xodd", "n113-inner", "bcast-xodd"):
        c = m.mlp_case(name)
        x, layers = m.mlp_data(c)
        mods = []
        for W, b, act in layers:
            lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
            with torch.no_grad():
                lin.weight.copy_(t64(W))
                lin.bias.copy_(t64(b))
            mods += [lin, acts[act]()]
        with torch.no_grad():
            ref = torch.nn.Sequential(*mods)(t64(x)).numpy()
        y, err = m.mlp(x, layers)
        np.testing.assert_allclose(y, ref, rtol=1e-12, atol=1e-12)
        assert err.shape == y.shape and (err > 0).all()
        full, _ = m.mlp_expect(c)
        np.testing.assert_allclose(full, np.broadcast_to(ref, full.shape) if c["x_ld"] == 0 else ref, rtol=1e-12, atol=1e-12)


def _agent64(g, d):
    from macjd_amd.core.networks import RNNAgent
    agent = RNNAgent(d["S"], make_args(d)).double()
    agent.load_state_dict({k[len("agent."):]: t64(g[k]) for k in g.files if k.startswith("agent.")})
    return agent


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_float64_rnn_agent_the_fixtures_and_the_oracle(tag):
    """One agent step of the reference on its own G3 inputs: actor chain, input transform, cell, all-action Q-head."""
    g, d = load(tag)
    H, A = d["H"], d["A"]
    agent = _agent64(g, d)
    sd = {k[len("agent."):]: g[k] for k in g.files if k.startswith("agent.")}
    obs, h = g["g3_obs"], g["g3_h"]
    with torch.no_grad():
        h_ref = agent.forward(t64(obs), t64(h)).numpy()
        p_ref = agent.actor_forward(t64(obs)).numpy()
        cell_ref = agent.rnn(torch.relu(agent.fc1(t64(obs))), t64(h)).numpy()
    actor = [(sd[f"actor.{i}.weight"], sd[f"actor.{i}.bias"], a) for i, a in ((0, m.ACT_RELU), (2, m.ACT_RELU), (4, m.ACT_SIGMOID))]
    P, p_err = m.mlp(obs, actor)
    gi, gi_err = m.mlp(obs, [(sd["fc1.weight"], sd["fc1.bias"], m.ACT_RELU), (sd["rnn.weight_ih"], sd["rnn.bias_ih"], m.ACT_NONE)])
    h_out = m.gru_cell(gi, h, sd["rnn.weight_hh"], sd["rnn.bias_hh"])
    np.testing.assert_allclose(P, p_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(h_out, h_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(h_out, cell_ref, rtol=1e-12, atol=1e-12)
    # the reference's float32 results and the float32 oracle: inside the model's own bound (+ half an ulp of the stored value)
    for name, p32 in (("fixture", g["g3_params_all"]), ("oracle", nets_oracle.actor_forward(sd, obs))):
        assert np.all(np.abs(p32 - P) <= p_err + m.U * np.abs(P)), (tag, name)
    TOL = 1e-5                                                          # the G3 bar (tests/test_nets_cpu.py)
    np.testing.assert_allclose(h_out, g["g3_h_out"], atol=TOL, rtol=0)
    np.testing.assert_allclose(h_out, nets_oracle.agent_forward(sd, obs, h), atol=TOL, rtol=0)
    # Q-head from the fixture's float32 hidden state
    W1, b1, w2, b2 = sd["fc2_q_head.0.weight"], sd["fc2_q_head.0.bias"], sd["fc2_q_head.2.weight"].reshape(-1), sd["fc2_q_head.2.bias"]
    h32, pall = g["g3_h_out"], g["g3_params_all"]
    base, base_err = m.qhead_base(h32, W1, b1)
    q, q_err = m.qhead_all(base, pall, W1, w2, b2, base_err=base_err)
    with torch.no_grad():
        cols = [agent.get_q_value_for_action(t64(h32), torch.full((h32.shape[0],), a), t64(pall[:, a])) for a in range(A)]
    np.testing.assert_allclose(q, torch.cat(cols, dim=1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(q, qm.all_actions(h32, pall, W1, b1, w2, b2, A), rtol=1e-12, atol=1e-12)
    for name, q32 in (("fixture", g["g3_q_all"]), ("oracle", nets_oracle.q_all_actions(sd, h32, pall))):
        assert np.all(np.abs(q32 - q) <= q_err + m.U * np.abs(q)), (tag, name)
    # the reference's greedy selection (G3: three steps with a partial mask) on the fixture's own states
    av = g["g3_sel_avail"].reshape(-1, A) != 0
    for t in range(3):
        hs = g["g3_sel_h"][t]
        with torch.no_grad():
            pt = agent.actor_forward(t64(obs) * (1.0 + 0.1 * t)).numpy()
        base, base_err = m.qhead_base(hs, W1, b1)
        q, q_err = m.qhead_all(base, pt.astype(f32), W1, w2, b2, base_err=base_err)
        sel = m.select(q, av, 0.0, 0, 0, np.arange(q.shape[0]), 1, tol=np.minimum(q_err, m.cap(q)))
        ok, _ = m.check_choice(sel, g["g3_sel_T"][t].reshape(-1))
        assert ok.all(), (tag, t)


def test_gates_match_float64_grucell():
    for H in (64, 128):
        rng = np.random.default_rng(H)
        cell = torch.nn.GRUCell(H, H).double()
        x, h = rng.standard_normal((9, H)), np.tanh(rng.standard_normal((9, H)))
        sd = {k: v.detach().numpy() for k, v in cell.state_dict().items()}
        with torch.no_grad():
            ref = cell(t64(x), t64(h)).numpy()
        gi = x @ sd["weight_ih"].T + sd["bias_ih"]
        np.testing.assert_allclose(m.gru_cell(gi, h, sd["weight_hh"], sd["bias_hh"]), ref, rtol=1e-12, atol=1e-12)
        # b_hh of gate n belongs inside r * (...): moving it out changes the result
        moved = m.gru_cell(gi + np.r_[np.zeros(2 * H), sd["bias_hh"][2 * H:]], h, sd["weight_hh"], np.r_[sd["bias_hh"][:2 * H], np.zeros(H)])
        assert np.abs(moved - ref).max() > 1e-4


# ------------------------------------------------------------------------------------------------- the selection rule
def test_greedy_part_is_the_references_selector():
    from macjd_amd.utils.action_selectors import EpsilonGreedyActionSelector
    sel_ref = EpsilonGreedyActionSelector(make_args(dict(J=3, A=9, S=5, H=64)))
    rng = np.random.default_rng(5)
    q = rng.standard_normal((40, 3, 9))
    av = rng.random((40, 3, 9)) < 0.6
    av[0], av[1], av[2] = False, False, True                # nothing, one, all
    av[1, :, 4] = True
    q[3, :, 2] = q[3, :, 6] = 9.0                           # an exact tie: the first maximum
    av[3, :, [2, 6]] = True
    ref = sel_ref.select_action(t64(q), torch.tensor(av.astype(np.int64)), 0, test_mode=True).numpy().reshape(-1)
    got = m.select(q.reshape(-1, 9), av.reshape(-1, 9), 1.0, 1, 1, np.arange(120), 1)
    assert np.array_equal(got["greedy"], ref) and np.array_equal(got["action"], ref) and not got["explore"].any()
    assert (got["greedy"][:3] == 0).all() and (got["greedy"][3:6] == 4).all() and (got["greedy"][9:12] == 2).all()
    oracle_T, _ = nets_oracle.select_greedy(q.reshape(-1, 9), q.reshape(-1, 9), av.reshape(-1, 9).astype(np.int64))
    assert np.array_equal(oracle_T, ref)


def test_draw_is_uniform_over_the_pool_and_keyed_as_the_header_says():
    n = np.arange(4096)
    v0, v1 = m.draw(n, 2 ** 32 + 5, 2 ** 40 + 9)
    from tests_golden_helpers import philox4x32_10
    for i in (0, 1, 4095):
        w = philox4x32_10((i, 0, 5, 1), (9, 2 ** 8))
        assert (int(v0[i]), int(v1[i])) == (w[0], w[1])
    w = philox4x32_10((3, 2, 0xFFFFFFFF, 0), (7, 0))
    a, b = m.draw(np.array([2 ** 33 + 3]), 2 ** 32 - 1, 7)
    assert (int(a[0]), int(b[0])) == (w[0], w[1])
    q = np.zeros((4096, 64))
    for pool in range(1, 65):
        av = np.zeros((4096, 64), bool)
        where = np.sort(np.random.default_rng(pool).choice(64, pool, replace=False))
        av[:, where] = True
        s = m.select(q, av, 1.0, 99, pool, n, 0)
        assert s["explore"].all() and av[n, s["action"]].all()
        counts = np.bincount(s["action"], minlength=64)[where]
        # multinomial(4096, 1 / pool): every count within 6 sigma of the mean
        mean, sd = 4096 / pool, np.sqrt(4096 / pool * (1 - 1 / pool))
        assert (np.abs(counts - mean) <= 6 * sd + 1e-9).all(), pool
        v0, v1 = m.draw(n, pool, 99)
        k = (v1.astype(object) * pool) >> 32               # exact integers
        assert np.array_equal(s["action"], where[np.array(k, np.int64)])
    none = m.select(q[:, :9], np.zeros((4096, 9), bool), 1.0, 99, 3, n, 0)      # nothing available: uniform over all A
    assert (np.bincount(none["action"], minlength=9) > 4096 / 9 - 6 * np.sqrt(4096 / 9)).all()
    assert (m.select(q[:, :9], np.zeros((4096, 9), bool), 1.0, 99, 3, n, 1)["action"] == 0).all()


def test_explore_compare_is_the_float32_compare():
    n = np.arange(1 << 16)
    v0, _ = m.draw(n, 1, 2)
    u32 = (v0 >> np.uint64(8)).astype(f32) * f32(1.0 / 16777216.0)
    q = np.zeros((n.size, 3))
    for eps in (0.0, 2.0 ** -24, 0.3, 1.0 - 2.0 ** -24, 1.0):
        got = m.select(q, None, eps, 2, 1, n, 0)["explore"]
        assert np.array_equal(got, (u32 < f32(eps)) & (f32(eps) > 0)), eps
    assert not m.select(q, None, 0.0, 2, 1, n, 0)["explore"].any() and m.select(q, None, 1.0, 2, 1, n, 0)["explore"].all()
    assert not m.select(q, None, 1.0, 2, 1, n, 1)["explore"].any()          # greedy_only
    share = m.select(q, None, 0.3, 2, 1, n, 0)["explore"].mean()
    assert abs(share - 0.3) < 6 * np.sqrt(0.21 / n.size)
    # eps = 2^-24 explores exactly where the 24-bit word is zero
    assert np.array_equal(m.select(q, None, 2.0 ** -24, 2, 1, n, 0)["explore"], (v0 >> np.uint64(8)) == 0)


def test_counter_dev_is_added_to_counter():
    """The carry case draws with the sum 2^32 + 2, reached through a carry out of the low word."""
    c = m.qs_case("counter-carry")
    a, av = m.qs_expect(c), m.qs_data(c)["avail"].reshape(130, 9)
    assert c["counter"] + c["counter_dev"] == 2 ** 32 + 2 and a["sel"]["explore"].all()
    same = m.select(a["q"], av, 1.0, c["seed"], 2 ** 32 + 2, np.arange(130), 0)
    assert np.array_equal(same["action"], a["sel"]["action"])
    for counter in (c["counter"], 2, c["counter_dev"]):     # *counter_dev dropped / the carry lost / counter dropped
        other = m.select(a["q"], av, 1.0, c["seed"], counter, np.arange(130), 0)
        assert not np.array_equal(other["action"], a["sel"]["action"])


# ------------------------------------------------------------------------------------------------- the tables are fair
def test_mlp_table_restatement_inside_tolerance_and_tolerance_under_the_cap():
    worst = 0.0
    for c in m.mlp_cases():
        y, tol = m.mlp_expect(c)
        x, layers = m.mlp_data(c)
        assert (tol > 0).all() and tol.max() <= m.cap(y) and y.shape == (c["rows"], c["dims"][-1])
        rows = m.mlp_restated_rows(c)
        xr = np.broadcast_to(x, (c["rows"], x.shape[1])) if c["x_ld"] == 0 else x
        y32, _ = m.mlp(xr[rows], layers, f32)
        assert y32.dtype == f32
        r = float((np.abs(y32 - y[rows]) / tol[rows]).max())
        assert r <= 0.5, (c["name"], r)                    # half the tolerance is left to the summation order
        worst = max(worst, r)
    print("mlp: worst |restatement - model| / tol", round(worst, 3))


def test_qhead_select_table_is_fair():
    worst = 0.0
    for c in m.qs_cases():
        d, e = m.qs_data(c), m.qs_expect(c)
        assert e["tol"].max() <= m.cap(e["q"]) and (e["tol"] > 0).all()
        q32, _ = m.qhead_all(d["base"], d["P"], d["W1"], d["w2"], d["b2"], dt=f32)
        assert q32.dtype == f32
        r = float((np.abs(q32 - e["q"]) / e["tol"]).max())
        assert r <= 0.5, (c["name"], r)
        worst = max(worst, r)
        for sel, what in ((e["sel"], "selection"), (e["plain"], "argmax_out")):
            greedy = ~sel["explore"]
            loose = greedy & ~sel["binding"]
            assert loose.sum() <= m.NONBINDING_SHARE * greedy.sum(), (c["name"], what, int(loose.sum()), int(greedy.sum()))
        if c["tie"]:
            a = d["pair"]
            assert all(np.array_equal(e["q"][:, a[0]], e["q"][:, k]) for k in a[1:]), c["name"]      # exact in the model too
            led = e["sel"]["binding"] & np.isin(e["sel"]["greedy"], a)          # the tie leads, by more than 4 x tol
            assert led.sum() >= c["rows"] // 2, c["name"]
            av = d["avail"].reshape(c["rows"], c["A"])
            first = np.argmax(av[:, list(a)], axis=1)
            assert np.array_equal(e["sel"]["greedy"][led], np.asarray(a)[first][led]), (c["name"], "lowest available index of the tie")
    print("qhead_select: worst |restatement - model| / tol", round(worst, 3))


def test_episode_tables_are_fair():
    worst_dev, rows, loose = 0.0, 0, 0
    for c in m.all_ep_cases():
        f = m.ep_fair(c)
        assert m.FACTOR * f["dev"] <= m.CAP, (c["name"], f["dev"])           # the factor 8 never reaches the cap
        assert gm.FLOOR_H <= f["tol_step"] <= m.CAP and gm.FLOOR_H <= f["tol_free"] <= m.CAP
        assert f["nonbinding"] <= m.NONBINDING_SHARE * f["greedy"], (c["name"], f["nonbinding"], f["greedy"])
        assert np.abs(f["model"]).max() < 1.0
        worst_dev, rows, loose = max(worst_dev, f["dev"]), rows + f["greedy"], loose + f["nonbinding"]
        # Q restatement along the model's trajectory
        d = m.ep_data(c)
        t = c["T"] - 1
        h32 = f["model"][t].astype(f32)
        q, tol, sel, P = m.step_choice(c, d, t, h32)
        b32, _ = m.qhead_base(h32, d["W1"], d["b1"], dt=f32)
        q32, _ = m.qhead_all(b32, P, d["W1"][:, :c["H"] + c["A"] + 1], d["w2"], d["b2"], dt=f32)
        assert tol.max() <= m.cap(q) and float((np.abs(q32 - q) / tol).max()) <= 0.5, c["name"]
    print(f"episodes: worst restatement deviation {worst_dev:.2e} ({worst_dev / m.CAP:.1%} of the cap), "
          f"{loose} of {rows} greedy rows not binding")


# ------------------------------------------------------------------------------------------------- the tables are complete
def test_mlp_table_covers_the_issue():
    cs = m.mlp_cases()
    assert len({c["name"] for c in cs}) == len(cs)
    assert m.mlp_form(m.RES) == "resident" and m.mlp_form(m.STAGED) == "staged" and m.mlp_form((16, 16)) == "resident"
    for dims in (m.RES, m.STAGED):
        assert {c["rows"] for c in cs if c["dims"] == dims and c["x_ld"] != 0} >= {1, 15, 16, 17, 63, 64, 65, 16384, 16385, 16449}
    assert any(c["rows"] == 3 * 16384 + 1 and c["dims"] == (16, 16) for c in cs)
    for x_off, w_off in ((0, 0), (1, 0), (0, 1)):
        assert {c["dims"][0] for c in cs if (c["x_off"], c["w_off"]) == (x_off, w_off)} >= {1, 3, 15, 16, 17, 64, 65, 252, 255, 256}
    inner = {c["dims"][1] for c in cs if len(c["dims"]) > 2}
    last = {c["dims"][-1] for c in cs}
    assert inner >= set(m.MLP_N_ANY) and last >= set(m.MLP_N_ANY) | set(m.MLP_N_LAST)
    assert {(c["dims"][-1] + 15) // 16 for c in cs} | {(n + 15) // 16 for n in inner} == {1, 2, 3, 4, 8, 12, 24}
    assert {(15 + d[-1]) // 16 for d in m.MLP_UNSUPPORTED if len(d) == 2 and d[0] == 20} >= {5, 6, 7, 9, 11, 13, 23}
    assert {(257, 16), (20, 129, 16), (24, 128, 384), (20, 65), (20, 193), (20, 112)} <= set(m.MLP_UNSUPPORTED)
    assert all(m.mlp_form(d) == "unsupported" for d in m.MLP_UNSUPPORTED)
    assert {c["acts"][0] for c in cs if len(c["acts"]) > 1} == set(m.ACTS) and {c["acts"][-1] for c in cs} == set(m.ACTS)
    assert any(c["acts"][0] == m.ACT_SIGMOID and c["dims"][1] == 9 and len(c["dims"]) > 2 for c in cs)      # 0.5 in the pad columns
    assert {len(c["acts"]) for c in cs} == {1, 2, 3}
    assert {c["x_ld"] for c in cs} == {0, "min", "pad"} and any(c["y_pad"] for c in cs)
    assert {m.mlp_form(c["dims"]) for c in cs if c["x_ld"] == 0} == {"resident", "staged"}
    forms = lambda p: {m.mlp_form(m.mlp_case(n)["dims"]) for n in p}
    rows = lambda p: sorted(m.mlp_case(n)["rows"] for n in p)
    assert any(forms(p) == {"resident", "staged"} for p in m.MLP_PAIRS) and any(rows(p) == [1, 16449] for p in m.MLP_PAIRS)
    assert any(p[0] == p[1] for p in m.MLP_PAIRS)


def test_qhead_select_table_covers_the_issue():
    cs = m.qs_cases()
    assert len({c["name"] for c in cs}) == len(cs)
    one_lane = lambda c: c["rows"] >= 65536 or c["H"] < 16
    assert {c["rows"] for c in cs if not one_lane(c)} >= {1, 63, 64, 65, 129}
    assert any(c["rows"] == 65537 and c["H"] == 16 and c["A"] == 5 for c in cs) and any(c["H"] == 8 and c["rows"] == 70 for c in cs)
    assert {c["H"] for c in cs if c["base"] == "vec"} >= set(m.QS_H) and {c["base"] for c in cs} == {"vec", "oddld", "oddoff"}
    assert {c["A"] for c in cs} >= set(m.QS_A_COMPILED) | set(m.QS_A_GENERIC)
    d = m.qs_data(m.qs_case("a64"))
    only = d["avail"].reshape(-1, 64)
    assert (only[:, 63] & (only.sum(axis=1) == 1)).sum() >= 10
    assert {c["na"] for c in cs} >= {1, 3, 12} and {c["avail"] for c in cs} >= {None, "i32", "i64", "perm32", "perm64"}
    for c in cs:
        if c["avail"] and not c["tie"] and c["rows"] > 1:
            n_av = m.qs_data(c)["avail"].reshape(c["rows"], c["A"]).sum(axis=1)
            assert n_av[0] == 0 and n_av[1] == 1, c["name"]
    outs = {c["outs"] for c in cs}
    assert outs >= {("Q",), ("T32",), ("T64",), ("T32", "P"), ("argmax",), ("gather",), ("Q", "T32", "T64", "P", "argmax", "gather")}
    assert {c["t_layout"] for c in cs} == {"ej", "je"}
    g = m.qs_data(m.qs_case("rows129"))["gather"]
    assert {0, 8, -1, 9, 2 ** 33} <= set(g.tolist())
    assert {(c["eps"], c["eps_dev"]) for c in cs} >= {(e, k) for e in (0.0, 0.3, 1.0) for k in (False, True)}
    assert any(c["counter_dev"] and c["counter"] < 2 ** 32 <= c["counter"] + c["counter_dev"] and c["seed"] > 2 ** 32 for c in cs)
    assert any(c["greedy_only"] and c["eps"] == 1.0 for c in cs)
    assert {(c["tie"], one_lane(c)) for c in cs if c["tie"]} == {(t, k) for t in m.TIES for k in (False, True)}
    some_explore = [c for c in cs if 0 < c["eps"] < 1 and not c["greedy_only"]]
    assert all(0 < m.qs_expect(c)["sel"]["explore"].sum() < c["rows"] for c in some_explore if c["rows"] >= 60)


def test_episode_tables_cover_the_issue():
    cs, sq = m.ep_cases(), m.seq_cases()
    assert len({c["name"] for c in cs + sq}) == len(cs + sq)
    tile = [c for c in cs if not m.ep_is_flat(c)]
    flat = [c for c in cs if m.ep_is_flat(c)]
    assert {(c["H"], c["J"], c["A"], c["E"]) for c in tile} == {(H, J, A, E) for H, J, A in m.ONE_TILE for E in m.ONE_TILE_E}
    assert {(c["J"], c["A"], c["E"]) for c in flat} == set(m.FLAT) and all(c["H"] == 64 for c in flat)
    assert {c["E"] * c["J"] for c in flat} >= {1, 12, 60, 63, 64, 65, 66, 68, 72, 192}
    assert any(c["J"] >= 4 and c["avail"] and c["avail"].startswith("perm") for c in flat)      # mask on the (env, agent) split of the row
    for group in (tile, flat, [c for c in cs if c["H"] == 128]):
        assert {c["T"] for c in group} == set(m.EP_T)
        assert {c["gi_ld"] for c in group} == set(m.EP_GI_LD) and {c["p_ld"] for c in group} == set(m.EP_P_LD)
        assert {(c["gi_ld"] == "0", c["p_ld"] == "0") for c in group} >= {(False, False), (False, True), (True, False)}
        assert {c["h0"] for c in group} == {False, True} and {c["h_final"] for c in group} == {False, True}
        assert {c["w1_pad"] for c in group} == {0, 5} and {c["w1_off"] for c in group} == {0, 1}
        assert {c["avail"] for c in group} == set(m.EP_AVAIL)
        assert {c["counter_base"] for c in group} == set(m.EP_COUNTER)
        assert any(c["eps"] is None for c in group) and any(c["eps"] and {0.0, 0.3, 1.0} <= set(c["eps"]) for c in group)
        assert any(c["counter_base"] == 2 ** 32 - 2 and c["T"] >= 3 and c["eps"] and max(c["eps"][2:]) > 0 for c in group)
    assert any(c["gi_ld"] == "0" and c["p_ld"] == "0" for c in cs)
    assert any(c["T"] == 1 and c["h_final"] and c["H"] == 128 for c in cs) and any(c["T"] == 1 and c["h_final"] and c["H"] == 64 for c in cs)
    assert any(c["J"] == 6 and c["eps"] and c["avail"] for c in tile)              # the second Q-head pass, masked and exploring
    for c in cs + sq:
        if c["avail"] and c["E"] * c["J"] > 1:
            n_av = m.ep_data(c)["avail"].reshape(-1, c["A"]).sum(axis=1)
            assert n_av[0] == 0 and n_av[1] == 1
    assert {(c["H"], c["J"], c["A"], c["seq"]) for c in sq} == {s + (k,) for s in m.SEQ_SIZES for k in m.SEQ_MODES}
    for c in sq:
        d = m.ep_data(c)
        steps = 1 if c["seq"] == "zero" else c["T"]
        assert d["gi"].shape[0] == steps and d["P"].shape[0] == steps
        if c["seq"] == "frame":
            assert d["gi"].shape[1] == 1 and d["P"].shape[1] == 1
        if c["seq"] == "full":
            assert d["gi"].shape[1] == c["E"] * c["J"] == d["P"].shape[1]


# ------------------------------------------------------------------------------------------------- struct layouts
@pytest.mark.parametrize("cls,cname", [("MlpIO", "macjd_mlp_io"), ("QheadIO", "macjd_qhead_io"), ("AgentEpisodeIO", "macjd_agent_episode_io"),
                                       ("AgentEpisodeSeqIO", "macjd_agent_episode_seq_io")])
def test_struct_layout_matches_the_header(cls, cname):
    from macjd_amd import _native
    IO = getattr(_native, cls)
    fields = [n for n, *_ in IO._fields_]
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    body = hdr[hdr.index("typedef struct " + cname + " {"):hdr.index("} " + cname + ";")]
    assert all(re.search(rf"\b{n}\b", body) for n in fields)      # every mirrored field is a field of the header's struct
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           f'int main(){{printf("%zu", sizeof({cname}));\n'
           + "".join(f'printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO)
    assert out[1:] == sorted(out[1:]) and len(set(out[1:])) == len(fields)      # the mirror lists the fields in the header's order
    for name, off in zip(fields, out[1:]):
        assert getattr(IO, name).offset == off, name
