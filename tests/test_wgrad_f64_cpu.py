"""tests/wgrad_f64_model.py proved without a GPU: the model against float64 torch autograd (F.linear's parameter gradients,
ReLU -> one-output Linear for the outer_vec form, relu / split / cat for the split ReLU, F.linear's forward for the row dot),
the fairness of its bounds and of its exact data from the model alone, and the coverage of its case tables."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import wgrad_f64_model as m  # noqa: E402

f32, f64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a, f64))  # noqa: E731


# ------------------------------------------------------------------------------------------------ model against autograd
@pytest.mark.parametrize("name", ["k65", "k513", "k2113"])
@pytest.mark.parametrize("kind", m.KINDS)
def test_weight_gradient_is_autograd_of_linear(name, kind):
    c = m.wgrad_case(name)
    d = m.wgrad_data(c, kind)
    W = torch.zeros(c["M"], c["N"], dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c["M"], dtype=torch.float64, requires_grad=True)
    F.linear(T(d["inp"]), W, b).backward(T(d["gout"]))
    dW, db, tW, tb = m.wgrad_expect(c, kind)
    assert np.allclose(dW, W.grad.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(db, b.grad.numpy(), rtol=1e-12, atol=1e-12)
    if kind == "exact":
        assert np.array_equal(dW, W.grad.numpy()) and np.array_equal(db, b.grad.numpy())


@pytest.mark.parametrize("name", ["outer-k65", "outer-k130"])
def test_outer_form_is_autograd_of_relu_then_one_output_linear(name):
    """q = relu(inp W^T + b) . w2, backward with the gradient `vec` of q: the gradient of W is the model's dW when `gout` is the
    ReLU's output.  Multiples of 1/4 for vec and w2: their product is exact, so the one float32 rounding changes nothing."""
    c = m.wgrad_case(name)
    d = m.wgrad_data(c, "exact")
    rng = np.random.default_rng(5)
    W0, b0 = m.eighths(rng, (c["M"], c["N"])), m.eighths(rng, c["M"])
    W, b = T(W0).requires_grad_(), T(b0).requires_grad_()
    a = torch.relu(F.linear(T(d["inp"]), W, b))
    (a @ T(d["outer_w"])).backward(T(d["outer_vec"]))
    act = a.detach().numpy().astype(f32)
    assert 0.2 < (act > 0).mean() < 0.8
    dW, db, _, _ = m.wgrad(act, d["inp"], d["outer_vec"], d["outer_w"])
    assert np.array_equal(dW, W.grad.numpy()) and np.array_equal(db, b.grad.numpy())
    # and the form is the materialised operand of the ordinary problem
    G = m.wgrad_operand(act, d["outer_vec"], d["outer_w"])
    assert np.array_equal(m.wgrad(G.astype(f32), d["inp"])[0], dW)


def test_outer_form_rounds_the_product_once():
    vec, w = np.array([1 + 2.0 ** -23], f32), np.array([1 + 2.0 ** -23], f32)
    A = m.wgrad_operand(np.ones((1, 1), f32), vec, w)
    assert A[0, 0] == float(f32(vec[0] * w[0])) and A[0, 0] != float(vec[0]) * float(w[0])
    assert m.wgrad_operand(np.array([[-0.0, 0.0, -1.0, np.nan]], f32), np.ones(1, f32), np.ones(4, f32)).tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize("name", [c["name"] for c in m.splitrelu_cases() if c["M"] <= 16 and not c["special"] and c["M"]])
def test_split_relu_is_autograd_of_relu_split_cat(name):
    c = m.splitrelu_case(name)
    d = m.splitrelu_data(c)
    M, Cr, Cp = c["M"], sum(c["widths"]), c["Cp"]
    rng = np.random.default_rng(3)
    pre = np.where(d["act"] > 0, d["act"], -np.abs(m.bounded(rng, (M, Cr))))          # act = relu(pre)
    x = T(np.concatenate([pre, m.bounded(rng, (M, Cp))], 1)).requires_grad_()
    h = torch.cat([torch.relu(x[:, :Cr]), x[:, Cr:]], 1)
    blocks = torch.split(h[:, :Cr], list(c["widths"]), dim=1)
    loss = torch.zeros((), dtype=torch.float64)
    for k, blk in enumerate(blocks):
        if d["g"][k] is None:
            continue
        loss = loss + ((blk @ T(d["ow"][k])) * T(d["g"][k])).sum() if d["ow"][k] is not None else loss + (blk * T(d["g"][k])).sum()
    if Cp and d["g_pass"] is not None:
        loss = loss + (h[:, Cr:] * T(d["g_pass"])).sum()
    if loss.requires_grad:
        loss.backward()
    want = x.grad.numpy() if x.grad is not None else np.zeros((M, Cr + Cp))
    got = m.splitrelu_expect(c).astype(f64)
    assert np.allclose(got, want, rtol=2.0 ** -23, atol=0)                          # the one float32 multiply of an outer_w block
    plain = [k for k in range(len(c["widths"])) if k not in c["ow"]]
    start = np.concatenate([[0], np.cumsum(c["widths"])])
    for k in plain:
        assert np.array_equal(got[:, start[k]:start[k + 1]], want[:, start[k]:start[k + 1]])
    assert np.array_equal(got[:, Cr:], want[:, Cr:])


def test_split_relu_special_values():
    c = m.splitrelu_case("b4-ow-none")
    d, out = m.splitrelu_data(c), m.splitrelu_expect(c)
    act = d["act"].reshape(-1)
    assert act[0] == 0 and not np.signbit(act[0]) and np.signbit(act[1]) and act[2] == m.SMALLEST_NORMAL and np.isnan(act[3])
    assert out[0, :4].tolist() == [0.0, 0.0, float(d["g"][2][0, 0]), 0.0] and d["g"][3][0, 0] != 0    # NaN > 0 is false: 0
    assert np.isfinite(out).all()


@pytest.mark.parametrize("name", ["k4-vec", "k68-ld-odd", "k1024-w-off", "rows17-scalar"])
@pytest.mark.parametrize("kind", m.KINDS)
def test_row_dot_is_linear_forward(name, kind):
    c = m.rowdot_case(name)
    d = m.rowdot_data(c, kind)
    y, tol = m.rowdot_expect(c, kind)
    want = F.linear(T(d["x"]), T(d["w"])[None, :], None if d["b"] is None else T(d["b"]))[:, 0].numpy()
    assert np.allclose(y, want, rtol=1e-13, atol=1e-13) and (tol > 0).all()
    if kind == "exact":
        assert np.array_equal(y, want)


# ------------------------------------------------------------------------------------------------ fairness
def _terms_ok_exact(terms_abs_sum, q):
    """every partial sum of terms that are multiples of 2^-q is a float32 when the sum of their magnitudes is < 2^(24 - q)"""
    return bool((terms_abs_sum * 2.0 ** q < 2.0 ** 24).all())


@pytest.mark.parametrize("name", [c["name"] for c in m.wgrad_cases()])
def test_weight_gradient_data_is_fair(name):
    c = m.wgrad_case(name)
    # bounded: operands in [2^-6, 2^3] or exactly 0, tolerance at most 1/64 of the output's largest term
    d = m.wgrad_data(c, "bounded")
    A, X = m.wgrad_operand(d["gout"], d["outer_vec"], d["outer_w"]), d["inp"].astype(f64)
    for v in [np.abs(X)] + ([np.abs(A)] if not c["outer"] else [np.abs(d["outer_vec"]), np.abs(d["outer_w"])]):
        assert ((v >= m.LO) & (v <= m.HI)).all()
    if c["outer"]:
        a = np.abs(A)
        assert (((a >= m.LO ** 2) & (a <= m.HI ** 2)) | (a == 0)).all() and 0.3 < (a == 0).mean() < 0.7
        assert np.signbit(d["gout"][d["gout"] == 0]).any() and not np.signbit(d["gout"][d["gout"] == 0]).all()
    _, _, tW, tb = m.wgrad_expect(c, "bounded")
    largest = np.zeros((c["M"], c["N"]))
    for k in range(c["K"]):                                            # max_k |A[k, m] X[k, n]|
        largest = np.maximum(largest, np.abs(A[k])[:, None] * np.abs(X[k])[None, :])
    assert (tW <= largest / 64).all() and (tb <= np.abs(A).max(0) / 64).all()
    assert ((tW > 0) | (largest == 0)).all()
    # exact: terms nonzero, every partial sum representable
    e = m.wgrad_data(c, "exact")
    Ae, Xe = m.wgrad_operand(e["gout"], e["outer_vec"], e["outer_w"]), e["inp"].astype(f64)
    q = 7 if c["outer"] else 6
    assert (Xe != 0).all() and np.array_equal(Xe * 8, np.round(Xe * 8)) and np.abs(Xe).max() <= 1
    if c["outer"]:
        assert (e["outer_vec"] != 0).all() and (e["outer_w"] != 0).all() and np.array_equal(Ae * 16, np.round(Ae * 16))
        assert ((Ae != 0) == (e["gout"] > 0)).all()
    else:
        assert (Ae != 0).all() and np.array_equal(Ae * 8, np.round(Ae * 8))
    assert np.abs(Ae).max() <= 1 and c["K"] < 2 ** 17
    assert _terms_ok_exact(np.abs(Ae).T @ np.abs(Xe), q) and _terms_ok_exact(np.abs(Ae).sum(0), q - 3)
    dW, db, _, _ = m.wgrad_expect(c, "exact")
    assert np.array_equal(dW.astype(f32).astype(f64), dW) and np.array_equal(db.astype(f32).astype(f64), db)


def test_the_bound_at_the_largest_shape():
    """(2113, 129, 129): the bound is a small multiple of an output's smallest term and a small share of its largest."""
    c = m.wgrad_case("k2113")
    d = m.wgrad_data(c, "bounded")
    _, _, tW, _ = m.wgrad_expect(c, "bounded")
    assert m.wgrad_c(2113) == 65 + 2 + 5 and m.chunks_of(2113) == 34
    A, X = np.abs(d["gout"].astype(f64)), np.abs(d["inp"].astype(f64))
    lo, hi = tW[:8, :8].copy(), tW[:8, :8].copy()
    for i in range(8):
        for j in range(8):
            t = A[:, i] * X[:, j]
            lo[i, j], hi[i, j] = tW[i, j] / t.min(), tW[i, j] / t.max()
    assert lo.max() < 64 and hi.max() < 1 / 64


@pytest.mark.parametrize("name", [c["name"] for c in m.rowdot_cases() if c["rows"] and c["rows"] < 100])
def test_row_dot_data_is_fair(name):
    c = m.rowdot_case(name)
    d = m.rowdot_data(c, "bounded")
    _, tol = m.rowdot_expect(c, "bounded")
    terms = np.abs(d["x"].astype(f64)) * np.abs(d["w"].astype(f64))[None, :]
    assert ((np.abs(d["x"]) >= m.LO) & (np.abs(d["x"]) <= m.HI)).all() and (tol <= terms.max(1) / 64).all()
    e = m.rowdot_data(c, "exact")
    te = np.abs(e["x"].astype(f64)) * np.abs(e["w"].astype(f64))[None, :]
    assert (te != 0).all() and np.array_equal(te * 64, np.round(te * 64))
    assert _terms_ok_exact(te.sum(1) + (0 if e["b"] is None else abs(float(e["b"][0]))), 6)
    assert e["b"] is None or e["b"][0] != 0


# ------------------------------------------------------------------------------------------------ coverage
def test_weight_gradient_table_reaches_every_edge():
    cases = m.wgrad_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    K = {c["K"] for c in cases}
    assert {1, 63, 64, 65, 512, 513, 1536, 1537, 2048, 2049, 2113} <= K
    assert [m.chunks_of(k) for k in (1, 63, 64, 65, 512, 513, 1536, 1537, 2048, 2049, 2113)] == [1, 1, 1, 2, 8, 9, 24, 25, 32, 33, 34]
    assert 2113 % m.CHUNK == 1
    edge = {1, 2, 63, 64, 65, 66, 128, 129}
    plain = [c for c in cases if not c["outer"] and not c["name"].startswith("cap")]
    assert edge <= {c["M"] for c in plain} and edge <= {c["N"] for c in plain}
    assert max(c["K"] * c["M"] * c["N"] for c in cases) == 2113 * 129 * 129 and m.wgrad_case("k2113")["M"] == 129
    for op, off in (("g_ld", "g_off"), ("x_ld", "x_off")):
        assert {c[op] for c in cases} == {"min", "pad4", "even", "odd"} and {c[off] for c in cases} == {0, 1, 2}
    assert {c["dw_pad"] > 0 for c in plain} == {True, False} and {c["bias"] for c in plain} == {True, False}
    outer = [c for c in cases if c["outer"]]
    assert any(c["M"] == 65 for c in outer) and any(c["K"] % m.CHUNK and c["K"] > m.CHUNK for c in outer)
    assert {c["bias"] for c in outer} == {True, False}
    # the reduce grid's cap: exactly 8192 groups of 64 outputs, and one group more
    a, b = m.wgrad_case("cap-exact"), m.wgrad_case("cap-plus")
    assert a["M"] * a["N"] + a["M"] == m.RED_CAP * m.RED_GROUP and a["K"] == b["K"] == 2 and a["bias"] and b["bias"]
    assert 0 < b["M"] * b["N"] + b["M"] - m.RED_CAP * m.RED_GROUP <= m.RED_GROUP
    assert max(m.workspace_floats(c["K"], c["M"], c["N"]) for c in (a, b)) * 4 < 4 << 20


def test_load_width_helper_and_its_coverage():
    assert m.load_width(0, 64, 64, 0) == 16 and m.load_width(0, 68, 65, 0) == 16
    assert m.load_width(0, 68, 65, 1) == 4 and m.load_width(0, 68, 66, 1) == 8            # the ragged tile of a 16-byte operand
    assert m.load_width(1, 64, 64, 0) == 4 and m.load_width(2, 64, 64, 0) == 8 and m.load_width(0, 66, 64, 0) == 8
    assert m.load_width(0, 65, 64, 0) == 4 and m.load_width(2, 2, 2, 0) == 8 and m.load_width(0, 1, 1, 0) == 4
    assert m.load_width(0, 130, 129, 0) == 4                                              # odd length: a pair may straddle the end
    reached = {w for c in m.wgrad_cases() for w in m.wgrad_widths(c)}
    want = {(op, where, w) for op in ("gout", "inp") for where in ("interior", "ragged") for w in (16, 8, 4)}
    # by the rule itself a 16-byte load needs its tile inside the matrix: a ragged tile never takes it
    impossible = {(op, "ragged", 16) for op in ("gout", "inp")}
    assert not (reached & impossible) and reached == want - impossible
    # ... what the table reaches instead: the ragged second tile (65 and 66 columns) next to a 16-byte first tile, both operands
    for op in ("gout", "inp"):
        for cols, w in ((65, 4), (66, 8)):
            assert any(c["M" if op == "gout" else "N"] == cols and [x[2] for x in m.wgrad_widths(c) if x[0] == op] == [16, w]
                       for c in m.wgrad_cases()), (op, cols)


def test_many_sets():
    names = {c["name"] for c in m.wgrad_cases()}
    for s in m.MANY_SETS.values():
        assert set(s) <= names and 1 <= len(s) <= m.MAX_BATCH
    e = [m.wgrad_case(n) for n in m.MANY_SETS["eight"]]
    assert len(e) == m.MAX_BATCH and len({(c["K"], c["M"], c["N"]) for c in e}) == 8
    assert m.MANY_SETS["eight-reversed"] == m.MANY_SETS["eight"][::-1] and len(m.MANY_SETS["one"]) == 1
    tiles = [-(-c["M"] // 64) * -(-c["N"] // 64) for c in e]
    assert any(tiles[i] == 1 and tiles[i - 1] > 1 and tiles[i + 1] > 1 for i in range(1, 7))
    assert any(not e[i]["bias"] and e[i - 1]["bias"] and e[i + 1]["bias"] for i in range(1, 7))
    assert any(c["outer"] for c in e)


def test_row_dot_table():
    cases = m.rowdot_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    assert {c["K"] for c in cases} >= set(m.ROWDOT_K) == {4, 60, 64, 68, 1020, 1024}
    assert {c["rows"] for c in cases} >= {0, 1, 15, 16, 17, 8192 * 16, 8192 * 16 + 1}
    for K in m.ROWDOT_K:
        mine = [c for c in cases if c["K"] == K]
        assert {m.rowdot_vec(c) for c in mine} == {True, False} and {c["bias"] for c in mine} == {True, False}
        scalar = [c for c in mine if not m.rowdot_vec(c)]
        assert any(m.ld_of(K, c["x_ld"]) % 4 for c in scalar) and any(c["x_off"] == 1 for c in scalar) and any(c["w_off"] == 1 for c in scalar)
        assert any(m.rowdot_vec(c) and m.ld_of(K, c["x_ld"]) > K for c in mine)                  # NaN gaps on the vector path
    for lay, (x_ld, x_off, w_off, vec) in m.ROWDOT_LAYOUTS.items():
        assert m.rowdot_vec(dict(K=64, x_ld=x_ld, x_off=x_off, w_off=w_off)) == vec, lay
    for rows in m.ROWDOT_ROWS:
        assert {m.rowdot_vec(c) for c in cases if c["rows"] == rows} == {True, False}


def test_split_relu_table():
    cases = m.splitrelu_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    assert {len(c["widths"]) for c in cases} == {1, 2, 3, 4}
    assert all(any(1 in c["widths"] for c in cases if len(c["widths"]) == n) for n in (1, 2, 3, 4))
    pos = {("first" if k == 0 else "last" if k == len(c["widths"]) - 1 else "inner") for c in cases for k in c["null"]}
    assert pos == {"first", "inner", "last"}
    assert any(not c["ow"] for c in cases) and any(set(c["ow"]) == set(range(len(c["widths"]))) for c in cases)
    assert any(c["ow"] and len(c["ow"]) < len(c["widths"]) for c in cases)
    assert {(c["Cp"] > 0, c["gpass"]) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}
    assert {0, 1, 7} <= {c["M"] for c in cases}
    sizes = {c["M"] * (sum(c["widths"]) + c["Cp"]) for c in cases}
    assert {255, 256, 257, 8192 * 256, 8192 * 256 + 1} <= sizes
    for c in cases:
        g_ld, gp_ld, act_ld, gout_ld = m.splitrelu_strides(c)
        Cr = sum(c["widths"])
        assert gp_ld > c["Cp"] and act_ld > Cr and gout_ld > Cr + c["Cp"]
        assert all(ld == 1 if k in c["ow"] else ld > c["widths"][k] for k, ld in enumerate(g_ld))
    assert sum(c["special"] for c in cases) >= 2
