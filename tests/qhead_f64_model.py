"""Float64 model of the update's Q-head launches, written from the contract in include/macjd_nets.h
(``macjd_qtaken_io``, ``macjd_doubleq_io``, ``macjd_wgrad_io.outer_vec``) and the reference lines cited there
(core/networks.py:131-180 one_hot / cat / Linear / ReLU / Linear; core/qmix.py:138-147 arg-max over the eval values,
gather from the target values) — not from the kernels.  Plain NumPy float64 on the float32 operands.

Also here, shared by tests/test_qhead_f64_cpu.py (which proves the model and the fairness of the inputs) and
tests/test_qhead_f64_gpu.py (which holds the kernels to it): the case lists, the case builders (fixed seeds; h ~ 0.7 N(0,1),
P ~ U(0,1), W1 ~ 0.3 N(0,1), b1 ~ 0.3 N(0,1), w2 ~ N(0,1) / sqrt(H), b2 ~ 0.3 N(0,1)), the tie cases and the tolerances.

Tolerances of act / q / out.  Hard ceiling, componentwise worst case of any float32 evaluation order:
    E_act = gamma_(H+4) (|W1[:, :H]| |h| + |b1| + |W1[:, H+a]| + |W1[:, H+A] P|)
    E_q   = |w2| E_act + gamma_(H+2) (|w2| act + |b2|)          gamma_k = k u / (1 - k u), u = 2^-24
(ReLU is 1-Lipschitz, so no mask decision enters).  The ceiling is loose (~1e-3 on O(1) values); the ASSERTED tolerance is
min(ceiling, 8 Y) per case and tensor, Y = the worst |float32 oracle - this model| of that tensor over 256 yardstick rows
drawn with the case's weights (oracle/nets_oracle.py: the reference's formulation in float32).  The kernels and the oracle
make the same count of float32 roundings in another order; Y is computed on the CPU from oracle and model alone."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

from _harness import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import nets_oracle  # noqa: E402  (test infrastructure)

U = 2.0 ** -24
INT32_MIN = -2 ** 31
BIG64 = 2 ** 33 + 1          # an int64 action index that is no int32 value (its low 32 bits say 1)
YARD_ROWS = 256
FACTOR = 8.0                 # asserted tolerance = min(ceiling, FACTOR x Y)
GAP = 4.0                    # fairness: top-two gaps and tie leads exceed GAP x tolerance
f32, f64 = np.float32, np.float64


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ the contract
def onehot(idx, A):
    """[n, A] float32; the block of a row is empty for idx outside [0, A) — compared as int64, never narrowed."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    return (idx[:, None] == np.arange(A, dtype=np.int64)[None, :]).astype(f32)


def taken(h, idx, P, W1, b1, w2, b2, A):
    """-> x [n, H + A + 1] float32 (exact), pre, act [n, H], q [n] in float64."""
    n = h.shape[0]
    x = np.concatenate([np.asarray(h, f32), onehot(idx, A), np.asarray(P, f32).reshape(n, 1)], axis=1)
    pre = x.astype(f64) @ np.asarray(W1, f64).T + np.asarray(b1, f64)
    act = np.maximum(pre, 0.0)
    q = (act * np.asarray(w2, f64).reshape(1, -1)).sum(axis=1) + (0.0 if b2 is None else float(np.asarray(b2, f64).reshape(-1)[0]))
    return x, pre, act, q


def _pre_all(h, P_rows, W1, b1, A):
    H = h.shape[1]
    W1 = np.asarray(W1, f64)
    base = np.asarray(h, f64) @ W1[:, :H].T + np.asarray(b1, f64)                       # [n, H]
    return base[:, None, :] + W1[:, H:H + A].T[None] + np.asarray(P_rows, f64)[:, :, None] * W1[:, H + A][None, None, :]


def all_actions(h, P_rows, W1, b1, w2, b2, A):
    """Q(h[n], a, P_rows[n, a]) for every a: [n, A] float64."""
    act = np.maximum(_pre_all(h, P_rows, W1, b1, A), 0.0)
    return (act * np.asarray(w2, f64).reshape(1, 1, -1)).sum(axis=2) + float(np.asarray(b2, f64).reshape(-1)[0])


def map_rows(n, row_map):
    """P row read by row 0 .. n-1 under the optional (p_group, p_inner) map of macjd_doubleq_io."""
    r = np.arange(n, dtype=np.int64)
    if row_map is None:
        return r
    g, i = row_map
    return (r // g) * i + r % i


def double_q(h_e, h_t, P_e, P_t, head_e, head_t, A, row_map=None):
    """-> q_e, q_t [n, A], the FIRST-maximum arg-max of q_e [n] (torch.argmax / np.argmax), q_t[n, arg-max]."""
    rows = map_rows(h_e.shape[0], row_map)
    q_e = all_actions(h_e, np.asarray(P_e)[rows], *head_e, A)
    q_t = all_actions(h_t, np.asarray(P_t)[rows], *head_t, A)
    am = np.argmax(q_e, axis=1)
    return q_e, q_t, am, q_t[np.arange(q_t.shape[0]), am]


def qhead_grads(x32, act32, gq32, w2_32):
    """Parameter gradients of Linear-ReLU-Linear(1) from the taken launch's saved operands, as the weight-gradient launches
    with ``outer_vec`` form them: g_hid[k, m] = float32(gq[k] w2[m]) where act32[k, m] > 0 else 0 (ONE rounding, the mask
    from the float32 operand: no decision), everything else float64.  -> values and the matching sums of |terms|."""
    x, act = np.asarray(x32, f32).astype(f64), np.asarray(act32, f32)
    gq, w2 = np.asarray(gq32, f32).reshape(-1), np.asarray(w2_32, f32).reshape(-1)
    g_hid = np.where(act > 0, gq[:, None] * w2[None, :], f32(0)).astype(f32).astype(f64)
    gq, a64 = gq.astype(f64), act.astype(f64)
    val = {"dW1": g_hid.T @ x, "db1": g_hid.sum(axis=0), "dw2": gq @ a64, "db2": gq.sum()}
    mag = {"dW1": np.abs(g_hid).T @ np.abs(x), "db1": np.abs(g_hid).sum(axis=0), "dw2": np.abs(gq) @ np.abs(a64),
           "db2": np.abs(gq).sum()}
    return val, mag


# ------------------------------------------------------------------------------------------------ ceilings
def ceiling_taken(h, idx, P, W1, b1, w2, b2, A):
    """(E_act [n, H], E_q [n]) of the module docstring."""
    H = h.shape[1]
    aW, ah = np.abs(np.asarray(W1, f64)), np.abs(np.asarray(h, f64))
    col = onehot(idx, A).astype(f64) @ aW[:, H:H + A].T                                  # |W1[:, H + a]| or 0
    e_act = gamma(H + 4) * (ah @ aW[:, :H].T + np.abs(np.asarray(b1, f64)) + col + np.abs(np.asarray(P, f64)).reshape(-1, 1) * aW[:, H + A])
    _, _, act, _ = taken(h, idx, P, W1, b1, w2, b2, A)
    aw2 = np.abs(np.asarray(w2, f64)).reshape(-1)
    ab2 = 0.0 if b2 is None else abs(float(np.asarray(b2).reshape(-1)[0]))
    return e_act, e_act @ aw2 + gamma(H + 2) * (act @ aw2 + ab2)


def ceiling_all(h, P_rows, W1, b1, w2, b2, A):
    """E_q [n, A] of the all-action head."""
    H = h.shape[1]
    aW, ah = np.abs(np.asarray(W1, f64)), np.abs(np.asarray(h, f64))
    base = ah @ aW[:, :H].T + np.abs(np.asarray(b1, f64))
    e_act = gamma(H + 4) * (base[:, None, :] + aW[:, H:H + A].T[None] + np.abs(np.asarray(P_rows, f64))[:, :, None] * aW[:, H + A])
    act = np.maximum(_pre_all(h, P_rows, W1, b1, A), 0.0)
    aw2 = np.abs(np.asarray(w2, f64)).reshape(-1)
    return e_act @ aw2 + gamma(H + 2) * (act @ aw2 + abs(float(np.asarray(b2).reshape(-1)[0])))


# ------------------------------------------------------------------------------------------------ cases
TakenCase = namedtuple("TakenCase", "n A idx_size h_ld w1_pad act_ld x_pad b2 seed")     # x_pad None: x = NULL
DqCase = namedtuple("DqCase", "H A n h_pad h_off shared p_pad row_map argmax seed")
TieCase = namedtuple("TieCase", "H A cls n seed")
WgradCase = namedtuple("WgradCase", "K A x_ld act_ld dw_pad seed")

H64 = 64
# every n with two values of A; every A, index width, h_ld, w1_ld, act_ld, x_ld / NULL and b2 / NULL occurs
TAKEN_CASES = [
    TakenCase(1, 1, 4, 64, 0, 64, 0, True, 1), TakenCase(1, 64, 8, 68, 3, 67, 2, False, 1),
    TakenCase(15, 5, 8, 64, 3, 67, None, True, 1), TakenCase(15, 33, 4, 68, 0, 64, 2, True, 1),
    TakenCase(16, 9, 4, 68, 3, 64, 0, False, 1), TakenCase(16, 64, 8, 64, 0, 67, None, True, 1),
    TakenCase(17, 1, 8, 68, 3, 67, 2, True, 1), TakenCase(17, 5, 4, 64, 0, 64, 0, True, 1),
    TakenCase(31, 9, 8, 64, 0, 67, 2, True, 1), TakenCase(31, 33, 4, 68, 3, 64, None, False, 1),
    TakenCase(32, 5, 4, 68, 3, 67, 0, True, 1), TakenCase(32, 64, 8, 64, 0, 64, 2, True, 1),
    TakenCase(33, 9, 8, 68, 0, 64, None, True, 1), TakenCase(33, 1, 4, 64, 3, 67, 0, False, 1),
    TakenCase(65, 33, 8, 64, 3, 67, 0, True, 1), TakenCase(65, 9, 4, 68, 0, 64, 2, True, 1),
]
MAP = (6, 2)     # (T J, J)
DQ_CASES = [
    DqCase(64, 5, 1, 0, 0, True, 0, None, True, 1), DqCase(64, 9, 15, 3, 1, False, 2, None, True, 1),
    DqCase(64, 17, 16, 0, 1, False, 0, None, False, 1), DqCase(64, 33, 17, 3, 1, True, 2, MAP, True, 1),
    DqCase(64, 5, 33, 3, 1, False, 2, None, True, 1), DqCase(64, 33, 33, 0, 0, False, 0, None, True, 1),
    DqCase(64, 9, 17, 0, 1, True, 0, MAP, False, 1), DqCase(64, 17, 1, 3, 1, False, 2, None, True, 1),
    DqCase(128, 5, 17, 3, 1, False, 2, MAP, True, 1), DqCase(128, 9, 33, 0, 0, True, 0, None, True, 1),
    DqCase(128, 17, 1, 3, 1, False, 2, None, False, 1), DqCase(128, 17, 16, 0, 1, True, 0, None, True, 1),
    DqCase(128, 9, 15, 3, 1, False, 2, None, True, 1), DqCase(128, 5, 33, 0, 1, False, 0, None, True, 1),
]
TIE_CASES = [TieCase(H, A, cls, 33, 1) for H, A in ((64, 5), (64, 33), (128, 9)) for cls in "abcd"]
PAIR_CASES = [(33, 17), (1, 65), (0, 16), (32, 0)]     # (n_taken, n_dq) at A = 9
# x_ld: N (8-byte loads), 72 at N = 70 (16-byte loads on the first column tile), N + 1 (4-byte loads)
WGRAD_CASES = [
    WgradCase(1, 5, 72, 64, 0, 1), WgradCase(1, 9, 75, 67, 0, 1), WgradCase(63, 5, 70, 67, 0, 1), WgradCase(63, 33, 99, 64, 0, 1),
    WgradCase(64, 9, 74, 64, 3, 1), WgradCase(64, 5, 71, 67, 0, 1), WgradCase(65, 33, 98, 67, 0, 1), WgradCase(65, 5, 72, 64, 0, 1),
    WgradCase(129, 9, 75, 64, 0, 1), WgradCase(129, 33, 98, 67, 0, 1), WgradCase(129, 5, 70, 64, 0, 1),
]


def tie_pair(A, cls):
    """The tied action pair of a class; AH = (A + 1) / 2 is where macjd_qhead_double_q splits the actions over two waves."""
    AH = (A + 1) // 2
    return {"a": (0, AH - 1), "b": (AH - 1, AH), "c": (AH, A - 1), "d": (0, A - 1)}[cls]


def _rng(*key):
    """Generator seeded by a tuple of ints and one-letter strings (fixed: no hash() of the interpreter enters)."""
    return np.random.default_rng([ord(k) if isinstance(k, str) else int(k) for k in key])


def head(rng, H, A):
    """(W1 [H, H + A + 1], b1 [H], w2 [H], b2 [1]) float32."""
    n = lambda *s: rng.standard_normal(s)
    return ((0.3 * n(H, H + A + 1)).astype(f32), (0.3 * n(H)).astype(f32), (n(H) / np.sqrt(H)).astype(f32), (0.3 * n(1)).astype(f32))


def _rows(rng, n, H):
    return (0.7 * rng.standard_normal((n, H))).astype(f32)


@functools.lru_cache(maxsize=None)
def taken_inputs(case):
    """dict(h, idx int64 [n], P [n], W1, b1, w2, b2 or None).  idx holds -1, A, INT32_MIN (and 2^33 + 1 at 8 bytes) where
    the rows are there for them; with one row the 8-byte case takes 2^33 + 1."""
    rng = _rng(101, case.n, case.A, case.idx_size, case.seed)
    W1, b1, w2, b2 = head(rng, H64, case.A)
    h, P = _rows(rng, case.n, H64), rng.random(case.n).astype(f32)
    idx = rng.integers(0, case.A, case.n).astype(np.int64)
    if case.n >= 15:
        idx[1], idx[case.n - 1], idx[case.n // 2] = -1, case.A, INT32_MIN
        if case.idx_size == 8:
            idx[3] = BIG64
    elif case.idx_size == 8:
        idx[0] = BIG64
    return dict(h=h, idx=idx, P=P, W1=W1, b1=b1, w2=w2, b2=b2 if case.b2 else None)


def _dq_common(rng, H, A, n, shared, row_map):
    n_p = n if row_map is None else int(map_rows(n, row_map).max()) + 1
    h_e = _rows(rng, n, H)
    h_t = h_e if shared else _rows(rng, n, H)
    return dict(h_e=h_e, h_t=h_t, P_e=rng.random((n_p, A)).astype(f32), P_t=rng.random((n_p, A)).astype(f32),
                head_e=head(rng, H, A), head_t=head(rng, H, A))


@functools.lru_cache(maxsize=None)
def dq_inputs(case):
    rng = _rng(202, case.H, case.A, case.n, case.seed)
    return _dq_common(rng, case.H, case.A, case.n, case.shared, case.row_map)


TIE_BOOST = 0.08


@functools.lru_cache(maxsize=None)
def tie_inputs(case):
    """Random case whose eval head has BIT-IDENTICAL W1 columns for the pair's actions and P_e equal on them, so that the
    two values come out of identical instruction sequences; class d: every action column identical, P_e constant along a
    row.  The shared column leans towards w2 (TIE_BOOST) so that the pair is the maximum on enough rows."""
    H, A = case.H, case.A
    rng = _rng(303, H, A, case.cls, case.seed)
    d = _dq_common(rng, H, A, case.n, False, None)
    W1, b1, w2, b2 = d["head_e"]
    W1, P_e = W1.copy(), d["P_e"].copy()
    a, a2 = tie_pair(A, case.cls)
    if case.cls == "d":
        W1[:, H:H + A] = W1[:, H:H + 1]
        P_e[:] = P_e[:, :1]
    else:
        W1[:, H + a] = (W1[:, H + a] + f32(TIE_BOOST * np.sqrt(H)) * w2).astype(f32)
        W1[:, H + a2] = W1[:, H + a]
        P_e[:, a2] = P_e[:, a]
    d["head_e"], d["P_e"], d["pair"] = (W1, b1, w2, b2), P_e, (a, a2)
    return d


def tie_rows(case):
    """Rows on which the tied actions are the float64 maximum and lead the best other action by more than GAP x tolerance
    (class d: every row — there is no other action)."""
    d = tie_inputs(case)
    q_e, _, _, _ = double_q(d["h_e"], d["h_t"], d["P_e"], d["P_t"], d["head_e"], d["head_t"], case.A)
    a, a2 = d["pair"]
    assert np.array_equal(q_e[:, a], q_e[:, a2])
    if case.cls == "d":
        return np.arange(case.n)
    others = np.delete(q_e, [a, a2], axis=1).max(axis=1)
    return np.nonzero(q_e[:, a] - others > GAP * tolerance(case, "q").max(axis=1))[0]


@functools.lru_cache(maxsize=None)
def wgrad_inputs(case):
    """The taken launch's inputs at n = K rows (its x and act are the weight-gradient operands) and gq [K]."""
    rng = _rng(404, case.K, case.A, case.seed)
    W1, b1, w2, b2 = head(rng, H64, case.A)
    return dict(h=_rows(rng, case.K, H64), idx=rng.integers(0, case.A, case.K).astype(np.int64), P=rng.random(case.K).astype(f32),
                W1=W1, b1=b1, w2=w2, b2=b2, gq=rng.standard_normal(case.K).astype(f32))


# ------------------------------------------------------------------------------------------------ tolerances
def _oracle_sd(W1, b1, w2, b2, A):
    b2 = np.zeros(1, f32) if b2 is None else np.asarray(b2, f32).reshape(1)
    return {"actor.4.bias": np.zeros(A, f32), "fc2_q_head.0.weight": W1, "fc2_q_head.0.bias": b1,
            "fc2_q_head.2.weight": np.asarray(w2, f32).reshape(1, -1), "fc2_q_head.2.bias": b2}


@functools.lru_cache(maxsize=None)
def yardstick(case):
    """Y per tensor: worst |float32 oracle - model| over YARD_ROWS rows drawn with the case's weights."""
    rng = _rng(505, *[v for v in case[:4] if isinstance(v, (int, str))])
    if isinstance(case, TakenCase):
        d = taken_inputs(case)
        H, A = H64, case.A
        h, idx, P = _rows(rng, YARD_ROWS, H), rng.integers(0, A, YARD_ROWS), rng.random(YARD_ROWS).astype(f32)
        sd = _oracle_sd(d["W1"], d["b1"], d["w2"], d["b2"], A)
        x, _, act, q = taken(h, idx, P, d["W1"], d["b1"], d["w2"], d["b2"], A)
        act32 = np.maximum(nets_oracle._linear(x, d["W1"], d["b1"]), 0)                  # networks.py:171-176, first layer
        q32 = nets_oracle.q_value_for_action(sd, h, idx, P)[:, 0]
        return {"act": float(np.abs(act32 - act).max()), "q": float(np.abs(q32 - q).max())}
    d = tie_inputs(case) if isinstance(case, TieCase) else dq_inputs(case)
    H, A = case.H, case.A
    h, P = _rows(rng, YARD_ROWS, H), rng.random((YARD_ROWS, A)).astype(f32)
    out = {}
    for name, hd in (("q", d["head_e"]), ("out", d["head_t"])):
        q32 = nets_oracle.q_all_actions(_oracle_sd(*hd, A), h, P)
        out[name] = float(np.abs(q32 - all_actions(h, P, *hd, A)).max())
    return out


def ceiling(case, tensor):
    if isinstance(case, TakenCase):
        d = taken_inputs(case)
        e_act, e_q = ceiling_taken(d["h"], d["idx"], d["P"], d["W1"], d["b1"], d["w2"], d["b2"], case.A)
        return {"act": e_act, "q": e_q}[tensor]
    tie = isinstance(case, TieCase)
    d = tie_inputs(case) if tie else dq_inputs(case)
    rows = map_rows(case.n, None if tie else case.row_map)
    if tensor == "q":
        return ceiling_all(d["h_e"], d["P_e"][rows], *d["head_e"], case.A)
    return ceiling_all(d["h_t"], d["P_t"][rows], *d["head_t"], case.A)


def tolerance(case, tensor):
    """min(ceiling, FACTOR x Y) per element.  Taken cases: "act" [n, H], "q" [n]; Double-DQN and tie cases: "q" (the eval
    head's values) and "out" (the target head's), both [n, A] — the launch's out[n] is held to column arg-max of "out"."""
    return np.minimum(ceiling(case, tensor), FACTOR * yardstick(case)[tensor])
