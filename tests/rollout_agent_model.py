"""Float64 model of the rollout's agent launches, written from the contract in include/macjd_nets.h (``macjd_mlp_io``,
``macjd_qhead_io``, ``macjd_agent_episode_io``, ``macjd_agent_episode_seq_io``) — not from the kernels — and the case tables
that tests/test_rollout_agent_cpu.py proves fair and tests/test_mlp_f64_gpu.py, tests/test_qhead_select_f64_gpu.py and
tests/test_agent_episode_f64_gpu.py run.  Plain NumPy; it shares no code with the package.  Reused test models:
tests/gru_scan_model.py (gate expressions, FLOOR_H, FLOOR_P), tests_golden_helpers.philox4x32_10 (pinned on the Random123
known answers).

Every operation takes ``dt``: float64 is the model, float32 the RESTATEMENT (np.float32 throughout, sums in k order).

Tolerances, u = 2^-24, gamma_k = k u / (1 - k u):
* ``mlp``: running forward bound  err_l = gamma(K16_l + 2) (|W_l| (|a_(l-1)| + err_(l-1)) + |b_l|) + |W_l| err_(l-1)  (K16 =
  K rounded up to 16: the products with the zero pad columns are exact but the chain has that length; + 2: bias and slack),
  times the activation's Lipschitz constant (ReLU, none: 1; sigmoid: 1/4), plus the sigmoid's own rounding, 2 ulp of 2^-23
  = gru_scan_model.FLOOR_P (libm expf and IEEE division are no worse than one ulp each: csrc/macjd_gru_math.h, DESIGN 4.3 and
  the derivation in tests/gru_scan_model.py).  ReLU is 1-Lipschitz, so no side of a ReLU is ever excluded.
* ``qhead_all``: gamma(H + 4) sum |terms|, terms = |w2| (|base| + |W1[:, H + a]| + |W1[:, H + A] P_a|) and |b2| (+ |w2| times
  the error of a base that the launch computed itself: gamma(H + 2) (|W1[:, :H]| |h| + |b1|)).
* every asserted tolerance is min(bound, cap), cap = 1e-5 max(1, max|ref|), the project's parity bar.
* gates and free-running trajectories: tol = min(cap, max(FLOOR_H, 8 x the restatement's deviation)) (gru_scan_model's rule;
  FLOOR_H = 12.5 ulp is derived there).
Discrete outputs: an exploring row is decided by integers and must equal the model; a greedy row is BINDING when the model's
masked leader (all actions whose float64 value equals the maximum exactly: constructed ties) leads the best other available
action by more than 4 x tol(Q) — the launch must then choose the lowest index of the leader — otherwise it may choose the
leader or the runner-up.  At most 0.5 % of a case's greedy rows may be non-binding (asserted on the CPU from the model alone).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gru_scan_model as gm  # noqa: E402
from tests_golden_helpers import philox4x32_10  # noqa: E402

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
CAP = 1e-5
FACTOR = 8.0
GAP = 4.0
NONBINDING_SHARE = 0.005
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2          # MACJD_ACT_*
SIGMOID_ROUNDING = gm.FLOOR_P                      # 2 ulp of 2^-23
M32 = 0xFFFFFFFF


def gamma(k):
    return k * U / (1.0 - k * U)


def cap(ref):
    ref = np.asarray(ref, f64)
    return CAP * max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)


def _rng(*key):
    return np.random.default_rng([ord(c) for k in key for c in str(k)] or [0])


def ksum32(a, W, b):
    """float32 a [n, K] @ W [N, K]^T + b with the sum taken in k order, every operation rounded to float32."""
    a, W = np.asarray(a, f32), np.asarray(W, f32)
    acc = np.zeros((a.shape[0], W.shape[0]), f32)
    for k in range(W.shape[1]):
        acc = acc + a[:, k:k + 1] * W[:, k][None, :]
    return acc + np.asarray(b, f32)[None, :]


# ---------------------------------------------------------------------------------------------------- macjd_mlp_io
def mlp(x, layers, dt=f64):
    """layers = [(W [N, K], b [N], act)] -> (y [n, N_last], err [n, N_last]); err is the bound of the module docstring (zeros
    for the float32 restatement)."""
    a = np.asarray(x, dt)
    err = np.zeros(a.shape, f64)
    for W, b, act in layers:
        if dt is f32:
            z = ksum32(a, W, b)
        else:
            W64, b64 = np.asarray(W, f64), np.asarray(b, f64)
            z = a @ W64.T + b64
            K16 = (W64.shape[1] + 15) & ~15
            aW = np.abs(W64)
            err = gamma(K16 + 2) * ((np.abs(a) + err) @ aW.T + np.abs(b64)) + err @ aW.T
        if act == ACT_RELU:
            a = np.maximum(z, dt(0))
        elif act == ACT_SIGMOID:
            a = gm.sigmoid(z).astype(dt)
            err = 0.25 * err + SIGMOID_ROUNDING
        else:
            a = z
    return a, err


def _pitch(width):
    return ((width + 7) // 16) * 16 + 8


def mlp_form(dims):
    """"resident" / "staged" / "unsupported" by the limits of the header: dims[0] <= 256, hidden <= 128, last <= 384, tile
    counts in {1,2,3,4,8,12,24}, padded weight images (+ four 16-row activation strips) against 160 KB of LDS."""
    L = len(dims) - 1
    imgs = []
    for l in range(L):
        K, N = dims[l], dims[l + 1]
        if (l == 0 and K > 256) or (l > 0 and K > 128) or (l < L - 1 and N > 128) or N > 384 or (N + 15) // 16 not in (1, 2, 3, 4, 8, 12, 24):
            return "unsupported"
        n16 = (N + 15) & ~15
        imgs.append(n16 * _pitch((K + 15) & ~15) + n16)
    budget = 160 * 1024 // 4 - 4 * 16 * _pitch((max(dims[:-1]) + 15) & ~15)
    if sum(imgs) <= budget:
        return "resident"
    return "staged" if max(imgs) <= budget else "unsupported"


RES, STAGED = (46, 64, 192), (184, 128, 128, 33)
RES_ACTS, STAGED_ACTS = (ACT_RELU, ACT_NONE), (ACT_RELU, ACT_RELU, ACT_SIGMOID)
MLP_ROWS = (1, 15, 16, 17, 63, 64, 65, 16384, 16385, 16449)
MLP_K0 = (1, 3, 15, 16, 17, 64, 65, 252, 255, 256)
MLP_N_ANY = (1, 9, 16, 17, 33, 48, 49, 64, 113, 128)
MLP_N_LAST = (177, 192, 369, 384)
MLP_UNSUPPORTED = [(20, 80), (20, 96), (20, 112), (20, 144), (20, 176), (20, 208), (20, 368), (20, 65), (20, 112, 16), (20, 193),
                   (257, 16), (20, 129, 16), (24, 128, 384)]
ACTS = (ACT_NONE, ACT_RELU, ACT_SIGMOID)


def _mc(name, rows, dims, acts, x_off=0, w_off=0, x_ld="min", y_pad=0):
    return dict(name=name, rows=rows, dims=tuple(dims), acts=tuple(acts), x_off=x_off, w_off=w_off, x_ld=x_ld, y_pad=y_pad)


def mlp_cases():
    """x_off / w_off: float offset of x / of every W from a 16-byte boundary (1: the 4-byte DMA is taken); x_ld "min" = K,
    "pad" = K + 4 (+ 1 when x_off: odd), 0 = one broadcast row; y_pad: y_ld - N."""
    c = []
    for i, rows in enumerate(MLP_ROWS):
        c.append(_mc(f"rows{rows}-resident", rows, RES, RES_ACTS, y_pad=3 * (i % 2)))
        c.append(_mc(f"rows{rows}-staged", rows, STAGED, STAGED_ACTS, x_ld="pad" if i % 2 else "min", y_pad=2 * ((i + 1) % 2)))
    c.append(_mc("rows49153-onelayer", 3 * 16384 + 1, (16, 16), (ACT_RELU,)))
    c.append(_mc("rows16449-linear-resident", 16449, RES, (ACT_NONE, ACT_NONE)))      # no ReLU: a NaN row stays NaN on chip
    for K in MLP_K0:
        c.append(_mc(f"k{K}-aligned", 65, (K, 48, 9), (ACT_RELU, ACT_NONE)))
        c.append(_mc(f"k{K}-xodd", 65, (K, 48, 9), (ACT_RELU, ACT_NONE), x_off=1, x_ld="pad"))
        c.append(_mc(f"k{K}-wodd", 65, (K, 48, 9), (ACT_RELU, ACT_NONE), w_off=1))
    for N in MLP_N_ANY:
        c.append(_mc(f"n{N}-inner", 33, (20, N, 16), (ACT_RELU, ACT_NONE)))
        c.append(_mc(f"n{N}-last", 33, (20, N), (ACT_NONE,), y_pad=1))
    for N in MLP_N_LAST:
        c.append(_mc(f"n{N}-last", 33, (20, N), (ACT_RELU,)))
    for a0 in ACTS:
        for a1 in ACTS:
            c.append(_mc(f"act{a0}{a1}", 33, (20, 9, 20), (a0, a1)))
    c.append(_mc("act-sigmoid-3layers", 17, (20, 9, 17, 5), (ACT_SIGMOID, ACT_SIGMOID, ACT_NONE)))
    c.append(_mc("bcast-resident", 130, RES, RES_ACTS, x_ld=0, y_pad=5))
    c.append(_mc("bcast-staged", 65, STAGED, STAGED_ACTS, x_ld=0))
    c.append(_mc("bcast-xodd", 65, (65, 48, 9), (ACT_RELU, ACT_SIGMOID), x_off=1, x_ld=0))
    return c


# pairs of case names (macjd_mlp_forward_pair)
MLP_PAIRS = [("rows65-resident", "rows65-staged"), ("rows1-staged", "rows16449-resident"), ("rows1-resident", "rows16449-staged"),
             ("rows17-staged", "rows17-staged")]


def mlp_case(name):
    return next(c for c in mlp_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _mlp_data(name):
    c = mlp_case(name)
    rng = _rng("mlp", name)
    K0 = c["dims"][0]
    n_x = 1 if c["x_ld"] == 0 else c["rows"]
    x = rng.standard_normal((n_x, K0)).astype(f32)
    layers = []
    for l, act in enumerate(c["acts"]):
        K, N = c["dims"][l], c["dims"][l + 1]
        s = 1.0 / np.sqrt(K)
        layers.append((rng.uniform(-s, s, (N, K)).astype(f32), rng.uniform(-s, s, N).astype(f32), act))
    return x, layers


def mlp_data(c):
    return _mlp_data(c["name"])


@functools.lru_cache(maxsize=None)
def _mlp_expect(name):
    c = mlp_case(name)
    x, layers = _mlp_data(name)
    xr = np.broadcast_to(x, (c["rows"], x.shape[1])) if c["x_ld"] == 0 else x
    y, err = mlp(xr, layers)
    return y, np.minimum(err, cap(y))


def mlp_expect(c):
    """(model y [rows, N], asserted tolerance [rows, N] = min(bound, cap))."""
    return _mlp_expect(c["name"])


def mlp_restated_rows(c):
    """Rows on which the CPU test evaluates the float32 restatement (all of a small case, both ends of a large one)."""
    n = c["rows"]
    return np.arange(n) if n <= 200 else np.r_[0:70, n - 90:n]


# ---------------------------------------------------------------------------------------------------- macjd_qhead_io
def qhead_all(base, P, W1, w2, b2, base_err=None, dt=f64):
    """Q [n, A] = w2 . ReLU(base + W1[:, H + a] + W1[:, H + A] P_a) + b2 for every action, and its bound."""
    base, P, W1 = np.asarray(base, dt), np.asarray(P, dt), np.asarray(W1, dt)
    w2, b2 = np.asarray(w2, dt).reshape(-1), dt(np.asarray(b2, dt).reshape(-1)[0])
    H, A = base.shape[1], P.shape[1]
    q = np.zeros((base.shape[0], A), dt)
    mag = np.zeros((base.shape[0], A), f64)
    for h in range(H):                                    # k order; float64: any order
        t = base[:, h:h + 1] + W1[h, H:H + A][None, :]
        t = np.maximum(t + P * W1[h, H + A], dt(0))
        q = q + t * w2[h]
        mag += abs(float(w2[h])) * (np.abs(base[:, h:h + 1]).astype(f64) + np.abs(W1[h, H:H + A][None, :].astype(f64))
                                    + np.abs(P.astype(f64) * float(W1[h, H + A])))
    q = q + b2
    err = gamma(H + 4) * (mag + abs(float(b2)))
    if base_err is not None:
        err = err + (np.asarray(base_err, f64) @ np.abs(w2.astype(f64)))[:, None]
    return q, err


def qhead_base(h, W1, b1, dt=f64):
    """base = W1[:, :H] h + b1 and the bound gamma(H + 2) (|W1[:, :H]| |h| + |b1|) of a float32 evaluation."""
    H = np.asarray(h).shape[1]
    W = np.asarray(W1)[:, :H]
    if dt is f32:
        return ksum32(h, W, b1), None
    h64, W64, b64 = np.asarray(h, f64), np.asarray(W, f64), np.asarray(b1, f64)
    return h64 @ W64.T + b64, gamma(H + 2) * (np.abs(h64) @ np.abs(W64).T + np.abs(b64))


def draw(n, counter, seed):
    """Philox words (v0, v1) of rows n: counter words (n lo, n hi, counter lo, counter hi), key (seed lo, seed hi)."""
    n = np.asarray(n, np.uint64)
    counter, seed = int(counter) % 2 ** 64, int(seed) % 2 ** 64
    z = np.zeros(n.shape, np.uint64)
    v = philox4x32_10((n & np.uint64(M32), n >> np.uint64(32), z + np.uint64(counter & M32), z + np.uint64(counter >> 32)),
                      (seed & M32, seed >> 32))
    return np.asarray(v[0], np.uint64), np.asarray(v[1], np.uint64)


def select(q, avail, eps, seed, counter, n, greedy_only, tol=None):
    """The selection stage for rows n with values q [rows, A] and mask avail [rows, A] (bool; None: all available).
    -> dict: greedy (masked first arg-max; 0 when nothing is available), explore [rows] bool, action [rows] (the rule's
    choice), runner (best available action outside the leader, -1: none), lead (leader's value - runner's; inf: none),
    binding (lead > GAP x max tol of the row; only with ``tol``)."""
    q = np.asarray(q, f64)
    rows, A = q.shape
    av = np.ones((rows, A), bool) if avail is None else np.asarray(avail, bool)
    qm = np.where(av, q, -np.inf)
    greedy = np.argmax(qm, axis=1)                       # first maximum; all -inf: 0
    top = qm[np.arange(rows), greedy]
    rest = np.where(qm == top[:, None], -np.inf, qm)     # everything but the leader (exact ties are ONE leader)
    runner = np.where(np.isfinite(rest.max(axis=1)), np.argmax(rest, axis=1), -1)
    with np.errstate(invalid="ignore"):
        lead = np.where(runner >= 0, top - rest.max(axis=1), np.inf)
    n_avail = av.sum(axis=1)
    lead = np.where(n_avail == 0, np.inf, lead)          # nothing available: action 0 whatever the values
    eps32 = float(f32(eps))
    explore = np.zeros(rows, bool)
    action = greedy.copy()
    if not greedy_only and eps32 > 0.0:
        v0, v1 = draw(n, counter, seed)
        explore = (v0 >> np.uint64(8)).astype(f64) < eps32 * 2.0 ** 24     # exact: (v0 >> 8) 2^-24 < eps in float32
        pool = np.where(n_avail > 0, n_avail, A).astype(np.uint64)
        k = ((v1 * pool) >> np.uint64(32)).astype(np.int64)
        pick_from = np.where((n_avail > 0)[:, None], av, True)
        order = np.cumsum(pick_from, axis=1) - 1          # rank of every eligible action in index order
        kth = np.argmax(pick_from & (order == k[:, None]), axis=1)
        action = np.where(explore, kth, greedy)
    out = dict(greedy=greedy, explore=explore, action=action, runner=runner, lead=lead)
    if tol is not None:
        out["binding"] = lead > GAP * np.broadcast_to(np.asarray(tol, f64), q.shape).max(axis=1)
    return out


def check_choice(sel, chosen):
    """-> (ok [rows] bool, nonbinding [rows] bool) for the launch's choice under the rule of the module docstring."""
    chosen = np.asarray(chosen, np.int64).reshape(-1)
    exact = sel["explore"] | sel["binding"]
    ok = np.where(exact, chosen == sel["action"], (chosen == sel["greedy"]) | (chosen == sel["runner"]))
    return ok, ~sel["explore"] & ~sel["binding"]


def head(rng, H, A, w1_pad=0):
    """Q-head at torch's default scale x 3 (tests/test_episode_h128_gpu.py), the action columns x 4 more: W1 [H, H+A+1+pad],
    b1 [H], w2 [H], b2 [1]."""
    s1, s2 = 3.0 / np.sqrt(H + A + 1), 3.0 / np.sqrt(H)
    W1 = rng.uniform(-s1, s1, (H, H + A + 1 + w1_pad)).astype(f32)
    W1[:, H:H + A] *= f32(4.0)
    return W1, rng.uniform(-s1, s1, H).astype(f32), rng.uniform(-s2, s2, H).astype(f32), rng.uniform(-s2, s2, 1).astype(f32)


TIES = ("first", "last", "masked", "all")


def make_tie(kind, W1, P, avail, H, A, w2):
    """Bit-identical action columns and powers (so the launch's values are bitwise equal) on every row; the tied actions'
    column leans towards w2 so that they lead on most rows.  -> the tied actions."""
    pair = {"first": (0, 1), "last": (A - 2, A - 1), "masked": (0, 2), "all": tuple(range(A))}[kind]
    if kind == "all":
        W1[:, H:H + A] = W1[:, H:H + 1]
        P[:] = P[:, :1]
    else:
        a, a2 = pair
        W1[:, H + a] = (W1[:, H + a] + f32(3.0) * np.sign(w2)).astype(f32)
        W1[:, H + a2] = W1[:, H + a]
        P[:, a2] = P[:, a]
        if avail is not None:
            avail[:, [a, a2]] = True
            if kind == "masked":
                avail[:, 1] = False
                W1[:, H + 1] = (W1[:, H + a] + f32(1.0) * np.sign(w2)).astype(f32)   # the masked action would win
    return pair


def make_avail(rng, E, J, A, only_last=False):
    """[E, J, A] bool: ~70 % available; row 0 of the flattened rows nothing, row 1 exactly one (when there are that many)."""
    av = rng.random((E, J, A)) < 0.7
    flat = av.reshape(E * J, A)
    if only_last:
        flat[::2] = False
        flat[::2, A - 1] = True
    flat[0] = False
    if E * J > 1:
        flat[1] = False
        flat[1, A // 2] = True
    return av


def _qc(name, rows, H, A, na=1, base="vec", avail="i32", outs=("Q", "T32", "T64", "P", "argmax", "gather"), t_layout="ej",
        eps=0.3, eps_dev=False, counter=7, counter_dev=None, seed=11, greedy_only=0, tie=None, w1_pad=0, salt=0):
    """salt: re-draws a case's data (the tables must meet the non-binding share; the CPU test asserts it from the model alone)."""
    return dict(salt=salt, name=name, rows=rows, H=H, A=A, na=na, base=base, avail=avail, outs=tuple(outs), t_layout=t_layout, eps=eps,
                eps_dev=eps_dev, counter=counter, counter_dev=counter_dev, seed=seed, greedy_only=greedy_only, tie=tie, w1_pad=w1_pad)


QS_A_COMPILED, QS_A_GENERIC = (1, 2, 5, 7, 9, 17, 33), (6, 34, 64)
QS_H = (8, 16, 17, 20, 64, 128)


def qs_cases():
    """base: "vec" (16-byte aligned, base_ld = H rounded up to 4), "oddld" (base_ld = H + 1 or + 3: odd), "oddoff" (one float
    off 16 bytes); avail: None / "i32" / "i64" / "perm32" / "perm64" (strides over [A, J, E]); t_layout: "ej" ([E, J, 1]
    strides) or "je" (agent-major)."""
    c = [_qc("rows1", 1, 64, 5), _qc("rows64", 64, 64, 5, avail="i64"), _qc("rows65", 65, 64, 5, na=5, avail="perm32"),
         _qc("rows63", 63, 64, 9, na=3, avail="perm64", t_layout="je"), _qc("rows129", 129, 64, 9, na=3, w1_pad=3),
         _qc("rows60-12agents", 60, 64, 33, na=12, t_layout="je"),
         _qc("onelane-65537", 65537, 16, 5, eps=0.3, seed=2 ** 40 + 5), _qc("onelane-h8", 70, 8, 7, na=1)]
    for H in QS_H:
        c.append(_qc(f"h{H}-vec", 65, H, 9))
    c += [_qc("h17-oddld", 65, 17, 9, base="oddld"), _qc("h64-oddld", 65, 64, 9, base="oddld"),
          _qc("h20-oddoff", 65, 20, 9, base="oddoff"), _qc("h128-oddoff", 65, 128, 9, base="oddoff"),
          _qc("h8-oddoff", 70, 8, 5, base="oddoff")]
    for A in QS_A_COMPILED + QS_A_GENERIC:
        c.append(_qc(f"a{A}", 66, 64, A, na=3, avail="i64" if A % 2 else "i32", eps=0.5))
    c.append(_qc("a64-onelane", 70, 8, 64, avail="i64", eps=0.5))
    for outs in (("Q",), ("T32",), ("T64",), ("T32", "P"), ("argmax",), ("gather",)):
        c.append(_qc("only-" + "-".join(outs), 65, 64, 9, na=5, outs=outs, t_layout="je" if outs == ("T64",) else "ej"))
    c.append(_qc("no-mask", 65, 64, 9, avail=None))
    for eps in (0.0, 0.3, 1.0):
        c.append(_qc(f"eps{eps}", 130, 64, 9, na=2, eps=eps))
        c.append(_qc(f"eps{eps}-dev", 130, 64, 9, na=2, eps=eps, eps_dev=True, salt=1))
    c.append(_qc("counter-carry", 130, 64, 9, na=2, eps=1.0, counter=2 ** 32 - 3, counter_dev=5, seed=2 ** 33 + 12345))
    c.append(_qc("counter-dev-zero", 130, 64, 9, na=2, eps=1.0, counter=2 ** 32 + 2, counter_dev=0, seed=2 ** 33 + 12345))
    c.append(_qc("greedy-only-eps1", 130, 64, 9, na=2, eps=1.0, greedy_only=1))
    for tie in TIES:
        c.append(_qc(f"tie-{tie}-split", 65, 64, 9, tie=tie, eps=0.0))
        c.append(_qc(f"tie-{tie}-onelane", 70, 8, 6, tie=tie, eps=0.0))
    return c


def qs_case(name):
    return next(c for c in qs_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _qs_data(name):
    c = qs_case(name)
    rng = _rng("qs", name, c["salt"])
    N, H, A, na = c["rows"], c["H"], c["A"], c["na"]
    E = N // na
    assert E * na == N
    W1, _, w2, b2 = head(rng, H, A, c["w1_pad"])
    base = rng.standard_normal((N, H)).astype(f32)
    P = rng.random((N, A)).astype(f32)
    avail = None if c["avail"] is None else make_avail(rng, E, na, A, only_last=(A == 64))
    pair = None
    if c["tie"]:
        pair = make_tie(c["tie"], W1, P, None if avail is None else avail.reshape(N, A), H, A, w2)
    gather = rng.integers(0, A, N).astype(np.int64)
    gather[0] = 0
    gather[N // 2] = A - 1
    if N >= 60:
        gather[3], gather[5], gather[7] = -1, A, 2 ** 33
    return dict(base=base, P=P, W1=W1, w2=w2, b2=b2, avail=avail, gather=gather, pair=pair)


def qs_data(c):
    return _qs_data(c["name"])


@functools.lru_cache(maxsize=None)
def _qs_expect(name):
    c = qs_case(name)
    d = _qs_data(name)
    N, A = c["rows"], c["A"]
    q, err = qhead_all(d["base"], d["P"], d["W1"], d["w2"], d["b2"])
    tol = np.minimum(err, cap(q))
    av = None if d["avail"] is None else d["avail"].reshape(N, A)
    eps = c["eps"]
    counter = c["counter"] + (c["counter_dev"] or 0)
    sel = select(q, av, eps, c["seed"], counter, np.arange(N), c["greedy_only"], tol=tol)
    plain = select(q, None, 0.0, 0, 0, np.arange(N), 1, tol=tol)        # argmax_out: unmasked first maximum
    g = d["gather"]
    inside = (g >= 0) & (g < A)
    q_gather = np.where(inside, q[np.arange(N), np.where(inside, g, 0)], 0.0)
    return dict(q=q, tol=tol, sel=sel, plain=plain, q_gather=q_gather, gather_tol=np.where(inside, tol[np.arange(N), np.where(inside, g, 0)], 0.0))


def qs_expect(c):
    return _qs_expect(c["name"])


# ---------------------------------------------------------------------------------------- macjd_agent_episode(_seq)_io
def gru_cell(gi, h, w_hh, b_hh, dt=f64):
    """torch.nn.GRUCell behind its input transform: gate order r, z, n; b_hh of n inside r * (...)."""
    gh = ksum32(h, w_hh, b_hh) if dt is f32 else np.asarray(h, f64) @ np.asarray(w_hh, f64).T + np.asarray(b_hh, f64)
    return gm.gru_step(np.asarray(gi, dt), gh, np.asarray(h, dt), dt)


def episode_step(c, d, t, h_prev, dt=f64):
    """h_t of step t from the hidden state h_prev [N, H] (teacher-forced: the launch's own stored h_(t-1))."""
    gi, _ = step_inputs(c, d, t)
    return gru_cell(gi, h_prev, d["w_hh"], d["b_hh"], dt)


def step_inputs(c, d, t):
    """(gi [N, 3H], P [N, A]) of step t, rows expanded."""
    N = c["E"] * c["J"]
    gi, P = d["gi"], d["P"]
    gi = gi[t if gi.shape[0] > 1 else 0]
    P = P[t if P.shape[0] > 1 else 0]
    return np.broadcast_to(gi, (N, gi.shape[1])), np.broadcast_to(P, (N, P.shape[1]))


def step_choice(c, d, t, h_t):
    """Q-head and selection of step t on the hidden state h_t (float32 values: the launch's stored state or the model's)."""
    N, A = c["E"] * c["J"], c["A"]
    _, P = step_inputs(c, d, t)
    base, base_err = qhead_base(np.asarray(h_t, f32), d["W1"], d["b1"])
    q, err = qhead_all(base, P, d["W1"][:, :c["H"] + A + 1], d["w2"], d["b2"], base_err=base_err)
    tol = np.minimum(err, cap(q))
    av = None if d["avail"] is None else d["avail"].reshape(N, A)
    greedy_only = c["eps"] is None
    eps = 0.0 if greedy_only else c["eps"][t]
    cb = 0 if c["counter_base"] is None else c["counter_base"]
    sel = select(q, av, eps, c["seed"], cb + t + 1, np.arange(N), greedy_only, tol=tol)
    return q, tol, sel, P


def episode(c, d, dt=f64):
    """Free-running hidden trajectory [T, N, H] from h0."""
    N, H = c["E"] * c["J"], c["H"]
    h = np.zeros((N, H), dt) if d["h0"] is None else np.asarray(d["h0"], dt)
    out = np.zeros((c["T"], N, H), dt)
    for t in range(c["T"]):
        h = episode_step(c, d, t, h, dt)
        out[t] = h
    return out


def hidden_tolerances(c, d):
    """(teacher-forced tol, free-running tol, worst restatement deviation of either): the rule of the module docstring with the
    restatement taken along the MODEL's trajectory — one step from the model's float32-rounded h_(t-1), and the whole episode."""
    model = episode(c, d)
    dev_free = float(np.abs(episode(c, d, f32).astype(f64) - model).max())
    N, H = c["E"] * c["J"], c["H"]
    prev = np.zeros((N, H), f32) if d["h0"] is None else np.asarray(d["h0"], f32)
    dev_step = 0.0
    for t in range(c["T"]):
        dev_step = max(dev_step, float(np.abs(episode_step(c, d, t, prev, f32).astype(f64) - episode_step(c, d, t, prev)).max()))
        prev = model[t].astype(f32)
    rule = lambda dev: min(cap(model), max(gm.FLOOR_H, FACTOR * dev))
    return rule(dev_step), rule(dev_free), max(dev_step, dev_free)


ONE_TILE = [(64, 2, 5), (64, 3, 9), (64, 6, 17), (64, 2, 17), (64, 6, 5), (128, 2, 5), (128, 2, 9), (128, 3, 5), (128, 3, 9)]
ONE_TILE_E = (1, 15, 16, 17, 33)
FLAT = [(1, 5, 1), (1, 5, 63), (1, 5, 64), (1, 5, 65), (4, 9, 15), (4, 9, 16), (4, 9, 17), (5, 17, 13), (12, 33, 1), (12, 33, 5),
        (12, 33, 6), (12, 33, 16), (3, 33, 22)]
SEQ_SIZES = [(64, 2, 5), (64, 3, 9), (64, 6, 17), (128, 2, 5), (128, 3, 9)]
EP_T = (1, 2, 3, 7)
EP_GI_LD = ("0", "min", "pad4", "odd")
EP_P_LD = ("0", "min", "pad3")
EP_AVAIL = (None, "i32", "i64", "perm32")
EP_EPS = ("mixed", "greedy", "ones")
EP_COUNTER = (None, 1000, 2 ** 32 - 2)
SEQ_MODES = ("zero", "block", "padded", "frame", "full")


def _ec(name, H, J, A, E, i, seq=None):
    """Case number i takes option i mod len(options) of every list: the lists have pairwise different lengths where it
    matters, and the coverage test checks what the table reaches."""
    T = EP_T[i % 4]
    eps_kind = EP_EPS[i % 3]
    eps = None if eps_kind == "greedy" else ([1.0] * T if eps_kind == "ones" else [(0.0, 0.3, 1.0)[(i + k) % 3] for k in range(T)])
    return dict(name=name, H=H, J=J, A=A, E=E, T=T, gi_ld=EP_GI_LD[(i // 2) % 4], p_ld=EP_P_LD[(i // 3) % 3], h0=bool(i % 2),
                w1_pad=5 * ((i // 2) % 2), w1_off=(i // 3) % 2, avail=EP_AVAIL[(i + i // 4) % 4], eps=eps,
                counter_base=EP_COUNTER[(i + i // 3) % 3], seed=2 ** 35 + 17 * i + 1, h_final=bool((i // 2 + 1) % 2 or T == 1), seq=seq)


def ep_cases():
    c, i = [], 0
    for H, J, A in ONE_TILE:
        for E in ONE_TILE_E:
            c.append(_ec(f"tile-h{H}-j{J}-a{A}-e{E}", H, J, A, E, i))
            i += 1
    for J, A, E in FLAT:
        c.append(_ec(f"flat-j{J}-a{A}-e{E}", 64, J, A, E, i))
        i += 1
    return c


def seq_cases():
    """seq: "zero" (both time strides 0), "block" (the row block), "padded" (row block + 7 / + 3), "frame" (gi_ld = p_ld = 0,
    gi_lt = 3H, p_lt = A: one row per step), "full" (per row and step, minimal strides)."""
    c, i = [], 100
    for H, J, A in SEQ_SIZES:
        for k, mode in enumerate(SEQ_MODES):
            e = _ec(f"seq-h{H}-j{J}-a{A}-{mode}", H, J, A, (17, 1, 16, 33, 15)[k], i, seq=mode)
            e["T"] = (3, 2, 3, 7, 2)[k]
            if e["eps"] is not None:
                e["eps"] = [(1.0, 0.3, 0.0)[(i + t) % 3] for t in range(e["T"])]
            if mode == "frame":
                e["gi_ld"], e["p_ld"] = "0", "0"
            elif mode == "full":
                e["gi_ld"], e["p_ld"] = "min", "min"
            c.append(e)
            i += 1
    return c


def all_ep_cases():
    return ep_cases() + seq_cases()


def ep_case(name):
    return next(c for c in all_ep_cases() if c["name"] == name)


def ep_is_flat(c):
    return c["H"] == 64 and (c["J"] not in (2, 3, 6) or c["A"] == 33)


@functools.lru_cache(maxsize=None)
def _ep_data(name):
    c = ep_case(name)
    rng = _rng("ep", name)
    H, J, A, E, T = c["H"], c["J"], c["A"], c["E"], c["T"]
    N = E * J
    s = 1.0 / np.sqrt(H)
    W1, b1, w2, b2 = head(rng, H, A, c["w1_pad"])
    steps = T if c["seq"] in ("block", "padded", "frame", "full") else 1
    gi = rng.standard_normal((steps, 1 if c["gi_ld"] == "0" else N, 3 * H)).astype(f32)
    P = rng.random((steps, 1 if c["p_ld"] == "0" else N, A)).astype(f32)
    h0 = np.clip(0.5 * rng.standard_normal((N, H)), -0.99, 0.99).astype(f32) if c["h0"] else None
    avail = None if c["avail"] is None else make_avail(rng, E, J, A)
    return dict(gi=gi, P=P, h0=h0, w_hh=rng.uniform(-s, s, (3 * H, H)).astype(f32), b_hh=rng.uniform(-s, s, 3 * H).astype(f32),
                W1=W1, b1=b1, w2=w2, b2=b2, avail=avail)


def ep_data(c):
    return _ep_data(c["name"])


@functools.lru_cache(maxsize=None)
def _ep_fair(name):
    c = ep_case(name)
    d = _ep_data(name)
    tol_step, tol_free, dev = hidden_tolerances(c, d)
    model = episode(c, d)
    greedy = nonbinding = 0
    for t in range(c["T"]):
        _, _, sel, _ = step_choice(c, d, t, model[t].astype(f32))
        greedy += int((~sel["explore"]).sum())
        nonbinding += int((~sel["explore"] & ~sel["binding"]).sum())
    return dict(tol_step=tol_step, tol_free=tol_free, dev=dev, greedy=greedy, nonbinding=nonbinding, model=model)


def ep_fair(c):
    """Tolerances, the model's free-running trajectory and the count of non-binding greedy rows along it."""
    return _ep_fair(c["name"])
