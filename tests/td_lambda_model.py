"""Float64 model of the TD(lambda) loss launch (``macjd_tdlambda_io``), written from the comment above that struct in
include/macjd_nets.h, not from the kernel.  Plain NumPy float64 on the float32 operands; gamma and lambda are the float32
values the struct carries, widened.  No torch, nothing from the package.

Shared by tests/test_td_lambda_cpu.py (which proves the model against an independent forward view and checks that the
float32 restatements stay inside the bounds) and tests/test_td_lambda_gpu.py (which holds the launch to it): the case
table, the case builder (fixed seeds), the bounds and the tolerances.  u = 2^-24, gamma_k = k u / (1 - k u)
(update_tail_model).

The recursion is the affine map G[t] = a[t] + c[t] G[t+1], a = r + (boot (1 - lam)) tq, c = boot lam, so
G[t] = sum_{j >= t} C[t, j] a[j] with C[t, j] = prod_{t <= i < j} c[i], the sum ending at the chain's stop (c = 0).

Bound of a return (the chain it comes from).  The per-term scale is the sum of ABSOLUTE terms, S[j] = |r[j]| + |boot (1 - lam)
tq[j]|, accumulated through |c|:  A[t] = S[t] + |c[t]| A[t+1]  — not |a|: a cancels, and a bound relative to |a| fails
already for the one-step target.  Roundings met by the term j of G[t], L = j - t <= the steps to the stop:
  a[j]            1 - lambda, boot (1 - lam), the product with tq, the sum with r                        4
  C[t, j]         one rounding per factor c[i] = boot lam, and at most one per product: the chunked scan multiplies
                  composed factors pairwise (6 rounds a chunk, one more where a carry enters)            2 L + spans
  additions       every fused multiply-add the term passes: at most 6 in a chunk's scan + the carry      7 spans
spans = the number of 64-step chunks the chain from t to its stop touches (>= 1).  (The sequential order, one fused
multiply-add per step, passes at most L additions and no product of factors: a term meets 4 + 2 L roundings, below the same
count.)  Hence  E_G[t] = gamma_k A[t],  k = 4 + 2 L + 8 spans.                                              -> ``bounds``
Elementwise:
  gy      scale = 2 / sum(filled) (1 rounding), y - G on the STORED return (E_G + u (|y| + |G|)), the product (1):
          E = scale (E_G + u (|y| + |G|)) filled + 2u |gy|
Sums (additions on the longest path): ceil(B / 16) ceil(Tm1 / 64) per thread + 6 (wave) + 4 (the 16 waves), relative to the sum
of |terms|, plus the terms' own errors: e = (y - G) filled carries E_e = E_G + u (|y| + |G|), e e: 2 |e| E_e + E_e^2 + u e^2.
The quotients add one rounding each.  stats[3], a sum of 0 / 1 below 2^24, is exact.

The ASSERTED tolerance is the project's rule (update_tail_model.param_tolerance): per output min(ceiling, FACTOR x Y), Y = the
worst deviation of the float32 restatement below from this model over that output, never less than one float32 ulp of the
value.  The restatement (``td_lambda_f32``) follows the order csrc/macjd_tdlambda.h states: wave w takes episodes w, w + 16,
..; chunks of 64 steps from the last; six rounds of pairwise composition, fma(c, a', a) skipped where c == 0; G = fma(c, carry,
a); per-thread sums in the order the items are met, a halving tree over the 64 lanes, another over the 16 waves.
``td_lambda_seq_f32`` is the other order (one step at a time from the end); both must reproduce the float64 returns exactly on
the exact cases (gamma = lambda = 1/2, data in eighths, |x| <= 4, a stop at most every 8 steps: every partial result is a
multiple of 2^-19 below 8).
"""
import functools
from collections import namedtuple

import numpy as np

from update_tail_model import FACTOR, U, gamma as gamma_k, td_loss_model  # noqa: F401 (td_loss_model: re-exported)

f32, f64 = np.float32, np.float64
BAR = 1e-5            # the project's bar for a float32 value under another order, relative to the case's max |G|


def _w(x):
    return float(f32(x))


def _stops(terminated, filled):
    """cont [B, Tm1] bool: the chain of step t goes on into step t + 1."""
    term, fill = np.asarray(terminated) != 0, np.asarray(filled) != 0
    cont = np.zeros(term.shape, bool)
    cont[:, :-1] = fill[:, 1:] & ~term[:, :-1]
    return term, fill, cont


# ------------------------------------------------------------------------------------------------ the contract
def td_lambda_model(y, tq, reward, terminated, filled, gamma_, lam, gy_cols=None):
    """y / tq / reward [B, Tm1] float32, terminated / filled [B, Tm1] (non-zero = true).
    -> stats [4] = loss, mean(y), mean(G), sum(filled); gy [B, gy_cols] (columns Tm1.. = +0); G [B, Tm1]."""
    y, tq, r = (np.asarray(a, f32).astype(f64) for a in (y, tq, reward))
    term, fill, cont = _stops(terminated, filled)
    B, Tm1 = y.shape
    g_, l_ = _w(gamma_), _w(lam)
    G = np.zeros((B, Tm1))
    for t in range(Tm1 - 1, -1, -1):
        boot = g_ * (1.0 - term[:, t])
        nxt = G[:, t + 1] if t + 1 < Tm1 else np.zeros(B)
        mix = np.where(cont[:, t], (1.0 - l_) * tq[:, t] + l_ * np.where(cont[:, t], nxt, 0.0), tq[:, t])
        G[:, t] = r[:, t] + boot * mix
    m = fill.astype(f64)
    tot = m.sum()
    e = (y - G) * m
    stats = np.array([(e * e).sum() / tot, y.sum() / (B * Tm1), G.sum() / (B * Tm1), tot])
    gy = np.zeros((B, Tm1 if gy_cols is None else gy_cols))
    gy[:, :Tm1] = 2.0 * m * (y - G) / tot
    return stats, gy, G


# ------------------------------------------------------------------------------------------------ float32 restatements
def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded to float64 and once more
    to float32 (a double rounding in the rare case of a float64 result half-way between two float32)."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _terms_f32(tq, r, term, cont, gamma_, lam):
    g_, l_, one = f32(gamma_), f32(lam), f32(1)
    boot = np.where(term, f32(0), g_).astype(f32)
    k = np.where(cont, boot * (one - l_), boot).astype(f32)
    a = (r + (k * tq).astype(f32)).astype(f32)
    c = np.where(cont, boot * l_, f32(0)).astype(f32)
    return a, c


def _tree(s):
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = (s[..., :h] + s[..., h:]).astype(f32)
    return s[..., 0]


def td_lambda_f32(y, tq, reward, terminated, filled, gamma_, lam, gy_cols=None):
    """The chunked-scan order (module docstring) -> stats [4], gy, G, all float32."""
    y, tq, r = (np.asarray(a, f32) for a in (y, tq, reward))
    term, fill, cont = _stops(terminated, filled)
    B, Tm1 = y.shape
    n_chunks, n_groups = -(-Tm1 // 64), -(-B // 16)
    Tp, Bp = 64 * n_chunks, 16 * n_groups

    def pad(x, value):
        out = np.full((Bp, Tp), value, x.dtype)
        out[:B, :Tm1] = x
        return out

    a, c = _terms_f32(pad(tq, f32(0)), pad(r, f32(0)), pad(term, True), pad(cont, False), gamma_, lam)
    yp, mp = pad(y, f32(0)), pad(fill.astype(f32), f32(0))
    valid = pad(np.ones((B, Tm1), bool), False)
    G = np.zeros((Bp, Tp), f32)
    acc = np.zeros((4, 16, 64), f32)            # filled, e^2, y, G per thread (wave, lane)
    lane = np.arange(64)
    for grp in range(n_groups):
        rows = slice(16 * grp, 16 * grp + 16)
        carry = np.zeros((16, 1), f32)
        for ch in range(n_chunks - 1, -1, -1):
            cols = slice(64 * ch, 64 * ch + 64)
            aa, cc = a[rows, cols].copy(), c[rows, cols].copy()
            k = 1
            while k < 64:
                a2, c2 = np.zeros_like(aa), np.zeros_like(cc)
                a2[:, :64 - k], c2[:, :64 - k] = aa[:, k:], cc[:, k:]
                act = (lane + k < 64)[None, :]
                aa = np.where(act & (cc != 0), _fma(cc, a2, aa), aa)
                cc = np.where(act, (cc * c2).astype(f32), cc)
                k *= 2
            g = np.where(cc != 0, _fma(cc, np.broadcast_to(carry, cc.shape), aa), aa).astype(f32)
            carry = g[:, :1].copy()
            G[rows, cols] = g
            v = valid[rows, cols]
            e = ((yp[rows, cols] - g).astype(f32) * mp[rows, cols]).astype(f32)
            for i, term_ in enumerate((mp[rows, cols], (e * e).astype(f32), yp[rows, cols], g)):
                acc[i] = np.where(v, (acc[i] + term_).astype(f32), acc[i])
    tot4 = _tree(_tree(acc))                     # the 64 lanes, then the 16 waves
    tot, M = tot4[0], f32(B * Tm1)
    stats = np.array([tot4[1] / tot, tot4[2] / M, tot4[3] / M, tot], f32)
    G = G[:B, :Tm1]
    gy = np.zeros((B, Tm1 if gy_cols is None else gy_cols), f32)
    gy[:, :Tm1] = ((f32(2) / tot) * fill.astype(f32) * (y - G).astype(f32)).astype(f32)
    return stats, gy, G


def td_lambda_seq_f32(tq, reward, terminated, filled, gamma_, lam):
    """The sequential order: G[t] = fma(c[t], G[t+1], a[t]) from the end, skipped where c == 0 -> G float32."""
    tq, r = np.asarray(tq, f32), np.asarray(reward, f32)
    term, _, cont = _stops(terminated, filled)
    a, c = _terms_f32(tq, r, term, cont, gamma_, lam)
    G = np.zeros(tq.shape, f32)
    nxt = np.zeros(tq.shape[0], f32)
    for t in range(tq.shape[1] - 1, -1, -1):
        nxt = np.where(c[:, t] != 0, _fma(c[:, t], nxt, a[:, t]), a[:, t]).astype(f32)
        G[:, t] = nxt
    return G


# ------------------------------------------------------------------------------------------------ bounds
def bounds(y, tq, reward, terminated, filled, gamma_, lam):
    """-> (E_stats [4], E_gy [B, Tm1], E_G [B, Tm1]): the ceilings of the module docstring around td_lambda_model."""
    y, tq, r = (np.asarray(a, f32).astype(f64) for a in (y, tq, reward))
    term, fill, cont = _stops(terminated, filled)
    B, Tm1 = y.shape
    g_, l_ = _w(gamma_), _w(lam)
    boot = g_ * (1.0 - term)
    S = np.abs(r) + np.abs(np.where(cont, boot * (1.0 - l_), boot) * tq)
    c = np.where(cont, boot * l_, 0.0)
    A, L = np.zeros((B, Tm1)), np.zeros((B, Tm1), np.int64)
    for t in range(Tm1 - 1, -1, -1):
        go = cont[:, t] & (c[:, t] != 0)
        A[:, t] = S[:, t] + (np.abs(c[:, t]) * A[:, t + 1] if t + 1 < Tm1 else 0.0) * go
        L[:, t] = np.where(go, (L[:, t + 1] if t + 1 < Tm1 else 0) + 1, 0)
    t_idx = np.arange(Tm1)[None, :]
    spans = (t_idx + L) // 64 - t_idx // 64 + 1
    e_g = gamma_k(4 + 2 * L + 8 * spans) * A
    _, gy, G = td_lambda_model(y, tq, reward, terminated, filled, gamma_, lam)
    m = fill.astype(f64)
    tot, M = m.sum(), B * Tm1
    e_e = (e_g + U * (np.abs(y) + np.abs(G))) * m
    e_gy = (2.0 / tot) * e_e + 2 * U * np.abs(gy)
    chain = gamma_k(-(-B // 16) * -(-Tm1 // 64) + 6 + 4)
    e = (y - G) * m
    loss = (e * e).sum() / tot
    sum_e2 = chain * (e * e).sum() + (2 * np.abs(e) * e_e + e_e ** 2 + U * e * e).sum()
    e_stats = np.array([sum_e2 / tot + U * loss,
                        chain * np.abs(y).sum() / M + U * abs(y.sum() / M),
                        (chain * np.abs(G).sum() + e_g.sum()) / M + U * abs(G.sum() / M),
                        0.0])
    return e_stats, e_gy, e_g


def tolerance(ceiling, restated, model):
    """min(ceiling, FACTOR x Y), Y = max |float32 restatement - model| over the output, at least one float32 ulp of the value."""
    model = np.asarray(model, f64)
    y = float(np.abs(np.asarray(restated, f64) - model).max())
    return np.maximum(np.minimum(ceiling, FACTOR * y), np.spacing(np.abs(model).astype(f32)).astype(f64))


def stats_tolerance(ceiling, restated, model):
    """The same rule for the four scalars, each its own output (stats[3] is exact: tolerance 0)."""
    tol = np.array([tolerance(ceiling[i], restated[i], model[i]) for i in range(4)], f64)
    tol[3] = 0.0
    return tol


# ------------------------------------------------------------------------------------------------ cases
# mask: "all"; "ragged" unfilled tails; "term" terminated mid-episode (filled goes on behind it); "hole" one unfilled step inside a
# filled run; "deadrow" one all-unfilled row beside filled ones; "exact" the exact cases' stops.
# layout (how the C-ABI test lays the operands out): "dense"; "sliced" = [:, :-1] / [:, 1:] slices of [B, Tm1 + 1, 1] tensors;
# "strided" = padded rows, reward / terminated / filled at step strides 2 / 3 / 2 with live bytes in between.
Case = namedtuple("Case", "name B Tm1 lam gamma mask gy_extra layout exact")
MASKS = ["all", "ragged", "term", "hole", "deadrow", "exact"]


def _case(B, Tm1, lam, gamma_, mask, gy_extra, layout):
    exact = mask == "exact"
    return Case(f"b{B}-t{Tm1}-l{lam:g}-g{gamma_:g}-{mask}-x{gy_extra}-{layout}", B, Tm1, lam, gamma_, mask, gy_extra, layout, exact)


CASES = [
    _case(1, 1, 0.8, 0.99, "all", 0, "dense"),
    _case(2, 2, 0.5, 0.99, "ragged", 1, "sliced"),
    _case(16, 63, 0.8, 0.99, "term", 5, "strided"),
    _case(17, 64, 1.0, 0.99, "hole", 0, "sliced"),
    _case(33, 65, 0.8, 1.0, "ragged", 1, "strided"),
    _case(2, 128, 0.5, 1.0, "term", 5, "dense"),
    _case(17, 129, 1.0, 1.0, "all", 0, "sliced"),
    _case(33, 200, 0.8, 0.99, "deadrow", 1, "dense"),
    _case(1, 200, 1.0, 0.99, "all", 5, "strided"),
    _case(32, 99, 0.8, 0.99, "ragged", 0, "sliced"),          # the learner's own shape
    _case(17, 200, 0.0, 0.99, "hole", 0, "strided"),
    _case(3, 65, 0.0, 1.0, "deadrow", 5, "sliced"),
    _case(16, 128, 1.0, 0.99, "term", 1, "sliced"),
] + [_case(B, Tm1, 0.5, 0.5, "exact", x, lay) for B, Tm1, x, lay in [
    (1, 1, 0, "dense"), (2, 2, 1, "sliced"), (17, 64, 5, "strided"), (16, 65, 0, "sliced"), (33, 129, 1, "dense"),
    (17, 200, 5, "sliced"), (32, 99, 0, "strided"), (1, 63, 1, "dense"), (2, 128, 0, "strided")]]
EXACT_SHAPES = [(1, 1), (2, 3), (5, 63), (16, 64), (17, 65), (32, 99), (3, 128), (33, 129), (17, 200)]


def _rng(*key):
    return np.random.default_rng([ord(k) if isinstance(k, str) else int(k) for k in key])


@functools.lru_cache(maxsize=None)
def inputs(B, Tm1, mask, salt=0):
    """dict(y, tq, reward float32 [B, Tm1]; terminated, filled uint8 [B, Tm1]), at least one filled step."""
    rng = _rng(1201, B, Tm1, MASKS.index(mask), salt)
    t = np.arange(Tm1)[None, :]
    if mask == "exact":
        y, tq, reward = (rng.integers(-32, 33, (B, Tm1)).astype(f32) / f32(8) for _ in range(3))
        terminated, filled = np.zeros((B, Tm1), np.uint8), np.ones((B, Tm1), np.uint8)
        for b in range(B):
            s = int(rng.integers(0, 8))
            while s < Tm1:
                if s + 1 < Tm1 and rng.random() < 0.5:
                    filled[b, s + 1] = 0            # stop in front of an unfilled step
                else:
                    terminated[b, s] = 1
                s += int(rng.integers(1, 9))
        filled[0, 0] = 1
        reward[0, 0] = f32(3.875)                   # (no case whose returns are all zero)
    else:
        y, tq, reward = ((s * rng.standard_normal((B, Tm1))).astype(f32) for s in (3.0, 3.0, 1.0))
        terminated, filled = np.zeros((B, Tm1), np.uint8), np.ones((B, Tm1), np.uint8)
        if mask == "ragged":
            length = rng.integers(0 if B > 1 else 1, Tm1 + 1, (B, 1))
            length[0, 0] = max(1, Tm1 // 2)
            filled = (t < length).astype(np.uint8)
            terminated = (t == length - 1).astype(np.uint8)
        elif mask == "term":
            at = rng.integers(0, Tm1, (B, 1))
            terminated = ((t == at) | (rng.random((B, Tm1)) < 0.03)).astype(np.uint8)
        elif mask == "hole":
            at = rng.integers(0, Tm1, (B, 1))
            filled = ((t != at) | (Tm1 == 1)).astype(np.uint8)
            filled[0, 0] = 1
        elif mask == "deadrow":
            filled[B // 2] = 0
            terminated[:, Tm1 - 1] = 1
    assert filled.sum() >= 1
    return dict(y=y, tq=tq, reward=reward, terminated=terminated, filled=filled)


def case_args(case, salt=0):
    d = inputs(case.B, case.Tm1, case.mask, salt)
    return (d["y"], d["tq"], d["reward"], d["terminated"], d["filled"], case.gamma, case.lam)


@functools.lru_cache(maxsize=None)
def expectation(case):
    """Model outputs, float32 restatement and tolerances of one case, computed once:
    dict(stats, gy, G: (value, tolerance); restated: (stats, gy, G) float32; ceilings)."""
    args = case_args(case)
    cols = case.Tm1 + case.gy_extra
    stats, gy, G = td_lambda_model(*args, gy_cols=cols)
    r_stats, r_gy, r_G = td_lambda_f32(*args, gy_cols=cols)
    e_stats, e_gy, e_g = bounds(*args)
    T = case.Tm1
    tol_gy = np.zeros(gy.shape)
    tol_gy[:, :T] = tolerance(e_gy, r_gy[:, :T], gy[:, :T]) * (np.asarray(args[4]) != 0)   # unfilled: exactly zero
    return dict(stats=(stats, stats_tolerance(e_stats, r_stats, stats)), gy=(gy, tol_gy), G=(G, tolerance(e_g, r_G, G)),
                restated=(r_stats, r_gy, r_G), ceilings=(e_stats, e_gy, e_g))
