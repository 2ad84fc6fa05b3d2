"""Float64 model of the tail of the update chain — the TD loss (``macjd_tdloss_io``), the LayerNorm parameter gradients
(``macjd_lnparam_io``) and gradient clipping + Adam (``macjd_adam_io``) — written from the comments above those structs
in include/macjd_nets.h, not from the kernels.  Plain NumPy float64 on the float32 operands; the hyper-parameters are the
float32 values the structs carry, widened (so is the 1e-6 of the clip coefficient, which the header's formula adds in
float32).  No torch, nothing from the package.

Shared by tests/test_update_tail_cpu.py (which proves the model against float64 torch and checks that the float32
restatement of the same formulas stays inside the bounds below) and tests/test_update_tail_gpu.py (which holds the
launches to it): the case lists, the case builders (fixed seeds) and the bounds.  u = 2^-24, gamma_k = k u / (1 - k u).

Summation chains (additions on the longest path of one sum; a fused multiply-add counts once):
  squared norm   ceil(n / (256 blocks)) per thread (blocks = min(ceil(n / 256), 256) workgroups, grid-stride), 6 across the
                 wave, 2 across the four waves; then the sum of the P partials:
                   two-launch step / _sample / _ln   one wave: ceil(P / 64) + 6          (P = blocks, or blocks + K)
                   _reduced                          ceil(P / 256) + 6 + 2
                 bound: x = gamma_chain (a sum of non-negative terms: relative), plus whatever error the terms themselves
                 carry, over the sum; the square root turns x into x / (1 + sqrt(1 - x)) (half of it), plus 2u for the root
                 and the margin of the halving.                                             -> ``norm_rel_bound``
  dgamma/dbeta   ceil(C / 256) fused multiply-adds per thread + 6 + 2:  gamma_chain x sum_c |W[c, k] G[c, k]|  (|W| |gb|)
                 The _ln launch squares the values it STORED: their error enters its norm as 2 |d| E + E^2 per element,
                 plus 2 roundings of the partial d_gamma^2 + d_beta^2.                       -> ``ln_bounds``
  TD sums        ceil(M / 1024) per thread + 6 (wave) + 4 (the 16 waves), relative to the sum of |terms|, plus the
                 roundings of a term itself, first order:  target = r + gamma (1 - term) tq : 2 roundings, E_t = 2u A_t,
                 A_t = |r| + |gamma tq|;  e = (y - target) m : E_e = 3u A_e, A_e = |y| + A_t;  e e : 2 |e| E_e + u e^2.
                 The quotients (loss, the two means) add one rounding each.                  -> ``td_bounds``
Elementwise (counted from the expressions; rho_c = relative error of the clip coefficient = norm bound + 2u):
  gy             scale = 2 / sum(filled) (1 rounding), y - target (E_e), the product (1):  E = scale (3u A_e) + 2u |gy|
  clipped grad   one product:  E_g = |g| (rho_c + u)
  m              m + (1 - b1)(g - m), 1 - b1 exact in float32:  d = g - m, p = (1 - b1) d, m' = m + p, a rounding each
  v              v b2 + ((1 - b2) g) g:  four products / one sum, a rounding each, E_g carried through g twice
                                                                                             -> ``adam_bounds``
  param          param - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps)), bc = 1 - pow(beta, step): how accurately the device
                 evaluates powf is not known here.  The CEILING assumes POW_ULPS float32 ulps for it and carries every
                 rounding of the expression to first order (times CEIL_SLACK for the neglected second-order terms; the
                 relative errors involved stay below 1e-3).  The ASSERTED tolerance is the project's rule
                 (tests/qhead_f64_model.py): min(ceiling, FACTOR x Y) per element, Y = the worst deviation of the float32
                 restatement below from this model over the tensor, never less than one float32 ulp of the value.
                                                                                             -> ``param_tolerance``
The float32 restatement (``*_f32``) evaluates the same formulas in np.float32, its sums in lanes and a halving tree no
longer than the chains above."""
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FACTOR = 8.0          # asserted tolerance = min(ceiling, FACTOR x Y): the project's margin for another order on the device
POW_ULPS = 16.0       # the ceiling's assumption on powf
CEIL_SLACK = 1.001
ADAM_BLOCKS = 256     # workgroup cap of the optimiser launches (grid-stride beyond 256 x 256 = 65536 elements)
f32, f64 = np.float32, np.float64
CLIP_EPS = f32(1e-6)


def gamma(k):
    return k * U / (1.0 - k * U)


def _w(x):
    """float32 value of a hyper-parameter, widened."""
    return float(f32(x))


# ------------------------------------------------------------------------------------------------ the contract
def td_loss_model(y, tq, reward, terminated, filled, gamma_, gy_cols=None):
    """y / tq / reward [B, Tm1] float32, terminated / filled [B, Tm1] (non-zero = true).
    -> stats [4] = loss, mean(y), mean(target), sum(filled); gy [B, gy_cols], columns Tm1.. = +0."""
    y, tq, r = (np.asarray(a, f32).astype(f64) for a in (y, tq, reward))
    term, m = (np.asarray(terminated) != 0).astype(f64), (np.asarray(filled) != 0).astype(f64)
    B, Tm1 = y.shape
    target = r + _w(gamma_) * (1.0 - term) * tq
    tot = m.sum()
    e = (y - target) * m
    stats = np.array([(e * e).sum() / tot, y.sum() / (B * Tm1), target.sum() / (B * Tm1), tot])
    gy = np.zeros((B, Tm1 if gy_cols is None else gy_cols))
    gy[:, :Tm1] = 2.0 * m * (y - target) / tot
    return stats, gy


def clip_adam_model(param, grad, m, v, step, lr, b1, b2, eps, max_norm):
    """step: the counter BEFORE the advance.  -> param, clipped grad, m, v, step + 1, the pre-clip norm."""
    p, g0, m, v = (np.asarray(a, f32).astype(f64) for a in (param, grad, m, v))
    lr, b1, b2, eps, max_norm = _w(lr), _w(b1), _w(b2), _w(eps), _w(max_norm)
    norm = float(np.sqrt((g0 * g0).sum()))
    coef = min(1.0, max_norm / (norm + float(CLIP_EPS)))
    g = coef * g0
    t = float(step) + 1.0
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return p, g, m, v, t, norm


def ln_param_model(W, G, gb):
    """W, G [C, K], gb [C] -> dgamma [K] = sum_c W[c, k] G[c, k], dbeta [K] = sum_c gb[c] W[c, k]."""
    W, G, gb = np.asarray(W, f32).astype(f64), np.asarray(G, f32).astype(f64), np.asarray(gb, f32).astype(f64)
    return (W * G).sum(axis=0), gb @ W


# ------------------------------------------------------------------------------------------------ float32 restatement
def lane_sum_f32(terms, lanes, fused_square=False):
    """Sum of a float32 vector: element i goes to lane i % lanes (added in index order), the lanes through a halving tree.
    ``fused_square``: the terms are squared inside the addition (one rounding, as fmaf does)."""
    t = np.asarray(terms, f32).reshape(-1)
    rows = -(-t.size // lanes)
    t = np.concatenate([t, np.zeros(rows * lanes - t.size, f32)]).reshape(rows, lanes)
    s = np.zeros(lanes, f32)
    for r in range(rows):
        s = (t[r].astype(f64) ** 2 + s.astype(f64)).astype(f32) if fused_square else (s + t[r]).astype(f32)
    while s.size > 1:
        s = (s[:s.size // 2] + s[s.size // 2:]).astype(f32)
    return f32(s[0])


def blocks_of(n):
    return min(-(-n // 256), ADAM_BLOCKS)


def sq_partials_f32(grad, skip=()):
    """One partial per workgroup: workgroup b of ``blocks_of(n)`` takes the elements b 256 + t + j 256 blocks; the ranges
    ``skip`` ((offset, length), ..) count zero."""
    g = np.asarray(grad, f32).copy()
    for off, k in skip:
        g[off:off + k] = 0
    nb = blocks_of(g.size)
    rows = -(-g.size // (256 * nb))
    g = np.concatenate([g, np.zeros(rows * 256 * nb - g.size, f32)]).reshape(rows, nb, 256)
    return np.array([lane_sum_f32(g[:, b, :].reshape(-1), 256, fused_square=True) for b in range(nb)], f32)


def ln_param_f32(W, G, gb):
    W, G, gb = np.asarray(W, f32), np.asarray(G, f32), np.asarray(gb, f32)
    K = W.shape[1]
    dg = np.array([lane_sum_f32((W[:, k] * G[:, k]).astype(f32), 256) for k in range(K)], f32)
    db = np.array([lane_sum_f32((W[:, k] * gb).astype(f32), 256) for k in range(K)], f32)
    return dg, db


def clip_adam_f32(param, grad, m, v, step, lr, b1, b2, eps, max_norm, norm):
    """The header's formula block in float32 from a given float32 norm on."""
    p, g0, m, v = (np.asarray(a, f32) for a in (param, grad, m, v))
    lr, b1, b2, eps, max_norm, one = f32(lr), f32(b1), f32(b2), f32(eps), f32(max_norm), f32(1)
    norm = f32(norm)
    coef = min(one, max_norm / (norm + CLIP_EPS))
    g = g0 * coef
    t = f32(f32(step) + one)
    m = m + (one - b1) * (g - m)
    v = v * b2 + (one - b2) * g * g
    bc1, bc2 = one - np.power(b1, t), one - np.power(b2, t)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    assert all(a.dtype == f32 for a in (p, g, m, v))
    return p, g, m, v, t, norm


def td_loss_f32(y, tq, reward, terminated, filled, gamma_, gy_cols=None):
    y, tq, r = (np.asarray(a, f32) for a in (y, tq, reward))
    term, m = (np.asarray(terminated) != 0).astype(f32), (np.asarray(filled) != 0).astype(f32)
    B, Tm1 = y.shape
    target = r + f32(gamma_) * (f32(1) - term) * tq
    e = (y - target) * m
    tot = lane_sum_f32(m, 1024)
    stats = np.array([lane_sum_f32(e * e, 1024) / tot, lane_sum_f32(y, 1024) / f32(B * Tm1),
                      lane_sum_f32(target, 1024) / f32(B * Tm1), tot], f32)
    gy = np.zeros((B, Tm1 if gy_cols is None else gy_cols), f32)
    gy[:, :Tm1] = (f32(2) / tot) * m * (y - target)
    return stats, gy


# ------------------------------------------------------------------------------------------------ bounds
def td_bounds(y, tq, reward, terminated, filled, gamma_):
    """-> (E_stats [4], E_gy [B, Tm1]) of the module docstring (stats[3], a sum of 0 / 1 below 2^24, is exact)."""
    y, tq, r = (np.asarray(a, f32).astype(f64) for a in (y, tq, reward))
    term, m = (np.asarray(terminated) != 0).astype(f64), (np.asarray(filled) != 0).astype(f64)
    M = y.size
    chain = gamma(-(-M // 1024) + 6 + 4)
    gtq = _w(gamma_) * (1.0 - term) * tq
    target = r + gtq
    a_t = np.abs(r) + np.abs(gtq)
    a_e = np.abs(y) + a_t
    e = (y - target) * m
    tot = m.sum()
    e_e = 3 * U * a_e * m
    sum_e2 = chain * (e * e).sum() + (2 * np.abs(e) * e_e + U * e * e).sum()
    loss = (e * e).sum() / tot
    e_stats = np.array([sum_e2 / tot + U * loss,
                        chain * np.abs(y).sum() / M + U * abs(y.sum() / M),
                        (chain * np.abs(target).sum() + (2 * U * a_t).sum()) / M + U * abs(target.sum() / M),
                        0.0])
    gy = 2.0 * m * (y - target) / tot
    return e_stats, (2.0 / tot) * 3 * U * a_e * m + 2 * U * np.abs(gy)


def norm_rel_bound(sq_sum, chain, term_err=0.0):
    """Relative bound of sqrt(sum) for a sum of non-negative terms over ``chain`` additions whose terms carry the absolute
    error ``term_err`` in total (0 for a zero sum: every order gives exactly 0)."""
    if sq_sum == 0.0:
        return 0.0
    x = gamma(chain) + term_err / sq_sum
    return x / (1.0 + np.sqrt(1.0 - x)) + 2 * U


def sqnorm_chain(n, n_partials, reduced=False, per_partial=None):
    """Chain of the squared norm: the partials' own chain (``per_partial``; default: a workgroup of the squared-norm
    launch) plus that of the launch that sums them."""
    if per_partial is None:
        per_partial = -(-n // (256 * blocks_of(n))) + 6 + 2
    return per_partial + ((-(-n_partials // 256) + 6 + 2) if reduced else (-(-n_partials // 64) + 6))


def ln_bounds(W, G, gb):
    """-> (E_dgamma [K], E_dbeta [K])."""
    W, G, gb = np.abs(np.asarray(W, f64)), np.abs(np.asarray(G, f64)), np.abs(np.asarray(gb, f64))
    c = gamma(-(-W.shape[0] // 256) + 6 + 2)
    return c * (W * G).sum(axis=0), c * (gb @ W)


def adam_bounds(grad, m, v, b1, b2, max_norm, norm_rel):
    """-> dict(grad, m, v) of elementwise bounds around clip_adam_model's outputs, ``norm_rel`` = the norm's bound."""
    g0, m, v = (np.asarray(a, f32).astype(f64) for a in (grad, m, v))
    b1, b2 = _w(b1), _w(b2)
    norm = float(np.sqrt((g0 * g0).sum()))
    coef = min(1.0, _w(max_norm) / (norm + float(CLIP_EPS)))
    rho = norm_rel + 2 * U
    rho_c = rho / (1.0 - rho)
    g = np.abs(coef * g0)
    e_g = g * (rho_c + U + rho_c * U)
    gm = g + e_g
    # m' = m + (1 - b1) (g - m)
    d = np.abs(coef * g0 - m)
    e_d = e_g + U * (d + e_g)
    e_p = (1 - b1) * e_d + U * (1 - b1) * (d + e_d)
    e_m = e_p + U * (np.abs(m) + (1 - b1) * d + e_p)
    # v' = v b2 + ((1 - b2) g) g
    e_a = U * v * b2
    q = (1 - b2) * g
    e_q = (1 - b2) * e_g + U * (1 - b2) * gm
    e_r = e_q * gm + q * e_g + U * (q + e_q) * gm
    e_v = e_a + e_r + U * (v * b2 + q * g + e_a + e_r)
    return {"grad": e_g, "m": e_m, "v": e_v}


def param_ceiling(param, m_new, v_new, e_m, e_v, step, lr, b1, b2, eps):
    """Worst-case ceiling of the parameter update around clip_adam_model's value (module docstring)."""
    p, m_new, v_new = np.asarray(param, f32).astype(f64), np.asarray(m_new, f64), np.asarray(v_new, f64)
    lr, b1, b2, eps = _w(lr), _w(b1), _w(b2), _w(eps)
    t = float(step) + 1.0
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    rel_ss = POW_ULPS * U * b1 ** t / bc1 + 2 * U
    rel_bs = (POW_ULPS * U * b2 ** t / bc2 + U) / 2 + U
    sv = np.sqrt(v_new)
    e_sv = np.divide(e_v, 2 * sv, out=np.zeros_like(sv), where=sv > 0) + U * sv
    tt = sv / np.sqrt(bc2)
    e_t = e_sv / np.sqrt(bc2) + tt * (rel_bs + U)
    den = tt + eps
    e_den = e_t + U * den
    r = np.abs(m_new) / den
    e_r = e_m / den + r * (e_den / den + U)
    ss = lr / bc1
    upd = ss * r
    e_upd = upd * (rel_ss + U) + ss * e_r
    return CEIL_SLACK * (e_upd + U * (np.abs(p) + upd + e_upd))


def param_tolerance(ceiling, restated, model):
    """min(ceiling, FACTOR x Y) per element, Y = max |float32 restatement - model|, at least one float32 ulp of the value."""
    y = float(np.abs(np.asarray(restated, f64) - model).max())
    return np.maximum(np.minimum(ceiling, FACTOR * y), np.spacing(np.abs(model).astype(f32)).astype(f64))


# ------------------------------------------------------------------------------------------------ cases
HYPER = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8)     # the learner's Adam (reference core/qmix.py)
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537]     # + the learner's own flat length
STEPS = [0, 1, 9, 999, 99999]
AdamState = namedtuple("AdamState", "name step moments grad clip")
# grad: "normal" N(0,1) with the largest magnitudes at 0, n - 1 (and 65536); "zero"; "eps" |g| ~ 1e-8; "tiny" |g| ~ 1e-5 (the
# 1e-6 of the clip coefficient is then a percent of the norm); "ints" small integers over 8 (every sum exact in float32).
# clip: "off" max_norm = 1e9; "on" a quarter of the norm; "edge" max_norm = the float32 norm itself (grad "ints" only).
STATES = [
    AdamState("s0-zero-moments-off", 0, False, "normal", "off"),
    AdamState("s0-moments-on", 0, True, "normal", "on"),
    AdamState("s1-moments-on", 1, True, "normal", "on"),
    AdamState("s9-moments-off", 9, True, "normal", "off"),
    AdamState("s999-zero-moments-on", 999, False, "normal", "on"),
    AdamState("s99999-moments-off", 99999, True, "normal", "off"),
    AdamState("zero-grad", 9, True, "zero", "on"),
    AdamState("grad-of-eps", 0, False, "eps", "off"),
    AdamState("tiny-grad-clipped", 1, True, "tiny", "on"),
    AdamState("edge-exact-norm", 9, True, "ints", "edge"),
]


def _rng(*key):
    return np.random.default_rng([ord(k) if isinstance(k, str) else int(k) for k in key])


def flat_length(numels):
    """Length of the learner's flat vector: every parameter starts at a multiple of 4 elements (core/qmix.py)."""
    return sum((int(k) + 3) // 4 * 4 for k in numels)


def big_indices(n):
    return sorted({0, n - 1} | ({65536} if n > 65536 else set()))


@functools.lru_cache(maxsize=None)
def adam_inputs(n, state, salt=0):
    """dict(param, grad, m, v float32 [n]; step; max_norm float32; lr, b1, b2, eps).  The parameters span four decades so
    that an error of the update is not hidden behind the rounding of large values."""
    rng = _rng(701, n, STATES.index(state), salt)
    param = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n)).astype(f32)
    if state.grad == "ints":
        grad = (rng.integers(-2, 3, n) / 8.0).astype(f32)
        grad[big_indices(n)] = 0.375
    elif state.grad == "zero":
        grad = np.zeros(n, f32)
    else:
        scale = {"normal": 1.0, "eps": 1e-8, "tiny": 1e-5}[state.grad]
        grad = rng.standard_normal(n)
        grad[big_indices(n)] = rng.choice([-1.0, 1.0], len(big_indices(n))) * max(1.0, np.sqrt(n))
        grad = (scale * grad).astype(f32)
    if state.moments:
        m = (0.3 * rng.standard_normal(n)).astype(f32)
        v = (rng.random(n) * 0.2).astype(f32)
    else:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    sq = float((grad.astype(f64) ** 2).sum())
    if state.clip == "edge":
        assert sq * 64 == int(sq * 64) < 2 ** 24 and sq > 0
    max_norm = {"off": f32(1e9), "on": f32(0.25 * np.sqrt(sq)) if sq > 0 else f32(1.0), "edge": f32(np.sqrt(sq))}[state.clip]
    return dict(param=param, grad=grad, m=m, v=v, step=state.step, max_norm=max_norm, **HYPER)


def chunk_partials(grad, chunk=64):
    """What a launch ahead of macjd_clip_adam_step_reduced leaves: one float32 square sum per ``chunk`` elements (each the
    float64 sum rounded once)."""
    g = np.asarray(grad, f32).astype(f64)
    k = -(-g.size // chunk)
    g = np.concatenate([g, np.zeros(k * chunk - g.size)]).reshape(k, chunk)
    return (g * g).sum(axis=1).astype(f32)


def adam_expectation(d, norm_rel, restated_norm):
    """Model outputs, bounds and the parameter tolerance of one optimiser case: dict name -> (value, tolerance), + norm."""
    args = (d["param"], d["grad"], d["m"], d["v"], d["step"], d["lr"], d["b1"], d["b2"], d["eps"], d["max_norm"])
    p, g, m, v, t, norm = clip_adam_model(*args)
    b = adam_bounds(d["grad"], d["m"], d["v"], d["b1"], d["b2"], d["max_norm"], norm_rel)
    ceil_p = param_ceiling(d["param"], m, v, b["m"], b["v"], d["step"], d["lr"], d["b1"], d["b2"], d["eps"])
    p32 = clip_adam_f32(*args, restated_norm)[0]
    return {"param": (p, param_tolerance(ceil_p, p32, p)), "grad": (g, b["grad"]), "m": (m, b["m"]), "v": (v, b["v"]),
            "norm": (norm, norm * norm_rel), "step": t, "ceiling": ceil_p}


def plain_expectation(d):
    """macjd_clip_adam_step / _sample: blocks_of(n) partials of the squared-norm launch, one wave over them."""
    n = d["param"].size
    rel = norm_rel_bound(float((d["grad"].astype(f64) ** 2).sum()), sqnorm_chain(n, blocks_of(n)))
    return adam_expectation(d, rel, restated_norm(d["grad"]))


def reduced_norm_f32(parts):
    """float32 norm as macjd_clip_adam_step_reduced forms it from the partials it is given: 256 lanes, a tree, sqrt."""
    return f32(np.sqrt(lane_sum_f32(parts, 256)))


def reduced_expectation(d, parts):
    """macjd_clip_adam_step_reduced fed ``chunk_partials`` (one float32 partial per 64 elements, each rounded once: chain 1)."""
    n = d["param"].size
    rel = norm_rel_bound(float((d["grad"].astype(f64) ** 2).sum()), sqnorm_chain(n, parts.size, reduced=True, per_partial=1))
    return adam_expectation(d, rel, reduced_norm_f32(parts))


def restated_norm(grad, skip=(), extra=()):
    """float32 norm as the two-launch step forms it: workgroup partials (+ ``extra`` ones), one wave over them, sqrt."""
    parts = np.concatenate([sq_partials_f32(grad, skip), np.asarray(extra, f32)])
    return f32(np.sqrt(lane_sum_f32(parts, 64)))


# --- the LayerNorm-fused step
LnCase = namedtuple("LnCase", "name n K C w_pad g_pad gamma_off beta_off")
LN_CASES = [
    LnCase("k1-c1-ends", 300, 1, 1, 0, 0, 0, 299),
    LnCase("k46-c255-front-back", 1000, 46, 255, 3, 0, 0, 1000 - 46),
    LnCase("k46-c256-straddle-256", 1000, 46, 256, 0, 2, 256 - 20, 600),
    LnCase("k46-c257-adjacent", 1000, 46, 257, 1, 1, 300, 346),
    LnCase("k46-c257-adjacent-swapped", 1000, 46, 257, 0, 0, 346, 300),
    LnCase("k46-c255-second-pass", 65536 + 300, 46, 255, 3, 2, 65536 - 20, 65536 + 200),
    LnCase("k1024-c1-limit", 4000, 1024, 1, 0, 5, 0, 4000 - 1024),
    LnCase("k1024-c257-limit-adjacent", 2048 + 7, 1024, 257, 2, 0, 3, 1027),
]


def ln_case_at_length(n):
    """The LayerNorm-fused step at one of LENGTHS (n >= 4: two disjoint ranges beside elements 0 and n - 1)."""
    K = 1 if n < 128 else 46
    return LnCase(f"length-{n}", n, K, 70, 1, 0, 1, n - 1 - K)


@functools.lru_cache(maxsize=None)
def ln_inputs(case, clip):
    """The optimiser inputs of an LnCase (grad NaN on the two ranges) + W, G [C, K], gb [C], scaled so that the LayerNorm
    gradients carry at least a quarter of the squared norm (about half: the other elements share as much again, half of
    that in the large elements)."""
    rng = _rng(801, case.n, case.K, case.C, case.gamma_off, case.beta_off, clip)
    n, K, C = case.n, case.K, case.C
    W, G, gb = (rng.standard_normal(s).astype(f32) for s in ((C, K), (C, K), (C,)))
    dg, db = ln_param_model(W, G, gb)
    rest = n - 2 * K
    ln_sq = float((dg ** 2).sum() + (db ** 2).sum())
    grad = rng.standard_normal(n) * np.sqrt(ln_sq / (2 * max(rest, 1)))
    # as in adam_inputs: single large elements at 0, n - 1 (and 65536) where no range covers them, a sixth of the
    # LayerNorm share each, so that an element dropped at the ends of a pass moves the norm by percents
    in_range = lambda i: case.gamma_off <= i < case.gamma_off + K or case.beta_off <= i < case.beta_off + K
    for i in big_indices(n):
        if not in_range(i):
            grad[i] = rng.choice([-1.0, 1.0]) * np.sqrt(ln_sq / 6)
    grad = grad.astype(f32)
    grad[case.gamma_off:case.gamma_off + K] = np.nan
    grad[case.beta_off:case.beta_off + K] = np.nan
    full = grad.astype(f64)
    full[case.gamma_off:case.gamma_off + K], full[case.beta_off:case.beta_off + K] = dg, db
    sq = float((full ** 2).sum())
    assert (dg ** 2).sum() + (db ** 2).sum() >= 0.25 * sq
    d = dict(param=(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n)).astype(f32), grad=grad,
             m=(0.3 * rng.standard_normal(n)).astype(f32), v=(rng.random(n) * 0.2).astype(f32), step=1 if clip else 9,
             max_norm=f32(0.25 * np.sqrt(sq)) if clip else f32(1e9), W=W, G=G, gb=gb, **HYPER)
    return d


def ln_expectation(case, d):
    """The model of macjd_clip_adam_step_ln: LayerNorm gradients placed into the vector, then the step.  The gradient the
    device clips in the two ranges is the one it STORED (bound E_d), so those elements' bounds are widened by E_d, first
    order: E_g += coef E_d, and through g into m and v."""
    K = case.K
    dg, db = ln_param_model(d["W"], d["G"], d["gb"])
    e_dg, e_db = ln_bounds(d["W"], d["G"], d["gb"])
    full = d["grad"].astype(f64)
    sl_g, sl_b = slice(case.gamma_off, case.gamma_off + K), slice(case.beta_off, case.beta_off + K)
    full[sl_g], full[sl_b] = dg, db
    # the device squares float32 values: the vector the model steps on is the float32 rounding of the LayerNorm gradients
    # (one more u on those elements, counted into E_d)
    g32 = full.astype(f32)
    e_d = np.zeros(case.n)
    e_d[sl_g], e_d[sl_b] = e_dg + U * np.abs(dg), e_db + U * np.abs(db)
    sq = float((g32.astype(f64) ** 2).sum())
    term_err = float((2 * np.abs(g32.astype(f64)) * e_d + e_d ** 2).sum()) + 2 * U * float((dg ** 2 + db ** 2).sum())
    nb = blocks_of(case.n)
    chain = sqnorm_chain(case.n, nb + K)
    rel = norm_rel_bound(sq, chain, term_err)
    dg32, db32 = ln_param_f32(d["W"], d["G"], d["gb"])
    r_norm = restated_norm(np.nan_to_num(d["grad"]), extra=(dg32.astype(f64) ** 2 + db32.astype(f64) ** 2).astype(f32))
    dd = dict(d, grad=g32)
    exp = adam_expectation(dd, rel, r_norm)
    coef = min(1.0, _w(d["max_norm"]) / (exp["norm"][0] + float(CLIP_EPS)))
    b1, b2 = _w(d["b1"]), _w(d["b2"])
    add_g = coef * e_d * (1 + 4 * U + rel)
    g_abs = np.abs(exp["grad"][0])
    extra = {"grad": add_g, "m": (1 - b1) * add_g * (1 + 4 * U), "v": (1 - b2) * (2 * g_abs + add_g) * add_g * (1 + 4 * U)}
    out = dict(exp)
    for k in ("grad", "m", "v"):
        out[k] = (exp[k][0], exp[k][1] + extra[k])
    e_m, e_v = out["m"][1], out["v"][1]
    ceil_p = param_ceiling(d["param"], exp["m"][0], exp["v"][0], e_m, e_v, d["step"], d["lr"], d["b1"], d["b2"], d["eps"])
    p32 = clip_adam_f32(d["param"], g32, d["m"], d["v"], d["step"], d["lr"], d["b1"], d["b2"], d["eps"], d["max_norm"], r_norm)[0]
    out["param"] = (exp["param"][0], param_tolerance(ceil_p, p32, exp["param"][0]))
    out["ceiling"] = ceil_p
    out["dgamma"], out["dbeta"] = (dg, e_dg), (db, e_db)
    return out


# --- the TD loss
TD_SHAPES = [(1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 2), (7, 341), (32, 99)]
TD_MASKS = ["all", "ragged", "one"]
GY_EXTRA = [0, 1, 5]
TD_GAMMA = 0.99


@functools.lru_cache(maxsize=None)
def td_inputs(B, Tm1, mask):
    """dict(y, tq, reward float32 [B, Tm1]; terminated, filled uint8 [B, Tm1]).  ragged: every episode filled up to its own
    length (>= 1 pair over the batch) and terminated on its last filled step; one: a single filled pair."""
    rng = _rng(901, B, Tm1, TD_MASKS.index(mask))
    y, tq, reward = ((s * rng.standard_normal((B, Tm1))).astype(f32) for s in (3.0, 3.0, 1.0))
    t = np.arange(Tm1)[None, :]
    if mask == "all":
        length = np.full((B, 1), Tm1)
    elif mask == "ragged":
        length = rng.integers(0 if B > 1 else 1, Tm1 + 1, (B, 1))
        length[0, 0] = max(1, Tm1 // 2)
    else:
        length = np.zeros((B, 1), np.int64)
    filled = (t < length).astype(np.uint8)
    terminated = (t == length - 1).astype(np.uint8) | (rng.random((B, Tm1)) < 0.1).astype(np.uint8)
    if mask == "one":
        filled[B // 2, Tm1 // 3] = 1
        terminated[B // 2, Tm1 // 3] = B * Tm1 > 1
    assert filled.sum() >= 1 and (mask != "one" or filled.sum() == 1)
    return dict(y=y, tq=tq, reward=reward, terminated=terminated, filled=filled)
