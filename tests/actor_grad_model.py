"""Float64 model of the actor-gradient contract (include/macjd_nets.h, macjd_actor_grad_io) and the shared case table
(test infrastructure; NumPy only, shares no code with macjd_amd.ops).

ReLU ties.  The outputs g1 / g2 / g3 are discontinuous where a ReLU pre-activation (p1 = W1a x + b1a, p2 = W2a a1 + b2a,
z_a = base + W1q[:, H+a] + W1q[:, H+A] P_a) crosses zero, and a float32 evaluation under another summation order may
legitimately sit on the other side of a pre-activation that is tiny against the terms it was summed from.  The model
therefore computes for every pre-activation the sum of the absolute values of its terms (|W1a||x| + |b1a|, ...,
|base| + |col| + |wp P|) and calls an element NEAR when |pre| < 64 * 2^-24 * abs_sum.  A ROW with any near element is
excluded from the comparison of g1 / g2 / g3 (rows are independent); a1, a2 and qsum are continuous and compared on all
rows.  The cap on excluded rows is a condition on the cases, checked in tests/test_actor_grad_cpu.py on the model alone:
at most 2 % of a case's rows, and none in a case with fewer than 100 rows (those seeds were chosen so).
"""
import numpy as np

NEAR = 64.0 * 2.0 ** -24
GEOMETRIES = [(24, 128, 128, 5), (46, 128, 64, 9), (92, 128, 64, 17), (184, 128, 64, 33)]   # (S, Ha, H, A): the fixtures'


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def actor_grad_model(x, base, m, actor, W1q, w2q, b2q=None):
    """All outputs of the contract in float64, the six weight gradients, and the per-row exclusion mask.
    x [N,S], base [N,H], m [N], actor = [(W1a, b1a), (W2a, b2a), (W3a, b3a)], W1q [H, H+A+1], w2q [H], b2q scalar."""
    f = lambda a: np.asarray(a, np.float64)
    x, base, m, W1q, w2q = f(x), f(base), f(m).reshape(-1), f(W1q), f(w2q).reshape(-1)
    (W1a, b1a), (W2a, b2a), (W3a, b3a) = [(f(w), f(b)) for w, b in actor]
    H, A = base.shape[1], W3a.shape[0]
    b2 = 0.0 if b2q is None else float(np.asarray(b2q).reshape(-1)[0])
    p1 = x @ W1a.T + b1a
    a1 = np.maximum(p1, 0.0)
    p2 = a1 @ W2a.T + b2a
    a2 = np.maximum(p2, 0.0)
    u = a2 @ W3a.T + b3a
    P = _sig(u)
    col, wp = W1q[:, H:H + A].T, W1q[:, H + A]                       # [A,H], [H]
    z = base[:, None, :] + col[None] + P[:, :, None] * wp[None, None]          # [N,A,H]
    pos = z > 0.0
    Q = (np.where(pos, z, 0.0) * w2q).sum(2) + b2                    # [N,A]
    s = (pos * (w2q * wp)).sum(2)                                    # [N,A]
    g3 = -m[:, None] * s * P * (1.0 - P)
    g2 = (g3 @ W3a) * (a2 > 0.0)
    g1 = (g2 @ W2a) * (a1 > 0.0)
    near1 = np.abs(p1) < NEAR * (np.abs(x) @ np.abs(W1a).T + np.abs(b1a))
    near2 = np.abs(p2) < NEAR * (np.abs(a1) @ np.abs(W2a).T + np.abs(b2a))
    nearz = np.abs(z) < NEAR * (np.abs(base)[:, None, :] + np.abs(col)[None] + np.abs(P[:, :, None] * wp[None, None]))
    excluded = near1.any(1) | near2.any(1) | nearz.any(axis=(1, 2))
    return dict(a1=a1, a2=a2, P=P, g3=g3, g2=g2, g1=g1, qsum=Q.sum(1), Q=Q, excluded=excluded,
                dW1a=g1.T @ x, db1a=g1.sum(0), dW2a=g2.T @ a1, db2a=g2.sum(0), dW3a=g3.T @ a2, db3a=g3.sum(0))


def rel_err(got, ref):
    """max|got - ref| / max|ref| (0 / 0 counts as 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    diff = float(np.abs(got - ref).max()) if ref.size else 0.0
    return diff / scale if scale > 0 else diff


# --------------------------------------------------------------------------------------------- cases
def _linear(rng, n_out, n_in, scale):
    """nn.Linear-style uniform initialisation times ``scale``, float32."""
    k = scale / np.sqrt(n_in)
    return (rng.uniform(-k, k, (n_out, n_in)).astype(np.float32), rng.uniform(-k, k, n_out).astype(np.float32))


def make_case(case):
    """Inputs of one table entry, float32 (the model reads the same float32 numbers, widened).  x / base are views with
    the case's row strides (x_pad / base_pad extra columns); m has zeros in rows [zero_lo, zero_hi)."""
    S, Ha, H, A = case["geom"]
    N, scale = case["N"], case["scale"]
    rng = np.random.default_rng(case["seed"])
    actor = [_linear(rng, Ha, S, scale), _linear(rng, Ha, Ha, scale), _linear(rng, A, Ha, scale)]
    W1q, b1q = _linear(rng, H, H + A + 1, scale)
    w2q, b2q = _linear(rng, 1, H, scale)
    x_full = rng.standard_normal((N, S + case.get("x_pad", 0))).astype(np.float32)
    h = np.tanh(rng.standard_normal((N, H)))
    base_full = np.full((N, H + case.get("base_pad", 0)), 7.0, dtype=np.float32)
    base_full[:, :H] = (h @ W1q[:, :H].astype(np.float64).T + b1q).astype(np.float32)
    m = (rng.random(N) / N).astype(np.float32)
    lo, hi = case.get("zero", (0, 0))
    m[lo:hi] = 0.0
    return dict(x=x_full[:, :S], base=base_full[:, :H], m=m, actor=actor, W1q=W1q, w2q=w2q.reshape(-1), b2q=b2q,
                geom=case["geom"], zero=(lo, hi))


def run_model(case):
    c = make_case(case)
    return c, actor_grad_model(c["x"], c["base"], c["m"], c["actor"], c["W1q"], c["w2q"], c["b2q"])


def case_id(case):
    S, Ha, H, A = case["geom"]
    extra = "".join(f"-{k}" for k in ("x_pad", "zero") if k in case)
    return f"S{S}H{H}A{A}-N{case['N']}-x{case['scale']}{extra}"


# Seeds of the cases with fewer than 100 rows: the first seed >= 1 at which the MODEL excludes no row (seed 1 unless
# listed here; found by trying 1, 2, ... on the model alone, before any kernel ran).
SMALL_SEEDS = {((46, 128, 64, 9), 65, 3): 2, ((92, 128, 64, 17), 65, 1): 3, ((184, 128, 64, 33), 65, 3): 3}


def _small_seed(geom, N, scale):
    return SMALL_SEEDS.get((geom, N, scale), 1)


def case_table():
    cases = []
    for geom in GEOMETRIES:
        for N in (1, 15, 16, 17, 65, 257):
            for scale in (1, 3):
                cases.append(dict(geom=geom, N=N, scale=scale, seed=_small_seed(geom, N, scale)))
    for geom, scale in zip(GEOMETRIES, (1, 3, 1, 3)):
        cases.append(dict(geom=geom, N=4096, scale=scale, seed=4096 + geom[0]))
    cases.append(dict(geom=GEOMETRIES[1], N=257, scale=1, seed=7, x_pad=3, base_pad=5))      # x_ld > S, base_ld > H
    cases.append(dict(geom=GEOMETRIES[2], N=257, scale=1, seed=8, zero=(100, 180)))          # a block of m = 0 rows
    return cases
