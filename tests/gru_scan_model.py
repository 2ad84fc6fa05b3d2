"""Float64 model of what feeds the update chain: the learner's GRU scan (``macjd_gru_sequence``: the recurrence, the
in-kernel input transform and the in-kernel actor chain), the rollout's cell (``macjd_gru_gates``) and the one-launch
prefetch (``macjd_prefetch_batch`` / ``macjd_prefetch_batches``) — include/macjd_nets.h.  Plain NumPy in plain order; the
sigmoid and tanh are written so that no intermediate overflows.  Proved against float64 torch in
tests/test_gru_scan_cpu.py; the GPU tests (tests/test_gru_scan_gpu.py, tests/test_prefetch_model_gpu.py) hold the launches
to it.

Every function takes ``dt``: float64 is the model, float32 the RESTATEMENT — the same expressions, rounded to float32
after every operation, with exact (libm) exp.  The restatement is what an ideal float32 kernel would compute up to
summation order; its distance to the model measures how much float32 a case amplifies.

Tolerance rule (per case and per output, never fixed in advance):

    tol = min(cap, max(floor, 8 * max|restatement - model|))

* cap: the project's existing bar — for hidden states TOL = 1e-5 absolute (tests/test_nets_gpu.py), for the actor rows
  1e-6 + 1e-5 |value| (test_gru_scan_with_in_kernel_input_transform_and_actor).
* 8: the factor of the Q-head pin (tests/qhead_f64_model.py).
* floor: the absolute error of ONE step's expression when the inputs of the step are exact and the hardware exp2 and
  rcp are each good to one ulp, u = 2^-23 (the accuracy that AMD's CDNA instruction-set reference gives for v_exp_f32 and
  v_rcp_f32, and that csrc/macjd_gru_math.h relies on).  With s = rcp(1 + exp2(-x log2 e)):
      - the two roundings of the exponent's argument (x log2 e, and log2 e itself) move exp2 by |x| u relative, i.e. s by
        |x| s (1 - s) u <= 0.224 u (the maximum of x s (1 - s) is 0.2239 at x = 1.54);
      - exp2 to one ulp moves s by s (1 - s) u <= 0.25 u; the rounding of 1 + e by s u / 2 <= 0.5 u; rcp to one ulp by
        s u <= u: a sigmoid is good to 1.97 u, say 2 u.
      - tanh(x) = 1 - 2 q, q = rcp(exp2(2 x log2 e) + 1), carries the same four terms twice (3.95 u) and the rounding
        of the final subtraction (<= 0.5 u): 4.5 u.
      - n's argument gi_n + r gh_n inherits 2 u |gh_n| from r and two roundings (u |arg| / 2 each, damped by
        tanh' <= 1 and |x| tanh'(x) <= 0.45): with |gh_n| <= 1 (weights at torch's default scale and |h| <= 1) another
        2 u + 0.5 u.
      - h' = (h - n) z + n with |h|, |n| <= 1: |h - n| dz <= 2 * 2 u, (1 - z) dn <= 4.5 u + 2.5 u, three roundings of values
        below 2: <= 1.5 u.
  Sum: 4 + 7 + 1.5 = 12.5 u -> FLOOR_H = 12.5 * 2^-23 = 1.49e-6.  The same figure serves macjd_gru_gates (libm expf and
  IEEE division are no worse than one ulp each).  The actor's last step is one sigmoid behind a mat-vec: FLOOR_P = 2 u.
* fairness, asserted on the CPU for every case: the restatement's own deviation is at most cap / 8, so that the factor 8
  never reaches the cap for a reason that lies in the inputs (recurrent weights are drawn at torch's default scale,
  uniform +-1/sqrt(H): the scan is then contractive; at three times that scale it is not).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
from tests_golden_helpers import sample_episodes_mirror  # noqa: E402

f32, f64 = np.float32, np.float64
U = 2.0 ** -23
FLOOR_H = 12.5 * U
FLOOR_P = 2.0 * U
CAP_H = 1e-5
FACTOR = 8.0
SAT = (30.0, -30.0, 100.0, -100.0, 1e4, -1e4)   # gate inputs that overflow / underflow exp on either side


def cap_p(value):
    return 1e-6 + 1e-5 * np.abs(np.asarray(value, f64))


def _rng(*key):
    return np.random.default_rng([ord(c) for k in key for c in str(k)] or [0])


# ---------------------------------------------------------------------------------------------- the operations
def sigmoid(x):
    """1 / (1 + exp(-x)) without overflow: exp is only taken of -|x|."""
    x = np.asarray(x)
    one = x.dtype.type(1)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, one / (one + e), e / (one + e))


def tanh(x):
    """sign(x) (1 - e) / (1 + e), e = exp(-2 |x|) <= 1."""
    x = np.asarray(x)
    one, two = x.dtype.type(1), x.dtype.type(2)
    e = np.exp(-two * np.abs(x))
    return np.sign(x) * ((one - e) / (one + e))


def gru_step(gi, gh, h, dt=f64):
    """One cell step behind its two mat-vecs: gi, gh [..., 3H] (gate order r, z, n), h [..., H] -> h' [..., H]."""
    gi, gh, h = (np.asarray(a, dt) for a in (gi, gh, h))
    H = h.shape[-1]
    r = sigmoid(gi[..., :H] + gh[..., :H])
    z = sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return ((h - n) * z + n).astype(dt)


def linear(x, w, b, dt=f64):
    return (np.asarray(x, dt) @ np.asarray(w, dt).T + np.asarray(b, dt)).astype(dt)


def gru_scan(gi, w_hh, b_hh, h0, T, static=False, dt=f64):
    """gi [B, T, J, 3H] (static: [B, 1, J, 3H], the same row at every step), h0 [B, J, H] or None -> every h' [B, T, J, H]."""
    gi = np.asarray(gi, dt)
    B, _, J, H3 = gi.shape
    H = H3 // 3
    h = np.zeros((B, J, H), dt) if h0 is None else np.asarray(h0, dt).reshape(B, J, H)
    out = np.zeros((B, T, J, H), dt)
    for t in range(T):
        h = gru_step(gi[:, 0 if static else t], linear(h, w_hh, b_hh, dt), h, dt)
        out[:, t] = h
    return out


def input_transform(x, fc1_w, fc1_b, w_ih, b_ih, dt=f64):
    """gi = W_ih ReLU(fc1 x + b) + b_ih for rows x [..., S]."""
    return linear(np.maximum(linear(x, fc1_w, fc1_b, dt), dt(0)), w_ih, b_ih, dt)


def actor_rows(x, layers, dt=f64):
    """sigmoid(L3 ReLU(L2 ReLU(L1 x))); layers = [(w, b)] * 3."""
    v = np.maximum(linear(x, *layers[0], dt), dt(0))
    v = np.maximum(linear(v, *layers[1], dt), dt(0))
    return sigmoid(linear(v, *layers[2], dt)).astype(dt)


def gates(gi, gh, h, dt=f64):
    """macjd_gru_gates: gh [N, 3H], h [N, H]; gi [N, 3H], or ONE row ([3H] / [1, 3H]: gi_ld = 0) for all N."""
    gi = np.asarray(gi, dt)
    if gi.ndim == 1 or gi.shape[0] == 1:
        gi = np.broadcast_to(gi.reshape(1, -1), np.asarray(gh).shape)
    return gru_step(gi, gh, h, dt)


def draw_indices(n, N, counter, seed):
    """Element t of the draw of counter value ``counter``: the keyed permutation's first n images, or t mod N when N < n."""
    return [t % N for t in range(n)] if N < n else sample_episodes_mirror(n, N, counter, seed)


def scan_from_obs(obs, rows, w, T, with_actor=True, dt=f64):
    """The scan with the in-kernel input transform: obs [N, T+1, J, S] (only step 0 is read), rows = ring row of every
    batch entry, w = agent weights (``agent_weights``) -> (h [B, T, J, H], P [B, J, A] or None)."""
    x = np.asarray(obs, dt)[np.asarray(rows, np.int64), 0]                      # [B, J, S]
    gi = input_transform(x, w["fc1_w"], w["fc1_b"], w["w_ih"], w["b_ih"], dt)[:, None]
    h = gru_scan(gi, w["w_hh"], w["b_hh"], w.get("h0"), T, static=True, dt=dt)
    return h, (actor_rows(x, w["actor"], dt) if with_actor else None)


def prefetch_model(ring, idx, w, T, Tm1, dt=f64):
    """One batch of the prefetch launch.  ring: dict(obs [N, T+1, J, S], filled [N, Tf, 1] bool, srcs = [arrays whose
    first axis is the ring row]); idx: the ring row of every batch entry.  -> dict(h, P, rows = the gathered rows as raw
    bytes [B, row_bytes] per source, tot_m = the exact count of set mask entries in the first Tm1 steps)."""
    idx = np.asarray(idx, np.int64)
    h, P = scan_from_obs(ring["obs"], idx, w, T, True, dt)
    rows = [np.ascontiguousarray(s).reshape(s.shape[0], -1).view(np.uint8)[idx] for s in ring["srcs"]]
    tot = int(np.count_nonzero(np.asarray(ring["filled"])[idx, :Tm1]))
    return dict(h=h, P=P, rows=rows, tot_m=tot)


# ---------------------------------------------------------------------------------------------- tolerance rule
def tolerance(kind, model, restate):
    """-> (tol array broadcastable to model, the restatement's largest deviation as a share of the cap)."""
    model, restate = np.asarray(model, f64), np.asarray(restate, f64)
    dev = np.abs(restate - model)
    y = float(dev.max()) if dev.size else 0.0
    if kind == "h":
        cap, floor = np.full(model.shape, CAP_H), FLOOR_H
    else:
        cap, floor = cap_p(model), FLOOR_P
    tol = np.minimum(cap, max(floor, FACTOR * y))
    share = float((dev / cap).max()) if dev.size else 0.0
    return tol, share


def fair(share):
    return share <= 1.0 / FACTOR


# ---------------------------------------------------------------------------------------------- case builders
def default_uniform(rng, shape, fan_in):
    """torch's default initialisation of Linear / GRUCell: uniform +- 1 / sqrt(fan_in), as float32 values."""
    k = 1.0 / np.sqrt(fan_in)
    return rng.uniform(-k, k, size=shape).astype(f32)


def recurrent_weights(rng, H):
    return dict(w_hh=default_uniform(rng, (3 * H, H), H), b_hh=default_uniform(rng, (3 * H,), H))


def agent_weights(rng, S, H, Ah, A, dead=False):
    """fc1, the GRU cell and the actor at the default scale.  ``dead``: fc1's bias leaves every ReLU dead (gi = b_ih)."""
    w = recurrent_weights(rng, H)
    w.update(fc1_w=default_uniform(rng, (H, S), S), fc1_b=default_uniform(rng, (H,), S),
             w_ih=default_uniform(rng, (3 * H, H), H), b_ih=default_uniform(rng, (3 * H,), H))
    if dead:
        w["fc1_b"] = np.full((H,), -1e3, f32)
    w["actor"] = [(default_uniform(rng, (Ah, S), S), default_uniform(rng, (Ah,), S)),
                  (default_uniform(rng, (Ah, Ah), Ah), default_uniform(rng, (Ah,), Ah)),
                  (default_uniform(rng, (A, Ah), Ah), default_uniform(rng, (A,), Ah))]
    return w


def saturate(gi, H):
    """Columns 0 .. 5 of every gate of gi [..., 3H] <- +-30, +-100, +-1e4 (in place)."""
    for g in range(3):
        for c, v in enumerate(SAT):
            gi[..., g * H + c] = v
    return gi


def special_h0(h0):
    """Entries 6, 7, 8 of every row of h0 [..., H] <- exactly 0, 1, -1 (in place; beside the saturated gate columns too:
    entries 0, 1, 2)."""
    h0[..., 6], h0[..., 7], h0[..., 8] = 0.0, 1.0, -1.0
    h0[..., 0], h0[..., 1], h0[..., 2] = 0.0, 1.0, -1.0
    return h0


FORMS = [("units", 64), ("ksplit", 64), ("ksplit", 128)]   # MACJD_GRU_SCAN value, H: the four kernels behind the entry
BJS = [(1, 1), (3, 2), (2, 3)]
# h0 of a case, per net: None, or the batch stride handed to the kernel — "0" (h0_sb = 0: contiguous), "JH", "T1JH"
# (step 0 of a stored [B, T+1, J, H]) or "JH4" (J H + 4: a padded row)
_H0_ONE = ["0", "JH", "T1JH", "JH4", None, "T1JH"]
_H0_TWO = [(None, "JH4"), ("T1JH", None), ("0", "JH4")]


def scan_cases():
    """(form, H, B, J, T, static, h0 spec per net, saturated) of the recurrence itself (gi supplied).  T = 1 .. 7: both
    remainders of the unroll by three, the first two ring slots (T = 1: both read row 0), the t + 2 clamp at T - 1;
    T = 101: the learner's own, where the error growth shows."""
    cases = []
    for form, H in FORMS:
        for i, T in enumerate([1, 2, 3, 4, 5, 7]):
            B, J = BJS[i % 3]
            h0 = (_H0_ONE[i],) if i % 2 == 0 else _H0_TWO[i // 2]
            cases.append((form, H, B, J, T, False, h0, i % 2 == 1))
        cases.append((form, H, 2, 3, 3, False, ("JH4",), True))
        cases.append((form, H, 3, 2, 101, False, (None, "T1JH"), False))
        cases.append((form, H, 3, 2, 4, True, (None, "JH4"), True))
        cases.append((form, H, 2, 3, 5, True, ("JH",), False))
        cases.append((form, H, 1, 1, 1, True, (None,), True))
    return cases


def h0_stride(spec, T, J, H):
    return {"0": J * H, "JH": J * H, "T1JH": (T + 1) * J * H, "JH4": J * H + 4}[spec]


def scan_case_data(case):
    """-> list per net of dict(gi, w_hh, b_hh, h0 or None), float32 values; different data per sequence and step."""
    form, H, B, J, T, static, h0s, sat = case
    out = []
    for k, spec in enumerate(h0s):
        rng = _rng("scan", H, B, J, T, int(static), int(sat), k)   # (not keyed by the form: both H = 64 forms see one case)
        gi = rng.standard_normal((B, 1 if static else T, J, 3 * H)).astype(f32)
        if sat:
            saturate(gi, H)
        d = recurrent_weights(rng, H)
        d["gi"] = gi
        d["h0"] = None if spec is None else special_h0((0.5 * rng.standard_normal((B, J, H))).astype(f32))
        out.append(d)
    return out


def scan_case_expect(case):
    """-> per net (model h, restatement h)."""
    _, H, B, J, T, static, _, _ = case
    return [(gru_scan(d["gi"], d["w_hh"], d["b_hh"], d["h0"], T, static, f64),
             gru_scan(d["gi"], d["w_hh"], d["b_hh"], d["h0"], T, static, f32)) for d in scan_case_data(case)]


# the in-kernel transform and actor: (S, Ah, A) chosen so that each of the prologue's UN = 16, 8, 4 outputs per pass
# (K <= 64, <= 128, <= 256 columns) meets an output count that is no multiple of it, and K = 1, 64, 65, 129, 256
OBS_SHAPES = [(1, 63, 5), (64, 1, 1), (65, 65, 9), (129, 129, 17), (256, 256, 64)]
# p_out per net: which nets carry the actor rows
_P_SPECS = [(True,), (True, False), (False, True), (True, True), (False,)]
_INDEX = ["none", "dup", "ends", "dup", "ends"]
NRING = 5


def obs_cases():
    """(form, H, S, Ah, A, B, J, T, p_out per net, obs_index kind, dead ReLUs)."""
    cases = []
    for f, (form, H) in enumerate(FORMS):
        for i, (S, Ah, A) in enumerate(OBS_SHAPES):
            B, J = BJS[(i + f) % 3]
            cases.append((form, H, S, Ah, A, B, J, 2 + (i + f) % 3, _P_SPECS[(i + f) % 5], _INDEX[(i + 2 * f) % 5], False))
        cases.append((form, H, 65, 63, 9, 3, 2, 4, (True, True), "ends", True))
    return cases


def obs_case_data(case):
    """-> dict(obs [NRING, T+1, J, S], index (list or None), nets = [agent_weights ...])."""
    form, H, S, Ah, A, B, J, T, ps, kind, dead = case
    rng = _rng("obs", H, S, Ah, A, B, J, T, len(ps), kind, int(dead))
    obs = rng.standard_normal((NRING, T + 1, J, S)).astype(f32)
    index = {"none": None, "dup": [(3 * b) % 2 + 1 for b in range(B)],
             "ends": [0 if b % 2 == 0 else NRING - 1 for b in range(B)]}[kind]
    nets = [agent_weights(rng, S, H, Ah, A, dead) for _ in ps]
    return dict(obs=obs, index=index, nets=nets)


def obs_case_expect(case):
    """-> per net ((h model, h restatement), (P model, P restatement))."""
    B, T = case[5], case[7]
    d = obs_case_data(case)
    rows = list(range(B)) if d["index"] is None else d["index"]
    out = []
    for w in d["nets"]:
        h64, p64 = scan_from_obs(d["obs"], rows, w, T, True, f64)
        h32, p32 = scan_from_obs(d["obs"], rows, w, T, True, f32)
        out.append(((h64, h32), (p64, p32)))
    return out


GATE_NS = [1, 63, 64, 65]
GATE_HS = [4, 12, 64, 128]
GATE_VARIANTS = ["vector", "base4", "oddld", "bcast"]   # the 16-byte path; the scalar path entered by a base 4 bytes off
#                                                        16 and by a row stride that is no multiple of 4; gi_ld = 0


def gates_case_data(N, H, variant):
    """gi [N, 3H] ([1, 3H] for the broadcast row), gh [N, 3H], h [N, H] with the saturating values in both operands."""
    rng = _rng("gates", N, H, variant)
    gi = rng.standard_normal((1 if variant == "bcast" else N, 3 * H)).astype(f32)
    gh = rng.standard_normal((N, 3 * H)).astype(f32)
    h = (0.5 * rng.standard_normal((N, H))).astype(f32)
    h[:, 0], h[:, 1], h[:, 2] = 0.0, 1.0, -1.0
    if H >= 12:
        saturate(gi, H)
        saturate(gh[1::2], H)    # odd rows: saturated in both operands (+-60 .. +-2e4); even rows: in gi only
    else:                        # H = 4: r sees +-30, +-100 and z +-1e4 from gi; on odd rows z sees +-30 and n the rest from gh
        gi[:, 0:6] = SAT
        gh[1::2, 6:12] = SAT
    return dict(gi=gi, gh=gh, h=h)


def gates_expect(d):
    return gates(d["gi"], d["gh"], d["h"], f64), gates(d["gi"], d["gh"], d["h"], f32)


# the prefetch: n batches of one launch; per batch (offset, no_draw).  tensors: (row bytes, destination pitch or 0,
# source base offset in bytes, destination base offset in bytes) — rows of 4 / 12 bytes on the 4-byte copy path, rows of
# 16 / 48 bytes once with 16-byte aligned bases (16-byte path) and once 4 bytes off (4-byte path)
_T4 = [(4, 0, 0, 0), (12, 20, 0, 0), (16, 0, 0, 0), (48, 64, 0, 0), (16, 0, 4, 0), (48, 0, 0, 4), (16, 32, 4, 4), (48, 52, 0, 0)]
PREFETCH_CASES = [
    # key, n, B, J, T1 (scan steps), N stored, [(offset, no_draw)], gather_blocks, tensors, (S, Ah, A)
    ("one", 1, 1, 1, 2, 7, [(0, 0)], 1, _T4[:1], (5, 7, 3)),
    ("few", 1, 2, 3, 4, 1, [(3, 0)], 3, _T4, (9, 63, 5)),
    ("pair", 2, 5, 3, 5, 8, [(0, 0), (3, 1)], 0, _T4, (65, 65, 9)),
    ("four", 4, 5, 1, 4, 9, [(0, 0), (1, 1), (2, 0), (3, 1)], 1000000, _T4[:1], (17, 33, 17)),
    ("four7", 4, 2, 3, 2, 7, [(3, 1), (0, 0), (3, 0), (1, 0)], 3, _T4, (9, 12, 4)),
    ("last", 2, 5, 1, 5, 9, [(0, 1), (0, 1)], 1, _T4[2:4], (5, 7, 3)),
    ("wide", 1, 1024, 1, 2, 9, [(3, 0)], 0, _T4[:3], (4, 8, 2)),
]
PREFETCH_RING = 9
PREFETCH_SEED, PREFETCH_COUNTER = 0x5EED1234ABCD, 11


def prefetch_case_data(key):
    """-> dict(ring (obs, filled, srcs as uint8 [NR, row_bytes]), w, presets (idx_out as found, per batch), idx (the index
    of every batch), Tm1)."""
    _, n, B, J, T1, N, slots, G, tensors, (S, Ah, A) = next(c for c in PREFETCH_CASES if c[0] == key)
    rng = _rng("prefetch", key)
    NR = PREFETCH_RING
    Tf = max(1, T1 - 1)
    Tm1 = max(1, Tf - 1) if T1 > 2 else 1
    obs = rng.standard_normal((NR, T1, J, S)).astype(f32)
    filled = np.zeros((NR, Tf, 1), np.bool_)
    for e in range(NR):
        filled[e, :1 + e % Tf] = True
        if e % 4 == 3:
            filled[e] = False
    srcs = [rng.integers(0, 256, size=(NR, rb), dtype=np.uint8) for rb, _, _, _ in tensors]
    w = agent_weights(rng, S, 64, Ah, A)
    presets, idx = [], []
    for i, (off, nd) in enumerate(slots):
        pre = [(NR - 1 - 2 * t - i) % NR for t in range(B)]     # names the last ring row first
        presets.append(pre)
        idx.append(pre if nd else draw_indices(B, N, PREFETCH_COUNTER + off, PREFETCH_SEED))
    return dict(ring=dict(obs=obs, filled=filled, srcs=srcs), w=w, presets=presets, idx=idx, Tm1=Tm1)
