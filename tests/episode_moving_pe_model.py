"""Float64 model of ``macjd_agent_episode_moving_pe`` (the agent side of an episode batch on per-env moving frames),
written from the contract comment in include/macjd_nets.h (``macjd_agent_episode_moving_pe_io``) — not from the kernel — with
its float32 restatement and the case table that tests/test_episode_moving_pe_cpu.py proves fair and
tests/test_episode_moving_pe_gpu.py runs.  Plain NumPy; it shares no code with the package.  It composes the existing test
models: tests/rollout_agent_model.py (``mlp``, ``gru_cell``, ``qhead_base``, ``qhead_all``, ``select``, ``check_choice``,
``cap``, ``gamma``, FACTOR, GAP, NONBINDING_SHARE) and, through ``gru_cell``, the gate expressions of tests/gru_scan_model.py
(whose FLOOR_H is the floor of the hidden-state tolerance).

Step t, row n = e J + j (every operation takes ``dt``: float64 the model, float32 the restatement with sums in k order):
  obs[e]  = state[e, :S] with column position_columns[p] <- positions[e, min(step0[e] + t, F), p]
  gi      = W_ih ReLU(fc1 obs + b) + b_ih,  P = sigmoid(L3 ReLU(L2 ReLU(L1 obs)))            (once per env, repeated per agent)
  h_t     = GRUCell(gi, h_(t-1));  Q_a = w2 . ReLU(W1[:, :H] h_t + b1 + W1[:, H + a] + W1[:, H + A] P_a) + b2
  choice  = masked first arg-max, or the Philox draw of (row n, counter_base + t + 1) when it explores

Tolerances, rollout_agent_model's rule with nothing new:
* P: min(``mlp``'s bound, cap).
* Q: ``qhead_all``'s bound + the base bound + |w2| . |W1[:, H + A]| tol(P); the minimum of that and cap is asserted.
* h, teacher-forced and free-running: min(cap, max(FLOOR_H, 8 x the float32 restatement's deviation)); the restatement
  includes the first layers and gi.
* a greedy row is binding when the leader's lead exceeds 4 x tol(Q).
Scenario-scale inputs (coordinates of several hundred) are not model cases: at +-400 the restatement alone deviates by more
than the cap.  They are covered by tests/test_moving_pe_rollout_gpu.py against the package's step path.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gru_scan_model as gm  # noqa: E402
import rollout_agent_model as m  # noqa: E402

f32, f64 = np.float32, np.float64
H, AH = 64, 128
# (J, R, A) -> state width S and the position columns of a state row in state order (per radar x, y; then per jammer x, y):
# the ring scenarios' own (tests/test_episode_moving_pe_cpu.py holds them against the package's Scenario)
SIZES = {(3, 4, 9): (46, (8, 9, 18, 19, 28, 29, 38, 39, 40, 41, 42, 43, 44, 45)),
         (2, 2, 5): (24, (8, 9, 18, 19, 20, 21, 22, 23))}
EP_E = (1, 15, 16, 17, 33)
EP_T = (1, 2, 7)
EP_F = (1, 5)
EP_TILE = (4, 24, 256)
EP_STEP = (None, "zero", "stagger")
EP_AVAIL = (None, "i32", "i64")
EP_EPS = ("mixed", "greedy", "ones")
EP_COUNTER = (None, 1000, 2 ** 32 - 2)


def _case(name, size, E, i, T=None, F=None, tile=None, step=None, scale=1.0, salt=0):
    """Case number i takes option i mod len(options) of every list (shifted so that the lists do not move in step); the
    coverage test checks what the table reaches.  salt re-draws a case's data."""
    J, R, A = size
    T = EP_T[i % 3] if T is None else T
    eps_kind = EP_EPS[(i + i // 3) % 3]
    eps = None if eps_kind == "greedy" else ([1.0] * T if eps_kind == "ones" else [(0.0, 0.3, 1.0)[(i + k) % 3] for k in range(T)])
    return dict(name=name, J=J, R=R, A=A, S=SIZES[size][0], H=H, E=E, T=T, F=EP_F[(i // 2) % 2] if F is None else F,
                tile=EP_TILE[(i + i // 5) % 3] if tile is None else tile, step=EP_STEP[(i + i // 2) % 3] if step is None else step,
                st_pad=3 * (i % 2), cols="own" if (i // 3) % 2 == 0 else "shuffled", h0=bool((i // 2) % 2),
                avail=EP_AVAIL[(i + i // 4) % 3], eps=eps, counter_base=EP_COUNTER[(i + i // 6) % 3], seed=2 ** 35 + 29 * i + 3,
                w1_pad=5 * ((i // 2) % 2), w1_off=(i // 3) % 2, h_final=bool(i % 2 or T == 1), scale=scale, salt=salt)


def cases():
    c, i = [], 0
    for size in SIZES:
        J = size[0]
        for E in EP_E:
            for k in range(2):
                c.append(_case(f"j{J}-e{E}-{k}", size, E, i))
                i += 1
        # the edges that must meet in ONE case: a tile boundary inside a workgroup, several tiles per workgroup, the clamp
        c.append(_case(f"j{J}-e33-tile24-stagger", size, 33, i, T=7, F=5, tile=24, step="stagger"))
        c.append(_case(f"j{J}-e33-tile4-stagger", size, 33, i + 1, T=7, F=1, tile=4, step="stagger"))
        c.append(_case(f"j{J}-e17-tile256-nullstep", size, 17, i + 2, T=7, F=5, tile=256, step="none"))
        i += 3
    for size in SIZES:   # the family at +-4
        J = size[0]
        c.append(_case(f"pm4-j{J}-e33", size, 33, i, T=7, F=5, tile=24, step="stagger", scale=4.0))
        c.append(_case(f"pm4-j{J}-e17", size, 17, i + 1, T=2, F=1, tile=4, step="zero", scale=4.0))
        i += 2
    for e in c:
        if e["step"] == "none":
            e["step"] = None
    return c


def families():
    """name -> case names: per size the grid, and the +-4 family."""
    out = {"j3": [], "j2": [], "pm4": []}
    for c in cases():
        out["pm4" if c["name"].startswith("pm4") else f"j{c['J']}"].append(c["name"])
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)


def _uniform(rng, shape, fan_in):
    """torch's default initialisation of Linear / GRUCell: uniform +- 1 / sqrt(fan_in), as float32 values."""
    k = 1.0 / np.sqrt(fan_in)
    return rng.uniform(-k, k, size=shape).astype(f32)


def step0(c):
    """The step counters at entry [E] (int64), zeros for a NULL / all-zero ``step``; "stagger": e mod (F + 3), so that some
    envs are at or past F at entry and others cross F inside a launch of T >= 2 steps."""
    E, F = c["E"], c["F"]
    return (np.arange(E) % (F + 3)).astype(np.int64) if c["step"] == "stagger" else np.zeros(E, np.int64)


@functools.lru_cache(maxsize=None)
def _data(name):
    c = case(name)
    rng = m._rng("moving-pe", name, c["salt"])
    J, A, S, E, T, F = c["J"], c["A"], c["S"], c["E"], c["T"], c["F"]
    N = E * J
    n_pos = 2 * c["R"] + 2 * J
    own = np.asarray(SIZES[(J, c["R"], A)][1], np.int32)
    cols = own if c["cols"] == "own" else rng.permutation(S)[:n_pos].astype(np.int32)
    W1, b1, w2, b2 = m.head(rng, H, A, c["w1_pad"])
    d = dict(fc1_w=_uniform(rng, (H, S), S), fc1_b=_uniform(rng, (H,), S),
             w_ih=_uniform(rng, (3 * H, H), H), b_ih=_uniform(rng, (3 * H,), H),
             w_hh=_uniform(rng, (3 * H, H), H), b_hh=_uniform(rng, (3 * H,), H),
             a1_w=_uniform(rng, (AH, S), S), a1_b=_uniform(rng, (AH,), S), a2_w=_uniform(rng, (AH, AH), AH), a2_b=_uniform(rng, (AH,), AH),
             a3_w=_uniform(rng, (A, AH), AH), a3_b=_uniform(rng, (A,), AH), W1=W1, b1=b1, w2=w2, b2=b2, cols=cols)
    s = c["scale"]
    d["state"] = rng.uniform(-s, s, (E, S)).astype(f32)
    d["positions"] = rng.uniform(-s, s, (E, F + 1, n_pos)).astype(f32)
    d["h0"] = np.clip(0.5 * rng.standard_normal((N, H)), -0.99, 0.99).astype(f32) if c["h0"] else None
    d["avail"] = None if c["avail"] is None else m.make_avail(rng, E, J, A)
    return d


def data(c):
    return _data(c["name"])


def observations(c, d, steps=None):
    """f32 [T, E, S]: the observation of every env at every step of the launch (position columns from the clamped frame)."""
    T = c["T"] if steps is None else steps
    s0 = step0(c)
    obs = np.repeat(d["state"][None], T, axis=0).copy()
    e = np.arange(c["E"])
    for t in range(T):
        obs[t][:, d["cols"]] = d["positions"][e, np.minimum(s0 + t, c["F"])]
    return obs


def obs_work(c, d, obs_t, dt=f64):
    """(gi [N, 3H], P [N, A], P's bound [N, A]) of one step's observation rows [E, S], expanded to the agent rows."""
    gi, _ = m.mlp(obs_t, [(d["fc1_w"], d["fc1_b"], m.ACT_RELU), (d["w_ih"], d["b_ih"], m.ACT_NONE)], dt)
    P, perr = m.mlp(obs_t, [(d["a1_w"], d["a1_b"], m.ACT_RELU), (d["a2_w"], d["a2_b"], m.ACT_RELU), (d["a3_w"], d["a3_b"], m.ACT_SIGMOID)], dt)
    J = c["J"]
    return np.repeat(gi, J, axis=0), np.repeat(P, J, axis=0), np.repeat(perr, J, axis=0)


@functools.lru_cache(maxsize=None)
def _inputs(name, dt_name):
    c = case(name)
    d = _data(name)
    dt = f64 if dt_name == "f64" else f32
    obs = observations(c, d)
    return [obs_work(c, d, obs[t], dt) for t in range(c["T"])]


def step_inputs(c, t, dt=f64):
    return _inputs(c["name"], "f64" if dt is f64 else "f32")[t]


def episode_step(c, d, t, h_prev, dt=f64):
    """h_t of step t from the hidden state h_prev [N, H] (teacher-forced: the launch's own stored h_(t-1))."""
    gi, _, _ = step_inputs(c, t, dt)
    return m.gru_cell(gi, h_prev, d["w_hh"], d["b_hh"], dt)


def episode(c, d, dt=f64):
    """Free-running hidden trajectory [T, N, H] from h0."""
    N = c["E"] * c["J"]
    h = np.zeros((N, H), dt) if d["h0"] is None else np.asarray(d["h0"], dt)
    out = np.zeros((c["T"], N, H), dt)
    for t in range(c["T"]):
        h = episode_step(c, d, t, h, dt)
        out[t] = h
    return out


def step_choice(c, d, t, h_t):
    """Actor output, Q-head and selection of step t on the hidden state h_t (float32 values: the launch's stored state or the
    model's).  -> (q, tol(Q), sel, P, tol(P))."""
    N, A = c["E"] * c["J"], c["A"]
    _, P, perr = step_inputs(c, t)
    p_tol = np.minimum(perr, m.cap(P))
    base, base_err = m.qhead_base(np.asarray(h_t, f32), d["W1"], d["b1"])
    W1 = d["W1"][:, :H + A + 1]
    q, err = m.qhead_all(base, P, W1, d["w2"], d["b2"], base_err=base_err)
    err = err + float(np.abs(d["w2"].astype(f64)) @ np.abs(W1[:, H + A].astype(f64))) * p_tol
    tol = np.minimum(err, m.cap(q))
    av = None if d["avail"] is None else d["avail"].reshape(N, A)
    greedy_only = c["eps"] is None
    eps = 0.0 if greedy_only else c["eps"][t]
    cb = 0 if c["counter_base"] is None else c["counter_base"]
    sel = m.select(q, av, eps, c["seed"], cb + t + 1, np.arange(N), greedy_only, tol=tol)
    return q, tol, sel, P, p_tol


def hidden_tolerances(c, d):
    """(teacher-forced tol, free-running tol, worst restatement deviation of either): rollout_agent_model's rule, the
    restatement (first layers, gi and the cell in float32) taken along the MODEL's trajectory."""
    model = episode(c, d)
    dev_free = float(np.abs(episode(c, d, f32).astype(f64) - model).max())
    N = c["E"] * c["J"]
    prev = np.zeros((N, H), f32) if d["h0"] is None else np.asarray(d["h0"], f32)
    dev_step = 0.0
    for t in range(c["T"]):
        dev_step = max(dev_step, float(np.abs(episode_step(c, d, t, prev, f32).astype(f64) - episode_step(c, d, t, prev)).max()))
        prev = model[t].astype(f32)
    rule = lambda dev: min(m.cap(model), max(gm.FLOOR_H, m.FACTOR * dev))
    return rule(dev_step), rule(dev_free), max(dev_step, dev_free)


@functools.lru_cache(maxsize=None)
def _fair(name):
    c = case(name)
    d = _data(name)
    tol_step, tol_free, dev = hidden_tolerances(c, d)
    model = episode(c, d)
    greedy = nonbinding = 0
    q_tol = p_tol = 0.0
    for t in range(c["T"]):
        _, tol, sel, _, ptol = step_choice(c, d, t, model[t].astype(f32))
        greedy += int((~sel["explore"]).sum())
        nonbinding += int((~sel["explore"] & ~sel["binding"]).sum())
        q_tol, p_tol = max(q_tol, float(tol.max())), max(p_tol, float(ptol.max()))
    return dict(tol_step=tol_step, tol_free=tol_free, dev=dev, greedy=greedy, nonbinding=nonbinding, model=model, q_tol=q_tol, p_tol=p_tol)


def fair(c):
    """Tolerances, the model's free-running trajectory and the count of non-binding greedy rows along it."""
    return _fair(c["name"])
