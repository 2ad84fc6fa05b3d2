"""Float64 restatement of the fused QMix mixer's exact-f32 contract (include/macjd_nets.h, ``macjd_mixerf_io`` with
``operand_dtype = 0``) and of the TD loss's gradient, written from the header's formulas: torch on the CPU in float64,
explicit forward and backward expressions (no autograd), nothing imported from the package.

    s~ = LayerNorm(s)                    two-pass, eps inside the root
    [h_w1 | h_wf | h_V | b1_raw] = s~ W1^T + b1, ReLU on the first 2 Hh + Em columns
    w1_raw = h_w1 W2^T + b2   wf_raw = h_wf Wf2^T + bf2   v_raw = h_V . wV2 + bV2
    y = ELU(q . clamp(w1_raw, 0, 5) + clamp(b1_raw, -5, 5)) . clamp(wf_raw, 0, 5) + clamp(v_raw, -5, 5)

Mask decisions.  The gradients are discontinuous at a ReLU or clamp threshold, and a float64 pre-activation within float32
rounding of a threshold may sit on the other side in the kernel.  ``forward_backward`` therefore reports for each of the
five tensors that carry a decision (DECISIONS) the pre-activation (``pre``), the side it lies on (``side``: True = the
gradient passes; ReLU x > 0, clamp lo <= x <= hi, torch's rule) and whether it lies within
``band = BAND * max(1, max|x|)`` of a threshold (``near``).  With ``decisions`` given (same keys, bool tensors) the model
takes the given side on the near elements and its own float64 side everywhere else."""
import numpy as np
import torch

HH, EM = 128, 64                 # hyper_hidden_dim, mixing_embed_dim: the only sizes the kernels cover
NRELU = 2 * HH + EM              # first-layer columns under the ReLU
N1 = 2 * HH + 2 * EM             # merged first layer: hyper_w_1.0 | hyper_w_final.0 | V.0 | hyper_b_1
BAND = 1e-4
LN_EPS = 1e-5
PARAMS = ("ln_w", "ln_b", "W1", "b1", "W2", "b2", "Wf2", "bf2", "wV2", "bV2")
OUTPUTS = ("y", "sn", "xhat", "act", "gq", "gout1", "g_w1raw", "g_wfraw", "g_v")
DECISIONS = ("relu", "w1_raw", "wf_raw", "v_raw", "b1_raw")
THRESHOLDS = {"relu": (0.0,), "w1_raw": (0.0, 5.0), "wf_raw": (0.0, 5.0), "v_raw": (-5.0, 5.0), "b1_raw": (-5.0, 5.0)}


def f64(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    return t.detach().cpu().to(torch.float64)


def param_shapes(J, S):
    return {"ln_w": (S,), "ln_b": (S,), "W1": (N1, S), "b1": (N1,), "W2": (J * EM, HH), "b2": (J * EM,),
            "Wf2": (EM, HH), "bf2": (EM,), "wV2": (EM,), "bV2": (1,)}


def raw_params(rng, J, S, scale=3.0):
    """Raw float32 parameter arrays with the header's shapes: nn.Linear-style uniform(-1/sqrt(fan_in), 1/sqrt(fan_in))
    times ``scale`` (x3: every clamp gets elements on both sides), LayerNorm weight around 1 / bias around 0 likewise
    spread, from a NumPy generator — any S, no scenario needed."""
    u = lambda shape, fan_in: (scale * rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in)).astype(np.float32)
    p = {"ln_w": (1.0 + 0.5 * rng.uniform(-1.0, 1.0, (S,))).astype(np.float32), "ln_b": u((S,), 4.0),
         "W1": u((N1, S), S), "b1": u((N1,), S), "W2": u((J * EM, HH), HH), "b2": u((J * EM,), HH),
         "Wf2": u((EM, HH), HH), "bf2": u((EM,), HH), "wV2": u((EM,), EM), "bV2": u((1,), EM)}
    p["eps"] = LN_EPS
    return p


def params_from_state_dict(sd, eps=LN_EPS):
    """The header's merged layout from a QMixer state dict (reference core/networks.py:215-248)."""
    g = lambda k: f64(sd[k])
    return {"ln_w": g("state_norm.weight"), "ln_b": g("state_norm.bias"),
            "W1": torch.cat([g("hyper_w_1.0.weight"), g("hyper_w_final.0.weight"), g("V.0.weight"), g("hyper_b_1.weight")], 0),
            "b1": torch.cat([g("hyper_w_1.0.bias"), g("hyper_w_final.0.bias"), g("V.0.bias"), g("hyper_b_1.bias")]),
            "W2": g("hyper_w_1.2.weight"), "b2": g("hyper_w_1.2.bias"), "Wf2": g("hyper_w_final.2.weight"),
            "bf2": g("hyper_w_final.2.bias"), "wV2": g("V.2.weight").reshape(-1), "bV2": g("V.2.bias").reshape(-1), "eps": eps}


def state_dict_grads(grads, S):
    """The model's parameter gradients under QMixer's parameter names (the merged first layer split into its rows)."""
    W1, b1 = grads["W1"], grads["b1"]
    rows = {"hyper_w_1.0": slice(0, HH), "hyper_w_final.0": slice(HH, 2 * HH), "V.0": slice(2 * HH, NRELU),
            "hyper_b_1": slice(NRELU, N1)}
    out = {"state_norm.weight": grads["ln_w"], "state_norm.bias": grads["ln_b"], "hyper_w_1.2.weight": grads["W2"],
           "hyper_w_1.2.bias": grads["b2"], "hyper_w_final.2.weight": grads["Wf2"], "hyper_w_final.2.bias": grads["bf2"],
           "V.2.weight": grads["wV2"].reshape(1, EM), "V.2.bias": grads["bV2"].reshape(1)}
    for name, sl in rows.items():
        out[name + ".weight"], out[name + ".bias"] = W1[sl], b1[sl]
    return out


def _near(x, thresholds):
    band = BAND * max(1.0, float(x.abs().max()) if x.numel() else 0.0)
    near = torch.zeros_like(x, dtype=torch.bool)
    for t in thresholds:
        near |= (x - t).abs() < band
    return near


def _side(name, x):
    th = THRESHOLDS[name]
    return x > th[0] if len(th) == 1 else (x >= th[0]) & (x <= th[1])


def forward_backward(params, q, s, gy, decisions=None):
    """The whole chain and its gradients in float64.  params: PARAMS + "eps"; q [M, J], s [M, S], gy [M].  Returns a dict
    with every tensor the kernels write (OUTPUTS), "grads" (the parameter gradients, PARAMS' names), "pre" / "side" /
    "near" (per DECISIONS name, see the module docstring), "readable" (where the side shows in the kernel's outputs; where a
    clamp's unmasked gradient is zero the decision has no effect) and the counts "n_decisions" / "n_near" / "n_blind"
    (near-threshold clamp decisions that cannot be read off the kernel's outputs and whose gradient exceeds 1e-6 of the
    tensor's largest: a case must have none, so an unread side moves no element by more than 1e-6 max|.|)."""
    p = {k: f64(params[k]) for k in PARAMS}
    eps = float(params["eps"])
    q, s, gy = f64(q), f64(s), f64(gy).reshape(-1)
    M, J = q.shape
    # ---- forward ----
    mean = s.mean(1, keepdim=True)
    var = ((s - mean) ** 2).mean(1, keepdim=True)
    xhat = (s - mean) / torch.sqrt(var + eps)
    sn = xhat * p["ln_w"] + p["ln_b"]
    out1 = sn @ p["W1"].T + p["b1"]
    pre = {"relu": out1[:, :NRELU], "b1_raw": out1[:, NRELU:]}

    def decide(name):
        side, near = _side(name, pre[name]), _near(pre[name], THRESHOLDS[name])
        if decisions is not None:
            side = torch.where(near, decisions[name].reshape(side.shape).bool(), side)
        return side, near

    side, near = {}, {}
    side["relu"], near["relu"] = decide("relu")
    relu_out = torch.where(side["relu"], pre["relu"], torch.zeros_like(pre["relu"]))
    act = torch.cat([relu_out, pre["b1_raw"]], 1)
    h_w1, h_wf, h_v = act[:, :HH], act[:, HH:2 * HH], act[:, 2 * HH:NRELU]
    pre["w1_raw"] = (h_w1 @ p["W2"].T + p["b2"]).view(M, J, EM)
    pre["wf_raw"] = h_wf @ p["Wf2"].T + p["bf2"]
    pre["v_raw"] = h_v @ p["wV2"] + p["bV2"]
    for name in ("w1_raw", "wf_raw", "v_raw", "b1_raw"):
        side[name], near[name] = decide(name)
    w1, wf = pre["w1_raw"].clamp(0.0, 5.0), pre["wf_raw"].clamp(0.0, 5.0)
    hid = (q[:, :, None] * w1).sum(1) + pre["b1_raw"].clamp(-5.0, 5.0)
    h = torch.where(hid > 0, hid, torch.expm1(hid))
    y = (h * wf).sum(1) + pre["v_raw"].clamp(-5.0, 5.0)
    # ---- backward ----
    zero = lambda t: torch.zeros_like(t)
    delu = torch.where(hid > 0, torch.ones_like(hid), torch.exp(hid))
    ghid = gy[:, None] * wf * delu
    unmasked = {"w1_raw": ghid[:, None, :] * q[:, :, None], "wf_raw": gy[:, None] * h, "v_raw": gy, "b1_raw": ghid}
    # where a clamp's side can be read off the kernel's gradient (zero or not): the unmasked gradient is non-zero and none of
    # its factors can vanish in float32 (ELU' = exp(hid) rounds to 0 below 2^-25; clamp(wf_raw) next to 0 may be 0 there)
    live = (gy != 0)[:, None] & (wf > 1e-3) & (delu > 1e-6)
    readable = {"relu": torch.ones_like(side["relu"]), "w1_raw": live[:, None, :] & (q != 0)[:, :, None],
                "wf_raw": (gy != 0)[:, None] & (h.abs() > 1e-6), "v_raw": gy != 0, "b1_raw": live}
    g_w1 = torch.where(side["w1_raw"], unmasked["w1_raw"], zero(unmasked["w1_raw"])).reshape(M, J * EM)
    g_wf = torch.where(side["wf_raw"], unmasked["wf_raw"], zero(h))
    g_v = torch.where(side["v_raw"], gy, zero(gy))
    g_b1 = torch.where(side["b1_raw"], ghid, zero(ghid))
    gq = (ghid[:, None, :] * w1).sum(2)
    mask = side["relu"].to(torch.float64)
    gout1 = torch.cat([(g_w1 @ p["W2"]) * mask[:, :HH], (g_wf @ p["Wf2"]) * mask[:, HH:2 * HH],
                       g_v[:, None] * p["wV2"][None, :] * mask[:, 2 * HH:], g_b1], 1)
    G = gout1 @ p["W1"]                                            # dL/d s~
    grads = {"W1": gout1.T @ sn, "b1": gout1.sum(0), "W2": g_w1.T @ h_w1, "b2": g_w1.sum(0), "Wf2": g_wf.T @ h_wf,
             "bf2": g_wf.sum(0), "wV2": g_v @ h_v, "bV2": g_v.sum().reshape(1), "ln_w": (G * xhat).sum(0), "ln_b": G.sum(0)}
    return {"y": y, "sn": sn, "xhat": xhat, "act": act, "gq": gq, "gout1": gout1, "g_w1raw": g_w1, "g_wfraw": g_wf,
            "g_v": g_v, "grads": grads, "pre": pre, "side": side, "near": near, "readable": readable,
            "n_decisions": sum(int(v.numel()) for v in near.values()), "n_near": sum(int(v.sum()) for v in near.values()),
            "n_blind": sum(int((near[k] & ~readable[k] & (unmasked[k].abs() > 1e-6 * unmasked[k].abs().max())).sum())
                           for k in unmasked)}


def td_gradient(y, tq, reward, terminated, filled, gamma):
    """dL/dy of the masked TD loss (reference core/qmix.py:155,190-194) on [B, T1] arrays: eval row (b, t) against the
    target's row (b, t + 1),
        gy[b, t] = 2 filled (y[b, t] - (r + gamma (1 - term) tq[b, t + 1])) / sum(filled[:, :T1-1])   for t < T1 - 1
    and 0 for t = T1 - 1.  -> (gy [B, T1], loss, mean(y[:, :T1-1]), mean(target))."""
    y, tq, r = f64(y), f64(tq), f64(reward)
    term, m = f64(terminated)[:, :-1], f64(filled)[:, :-1]
    target = r[:, :-1] + gamma * (1.0 - term) * tq[:, 1:]
    err = (y[:, :-1] - target) * m
    tot = m.sum()
    gy = torch.zeros_like(y)
    gy[:, :-1] = 2.0 * err / tot
    return gy, (err ** 2).sum() / tot, y[:, :-1].mean(), target.mean()


def td_reference(pe, q_e, state, tq, reward, terminated, filled, gamma, decisions=None):
    """One update's mixer half: the eval mixer's forward on [B, T1] rows, ``td_gradient`` against the target values tq
    [B, T1], the eval mixer's backward.  -> (forward_backward's dict, (loss, mean y, mean target))."""
    B, T1, J = q_e.shape
    M = B * T1
    q2, s2 = f64(q_e).reshape(M, J), f64(state).reshape(M, -1)
    y = forward_backward(pe, q2, s2, torch.zeros(M), decisions)["y"]     # (y does not depend on the decisions' sides)
    gy, loss, mean_y, mean_t = td_gradient(y.view(B, T1), f64(tq).reshape(B, T1), f64(reward).reshape(B, T1),
                                           f64(terminated).reshape(B, T1), f64(filled).reshape(B, T1), gamma)
    return forward_backward(pe, q2, s2, gy.reshape(M), decisions), (loss, mean_y, mean_t)


def target_values(pt, q_t, state):
    """The target mixer's Q_tot [B, T1] (forward only)."""
    B, T1, J = q_t.shape
    M = B * T1
    return forward_backward(pt, f64(q_t).reshape(M, J), f64(state).reshape(M, -1), torch.zeros(M))["y"].view(B, T1)


# ---------------------------------------------------------------------------------------------------------------
# The case table of tests/test_mixer_f64_gpu.py: tests/test_mixer_f64_cpu.py asserts the decisions cap on every entry
# from the model alone, with the inputs made here from the same seeds.
JS = (2, 3, 6, 12)
SHIPPED_S = {2: 24, 3: 46, 6: 92, 12: 184}
MS = (1, 15, 16, 17, 33)
TD_BATCHES = ((1, 2), (3, 5), (2, 16), (3, 17), (5, 23))
NARROW_S = 5                     # S <= 16 (J - 1) at every J: the kernels' narrow-row variants
MODULE_BATCH = (3, 17)
GAMMA = 0.99
CAP = 0.005


def td_cases(J):
    """(B, T1, S): every batch at the shipped width, one at a narrow width (the narrow pair / training kernels)."""
    return [(B, T1, SHIPPED_S[J]) for B, T1 in TD_BATCHES] + [(3, 17, NARROW_S)]


def widths(J):
    return (1, 5, 16 * J - 1, 16 * J, SHIPPED_S[J])


def fwd_bwd_cases():
    """(J, S, M, layout): layout "plain", "s_ld" (the state is a column slice of a wider tensor) or "flat" (every
    parameter a view at an odd float offset of one flat vector), the last two once per J."""
    cases = [(J, S, M, "plain") for J in JS for S in widths(J) for M in MS]
    for J in JS:
        cases += [(J, SHIPPED_S[J], 33, "s_ld"), (J, 16 * J - 1, 17, "flat")]
    return cases


def case_seed(*key):
    return [20260 + 7 * i + int(k) for i, k in enumerate(key)]


def fwd_bwd_inputs(J, S, M, layout="plain"):
    """(params, q, s, gy) float32 arrays of one forward / backward case; states 3 N(0, 1)."""
    rng = np.random.default_rng(case_seed(J, S, M, ("plain", "s_ld", "flat").index(layout)))
    p = raw_params(rng, J, S)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return p, f(M, J), 3.0 * f(M, S), f(M)


def degenerate_inputs(J, S):
    """33 rows (three tiles, the last one ragged); some state rows all zero, some a constant small integer."""
    M = 33
    rng = np.random.default_rng(case_seed(J, S, 99))
    p = raw_params(rng, J, S)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    q, s, gy = f(M, J), 3.0 * f(M, S), f(M)
    zero_rows, const_rows = [0, 7, 16, 32], [3, 15, 17, 31]
    s[zero_rows] = 0.0
    for i, r in enumerate(const_rows):
        s[r] = float(i - 1 if i != 1 else 3)     # -1, 3, 1, 2
    return p, q, s, gy, zero_rows + const_rows


def td_inputs(J, B, T1, salt=7, S=None):
    """One learner batch at the shipped width of J: eval / target parameters, Q-values, states, reward and the episode
    structure — episode 0 has one filled step and terminates at t = 0, the last episode runs the full length and never
    terminates, ragged ones between."""
    S = SHIPPED_S[J] if S is None else S
    rng = np.random.default_rng(case_seed(J, B, T1, salt, S))
    pe, pt = raw_params(rng, J, S), raw_params(rng, J, S)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    q_e, q_t, state, reward = f(B, T1, J), f(B, T1, J), 3.0 * f(B, T1, S), f(B, T1, 1)
    lens = np.empty(B, dtype=np.int64)
    lens[:] = rng.integers(2, T1, B) if T1 > 2 else 1
    lens[0] = 1
    terminates = np.ones(B, dtype=bool)
    if B > 1:
        lens[-1], terminates[-1] = T1, False
    steps = np.arange(T1)[None, :, None]
    filled = steps < lens[:, None, None]
    terminated = (steps == lens[:, None, None] - 1) & terminates[:, None, None]
    return pe, pt, q_e, q_t, state, reward, terminated, filled


def x3_mixer(QMixer, args):
    """The x3 weight set: ``QMixer`` initialised under torch.manual_seed(5), every parameter multiplied by 3."""
    torch.manual_seed(5)
    m = QMixer(args)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)
    return m


def module_inputs(J):
    """The batch of the through-the-module test at the shipped width of J: (q, tq, state, reward, terminated, filled) as
    in ``td_inputs``, B = 3, T1 = 17; tq [B, T1, 1] stands in for a target mixer's output (any values will do)."""
    _, _, q, q_t, state, reward, terminated, filled = td_inputs(J, *MODULE_BATCH, salt=11)
    return q, q_t.sum(-1, keepdims=True), state, reward, terminated, filled
