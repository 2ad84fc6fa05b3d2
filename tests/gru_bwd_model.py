"""Float64 models behind the GRU backward tests (test infrastructure; shares no code with macjd_amd.ops).

(The header's reverse-time formulas themselves are restated in tests/test_gru_bwd_cpu.py and proved there against these.)
* ``autograd_reference``: stock float64 autograd of the step-by-step recurrence, with the per-step gh kept as a
  graph node so that dL/dgh can be read as well.
* ``grucell_reference``: the same gradients through ``torch.nn.GRUCell`` (identity input weights, so that x_t = gi_t).
* ``train_body_loss``: the learner's whole loss with a differentiable agent body, restated with stock modules.
"""
import numpy as np
import torch
import torch.nn.functional as F


def autograd_reference(gi, w_hh, b_hh, dh_all, h0=None):
    """Float64 stock autograd of the stepping loop, seeded with dh_all on the stacked hidden states.
    Returns dict(h_all, gh, dgi, dgh, dh0, dW_hh, db_hh) as NumPy float64 (dh0 = None without h0)."""
    gi = torch.tensor(np.asarray(gi, np.float64), requires_grad=True)
    w = torch.tensor(np.asarray(w_hh, np.float64), requires_grad=True)
    bb = torch.tensor(np.asarray(b_hh, np.float64), requires_grad=True)
    B, T, J, H3 = gi.shape
    H = H3 // 3
    h_in = None if h0 is None else torch.tensor(np.asarray(h0, np.float64).reshape(B, J, H), requires_grad=True)
    h = torch.zeros(B, J, H, dtype=torch.float64) if h_in is None else h_in
    hs, ghs = [], []
    for t in range(T):
        gh = F.linear(h, w, bb)
        gh.retain_grad()
        r = torch.sigmoid(gi[:, t, :, :H] + gh[..., :H])
        z = torch.sigmoid(gi[:, t, :, H:2 * H] + gh[..., H:2 * H])
        n = torch.tanh(gi[:, t, :, 2 * H:] + r * gh[..., 2 * H:])
        h = (h - n) * z + n
        hs.append(h)
        ghs.append(gh)
    h_all = torch.stack(hs, dim=1)
    h_all.backward(torch.tensor(np.asarray(dh_all, np.float64)))
    return dict(h_all=h_all.detach().numpy(), gh=torch.stack([g.detach() for g in ghs], 1).numpy(),
                dgi=gi.grad.numpy(), dgh=torch.stack([g.grad for g in ghs], 1).numpy(),
                dh0=None if h_in is None else h_in.grad.numpy(), dW_hh=w.grad.numpy(), db_hh=bb.grad.numpy())


def grucell_reference(gi, w_hh, b_hh, dh_all, h0=None):
    """The same gradients through torch.nn.GRUCell in float64: input size 3H with identity input weights and a zero
    input bias, so that the cell's W_ih x + b_ih is gi itself."""
    gi = torch.tensor(np.asarray(gi, np.float64), requires_grad=True)
    B, T, J, H3 = gi.shape
    H = H3 // 3
    cell = torch.nn.GRUCell(H3, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(H3, dtype=torch.float64))
        cell.bias_ih.zero_()
        cell.weight_hh.copy_(torch.tensor(np.asarray(w_hh, np.float64)))
        cell.bias_hh.copy_(torch.tensor(np.asarray(b_hh, np.float64)))
    h_in = None if h0 is None else torch.tensor(np.asarray(h0, np.float64).reshape(B * J, H), requires_grad=True)
    h = torch.zeros(B * J, H, dtype=torch.float64) if h_in is None else h_in
    hs = []
    for t in range(T):
        h = cell(gi[:, t].reshape(B * J, H3), h)
        hs.append(h.view(B, J, H))
    torch.stack(hs, dim=1).backward(torch.tensor(np.asarray(dh_all, np.float64)))
    return dict(dgi=gi.grad.numpy(), dh0=None if h_in is None else h_in.grad.numpy().reshape(B, J, H),
                dW_hh=cell.weight_hh.grad.numpy(), db_hh=cell.bias_hh.grad.numpy())


def rel_err(got, ref):
    """max|got - ref| / max|ref| (0 / 0 counts as 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    diff = float(np.abs(got - ref).max()) if ref.size else 0.0
    return diff / scale if scale > 0 else diff


# --------------------------------------------------------------------------------------------- learner
def make_batch(rng, B, T, J, S, A, H):
    """A learner batch of B full-length episodes with T steps (T+1 rows of state / obs / hidden_state)."""
    return {
        "state": rng.standard_normal((B, T + 1, S)).astype(np.float32),
        "obs": rng.standard_normal((B, T + 1, J, S)).astype(np.float32),
        "actions_discrete": rng.integers(0, A, size=(B, T, J, 1)).astype(np.int32),
        "actions_continuous": rng.random((B, T, J, 1)).astype(np.float32),
        "reward": rng.standard_normal((B, T, 1)).astype(np.float32),
        "terminated": np.zeros((B, T, 1), dtype=bool),
        "filled": np.ones((B, T, 1), dtype=bool),
        "hidden_state": np.zeros((B, T + 1, J, H), dtype=np.float32),
        "max_seq_len": T,
    }


def _mixer(sd, q, s, J):
    """QMixer.forward with stock ops from a state dict: q [M,J], s [M,S] -> [M,1]."""
    x = F.layer_norm(s, (s.shape[1],), sd["state_norm.weight"], sd["state_norm.bias"], 1e-5)
    two = lambda p: F.linear(F.relu(F.linear(x, sd[p + ".0.weight"], sd[p + ".0.bias"])), sd[p + ".2.weight"], sd[p + ".2.bias"])
    M = q.shape[0]
    w1 = two("hyper_w_1").clamp(0.0, 5.0).view(M, J, -1)
    b1 = F.linear(x, sd["hyper_b_1.weight"], sd["hyper_b_1.bias"]).clamp(-5.0, 5.0)
    wf = two("hyper_w_final").clamp(0.0, 5.0)
    v = two("V").clamp(-5.0, 5.0)
    hidden = F.elu(torch.bmm(q.view(M, 1, J), w1).squeeze(1) + b1)
    return (hidden * wf).sum(1, keepdim=True) + v


def train_body_loss(agent_sd, tagent_sd, mixer_sd, tmixer_sd, batch, gamma, dtype=torch.float64):
    """The learner's loss with the eval agent's fc1 / GRU inside the graph, written with torch.nn.GRUCell stepping
    loops and per-action Q-head evaluations.  Returns (loss, {name: leaf tensor} of the eval agent and mixer, extras)
    where extras holds the fc1 / Q-head pre-activations of the eval network and the top-2 gap of its all-action Q at the
    Double-DQN steps (for the tests' ReLU-margin and argmax-margin conditions)."""
    T = int(batch["max_seq_len"])
    leaf = lambda sd: {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    ag, mx = leaf(agent_sd), leaf(mixer_sd)
    tag = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in tagent_sd.items()}
    tmx = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in tmixer_sd.items()}
    obs = torch.as_tensor(batch["obs"]).to(dtype)[:, :T]
    state = torch.as_tensor(batch["state"]).to(dtype)[:, :T]
    B, _, J, S = obs.shape
    H = ag["rnn.weight_hh"].shape[1]
    A = ag["actor.4.weight"].shape[0]

    def unroll(p):
        cell = lambda x, h: torch._VF.gru_cell(x, h, p["rnn.weight_ih"], p["rnn.weight_hh"], p["rnn.bias_ih"], p["rnn.bias_hh"])
        h = torch.zeros(B * J, H, dtype=dtype)
        hs, pre = [], []
        for t in range(T):
            a1 = F.linear(obs[:, t].reshape(B * J, S), p["fc1.weight"], p["fc1.bias"])
            pre.append(a1)
            h = cell(F.relu(a1), h)
            hs.append(h.view(B, J, H))
        return torch.stack(hs, dim=1), torch.stack(pre, dim=0)

    def qhead(p, h, a_idx, P):   # h [n,H], a_idx [n], P [n] -> (q [n], first-layer pre-activation)
        x = torch.cat([h, F.one_hot(a_idx.long(), A).to(dtype), P.reshape(-1, 1)], dim=1)
        a1 = F.linear(x, p["fc2_q_head.0.weight"], p["fc2_q_head.0.bias"])
        return F.linear(F.relu(a1), p["fc2_q_head.2.weight"], p["fc2_q_head.2.bias"]).squeeze(1), a1

    def actor(p, rows):
        x = F.relu(F.linear(rows, p["actor.0.weight"], p["actor.0.bias"]))
        x = F.relu(F.linear(x, p["actor.2.weight"], p["actor.2.bias"]))
        return torch.sigmoid(F.linear(x, p["actor.4.weight"], p["actor.4.bias"]))

    def q_all(p, h_all):
        n = B * T * J
        P = actor(p, obs.reshape(n, S))
        return torch.stack([qhead(p, h_all.reshape(n, H), torch.full((n,), a), P[:, a])[0] for a in range(A)], 1).view(B, T, J, A)

    h_eval, fc1_pre = unroll(ag)
    with torch.no_grad():
        h_tgt, _ = unroll(tag)
        q_eval_all = q_all(ag, h_eval.detach())[:, 1:]
        next_a = q_eval_all.argmax(dim=3, keepdim=True)
        top2 = q_eval_all.topk(2, dim=3).values
        tq = torch.gather(q_all(tag, h_tgt)[:, 1:], 3, next_a).squeeze(3)
        tq_tot = _mixer(tmx, tq.reshape(-1, J), state[:, 1:].reshape(-1, state.shape[-1]), J).view(B, T - 1, 1)
    n_eff = B * (T - 1) * J
    q_taken, q_pre = qhead(ag, h_eval[:, :T - 1].reshape(n_eff, H),
                           torch.as_tensor(batch["actions_discrete"])[:, :T - 1].reshape(n_eff),
                           torch.as_tensor(batch["actions_continuous"]).to(dtype)[:, :T - 1].reshape(n_eff))
    q_tot = _mixer(mx, q_taken.view(-1, J), state[:, :-1].reshape(-1, state.shape[-1]), J).view(B, T - 1, 1)
    reward = torch.as_tensor(batch["reward"]).to(dtype)[:, :T - 1]
    term = torch.as_tensor(batch["terminated"]).to(dtype)[:, :T - 1]
    m = torch.as_tensor(batch["filled"]).to(dtype)[:, :T - 1]
    targets = reward + gamma * (1 - term) * tq_tot
    loss = (((q_tot - targets) * m) ** 2).sum() / m.sum()
    named = {"agent." + k: v for k, v in ag.items()}
    named.update({"mixer." + k: v for k, v in mx.items()})
    return loss, named, dict(fc1_pre=fc1_pre.detach(), q_pre=q_pre.detach(), h_eval=h_eval.detach(),
                             argmax_gap=(top2[..., 0] - top2[..., 1]), q_eval_all=q_eval_all)
