"""Actor-gradient kernel and the opt-in ``train_actor`` learner, host side: the float64 model against float64 autograd,
the exclusion cap of the case table, the stock-torch reference path, exported symbols and struct layout, the CPU learner."""
import copy
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as entry
from _harness import REPO
import actor_grad_model as model
import gru_bwd_model
from test_nets_cpu import TAGS, load, make_args, quiet, sd_from

from macjd_amd import _native, ops
from macjd_amd.core.mac import BasicMAC
from macjd_amd.core.networks import RNNAgent
from macjd_amd.core.qmix import QMixLearner

CASES = model.case_table()
ACTOR_KEYS = ["actor.0.weight", "actor.0.bias", "actor.2.weight", "actor.2.bias", "actor.4.weight", "actor.4.bias"]
MODEL_GRADS = ["dW1a", "db1a", "dW2a", "db2a", "dW3a", "db3a"]


def _bar(got, ref, msg):
    """The project's bar for float32 gradients under another summation order."""
    ref = np.asarray(ref)
    np.testing.assert_allclose(np.asarray(got), ref, rtol=1e-3, atol=2e-5 * float(np.abs(ref).max()), err_msg=msg)


# --------------------------------------------------------------------------------------------- the model itself
@pytest.mark.parametrize("tag", TAGS)
def test_model_equals_float64_autograd_on_the_fixture_weights(tag):
    """L_actor written with the agent's own modules (actor Sequential; one-hot / cat / fc2_q_head per action, the
    formulation of RNNAgent.get_q_value_for_action) and differentiated by stock float64 autograd."""
    g, d = load(tag)
    agent = RNNAgent(d["S"], make_args(d)).double()
    agent.load_state_dict({k: v.double() for k, v in sd_from(g, "agent.").items()})
    S, H, A, N = d["S"], d["H"], d["A"], 21
    assert (S, agent.actor_hidden_dim, H, A) in model.GEOMETRIES
    rng = np.random.default_rng(S)
    x = torch.tensor(rng.standard_normal((N, S)))
    h = torch.tensor(np.tanh(rng.standard_normal((N, H))))
    m = torch.tensor(rng.random(N) / N)
    m[3:6] = 0.0
    P = agent.actor(x)
    q = []
    for a in range(A):
        onehot = F.one_hot(torch.full((N,), a), A).double()
        q.append(agent.fc2_q_head(torch.cat([h, onehot, P[:, a:a + 1]], dim=1)).squeeze(1))
    Q = torch.stack(q, dim=1)
    (-(m * Q.sum(1)).sum()).backward()
    sd = {k: v.detach().numpy() for k, v in agent.state_dict().items()}
    W1q = sd["fc2_q_head.0.weight"]
    base = h.numpy() @ W1q[:, :H].T + sd["fc2_q_head.0.bias"]
    ref = model.actor_grad_model(x.numpy(), base, m.numpy(), [(sd[ACTOR_KEYS[2 * i]], sd[ACTOR_KEYS[2 * i + 1]]) for i in range(3)],
                                 W1q, sd["fc2_q_head.2.weight"], sd["fc2_q_head.2.bias"])
    np.testing.assert_allclose(ref["P"], P.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref["Q"], Q.detach().numpy(), rtol=1e-11, atol=1e-13)
    named = dict(agent.named_parameters())
    for key, mk in zip(ACTOR_KEYS, MODEL_GRADS):
        got = named[key].grad.numpy()
        np.testing.assert_allclose(ref[mk], got, rtol=1e-9, atol=1e-11 * max(1.0, float(np.abs(got).max())), err_msg=key)
    assert not ref["g3"][3:6].any() and not ref["g1"][3:6].any()


@pytest.fixture(scope="module")
def table():
    """(inputs, model outputs) of every table entry, computed once, read-only."""
    return [model.run_model(c) for c in CASES]


def test_case_table_covers_the_issue_and_respects_the_exclusion_cap(table):
    geoms = {c["geom"] for c in CASES}
    assert geoms == set(model.GEOMETRIES)
    for geom in model.GEOMETRIES:
        ns = {c["N"] for c in CASES if c["geom"] == geom}
        assert {1, 15, 16, 17, 65, 257, 4096} <= ns
        assert {c["scale"] for c in CASES if c["geom"] == geom} == {1, 3}
    assert any(c.get("x_pad") and c.get("base_pad") for c in CASES) and any("zero" in c for c in CASES)
    for case, (inp, ref) in zip(CASES, table):
        n_ex, N = int(ref["excluded"].sum()), case["N"]
        assert n_ex <= 0.02 * N, (model.case_id(case), n_ex)
        if N < 100:
            assert n_ex == 0, (model.case_id(case), n_ex)
        if case.get("x_pad"):
            assert inp["x"].strides[0] > 4 * inp["x"].shape[1] and inp["base"].strides[0] > 4 * inp["base"].shape[1]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ops_inputs(inp, dev="cpu", m=None):
    """Torch views of a case's inputs with the case's row strides kept."""
    def strided(a):   # a [N, w] view of a wider array -> the same view of a tensor
        if a.strides[0] == a.itemsize * a.shape[1]:
            return _t(a).to(dev)
        full = np.lib.stride_tricks.as_strided(a, shape=(a.shape[0], a.strides[0] // a.itemsize), strides=a.strides)
        return _t(full).to(dev)[:, :a.shape[1]]
    layers = [(_t(w).to(dev), _t(b).to(dev)) for w, b in inp["actor"]]
    return (strided(inp["x"]), strided(inp["base"]), _t(inp["m"] if m is None else m).to(dev), layers, _t(inp["W1q"]).to(dev),
            _t(inp["w2q"]).to(dev), _t(inp["b2q"]).to(dev))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[model.case_id(c) for c in CASES])
def test_reference_path_and_weight_grads_on_host_tensors(table, i):
    inp, ref = table[i]
    S, Ha, H, A = inp["geom"]
    args = _ops_inputs(inp)
    assert not ops.actor_gradient_supported(args[0], S, Ha, H, A)          # host tensors: the reference path
    a1, a2, g3, g2, g1, qsum = [t.numpy() for t in ops.actor_gradient(*args, H, A)]
    keep = ~ref["excluded"]
    for name, got in (("a1", a1), ("a2", a2), ("qsum", qsum)):
        _bar(got, ref[name], name)
    for name, got in (("g3", g3), ("g2", g2), ("g1", g1)):
        _bar(got[keep], ref[name][keep], name)
    lo, hi = inp["zero"]
    assert not g3[lo:hi].any() and not g2[lo:hi].any() and not g1[lo:hi].any()
    # weight gradients: sums over rows, so the excluded rows are given zero weight on both sides
    m_eff = np.where(keep, inp["m"], np.float32(0))
    ref_w = model.actor_grad_model(inp["x"], inp["base"], m_eff, inp["actor"], inp["W1q"], inp["w2q"], inp["b2q"])
    args = _ops_inputs(inp, m=m_eff)
    out = ops.actor_gradient(*args, H, A)
    grads = ops.actor_weight_grads(args[0], *out[:5])
    assert len(grads) == 6
    for mk, got in zip(MODEL_GRADS, grads):
        _bar(got.numpy(), ref_w[mk], mk)


# --------------------------------------------------------------------------------------------- library surface
@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_library_exports_the_actor_gradient_symbols(built):
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    for sym in ("macjd_actor_gradient_supported", "macjd_actor_gradient"):
        assert sym in _native.EXPORTS and f"{sym}(" in hdr
        assert hasattr(built, sym), sym
    f = built.macjd_actor_gradient_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    for geom in model.GEOMETRIES + [(184, 128, 128, 33)]:
        assert f(*geom) == 1, geom
    assert f(46, 128, 96, 9) == 0 and f(46, 128, 64, 34) == 0 and f(46, 129, 64, 9) == 0 and f(46, 80, 64, 9) == 0
    assert f(257, 128, 64, 9) == 0 and f(256, 128, 64, 9) == 0       # as macjd_mlp_forward: the LDS budget at S = 256
    assert f(0, 128, 64, 9) == 0 and f(46, 128, 64, 0) == 0
    assert "macjd_actor_grad.hip" in entry.HIP_SOURCES


def test_actor_grad_io_struct_layout_matches_header():
    IO = _native.ActorGradIO
    fields = [n for n, *_ in IO._fields_]
    assert fields == ["n_rows", "S", "Ha", "H", "A", "x", "x_ld", "base", "base_ld", "m", "W1a", "b1a", "W2a", "b2a", "W3a",
                      "b3a", "W1q", "w1_ld", "w2q", "b2q", "a1", "a2", "g3", "g2", "g1", "qsum"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           'int main(){printf("%zu", sizeof(macjd_actor_grad_io));\n'
           + "".join(f'printf(" %zu", offsetof(macjd_actor_grad_io, {f}));\n' for f in fields)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO)
    for name, off in zip(fields, out[1:]):
        assert getattr(IO, name).offset == off, name


# --------------------------------------------------------------------------------------------- learner
TAG, B_, T_, COEF = "2j2r_h128", 3, 5, 0.7
STAT_KEYS = ["loss", "grad_norm", "eval_qtot_avg", "target_qtot_avg"]


def learner_for(g, d, device="cpu", **opts):
    kw = dict(device="cuda", use_cuda=True) if device == "cuda" else {}
    args = make_args(d, **kw, **opts)
    with quiet():
        mac = BasicMAC(d["S"], args)
        mac.load_state(sd_from(g, "g5_agent0."))
        learner = QMixLearner(mac, args)
    learner.eval_qmix_net.load_state_dict(sd_from(g, "g5_mixer0."))
    learner._update_targets()
    return mac, learner, args


def named_params(mac, learner):
    named = {"agent." + n: p for n, p in mac.agent.named_parameters()}
    named.update({"mixer." + n: p for n, p in learner.eval_qmix_net.named_parameters()})
    return named


def combined_reference(g, d, batch, coef, dtype=torch.float64):
    """Stock autograd of TD loss + L_actor (the TD loss as restated in gru_bwd_model.train_body_loss, whose unrolled hidden
    states are what the batch buffers).  Returns (loss, actor_q_avg, {name: grad or None}, extras incl. the model's
    exclusion mask of the actor rows)."""
    T = int(batch["max_seq_len"])
    agent_sd, mixer_sd = sd_from(g, "g5_agent0."), sd_from(g, "g5_mixer0.")
    loss, leaves, extra = gru_bwd_model.train_body_loss(agent_sd, agent_sd, mixer_sd, mixer_sd, batch, 0.99, dtype=dtype)
    J, S, H, A = d["J"], d["S"], d["H"], d["A"]
    B = batch["obs"].shape[0]
    n = B * (T - 1) * J
    filled = torch.as_tensor(batch["filled"]).to(dtype)[:, :T - 1].reshape(B, T - 1)
    w = (filled / (J * filled.sum())).unsqueeze(2).expand(B, T - 1, J).reshape(n)
    x = torch.as_tensor(batch["obs"]).to(dtype)[:, :T - 1].reshape(n, S)
    h = extra["h_eval"][:, :T - 1].reshape(n, H)
    ag = lambda k: leaves["agent." + k]
    a1 = F.relu(F.linear(x, ag("actor.0.weight"), ag("actor.0.bias")))
    a2 = F.relu(F.linear(a1, ag("actor.2.weight"), ag("actor.2.bias")))
    P = torch.sigmoid(F.linear(a2, ag("actor.4.weight"), ag("actor.4.bias")))
    W1, b1, W2, b2 = (ag(k).detach() for k in ("fc2_q_head.0.weight", "fc2_q_head.0.bias", "fc2_q_head.2.weight", "fc2_q_head.2.bias"))
    qs = 0
    for a in range(A):
        inp = torch.cat([h, F.one_hot(torch.full((n,), a), A).to(dtype), P[:, a:a + 1]], dim=1)
        qs = qs + F.linear(F.relu(F.linear(inp, W1, b1)), W2, b2).squeeze(1)
    actor_q = (w * qs).sum()
    (loss - coef * actor_q).backward()
    base = h.double().numpy() @ W1.double().numpy()[:, :H].T + b1.double().numpy()
    mdl = model.actor_grad_model(x.numpy(), base, w.numpy(), [(ag(ACTOR_KEYS[2 * i]).detach().numpy(), ag(ACTOR_KEYS[2 * i + 1]).detach().numpy())
                                                              for i in range(3)], W1.numpy(), W2.numpy(), b2.numpy())
    grads = {k: (None if v.grad is None else v.grad.numpy()) for k, v in leaves.items()}
    return float(loss.detach()), float(actor_q.detach()), grads, dict(extra, excluded=mdl["excluded"])


def make_learner_batch(g, d, B, T, seed):
    """A batch with one short episode (its last steps not filled) whose buffered hidden states are the eval agent's unroll."""
    batch = gru_bwd_model.make_batch(np.random.default_rng(seed), B, T, d["J"], d["S"], d["A"], d["H"])
    batch["filled"][0, T - 2:] = False
    sd, mx = sd_from(g, "g5_agent0."), sd_from(g, "g5_mixer0.")
    _, _, extra = gru_bwd_model.train_body_loss(sd, sd, mx, mx, batch, 0.99)
    batch["hidden_state"][:, :T] = extra["h_eval"].numpy().astype(np.float32)
    return batch


@pytest.fixture(scope="module")
def setting():
    g, d = load(TAG)
    batch = make_learner_batch(g, d, B_, T_, seed=11)
    loss, actor_q, grads, extra = combined_reference(g, d, batch, COEF)
    assert not extra["excluded"].any()      # no ReLU tie among the actor rows: every row is compared
    return g, d, batch, loss, actor_q, grads


def _check_grads(named, ref, none_prefixes):
    none = {k for k in named if k.startswith(none_prefixes)} if none_prefixes else set()
    assert {k for k, p in named.items() if p.grad is None} == none
    for k in sorted(set(named) - none):
        assert ref[k] is not None, k
        _bar(named[k].grad.detach().cpu().numpy(), ref[k], k)


def test_cpu_learner_actor_gradients_equal_float64_autograd(setting):
    g, d, batch, ref_loss, ref_q, ref = setting
    mac, learner, _ = learner_for(g, d, train_actor=True, actor_loss_coef=COEF)
    assert learner._body_is_shared() is False
    out = learner._forward_backward(copy.deepcopy(batch), T_)
    np.testing.assert_allclose(float(out[0]), ref_loss, rtol=1e-5)
    np.testing.assert_allclose(float(learner._last_actor_q), ref_q, rtol=1e-5)
    _check_grads(named_params(mac, learner), ref, ("agent.fc1.", "agent.rnn."))
    # the trainable set: the default one, then the six actor tensors at the very end; self.params keeps its order
    _, l0, _ = learner_for(g, d)
    tr0, tr1 = l0._trainable(), learner._trainable()
    assert [p.shape for p in tr1[:len(tr0)]] == [p.shape for p in tr0]
    assert [id(p) for p in tr1[len(tr0):]] == [id(p) for p in mac.agent.actor.parameters()]
    assert [p.shape for p in learner.params] == [p.shape for p in l0.params]


def test_cpu_learner_with_body_and_actor_equals_float64_autograd(setting):
    g, d, batch, ref_loss, ref_q, ref = setting
    mac, learner, _ = learner_for(g, d, train_actor=True, actor_loss_coef=COEF, train_agent_body=True)
    learner._forward_backward(copy.deepcopy(batch), T_)
    _check_grads(named_params(mac, learner), ref, None)
    tr = learner._trainable()
    body = list(mac.agent.fc1.parameters()) + list(mac.agent.rnn.parameters())
    assert [id(p) for p in tr[-6:]] == [id(p) for p in mac.agent.actor.parameters()]
    assert [id(p) for p in tr[-6 - len(body):-6]] == [id(p) for p in body]


def test_cpu_learner_step_statistics_and_optimizer_state(setting):
    g, d, batch, _, ref_q, ref = setting
    mac0, l0, _ = learner_for(g, d)
    mac1, l1, _ = learner_for(g, d, train_actor=True, actor_loss_coef=COEF)
    before = {k: v.clone() for k, v in mac1.agent.state_dict().items()}
    s0, s1 = l0.train(copy.deepcopy(batch), {}), l1.train(copy.deepcopy(batch), {})
    assert list(s0) == STAT_KEYS and list(s1) == STAT_KEYS + ["actor_q_avg"]
    for k in ("loss", "eval_qtot_avg", "target_qtot_avg"):
        assert s1[k] == s0[k], k                                   # the TD side does not see the option
    # ONE clipped vector: the gradient norm gains exactly the actor's part
    actor_sq = sum(float((ref["agent." + k] ** 2).sum()) for k in ACTOR_KEYS)
    np.testing.assert_allclose(s1["grad_norm"] ** 2, s0["grad_norm"] ** 2 + actor_sq, rtol=1e-4)
    np.testing.assert_allclose(s1["actor_q_avg"], ref_q, rtol=1e-5)
    after = mac1.agent.state_dict()
    for k in before:
        moved = not torch.equal(after[k], before[k])
        assert moved == k.startswith(("actor.", "fc2_q_head.")), k
    # default mode: the actor has no gradient and keeps its bits
    assert all(p.grad is None for p in mac0.agent.actor.parameters())
    for k, v in mac0.agent.state_dict().items():
        if k.startswith("actor."):
            assert torch.equal(v, before[k]), k
    # optimizer.pth round trip: a fresh learner that loads the state continues bit for bit
    mac2, l2, _ = learner_for(g, d, train_actor=True, actor_loss_coef=COEF)
    mac2.load_state(copy.deepcopy(mac1.agent.state_dict()))
    l2.eval_qmix_net.load_state_dict(copy.deepcopy(l1.eval_qmix_net.state_dict()))
    l2.target_mac.load_state(copy.deepcopy(l1.target_mac.agent.state_dict()))
    l2.target_qmix_net.load_state_dict(copy.deepcopy(l1.target_qmix_net.state_dict()))
    l2.load_optimizer_state(copy.deepcopy(l1.optimizer.state_dict()))
    l2.train_step, l2.last_target_update_step = l1.train_step, l1.last_target_update_step
    sd1 = l1.optimizer.state_dict()
    assert len(sd1["state"]) == len(l1._trainable())               # Q-head, mixer and the six actor tensors have moments
    a, b = l1.train(copy.deepcopy(batch), {}), l2.train(copy.deepcopy(batch), {})
    assert a == b
    for (k, v), (_, w) in zip(mac1.agent.state_dict().items(), mac2.agent.state_dict().items()):
        assert torch.equal(v, w), k


def test_empty_mask_and_empty_loss_give_zero_actor_gradients(setting):
    g, d, batch, *_ = setting
    mac, learner, _ = learner_for(g, d, train_actor=True)
    dead = copy.deepcopy(batch)
    dead["filled"][:] = False
    obs = torch.as_tensor(dead["obs"])[:, :T_]
    hid = torch.as_tensor(dead["hidden_state"])
    q = learner._actor_backward(obs, hid, torch.as_tensor(dead["filled"])[:, :T_], T_)
    assert float(q) == 0.0 and all(p.grad is not None and not p.grad.any() for p in mac.agent.actor.parameters())
    for p in mac.agent.actor.parameters():
        p.grad = None
    q = learner._actor_backward(obs[:, :1], hid, torch.as_tensor(batch["filled"])[:, :1], 1)
    assert float(q) == 0.0 and all(p.grad is not None and not p.grad.any() for p in mac.agent.actor.parameters())


def test_main_has_the_flags_and_the_config_does_not():
    from macjd_amd import main as main_mod
    import macjd_amd.main as mm
    cfg = open(os.path.join(os.path.dirname(main_mod.__file__), "config", "default.yaml")).read()
    assert "train_actor" not in cfg and "actor_loss_coef" not in cfg
    seen = {}
    orig = mm.run
    mm.run = lambda a: seen.update(t=getattr(a, "train_actor", False), c=getattr(a, "actor_loss_coef", None),
                                   b=getattr(a, "train_agent_body", False))
    try:
        cdir = os.path.join(os.path.dirname(main_mod.__file__), "config")
        with quiet():
            mm.main(["--config-dir", cdir, "--train-actor", "--actor-loss-coef", "0.25"])
        assert seen == dict(t=True, c=0.25, b=False)
        with quiet():
            mm.main(["--config-dir", cdir])
        assert seen == dict(t=False, c=None, b=False)
    finally:
        mm.run = orig
