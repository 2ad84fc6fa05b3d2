"""Reverse-time GRU kernel and the opt-in ``train_agent_body`` learner, host side: exported symbols, the ctypes mirror
against the header's layout, the header's backward formulas against float64 autograd, and the CPU learner."""
import copy
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from _harness import REPO
import gru_bwd_model as model
from test_nets_cpu import load, make_args, quiet, sd_from

from macjd_amd import _native, ops
from macjd_amd.core.mac import BasicMAC
from macjd_amd.core.qmix import QMixLearner


@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_library_exports_the_backward_symbols(built):
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    for sym in ("macjd_gru_sequence_backward_supported", "macjd_gru_sequence_backward"):
        assert sym in _native.EXPORTS and f"{sym}(" in hdr
        assert hasattr(built, sym), sym
    f = built.macjd_gru_sequence_backward_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32]
    assert f(64) == 1 and f(128) == 1 and f(96) == 0
    assert "macjd_gru_bwd.hip" in entry.HIP_SOURCES


def test_gru_bwd_io_struct_layout_matches_header():
    IO = _native.GruBwdIO
    fields = [n for n, *_ in IO._fields_]
    assert fields == ["B", "T", "J", "H", "gi", "gh", "h_all", "h0", "h0_sb", "w_hh", "dh_all", "dgi", "dgh", "dh0"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           'int main(){printf("%zu", sizeof(macjd_gru_bwd_io));\n'
           + "".join(f'printf(" %zu", offsetof(macjd_gru_bwd_io, {f}));\n' for f in fields)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO)
    for name, off in zip(fields, out[1:]):
        assert getattr(IO, name).offset == off, name


# The header's backward formulas (include/macjd_nets.h, macjd_gru_bwd_io) restated in float64 NumPy, here and nowhere else.
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward_f64(gi, w_hh, b_hh, h0=None):
    """(h_all [B,T,J,H], gh [B,T,J,3H]) of the recurrence in float64 NumPy."""
    gi = np.asarray(gi, np.float64)
    w, bb = np.asarray(w_hh, np.float64), np.asarray(b_hh, np.float64)
    B, T, J, H3 = gi.shape
    H = H3 // 3
    h = np.zeros((B, J, H)) if h0 is None else np.asarray(h0, np.float64).reshape(B, J, H)
    h_all, gh_all = np.empty((B, T, J, H)), np.empty((B, T, J, H3))
    for t in range(T):
        gh = h @ w.T + bb
        r = _sig(gi[:, t, :, :H] + gh[..., :H])
        z = _sig(gi[:, t, :, H:2 * H] + gh[..., H:2 * H])
        n = np.tanh(gi[:, t, :, 2 * H:] + r * gh[..., 2 * H:])
        h = (h - n) * z + n
        h_all[:, t], gh_all[:, t] = h, gh
    return h_all, gh_all


def contract_backward(gi, gh, h_all, w_hh, dh_all, h0=None):
    """The header's formulas, t = T-1 ... 0.  Returns dict(dgi, dgh, dh0, dW_hh, db_hh)."""
    gi, gh, h_all, dh_all = (np.asarray(a, np.float64) for a in (gi, gh, h_all, dh_all))
    w = np.asarray(w_hh, np.float64)
    B, T, J, H3 = gi.shape
    H = H3 // 3
    h_first = np.zeros((B, J, H)) if h0 is None else np.asarray(h0, np.float64).reshape(B, J, H)
    dgi, dgh = np.empty_like(gi), np.empty_like(gi)
    carry = np.zeros((B, J, H))
    dW, db = np.zeros_like(w), np.zeros(H3)
    for t in range(T - 1, -1, -1):
        g = dh_all[:, t] + carry
        h_prev = h_all[:, t - 1] if t > 0 else h_first
        gh_n = gh[:, t, :, 2 * H:]
        r = _sig(gi[:, t, :, :H] + gh[:, t, :, :H])
        z = _sig(gi[:, t, :, H:2 * H] + gh[:, t, :, H:2 * H])
        n = np.tanh(gi[:, t, :, 2 * H:] + r * gh_n)
        da_n = g * (1 - z) * (1 - n * n)
        da_z = g * (h_prev - n) * z * (1 - z)
        da_r = da_n * gh_n * r * (1 - r)
        dgi[:, t] = np.concatenate([da_r, da_z, da_n], axis=-1)
        dgh[:, t] = np.concatenate([da_r, da_z, da_n * r], axis=-1)
        carry = g * z + dgh[:, t] @ w
        dW += dgh[:, t].reshape(-1, H3).T @ h_prev.reshape(-1, H)
        db += dgh[:, t].reshape(-1, H3).sum(0)
    return dict(dgi=dgi, dgh=dgh, dh0=carry, dW_hh=dW, db_hh=db)


@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_header_formulas_equal_float64_autograd(T, with_h0):
    """The contract before any kernel is trusted: the reverse-time formulas of the header == float64 autograd of a
    torch.nn.GRUCell stepping loop (and of the explicit stepping loop, which also yields dL/dgh)."""
    rng = np.random.default_rng(100 * T + with_h0)
    B, J, H = 2, 3, 8
    gi = rng.standard_normal((B, T, J, 3 * H))
    w, bb = rng.standard_normal((3 * H, H)) * 0.7, rng.standard_normal(3 * H) * 0.3
    h0 = rng.standard_normal((B, J, H)) if with_h0 else None
    dh = rng.standard_normal((B, T, J, H))
    h_all, gh = forward_f64(gi, w, bb, h0)
    got = contract_backward(gi, gh, h_all, w, dh, h0)
    cell = model.grucell_reference(gi, w, bb, dh, h0)
    loop = model.autograd_reference(gi, w, bb, dh, h0)
    np.testing.assert_allclose(loop["h_all"], h_all, rtol=1e-12, atol=1e-14)
    for ref, keys in ((cell, ("dgi", "dW_hh", "db_hh")), (loop, ("dgi", "dgh", "dW_hh", "db_hh"))):
        for k in keys:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-10, atol=1e-10 * np.abs(ref[k]).max(), err_msg=k)
    if with_h0:
        np.testing.assert_allclose(got["dh0"], cell["dh0"], rtol=1e-10, atol=1e-10 * np.abs(cell["dh0"]).max())
        np.testing.assert_allclose(got["dh0"], loop["dh0"], rtol=1e-10, atol=1e-10 * np.abs(loop["dh0"]).max())


def test_gru_sequence_train_on_host_is_the_differentiable_reference():
    rng = np.random.default_rng(3)
    B, T, J, H = 2, 4, 2, 8
    gi = torch.tensor(rng.standard_normal((B, T, J, 3 * H)), requires_grad=True)
    w = torch.tensor(rng.standard_normal((3 * H, H)) * 0.5, requires_grad=True)
    bb = torch.tensor(rng.standard_normal(3 * H) * 0.2, requires_grad=True)
    dh = rng.standard_normal((B, T, J, H))
    h = ops.gru_sequence_train(gi, w, bb)
    h.backward(torch.tensor(dh))
    ref = model.autograd_reference(gi.detach().numpy(), w.detach().numpy(), bb.detach().numpy(), dh)
    np.testing.assert_allclose(h.detach().numpy(), ref["h_all"], rtol=1e-12, atol=1e-14)
    for got, k in ((gi.grad, "dgi"), (w.grad, "dW_hh"), (bb.grad, "db_hh")):
        np.testing.assert_allclose(got.numpy(), ref[k], rtol=1e-10, atol=1e-12)


# --------------------------------------------------------------------------------------------- learner
TAG, B_, T_ = "2j2r_h128", 3, 5


def _learner(train_body, g, d):
    args = make_args(d, **({"train_agent_body": True} if train_body else {}))
    with quiet():
        mac = BasicMAC(d["S"], args)
        mac.load_state(sd_from(g, "g5_agent0."))
        learner = QMixLearner(mac, args)
    learner.eval_qmix_net.load_state_dict(sd_from(g, "g5_mixer0."))
    learner._update_targets()
    return mac, learner, args


def _named(mac, learner):
    named = {"agent." + n: p for n, p in mac.agent.named_parameters()}
    named.update({"mixer." + n: p for n, p in learner.eval_qmix_net.named_parameters()})
    return named


@pytest.fixture(scope="module")
def setting():
    """Weights of the 2j/2r fixture, a B = 3, T = 5 batch whose buffered hidden states are the eval agent's own unroll,
    and the independent float64 restatement of the loss with its gradients (computed once, read-only)."""
    g, d = load(TAG)
    batch = model.make_batch(np.random.default_rng(11), B_, T_, d["J"], d["S"], d["A"], d["H"])
    agent_sd, mixer_sd = sd_from(g, "g5_agent0."), sd_from(g, "g5_mixer0.")
    loss, leaves, extra = model.train_body_loss(agent_sd, agent_sd, mixer_sd, mixer_sd, batch, 0.99)
    loss.backward()
    batch["hidden_state"][:, :T_] = extra["h_eval"].numpy().astype(np.float32)
    ref = {k: (None if v.grad is None else v.grad.numpy()) for k, v in leaves.items()}
    return g, d, batch, float(loss.detach()), ref


def test_cpu_learner_trains_the_recurrent_body(setting):
    g, d, batch, ref_loss, ref = setting
    mac0, l0, _ = _learner(False, g, d)
    mac1, l1, _ = _learner(True, g, d)
    assert l1._body_is_shared() is False and l0._body_is_shared() is True
    out0 = l0._forward_backward(copy.deepcopy(batch), T_)
    out1 = l1._forward_backward(copy.deepcopy(batch), T_)
    n0, n1 = _named(mac0, l0), _named(mac1, l1)
    # the reference's loss is the special case: same loss / statistics, same Q-head and mixer gradients
    for a, b in zip(out0, out1):
        np.testing.assert_allclose(float(b), float(a), rtol=1e-5)
    np.testing.assert_allclose(float(out1[0]), ref_loss, rtol=1e-5)
    body = {k for k in n1 if k.startswith(("agent.fc1.", "agent.rnn."))}
    actor = {k for k in n1 if k.startswith("agent.actor.")}
    assert {k for k, p in n0.items() if p.grad is None} == body | actor          # default mode: unchanged None-grad set
    assert {k for k, p in n1.items() if p.grad is None} == actor
    for k in set(n1) - body - actor:
        np.testing.assert_allclose(n1[k].grad.numpy(), n0[k].grad.numpy(), rtol=1e-5,
                                   atol=1e-5 * float(n0[k].grad.abs().max()), err_msg=k)
    for k in sorted(set(n1) - actor):
        assert ref[k] is not None, k
        np.testing.assert_allclose(n1[k].grad.numpy(), ref[k], rtol=0, atol=1e-5 * float(np.abs(ref[k]).max()), err_msg=k)
    assert all(ref[k] is None for k in actor)
    # the trainable set: Q-head and mixer first (merged first layer leading), then fc1 and the GRU; never the actor
    tr0, tr1 = l0._trainable(), l1._trainable()
    assert [id(p) for p in tr1[:8]] == [id(p) for p in l1.eval_qmix_net.first_layer_params()]
    assert len(tr1) == len(tr0) + 6 and [p.shape for p in tr1[:len(tr0)]] == [p.shape for p in tr0]
    assert [id(p) for p in tr1[len(tr0):]] == [id(p) for p in list(mac1.agent.fc1.parameters()) + list(mac1.agent.rnn.parameters())]


def test_cpu_learner_two_updates_move_fc1_and_gru_only(setting):
    g, d, batch, _, _ = setting
    mac, learner, _ = _learner(True, g, d)
    before = {k: v.clone() for k, v in mac.agent.state_dict().items()}
    for _ in range(2):
        stats = learner.train(copy.deepcopy(batch), {})
        assert all(np.isfinite(v) for v in stats.values())
    after = mac.agent.state_dict()
    for k in before:
        if k.startswith("actor."):
            assert torch.equal(after[k], before[k]), k
        else:
            assert not torch.equal(after[k], before[k]), k
    assert learner._body_is_shared() is False
    assert all(p.grad is None for p in mac.agent.actor.parameters())


def test_default_mode_is_untouched(setting):
    g, d, batch, _, _ = setting
    mac, learner, args = _learner(False, g, d)
    assert learner.train_agent_body is False and not hasattr(args, "train_agent_body")
    learner.train(copy.deepcopy(batch), {})
    named = _named(mac, learner)
    assert {k for k, p in named.items() if p.grad is None} == {k for k in named if k.startswith(("agent.fc1.", "agent.rnn.", "agent.actor."))}


def test_main_has_the_flag():
    import inspect
    from macjd_amd import main as main_mod
    assert "--train-agent-body" in inspect.getsource(main_mod.main)
    cfg = open(os.path.join(os.path.dirname(main_mod.__file__), "config", "default.yaml")).read()
    assert "train_agent_body" not in cfg
