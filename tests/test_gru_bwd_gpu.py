"""Reverse-time GRU kernel, ``ops.gru_sequence_train`` and the ``train_agent_body`` learner on the device.

Kernel bound.  Metric per output: max|got - ref| / max|ref| against float64 autograd.  Worst value measured over the
whole case table on an MI355X: MEASURED_WORST below (and DESIGN.md 4.3).  The assertion is the smaller of 4 x that
(rounded up to one digit) and the project's bar for float32 gradients under another summation order (rtol 1e-3 with
atol 2e-5 max|ref|) — as a pure max-norm bound that bar is its atol term, 2e-5: an output within
2e-5 max|ref| everywhere meets the bar whatever the rtol term adds."""
import contextlib
import copy
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch
import yaml

from _harness import REPO
import gru_bwd_model as model
from test_nets_cpu import load, make_args, quiet, sd_from

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
MEASURED_WORST = 1.274e-6    # MI355X, whole table below: dgi 1.19e-6, dgh 1.18e-6, dh0 1.27e-6 (T = 7, W_hh x 6, one sequence)
KERNEL_BOUND = min(6e-6, 2e-5)   # 4 x measured = 5.1e-6, one digit up; capped by the existing bar
PAD = 64                                           # NaN margin (floats) on each side of every output


def _case(rng, B, T, J, H, scale, with_h0, dh_mode="dense"):
    gi = rng.standard_normal((B, T, J, 3 * H)).astype(np.float32)
    w = (rng.standard_normal((3 * H, H)) * (scale / np.sqrt(H))).astype(np.float32)
    bb = (rng.standard_normal(3 * H) * 0.1).astype(np.float32)
    h0 = (rng.standard_normal((B, J, H)) * 0.5).astype(np.float32) if with_h0 else None
    dh = rng.standard_normal((B, T, J, H)).astype(np.float32)
    if dh_mode == "last":
        dh[:, :T - 1] = 0
    elif dh_mode == "first":
        dh[:, 1:] = 0
    return gi, w, bb, h0, dh


def _launch(gi, gh, h_all, w, dh, h0=None, h0_strided=False):
    """The C entry point on caller-owned outputs with NaN margins; returns (dgi, dgh, dh0) and checks the margins."""
    from macjd_amd import _native
    lib = _native.load()
    B, T, J, H3 = gi.shape
    H = H3 // 3
    dev = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    t_gi, t_gh, t_h, t_w, t_dh = dev(gi), dev(gh), dev(h_all), dev(w), dev(dh)
    io_ = _native.GruBwdIO()
    io_.B, io_.T, io_.J, io_.H = B, T, J, H
    io_.gi, io_.gh, io_.h_all, io_.w_hh, io_.dh_all = (t.data_ptr() for t in (t_gi, t_gh, t_h, t_w, t_dh))
    keep = None
    if h0 is not None:
        if h0_strided:   # step 0 of a stored [B, 3, J, H] tensor: batch stride 3 J H, no copy
            keep = torch.full((B, 3, J, H), float("nan"), device=DEV)
            keep[:, 0] = dev(h0)
            io_.h0, io_.h0_sb = keep.data_ptr(), keep.stride(0)
        else:
            keep = dev(h0)
            io_.h0, io_.h0_sb = keep.data_ptr(), 0
    n3, n1 = B * T * J * H3, B * J * H
    bufs = [torch.full((n + 2 * PAD,), float("nan"), device=DEV) for n in (n3, n3, n1)]
    io_.dgi, io_.dgh = bufs[0][PAD:].data_ptr(), bufs[1][PAD:].data_ptr()
    io_.dh0 = bufs[2][PAD:].data_ptr() if h0 is not None else None
    _native.check(lib.macjd_gru_sequence_backward(ctypes.byref(io_), torch.cuda.current_stream().cuda_stream),
                  "macjd_gru_sequence_backward")
    torch.cuda.synchronize()
    out = []
    for b_, n in zip(bufs, (n3, n3, n1)):
        host = b_.cpu().numpy()
        assert np.isnan(host[:PAD]).all() and np.isnan(host[PAD + n:]).all(), "write outside the output"
        out.append(host[PAD:PAD + n])
    if h0 is None:
        assert np.isnan(out[2]).all()      # no dh0 requested: nothing written
    return out[0].reshape(gi.shape), out[1].reshape(gi.shape), (out[2].reshape(B, J, H) if h0 is not None else None)


def _check_kernel(rng, B, T, J, H, scale, with_h0, dh_mode="dense", h0_strided=False):
    gi, w, bb, h0, dh = _case(rng, B, T, J, H, scale, with_h0, dh_mode)
    ref = model.autograd_reference(gi, w, bb, dh, h0)
    dgi, dgh, dh0 = _launch(gi, ref["gh"], ref["h_all"], w, dh, h0, h0_strided)
    errs = {"dgi": model.rel_err(dgi, ref["dgi"]), "dgh": model.rel_err(dgh, ref["dgh"])}
    if with_h0:
        errs["dh0"] = model.rel_err(dh0, ref["dh0"])
    print(f"gru_bwd B={B} T={T} J={J} H={H} x{scale} h0={with_h0} dh={dh_mode}: "
          + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert np.isfinite(v) and v <= KERNEL_BOUND, (k, v)
    return max(errs.values())


SEQS = {1: (1, 1), 3: (1, 3), 17: (17, 1)}   # B*J sequences -> (B, J)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("nseq", [1, 3, 17])
def test_kernel_against_float64_autograd(nseq, T, H):
    B, J = SEQS[nseq]
    rng = np.random.default_rng(1000 * nseq + 10 * T + H)
    for scale in (1.0, 6.0):            # an unsaturated and a partly saturated GRU
        for with_h0 in (False, True):
            _check_kernel(rng, B, T, J, H, scale, with_h0)


@pytest.mark.parametrize("H", [64, 128])
def test_kernel_sparse_output_gradients_and_strided_h0(H):
    rng = np.random.default_rng(H)
    _check_kernel(rng, 2, 7, 3, H, 1.0, True, dh_mode="last")      # everything arrives through the carry
    _check_kernel(rng, 2, 7, 3, H, 6.0, True, dh_mode="first")     # steps t > 0 see a zero gradient: exact zeros
    _check_kernel(rng, 3, 4, 2, H, 1.0, True, h0_strided=True)


def test_kernel_argument_errors():
    from macjd_amd import _native
    lib = _native.load()
    t = torch.zeros(3 * 96 * 96, device=DEV)
    io_ = _native.GruBwdIO()
    io_.B, io_.T, io_.J, io_.H = 1, 1, 1, 64
    assert lib.macjd_gru_sequence_backward(ctypes.byref(io_), None) == -1          # NULL pointers: MACJD_EINVAL
    io_.gi = io_.gh = io_.h_all = io_.w_hh = io_.dh_all = io_.dgi = io_.dgh = t.data_ptr()
    for field in ("B", "T", "J"):
        setattr(io_, field, 0)
        assert lib.macjd_gru_sequence_backward(ctypes.byref(io_), None) == -1
        setattr(io_, field, 1)
    io_.H = 96
    assert lib.macjd_gru_sequence_backward(ctypes.byref(io_), None) == -4          # MACJD_EUNSUPPORTED
    assert lib.macjd_gru_sequence_backward(None, None) == -1


# --------------------------------------------------------------------------------------------- ops
def _ops_case(B, T, J, H, with_h0, seed):
    from macjd_amd import ops
    rng = np.random.default_rng(seed)
    gi, w, bb, h0, dh = _case(rng, B, T, J, H, 1.0, with_h0)
    ref = model.autograd_reference(gi, w, bb, dh, h0)
    leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
    t_gi, t_w, t_b = leaf(gi), leaf(w), leaf(bb)
    t_h0 = leaf(h0) if with_h0 else None
    h = ops.gru_sequence_train(t_gi, t_w, t_b, t_h0)
    with torch.no_grad():
        plain = ops.gru_sequence(t_gi, t_w, t_b, t_h0)
    assert torch.equal(h.detach(), plain)                       # the forward IS the scan launch
    h.backward(torch.tensor(dh, device=DEV))
    got = {"dgi": t_gi.grad, "dW_hh": t_w.grad, "db_hh": t_b.grad}
    if with_h0:
        got["dh0"] = t_h0.grad
    return {k: v.cpu().numpy() for k, v in got.items()}, ref


@pytest.mark.parametrize("shape", [(2, 7, 3, 64), (2, 4, 2, 128)])
@pytest.mark.parametrize("with_h0", [False, True])
def test_gru_sequence_train_gradients(shape, with_h0):
    got, ref = _ops_case(*shape, with_h0, seed=sum(shape))
    for k, v in got.items():
        e = model.rel_err(v, ref[k])
        print(f"gru_sequence_train {shape} h0={with_h0} {k}: {e:.3e}")
        assert e <= KERNEL_BOUND, (k, e)


@pytest.mark.parametrize("H", [64, 128])
def test_gru_sequence_train_split_k_weight_gradient(H):
    """>= 1024 rows: dW_hh / db_hh come from the split-K weight-gradient kernel (the learner's case; M = 3H, N = H).
    T = 22 steps of error growth are outside the kernel table, so this holds the project's bar for float32 gradients
    itself."""
    got, ref = _ops_case(16, 22, 3, H, False, seed=5 + H)
    for k, v in got.items():
        print(f"gru_sequence_train split-K H={H} {k}: {model.rel_err(v, ref[k]):.3e}")
        np.testing.assert_allclose(v, ref[k], rtol=1e-3, atol=2e-5 * float(np.abs(ref[k]).max()), err_msg=k)


@pytest.mark.parametrize("H", [64, 128])
def test_gru_sequence_train_non_dense_inputs(H):
    """The kernel reads dense tensors; the op must make them so.  gi is an expand over time of one [B,1,J,3H] row (stride 0
    in T: the static-observation form), h0 comes as [B*J, H] (the controllers' hidden_states layout) and requires grad, and
    the consumer permutes h before copying it, so dL/dh arrives as a transposed view (unit last stride, not dense)."""
    from macjd_amd import ops
    B, T, J = 3, 5, 2
    rng = np.random.default_rng(700 + H)
    gi, w, bb, h0, _ = _case(rng, B, T, J, H, 1.0, True)
    gi[:] = gi[:, :1]                                            # the same input transform at every step
    dh_perm = rng.standard_normal((B, J, T, H)).astype(np.float32)    # gradient of h.transpose(1, 2).contiguous()
    ref = model.autograd_reference(gi, w, bb, dh_perm.transpose(0, 2, 1, 3), h0)
    leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
    g1, t_w, t_b, t_h0 = leaf(gi[:, :1].copy()), leaf(w), leaf(bb), leaf(h0.reshape(B * J, H))
    gi_exp = g1.expand(B, T, J, 3 * H)
    assert gi_exp.stride(1) == 0 and gi_exp.stride(-1) == 1
    h = ops.gru_sequence_train(gi_exp, t_w, t_b, t_h0)
    with torch.no_grad():
        assert torch.equal(h.detach(), ops.gru_sequence(gi_exp, t_w, t_b, t_h0))
    h.transpose(1, 2).contiguous().backward(torch.tensor(dh_perm, device=DEV))
    assert tuple(t_h0.grad.shape) == (B * J, H)
    got = {"dgi": g1.grad.cpu().numpy(), "dW_hh": t_w.grad.cpu().numpy(), "db_hh": t_b.grad.cpu().numpy(),
           "dh0": t_h0.grad.cpu().numpy().reshape(B, J, H)}
    want = dict(ref, dgi=ref["dgi"].sum(axis=1, keepdims=True))      # the expand's backward sums over time
    for k, v in got.items():
        e = model.rel_err(v, want[k])
        print(f"gru_sequence_train non-dense H={H} {k}: {e:.3e}")
        assert e <= KERNEL_BOUND, (k, e)


def test_gru_sequence_train_other_sizes_use_stock_autograd():
    from macjd_amd import ops
    rng = np.random.default_rng(0)
    gi, w, bb, _, dh = _case(rng, 2, 3, 2, 32, 1.0, False)      # H = 32: no kernel, gru_sequence_reference
    leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
    t_gi, t_w, t_b = leaf(gi), leaf(w), leaf(bb)
    ops.gru_sequence_train(t_gi, t_w, t_b).backward(torch.tensor(dh, device=DEV))
    ref = model.autograd_reference(gi, w, bb, dh)
    np.testing.assert_allclose(t_gi.grad.cpu().numpy(), ref["dgi"], rtol=1e-3, atol=2e-5 * np.abs(ref["dgi"]).max())


# --------------------------------------------------------------------------------------------- learner
LEARNER_CASES = {"3j4r_h64": (4, 6, 3), "2j2r_h128": (3, 4, 3)}   # tag -> (B, T, batch seed)


def _learner(g, d, device, train_body=True):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    kw = dict(device="cuda", use_cuda=True) if device == "cuda" else {}
    if train_body:
        kw["train_agent_body"] = True
    args = make_args(d, **kw)
    with quiet():
        mac = BasicMAC(d["S"], args)
        mac.load_state(sd_from(g, "g5_agent0."))
        learner = QMixLearner(mac, args)
    learner.eval_qmix_net.load_state_dict(sd_from(g, "g5_mixer0."))
    learner._update_targets()
    return mac, learner


def _named(mac, learner):
    named = {"agent." + n: p for n, p in mac.agent.named_parameters()}
    named.update({"mixer." + n: p for n, p in learner.eval_qmix_net.named_parameters()})
    return named


@pytest.fixture(scope="module", params=sorted(LEARNER_CASES))
def cpu_side(request):
    """The CPU float32 learner's update on the case's batch, computed once: statistics, gradients, parameters after one
    train(); plus the ReLU-margin condition, evaluated on the CPU model alone."""
    tag = request.param
    B, T, seed = LEARNER_CASES[tag]
    g, d = load(tag)
    batch = model.make_batch(np.random.default_rng(seed), B, T, d["J"], d["S"], d["A"], d["H"])
    agent_sd, mixer_sd = sd_from(g, "g5_agent0."), sd_from(g, "g5_mixer0.")
    _, _, extra = model.train_body_loss(agent_sd, agent_sd, mixer_sd, mixer_sd, batch, 0.99, dtype=torch.float32)
    batch["hidden_state"][:, :T] = extra["h_eval"].numpy()
    # no fc1 / Q-head pre-activation so close to zero that a ReLU side could decide the comparison
    for k in ("fc1_pre", "q_pre"):
        x = extra[k].abs()
        assert float(x.min()) > 1e-5 * max(1.0, float(x.max())), (tag, k, float(x.min()))
    # ... and no near tie in the Double-DQN argmax over the all-action Q, so that a statistics mismatch is not an argmax flip
    gap, qmax = float(extra["argmax_gap"].min()), float(extra["q_eval_all"].abs().max())
    assert gap > 1e-5 * max(1.0, qmax), (tag, gap)
    mac, learner = _learner(g, d, "cpu")
    stats = learner.train(copy.deepcopy(batch), {})
    named = _named(mac, learner)
    grads = {k: (None if p.grad is None else p.grad.detach().numpy().copy()) for k, p in named.items()}
    params = {k: p.detach().numpy().copy() for k, p in named.items()}
    return tag, g, d, batch, stats, grads, params


def test_learner_on_device_matches_cpu_learner(cpu_side):
    tag, g, d, batch, ref_stats, ref_grads, ref_params = cpu_side
    mac, learner = _learner(g, d, "cuda")
    assert next(mac.agent.parameters()).is_cuda and learner._body_is_shared() is False
    stats = learner.train(copy.deepcopy(batch), {})
    keys = ("loss", "grad_norm", "eval_qtot_avg", "target_qtot_avg")
    np.testing.assert_allclose([stats[k] for k in keys], [ref_stats[k] for k in keys], rtol=1e-4)
    named = _named(mac, learner)
    assert {k for k, p in named.items() if p.grad is None} == {k for k in named if k.startswith("agent.actor.")}
    assert {k for k, v in ref_grads.items() if v is None} == {k for k in named if k.startswith("agent.actor.")}
    for k, p in named.items():
        if ref_grads[k] is not None:
            ref = ref_grads[k]
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * float(np.abs(ref).max()), err_msg=k)
    # after one train(): the flat parameter vector (Q-head, mixer, then fc1 / GRU) agrees with the CPU learner's
    tr = learner._trainable()
    by_id = {id(p): k for k, p in named.items()}
    assert {by_id[id(p)] for p in tr} == {k for k in named if not k.startswith("agent.actor.")}
    flat = learner._flat_param.cpu().numpy()
    for p, off in zip(tr, learner._flat_offsets):
        ref = ref_params[by_id[id(p)]].reshape(-1)
        np.testing.assert_allclose(flat[off:off + ref.size], ref, rtol=1e-3, atol=1e-6, err_msg=by_id[id(p)])
        assert p.data_ptr() == learner._flat_param.data_ptr() + 4 * off
    for k, p in named.items():
        if k.startswith("agent.actor."):
            np.testing.assert_array_equal(p.detach().cpu().numpy(), g["g5_agent0." + k[len("agent."):]])


def test_enable_graphs_refuses_and_default_mode_keeps_the_body_frozen(cpu_side):
    tag, g, d, batch, *_ = cpu_side
    mac, learner = _learner(g, d, "cuda")
    with pytest.raises(RuntimeError, match="train_agent_body"):
        learner.enable_graphs(None, 4)
    mac0, l0 = _learner(g, d, "cuda", train_body=False)
    l0.train(copy.deepcopy(batch), {})
    for n, p in mac0.agent.named_parameters():
        assert (p.grad is None) == (not n.startswith("fc2_q_head")), n
    assert l0._body_is_shared() is True


def test_static_observation_inputs_follow_the_trained_body(cpu_side):
    """The controller caches the body's outputs for a static observation, keyed on version counters that the fused
    optimiser step (writes through .data views) does not move: train() must drop that cache."""
    tag, g, d, batch, *_ = cpu_side
    mac, learner = _learner(g, d, "cuda")
    obs = torch.tensor(batch["obs"][:, 0], device=DEV)           # [B, J, S]
    mac.prepare_static_obs(obs)
    gi0 = mac.static_inputs[1].clone()
    learner.train(copy.deepcopy(batch), {})
    mac.prepare_static_obs(obs)
    gi1 = mac.static_inputs[1]
    assert not torch.equal(gi1, gi0)
    with torch.no_grad():
        a = mac.agent
        x = torch.relu(torch.nn.functional.linear(obs.reshape(-1, d["S"]), a.fc1.weight, a.fc1.bias))
        ref = torch.nn.functional.linear(x, a.rnn.weight_ih, a.rnn.bias_ih)
    np.testing.assert_allclose(gi1.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))


# --------------------------------------------------------------------------------------------- driver
def test_main_run_with_train_agent_body(tmp_path):
    from macjd_amd.main import build_components, load_config, main, run, save_checkpoint
    from macjd_amd.scenario import ring_scenario_dict
    import macjd_amd.main as main_mod
    sim = str(tmp_path / "scenario_2j2r.yaml")
    with open(sim, "w") as f:
        yaml.safe_dump(ring_scenario_dict(2, 2), f)

    def cfg(**kw):
        with contextlib.redirect_stdout(io.StringIO()):
            c = load_config("default", os.path.join(PKG, "config"))
        c.device_request, c.sim_config_path = "cuda", sim
        c.save_model_dir, c.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
        c.log_interval_seconds, c.gemm_tuning, c.resume = 0, False, None
        E = 8
        c.batch_envs, c.buffer_size, c.batch_size, c.start_training_steps = E, 2 * E, E, 0
        c.total_env_steps, c.save_interval, c.updates_per_rollout, c.lr = 3 * E * 100, 10 ** 9, 3, 1e-3
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    # the initial weights, as a checkpoint the run resumes from
    c0 = cfg(train_agent_body=True)
    with contextlib.redirect_stdout(io.StringIO()):
        main_mod._pick_device(c0, 0)
        torch.manual_seed(c0.seed)
        env, mac, buffer, learner, runner = build_components(c0, sim)[:5]
        start = str(tmp_path / "start")
        save_checkpoint(learner, runner, start, 0, 0)
    first = torch.load(os.path.join(start, "agent.pth"), weights_only=True)
    c1 = cfg(train_agent_body=True, resume=start)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = run(c1)
    assert res["total_steps"] == 3 * 8 * 100 and res["train_steps"] == 9 and "Training finished." in out.getvalue()
    rows = [json.loads(l) for l in open(os.path.join(res["log_dir"], "scalars.jsonl"))]
    losses = [r["value"] for r in rows if r["tag"].startswith("Loss/")]
    assert losses and all(np.isfinite(v) for v in losses)
    last = os.path.join(c1.save_model_dir, c1.test_name, f"step_{3 * 8 * 100}")
    final = torch.load(os.path.join(last, "agent.pth"), weights_only=True)
    assert not torch.equal(final["fc1.weight"], first["fc1.weight"])
    assert not torch.equal(final["rnn.weight_hh"], first["rnn.weight_hh"])
    for k in first:
        if k.startswith("actor."):
            assert torch.equal(final[k], first[k]), k
    # the command-line flag sets the argument
    seen = {}
    orig = main_mod.run
    main_mod.run = lambda a: seen.setdefault("v", getattr(a, "train_agent_body", False))
    try:
        main(["--config-dir", os.path.join(PKG, "config"), "--train-agent-body"])
        assert seen["v"] is True
        seen.clear()
        main(["--config-dir", os.path.join(PKG, "config")])
        assert seen["v"] is False
    finally:
        main_mod.run = orig
