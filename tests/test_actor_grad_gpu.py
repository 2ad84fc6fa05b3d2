"""Actor-gradient kernel, ``ops.actor_gradient`` / ``ops.actor_weight_grads`` and the ``train_actor`` learner on the device.

Kernel bound.  Metric per output: max|got - ref| / max|ref| against the float64 model (tests/actor_grad_model.py), over all
rows for a1 / a2 / qsum and over the rows the model does not exclude (ReLU near-ties, see there) for g1 / g2 / g3.  Worst
value measured over the whole case table on an MI355X: MEASURED_WORST below (and DESIGN.md 4.5).  The assertion is the
smaller of 4 x that (rounded up to one digit; the factor covers summation-order differences between launch geometries)
and 2e-5, the atol term of the project's bar for float32 gradients under another summation order — the rule of
tests/test_gru_bwd_gpu.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import actor_grad_model as model
from test_nets_cpu import load
from test_actor_grad_cpu import (ACTOR_KEYS, CASES, MODEL_GRADS, STAT_KEYS, _bar, _ops_inputs, combined_reference, learner_for,
                                 make_learner_batch, named_params)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED_WORST = 8.286e-7    # MI355X, whole table: g3 8.29e-7 (12j/16r, N = 4096, x3), g1 8.14e-7, a1 5.71e-7, g2 5.27e-7, a2 4.04e-7, qsum 2.28e-7
KERNEL_BOUND = min(4e-6, 2e-5)   # 4 x measured = 3.3e-6, one digit up; capped by the existing bar
PAD = 64                     # NaN margin (floats) on each side of every output
OUTS = ("a1", "a2", "g3", "g2", "g1", "qsum")


@pytest.fixture(scope="module")
def table():
    """(inputs, model outputs) of every table entry, computed once, read-only."""
    return [model.run_model(c) for c in CASES]


def _launch(inp, want_qsum=True):
    """The C entry point on caller-owned outputs with NaN margins; returns the six outputs (NumPy) and checks the margins."""
    from macjd_amd import _native
    lib = _native.load()
    S, Ha, H, A = inp["geom"]
    x, base, m, layers, W1q, w2q, b2q = _ops_inputs(inp, DEV)
    N = x.shape[0]
    io_ = _native.ActorGradIO()
    io_.n_rows, io_.S, io_.Ha, io_.H, io_.A = N, S, Ha, H, A
    io_.x, io_.x_ld, io_.base, io_.base_ld, io_.m = x.data_ptr(), x.stride(0), base.data_ptr(), base.stride(0), m.data_ptr()
    (io_.W1a, io_.b1a), (io_.W2a, io_.b2a), (io_.W3a, io_.b3a) = [(w.data_ptr(), b.data_ptr()) for w, b in layers]
    io_.W1q, io_.w1_ld, io_.w2q, io_.b2q = W1q.data_ptr(), W1q.stride(0), w2q.data_ptr(), b2q.data_ptr()
    sizes = dict(a1=N * Ha, a2=N * Ha, g3=N * A, g2=N * Ha, g1=N * Ha, qsum=N)
    bufs = {k: torch.full((n + 2 * PAD,), float("nan"), device=DEV) for k, n in sizes.items()}
    for k in OUTS:
        setattr(io_, k, bufs[k][PAD:].data_ptr() if (k != "qsum" or want_qsum) else None)
    _native.check(lib.macjd_actor_gradient(ctypes.byref(io_), torch.cuda.current_stream().cuda_stream), "macjd_actor_gradient")
    torch.cuda.synchronize()
    out = {}
    for k, n in sizes.items():
        host = bufs[k].cpu().numpy()
        assert np.isnan(host[:PAD]).all() and np.isnan(host[PAD + n:]).all(), f"write outside {k}"
        out[k] = host[PAD:PAD + n].reshape(N, -1) if k != "qsum" else host[PAD:PAD + n]
    return out


def _errors(got, ref):
    keep = ~ref["excluded"]
    errs = {k: model.rel_err(got[k], ref[k]) for k in ("a1", "a2", "qsum")}
    errs.update({k: model.rel_err(got[k][keep], ref[k][keep]) for k in ("g3", "g2", "g1")})
    return errs


@pytest.mark.parametrize("i", range(len(CASES)), ids=[model.case_id(c) for c in CASES])
def test_kernel_against_the_float64_model(table, i):
    inp, ref = table[i]
    got = _launch(inp)
    errs = _errors(got, ref)
    print(f"actor_grad {model.case_id(CASES[i])} excluded={int(ref['excluded'].sum())}: "
          + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert np.isfinite(v) and v <= KERNEL_BOUND, (k, v)
    for k in OUTS:
        assert np.isfinite(got[k]).all(), k          # every element written, excluded rows included


def test_zero_weight_rows_give_exact_zeros_and_qsum_is_optional(table):
    i = next(i for i, c in enumerate(CASES) if "zero" in c)
    inp, ref = table[i]
    lo, hi = inp["zero"]
    assert hi - lo > 64 and lo % 16 != 0                       # whole waves of zero rows and mixed ones
    got = _launch(inp, want_qsum=False)
    for k in ("g3", "g2", "g1"):
        assert not got[k][lo:hi].any(), k
        assert got[k][:lo].any() and got[k][hi:].any(), k
    assert np.isnan(got["qsum"]).all()                         # not requested: not written
    for k in ("a1", "a2"):                                      # ... and the activations are written all the same
        assert model.rel_err(got[k][lo:hi], ref[k][lo:hi]) <= KERNEL_BOUND


def test_kernel_argument_errors(table):
    from macjd_amd import _native
    lib = _native.load()
    assert lib.macjd_actor_gradient(None, None) == -1
    t = torch.zeros(256 * 256, device=DEV)
    ptrs = ("x", "base", "m", "W1a", "b1a", "W2a", "b2a", "W3a", "b3a", "W1q", "w2q", "a1", "a2", "g3", "g2", "g1")

    def io(**kw):
        io_ = _native.ActorGradIO()
        io_.n_rows, io_.S, io_.Ha, io_.H, io_.A = 4, 46, 128, 64, 9
        io_.x_ld, io_.base_ld, io_.w1_ld = 46, 64, 64 + 9 + 1
        for p in ptrs:
            setattr(io_, p, t.data_ptr())
        for k, v in kw.items():
            setattr(io_, k, v)
        return io_

    call = lambda io_: lib.macjd_actor_gradient(ctypes.byref(io_), None)
    for p in ptrs:                                              # NULL required pointers: MACJD_EINVAL
        assert call(io(**{p: None})) == -1, p
    for f in ("n_rows", "S", "Ha", "H", "A"):                   # non-positive sizes
        assert call(io(**{f: 0})) == -1, f
    assert call(io(x_ld=45)) == -1 and call(io(base_ld=63)) == -1 and call(io(w1_ld=73)) == -1
    assert call(io(H=96, base_ld=96, w1_ld=106)) == -4          # MACJD_EUNSUPPORTED, nothing launched
    assert call(io(A=34, w1_ld=99)) == -4
    torch.cuda.synchronize()
    assert not t.any()


# --------------------------------------------------------------------------------------------- ops
@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c["N"] in (17, 257, 4096)],
                         ids=[model.case_id(c) for c in CASES if c["N"] in (17, 257, 4096)])
def test_ops_actor_gradient_and_weight_grads_on_device(table, i):
    from macjd_amd import ops
    inp, ref = table[i]
    S, Ha, H, A = inp["geom"]
    # sums over rows: the rows the model excludes get zero weight on both sides (rows are independent)
    m_eff = np.where(ref["excluded"], np.float32(0), inp["m"])
    ref_w = model.actor_grad_model(inp["x"], inp["base"], m_eff, inp["actor"], inp["W1q"], inp["w2q"], inp["b2q"])
    args = _ops_inputs(inp, DEV, m=m_eff)
    assert ops.actor_gradient_supported(args[0], S, Ha, H, A)
    out = ops.actor_gradient(*args, H, A)
    errs = _errors({k: v.cpu().numpy() for k, v in zip(OUTS, out)}, dict(ref_w, excluded=ref["excluded"]))
    assert max(errs.values()) <= KERNEL_BOUND, errs
    grads = ops.actor_weight_grads(args[0], *out[:5])
    torch.cuda.synchronize()
    for mk, got in zip(MODEL_GRADS, grads):
        print(f"actor_weight_grads {model.case_id(CASES[i])} {mk}: {model.rel_err(got.cpu().numpy(), ref_w[mk]):.3e}")
        _bar(got.cpu().numpy(), ref_w[mk], mk)


def test_unsupported_shape_takes_the_reference_on_device():
    from macjd_amd import ops
    case = dict(geom=(20, 80, 64, 5), N=9, scale=1, seed=1)      # Ha = 80: five tiles, outside the kernel's range
    inp, ref = model.run_model(case)
    assert not ref["excluded"].any()
    args = _ops_inputs(inp, DEV)
    assert not ops.actor_gradient_supported(args[0], 20, 80, 64, 5)
    out = ops.actor_gradient(*args, 64, 5)
    for k, v in zip(OUTS, out):
        _bar(v.cpu().numpy(), ref[k], k)


# --------------------------------------------------------------------------------------------- learner
LEARNER_CASES = {"3j4r_h64": (4, 6, 3), "2j2r_h128": (3, 4, 3)}   # tag -> (B, T, batch seed)
COEF = 0.7


@pytest.fixture(scope="module", params=sorted(LEARNER_CASES))
def cpu_side(request):
    """Float64 autograd of the combined objective on the case's batch and the CPU learner's train(): computed once."""
    tag = request.param
    B, T, seed = LEARNER_CASES[tag]
    g, d = load(tag)
    batch = make_learner_batch(g, d, B, T, seed)
    loss, actor_q, grads, extra = combined_reference(g, d, batch, COEF)
    assert not extra["excluded"].any()                             # no ReLU tie among the actor rows
    for k in ("fc1_pre", "q_pre"):                                 # ... nor in the TD loss's path, nor an argmax near-tie
        v = extra[k].abs()
        assert float(v.min()) > 1e-5 * max(1.0, float(v.max())), (tag, k)
    assert float(extra["argmax_gap"].min()) > 1e-5 * max(1.0, float(extra["q_eval_all"].abs().max())), tag
    mac, learner, _ = learner_for(g, d, train_actor=True, actor_loss_coef=COEF)
    stats = learner.train(copy.deepcopy(batch), {})
    np.testing.assert_allclose(stats["actor_q_avg"], actor_q, rtol=1e-5)
    params = {k: p.detach().numpy().copy() for k, p in named_params(mac, learner).items()}
    return tag, g, d, batch, stats, grads, params


def test_learner_step_on_device_matches_the_cpu_side(cpu_side):
    tag, g, d, batch, ref_stats, ref_grads, ref_params = cpu_side
    mac, learner, _ = learner_for(g, d, "cuda", train_actor=True, actor_loss_coef=COEF)
    assert next(mac.agent.parameters()).is_cuda and learner._body_is_shared() is False
    stats = learner.train(copy.deepcopy(batch), {})
    keys = STAT_KEYS + ["actor_q_avg"]
    assert list(stats) == keys
    print(tag, {k: (stats[k], ref_stats[k]) for k in keys})
    np.testing.assert_allclose([stats[k] for k in keys], [ref_stats[k] for k in keys], rtol=1e-4, atol=1e-5)
    # the gradients before the clip scales them in place: a second learner's forward + backward alone
    mac_g, learner_g, _ = learner_for(g, d, "cuda", train_actor=True, actor_loss_coef=COEF)
    learner_g._forward_backward(copy.deepcopy(batch), int(batch["max_seq_len"]))
    named_g = named_params(mac_g, learner_g)
    body = {k for k in named_g if k.startswith(("agent.fc1.", "agent.rnn."))}
    assert {k for k, p in named_g.items() if p.grad is None} == body
    for k in sorted(set(named_g) - body):
        ref = ref_grads[k]
        np.testing.assert_allclose(named_g[k].grad.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=k)
    for k in ACTOR_KEYS:                                           # the actor's own, at the bar without the max(1, .) floor
        _bar(named_g["agent." + k].grad.cpu().numpy(), ref_grads["agent." + k], k)
    named = named_params(mac, learner)
    # the actor's gradients were written in place: they ARE the tail slices of the flat gradient vector
    tr = learner._trainable()
    assert [id(p) for p in tr[-6:]] == [id(p) for p in mac.agent.actor.parameters()]
    for p, off in zip(tr[-6:], learner._flat_offsets[-6:]):
        assert p.grad.data_ptr() == learner._flat_grad.data_ptr() + 4 * off
        assert p.data_ptr() == learner._flat_param.data_ptr() + 4 * off
    for k, p in named.items():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref_params[k], atol=5e-6, rtol=0, err_msg=k)


def test_actor_and_body_together_on_device(cpu_side):
    """Both options: every parameter of the eval agent and the mixer gets the float64 gradient of the combined objective."""
    tag, g, d, batch, _, ref_grads, _ = cpu_side
    mac, learner, _ = learner_for(g, d, "cuda", train_actor=True, actor_loss_coef=COEF, train_agent_body=True)
    learner._forward_backward(copy.deepcopy(batch), int(batch["max_seq_len"]))
    for k, p in named_params(mac, learner).items():
        assert p.grad is not None, k
        ref = ref_grads[k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=k)
    tr = learner._trainable()
    assert [id(p) for p in tr[-6:]] == [id(p) for p in mac.agent.actor.parameters()]
    stats = learner.train(copy.deepcopy(batch), {})
    assert all(np.isfinite(v) for v in stats.values()) and "actor_q_avg" in stats


def test_select_actions_uses_the_trained_actor_and_graphs_are_refused(cpu_side):
    tag, g, d, batch, *_ = cpu_side
    mac, learner, _ = learner_for(g, d, "cuda", train_actor=True, actor_loss_coef=COEF)
    with pytest.raises(RuntimeError, match="train_actor"):
        learner.enable_graphs(None, 4)
    obs = torch.tensor(batch["obs"][:, 0], device=DEV)           # [B, J, S]
    E, J = obs.shape[:2]
    avail = torch.ones((E, J, d["A"]), dtype=torch.int32, device=DEV)
    mac.init_hidden(E)
    mac.prepare_static_obs(obs)
    p0 = mac.static_inputs[0].clone()
    _, P_before = mac.select_actions(obs, avail, 0, test_mode=True)
    learner.train(copy.deepcopy(batch), {})
    mac.init_hidden(E)
    mac.prepare_static_obs(obs)                                    # the cache was invalidated: recomputed from the new actor
    p1 = mac.static_inputs[0]
    assert not torch.equal(p1, p0)
    with torch.no_grad():
        a = mac.agent.actor
        ref = a(obs.reshape(E * J, -1))
    np.testing.assert_allclose(p1.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=1e-5)
    T_sel, P_after = mac.select_actions(obs, avail, 0, test_mode=True)
    chosen = ref.view(E, J, -1).gather(2, T_sel.long().view(E, J, 1)).view(E, J)
    np.testing.assert_allclose(P_after.view(E, J).cpu().numpy(), chosen.cpu().numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("body", [False, True], ids=["actor", "actor+body"])
def test_large_batch_update_writes_every_gradient_in_place(body):
    """>= 1024 rows: the TD loss's weight gradients are split-K products too, and with the actor's they all land in the flat
    gradient vector's slices — no packing copy.  Also with ``train_agent_body`` on top."""
    tag, B, T = "3j4r_h64", 16, 24
    g, d = load(tag)
    assert B * (T - 1) * d["J"] >= 1024
    batch = make_learner_batch(g, d, B, T, seed=5)
    mac, learner, _ = learner_for(g, d, "cuda", train_actor=True, **({"train_agent_body": True} if body else {}))
    stats = learner.train(copy.deepcopy(batch), {})
    assert all(np.isfinite(v) for v in stats.values())
    assert learner.grad_pack_launches == 0
    base = learner._flat_grad.data_ptr()
    for p, off in zip(learner._trainable(), learner._flat_offsets):
        assert p.grad.data_ptr() == base + 4 * off
    assert all(p.grad.abs().sum() > 0 for p in mac.agent.actor.parameters())


# --------------------------------------------------------------------------------------------- driver
def test_main_run_with_train_actor(tmp_path):
    import contextlib
    import io
    import json
    import os
    import yaml
    from _harness import REPO
    from macjd_amd.main import build_components, load_config, run, save_checkpoint
    from macjd_amd.scenario import ring_scenario_dict
    import macjd_amd.main as main_mod
    pkg = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
    sim = str(tmp_path / "scenario_2j2r.yaml")
    with open(sim, "w") as f:
        yaml.safe_dump(ring_scenario_dict(2, 2), f)

    def cfg(**kw):
        with contextlib.redirect_stdout(io.StringIO()):
            c = load_config("default", os.path.join(pkg, "config"))
        c.device_request, c.sim_config_path = "cuda", sim
        c.save_model_dir, c.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
        c.log_interval_seconds, c.gemm_tuning, c.resume = 0, False, None
        E = 8
        c.batch_envs, c.buffer_size, c.batch_size, c.start_training_steps = E, 2 * E, E, 0
        c.total_env_steps, c.save_interval, c.updates_per_rollout, c.lr = 3 * E * 100, 10 ** 9, 3, 1e-3
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    c0 = cfg(train_actor=True)
    with contextlib.redirect_stdout(io.StringIO()):
        main_mod._pick_device(c0, 0)
        torch.manual_seed(c0.seed)
        env, mac, buffer, learner, runner = build_components(c0, sim)[:5]
        start = str(tmp_path / "start")
        save_checkpoint(learner, runner, start, 0, 0)
    first = torch.load(os.path.join(start, "agent.pth"), weights_only=True)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = run(cfg(train_actor=True, actor_loss_coef=0.5, resume=start))
    assert res["total_steps"] == 3 * 8 * 100 and res["train_steps"] == 9 and "Training finished." in out.getvalue()
    assert "Avg Actor Q" in out.getvalue()
    rows = [json.loads(l) for l in open(os.path.join(res["log_dir"], "scalars.jsonl"))]
    aq = [r["value"] for r in rows if r["tag"] == "QValues/actor_q_avg"]
    losses = [r["value"] for r in rows if r["tag"].startswith("Loss/")]
    assert aq and all(np.isfinite(v) for v in aq) and losses and all(np.isfinite(v) for v in losses)
    last = os.path.join(c0.save_model_dir, c0.test_name, f"step_{3 * 8 * 100}")
    final = torch.load(os.path.join(last, "agent.pth"), weights_only=True)
    for k in first:
        moved = not torch.equal(final[k], first[k])
        assert moved == k.startswith(("actor.", "fc2_q_head.")), k
