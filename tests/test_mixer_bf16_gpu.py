"""bf16 operands in the fused mixer kernels (``macjd_mixerf_io.operand_dtype = 1``, include/macjd_nets.h): the option
``mixer_dtype: bf16`` runs them (no library / autocast fallback), they compute the numerics contract of the header
(checked through the C-ABI against a float64 emulation of it at every covered size), the paired / one-launch forms of
the learner update equal the launches they replace bit for bit under bf16 as they do in f32, and the learner's
graph-replayed and grouped updates agree with its eager and single ones."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO  # noqa: F401

sys.path.insert(0, os.path.dirname(__file__))
from test_nets_cpu import load, make_args, sd_from  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99
HH, EM, N1 = 128, 64, 384


def _mixers(tag, weights, mixer_dtype="fp32"):
    from macjd_amd.core.networks import QMixer
    g, d = load(tag)
    args = make_args(d, device="cuda", use_cuda=True, mixer_dtype=mixer_dtype)
    torch.manual_seed(5)
    me, mt = QMixer(args).to(DEV), QMixer(args).to(DEV)
    with torch.no_grad():
        if weights == "g4_saturating":   # G4's weight set x 25: every clamp saturates on most rows
            me.load_state_dict(sd_from(g, "mixer."))
            mt.load_state_dict(sd_from(g, "mixer."))
            for p_e, p_t in zip(me.parameters(), mt.parameters()):
                p_e.mul_(25.0)
                p_t.mul_(0.9 * 25.0)
        else:                            # random, spread so that every clamp has rows on both sides
            for p in list(me.parameters()) + list(mt.parameters()):
                p.mul_(3.0)
    return d, args, me, mt


def _params(m):
    from macjd_amd import ops
    ln, (w_cat, b_cat) = m.state_norm, m._first_layer_cat()
    return ops._mixerf_params(ln.weight, ln.bias, ln.eps, w_cat, b_cat, m.hyper_w_1[2].weight, m.hyper_w_1[2].bias,
                              m.hyper_w_final[2].weight, m.hyper_w_final[2].bias, m.V[2].weight, m.V[2].bias,
                              bf16=m.bf16_hyper)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _fwd_bwd(p, q, s, gy, operand_dtype):
    """Forward (activations saved) and backward launches through the C-ABI; every output pre-filled with NaN."""
    from macjd_amd import _native, ops
    lib = _native.load()
    M, J = q.shape
    S = s.shape[1]
    out = {"y": _nan(M), "sn": _nan(M, S), "xhat": _nan(M, S), "act": _nan(M, N1), "gq": _nan(M, J), "gout1": _nan(M, N1),
           "g_w1raw": _nan(M, J * EM), "g_wfraw": _nan(M, EM), "g_v": _nan(M)}
    io = ops._mixerf_io(q, s, p)
    assert io.operand_dtype == (1 if p["bf16"] else 0)   # the argument block carries the parameters' operand type
    io.operand_dtype, io.save = operand_dtype, 1
    for k in ("y", "sn", "xhat", "act"):
        setattr(io, k, out[k].data_ptr())
    _native.check(lib.macjd_mixer_fused_forward(ctypes.byref(io), _stream()), "macjd_mixer_fused_forward")
    bio = ops._mixerf_io(q, None, p)
    bio.operand_dtype = operand_dtype
    bio.act, bio.gy = out["act"].data_ptr(), gy.data_ptr()
    for k in ("gq", "gout1", "g_w1raw", "g_wfraw", "g_v"):
        setattr(bio, k, out[k].data_ptr())
    _native.check(lib.macjd_mixer_fused_backward(ctypes.byref(bio), _stream()), "macjd_mixer_fused_backward")
    torch.cuda.synchronize()
    return out


def _emulate(p, q, s, gy, k):
    """The bf16 contract of include/macjd_nets.h in float64: bf16 rounding (round to nearest even) of exactly the listed
    operands, everything else float64.  The rounded activations / gradients are the kernel's own f32 values (k = its
    saved sn / act and its g_w1raw / g_wfraw): rounding a float64 value and the kernel's f32 value of the same quantity
    lands on different bf16 neighbours for about one element in 2^16, which would move that product by 2^-8 — each of
    those f32 values is itself checked against this chain below."""
    d = lambda t: t.detach().cpu().double()
    bf = lambda t: t.detach().float().cpu().bfloat16().double()
    q, s, gy = d(q), d(s), d(gy)
    M, J = q.shape
    W1, b1, W2, b2, Wf2, bf2, wV2, bV2 = (d(p[n]) for n in ("W1", "b1", "W2", "b2", "Wf2", "bf2", "wV2", "bV2"))
    # forward: LayerNorm f32 (here f64); merged first layer on bf16 operands
    mean = s.mean(1, keepdim=True)
    xhat = (s - mean) / torch.sqrt(((s - mean) ** 2).mean(1, keepdim=True) + float(p["eps"]))
    sn = xhat * d(p["ln_w"]) + d(p["ln_b"])
    out1 = bf(k["sn"]) @ bf(p["W1"]).T + b1
    act = torch.cat([out1[:, :2 * HH + EM].clamp_min(0.0), out1[:, 2 * HH + EM:]], 1)
    ka = d(k["act"])
    h_w1, h_wf, h_v, b1_raw = ka[:, :HH], ka[:, HH:2 * HH], ka[:, 2 * HH:2 * HH + EM], ka[:, 2 * HH + EM:]
    w1_raw = (bf(k["act"][:, :HH]) @ bf(p["W2"]).T + b2).view(M, J, EM)
    wf_raw = bf(k["act"][:, HH:2 * HH]) @ bf(p["Wf2"]).T + bf2
    v_raw = h_v @ wV2 + bV2
    w1, wf = w1_raw.clamp(0.0, 5.0), wf_raw.clamp(0.0, 5.0)
    hid = torch.einsum("mj,mje->me", q, w1) + b1_raw.clamp(-5.0, 5.0)
    h = torch.where(hid > 0, hid, torch.expm1(hid))
    y = (h * wf).sum(1) + v_raw.clamp(-5.0, 5.0)
    # backward: tail gradients f64; the two transposed products on bf16 operands
    inside = lambda x, lo, hi: (x >= lo) & (x <= hi)
    ghid = gy[:, None] * wf * torch.where(hid > 0, torch.ones_like(hid), h + 1.0)
    g_wf = torch.where(inside(wf_raw, 0.0, 5.0), gy[:, None] * h, torch.zeros_like(h))
    g_b1 = torch.where(inside(b1_raw, -5.0, 5.0), ghid, torch.zeros_like(ghid))
    g_w1 = torch.where(inside(w1_raw, 0.0, 5.0), ghid[:, None, :] * q[:, :, None], torch.zeros_like(w1_raw)).reshape(M, J * EM)
    gq = torch.einsum("me,mje->mj", ghid, w1)
    g_v = torch.where(inside(v_raw, -5.0, 5.0), gy, torch.zeros_like(gy))
    relu = lambda c0, c1: (ka[:, c0:c1] > 0).double()
    gout1 = torch.cat([(bf(k["g_w1raw"]) @ bf(p["W2"])) * relu(0, HH), (bf(k["g_wfraw"]) @ bf(p["Wf2"])) * relu(HH, 2 * HH),
                       g_v[:, None] * wV2[None, :] * relu(2 * HH, 2 * HH + EM), g_b1], 1)
    # weight / bias gradients: f32 products of the f32 saved matrices (here f64 of the emulated ones)
    wg = {"W1": gout1.T @ sn, "b1": gout1.sum(0), "W2": g_w1.T @ h_w1, "b2": g_w1.sum(0), "Wf2": g_wf.T @ h_wf,
          "bf2": g_wf.sum(0), "wV2": g_v[None, :] @ h_v, "bV2": g_v.sum(0, keepdim=True)}
    return {"y": y, "sn": sn, "xhat": xhat, "act": act, "gq": gq, "gout1": gout1, "g_w1raw": g_w1, "g_wfraw": g_wf,
            "g_v": g_v}, wg


@pytest.mark.parametrize("tag", ["2j2r_h128", "3j4r_h64", "6j8r_h64", "12j16r_h64"])
@pytest.mark.parametrize("M", [3232, 37])
def test_bf16_kernels_match_the_contract(tag, M):
    """Q_tot, dL/dq, the saved activations, every backward output and the weight-gradient products at bf16 against the
    float64 emulation of the contract.  Tolerance 3e-5 x max|ref| (+ rtol 1e-4): with the rounded operands identical,
    what is left is f32 accumulation — sums of at most 768 terms (the transposed hyper_w_1.2 product at J = 12; 3232 rows
    in a weight gradient), worst case K 2^-24 = 4.6e-5 of the sum of magnitudes, typically sqrt(K) 2^-24 ~ 2e-6 — while a
    single bf16 rounding that differed would move a product by 2^-9 ~ 2e-3 of itself."""
    from macjd_amd import ops
    d, args, me, _ = _mixers(tag, "random")
    rng = np.random.default_rng(M + d["J"])
    f = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=DEV)
    q, s, gy = f(M, d["J"]), 3.0 * f(M, args.state_shape), f(M)
    p = _params(me)
    got = _fwd_bwd(p, q, s, gy, 1)
    ref, wg = _emulate(p, q, s, gy, got)
    for k, r in ref.items():
        g_ = got[k].cpu().double().reshape(r.shape)
        assert not torch.isnan(g_).any(), k
        top = float(r.abs().max())
        np.testing.assert_allclose(g_.numpy(), r.numpy(), rtol=1e-4, atol=3e-5 * max(top, 1e-30), err_msg=k)
    # the clamps really go both ways
    assert float(got["g_w1raw"].abs().max()) > 0 and float((got["g_w1raw"] == 0).float().mean()) > 0.01
    # weight / bias gradients: the unchanged f32 split-K products of the kernel's matrices
    Hh = HH
    prods = {("W1", "b1"): ops.linear_wgrad(got["gout1"], got["sn"]),
             ("W2", "b2"): ops.linear_wgrad(got["g_w1raw"], got["act"][:, :Hh]),
             ("Wf2", "bf2"): ops.linear_wgrad(got["g_wfraw"], got["act"][:, Hh:2 * Hh]),
             ("wV2", "bV2"): ops.linear_wgrad(got["g_v"].view(M, 1), got["act"][:, 2 * Hh:2 * Hh + EM])}
    torch.cuda.synchronize()
    for names, vals in prods.items():
        for n, v in zip(names, vals):
            r = wg[n]
            np.testing.assert_allclose(v.cpu().double().reshape(r.shape).numpy(), r.numpy(), rtol=1e-4,
                                       atol=3e-5 * float(r.abs().max()), err_msg=n)
    # ... and bf16 really ran: the f32 launches on the same inputs differ by more than 2^-12 max|Q_tot|
    f32 = _fwd_bwd(p, q, s, gy, 0)
    dy = float((f32["y"] - got["y"]).abs().max())
    assert dy > 2.0 ** -12 * float(got["y"].abs().max()), dy


def _update(kind, me, mt, q_e, q_t, state, reward, terminated, filled, tot_m, operand_dtype=1):
    """One learner update's mixer launches (bf16 unless told otherwise) through the C-ABI: "single" = saving forward + plain forward +
    backward_td, "pair" = forward_pair + backward_td, "train" = the one-launch form.  Outputs pre-filled with NaN."""
    from macjd_amd import _native, ops
    lib = _native.load()
    B, T1, J = q_e.shape
    M, S = B * T1, state.shape[-1]
    qe, qt, s = q_e.reshape(M, J).contiguous(), q_t.reshape(M, J).contiguous(), state.reshape(M, S).contiguous()
    out = {"y": _nan(M), "tq": _nan(M), "sn": _nan(M, S), "xhat": _nan(M, S), "act": _nan(M, N1), "gq": _nan(M, J),
           "gout1": _nan(M, N1), "g_w1raw": _nan(M, J * EM), "g_wfraw": _nan(M, EM), "g_v": _nan(M)}
    io = ops._mixerf_io(qe, s, _params(me))
    io.save, io.operand_dtype = 1, operand_dtype
    for k in ("y", "sn", "xhat", "act", "gq", "gout1", "g_w1raw", "g_wfraw", "g_v"):
        setattr(io, k, out[k].data_ptr())
    tio = ops._mixerf_io(qt, s, _params(mt))
    tio.y, tio.operand_dtype = out["tq"].data_ptr(), operand_dtype
    td = _native.TdLossIO()
    td.B, td.Tm1, td.gamma = B, T1 - 1, GAMMA
    td.y, td.y_sb = out["y"].data_ptr(), T1
    td.tq, td.tq_sb = out["tq"].data_ptr() + 4, T1
    td.gy, td.gy_sb, td.gy_cols = None, T1, T1
    td.reward, td.r_sb, td.r_st = reward.data_ptr(), reward.stride(0), reward.stride(1)
    td.terminated, td.t_sb, td.t_st = terminated.data_ptr(), terminated.stride(0), terminated.stride(1)
    td.filled, td.f_sb, td.f_st = filled.data_ptr(), filled.stride(0), filled.stride(1)
    st = _stream()
    if kind == "train":
        _native.check(lib.macjd_mixer_fused_train(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(), st),
                      "macjd_mixer_fused_train")
    else:
        if kind == "pair":
            _native.check(lib.macjd_mixer_fused_forward_pair(ctypes.byref(io), ctypes.byref(tio), st),
                          "macjd_mixer_fused_forward_pair")
        else:
            _native.check(lib.macjd_mixer_fused_forward(ctypes.byref(io), st), "macjd_mixer_fused_forward")
            _native.check(lib.macjd_mixer_fused_forward(ctypes.byref(tio), st), "macjd_mixer_fused_forward")
        _native.check(lib.macjd_mixer_fused_backward_td(ctypes.byref(io), ctypes.byref(td), tot_m.data_ptr(), st),
                      "macjd_mixer_fused_backward_td")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag", ["3j4r_h64", "2j2r_h128", "6j8r_h64", "12j16r_h64"])
@pytest.mark.parametrize("weights", ["random", "g4_saturating"])
def test_bf16_pairing_is_bitwise(tag, weights):
    """Under bf16, forward_pair equals the two single forwards and (J in {2, 3}) the training launch equals forward_pair +
    backward_td, every output bit for bit — the grid forms re-derive w1_raw / wf_raw with the same bf16 instruction
    sequence as the forward they stand in for.  6j/8r: the single and the pair forward both load late at bf16 (LATE2);
    12j/16r: the wide pair and the wide backward_td."""
    from macjd_amd import ops
    d, args, me, mt = _mixers(tag, weights)
    B, T1 = 32, 101                            # M = 3232
    rng = np.random.default_rng(7)
    f = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=DEV)
    q_e, q_t, state, reward = f(B, T1, d["J"]), f(B, T1, d["J"]), 3.0 * f(B, T1, args.state_shape), f(B, T1, 1)
    lens = torch.tensor(rng.integers(2, T1 + 1, B))
    steps = torch.arange(T1).view(1, T1, 1)
    filled = (steps < lens.view(B, 1, 1)).to(DEV)
    terminated = (steps >= (lens.view(B, 1, 1) - 1)).to(DEV)
    batch = (q_e, q_t, state, reward, terminated, filled)
    tot_m = ops.td_mask_sum(filled, T1 - 1)
    pair = _update("pair", me, mt, *batch, tot_m)
    single = _update("single", me, mt, *batch, tot_m)
    for k in pair:
        assert not torch.isnan(pair[k]).any(), k
        assert torch.equal(pair[k], single[k]), k
    if weights == "random":                    # (the clamps really go both ways: the gradients are not all zero)
        assert float(pair["g_w1raw"].abs().max()) > 0 and float(pair["gout1"].abs().max()) > 0
    if d["J"] in (2, 3):
        train = _update("train", me, mt, *batch, tot_m)
        for k in pair:
            a, b = pair[k], train[k]
            if k == "tq":                      # row 0 is no loss row's target: the training launch does not write it
                a, b = a[1:], b[1:]
            assert not torch.isnan(b).any(), k
            assert torch.equal(a, b), k


_SIZES = ["2j2r_h128", "3j4r_h64", "6j8r_h64", "12j16r_h64"]   # the BASELINE scenario sizes


@pytest.mark.parametrize("tag", _SIZES)
def test_bf16_option_runs_the_fused_kernels(tag, monkeypatch):
    """``mixer_dtype: bf16`` takes the one-launch mixer with bf16 operands: ``fused_available`` is True (False under an
    outer autocast), a training forward + backward and an inference forward go through the native entry points only —
    the library / autocast path (ops.linear, ops.layer_norm, QMixer._hyper_networks) raises if touched — and Q_tot and
    dL/dq are the bf16 launches' results bit for bit."""
    from macjd_amd import _native, ops
    from macjd_amd.core.networks import QMixer
    d, args, me, _ = _mixers(tag, "random", mixer_dtype="bf16")
    assert me.bf16_hyper
    probe = torch.zeros(1, device=DEV)
    assert me.fused_available(probe)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not me.fused_available(probe)

    def boom(*a, **k):
        raise AssertionError("library / autocast mixer path taken under mixer_dtype=bf16")
    for name in ("linear", "layer_norm", "merged_linear", "norm_merged_linear", "split_relu", "mixer_tail"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(QMixer, "_hyper_networks", boom)
    lib = _native.load()
    seen = []
    for name in ("macjd_mixer_fused_forward", "macjd_mixer_fused_backward"):
        real = getattr(lib, name)

        def spy(io, stream, real=real, name=name):
            seen.append((name, io._obj.operand_dtype))
            return real(io, stream)
        monkeypatch.setattr(lib, name, spy)
    B, T = 4, 101
    rng = np.random.default_rng(3)
    f = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32, device=DEV)
    q, s, gy = f(B, T, d["J"]), 3.0 * f(B, T, args.state_shape), f(B, T, 1)
    qg = q.clone().requires_grad_(True)
    y = me(qg, s)
    y.backward(gy)
    torch.cuda.synchronize()
    assert seen == [("macjd_mixer_fused_forward", 1), ("macjd_mixer_fused_backward", 1)], seen
    for n, p_ in me.named_parameters():
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), n
    assert float(me.hyper_w_1[2].weight.grad.abs().max()) > 0
    with torch.no_grad():
        y_inf = me(q, s)
    assert seen[-1] == ("macjd_mixer_fused_forward", 1)
    monkeypatch.undo()
    M = B * T
    p = _params(me)
    assert p["bf16"]
    raw = _fwd_bwd(p, q.reshape(M, -1).contiguous(), s.reshape(M, -1).contiguous(), gy.reshape(M).contiguous(), 1)
    assert torch.equal(y.detach().reshape(M), raw["y"]) and torch.equal(y_inf.reshape(M), raw["y"])
    assert torch.equal(qg.grad.reshape(M, -1), raw["gq"])


def _learner(tag, k, T=100, N=48, B=32):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    from test_nets_cpu import quiet
    from tests_golden_helpers import synthetic_batch
    g, d = load(tag)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=T, buffer_size=N, batch_size=B,
                     target_update_interval=200, lr=1e-3, mixer_dtype="bf16")
    torch.manual_seed(0)
    with quiet():
        mac = BasicMAC(d["S"], args)
        if tag == "3j4r_h64":
            mac.load_state(sd_from(g, "g5_agent0."))
        learner = QMixLearner(mac, args)
        buf = EpisodeReplayBuffer(args)
    if tag == "3j4r_h64":
        learner.eval_qmix_net.load_state_dict(sd_from(g, "g5_mixer0."))
    learner._update_targets()
    full = synthetic_batch(np.random.default_rng(9), args, N, T)
    for kk, v in buf.buffers.items():
        v.copy_(torch.as_tensor(full[kk]).to(v.dtype))
    buf.current_size, buf.current_index = N, 0
    buf.episode_lengths[:] = T
    obs = buf.buffers["obs"]   # static observations, as the batched runner stores them: the pipelined, paired update
    obs.copy_(obs[:, :1].expand_as(obs).clone())
    buf.obs_static = True
    learner.enable_graphs(buf, B, updates_per_graph=k)
    assert k == 1 or learner._g_pipelined
    import gc
    gc.collect()
    torch.cuda.empty_cache()   # (a baked address of a dead tensor would fault at the first replay)
    return mac, learner, buf


@pytest.mark.parametrize("tag", ["3j4r_h64", "12j16r_h64"])
def test_bf16_learner_updates(tag, monkeypatch):
    """The learner at mixer_dtype=bf16: the paired update forms apply (``_paired_heads_ok``; at 3j/4r the one-launch
    training kernel, MACJD_MIXER_TRAIN), the graph-replayed update equals the eager ``learner.train()`` on the same
    episodes at the fp32 tolerances of test_other_baseline_configs_end_to_end (f32 reordering, not bf16 error), and at
    3j/4r grouped updates (updates_per_graph = 3) end on the same weights as single updates, bit for bit."""
    from macjd_amd import ops
    from macjd_amd.core.qmix import QMixLearner
    oks, trains = [], []
    real_ok, real_train = QMixLearner._paired_heads_ok, ops._mixer_train
    monkeypatch.setattr(QMixLearner, "_paired_heads_ok", lambda self, *a: oks.append(real_ok(self, *a)) or oks[-1])
    monkeypatch.setattr(ops, "_mixer_train", lambda *a: trains.append(a[2]["bf16"]) or real_train(*a))
    mac_k, many, _ = _learner(tag, 3)
    assert many.eval_qmix_net.bf16_hyper and many.target_qmix_net.fused_available(torch.zeros(1, device=DEV))
    rows = []
    for _ in range(2):
        rows += [r.clone() for r in many.train_from_buffer_many(3)]
    assert bool(torch.isfinite(torch.stack(rows)).all())
    assert oks and all(oks), oks
    if tag == "3j4r_h64":
        assert trains and all(trains), trains
    # graph replay vs eager learner.train() on the same episodes from the same state
    mac_1, one, buf = _learner(tag, 1)
    idx = np.random.default_rng(1).choice(buf.current_size, 32, replace=False)
    snap = ([p_.detach().clone() for p_ in one.params], one._flat_exp_avg.clone(), one._flat_exp_avg_sq.clone(),
            one._adam_step.clone(), one.train_step, one.last_target_update_step)
    st_e = one.train(buf.sample(32, indices=idx), {})
    g_e = one._flat_grad.clone()
    with torch.no_grad():
        for p_, q_ in zip(one.params, snap[0]):
            p_.copy_(q_)
        one._flat_exp_avg.copy_(snap[1]); one._flat_exp_avg_sq.copy_(snap[2]); one._adam_step.copy_(snap[3])
    one.train_step, one.last_target_update_step = snap[4], snap[5]
    one._mark_body_shared()
    st_g = one.train_from_buffer(indices=idx)
    g_g = one._flat_grad.clone()
    for k_ in st_e:
        assert st_g[k_] == pytest.approx(st_e[k_], rel=1e-4, abs=1e-5), k_
    scale = float(g_e.abs().max())
    np.testing.assert_allclose(g_g.cpu().numpy(), g_e.cpu().numpy(), rtol=1e-3, atol=2e-5 * max(scale, 1e-12))
    if tag != "3j4r_h64":
        return
    # grouped (pipelined, paired, one-launch mixer) vs single updates: six updates each from the same state
    mac_s, single, _ = _learner(tag, 1)
    mac_g, grouped, _ = _learner(tag, 3)
    ref = torch.zeros(6, 4, device=DEV)
    for i in range(6):
        single.train_from_buffer(sync_stats=False, stats_row=ref[i])
    got = []
    for _ in range(2):
        got += [r.clone() for r in grouped.train_from_buffer_many(3)]
    np.testing.assert_allclose(torch.stack(got).cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-7)
    assert single.train_step == grouped.train_step == 6
    for (k_, a), b in zip(mac_s.agent.state_dict().items(), mac_g.agent.state_dict().values()):
        assert torch.equal(a, b), k_
    for (k_, a), b in zip(single.eval_qmix_net.state_dict().items(), grouped.eval_qmix_net.state_dict().values()):
        assert torch.equal(a, b), k_
