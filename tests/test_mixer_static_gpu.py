"""The static-state training launch (``macjd_mixer_fused_train_static``, csrc/macjd_mixer.hip) through the C-ABI, against
``macjd_mixer_fused_train`` on the same inputs and against the float64 model (tests/mixer_f64_model.py,
tests/mixer_static_model.py; the algebra itself: tests/test_mixer_static_cpu.py), and the learner's use of it.

J in {2, 3}, (B, T1) in {(3, 5), (2, 16), (2, 17), (3, 33), (1, 101)}: one tile with 11 dead rows, an exact tile, a second
tile with one live row, three tiles, the real T1; episode ends on the first row of a tile, on the last row of a tile and
mid-tile (mixer_static_model.CASES); states constant per episode, row T1 - 1 zeros as in the runner's stage buffers.
Outputs are pre-filled with NaN between NaN margins, inputs sit between NaN margins (test_mixer_f64_gpu.py's helpers).

Bars.  y, the target's y (rows >= 1) and gq: ``torch.equal`` with macjd_mixer_fused_train, f32 and bf16 operands; so are
the compact sn / xhat / act rows with that launch's rows at each tile's row 0.  Compact sums against float64 per-tile sums
of that launch's per-row outputs: rtol 1e-4, atol ATOL[name] x max|ref| of test_mixer_f64_gpu.py.  Module parameter
gradients after the grouped weight-gradient pass against the float64 model: that file's ``wgrad`` bar.  Learner: the bounds
of test_learner_static_observation_hoist_equals_per_step_evaluation (statistics rel 1e-4 / abs 1e-6, weights atol 2e-5).

Worst |got - ref| / max|ref| measured on MI355X over all cases (each test prints its own):
    compact sums (f32 and bf16 operands, against bars of 6e-6 .. 1e-5):
        gout1 9.04e-8    g_w1raw 1.77e-7    g_wfraw 1.15e-7    g_v 1.48e-7
    module path: parameter gradients 9.67e-7 (bar 7e-6), target values 1.36e-7 of max(1, max|ref|) (bar 1e-5)
    y, target y (rows >= 1), gq, the compact sn / xhat / act rows and a second launch: bit for bit."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _harness import REPO, load_scenario  # noqa: F401

sys.path.insert(0, os.path.dirname(__file__))
import mixer_f64_model as mm  # noqa: E402
import mixer_static_model as ms  # noqa: E402
import test_mixer_f64_gpu as mf  # noqa: E402
from test_nets_cpu import load, make_args, quiet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = mf.DEV
EM, N1 = mm.EM, mm.N1
EINVAL = -1
PER_ROW = ("y", "tq", "gq")
COMPACT = ms.ROW0 + ms.SUMMED


def _case(J, B, T1):
    host = ms.static_inputs(J, B, T1)
    pe, pt, q_e, q_t, state, reward, terminated, filled = host
    dev = {"pe": mf._device_params(pe), "pt": mf._device_params(pt)}
    dev["q_e"], dev["k0"] = mf._inp(q_e)
    dev["q_t"], dev["k1"] = mf._inp(q_t)
    dev["state"], dev["k2"] = mf._inp(state)
    dev["reward"] = mf._dev(reward)[:, :-1]
    dev["terminated"] = mf._dev(terminated, torch.bool)[:, :-1]
    dev["filled"] = mf._dev(filled, torch.bool)[:, :-1]
    return host, dev


def _blocks(dev, B, T1, J, bf16, out):
    """(eval io, target io, td) of one training call; per-row outputs y / tq / gq from ``out``."""
    from macjd_amd import _native, ops
    M, S = B * T1, dev["state"].shape[-1]
    io = ops._mixerf_io(dev["q_e"].view(M, J), dev["state"].view(M, S), dev["pe"])
    tio = ops._mixerf_io(dev["q_t"].view(M, J), dev["state"].view(M, S), dev["pt"])
    io.save, io.operand_dtype, tio.operand_dtype = 1, int(bf16), int(bf16)
    io.y, io.gq, tio.y = out["y"].t.data_ptr(), out["gq"].t.data_ptr(), out["tq"].t.data_ptr()
    td = _native.TdLossIO()
    td.B, td.Tm1, td.gamma = B, T1 - 1, mm.GAMMA
    td.y, td.y_sb = out["y"].t.data_ptr(), T1
    td.tq, td.tq_sb = out["tq"].t.data_ptr() + 4, T1
    td.gy, td.gy_sb, td.gy_cols = None, T1, T1
    r, t, f = dev["reward"], dev["terminated"], dev["filled"]
    td.reward, td.r_sb, td.r_st = r.data_ptr(), r.stride(0), r.stride(1)
    td.terminated, td.t_sb, td.t_st = t.data_ptr(), t.stride(0), t.stride(1)
    td.filled, td.f_sb, td.f_st = f.data_ptr(), f.stride(0), f.stride(1)
    return io, tio, td


def _compact_outputs(n_tiles, J, S):
    shapes = {"sn": (n_tiles, S), "xhat": (n_tiles, S), "act": (n_tiles, N1), "gout1": (n_tiles, N1),
              "g_w1raw": (n_tiles, J * EM), "g_wfraw": (n_tiles, EM), "g_v": (n_tiles,)}
    return {k: mf._Guarded(shapes[k], mf.OUT_MARGIN) for k in COMPACT}


def _static_io(out, n_tiles):
    from macjd_amd import _native
    st = _native.MixerStaticIO()
    st.n_tiles = n_tiles
    st.sn, st.xhat, st.act = (out[k].t.data_ptr() for k in ms.ROW0)
    st.gout1_sum, st.g_w1raw_sum, st.g_wfraw_sum, st.g_v_sum = (out[k].t.data_ptr() for k in ms.SUMMED)
    return st


def _train(dev, B, T1, J, tot_m, bf16):
    """macjd_mixer_fused_train: every per-row output."""
    from macjd_amd import _native
    lib = _native.load()
    out = mf._outputs(B * T1, J, dev["state"].shape[-1], mm.OUTPUTS + ("tq",))
    io, tio, td = _blocks(dev, B, T1, J, bf16, out)
    for k in ("sn", "xhat", "act", "gout1", "g_w1raw", "g_wfraw", "g_v"):
        setattr(io, k, out[k].t.data_ptr())
    _native.check(lib.macjd_mixer_fused_train(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                              mf._stream()), "macjd_mixer_fused_train")
    return mf._finish(out)


def _train_static(dev, B, T1, J, tot_m, bf16):
    """macjd_mixer_fused_train_static: y / tq / gq per row, the rest compact."""
    from macjd_amd import _native
    lib = _native.load()
    S, n_tiles = dev["state"].shape[-1], B * ms.tiles_per_episode(T1)
    out = mf._outputs(B * T1, J, S, PER_ROW)
    out.update(_compact_outputs(n_tiles, J, S))
    io, tio, td = _blocks(dev, B, T1, J, bf16, out)
    st = _static_io(out, n_tiles)
    _native.check(lib.macjd_mixer_fused_train_static(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                                     ctypes.byref(st), mf._stream()), "macjd_mixer_fused_train_static")
    return mf._finish(out)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T1", sorted(ms.CASES))
@pytest.mark.parametrize("J", [2, 3])
def test_static_launch_against_the_per_row_launch(J, B, T1, bf16):
    from macjd_amd import ops
    host, dev = _case(J, B, T1)
    filled = host[-1]
    tot_m = ops.td_mask_sum(dev["filled"], T1 - 1)
    assert float(tot_m) == float(filled[:, :-1].sum()) > 0
    rows = _train(dev, B, T1, J, tot_m, bf16)
    got = _train_static(dev, B, T1, J, tot_m, bf16)
    again = _train_static(dev, B, T1, J, tot_m, bf16)
    what = f"static J={J} B={B} T1={T1} {'bf16' if bf16 else 'f32'}"
    for k in got:
        g = got[k][1:] if k == "tq" else got[k]       # (row 0 of the target values is no loss row's target: not written)
        assert not bool(torch.isnan(g).any()), f"{what}: {k} has an unwritten element"
        assert torch.equal(g, again[k][1:] if k == "tq" else again[k]), f"{what}: {k} differs between two launches"
    assert bool(torch.isnan(got["tq"][0])), "row 0 of the target values was written"
    # per row: bit for bit
    assert torch.equal(got["y"], rows["y"]) and torch.equal(got["gq"], rows["gq"]), what
    assert torch.equal(got["tq"][1:], rows["tq"][1:]), what
    # one row per tile, the tile's row 0: bit for bit
    tr = ms.tile_rows(B, T1)
    first = torch.tensor([lo for lo, _ in tr], device=DEV)
    for k in ms.ROW0:
        assert torch.equal(got[k], rows[k].reshape(B * T1, -1)[first].reshape(got[k].shape)), f"{what}: {k}"
    # per-tile sums against float64 sums of the per-row launch's rows
    ref = ms.compact({k: rows[k] for k in COMPACT}, B, T1)
    worst, bad = {}, []
    for k in ms.SUMMED:
        r = ref[k]
        g = got[k].detach().cpu().double().reshape(r.shape)
        top = float(r.abs().max())
        worst[k] = float((g - r).abs().max()) / top if top > 0 else float((g - r).abs().max())
        if not np.allclose(g.numpy(), r.numpy(), rtol=1e-4, atol=mf.ATOL[k] * top):
            bad.append(k)
    print(f"{what}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert not bad, f"{what}: {bad} beyond the bar; worst |got - ref| / max|ref|: {worst}"
    assert float(ref["gout1"].abs().max()) > 0
    # tiles whose every row is without loss gradient (they begin at or past the episode's end, or hold only row T1 - 1)
    lens = filled.reshape(B, T1).sum(1)
    tpe = ms.tiles_per_episode(T1)
    dead = [b * tpe + k for b in range(B) for k in range(tpe) if ms.TILE * k >= min(int(lens[b]), T1 - 1)]
    assert (len(dead) >= 2) == ((B, T1) in ((2, 17), (3, 33))), dead
    for k in ms.SUMMED:
        assert bool((got[k].cpu().reshape(len(tr), -1)[dead] == 0).all()), f"{what}: {k} of a tile without loss is not zero"


@pytest.mark.parametrize("tag", ["2j2r_h128", "3j4r_h64"])
def test_module_gradients_through_the_static_launch(tag):
    """The target QMixer's paired block with ``static_rows``, the eval QMixer's forward (which takes it: one launch of
    macjd_mixer_fused_train_static), ``backward`` inside ``ops.deferred_wgrad()``: the five weight-gradient products run over
    K = n_tiles rows.  q.grad and every named parameter's gradient against the float64 model (the mask sides of the near-
    threshold elements read off the per-row launch, as in test_mixer_f64_gpu.py)."""
    from macjd_amd import ops
    from macjd_amd.core.networks import QMixer
    g, d = load(tag)
    J = d["J"]
    args = make_args(d, device="cuda", use_cuda=True)
    me = mm.x3_mixer(QMixer, args).to(DEV)
    mt = copy.deepcopy(me)
    with torch.no_grad():
        for p_ in mt.parameters():
            p_.mul_(0.9)
    B, T1 = 3, 33
    _, _, q, q_t, state, reward, terminated, filled = ms.static_inputs(J, B, T1)
    assert state.shape[-1] == d["S"]
    pe = mm.params_from_state_dict(me.state_dict(), me.state_norm.eps)
    pt = mm.params_from_state_dict(mt.state_dict(), mt.state_norm.eps)
    dq, dqt, dstate = mf._dev(q).requires_grad_(True), mf._dev(q_t), mf._dev(state)
    drew = mf._dev(reward)[:, :-1]
    dterm, dfill = mf._dev(terminated, torch.bool)[:, :-1], mf._dev(filled, torch.bool)[:, :-1]
    tot_m = ops.td_mask_sum(dfill, T1 - 1)
    launched = []
    real = ops._mixer_train
    ops._mixer_train = lambda *a: launched.append(a[3][4]) or real(*a)
    try:
        with torch.no_grad():
            tq_dev, placeholder = mt.forward_paired_with_next_fused(
                dqt, dstate, td=dict(reward=drew, terminated=dterm, filled=dfill, gamma=mm.GAMMA, Tm1=T1 - 1, tot_m=tot_m,
                                     static_rows=True))
        y = me(dq, dstate)
        ops.assert_pairs_launched()
    finally:
        ops._mixer_train = real
        ops.clear_pending_pairs()
    assert launched == [True]
    with ops.deferred_wgrad():
        y.backward(placeholder)
    torch.cuda.synchronize()
    tq_ref = mm.target_values(pt, q_t, state)
    first, _ = mm.td_reference(pe, q, state, tq_ref, reward, terminated, filled, mm.GAMMA)
    ln, (w_cat, b_cat) = me.state_norm, me._first_layer_cat()
    dp = ops._mixerf_params(ln.weight, ln.bias, ln.eps, w_cat, b_cat, me.hyper_w_1[2].weight, me.hyper_w_1[2].bias,
                            me.hyper_w_final[2].weight, me.hyper_w_final[2].bias, me.V[2].weight, me.V[2].bias)
    M = B * T1
    rows = mf._update("single", dp, None, dq.detach(), None, dstate, drew, dterm, dfill, tot_m, tq=tq_dev.reshape(B, T1).contiguous())
    assert torch.equal(rows["y"], y.detach().reshape(M)) and torch.equal(rows["gq"], dq.grad.reshape(M, J))
    decisions, _ = mf._kernel_decisions(first, rows)
    ref, _ = mm.td_reference(pe, q, state, tq_ref, reward, terminated, filled, mm.GAMMA, decisions)
    mf._compare({"tq": tq_dev.reshape(-1)[1:]}, {"tq": tq_ref.reshape(-1)[1:]}, ("tq",), f"static module {tag}")
    want = mm.state_dict_grads(ref["grads"], d["S"])
    grads = {n: p_.grad for n, p_ in me.named_parameters()}
    assert sorted(grads) == sorted(want) and all(v is not None for v in grads.values())
    mf._compare(grads, want, sorted(want), f"static module {tag} (parameters)", atol_key="wgrad")
    assert float(want["state_norm.weight"].abs().max()) > 0 and float(want["hyper_w_1.2.weight"].abs().max()) > 0


def test_argument_checks():
    """MACJD_EINVAL, nothing launched, nothing written: M != B x T1, J not in {2, 3}, differing operand types, a NULL
    compact pointer, a per-row operand buffer (this launch would not fill it)."""
    from macjd_amd import _native, ops
    lib = _native.load()
    J, B, T1 = 3, 2, 17
    host, dev = _case(J, B, T1)
    S, n_tiles = dev["state"].shape[-1], B * ms.tiles_per_episode(T1)
    tot_m = ops.td_mask_sum(dev["filled"], T1 - 1)
    out = mf._outputs(B * T1, J, S, PER_ROW)
    out.update(_compact_outputs(n_tiles, J, S))

    def call(change):
        io, tio, td = _blocks(dev, B, T1, J, False, out)
        st = _static_io(out, n_tiles)
        change(io, tio, td, st)
        return lib.macjd_mixer_fused_train_static(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                                  ctypes.byref(st), mf._stream())

    def rows_off(io, tio, td, st):
        td.B = B + 1

    def six_agents(io, tio, td, st):
        io.J = tio.J = 6

    def dtypes(io, tio, td, st):
        tio.operand_dtype = 1

    def per_row(io, tio, td, st):
        io.act = out["act"].t.data_ptr()

    def tiles(io, tio, td, st):
        st.n_tiles = n_tiles + 1

    changes = [rows_off, six_agents, dtypes, per_row, tiles]
    for name in ("sn", "xhat", "act", "gout1_sum", "g_w1raw_sum", "g_wfraw_sum", "g_v_sum"):
        changes.append(lambda io, tio, td, st, name=name: setattr(st, name, None))
    for change in changes:
        assert call(change) == EINVAL, getattr(change, "__name__", "NULL compact pointer")
    torch.cuda.synchronize()
    for k, g in out.items():
        assert bool(torch.isnan(g.buf).all()), k
    assert call(lambda *a: None) == 0
    mf._finish(out)


# ---------------------------------------------------------------------------------------------------------------
def _runner_learner(monkeypatch, switch, K, interval, E=64, Bsz=32):
    """3j/4r learner on a buffer filled by the batched runner (static observations and states), updates_per_graph = K."""
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    sc, _ = load_scenario("3j4r")
    monkeypatch.setenv("MACJD_MIXER_STATIC_STATE", switch)
    env = BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=5)
    info = env.get_env_info()
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=2 * E, batch_size=Bsz,
                     lr=1e-3, epsilon_start=0.5, target_update_interval=interval)
    args.env_info = info
    torch.manual_seed(3)
    with quiet():
        mac = BasicMAC(info["obs_shape"], args)
        buf = EpisodeReplayBuffer(args)
        learner = QMixLearner(mac, args)
    BatchedEpisodeRunner(env, mac, buf, args).run(sync_stats=False)
    assert buf.obs_static is True and buf.state_static is True
    state = buf.buffers["state"][:E]
    assert torch.equal(state[:, :-1], state[:, :1].expand_as(state[:, :-1])) and float(state[:, 0].abs().max()) > 0
    learner.enable_graphs(buf, Bsz, updates_per_graph=K)
    return learner, buf, mac


def _same(la, ma, lb, mb, sa, sb):
    for i, (ra, rb) in enumerate(zip(sa.cpu().numpy(), sb.cpu().numpy())):
        for col, k in enumerate(("loss", "eval_qtot_avg", "target_qtot_avg", "grad_norm")):
            assert ra[col] == pytest.approx(rb[col], rel=1e-4, abs=1e-6), (i, k)
    for (k, a), b in zip(ma.agent.state_dict().items(), mb.agent.state_dict().values()):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-5, rtol=0, err_msg=k)
    for (k, a), b in zip(la.eval_qmix_net.state_dict().items(), lb.eval_qmix_net.state_dict().values()):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-5, rtol=0, err_msg=k)


def test_learner_updates_equal_with_the_switch_on_and_off(monkeypatch):
    """Four updates (two replays of a two-update group, a target sync between them) on the runner's episodes with
    MACJD_MIXER_STATIC_STATE = 1 and = 0: same statistics and weights; the learner's bookkeeping says which launch each
    captured."""
    la, ba, ma = _runner_learner(monkeypatch, "1", 2, 2)
    lb, bb, mb = _runner_learner(monkeypatch, "0", 2, 2)
    assert la._g_pipelined and lb._g_pipelined and la._g_state_static and lb._g_state_static
    assert la._g_mixer_static is True and lb._g_mixer_static is False
    for k in ba.buffers:
        assert torch.equal(ba.buffers[k], bb.buffers[k]), k
    sa, sb = torch.zeros(4, 4, device=DEV), torch.zeros(4, 4, device=DEV)
    la.train_from_buffer_many(4, stats_out=sa)
    lb.train_from_buffer_many(4, stats_out=sb)
    assert la.train_step == lb.train_step == 4 and la.last_target_update_step == lb.last_target_update_step == 4
    assert len({float(x) for x in sa[:, 0]}) == 4
    _same(la, ma, lb, mb, sa, sb)


def test_grouped_replay_with_the_static_launch_equals_single_updates(monkeypatch):
    """One grouped replay of three updates with the switch on (the static-state launch) against three single updates (whose
    graph holds the general path: no mixer training launch there)."""
    lg, _, mg = _runner_learner(monkeypatch, "1", 3, 5)
    l1, _, m1 = _runner_learner(monkeypatch, "1", 1, 5)
    assert lg._g_mixer_static is True and lg._g_multi[0] == 3
    assert l1._g_mixer_static is False and l1._g_multi is None
    sg, s1 = torch.zeros(3, 4, device=DEV), torch.zeros(3, 4, device=DEV)
    lg.train_from_buffer_many(3, stats_out=sg)
    for i in range(3):
        l1.train_from_buffer(sync_stats=False, stats_row=s1[i])
    assert lg.train_step == l1.train_step == 3
    _same(lg, mg, l1, m1, sg, s1)


def test_synthetic_buffer_takes_the_general_path():
    """A buffer filled synthetically carries no certificate (``obs_static`` / ``state_static`` None) — and one whose
    ``obs_static`` a caller set by hand still says nothing about the states: the captured group keeps the per-row launch."""
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    from test_nets_cpu import sd_from
    from tests_golden_helpers import synthetic_batch
    g, d = load("3j4r_h64")
    T, N, B = 100, 40, 32
    for by_hand in (False, True):
        args = make_args(d, device="cuda", use_cuda=True, episode_limit=T, buffer_size=N, batch_size=B, target_update_interval=200)
        with quiet():
            mac = BasicMAC(d["S"], args)
            mac.load_state(sd_from(g, "g5_agent0."))
            learner = QMixLearner(mac, args)
            buf = EpisodeReplayBuffer(args)
        full = synthetic_batch(np.random.default_rng(9), args, N, T)
        for kk, v in buf.buffers.items():
            v.copy_(torch.as_tensor(full[kk]).to(v.dtype))
        buf.current_size, buf.current_index = N, 0
        buf.episode_lengths[:] = T
        assert buf.obs_static is None and buf.state_static is None
        if by_hand:
            obs = buf.buffers["obs"]
            obs.copy_(obs[:, :1].expand_as(obs).clone())
            buf.obs_static = True
        learner.enable_graphs(buf, B, updates_per_graph=2)
        assert learner._g_obs_static == by_hand and learner._g_pipelined == by_hand
        assert learner._g_state_static is False and learner._g_mixer_static is False
        rows = learner.train_from_buffer_many(2)
        assert bool(torch.isfinite(torch.stack(rows)).all())
