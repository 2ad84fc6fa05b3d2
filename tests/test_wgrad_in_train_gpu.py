"""The static-state training launch with the weight-gradient block (``macjd_mixer_fused_train_static_wgrad``,
csrc/macjd_mixer.hip) followed by the reduce launch alone (``macjd_linear_wgrad_many_norm`` on problems of kind external
slots / row products): the update chain without a partial-products launch, through the C-ABI.

J = 3 / A = 9 / S = 46 and J = 2 / A = 5 / S = 24, B = 2, T1 in {5, 16, 17, 33} with Tm1 = T1 - 1: one partial tile, exactly one
tile, a second tile whose single row (t = T1 - 1) is not live, three tiles.  Every buffer between NaN margins; some taken
indices outside [0, A).  A workgroup reads the Q-head rows of its own episode only: with NaN in every ``h`` / ``act_q`` row of
the OTHER episode the slots of an episode's tiles are bit-equal to the clean run's.

Asserted: everything the launch wrote before the block existed is bit-equal to the launch without it; two runs are bit-equal;
after the reduce, dW1 / db1 / dw2 / db2 of the Q-head, the mixer's five weight and bias gradients and dgamma / dbeta against a
float64 evaluation of the same sums of the same float32 operands (the launch's own gq and compact rows), within the forward
bound of a length-n float32 sum in any order, gamma_(n + 2) x sum |terms| with gamma_k = k u / (1 - k u), u = 2^-24 and the
sum of magnitudes in float64: n = the B T1 J agent rows for the Q-head's outputs, n_tiles for the mixer's, 384 n_tiles (terms
xhat W g) for dgamma / dbeta.  Nothing is NaN."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import mixer_f64_model as mm  # noqa: E402
import mixer_static_model as ms  # noqa: E402
import test_mixer_f64_gpu as mf  # noqa: E402
import test_mixer_static_gpu as st  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = mf.DEV
U = 2.0 ** -24
H = 64
EINVAL, EUNSUPPORTED = -1, -4
LENS = {5: (3, 4), 16: (1, 15), 17: (16, 8), 33: (17, 8)}
ACTIONS = {3: 9, 2: 5}


def _gamma(k):
    return k * U / (1.0 - k * U)


def _case(J, B, T1):
    host = ms.static_inputs(J, B, T1, lens=LENS[T1])
    pe, pt, q_e, q_t, state, reward, terminated, filled = host
    dev = {"pe": mf._device_params(pe), "pt": mf._device_params(pt)}
    dev["q_e"], dev["k0"] = mf._inp(q_e)
    dev["q_t"], dev["k1"] = mf._inp(q_t)
    dev["state"], dev["k2"] = mf._inp(state)
    dev["reward"] = mf._dev(reward)[:, :-1]
    dev["terminated"] = mf._dev(terminated, torch.bool)[:, :-1]
    dev["filled"] = mf._dev(filled, torch.bool)[:, :-1]
    return host, dev


def _qhead(J, A, B, T1):
    """The Q-head grid's side of the block on the B T1 J agent rows: ReLU output (about half zeros), h, taken index (some
    outside [0, A)), P, w2 — host float32 arrays."""
    n = B * T1 * J
    rng = np.random.default_rng(mm.case_seed(J, B, T1, 77))
    act = np.maximum(rng.standard_normal((n, H)), 0.0).astype(np.float32)
    h = rng.standard_normal((n, H)).astype(np.float32)
    idx = rng.integers(0, A, n).astype(np.int64)
    idx[::7], idx[3::11] = -1, A          # no one in those rows
    idx[5::13] = 2 ** 33 + 1              # (not an int32 value either)
    P = rng.random(n).astype(np.float32)
    w2 = rng.standard_normal(H).astype(np.float32)
    return act, h, idx, P, w2


def _launch(dev, qh, J, A, B, T1, tot_m, block=True, spoil=None, idx32=False, tweak=None):
    """One launch; returns (outputs, keep) — per-row y / tq / gq, the compact rows and, with ``block``, ws1 / ws2 / ln.
    ``spoil`` = episode whose h / act_q rows are NaN.  ``tweak(wb)`` edits the block (host-check cases: returns the code)."""
    from macjd_amd import _native
    lib = _native.load()
    S, tpe = dev["state"].shape[-1], ms.tiles_per_episode(T1)
    n_tiles = B * tpe
    out = mf._outputs(B * T1, J, S, st.PER_ROW)
    out.update(st._compact_outputs(n_tiles, J, S))
    io, tio, td = st._blocks(dev, B, T1, J, False, out)
    sio = st._static_io(out, n_tiles)
    if not block:
        _native.check(lib.macjd_mixer_fused_train_static_wgrad(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                                               ctypes.byref(sio), None, mf._stream()), "train_static_wgrad(NULL)")
        return mf._finish(out)
    act, h, idx, P, w2 = [np.array(a) for a in qh]
    if spoil is not None:
        rows = slice(spoil * T1 * J, (spoil + 1) * T1 * J)
        act[rows], h[rows] = np.nan, np.nan
    d_act, k0 = mf._inp(act)
    d_h, k1 = mf._inp(h)
    d_P, k2 = mf._inp(P)
    d_w2, k3 = mf._inp(w2)
    d_idx = torch.as_tensor(np.where((idx >= 0) & (idx < A), idx, -5).astype(np.int32) if idx32 else idx, device=DEV)
    out["ws1"] = mf._Guarded((int(lib.macjd_wgrad_slot_floats(H, H + A + 1, n_tiles)),), mf.OUT_MARGIN)
    out["ws2"] = mf._Guarded((int(lib.macjd_wgrad_slot_floats(1, H, n_tiles)),), mf.OUT_MARGIN)
    out["ln"] = mf._Guarded((n_tiles, 2, S), mf.OUT_MARGIN)
    wb = _native.MixerWgradBlock()
    wb.act_q, wb.act_ld, wb.h, wb.h_ld = d_act.data_ptr(), H, d_h.data_ptr(), H
    wb.idx, wb.idx_elem_size, wb.A, wb.P, wb.w2, wb.H = d_idx.data_ptr(), d_idx.element_size(), A, d_P.data_ptr(), d_w2.data_ptr(), H
    wb.ws1, wb.ws1_floats = out["ws1"].t.data_ptr(), out["ws1"].t.numel()
    wb.ws2, wb.ws2_floats = out["ws2"].t.data_ptr(), out["ws2"].t.numel()
    wb.ln_slots, wb.ln_floats = out["ln"].t.data_ptr(), out["ln"].t.numel()
    W1 = dev["pe"]["W1"]
    wb.W_first, wb.w_ld = W1.data_ptr(), W1.stride(0)
    if tweak is not None:
        tweak(wb)
        rc = lib.macjd_mixer_fused_train_static_wgrad(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                                      ctypes.byref(sio), ctypes.byref(wb), mf._stream())
        torch.cuda.synchronize()
        assert rc == 0 or all(bool(torch.isnan(g.buf).all()) for g in out.values()), "a refused call wrote something"
        return rc
    _native.check(lib.macjd_mixer_fused_train_static_wgrad(ctypes.byref(io), ctypes.byref(tio), ctypes.byref(td), tot_m.data_ptr(),
                                                           ctypes.byref(sio), ctypes.byref(wb), mf._stream()), "train_static_wgrad")
    return mf._finish(out)


def _slot_views(got, A, n_tiles):
    """(dW1 slots [n_tiles, 64, N1], db1 [n_tiles, 64], dw2 [n_tiles, 64], db2 [n_tiles], ln [n_tiles, 2, S])"""
    N1, Np1 = H + A + 1, 128
    ws1, ws2 = got["ws1"], got["ws2"]
    return (ws1[:n_tiles * 64 * Np1].view(n_tiles, 64, Np1)[:, :, :N1], ws1[n_tiles * 64 * Np1:].view(n_tiles, 64),
            ws2[:n_tiles * 64 * 64].view(n_tiles, 64, 64)[:, 0, :], ws2[n_tiles * 64 * 64:].view(n_tiles, 64)[:, 0], got["ln"])


def _reduce(dev, got, J, A, S, n_tiles):
    """The reduce launch alone on the seven problems; returns the gradients as float64 arrays."""
    from macjd_amd import _native
    lib = _native.load()
    shapes = {"W1": (mm.N1, S), "b1": (mm.N1,), "W2": (J * mm.EM, mm.HH), "b2": (J * mm.EM,), "Wf2": (mm.EM, mm.HH), "bf2": (mm.EM,),
              "wV2": (1, mm.EM), "bV2": (1,), "ln_w": (S,), "ln_b": (S,), "qW1": (H, H + A + 1), "qb1": (H,), "qw2": (1, H), "qb2": (1,)}
    o = {k: mf._Guarded(v, mf.OUT_MARGIN) for k, v in shapes.items()}
    act = got["act"]

    def rows(gout, inp, dW, db):
        io = _native.WgradIO()
        io.K, io.M, io.N, io.kind = n_tiles, gout.shape[1], inp.shape[1], _native.WGRAD_ROW_PRODUCTS
        io.gout, io.gout_ld, io.inp, io.inp_ld = gout.data_ptr(), gout.stride(0), inp.data_ptr(), inp.stride(0)
        io.dW, io.dw_ld, io.db = o[dW].t.data_ptr(), inp.shape[1], o[db].t.data_ptr()
        return io

    def ext(M, N, ws, dW, db):
        io = _native.WgradIO()
        io.K, io.M, io.N, io.kind, io.ext_chunks, io.workspace = 1, M, N, _native.WGRAD_EXT_SLOTS, n_tiles, ws.data_ptr()
        if dW is not None:
            io.dW, io.dw_ld, io.db = o[dW].t.data_ptr(), N, o[db].t.data_ptr()
        return io

    g_v = got["g_v"].view(n_tiles, 1)
    ios = [rows(got["gout1"], got["sn"], "W1", "b1"), ext(mm.N1, S, got["ln"], None, None),
           rows(got["g_w1raw"], act[:, :mm.HH], "W2", "b2"), rows(got["g_wfraw"], act[:, mm.HH:2 * mm.HH], "Wf2", "bf2"),
           rows(g_v, act[:, 2 * mm.HH:2 * mm.HH + mm.EM], "wV2", "bV2"),
           ext(H, H + A + 1, got["ws1"], "qW1", "qb1"), ext(1, H, got["ws2"], "qw2", "qb2")]
    arr = (_native.WgradIO * 7)(*ios)
    assert int(lib.macjd_linear_wgrad_many_norm_work_items(arr, 7, 1)) == 0
    n_partials = int(lib.macjd_linear_wgrad_many_norm_partials(arr, 7, 1))
    partials = mf._Guarded((n_partials,), mf.OUT_MARGIN)
    step = torch.tensor([2.0], device=DEV)
    nio = _native.WgradNormIO()
    nio.ln_problem, nio.partials_cap = 1, n_partials
    nio.dgamma, nio.dbeta, nio.partials, nio.step = o["ln_w"].t.data_ptr(), o["ln_b"].t.data_ptr(), partials.t.data_ptr(), step.data_ptr()
    _native.check(lib.macjd_linear_wgrad_many_norm(arr, 7, ctypes.byref(nio), mf._stream()), "macjd_linear_wgrad_many_norm")
    res = mf._finish(o)
    assert step.item() == 3.0 and partials.margins_intact()
    sq = sum(float((v.double() ** 2).sum()) for v in res.values())
    assert abs(float(partials.t.double().sum()) - sq) <= 1e-5 * sq
    return {k: v.detach().cpu().double().numpy() for k, v in res.items()}


@pytest.mark.parametrize("T1", [5, 16, 17, 33])
@pytest.mark.parametrize("J", [3, 2])
def test_training_launch_with_the_block_then_the_reduce_alone(J, T1):
    from macjd_amd import ops
    B, A = 2, ACTIONS[J]
    host, dev = _case(J, B, T1)
    S = dev["state"].shape[-1]
    assert S == mm.SHIPPED_S[J]
    qh = _qhead(J, A, B, T1)
    tot_m = ops.td_mask_sum(dev["filled"], T1 - 1)
    n_tiles = B * ms.tiles_per_episode(T1)
    what = f"J={J} T1={T1}"
    plain = _launch(dev, qh, J, A, B, T1, tot_m, block=False)
    got = _launch(dev, qh, J, A, B, T1, tot_m)
    again = _launch(dev, qh, J, A, B, T1, tot_m)
    # what the launch wrote before the block existed: bit for bit; two launches: bit for bit
    for k in plain:
        a, b = (plain[k][1:], got[k][1:]) if k == "tq" else (plain[k], got[k])
        assert torch.equal(a, b) and not bool(torch.isnan(b).any()), f"{what}: {k} differs from the launch without the block"
    slots, slots2 = _slot_views(got, A, n_tiles), _slot_views(again, A, n_tiles)
    for name, a, b in zip(("dW1", "db1", "dw2", "db2", "ln"), slots, slots2):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any()), f"{what}: slot {name}"
    # int32 indices: the same slots
    for a, b in zip(slots, _slot_views(_launch(dev, qh, J, A, B, T1, tot_m, idx32=True), A, n_tiles)):
        assert torch.equal(a, b), f"{what}: int32 indices"
    # a tile reads the Q-head rows of its own episode only
    tpe = n_tiles // B
    for other in range(B):
        mine = 1 - other
        spoiled = _slot_views(_launch(dev, qh, J, A, B, T1, tot_m, spoil=other), A, n_tiles)
        for name, a, b in zip(("dW1", "db1", "dw2", "db2", "ln"), slots, spoiled):
            assert torch.equal(a[mine * tpe:(mine + 1) * tpe], b[mine * tpe:(mine + 1) * tpe]), f"{what}: slot {name} read episode {other}"
    # ---- the gradients after the reduce against float64 of the same sums
    res = _reduce(dev, got, J, A, S, n_tiles)
    assert not any(np.isnan(v).any() for v in res.values())
    f64 = lambda t: t.detach().cpu().double().numpy()
    act_q, h, idx, P, w2 = qh
    n = B * T1 * J
    gq = f64(got["gq"]).reshape(n)
    g_hid32 = np.where(act_q > 0, (gq.astype(np.float32)[:, None] * w2[None, :]).astype(np.float32), np.float32(0))
    x = np.zeros((n, H + A + 1), dtype=np.float64)
    x[:, :H] = h
    ok = (idx >= 0) & (idx < A)
    x[np.nonzero(ok)[0], H + idx[ok]] = 1.0
    x[:, H + A] = P
    g_hid, a64 = g_hid32.astype(np.float64), act_q.astype(np.float64)
    worst = {}

    def check(name, ref, mag, terms):
        err = np.abs(res[name].reshape(ref.shape) - ref)
        bound = _gamma(terms + 2) * mag
        worst[name] = float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), f"{what}: {name} beyond gamma_({terms} + 2) sum|terms|: {worst[name]:.3f} of the bound"

    check("qW1", g_hid.T @ x, np.abs(g_hid).T @ np.abs(x), n)
    check("qb1", g_hid.sum(0), np.abs(g_hid).sum(0), n)
    check("qw2", gq @ a64, np.abs(gq) @ a64, n)
    check("qb2", gq.sum(keepdims=True), np.abs(gq).sum(keepdims=True), n)
    c = {k: f64(got[k]).reshape(n_tiles, -1) for k in st.COMPACT}
    act = c["act"]
    for w, b, g, inp in (("W1", "b1", c["gout1"], c["sn"]), ("W2", "b2", c["g_w1raw"], act[:, :mm.HH]),
                         ("Wf2", "bf2", c["g_wfraw"], act[:, mm.HH:2 * mm.HH]), ("wV2", "bV2", c["g_v"], act[:, 2 * mm.HH:2 * mm.HH + mm.EM])):
        check(w, g.T @ inp, np.abs(g).T @ np.abs(inp), n_tiles)
        check(b, g.sum(0), np.abs(g).sum(0), n_tiles)
    W1 = f64(dev["pe"]["W1"])
    u, u_abs = c["gout1"] @ W1, np.abs(c["gout1"]) @ np.abs(W1)
    check("ln_w", (c["xhat"] * u).sum(0), (np.abs(c["xhat"]) * u_abs).sum(0), mm.N1 * n_tiles)
    check("ln_b", u.sum(0), u_abs.sum(0), mm.N1 * n_tiles)
    print(f"{what}: worst error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert float(np.abs(res["qW1"]).max()) > 0 and float(np.abs(res["ln_w"]).max()) > 0


def test_host_checks_of_the_block():
    """MACJD_EINVAL for a workspace smaller than n_tiles slots, a NULL member, a bad stride, alignment or index size;
    MACJD_EUNSUPPORTED for sizes outside H = 64, 1 <= A <= 15.  A refused call launches nothing."""
    from macjd_amd import ops
    J, B, T1, A = 3, 2, 17, 9
    host, dev = _case(J, B, T1)
    qh = _qhead(J, A, B, T1)
    tot_m = ops.td_mask_sum(dev["filled"], T1 - 1)
    run = lambda tweak: _launch(dev, qh, J, A, B, T1, tot_m, tweak=tweak)

    def setter(name, value=None, delta=None):
        def f(wb):
            setattr(wb, name, value if delta is None else getattr(wb, name) + delta)
        return f

    for name in ("ws1_floats", "ws2_floats", "ln_floats"):
        assert run(setter(name, delta=-1)) == EINVAL, name
    for name in ("act_q", "h", "idx", "P", "w2", "ws1", "ws2", "ln_slots", "W_first"):
        assert run(setter(name, None)) == EINVAL, name
    for name, value in (("act_ld", 66), ("h_ld", 60), ("idx_elem_size", 2), ("w_ld", 45)):
        assert run(setter(name, value)) == EINVAL, name
    assert run(setter("h", delta=4)) == EINVAL and run(setter("act_q", delta=8)) == EINVAL
    for name, value in (("A", 16), ("A", 0), ("H", 128)):
        assert run(setter(name, value)) == EUNSUPPORTED, name
    assert run(lambda wb: None) == 0
