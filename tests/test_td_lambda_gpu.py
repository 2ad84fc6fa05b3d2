"""``macjd_td_lambda_loss`` (csrc/macjd_nets.hip, csrc/macjd_tdlambda.h) against the float64 model of its contract
(tests/td_lambda_model.py, proved in tests/test_td_lambda_cpu.py), through the C-ABI over the model's whole case table, then
``ops.td_lambda_loss`` and the ``td_lambda`` learner on the device.

Every output sits in a NaN slab between NaN margins with NaN gaps where a pitch exceeds the row (tests/nan_slab.py): all of
that must survive, every written value must be finite.  Tolerances: the model's (min(ceiling, 8 Y), at least one float32 ulp);
the exact cases bit for bit.  Each case prints its worst |got - model| / tolerance per output."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import nan_slab as ns
import td_lambda_model as tm
import update_tail_model as um
from test_actor_grad_cpu import learner_for, make_learner_batch, named_params
from test_nets_cpu import load

pytestmark = pytest.mark.gpu
DEV = ns.DEV
OK, EINVAL = 0, -1     # include/macjd.h
f32, f64 = np.float32, np.float64
IDS = [c.name for c in tm.CASES]


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def _bytes(values, sb, st):
    """uint8 [B, Tm1] at element strides (sb, st) inside a tensor of true bytes; -> (tensor, pointer)."""
    B, Tm1 = values.shape
    host = np.ones(64 + B * sb, np.uint8)
    host[32 + ns.offsets((B, Tm1), (sb, st))] = values
    t = torch.from_numpy(host).to(DEV)
    return t, t.data_ptr() + 32


class Launch:
    """The operands of one case laid out on the device (module docstring of the model: dense / sliced / strided), fresh NaN
    outputs per call."""

    def __init__(self, d, B, Tm1, gamma_, lam, layout):
        self.B, self.T, self.gamma, self.lam = B, Tm1, gamma_, lam
        T = Tm1
        y_sb, tq_sb, tq_off, r, t, f = {"dense": (T, T, 0, (T, 1), (T, 1), (T, 1)),
                                        "sliced": (T + 1, T + 1, 1, (T + 1, 1), (T + 1, 1), (T + 1, 1)),
                                        "strided": (T + 3, T + 1, 0, (2 * T + 3, 2), (3 * T + 2, 3), (2 * T + 5, 2))}[layout]
        self.y, _ = ns.strided(d["y"], (y_sb, 1))
        self.tq, _ = ns.strided(d["tq"], (tq_sb, 1), off=tq_off)
        self.reward, _ = ns.strided(d["reward"], r)
        self.term_t, self.term_p = _bytes(d["terminated"], *t)
        self.fill_t, self.fill_p = _bytes(d["filled"], *f)
        self.strides = (y_sb, tq_sb, r, t, f)
        self.inputs = [self.y, self.tq, self.reward]
        for s in self.inputs:
            s.ptr
        self.frozen = [s.t.clone() for s in self.inputs] + [self.term_t.clone(), self.fill_t.clone()]

    def td_io(self, _native, stats, gy, gy_sb, gy_cols, io=None):
        io = _native.TdLossIO() if io is None else io
        y_sb, tq_sb, r, t, f = self.strides
        io.B, io.Tm1, io.gamma = self.B, self.T, self.gamma
        io.y, io.tq, io.y_sb, io.tq_sb = self.y.ptr, self.tq.ptr, y_sb, tq_sb
        io.reward, (io.r_sb, io.r_st) = self.reward.ptr, r
        io.terminated, (io.t_sb, io.t_st) = self.term_p, t
        io.filled, (io.f_sb, io.f_st) = self.fill_p, f
        io.stats = stats.ptr
        if gy is not None:
            io.gy, io.gy_sb, io.gy_cols = gy.ptr, gy_sb, gy_cols
        return io

    def outputs(self, gy_extra):
        B, T = self.B, self.T
        cols = T + gy_extra
        o = dict(stats=ns.Slab(4), gy=ns.Slab(B * (cols + 2)), ret=ns.Slab(B * (T + 3)), cols=cols, gy_sb=cols + 2, ret_sb=T + 3)
        o["gy_off"], o["ret_off"] = ns.offsets((B, cols), (cols + 2, 1)), ns.offsets((B, T), (T + 3, 1))
        return o

    def lambda_io(self, _native, o, with_gy=True):
        io = _native.TdLambdaIO()
        self.td_io(_native, o["stats"], o["gy"] if with_gy else None, o["gy_sb"], o["cols"], io=io.td)
        if not with_gy:
            o["gy"].ptr
        io.lam, io.ret, io.ret_sb = self.lam, o["ret"].ptr, o["ret_sb"]
        return io

    def run(self, gy_extra=0, with_gy=True):
        _native, lib = _lib()
        o = self.outputs(gy_extra)
        with torch.cuda.device(DEV):
            rc = lib.macjd_td_lambda_loss(ctypes.byref(self.lambda_io(_native, o, with_gy)), ns.stream())
        torch.cuda.synchronize()
        assert rc == OK
        assert o["ret"].rest_intact(o["ret_off"])
        assert o["gy"].rest_intact(o["gy_off"] if with_gy else None)
        return dict(stats=o["stats"].read(), gy=o["gy"].read(o["gy_off"]), ret=o["ret"].read(o["ret_off"]))

    def inputs_untouched(self):
        now = [s.t for s in self.inputs] + [self.term_t, self.fill_t]
        return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(now, self.frozen))


def _ratio(key, got, value, tol):
    got = np.asarray(got, f64)
    assert np.isfinite(got).all(), key
    err = np.abs(got - value)
    assert not np.any(err > tol), (key, float(np.max(err - tol)), int(np.argmax(err - tol)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(tol > 0, err / tol, 0.0)))


def _for_case(case, d=None):
    d = d or tm.inputs(case.B, case.Tm1, case.mask)
    return Launch(d, case.B, case.Tm1, case.gamma, case.lam, case.layout)


@pytest.mark.parametrize("case", tm.CASES, ids=IDS)
def test_launch_against_the_model(case):
    """ret, gy and the four stats inside the model's tolerances (the exact cases bit for bit), the gy tail +0, unfilled steps
    zero, stats[3] exact; with gy == NULL stats[0..2] the same values, stats[3] and the gy slab untouched."""
    exp = tm.expectation(case)
    (stats, tol_s), (gy, tol_gy), (G, tol_g) = exp["stats"], exp["gy"], exp["G"]
    T = case.Tm1
    L = _for_case(case)
    out = L.run(case.gy_extra)
    worst = dict(stats=_ratio("stats", out["stats"], stats, tol_s), ret=_ratio("ret", out["ret"], G, tol_g),
                 gy=_ratio("gy", out["gy"], gy, tol_gy))
    print(case.name, {k: round(v, 3) for k, v in worst.items()})
    assert out["stats"][3] == stats[3]
    tail = out["gy"][:, T:]
    assert not tail.any() and not np.signbit(tail).any()
    assert not out["gy"][:, :T][tm.inputs(case.B, case.Tm1, case.mask)["filled"] == 0].any()
    if case.exact:
        assert np.array_equal(out["ret"].astype(f64), G)
        assert np.array_equal(out["gy"].view(np.uint32), exp["restated"][1].view(np.uint32))
    sums = L.run(case.gy_extra, with_gy=False)
    assert np.array_equal(sums["stats"][:3], out["stats"][:3]) and np.isnan(sums["stats"][3])
    assert np.array_equal(sums["ret"], out["ret"])
    assert L.inputs_untouched()


def _poisoned(d, which):
    """1e30 in reward and tq of every step behind one stop of each episode (``which``: the first, or the one nearest the
    middle); -> (inputs, front [B, Tm1] bool: the steps up to and including that stop)."""
    term, fill, cont = tm._stops(d["terminated"], d["filled"])
    B, T = cont.shape
    front = np.zeros((B, T), bool)
    for b in range(B):
        stops = np.flatnonzero(~cont[b])
        s = stops[0] if which == "first" else stops[np.argmin(np.abs(stops - T // 2))]
        front[b, :s + 1] = True
    p = dict(d)
    p["reward"], p["tq"] = np.where(front, d["reward"], f32(1e30)), np.where(front, d["tq"], f32(1e30))
    return p, front


@pytest.mark.parametrize("which", ["first", "middle"])
@pytest.mark.parametrize("case", [c for c in tm.CASES if c.lam > 0 and c.Tm1 >= 63 and c.mask != "all"][::2], ids=lambda c: c.name)
def test_nothing_behind_a_stop_leaks_forward(case, which):
    d = tm.inputs(case.B, case.Tm1, case.mask)
    p, front = _poisoned(d, which)
    assert front.any() and not front.all()
    clean, dirty = _for_case(case).run(), _for_case(case, p).run()
    for k in ("ret", "gy"):
        assert np.array_equal(clean[k].view(np.uint32)[front], dirty[k].view(np.uint32)[front]), k
    assert dirty["stats"][3] == clean["stats"][3]


@pytest.mark.parametrize("case", [c for c in tm.CASES if c.lam == 0] + [tm.CASES[9]._replace(lam=0.0)], ids=lambda c: c.name)
def test_lambda_zero_against_the_one_step_launch(case):
    """macjd_td_loss on the same buffers (not bit equal by contract: how a[t] is contracted is the compiler's).  At lambda = 0
    the float64 model IS update_tail_model.td_loss_model (proved in test_td_lambda_cpu.py), and the lambda launch is held to
    it at the model's own tolerance in test_launch_against_the_model (the lambda = 0 rows of the table) and again here
    through the sum below.  The one-step launch has no tolerance in this model: it is held to the same float64 values at
    the bound its own suite holds it to (update_tail_model.td_bounds, a derived ceiling), and the two launches to each other
    at the sum of the two — each side's own allowance, nothing added."""
    _native, lib = _lib()
    d = tm.inputs(case.B, case.Tm1, case.mask)
    L = _for_case(case)
    out = L.run(0)
    o = L.outputs(0)
    with torch.cuda.device(DEV):
        assert lib.macjd_td_loss(ctypes.byref(L.td_io(_native, o["stats"], o["gy"], o["gy_sb"], o["cols"])), ns.stream()) == OK
    torch.cuda.synchronize()
    one = dict(stats=o["stats"].read(), gy=o["gy"].read(o["gy_off"]))
    args = (d["y"], d["tq"], d["reward"], d["terminated"], d["filled"], case.gamma)
    e_stats, e_gy = um.td_bounds(*args)
    m_stats, m_gy = um.td_loss_model(*args)
    exp = tm.expectation(case)
    _ratio("one-step stats", one["stats"], m_stats, e_stats)
    _ratio("one-step gy", one["gy"], m_gy, e_gy)
    _ratio("stats", out["stats"], one["stats"].astype(f64), exp["stats"][1] + e_stats)
    _ratio("gy", out["gy"], one["gy"].astype(f64), exp["gy"][1][:, :case.Tm1] + e_gy)


def test_argument_errors_are_refused_before_any_launch():
    _native, lib = _lib()
    case = tm.CASES[1]
    L = _for_case(case)
    o = L.outputs(1)
    T = case.Tm1
    good = L.lambda_io(_native, o)

    def mutated(**kw):
        io = _native.TdLambdaIO()
        ctypes.memmove(ctypes.byref(io), ctypes.byref(good), ctypes.sizeof(io))
        for k, v in kw.items():
            setattr(io.td if k.startswith("td_") else io, k[3:] if k.startswith("td_") else k, v)
        return io

    bad = [("io=NULL", None)] + [(f"{k}=NULL", mutated(**{k: None})) for k in
                                 ("td_y", "td_tq", "td_reward", "td_terminated", "td_filled", "td_stats", "ret")]
    bad += [(k, mutated(**kw)) for k, kw in [
        ("B=0", dict(td_B=0)), ("B<0", dict(td_B=-3)), ("Tm1=0", dict(td_Tm1=0)), ("Tm1<0", dict(td_Tm1=-1)),
        ("y_sb<Tm1", dict(td_y_sb=T - 1)), ("tq_sb<Tm1", dict(td_tq_sb=T - 1)), ("gy_cols<Tm1", dict(td_gy_cols=T - 1)),
        ("gy_sb<gy_cols", dict(td_gy_sb=o["cols"] - 1)), ("ret_sb<Tm1", dict(ret_sb=T - 1)),
        ("lambda<0", dict(lam=-0.1)), ("lambda>1", dict(lam=1.5)), ("lambda=nan", dict(lam=float("nan"))),
        ("lambda=inf", dict(lam=float("inf")))]]
    with torch.cuda.device(DEV):
        for name, io in bad:
            assert lib.macjd_td_lambda_loss(ctypes.byref(io) if io is not None else None, ns.stream()) == EINVAL, name
        torch.cuda.synchronize()
        assert all(o[k].rest_intact(None) for k in ("stats", "gy", "ret")) and L.inputs_untouched()
        assert lib.macjd_td_lambda_loss(ctypes.byref(good), ns.stream()) == OK       # the unmutated call is a good one
    torch.cuda.synchronize()
    assert np.isfinite(o["ret"].read(o["ret_off"])).all()


def test_ops_on_the_device_value_backward_and_views():
    from macjd_amd import ops
    case = tm.CASES[9]                     # the learner's shape, ragged
    d = tm.inputs(case.B, case.Tm1, case.mask)
    B, T = case.B, case.Tm1
    exp = tm.expectation(case._replace(gy_extra=0))

    def full(a, dtype, at):               # [B, T + 1, 1] with the case's values at steps at .. at + T - 1
        x = torch.zeros((B, T + 1, 1), dtype=dtype)
        x[:, at:at + T, 0] = torch.as_tensor(a).to(dtype)
        return x.to(DEV)

    y_full = full(d["y"], torch.float32, 0).requires_grad_(True)
    tq_full = full(d["tq"], torch.float32, 1)
    r, term, fill = full(d["reward"], torch.float32, 0), full(d["terminated"], torch.bool, 0), full(d["filled"], torch.bool, 0)
    y, tq = y_full[:, :-1], tq_full[:, 1:]
    assert ops._unit_step_rows(y)[0].data_ptr() == y.data_ptr() and ops._unit_step_rows(tq)[0].data_ptr() == tq.data_ptr()
    loss, my, mg = ops.td_lambda_loss(y, tq, r[:, :-1], term[:, :-1], fill[:, :-1], case.gamma, case.lam)
    (3.0 * loss).backward()
    stats, tol_s = exp["stats"]
    _ratio("ops stats", [loss.item(), my.item(), mg.item()], stats[:3], tol_s[:3])
    grad = y_full.grad.squeeze(-1).cpu().numpy()
    gy, tol_gy = exp["gy"]
    _ratio("ops grad", grad[:, :T], 3.0 * gy, 3.0 * tol_gy + 2 * um.U * np.abs(3.0 * gy))
    assert not grad[:, T].any()
    G, tol_g = exp["G"]
    got = ops.td_lambda_returns(tq, r[:, :-1], term[:, :-1], fill[:, :-1], case.gamma, case.lam)
    assert got.shape == (B, T, 1)
    _ratio("ops returns", got.squeeze(-1).cpu().numpy(), G, tol_g)
    # a view whose steps are not adjacent takes the copy, and computes the same
    y2 = torch.stack([y.detach(), y.detach()], dim=2)[:, :, 1]
    again = ops.td_lambda_loss(y2, tq, r[:, :-1], term[:, :-1], fill[:, :-1], case.gamma, case.lam)
    assert again[0].item() == loss.item()


# --------------------------------------------------------------------------------------------- learner
TAG, B_, T_, SEED, LAM = "3j4r_h64", 4, 6, 3, 0.8
STAT_KEYS = ["loss", "grad_norm", "eval_qtot_avg", "target_qtot_avg"]


@pytest.fixture(scope="module")
def cpu_side():
    """The CPU float32 learner's gradients, train() statistics and stepped parameters: computed once."""
    g, d = load(TAG)
    batch = make_learner_batch(g, d, B_, T_, SEED)
    mac_g, learner_g, _ = learner_for(g, d, td_lambda=LAM)
    learner_g._forward_backward(copy.deepcopy(batch), T_)
    grads = {k: (None if p.grad is None else p.grad.numpy().copy()) for k, p in named_params(mac_g, learner_g).items()}
    mac, learner, _ = learner_for(g, d, td_lambda=LAM)
    stats = learner.train(copy.deepcopy(batch), {})
    params = {k: p.detach().numpy().copy() for k, p in named_params(mac, learner).items()}
    return g, d, batch, stats, grads, params


def test_learner_step_on_device_matches_the_cpu_side(cpu_side):
    g, d, batch, ref_stats, ref_grads, ref_params = cpu_side
    mac, learner, _ = learner_for(g, d, "cuda", td_lambda=LAM)
    assert next(mac.agent.parameters()).is_cuda and learner.td_lambda == LAM
    stats = learner.train(copy.deepcopy(batch), {})
    assert list(stats) == STAT_KEYS
    print({k: (stats[k], ref_stats[k]) for k in STAT_KEYS})
    np.testing.assert_allclose([stats[k] for k in STAT_KEYS], [ref_stats[k] for k in STAT_KEYS], rtol=1e-4, atol=1e-5)
    mac_g, learner_g, _ = learner_for(g, d, "cuda", td_lambda=LAM)        # the gradients before the clip scales them
    learner_g._forward_backward(copy.deepcopy(batch), T_)
    named_g = named_params(mac_g, learner_g)
    assert {k for k, p in named_g.items() if p.grad is None} == {k for k, v in ref_grads.items() if v is None}
    for k, ref in ref_grads.items():
        if ref is not None:
            np.testing.assert_allclose(named_g[k].grad.cpu().numpy(), ref, rtol=1e-3, atol=2e-5 * float(np.abs(ref).max()), err_msg=k)
    for k, p in named_params(mac, learner).items():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref_params[k], atol=5e-6, rtol=0, err_msg=k)


def test_graphs_are_refused_and_eager_updates_go_on(cpu_side):
    g, d, batch, *_ = cpu_side
    mac, learner, _ = learner_for(g, d, "cuda", td_lambda=LAM)
    with pytest.raises(RuntimeError, match="td_lambda"):
        learner.enable_graphs(None, 4)
    stats = learner.train(copy.deepcopy(batch), {})
    assert list(stats) == STAT_KEYS and all(np.isfinite(v) for v in stats.values())
