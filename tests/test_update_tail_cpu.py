"""tests/update_tail_model.py proved on the host: the float64 model of the TD loss, the LayerNorm parameter gradients and
clip + Adam against float64 torch (autograd, clip_grad_norm_, torch.optim.Adam); the float32 restatement of the same formulas
inside the model's own bounds for every case of tests/test_update_tail_gpu.py (the fairness check: the reference alone must
pass what the kernels are held to); the ctypes mirrors of the four structs against the header."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from _harness import REPO

sys.path.insert(0, os.path.dirname(__file__))
import update_tail_model as um  # noqa: E402
from test_nets_cpu import load, make_args, quiet  # noqa: E402

from macjd_amd import _native, ops  # noqa: E402

f32, f64 = np.float32, np.float64


def learner_flat_length():
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.core.qmix import QMixLearner
    g, d = load("3j4r_h64")
    args = make_args(d)
    with quiet():
        mac = BasicMAC(d["S"], args)
        learner = QMixLearner(mac, args)
    return um.flat_length(p.numel() for p in learner._trainable())


def _torch_step(shapes, p, g, m, v, step, w, max_norm):
    """One clip_grad_norm_ + torch.optim.Adam step in float64 from the given flat state -> param, grad, m, v, step, norm."""
    params, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        params.append(torch.nn.Parameter(torch.tensor(p[off:off + k].astype(f64)).reshape(s)))
        off += k
    opt = torch.optim.Adam(params, lr=w["lr"], betas=(w["b1"], w["b2"]), eps=w["eps"])
    off = 0
    for q in params:
        k = q.numel()
        opt.state[q] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor(m[off:off + k].astype(f64)).reshape(q.shape),
                        "exp_avg_sq": torch.tensor(v[off:off + k].astype(f64)).reshape(q.shape)}
        q.grad = torch.tensor(g[off:off + k].astype(f64)).reshape(q.shape)
        off += k
    norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    opt.step()
    flat = lambda ts: np.concatenate([t.detach().numpy().ravel() for t in ts])
    return (flat(params), flat([q.grad for q in params]), flat([opt.state[q]["exp_avg"] for q in params]),
            flat([opt.state[q]["exp_avg_sq"] for q in params]), float(opt.state[params[0]]["step"]), norm)


def test_clip_adam_model_is_clip_grad_norm_plus_torch_adam_in_float64():
    """12 consecutive steps from non-zero moments and a counter of 5 over one vector split into tensors, clipping active
    on some steps and inactive on others.  EVERY step calls clip_adam_model on the running float32 state and compares all
    its outputs, to 1e-12 relative, with one clip_grad_norm_ + torch.optim.Adam step in float64 from the same state on the
    same (float32-widened) hyper-parameters; the next state is the model's, rounded to float32 (the model takes float32
    operands).

    Then how far the float32 rounding of the hyper-parameters moves a step from the learner's nominal float64 ones, as a
    fraction of the GPU tolerance of that step (update_tail_model.adam_expectation), printed and asserted: parameters and
    m stay below it.  v does NOT: float32(0.999) moves 1 - b2 by 1.3e-5 of itself, and v by up to |delta b2| (v + g^2),
    several times the few-rounding bound of v (measured 5 .. 7 x) — which is why the model carries the float32 values of
    the struct and not the nominal ones; asserted for v is that formula, and that the parameters, which see v only through
    sqrt(v) / sqrt(1 - b2^t), stay inside their tolerance."""
    rng = np.random.default_rng(12)
    shapes = [(7, 11), (5,), (1, 13), (1,), (19, 3)]
    n = sum(int(np.prod(s)) for s in shapes)
    h = um.HYPER
    w = {k: float(f32(v)) for k, v in h.items()}
    p = rng.standard_normal(n).astype(f32)
    m, v = (0.3 * rng.standard_normal(n)).astype(f32), (0.2 * rng.random(n)).astype(f32)
    step, max_norm = 5, float(f32(6.0))
    active, worst = [], {}
    for it in range(12):
        grad = (rng.standard_normal(n) * (0.2 if it % 3 == 0 else 1.0)).astype(f32)
        got = um.clip_adam_model(p, grad, m, v, step, h["lr"], h["b1"], h["b2"], h["eps"], max_norm)
        ref = _torch_step(shapes, p, grad, m, v, step, w, max_norm)
        for name, a, b in zip(("param", "grad", "m", "v", "step", "norm"), got, ref):
            assert np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 1e-12 * np.abs(b) + 1e-300), (it, name)
        assert got[4] == step + 1
        active.append(bool(np.any(got[1] != grad.astype(f64))))
        # the same step on the nominal float64 hyper-parameters, against the GPU tolerance of this step
        d = dict(param=p, grad=grad, m=m, v=v, step=step, max_norm=f32(max_norm), **h)
        rel = um.norm_rel_bound(float((grad.astype(f64) ** 2).sum()), um.sqnorm_chain(n, um.blocks_of(n)))
        exp = um.adam_expectation(d, rel, um.restated_norm(grad))
        nom = _torch_step(shapes, p, grad, m, v, step, h, max_norm)
        for name, a, b in zip(("param", "grad", "m", "v"), nom, got):
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.abs(a - b) / exp[name][1]
            worst[name] = max(worst.get(name, 0.0), float(np.nanmax(np.where(exp[name][1] > 0, r, 0.0))))
        G = got[1]
        assert np.all(np.abs(nom[3] - got[3]) <= abs(h["b2"] - w["b2"]) * (v + G * G) * (1 + 1e-6))
        p, m, v, step = got[0].astype(f32), got[2].astype(f32), got[3].astype(f32), step + 1
    assert any(active) and not all(active) and step == 17
    print("float32 hyper-parameters against the nominal ones, worst shift / GPU tolerance:", {k: round(x, 3) for k, x in worst.items()})
    assert worst["param"] < 1.0 and worst["grad"] < 1.0 and worst["m"] < 1.0
    assert worst["v"] > 1.0     # (documented above: the reason the model widens the struct's float32 values)


@pytest.mark.parametrize("mask", um.TD_MASKS)
@pytest.mark.parametrize("B,Tm1", [(3, 2), (7, 341), (1, 1025)])
def test_td_loss_model_is_the_reference_in_float64(B, Tm1, mask):
    d = um.td_inputs(B, Tm1, mask)
    stats, gy = um.td_loss_model(d["y"], d["tq"], d["reward"], d["terminated"], d["filled"], um.TD_GAMMA, gy_cols=Tm1 + 2)
    t = lambda a: torch.tensor(np.asarray(a).astype(f64)).reshape(B, Tm1, 1)
    y = t(d["y"]).requires_grad_(True)
    term, fill = torch.tensor(d["terminated"].astype(bool)).reshape(B, Tm1, 1), torch.tensor(d["filled"].astype(bool)).reshape(B, Tm1, 1)
    loss, my, mt = ops.td_loss_reference(y, t(d["tq"]), t(d["reward"]), term.double(), fill.double(), float(f32(um.TD_GAMMA)))
    assert loss.dtype == torch.float64
    loss.backward()
    ref = np.array([float(loss.detach()), float(my), float(mt.detach()), float(d["filled"].sum())])
    assert np.all(np.abs(stats - ref) <= 1e-12 * np.abs(ref) + 1e-300)
    g = y.grad.numpy().reshape(B, Tm1)
    assert np.all(np.abs(gy[:, :Tm1] - g) <= 1e-12 * np.abs(g) + 1e-300)
    assert np.array_equal(gy[:, Tm1:], np.zeros((B, 2))) and not np.signbit(gy[:, Tm1:]).any()
    assert d["terminated"].any() or B * Tm1 == 1


@pytest.mark.parametrize("C,K", [(1, 1), (255, 46), (257, 5)])
def test_ln_param_model_is_autograd_through_layernorm_and_linear(C, K):
    """dgamma / dbeta from W, G = gout^T xhat and gb = column sums of gout == float64 autograd for the LayerNorm's weight
    and bias through LayerNorm -> Linear."""
    rng = np.random.default_rng(100 * C + K)
    R = 9
    x = torch.tensor(rng.standard_normal((R, K)) + (1.0 if K == 1 else 0.0))
    ln = torch.nn.LayerNorm(K).double()
    lin = torch.nn.Linear(K, C).double()
    with torch.no_grad():
        ln.weight.copy_(torch.tensor(rng.standard_normal(K)))
        ln.bias.copy_(torch.tensor(rng.standard_normal(K)))
    gout = torch.tensor(rng.standard_normal((R, C)))
    (lin(ln(x)) * gout).sum().backward()
    xhat = ((ln(x) - ln.bias) / ln.weight).detach() if K > 1 else torch.zeros(R, K, dtype=torch.float64)
    # float32 operands for the model: compare at the float32 rounding of W, G, gb by feeding the same rounded values
    W = lin.weight.detach().numpy().astype(f32)
    G = (gout.T @ xhat).numpy().astype(f32)
    gb = gout.sum(0).numpy().astype(f32)
    dg, db = um.ln_param_model(W, G, gb)
    dg_ref = (W.astype(f64) * G.astype(f64)).sum(0)
    assert np.allclose(dg, dg_ref, rtol=1e-15, atol=0)
    # against autograd: the float32 rounding of the operands moves each product by <= 2u (3u with the cross term)
    mag_g = (np.abs(lin.weight.detach().numpy()) * np.abs((gout.T @ xhat).numpy())).sum(0)
    mag_b = np.abs(gout.sum(0).numpy()) @ np.abs(lin.weight.detach().numpy())
    assert np.all(np.abs(dg - ln.weight.grad.numpy()) <= 3 * um.U * mag_g + 1e-12 * (1 + mag_g))
    assert np.all(np.abs(db - ln.bias.grad.numpy()) <= 3 * um.U * mag_b + 1e-12 * (1 + mag_b))


def _inside(name, got, value, bound):
    err = np.abs(np.asarray(got, f64) - value)
    ok = err <= bound
    assert np.all(ok), (name, float(np.max(err - bound)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))


def test_float32_restatement_of_the_optimiser_stays_inside_the_bounds():
    """Every length and state of the GPU file (the learner's own length included): the float32 restatement's norm, clipped
    gradient and moments within the derived bounds, its parameters within the ceiling — for the two-launch step and for
    the one-launch step behind host-made partials, each with its own summation order and chain."""
    worst = {}
    lengths = um.LENGTHS + [learner_flat_length()]
    assert lengths[-1] > 257 and lengths[-1] % 4 == 0
    for n in lengths:
        for st in um.STATES:
            d = um.adam_inputs(n, st)
            r_norm = um.restated_norm(d["grad"])
            exp = um.plain_expectation(d)
            p, g, m, v, t, norm = um.clip_adam_f32(d["param"], d["grad"], d["m"], d["v"], d["step"], d["lr"], d["b1"], d["b2"],
                                                   d["eps"], d["max_norm"], r_norm)
            assert t == exp["step"] and all(np.isfinite(a).all() for a in (p, g, m, v))
            got = {"norm": norm, "grad": g, "m": m, "v": v}
            for k in got:
                worst[k] = max(worst.get(k, 0.0), _inside((n, st.name, k), got[k], *exp[k]))
            worst["param"] = max(worst.get("param", 0.0), _inside((n, st.name, "param"), p, exp["param"][0], exp["ceiling"]))
            # the one-launch step behind host-made partials (chunk_partials): 256 lanes over them, its own chain
            parts = um.chunk_partials(d["grad"])
            exp_r = um.reduced_expectation(d, parts)
            norm_r = um.reduced_norm_f32(parts)
            p_r, g_r, m_r, v_r, _, _ = um.clip_adam_f32(d["param"], d["grad"], d["m"], d["v"], d["step"], d["lr"], d["b1"], d["b2"],
                                                        d["eps"], d["max_norm"], norm_r)
            for k, a in (("norm", norm_r), ("grad", g_r), ("m", m_r), ("v", v_r)):
                worst["reduced " + k] = max(worst.get("reduced " + k, 0.0), _inside((n, st.name, "reduced", k), a, *exp_r[k]))
            worst["reduced param"] = max(worst.get("reduced param", 0.0),
                                         _inside((n, st.name, "reduced param"), p_r, exp_r["param"][0], exp_r["ceiling"]))
            for nrm, gg in ((norm, g), (norm_r, g_r)):
                if st.clip == "edge":
                    assert nrm == f32(np.sqrt(float((d["grad"].astype(f64) ** 2).sum())))
                if st.grad == "zero":
                    assert nrm == 0 and not gg.any() and not np.signbit(gg).any()
    _ln_fair(um.ln_case_at_length(lengths[-1]))
    print("float32 restatement, worst error / bound:", {k: round(x, 3) for k, x in worst.items()})


@pytest.mark.parametrize("case", um.LN_CASES + [um.ln_case_at_length(n) for n in um.LENGTHS[1:]], ids=lambda c: c.name)
def test_float32_restatement_of_the_layernorm_step_stays_inside_the_bounds(case):
    _ln_fair(case)


def _ln_fair(case):
    for clip in (False, True):
        d = um.ln_inputs(case, clip)
        exp = um.ln_expectation(case, d)
        dg, db = um.ln_param_f32(d["W"], d["G"], d["gb"])
        _inside("dgamma", dg, *exp["dgamma"])
        _inside("dbeta", db, *exp["dbeta"])
        g = np.nan_to_num(d["grad"]).astype(f32)
        g[case.gamma_off:case.gamma_off + case.K], g[case.beta_off:case.beta_off + case.K] = dg, db
        r_norm = um.restated_norm(np.nan_to_num(d["grad"]), extra=(dg.astype(f64) ** 2 + db.astype(f64) ** 2).astype(f32))
        p, gc, m, v, t, norm = um.clip_adam_f32(d["param"], g, d["m"], d["v"], d["step"], d["lr"], d["b1"], d["b2"], d["eps"],
                                                d["max_norm"], r_norm)
        for k, a in (("norm", norm), ("grad", gc), ("m", m), ("v", v)):
            _inside((case.name, k), a, *exp[k])
        _inside((case.name, "param"), p, exp["param"][0], exp["ceiling"])
        # the LayerNorm gradients carry at least a quarter of the squared norm: without them the norm bound fails
        without = np.sqrt(float((np.nan_to_num(d["grad"]).astype(f64) ** 2).sum()))
        assert abs(without - exp["norm"][0]) > 1000 * exp["norm"][1]


@pytest.mark.parametrize("mask", um.TD_MASKS)
@pytest.mark.parametrize("B,Tm1", um.TD_SHAPES)
def test_float32_restatement_of_the_td_loss_stays_inside_the_bounds(B, Tm1, mask):
    d = um.td_inputs(B, Tm1, mask)
    args = (d["y"], d["tq"], d["reward"], d["terminated"], d["filled"], um.TD_GAMMA)
    stats, gy = um.td_loss_model(*args)
    e_stats, e_gy = um.td_bounds(*args)
    s32, g32 = um.td_loss_f32(*args)
    _inside("stats", s32, stats, e_stats)
    _inside("gy", g32, gy, e_gy)
    assert s32[3] == d["filled"].sum()


def test_struct_mirrors_match_the_header():
    """Size and every field offset of the four ctypes mirrors against what a C compiler makes of include/macjd_nets.h."""
    structs = [("macjd_adam_io", _native.AdamIO), ("macjd_tdloss_io", _native.TdLossIO), ("macjd_lnparam_io", _native.LnParamIO),
               ("macjd_sampler_io", _native.SamplerIO)]
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    items, expect = [], []
    for name, cls in structs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), plain, flags=re.S).group(1)
        assert re.findall(r"(\w+)\s*[;,]", body) == [f[0] for f in cls._fields_], name
        items.append("sizeof(%s)" % name)
        expect.append(ctypes.sizeof(cls))
        for f in cls._fields_:
            items.append("offsetof(%s, %s)" % (name, f[0]))
            expect.append(getattr(cls, f[0]).offset)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\nint main(){printf("' + "%zu " * len(items) + '\\n"'
           + "".join(", " + i for i in items) + ");return 0;}\n")
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "t.c"), "w") as f:
            f.write(src)
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(tmp, "t"), os.path.join(tmp, "t.c")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(tmp, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == expect
