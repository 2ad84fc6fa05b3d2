"""``macjd_gru_sequence`` (all four kernels behind it: the unit-split scan with streamed and with static gi, the K-split
scan at H = 64 and H = 128; the in-kernel input transform and actor chain of ``scan_prologue``) and ``macjd_gru_gates``
(csrc/macjd_nets.hip) against the float64 model of their contract (tests/gru_scan_model.py, proved on the CPU in
tests/test_gru_scan_cpu.py), through the C-ABI, at the smallest shapes at which these kernels can go wrong: T = 1 .. 7
(both remainders of the unroll by three, the first ring slots, the t + 2 clamp) and the learner's T = 101; sequences
(1,1), (3,2), (2,3) with different data per sequence and step; one and two nets with different weights, h0 NULL / set per
net, h0 batch strides 0, J H, (T+1) J H, J H + 4; static gi; gate inputs of +-30, +-100, +-1e4 and h0 entries of exactly
0 and +-1; observation widths 1, 64, 65, 129, 256 out of a padded ring through NULL / duplicated / first-and-last row
indices; actor widths (63,5), (1,1), (65,9), (129,17), (256,64) with p_out on either net or both; every refusal; the gates
at N in {1, 63, 64, 65} x H in {4, 12, 64, 128} on the vector path, on the scalar path entered by a base 4 bytes off 16
and by an odd row stride, with a broadcast gi row, in place, with and without the second destination, past the grid cap.

Every output sits in a NaN-filled allocation between NaN margins; padded inputs carry NaN gaps; what a launch may not
write must survive bit for bit, and what it writes must be finite.  Tolerance: gru_scan_model's rule,
min(cap, max(floor, 8 x the float32 restatement's deviation)), floor 12.5 ulp = 1.49e-6 (derived there), caps 1e-5 for h
and 1e-6 + 1e-5 |P|.  Each test prints its worst |got - model| / tolerance; largest on MI355X over this file (all <= 1):
    scan h              unit-split 0.142   K-split H = 64 0.163   K-split H = 128 0.168   (each at T = 101 or just below)
    from observations   h 0.086 / 0.088 / 0.100   P 0.157 / 0.149 / 0.130   (same order of forms)
    gates               vector path 0.144   scalar path 0.143   past the grid cap 0.131
The float32 restatement's own largest deviation, as a share of the cap (tests/test_gru_scan_cpu.py prints it): scan 2.5 %,
from observations h 1.5 % and P 1.0 %, gates 3.1 % — so the floor decides most tolerances (1.49e-6 .. 2.5e-6 for h).
The file runs in about 5 s.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import gru_scan_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, EUNSUPPORTED = 0, -1, -4     # include/macjd.h
f32, f64 = np.float32, np.float64
MARGIN = 64
_WORST = {}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


class Slab:
    """``n`` float32 elements behind ``off`` extra elements, in a NaN-filled allocation with NaN margins.  ``put`` writes
    values at element offsets (inputs; everything else stays NaN: gaps of a padded layout); after the launch ``read``
    returns the values at offsets and ``rest_intact`` tells whether every other element still holds its NaN bits."""

    def __init__(self, n, off=0):
        self.host = np.full(2 * MARGIN + off + n, np.nan, f32)
        self.base, self.n = MARGIN + off, n
        self.t = None

    def put(self, offsets, values):
        self.host[self.base + np.asarray(offsets).reshape(-1)] = np.asarray(values, f32).reshape(-1)
        return self

    @property
    def ptr(self):
        if self.t is None:
            self.t = torch.from_numpy(self.host).to(DEV)
        return self.t.data_ptr() + 4 * self.base

    def read(self, offsets=None):
        got = self.t.cpu().numpy()
        if offsets is None:
            return got[self.base:self.base + self.n].astype(f64)
        return got[self.base + np.asarray(offsets).reshape(-1)].astype(f64)

    def rest_intact(self, offsets=None):
        got = self.t.cpu().numpy().view(np.uint32)
        keep = np.ones(got.size, bool)
        if isinstance(offsets, str):      # "all": the n elements themselves were written
            keep[self.base:self.base + self.n] = False
        elif offsets is not None:
            keep[self.base + np.asarray(offsets).reshape(-1)] = False
        return bool(np.array_equal(got[keep], self.host.view(np.uint32)[keep]))


def dense(values, off=0):
    v = np.asarray(values, f32)
    s = Slab(v.size, off)
    s.host[s.base:s.base + v.size] = v.reshape(-1)
    return s


def strided(values, strides, off=0):
    """values [d0, d1, ...] laid out with the given element strides -> (Slab, element offsets of every value)."""
    v = np.asarray(values, f32)
    o = np.zeros(v.shape, np.int64)
    for ax, s in enumerate(strides):
        shape = [1] * v.ndim
        shape[ax] = v.shape[ax]
        o = o + (np.arange(v.shape[ax]) * s).reshape(shape)
    return Slab(int(o.max()) + 1, off).put(o, v), o


def _ratio(key, got, model, tol):
    got = np.asarray(got, f64).reshape(np.shape(model))
    assert np.isfinite(got).all(), key
    err = np.abs(got - model)
    assert np.all(err <= tol), (key, float(np.max(err / tol)), float(err.max()))
    r = float(np.max(err / tol)) if err.size else 0.0
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    return r


@pytest.fixture
def scan_form(monkeypatch):
    """Selects the kernel form for H = 64 (MACJD_GRU_SCAN, read by the library on reload) and restores the default."""
    _native, _ = _lib()

    def select(form):
        if form == "ksplit":
            monkeypatch.setenv("MACJD_GRU_SCAN", "ksplit")
        else:
            monkeypatch.delenv("MACJD_GRU_SCAN", raising=False)
        _native.reload_options()
    yield select
    monkeypatch.undo()
    _native.reload_options()


def _launch(lib, io):
    rc = lib.macjd_gru_sequence(ctypes.byref(io), _stream())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------ the recurrence (gi supplied)
def _scan_io(_native, case, data):
    form, H, B, J, T, static, h0s, sat = case
    io = _native.GruIO()
    io.n_nets, io.B, io.T, io.J, io.H, io.reserved = len(h0s), B, T, J, H, 1 if static else 0
    bufs = []
    for k, (spec, d) in enumerate(zip(h0s, data)):
        b = dict(gi=dense(d["gi"]), w=dense(d["w_hh"]), b=dense(d["b_hh"], off=1), out=Slab(B * T * J * H))
        io.gi[k], io.w_hh[k], io.b_hh[k], io.h_out[k] = b["gi"].ptr, b["w"].ptr, b["b"].ptr, b["out"].ptr
        if spec is not None:
            b["h0"], _ = strided(d["h0"], (gm.h0_stride(spec, T, J, H), H, 1), off=1)
            io.h0[k] = b["h0"].ptr
            io.h0_sb[k] = 0 if spec == "0" else gm.h0_stride(spec, T, J, H)
        bufs.append(b)
    return io, bufs


@pytest.mark.parametrize("form,H", gm.FORMS)
def test_scan_against_the_model(form, H, scan_form):
    _native, lib = _lib()
    scan_form(form)
    key = f"scan h {form}{H}"
    for case in [c for c in gm.scan_cases() if c[0] == form and c[1] == H]:
        io, bufs = _scan_io(_native, case, gm.scan_case_data(case))
        assert _launch(lib, io) == OK, case
        for b, (model, restate) in zip(bufs, gm.scan_case_expect(case)):
            tol, _ = gm.tolerance("h", model, restate)
            r = _ratio(key, b["out"].read(), model, tol)
            assert b["out"].rest_intact("all"), case
            assert all(b[k].rest_intact() for k in b if k != "out"), case     # inputs are not written
        print(case, "|got - model| / tol", round(r, 3))
    print(key, "worst", round(_WORST[key], 3))


@pytest.mark.parametrize("form,H", gm.FORMS)
def test_scan_of_nothing_writes_nothing(form, H, scan_form):
    _native, lib = _lib()
    scan_form(form)
    case = next(c for c in gm.scan_cases() if c[0] == form and c[1] == H and c[4] == 3)
    for B, T in ((0, 3), (case[2], 0), (0, 0)):
        io, bufs = _scan_io(_native, case, gm.scan_case_data(case))
        io.B, io.T = B, T
        assert _launch(lib, io) == OK
        assert all(b[k].rest_intact() for b in bufs for k in b)


def test_wrapper_materialises_an_initial_state_expanded_over_the_batch():
    """ops.gru_sequence_multi with h0 = row.expand(B, J, H) (stride 0 over the batch): every batch entry starts from the
    same block; the kernel's h0_sb = 0 means "contiguous", so the wrapper hands over a materialised copy."""
    from macjd_amd import ops
    rng = gm._rng("expand")
    B, T, J, H = 3, 4, 2, 64
    gi = rng.standard_normal((B, T, J, 3 * H)).astype(f32)
    w = gm.recurrent_weights(rng, H)
    row = (0.5 * rng.standard_normal((1, J, H))).astype(f32)
    h0 = torch.tensor(row).to(DEV).expand(B, J, H)
    assert h0.stride(0) == 0
    got = ops.gru_sequence_multi([torch.tensor(gi).to(DEV)], [torch.tensor(w["w_hh"]).to(DEV)],
                                 [torch.tensor(w["b_hh"]).to(DEV)], [h0])[0]
    full = np.broadcast_to(row, (B, J, H))
    model, restate = gm.gru_scan(gi, w["w_hh"], w["b_hh"], full, T), gm.gru_scan(gi, w["w_hh"], w["b_hh"], full, T, dt=f32)
    _ratio("scan h wrapper", got.cpu().numpy(), model, gm.tolerance("h", model, restate)[0])


# ------------------------------------------------------------------------------------------ in-kernel transform and actor
def _obs_io(_native, case, d):
    form, H, S, Ah, A, B, J, T, ps, kind, dead = case
    io = _native.GruIO()
    io.n_nets, io.B, io.T, io.J, io.H = len(ps), B, T, J, H
    sj = S + 3
    sb = (T + 1) * J * sj + 5
    obs, _ = strided(d["obs"], (sb, J * sj, sj, 1), off=1)
    io.obs, io.obs_sb, io.obs_sj, io.S = obs.ptr, sb, sj, S
    keep = dict(obs=obs)
    if d["index"] is not None:
        keep["index"] = torch.tensor([-1] + list(d["index"]) + [-1], dtype=torch.int64, device=DEV)
        io.obs_index = keep["index"].data_ptr() + 8
    io.Ah, io.A = Ah, A
    outs = []
    for k, (w, p) in enumerate(zip(d["nets"], ps)):
        ins = {n: dense(w[n]) for n in ("w_hh", "b_hh", "fc1_w", "fc1_b", "w_ih", "b_ih")}
        io.w_hh[k], io.b_hh[k], io.fc1_w[k], io.fc1_b[k], io.w_ih[k], io.b_ih[k] = (
            ins[n].ptr for n in ("w_hh", "b_hh", "fc1_w", "fc1_b", "w_ih", "b_ih"))
        for l, (ww, bb) in enumerate(w["actor"]):     # the layers are handed over whether or not the net carries p_out
            ins[f"aw{l}"], ins[f"ab{l}"] = dense(ww, off=l), dense(bb, off=1)
            io.act_w[k][l], io.act_b[k][l] = ins[f"aw{l}"].ptr, ins[f"ab{l}"].ptr
        o = dict(h=Slab(B * T * J * H), p=Slab(B * J * A, off=1) if p else None, ins=ins)
        io.h_out[k] = o["h"].ptr
        if p:
            io.p_out[k] = o["p"].ptr
        outs.append(o)
    return io, outs, keep


@pytest.mark.parametrize("form,H", gm.FORMS)
def test_scan_from_observations_against_the_model(form, H, scan_form):
    _native, lib = _lib()
    scan_form(form)
    kh, kp = f"obs h {form}{H}", f"obs P {form}{H}"
    for case in [c for c in gm.obs_cases() if c[0] == form and c[1] == H]:
        d = gm.obs_case_data(case)
        io, outs, keep = _obs_io(_native, case, d)
        assert _launch(lib, io) == OK, case
        for o, ((h64, h32), (p64, p32)) in zip(outs, gm.obs_case_expect(case)):
            rh = _ratio(kh, o["h"].read(), h64, gm.tolerance("h", h64, h32)[0])
            assert o["h"].rest_intact("all"), case
            rp = None
            if o["p"] is not None:
                rp = _ratio(kp, o["p"].read(), p64, gm.tolerance("p", p64, p32)[0])
                assert o["p"].rest_intact("all"), case
            assert all(s.rest_intact() for s in o["ins"].values()), case
            print(case, "h", round(rh, 3), "P", None if rp is None else round(rp, 3))
        assert keep["obs"].rest_intact()
        if "index" in keep:
            assert keep["index"].cpu().tolist() == [-1] + list(d["index"]) + [-1]
    print(kh, round(_WORST[kh], 3), kp, round(_WORST[kp], 3))


def _valid_obs_io(_native):
    case = next(c for c in gm.obs_cases() if c[0] == "units" and c[8] == (True, True) and not c[10])
    d = gm.obs_case_data(case)
    return (case, d) + _obs_io(_native, case, d)


def _refused(lib, io, outs, rc_want, what):
    assert lib.macjd_gru_sequence(ctypes.byref(io), _stream()) == rc_want, what
    torch.cuda.synchronize()
    for o in outs:
        assert o["h"].rest_intact() and (o["p"] is None or o["p"].rest_intact()), what


def test_scan_refusals_leave_the_outputs_alone():
    _native, lib = _lib()
    assert lib.macjd_gru_sequence(None, _stream()) == EINVAL

    def attempt(change, rc=EINVAL):
        case, d, io, outs, keep = _valid_obs_io(_native)
        what = change(io)
        _refused(lib, io, outs, rc, what)

    def setter(name, value):
        def f(io):
            setattr(io, name, value)
            return (name, value)
        return f

    def null(name, k, l=None):
        def f(io):
            if l is None:
                getattr(io, name)[k] = None
            else:
                getattr(io, name)[k][l] = None
            return (name, k, l)
        return f

    attempt(setter("H", 32), EUNSUPPORTED)
    for name, value in (("n_nets", 0), ("n_nets", 3), ("J", 0), ("B", -1), ("T", -1), ("S", 0), ("S", 257), ("Ah", 257),
                        ("Ah", 0), ("A", 65), ("A", 0)):
        attempt(setter(name, value))
    for k in (0, 1):
        for name in ("w_hh", "b_hh", "h_out", "fc1_w", "fc1_b", "w_ih", "b_ih"):
            attempt(null(name, k))
        for l in range(3):
            attempt(null("act_w", k, l))
            attempt(null("act_b", k, l))

    def misaligned(io):    # w_hh rows are read as float4: refused, never launched
        io.w_hh[1] = io.w_hh[1] + 4
        return "w_hh + 4 bytes"
    attempt(misaligned)

    # without obs: gi is required
    case = next(c for c in gm.scan_cases() if c[0] == "units" and len(c[6]) == 2 and c[4] == 4)
    for k in (0, 1):
        io, bufs = _scan_io(_native, case, gm.scan_case_data(case))
        io.gi[k] = None
        assert lib.macjd_gru_sequence(ctypes.byref(io), _stream()) == EINVAL
        io, bufs = _scan_io(_native, case, gm.scan_case_data(case))
        io.w_hh[k] = io.w_hh[k] + 8
        assert lib.macjd_gru_sequence(ctypes.byref(io), _stream()) == EINVAL
        torch.cuda.synchronize()
        assert all(b["out"].rest_intact() for b in bufs)


# ------------------------------------------------------------------------------------------ macjd_gru_gates
def _gates_io(_native, d, variant, alias, second):
    N, H = d["gh"].shape[0], d["h"].shape[1]
    off = 1 if variant == "base4" else 0            # 4 bytes off a 16-byte boundary
    pad = 3 if variant == "oddld" else (4 if variant == "vector" else 0)
    ld3, ld1 = 3 * H + pad, H + pad
    io = _native.GruGatesIO()
    io.n_rows, io.H = N, H
    s = {}
    if variant == "bcast":
        s["gi"] = dense(d["gi"])
        io.gi_ld = 0
    else:
        s["gi"], _ = strided(d["gi"], (ld3, 1), off=off)
        io.gi_ld = ld3
    s["gh"], _ = strided(d["gh"], (ld3, 1), off=off)
    s["h"], ho = strided(d["h"], (ld1, 1), off=off)
    io.gi, io.gh, io.gh_ld, io.h, io.h_ld = s["gi"].ptr, s["gh"].ptr, ld3, s["h"].ptr, ld1
    if alias:
        s["out"], oo = s["h"], ho
        io.ho_ld = ld1
    else:
        oo = ho + 0
        s["out"] = Slab(int(oo.max()) + 1, off=off)
        io.ho_ld = ld1
    io.h_out = s["out"].ptr
    o2 = None
    if second:
        ld2 = H + (8 if variant != "oddld" else 5)
        o2 = (np.arange(N) * ld2)[:, None] + np.arange(H)[None, :]
        s["out2"] = Slab(int(o2.max()) + 1, off=off)
        io.h_out2, io.ho2_ld = s["out2"].ptr, ld2
    return io, s, oo, o2


def _check_gates(key, lib, io, s, oo, o2, model, tol, alias):
    assert lib.macjd_gru_gates(ctypes.byref(io), _stream()) == OK
    torch.cuda.synchronize()
    r = _ratio(key, s["out"].read(oo), model, tol)
    assert s["out"].rest_intact(oo)
    if o2 is not None:
        assert np.array_equal(s["out2"].read(o2), s["out"].read(oo)) and s["out2"].rest_intact(o2)
    for k in ("gi", "gh") + (() if alias else ("h",)):
        assert s[k].rest_intact(), k
    return r


@pytest.mark.parametrize("H", gm.GATE_HS)
def test_gates_against_the_model(H):
    _native, lib = _lib()
    for iN, N in enumerate(gm.GATE_NS):
        for iv, variant in enumerate(gm.GATE_VARIANTS):
            d = gm.gates_case_data(N, H, variant)
            model, restate = gm.gates_expect(d)
            tol, _ = gm.tolerance("h", model, restate)
            for alias, second in (((iN + iv) % 2 == 0, iv % 2 == 0), ((iN + iv) % 2 == 1, iv % 2 == 1)):
                io, s, oo, o2 = _gates_io(_native, d, variant, alias, second)
                vec = all(p % 16 == 0 for p in (io.gi, io.gh, io.h, io.h_out, io.h_out2 or 0)) and \
                    all(l % 4 == 0 for l in (io.gi_ld, io.gh_ld, io.h_ld, io.ho_ld, io.ho2_ld))
                assert vec == (variant in ("vector", "bcast")), (variant, "takes the path it is meant to take")
                key = "gates " + ("vector" if vec else "scalar")
                r = _check_gates(key, lib, io, s, oo, o2, model, tol, alias)
            print(N, H, variant, round(r, 3))
    print({k: round(v, 3) for k, v in _WORST.items() if k.startswith("gates")})


def test_gates_past_the_grid_cap():
    """H = 4, one broadcast gi row, 8192 * 256 + 1 rows: the grid is capped at 8192 workgroups of 256 threads with one
    hidden quad each, so the last row is reached only by the second pass of the grid-stride loop."""
    _native, lib = _lib()
    N, H = 8192 * 256 + 1, 4
    d = gm.gates_case_data(N, H, "bcast")
    model, restate = gm.gates_expect(d)
    tol, share = gm.tolerance("h", model, restate)
    assert gm.fair(share)
    io = _native.GruGatesIO()
    gi, gh, h, out = dense(d["gi"]), dense(d["gh"]), dense(d["h"]), Slab(N * H)
    io.n_rows, io.H, io.gi, io.gi_ld, io.gh, io.gh_ld = N, H, gi.ptr, 0, gh.ptr, 3 * H
    io.h, io.h_ld, io.h_out, io.ho_ld = h.ptr, H, out.ptr, H
    assert lib.macjd_gru_gates(ctypes.byref(io), _stream()) == OK
    torch.cuda.synchronize()
    r = _ratio("gates past the cap", out.read(), model, tol)
    assert out.rest_intact("all") and gh.rest_intact() and h.rest_intact() and gi.rest_intact()
    print("gates past the grid cap", round(r, 3))


def test_gates_refusals():
    _native, lib = _lib()
    assert lib.macjd_gru_gates(None, _stream()) == EINVAL
    d = gm.gates_case_data(5, 12, "vector")

    def attempt(change):
        io, s, oo, o2 = _gates_io(_native, d, "vector", False, True)
        change(io)
        assert lib.macjd_gru_gates(ctypes.byref(io), _stream()) == EINVAL
        torch.cuda.synchronize()
        assert s["out"].rest_intact() and s["out2"].rest_intact()

    for name, value in (("n_rows", -1), ("H", 0), ("H", -4), ("H", 6), ("H", 13), ("gi", None), ("gh", None), ("h", None),
                        ("h_out", None), ("gi_ld", 1), ("gi_ld", 35), ("gi_ld", -36), ("gh_ld", 35), ("gh_ld", 0),
                        ("h_ld", 11), ("ho_ld", 11), ("ho2_ld", 11)):
        attempt(lambda io, n=name, v=value: setattr(io, n, v))
    # no rows: nothing to do, nothing written
    io, s, oo, o2 = _gates_io(_native, d, "vector", False, True)
    io.n_rows = 0
    assert lib.macjd_gru_gates(ctypes.byref(io), _stream()) == OK
    torch.cuda.synchronize()
    assert s["out"].rest_intact() and s["out2"].rest_intact()
