"""``macjd_qhead_select`` (``qhead_select_kernel<AT, HS>``, csrc/macjd_nets.hip) against the float64 model of its contract
(tests/rollout_agent_model.py, proved on the CPU in tests/test_rollout_agent_cpu.py), through the C-ABI: both forms (eight
waves over 64 rows; one lane per row, entered by 65537 rows and by H < 16), row counts around the 64-row workgroup, hidden
sizes whose wave chunk does not divide them (17, 20: waves without units), 16-byte and scalar loads of ``base``, every
compiled A and the generic form up to A = 64 (bit 63 of the availability word), one to twelve agents, int32 / int64 masks in
[E, J, A] and permuted order, rows with no and with exactly one available action, every optional output alone and all
together, [E, J, 1] and agent-major output strides, gather indices 0, A - 1 and out of range, epsilon by value and through
``eps_dev``, ``counter + *counter_dev`` across 2^32, a seed above 2^32, ``greedy_only`` with epsilon = 1, constructed exact
ties, every refusal.

The exploration draw is decided by integers: an exploring row must EQUAL the model's action (Philox words -> explore compare
-> k-th available action).  A greedy row must equal the model's masked first arg-max where the model's lead exceeds 4 x the
Q tolerance (the CPU test asserts that at most 0.5 % of a case's greedy rows are not binding); ``P_out`` is bitwise
``P_all[n, chosen]``.  Q: min(gamma(H + 4) sum |terms|, 1e-5 max(1, max|Q|)).  Outputs sit between sentinel margins; what the
launch may not write must survive bit for bit.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import rollout_agent_model as m  # noqa: E402
from nan_slab import Slab, dense, offsets, stream, strided  # noqa: E402

pytestmark = pytest.mark.gpu
OK, EINVAL = 0, -1     # include/macjd.h
f32, f64 = np.float32, np.float64
_WORST = {}


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def avail_slab(avail, mode):
    """[E, J, A] bool -> (Slab, elem size, (se, sj, sa)); available = a non-zero value, not always 1."""
    E, J, A = avail.shape
    dtype = np.int64 if mode.endswith("64") else np.int32
    strides = (1, E, J * E) if mode.startswith("perm") else (J * A, A, 1)
    vals = avail.astype(dtype) * (1 + (np.arange(avail.size).reshape(avail.shape) % 3))
    if dtype is np.int64:
        vals = vals * (2 ** 32)          # the low word alone would say "unavailable"
    s, _ = strided(vals, strides, off=1, dtype=dtype)
    return s, np.dtype(dtype).itemsize, strides


def _io(_native, c):
    d = m.qs_data(c)
    N, H, A, na = c["rows"], c["H"], c["A"], c["na"]
    E = N // na
    io = _native.QheadIO()
    io.n_rows, io.H, io.A, io.n_agents, io.greedy_only = N, H, A, na, c["greedy_only"]
    b, o = {}, {}
    base_ld = {"vec": (H + 3) & ~3, "oddoff": (H + 3) & ~3, "oddld": H + 1 + H % 2}[c["base"]]
    b["base"], _ = strided(d["base"], (base_ld, 1), off=1 if c["base"] == "oddoff" else 0)
    b["P"], _ = strided(d["P"], (A + 2, 1), off=1)
    b["W1"], b["w2"], b["b2"] = dense(d["W1"], off=1), dense(d["w2"]), dense(d["b2"], off=1)
    io.base, io.base_ld, io.P_all, io.p_ld = b["base"].ptr, base_ld, b["P"].ptr, A + 2
    io.W1, io.w1_ld, io.w2, io.b2 = b["W1"].ptr, d["W1"].shape[1], b["w2"].ptr, b["b2"].ptr
    vec = io.base % 16 == 0 and base_ld % 4 == 0
    assert vec == (c["base"] == "vec"), (c["name"], "takes the load path it is meant to take")
    if d["avail"] is not None:
        b["avail"], io.avail_elem_size, (io.av_se, io.av_sj, io.av_sa) = avail_slab(d["avail"], c["avail"])
        io.avail = b["avail"].ptr
    io.seed, io.counter = c["seed"], c["counter"]
    if c["eps_dev"]:
        b["eps"] = dense([c["eps"]], off=1)
        io.eps_dev, io.epsilon = b["eps"].ptr, 0.77 if c["eps"] != 0.77 else 0.1      # the value must be ignored
    else:
        io.epsilon = c["eps"]
    if c["counter_dev"] is not None:
        b["ctr"] = dense([c["counter_dev"]], off=1, dtype=np.int64)
        io.counter_dev = b["ctr"].ptr
    outs = c["outs"]
    se, sj = (na, 1) if c["t_layout"] == "ej" else (1, E)
    to = offsets((E, na), (se, sj)).reshape(-1)
    if "Q" in outs:
        o["Q"], o["Qo"] = Slab((N - 1) * (A + 1) + A, off=1), offsets((N, A), (A + 1, 1))
        io.Q, io.q_ld = o["Q"].ptr, A + 1
    if "T32" in outs:
        o["T32"] = Slab(N, off=1, dtype=np.int32)
        io.T_out32, io.t32_se, io.t32_sj = o["T32"].ptr, se, sj
    if "T64" in outs:
        o["T64"] = Slab(N, off=1, dtype=np.int64)
        io.T_out64, io.t64_se, io.t64_sj = o["T64"].ptr, se, sj
    if "P" in outs:
        o["P"] = Slab(N, off=1)
        io.P_out, io.po_se, io.po_sj = o["P"].ptr, se, sj
    if "argmax" in outs:
        o["argmax"] = Slab(N, off=1, dtype=np.int64)
        io.argmax_out = o["argmax"].ptr
    if "gather" in outs:
        b["gidx"], o["gather"] = dense(d["gather"], off=1, dtype=np.int64), Slab(N, off=1)
        io.gather_idx, io.q_gather_out = b["gidx"].ptr, o["gather"].ptr
    return io, b, o, to


def _launch(lib, io):
    rc = lib.macjd_qhead_select(ctypes.byref(io), stream())
    torch.cuda.synchronize()
    return rc


def _check(c, b, o, to):
    d, e = m.qs_data(c), m.qs_expect(c)
    N, A = c["rows"], c["A"]
    rows = np.arange(N)
    note = {}
    for k, s in b.items():
        assert s.rest_intact(), (c["name"], k, "an input was written")
    if "Q" in o:
        got = o["Q"].read(o["Qo"]).astype(f64)
        assert np.isfinite(got).all()
        r = float((np.abs(got - e["q"]) / e["tol"]).max())
        assert r <= 1.0, (c["name"], "Q", r)
        assert o["Q"].rest_intact(o["Qo"]), c["name"]
        _WORST["Q"] = max(_WORST.get("Q", 0.0), r)
        note["Q"] = round(r, 3)
    chosen = None
    for k in ("T32", "T64"):
        if k in o:
            got = o[k].read(to).astype(np.int64)
            assert o[k].rest_intact(to), (c["name"], k)
            assert chosen is None or np.array_equal(chosen, got), (c["name"], "T_out32 and T_out64 differ")
            chosen = got
    if chosen is not None:
        assert ((chosen >= 0) & (chosen < A)).all(), c["name"]
        ok, loose = m.check_choice(e["sel"], chosen)
        assert ok.all(), (c["name"], "rows", np.nonzero(~ok)[0][:8], chosen[~ok][:8], e["sel"]["action"][~ok][:8], e["sel"]["explore"][~ok][:8])
        if d["avail"] is not None:
            av = d["avail"].reshape(N, A)
            some = av.any(axis=1)
            assert av[rows, chosen][some].all(), (c["name"], "an unavailable action was chosen")
            assert (chosen[~some & ~e["sel"]["explore"]] == 0).all(), (c["name"], "nothing available, greedy: action 0")
        note["explored"], note["non-binding"] = int(e["sel"]["explore"].sum()), int(loose.sum())
        if c["tie"]:
            lowest = e["sel"]["greedy"]
            led = e["sel"]["binding"] & np.isin(lowest, d["pair"])             # the tie leads, by more than 4 x tol
            assert led.sum() >= N // 2, (c["name"], "the tie leads on too few rows", int(led.sum()))
            assert np.array_equal(chosen[led], lowest[led]), (c["name"], "the lower available index must win")
        if "P" in o:
            got = o["P"].read(to)
            assert np.array_equal(got.view(np.uint32), d["P"][rows, chosen].view(np.uint32)), (c["name"], "P_out")
            assert o["P"].rest_intact(to)
    elif "P" in o:
        assert o["P"].rest_intact()
    if "argmax" in o:
        got = o["argmax"].read()
        assert o["argmax"].rest_intact("all")
        ok, loose = m.check_choice(e["plain"], got)
        assert ok.all(), (c["name"], "argmax_out", np.nonzero(~ok)[0][:8])
        note["argmax non-binding"] = int(loose.sum())
    if "gather" in o:
        got = o["gather"].read().astype(f64)
        assert o["gather"].rest_intact("all")
        g = d["gather"]
        inside = (g >= 0) & (g < A)
        assert (got[~inside] == 0.0).all(), (c["name"], "an index outside [0, A) stores 0")
        assert (np.abs(got - e["q_gather"])[inside] <= e["gather_tol"][inside]).all(), (c["name"], "q_gather_out")
        if "Q" in o:
            q = o["Q"].read(o["Qo"])
            assert np.array_equal(got[inside].astype(f32).view(np.uint32), q[rows[inside], g[inside]].view(np.uint32))
    return note


GROUPS = {
    "rows and forms": lambda n: n.startswith("rows") or n.startswith("onelane"),
    "hidden sizes and load paths": lambda n: n.startswith("h"),
    "action counts": lambda n: n.startswith("a"),
    "outputs": lambda n: n.startswith("only") or n == "no-mask",
    "exploration": lambda n: n.startswith("eps") or n.startswith("counter") or n.startswith("greedy"),
    "ties": lambda n: n.startswith("tie"),
}


def test_groups_cover_the_table():
    names = [c["name"] for c in m.qs_cases()]
    assert all(sum(bool(f(n)) for f in GROUPS.values()) == 1 for n in names)


@pytest.mark.parametrize("group", list(GROUPS))
def test_qhead_select_against_the_model(group):
    _native, lib = _lib()
    for c in [c for c in m.qs_cases() if GROUPS[group](c["name"])]:
        io, b, o, to = _io(_native, c)
        assert _launch(lib, io) == OK, c["name"]
        print(c["name"], _check(c, b, o, to))
    print("worst |Q - model| / tol so far", {k: round(v, 3) for k, v in _WORST.items()})


def test_refusals_leave_the_outputs_alone():
    _native, lib = _lib()
    assert lib.macjd_qhead_select(None, stream()) == EINVAL
    c = m.qs_case("rows129")

    def attempt(change, what):
        io, b, o, to = _io(_native, c)
        change(io)
        assert _launch(lib, io) == EINVAL, what
        assert all(o[k].rest_intact() for k in o if isinstance(o[k], Slab)), what

    for name, value in (("n_rows", -1), ("H", 0), ("H", -64), ("A", 0), ("A", 65), ("A", -1), ("n_agents", 0), ("n_agents", -3),
                        ("base", None), ("P_all", None), ("W1", None), ("w2", None), ("b2", None), ("avail_elem_size", 2),
                        ("avail_elem_size", 0), ("avail_elem_size", 16)):
        attempt(lambda io, n=name, v=value: setattr(io, n, v), (name, value))

    def no_output(io):
        io.Q = io.T_out32 = io.T_out64 = io.argmax_out = None
        io.gather_idx = None           # q_gather_out alone is no output, nor is P_out
    attempt(no_output, "no output requested")

    def gather_without_destination(io):
        io.Q = io.T_out32 = io.T_out64 = io.argmax_out = io.q_gather_out = None
    attempt(gather_without_destination, "gather_idx without q_gather_out")
    io, b, o, to = _io(_native, c)                     # no rows: nothing to do, nothing written
    io.n_rows = 0
    assert _launch(lib, io) == OK
    assert all(o[k].rest_intact() for k in o if isinstance(o[k], Slab))
