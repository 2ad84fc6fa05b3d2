"""``macjd_agent_episode`` / ``macjd_agent_episode_seq`` (``agent_episode_kernel<H, J, A, FLAT, SEQ>``,
csrc/macjd_episode.hip) against the float64 model of their contract (tests/rollout_agent_model.py, proved on the CPU in
tests/test_rollout_agent_cpu.py), through the C-ABI: the nine one-tile-per-agent sizes at E around the 16-env workgroup,
the four-tile form at row counts that do not fill four tiles (J = 1, 4, 5, 12 and A = 33), T in {1, 2, 3, 7}, one gi / P row
for all and per-row strides (minimal, padded, odd) mixed, h0 NULL and given, W1 with a padded row and at an odd float
offset, masks NULL / int32 / int64 / permuted with rows that have nothing available, epsilon mixing 0, 0.3 and 1 within an
episode, greedy_only with eps = NULL, counter_base NULL and at 2^32 - 2 (the steps cross into the high counter word),
h_final present and NULL; per-step inputs in every stride form, bit for bit against T launches with T = 1.

Comparison: TEACHER-FORCED per step — h_t from the launch's own stored h_(t-1) against the float64 cell, then the Q-head
and the selection on the launch's stored h_t — and FREE-RUNNING over the episode.  Hidden states: min(1e-5, max(12.5 ulp,
8 x the float32 restatement's deviation along the model's trajectory)).  Exploring rows must equal the model's action;
greedy rows must equal the masked first arg-max where the model's lead exceeds 4 x the Q tolerance; P_out is bitwise
P_all[n, chosen].  ``hidden`` is allocated with T + 1 rows: row T, the margins and everything else must keep their bits.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import rollout_agent_model as m  # noqa: E402
from nan_slab import Slab, dense, stream, strided  # noqa: E402
from test_qhead_select_f64_gpu import avail_slab  # noqa: E402

pytestmark = pytest.mark.gpu
OK, EINVAL, EUNSUPPORTED = 0, -1, -4     # include/macjd.h
f32, f64 = np.float32, np.float64
_WORST = {}


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def _ld(c):
    H, A = c["H"], c["A"]
    return ({"0": 0, "min": 3 * H, "pad4": 3 * H + 4, "odd": 3 * H + 1}[c["gi_ld"]], {"0": 0, "min": A, "pad3": A + 3}[c["p_ld"]])


def _lt(c):
    """(gi_lt, p_lt) of a per-step case."""
    H, A, N = c["H"], c["A"], c["E"] * c["J"]
    gi_ld, p_ld = _ld(c)
    gb, pb = (N * gi_ld if gi_ld else 3 * H), (N * p_ld if p_ld else A)
    return {"zero": (0, 0), "block": (gb, pb), "padded": (gb + 7, pb + 3), "frame": (3 * H, A), "full": (gb, pb)}[c["seq"]]


def build(_native, c, d, gi=None, P=None, h0="case", eps="case", counter_base="case", T=None, seq=None):
    """-> (io or seq io, its base block, input slabs, output slabs).  gi [steps, rows or 1, 3H], P [steps, rows or 1, A]."""
    H, J, A, E = c["H"], c["J"], c["A"], c["E"]
    N = E * J
    T = c["T"] if T is None else T
    gi, P = (d["gi"] if gi is None else gi), (d["P"] if P is None else P)
    h0 = d["h0"] if isinstance(h0, str) else h0
    eps = c["eps"] if isinstance(eps, str) else eps
    counter_base = c["counter_base"] if isinstance(counter_base, str) else counter_base
    sio = _native.AgentEpisodeSeqIO() if seq else None
    io = sio.base if seq else _native.AgentEpisodeIO()
    io.n_envs, io.T, io.J, io.H, io.A, io.greedy_only = E, T, J, H, A, 1 if eps is None else 0
    gi_ld, p_ld = _ld(c)
    gi_lt, p_lt = _lt(c) if seq else (0, 0)
    b, o = {}, {}
    b["gi"], _ = strided(gi, (gi_lt, gi_ld if gi_ld else 3 * H, 1), off=1 if gi_ld % 2 else 0)
    b["P"], _ = strided(P, (p_lt, p_ld if p_ld else A, 1), off=1)
    io.gi, io.gi_ld, io.P_all, io.p_ld = b["gi"].ptr, gi_ld, b["P"].ptr, p_ld
    if seq:
        sio.gi_lt, sio.p_lt = gi_lt, p_lt
    if h0 is not None:
        b["h0"] = dense(h0, off=1)
        io.h0 = b["h0"].ptr
    b["w_hh"], b["b_hh"] = dense(d["w_hh"]), dense(d["b_hh"], off=1)
    b["W1"], b["b1"], b["w2"], b["b2"] = dense(d["W1"], off=c["w1_off"]), dense(d["b1"], off=1), dense(d["w2"]), dense(d["b2"], off=1)
    io.w_hh, io.b_hh, io.W1, io.w1_ld = b["w_hh"].ptr, b["b_hh"].ptr, b["W1"].ptr, d["W1"].shape[1]
    assert io.W1 % 16 == (4 if c["w1_off"] else 0) and io.w1_ld == H + A + 1 + c["w1_pad"]
    io.b1, io.w2, io.b2 = b["b1"].ptr, b["w2"].ptr, b["b2"].ptr
    if d["avail"] is not None:
        b["avail"], io.avail_elem_size, (io.av_se, io.av_sj, io.av_sa) = avail_slab(d["avail"], c["avail"])
        io.avail = b["avail"].ptr
    if eps is not None:
        b["eps"] = dense(eps, off=1)
        io.eps = b["eps"].ptr
    io.seed = c["seed"]
    if counter_base is not None:
        b["ctr"] = dense([counter_base], off=1, dtype=np.int64)
        io.counter_base = b["ctr"].ptr
    o["hidden"] = Slab((T + 1) * N * H)
    o["T"], o["P"] = Slab(T * N, off=1, dtype=np.int32), Slab(T * N, off=1)
    io.hidden, io.T_out, io.P_out = o["hidden"].ptr, o["T"].ptr, o["P"].ptr
    if c["h_final"]:
        o["h_final"] = Slab(N * H, off=1)
        io.h_final = o["h_final"].ptr
    return (sio if seq else io), io, b, o


def launch(lib, io, seq=False):
    rc = (lib.macjd_agent_episode_seq if seq else lib.macjd_agent_episode)(ctypes.byref(io), stream())
    torch.cuda.synchronize()
    return rc


def read_outputs(c, o, T=None):
    """hidden [T, N, H] float32, T_out [T, N], P_out [T, N] — after checking that nothing else was written."""
    T = c["T"] if T is None else T
    N, H = c["E"] * c["J"], c["H"]
    written = np.arange(T * N * H)
    assert o["hidden"].rest_intact(written), (c["name"], "hidden row T / margins")
    assert o["T"].rest_intact("all") and o["P"].rest_intact("all"), c["name"]
    hid = o["hidden"].read(written).reshape(T, N, H)
    assert np.isfinite(hid).all(), c["name"]
    if "h_final" in o:
        assert o["h_final"].rest_intact("all")
        assert np.array_equal(o["h_final"].read().view(np.uint32), hid[T - 1].reshape(-1).view(np.uint32)), (c["name"], "h_final")
    return hid, o["T"].read().reshape(T, N).astype(np.int64), o["P"].read().reshape(T, N)


def check_against_the_model(c, d, hid, T_out, P_out):
    fair = m.ep_fair(c)
    N, H, A = c["E"] * c["J"], c["H"], c["A"]
    prev = np.zeros((N, H), f32) if d["h0"] is None else d["h0"]
    rows = np.arange(N)
    r_step = r_free = 0.0
    loose = greedy = 0
    for t in range(c["T"]):
        want = m.episode_step(c, d, t, prev)
        r_step = max(r_step, float(np.abs(hid[t].astype(f64) - want).max()) / fair["tol_step"])
        r_free = max(r_free, float(np.abs(hid[t].astype(f64) - fair["model"][t]).max()) / fair["tol_free"])
        q, tol, sel, P = m.step_choice(c, d, t, hid[t])
        ch = T_out[t]
        assert ((ch >= 0) & (ch < A)).all(), (c["name"], t)
        ok, lo = m.check_choice(sel, ch)
        assert ok.all(), (c["name"], "step", t, "rows", np.nonzero(~ok)[0][:8], ch[~ok][:8], sel["action"][~ok][:8], sel["explore"][~ok][:8])
        loose, greedy = loose + int(lo.sum()), greedy + int((~sel["explore"]).sum())
        assert np.array_equal(P_out[t].view(np.uint32), np.ascontiguousarray(P[rows, ch], f32).view(np.uint32)), (c["name"], "P_out", t)
        if d["avail"] is not None:
            av = d["avail"].reshape(N, A)
            some = av.any(axis=1)
            assert av[rows, ch][some].all() and (ch[~some & ~sel["explore"]] == 0).all(), (c["name"], t)
        prev = hid[t]
    assert r_step <= 1.0 and r_free <= 1.0, (c["name"], "hidden: teacher-forced", r_step, "free-running", r_free)
    for k, v in (("hidden teacher-forced", r_step), ("hidden free-running", r_free)):
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    _WORST["greedy rows"] = _WORST.get("greedy rows", 0) + greedy
    _WORST["non-binding rows"] = _WORST.get("non-binding rows", 0) + loose
    return round(r_step, 3), round(r_free, 3), loose


def _groups():
    g = {f"tile-h{H}-j{J}-a{A}": [] for H, J, A in m.ONE_TILE}
    g.update({"flat-j1": [], "flat-j4-j5": [], "flat-j12": [], "flat-j3": []})
    for c in m.ep_cases():
        n = c["name"]
        key = n.rsplit("-", 1)[0] if n.startswith("tile") else {1: "flat-j1", 4: "flat-j4-j5", 5: "flat-j4-j5", 12: "flat-j12", 3: "flat-j3"}[c["J"]]
        g[key].append(n)
    return g


GROUPS = _groups()


@pytest.mark.parametrize("group", list(GROUPS))
def test_episode_against_the_model(group):
    _native, lib = _lib()
    assert GROUPS[group]
    for name in GROUPS[group]:
        c = m.ep_case(name)
        d = m.ep_data(c)
        io, _, b, o = build(_native, c, d)
        assert launch(lib, io) == OK, name
        hid, T_out, P_out = read_outputs(c, o)
        assert all(s.rest_intact() for s in b.values()), (name, "an input was written")
        print(name, "flat" if m.ep_is_flat(c) else "tile", "T", c["T"], "teacher-forced / free-running / non-binding",
              check_against_the_model(c, d, hid, T_out, P_out))
    print({k: (round(v, 3) if isinstance(v, float) else v) for k, v in _WORST.items()})


@pytest.mark.parametrize("size", m.SEQ_SIZES, ids=[f"h{H}-j{J}-a{A}" for H, J, A in m.SEQ_SIZES])
def test_per_step_inputs_against_the_model_and_the_static_launch(size):
    _native, lib = _lib()
    H, J, A = size
    for c in [c for c in m.seq_cases() if (c["H"], c["J"], c["A"]) == size]:
        d = m.ep_data(c)
        N, T = c["E"] * J, c["T"]
        io, _, b, o = build(_native, c, d, seq=True)
        assert launch(lib, io, seq=True) == OK, c["name"]
        hid, T_out, P_out = read_outputs(c, o)
        assert all(s.rest_intact() for s in b.values())
        print(c["name"], "T", T, check_against_the_model(c, d, hid, T_out, P_out))
        if c["seq"] == "zero":      # both time strides 0: the static launch, bit for bit
            io1, _, _, o1 = build(_native, c, d)
            assert launch(lib, io1) == OK
            parts = [read_outputs(c, o1)]
        else:                        # step t = a T = 1 launch on (gi[t], P[t], h0 = h_(t-1), eps + t, *counter_base + t)
            parts, prev = [], d["h0"]
            for t in range(T):
                cb = None if (c["counter_base"] is None and t == 0) else (c["counter_base"] or 0) + t     # NULL counts as 0
                io1, _, _, o1 = build(_native, c, d, gi=d["gi"][t:t + 1], P=d["P"][t:t + 1], h0=prev,
                                      eps=None if c["eps"] is None else c["eps"][t:t + 1], counter_base=cb, T=1)
                assert launch(lib, io1) == OK
                parts.append(read_outputs(c, o1, T=1))
                prev = parts[-1][0][0]
        for k, got in enumerate((hid, T_out, P_out)):
            one = np.concatenate([p[k] for p in parts], axis=0)
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(one).view(np.uint8)), (c["name"], "output", k)
    c = m.ep_case(f"seq-h{H}-j{J}-a{A}-block")
    for name, value in (("gi_lt", 3 * H - 1), ("gi_lt", 1), ("p_lt", A - 1), ("p_lt", 1), ("gi_lt", -1), ("p_lt", -1)):
        io, _, b, o = build(_native, c, m.ep_data(c), seq=True)
        setattr(io, name, value)
        assert launch(lib, io, seq=True) == EINVAL, (name, value)
        assert all(s.rest_intact() for s in o.values())


def test_unsupported_sizes():
    _native, lib = _lib()
    c = m.ep_case("tile-h64-j3-a9-e17")
    for H, J, A in ((128, 6, 17), (128, 2, 17), (64, 3, 7)):
        io, _, b, o = build(_native, c, m.ep_data(c))
        io.H, io.J, io.A = H, J, A
        assert launch(lib, io) == EUNSUPPORTED, (H, J, A)
        assert all(s.rest_intact() for s in o.values())
    c = m.ep_case("seq-h64-j3-a9-block")
    for H, J, A in ((64, 2, 9), (64, 12, 33), (128, 2, 9)):
        io, base, b, o = build(_native, c, m.ep_data(c), seq=True)
        base.H, base.J, base.A = H, J, A
        assert launch(lib, io, seq=True) == EUNSUPPORTED, (H, J, A)
        assert all(s.rest_intact() for s in o.values())


@pytest.mark.parametrize("seq", [False, True], ids=["static", "per-step"])
def test_argument_errors_leave_the_outputs_alone(seq):
    _native, lib = _lib()
    fn = lib.macjd_agent_episode_seq if seq else lib.macjd_agent_episode
    assert fn(None, stream()) == EINVAL
    c = m.ep_case("seq-h64-j2-a5-block") if seq else next(c for c in m.ep_cases() if c["H"] == 64 and c["eps"] is not None and c["avail"])
    d = m.ep_data(c)
    H, A = c["H"], c["A"]

    def attempt(change, what, rc=EINVAL):
        io, base, b, o = build(_native, c, d, seq=seq)
        change(base)
        assert launch(lib, io, seq=seq) == rc, what
        assert all(s.rest_intact() for s in o.values()), what

    for name, value in (("n_envs", -1), ("T", 0), ("T", -1), ("gi", None), ("P_all", None), ("w_hh", None), ("b_hh", None), ("W1", None),
                        ("b1", None), ("w2", None), ("b2", None), ("hidden", None), ("T_out", None), ("P_out", None), ("eps", None),
                        ("gi_ld", 3 * H - 1), ("gi_ld", 1), ("gi_ld", -3 * H), ("p_ld", A - 1), ("p_ld", -A), ("w1_ld", H + A),
                        ("avail_elem_size", 2), ("avail_elem_size", 0)):
        attempt(lambda io, n=name, v=value: setattr(io, n, v), (name, value))

    def misaligned(io):     # the rows of w_hh are read as 16-byte fragments: refused, never launched
        io.w_hh = io.w_hh + 4
    attempt(misaligned, "w_hh + 4 bytes")
    attempt(lambda io: setattr(io, "n_envs", 0), "no envs: nothing to do, nothing written", rc=OK)
