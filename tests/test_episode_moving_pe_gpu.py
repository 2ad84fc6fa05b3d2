"""``macjd_agent_episode_moving_pe`` (``agent_episode_moving_pe_kernel<J, R, A, SQ>``, csrc/macjd_episode_moving_pe.h) against
the float64 model of its contract (tests/episode_moving_pe_model.py, proved on the CPU in
tests/test_episode_moving_pe_cpu.py), through the C-ABI: both sizes (S = 46 and 24: the zero pad of the last 16-column
block), E around the 16-env workgroup, T in {1, 2, 7}, F in {1, 5}, position tables at tile 4 / 24 / 256 (a tile boundary inside
a workgroup, several tiles per workgroup) with the padded lanes of the last tile left at NaN, step counters NULL / zero /
staggered across the clamp, padded state rows whose position columns hold NaN (the contract ignores them), the scenario's
own and shuffled position columns, h0 NULL / given, masks NULL / int32 / int64, epsilon mixed / greedy / ones, counter_base
NULL / 1000 / 2^32 - 2.

Comparison: TEACHER-FORCED per step — h_t from the launch's own stored h_(t-1), then the actor output, the Q-head and the
selection on the launch's stored h_t — and FREE-RUNNING over the episode, with the tolerances of the model's docstring.
Exploring and binding rows must equal the model's action, the others the leader or the runner-up; the chosen power must be
the model's P[n, chosen] within tol(P).  Every output lies between NaN / sentinel margins that must keep their bits.

Measured on an MI355X: hidden states at most 0.133 (teacher-forced) / 0.142 (free-running) of the tolerance, chosen power at
most 0.008 of tol(P), no non-binding row among the 4 112 greedy rows, every choice the model's."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import episode_moving_pe_model as em  # noqa: E402
import rollout_agent_model as m  # noqa: E402
from nan_slab import Slab, dense, stream, strided  # noqa: E402
from test_qhead_select_f64_gpu import avail_slab  # noqa: E402

pytestmark = pytest.mark.gpu
OK, EINVAL, EUNSUPPORTED = 0, -1, -4     # include/macjd.h
f32, f64 = np.float32, np.float64
H = em.H
_WORST = {}


def _lib():
    from macjd_amd import _native
    return _native, _native.load()


def positions_slab(pos, tile):
    """[E, F + 1, n_pos] -> the tiled table [n_tiles, F + 1, n_pos, tile]; the padded lanes of the last tile stay NaN."""
    E, F1, n_pos = pos.shape
    e, f, p = np.meshgrid(np.arange(E), np.arange(F1), np.arange(n_pos), indexing="ij")
    offs = (((e // tile) * F1 + f) * n_pos + p) * tile + e % tile
    n_tiles = (E + tile - 1) // tile
    return Slab(n_tiles * F1 * n_pos * tile, off=1).put(offs, pos)


def build(_native, c, d, h0="case", eps="case", counter_base="case", T=None, step="case", h_final=None):
    """-> (io, input slabs, output slabs)."""
    J, R, A, S, E, F = c["J"], c["R"], c["A"], c["S"], c["E"], c["F"]
    N = E * J
    T = c["T"] if T is None else T
    h0 = d["h0"] if isinstance(h0, str) else h0
    eps = c["eps"] if isinstance(eps, str) else eps
    counter_base = c["counter_base"] if isinstance(counter_base, str) else counter_base
    if isinstance(step, str):
        step = None if c["step"] is None else em.step0(c)
    io = _native.AgentEpisodeMovingPeIO()
    io.n_envs, io.T, io.J, io.R, io.H, io.A, io.S = E, T, J, R, H, A, S
    io.actor_hidden, io.greedy_only = em.AH, 1 if eps is None else 0
    b, o = {}, {}
    if h0 is not None:
        b["h0"] = dense(h0, off=1)
        io.h0 = b["h0"].ptr
    for k in ("w_hh", "w_ih", "a2_w"):                       # read as 16-byte fragments
        b[k] = dense(d[k])
        assert b[k].ptr % 16 == 0
    for k in ("fc1_w", "fc1_b", "b_ih", "b_hh", "a1_w", "a1_b", "a2_b", "a3_w", "a3_b", "b1", "b2"):
        b[k] = dense(d[k], off=1)
    b["w2"] = dense(d["w2"])
    b["W1"] = dense(d["W1"], off=c["w1_off"])
    for k in ("fc1_w", "fc1_b", "w_ih", "b_ih", "w_hh", "b_hh", "a1_w", "a1_b", "a2_w", "a2_b", "a3_w", "a3_b", "W1", "b1", "w2", "b2"):
        setattr(io, k, b[k].ptr)
    io.w1_ld = d["W1"].shape[1]
    assert io.w1_ld == H + A + 1 + c["w1_pad"]
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
    st_se = S + c["st_pad"]
    state = d["state"].copy()
    state[:, d["cols"]] = np.nan                              # the position columns of the state rows are ignored
    b["state"], _ = strided(state, (st_se, 1), off=1)
    io.state, io.st_se = b["state"].ptr, st_se
    if step is not None:
        b["step"] = dense(step, off=1, dtype=np.int32)
        io.step = b["step"].ptr
    b["positions"] = positions_slab(d["positions"], c["tile"])
    b["cols"] = dense(d["cols"], off=1, dtype=np.int32)
    io.positions, io.position_columns = b["positions"].ptr, b["cols"].ptr
    io.n_frames, io.n_pos, io.tile = F, 2 * R + 2 * J, c["tile"]
    o["hidden"] = Slab((T + 1) * N * H)
    o["T"], o["P"] = Slab(T * N, off=1, dtype=np.int32), Slab(T * N, off=1)
    io.hidden, io.T_out, io.P_out = o["hidden"].ptr, o["T"].ptr, o["P"].ptr
    if c["h_final"] if h_final is None else h_final:
        o["h_final"] = Slab(N * H, off=1)
        io.h_final = o["h_final"].ptr
    return io, b, o


def launch(lib, io):
    rc = lib.macjd_agent_episode_moving_pe(ctypes.byref(io), stream())
    torch.cuda.synchronize()
    return rc


def read_outputs(c, o, T=None):
    """hidden [T, N, H] float32, T_out [T, N], P_out [T, N] — after checking that nothing else was written."""
    T = c["T"] if T is None else T
    N = c["E"] * c["J"]
    written = np.arange(T * N * H)
    assert o["hidden"].rest_intact(written), (c["name"], "hidden row T / margins")
    assert o["T"].rest_intact("all") and o["P"].rest_intact("all"), c["name"]
    hid = o["hidden"].read(written).reshape(T, N, H)
    assert np.isfinite(hid).all(), (c["name"], "a NaN reached the hidden state: a padded lane / an ignored column was read")
    if "h_final" in o:
        assert o["h_final"].rest_intact("all")
        assert np.array_equal(o["h_final"].read().view(np.uint32), hid[T - 1].reshape(-1).view(np.uint32)), (c["name"], "h_final")
    return hid, o["T"].read().reshape(T, N).astype(np.int64), o["P"].read().reshape(T, N)


def check_against_the_model(c, d, hid, T_out, P_out):
    fair = em.fair(c)
    N, A = c["E"] * c["J"], c["A"]
    prev = np.zeros((N, H), f32) if d["h0"] is None else d["h0"]
    rows = np.arange(N)
    r_step = r_free = r_p = 0.0
    loose = greedy = 0
    for t in range(c["T"]):
        want = em.episode_step(c, d, t, prev)
        r_step = max(r_step, float(np.abs(hid[t].astype(f64) - want).max()) / fair["tol_step"])
        r_free = max(r_free, float(np.abs(hid[t].astype(f64) - fair["model"][t]).max()) / fair["tol_free"])
        q, tol, sel, P, p_tol = em.step_choice(c, d, t, hid[t])
        ch = T_out[t]
        assert ((ch >= 0) & (ch < A)).all(), (c["name"], t)
        ok, lo = m.check_choice(sel, ch)
        assert ok.all(), (c["name"], "step", t, "rows", np.nonzero(~ok)[0][:8], ch[~ok][:8], sel["action"][~ok][:8], sel["explore"][~ok][:8])
        loose, greedy = loose + int(lo.sum()), greedy + int((~sel["explore"]).sum())
        r_p = max(r_p, float((np.abs(P_out[t].astype(f64) - P[rows, ch]) / p_tol[rows, ch]).max()))
        if d["avail"] is not None:
            av = d["avail"].reshape(N, A)
            some = av.any(axis=1)
            assert av[rows, ch][some].all() and (ch[~some & ~sel["explore"]] == 0).all(), (c["name"], t)
        prev = hid[t]
    print(c["name"], "T", c["T"], "hidden teacher-forced / free-running, chosen power (shares of the tolerance)", round(r_step, 3),
          round(r_free, 3), round(r_p, 3), "non-binding", loose, "of", greedy)
    assert r_step <= 1.0 and r_free <= 1.0 and r_p <= 1.0, (c["name"], "teacher-forced", r_step, "free-running", r_free, "power", r_p)
    for k, v in (("hidden teacher-forced", r_step), ("hidden free-running", r_free), ("chosen power", r_p)):
        _WORST[k] = max(_WORST.get(k, 0.0), v)


@pytest.mark.parametrize("family", list(em.families()))
def test_episode_against_the_model(family):
    _native, lib = _lib()
    for name in em.families()[family]:
        c = em.case(name)
        d = em.data(c)
        io, b, o = build(_native, c, d)
        assert launch(lib, io) == OK, name
        hid, T_out, P_out = read_outputs(c, o)
        assert all(s.rest_intact() for s in b.values()), (name, "an input was written")
        check_against_the_model(c, d, hid, T_out, P_out)
    print({k: round(v, 3) for k, v in _WORST.items()})


@pytest.mark.parametrize("name", ["j3-e33-tile24-stagger", "j3-e17-tile256-nullstep", "j2-e33-tile24-stagger", "j2-e33-tile4-stagger",
                                  "pm4-j3-e33", "j2-e17-1"])
def test_a_T_step_launch_equals_T_single_step_launches(name):
    """Step t = a T = 1 launch on (h0 = h_(t-1) through h_final, step + t, eps + t, *counter_base + t), bit for bit."""
    _native, lib = _lib()
    c = em.case(name)
    d = em.data(c)
    T = c["T"]
    assert T >= 2
    io, b, o = build(_native, c, d)
    assert launch(lib, io) == OK
    hid, T_out, P_out = read_outputs(c, o)
    parts, prev = [], d["h0"]
    s0 = em.step0(c)
    for t in range(T):
        cb = None if (c["counter_base"] is None and t == 0) else (c["counter_base"] or 0) + t     # NULL counts as 0
        st = None if (c["step"] is None and t == 0) else s0 + t
        io1, _, o1 = build(_native, c, d, h0=prev, eps=None if c["eps"] is None else c["eps"][t:t + 1], counter_base=cb, T=1, step=st,
                           h_final=True)
        assert launch(lib, io1) == OK
        parts.append(read_outputs(c, o1, T=1))
        prev = o1["h_final"].read().reshape(-1, H)
    for k, got in enumerate((hid, T_out, P_out)):
        one = np.concatenate([p[k] for p in parts], axis=0)
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(one).view(np.uint8)), (name, "output", k)


def test_unsupported_sizes():
    _native, lib = _lib()
    c = em.case("j3-e17-0")
    for J, R, Hh, A, ah in ((6, 8, 64, 17, 128), (3, 4, 128, 9, 128), (3, 4, 64, 5, 128), (2, 2, 64, 9, 128), (3, 3, 64, 7, 128),
                            (2, 4, 64, 5, 128), (3, 4, 64, 9, 64), (3, 4, 64, 9, 256)):
        io, b, o = build(_native, c, em.data(c))
        io.J, io.R, io.H, io.A, io.actor_hidden = J, R, Hh, A, ah
        io.n_pos = 2 * R + 2 * J
        assert launch(lib, io) == EUNSUPPORTED, (J, R, Hh, A, ah)
        assert all(s.rest_intact() for s in o.values())


def test_argument_errors_leave_the_outputs_alone():
    _native, lib = _lib()
    assert lib.macjd_agent_episode_moving_pe(None, stream()) == EINVAL
    c = next(c for c in em.cases() if c["eps"] is not None and c["avail"] and c["step"] is not None and c["h_final"])
    d = em.data(c)
    S, A = c["S"], c["A"]

    def attempt(change, what, rc=EINVAL):
        io, b, o = build(_native, c, d)
        change(io)
        assert launch(lib, io) == rc, what
        assert all(s.rest_intact() for s in o.values()), what

    required = ("fc1_w", "fc1_b", "w_ih", "b_ih", "w_hh", "b_hh", "a1_w", "a1_b", "a2_w", "a2_b", "a3_w", "a3_b", "W1", "b1", "w2", "b2",
                "eps", "state", "positions", "position_columns", "hidden", "T_out", "P_out")
    for name, value in [(n, None) for n in required] + [
            ("n_envs", -1), ("T", 0), ("T", -1), ("n_frames", 0), ("n_frames", -1), ("n_pos", 2 * c["R"] + 2 * c["J"] - 1),
            ("n_pos", 2 * c["R"] + 2 * c["J"] + 1), ("n_pos", 0), ("tile", 0), ("tile", -4), ("st_se", S - 1), ("st_se", 0), ("st_se", -S),
            ("S", 0), ("S", -1), ("S", 49), ("S", 64), ("avail_elem_size", 2), ("avail_elem_size", 0), ("avail_elem_size", 16),
            ("w1_ld", H + A), ("w1_ld", 0)]:
        attempt(lambda io, n=name, v=value: setattr(io, n, v), (name, value))
    for name in ("w_hh", "w_ih", "a2_w"):      # read as 16-byte fragments: refused, never launched
        for delta in (4, 8):
            attempt(lambda io, n=name, dl=delta: setattr(io, n, getattr(io, n) + dl), (name, "+", delta, "bytes"))
    # what may be NULL is accepted, and an empty batch is nothing to do
    attempt(lambda io: setattr(io, "n_envs", 0), "no envs: nothing written", rc=OK)
    for name in ("h0", "avail", "step", "counter_base", "h_final"):
        io, b, o = build(_native, c, d)
        setattr(io, name, None)
        assert launch(lib, io) == OK, name
    io, b, o = build(_native, c, d, eps=None)              # greedy_only: eps may be NULL
    assert io.greedy_only == 1 and not io.eps and launch(lib, io) == OK
