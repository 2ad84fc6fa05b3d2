"""Whole-episode rollout on per-env moving frames, host side: the header's declarations and the ctypes mirror against the
header's layout, the exported symbols and supported sizes, the runner's switch, ``moving_pe_rollout_available`` off its
ground — and tests/episode_moving_pe_model.py: the model against float64 torch (RNNAgent cast to double, the selector's
rule), its observations against ``MovingScenarioBatch.positions`` on a jittered ring, and, from the model alone for every
case, that the float32 restatement stays inside the asserted tolerance, that the tolerance is under the cap, that at most
0.5 % of a case's greedy rows are non-binding, and that the table reaches every edge the GPU file promises."""
import ctypes
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import __graft_entry__ as entry  # noqa: E402
import episode_moving_pe_model as em  # noqa: E402
import gru_scan_model as gm  # noqa: E402
import motion_cases as mcases  # noqa: E402
import rollout_agent_model as m  # noqa: E402
from _harness import REPO  # noqa: E402
from test_nets_cpu import make_args  # noqa: E402

from macjd_amd import _native, options  # noqa: E402

f32, f64 = np.float32, np.float64
t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
SYMS = ("macjd_agent_episode_moving_pe_supported", "macjd_agent_episode_moving_pe")
SWITCH = "MACJD_MOVING_PE_EPISODE_ROLLOUT"


@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


# ------------------------------------------------------------------------------------------------- header, library, switch
def test_header_declares_the_struct_and_both_functions():
    hdr = open(os.path.join(REPO, "include", "macjd_nets.h")).read()
    assert "typedef struct macjd_agent_episode_moving_pe_io {" in hdr and "} macjd_agent_episode_moving_pe_io;" in hdr
    assert "int macjd_agent_episode_moving_pe_supported(int32_t J, int32_t R, int32_t H, int32_t A);" in hdr
    assert "int macjd_agent_episode_moving_pe(const macjd_agent_episode_moving_pe_io* io, void* hip_stream);" in hdr
    # a kernel of its own, in its own file, compiled with the episode translation unit
    src = open(os.path.join(entry.CSRC, "macjd_episode.hip")).read()
    assert '#include "macjd_episode_moving_pe.h"' in src and "macjd_episode.hip" in entry.HIP_SOURCES
    own = open(os.path.join(entry.CSRC, "macjd_episode_moving_pe.h")).read()
    assert "agent_episode_moving_pe_kernel" in own and "agent_episode_moving_pe_kernel" not in src
    assert "agent_env_episode_scan_kernel<" not in own      # not one more variant of the closed-loop kernel


def test_struct_layout_matches_the_header():
    IO = _native.AgentEpisodeMovingPeIO
    names = [n for n, *_ in IO._fields_]
    t = "macjd_agent_episode_moving_pe_io"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd_nets.h"\n'
           f'int main(){{printf("%zu", sizeof({t}));\n'
           + "".join(f'printf(" %zu", offsetof({t}, {n}));\n' for n in names)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(IO)
    assert [getattr(IO, n).offset for n in names] == out[1:]
    # a flat block: no embedded struct, no gi / P_all / env members
    assert all(not issubclass(tp, ctypes.Structure) for _, tp in IO._fields_)
    assert not {"gi", "P_all", "scan", "track", "reward", "st_state", "st_obs", "pe_tables"} & set(names)
    # the agent's members carry the closed-loop block's names
    scan_names = {n for n, *_ in _native.AgentEnvEpisodeScanIO._fields_}
    for n in ("n_envs", "T", "J", "R", "H", "A", "S", "actor_hidden", "greedy_only", "h0", "fc1_w", "fc1_b", "w_ih", "b_ih", "w_hh",
              "b_hh", "a1_w", "a1_b", "a2_w", "a2_b", "a3_w", "a3_b", "W1", "w1_ld", "b1", "w2", "b2", "avail", "avail_elem_size",
              "av_se", "av_sj", "av_sa", "eps", "seed", "counter_base", "step", "hidden", "T_out", "P_out", "h_final"):
        assert n in names and n in scan_names, n
    for n in ("state", "st_se", "positions", "position_columns", "n_frames", "n_pos", "tile"):
        assert n in names, n


def test_library_exports_the_symbols_and_answers_the_supported_sizes(built):
    for sym in SYMS:
        assert sym in _native.EXPORTS and hasattr(built, sym), sym
    f = built.macjd_agent_episode_moving_pe_supported
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int32] * 4
    assert f(3, 4, 64, 9) == 1 and f(2, 2, 64, 5) == 1
    for J, R, H, A in ((6, 8, 64, 17), (3, 4, 128, 9), (3, 4, 64, 5), (2, 2, 64, 9), (2, 2, 128, 5), (12, 16, 64, 33), (3, 3, 64, 7),
                       (3, 2, 64, 9), (2, 4, 64, 5)):
        assert f(J, R, H, A) == 0, (J, R, H, A)
    assert _native.ABI_VERSION == 12
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == 12


def test_switch_is_off_by_default_documented_and_independent(monkeypatch):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    monkeypatch.delenv(SWITCH, raising=False)
    options.reload()
    try:
        assert options._DEFAULTS["MOVING_PE_EPISODE_ROLLOUT"] == "0" and options.get("MOVING_PE_EPISODE_ROLLOUT") == "0"
        assert BatchedEpisodeRunner.moving_pe_episode_rollout is False
        r = BatchedEpisodeRunner.__new__(BatchedEpisodeRunner)     # (no device needed to read a switch)
        assert r.moving_pe_episode_rollout is False
        monkeypatch.setenv(SWITCH, "1")
        options.reload()
        assert BatchedEpisodeRunner.moving_pe_episode_rollout is True and r.moving_pe_episode_rollout is True
        assert r.moving_episode_rollout is False and r.closed_loop_rollout is False and r.closed_loop_moving_rollout is False
        monkeypatch.delenv(SWITCH)
        monkeypatch.setenv("MACJD_MOVING_EPISODE_ROLLOUT", "1")     # the shared-frame switch keeps its meaning
        options.reload()
        assert r.moving_pe_episode_rollout is False and r.moving_episode_rollout is True
        r.moving_pe_episode_rollout = True                          # an instance can set it
        assert r.moving_pe_episode_rollout is True and BatchedEpisodeRunner.moving_pe_episode_rollout is False
    finally:
        for n in (SWITCH, "MACJD_MOVING_EPISODE_ROLLOUT"):
            monkeypatch.delenv(n, raising=False)
        options.reload()
    assert SWITCH in options.__doc__
    assert callable(r.moving_pe_rollout_available) and callable(r.rollout_moving_pe)


class _Trap:
    @property
    def agent(self):
        raise LookupError("the agent was asked for")


def _stub(moving_batch, production=True, kernel_flags=0, device="cuda", moving=True, scanning=False, scenario_batch=None):
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner as Runner
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    env = object.__new__(Env)
    env.scenario = SimpleNamespace(moving=moving, scanning=scanning)
    env.moving_batch, env.scenario_batch, env.kernel_flags = moving_batch, scenario_batch, kernel_flags
    env.step_many_has_production_form = lambda: production
    return Runner, SimpleNamespace(env=env, device=SimpleNamespace(type=device), mac=_Trap())


def test_moving_pe_rollout_available_is_false_off_its_ground():
    """Each stub fails on the env's kind alone — touching the agent would raise — and the last one shows that a per-env moving
    batch gets as far as the agent."""
    for kw in (dict(moving_batch=None),                                   # a shared-frame moving scenario
               dict(moving_batch=None, moving=False),                     # a static scenario
               dict(moving_batch=None, moving=False, scanning=True),      # scanning radars
               dict(moving_batch=None, scanning=True),                    # moving under scanning radars
               dict(moving_batch=None, moving=False, scenario_batch=object()),   # a per-env static / scanning batch
               dict(moving_batch=object(), device="cpu"),
               dict(moving_batch=object(), kernel_flags=1),
               dict(moving_batch=object(), production=False)):            # 6j/8r aside, a size without a production many-step
        Runner, stub = _stub(**kw)
        assert Runner.moving_pe_rollout_available(stub) is False, kw
    Runner, stub = _stub(moving_batch=object())
    with pytest.raises(LookupError):
        Runner.moving_pe_rollout_available(stub)
    stub.moving_pe_rollout_available = lambda: False
    with pytest.raises(RuntimeError, match="rollout_moving_pe: not available"):
        Runner.rollout_moving_pe(stub)


def test_environment_hands_over_only_on_a_per_env_moving_batch():
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    env = object.__new__(Env)        # (the class default: not a per-env moving batch)
    with pytest.raises(RuntimeError, match="episode_moving_pe_args: needs a per-env moving scenario batch"):
        env.episode_moving_pe_args()
    with pytest.raises(RuntimeError, match="frame_positions: needs a per-env moving scenario batch"):
        env.frame_positions()
    # the many-step launch of a per-env moving batch is compiled at the shared-frame launch's sizes
    for J, R, want in ((3, 4, True), (2, 2, True), (6, 8, True), (3, 3, False)):
        env = object.__new__(Env)
        env._motion_io, env._motion_scan_io, env._motion_pe_io = None, None, object()
        env.num_jammers, env.num_radars = J, R
        assert env.step_many_has_production_form() is want, (J, R)
    env._motion_pe_io = None
    env.num_jammers, env.num_radars = 3, 4
    assert env.step_many_has_production_form() is False


# ------------------------------------------------------------------------------------------------- the model is right
def _agent64(c, d):
    from macjd_amd.core.networks import RNNAgent
    A = c["A"]
    agent = RNNAgent(c["S"], make_args(dict(J=c["J"], A=A, S=c["S"], H=em.H))).double()
    sd = {"fc1.weight": d["fc1_w"], "fc1.bias": d["fc1_b"], "rnn.weight_ih": d["w_ih"], "rnn.bias_ih": d["b_ih"],
          "rnn.weight_hh": d["w_hh"], "rnn.bias_hh": d["b_hh"], "actor.0.weight": d["a1_w"], "actor.0.bias": d["a1_b"],
          "actor.2.weight": d["a2_w"], "actor.2.bias": d["a2_b"], "actor.4.weight": d["a3_w"], "actor.4.bias": d["a3_b"],
          "fc2_q_head.0.weight": d["W1"][:, :em.H + A + 1], "fc2_q_head.0.bias": d["b1"],
          "fc2_q_head.2.weight": d["w2"].reshape(1, -1), "fc2_q_head.2.bias": d["b2"]}
    agent.load_state_dict({k: t64(v) for k, v in sd.items()})
    return agent


@pytest.mark.parametrize("name", ["j3-e33-tile24-stagger", "j2-e17-tile256-nullstep", "pm4-j2-e33"])
def test_model_matches_float64_torch(name):
    """A whole episode of the stock RNNAgent in float64 on the model's observations, step by step: hidden trajectory, actor
    output and all-action Q-values to 1e-12, and the greedy choice against the reference's selector."""
    from macjd_amd.utils.action_selectors import EpsilonGreedyActionSelector
    c = em.case(name)
    d = em.data(c)
    J, A, E, T = c["J"], c["A"], c["E"], c["T"]
    N = E * J
    agent = _agent64(c, d)
    sel_ref = EpsilonGreedyActionSelector(make_args(dict(J=J, A=A, S=c["S"], H=em.H)))
    obs = em.observations(c, d)
    model = em.episode(c, d)
    h = torch.zeros(N, em.H, dtype=torch.float64) if d["h0"] is None else t64(d["h0"])
    for t in range(T):
        rows = t64(np.repeat(obs[t], J, axis=0))                      # every agent of an env sees the env's row
        with torch.no_grad():
            h = agent.forward(rows, h)
            p_ref = agent.actor_forward(rows).numpy()
        np.testing.assert_allclose(model[t], h.numpy(), rtol=1e-12, atol=1e-12)
        h32 = model[t].astype(f32)
        q, tol, sel, P, p_tol = em.step_choice(c, d, t, h32)
        np.testing.assert_allclose(P, p_ref, rtol=1e-12, atol=1e-12)
        with torch.no_grad():
            cols = [agent.get_q_value_for_action(t64(h32), torch.full((N,), a), t64(P[:, a])) for a in range(A)]
        q_ref = torch.cat(cols, dim=1)
        np.testing.assert_allclose(q, q_ref.numpy(), rtol=1e-12, atol=1e-12)
        av = np.ones((E, J, A), np.int64) if d["avail"] is None else d["avail"].astype(np.int64)
        ref = sel_ref.select_action(q_ref.view(E, J, A), torch.tensor(av), 0, test_mode=True).numpy().reshape(-1)
        assert np.array_equal(sel["greedy"], ref), (name, t)
        assert (tol > 0).all() and (p_tol > 0).all()


def test_observations_follow_the_batchs_positions_and_the_frame_clamp():
    """The model's observation rule on a jittered ring: env e at step t shows its own state vector with its own
    positions[e, min(step0[e] + t, F)] at the scenario's position columns — spelled out per element here."""
    from macjd_amd.scenario import MovingScenarioBatch
    for size in em.SIZES:
        J, R, A = size
        base = mcases.moving_ring_dict(J, R)
        mb = MovingScenarioBatch.randomized(base, 7, seed=4, config=SimpleNamespace(episode_limit=5), velocity_jitter=1.0, compile="host")
        S, cols = em.SIZES[size]
        assert mb.base.state_dim == S and tuple(int(x) for x in mb.position_columns) == cols and mb.base.n_actions == A
        F = mb.n_frames
        assert mb.positions.shape == (7, F + 1, 2 * R + 2 * J) and mb.positions.dtype == np.float32
        assert not np.array_equal(mb.positions[0], mb.positions[1])               # per-env trajectories
        c = dict(E=7, T=F + 2, F=F, step="stagger")
        d = dict(state=mb.state_vectors.astype(f32), positions=mb.positions, cols=np.asarray(mb.position_columns, np.int32))
        obs = em.observations(c, d)
        s0 = em.step0(c)
        assert s0.min() == 0 and s0.max() >= F
        other = np.setdiff1d(np.arange(S), cols)
        for e in range(7):
            for t in range(F + 2):
                k = min(int(s0[e]) + t, F)
                assert obs[t, e, list(cols)].tobytes() == mb.positions[e, k].tobytes(), (e, t)
                assert obs[t, e, other].tobytes() == mb.state_vectors[e, other].astype(f32).tobytes()
        # frame 0 is the state vector's own positions: a reset env with step = 0 observes its state row unchanged
        assert np.array_equal(mb.state_vectors[:, list(cols)].astype(f32), mb.positions[:, 0])


# ------------------------------------------------------------------------------------------------- the table is fair
@pytest.mark.parametrize("family", list(em.families()))
def test_cases_are_fair(family):
    names = em.families()[family]
    assert names
    greedy = 0
    for name in names:
        c = em.case(name)
        d = em.data(c)
        fair = em.fair(c)
        cap = m.cap(fair["model"])
        # the float32 restatement (first layers, gi and the cell) is inside the tolerance with the rule's factor to spare
        assert fair["dev"] * m.FACTOR <= max(fair["tol_step"], fair["tol_free"]) <= cap <= 1e-5 * (1 + 1e-12), (name, fair["dev"])
        assert gm.FLOOR_H <= fair["tol_step"] <= cap and gm.FLOOR_H <= fair["tol_free"] <= cap, name
        for t in range(c["T"]):
            _, P32, _ = em.step_inputs(c, t, f32)
            _, P, perr = em.step_inputs(c, t)
            p_tol = np.minimum(perr, m.cap(P))
            assert (np.abs(P32.astype(f64) - P) <= p_tol).all() and (p_tol <= m.cap(P)).all(), (name, t)
            h32 = fair["model"][t].astype(f32)
            q, tol, _, _, _ = em.step_choice(c, d, t, h32)
            base32, _ = m.qhead_base(h32, d["W1"], d["b1"], f32)
            q32, _ = m.qhead_all(base32, P32, d["W1"][:, :em.H + c["A"] + 1], d["w2"], d["b2"], dt=f32)
            assert (np.abs(q32.astype(f64) - q) <= tol).all() and (tol <= m.cap(q)).all(), (name, t)
        assert fair["nonbinding"] <= m.NONBINDING_SHARE * max(fair["greedy"], 1), (name, fair["nonbinding"], fair["greedy"])
        greedy += fair["greedy"]
    assert greedy >= 100, (family, greedy)          # so that the share means something


def test_table_reaches_every_edge():
    cs = em.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    for size, (S, cols) in em.SIZES.items():
        mine = [c for c in cs if (c["J"], c["R"], c["A"]) == size]
        assert S in (46, 24) and S % 16 != 0 and all(c["S"] == S for c in mine)        # the zero pad of the last 16-column block
        assert {c["E"] for c in mine} == {1, 15, 16, 17, 33}
        assert {c["T"] for c in mine} == {1, 2, 7} and {c["F"] for c in mine} == {1, 5}
        assert {c["tile"] for c in mine} == {4, 24, 256}
        assert {c["step"] for c in mine} == {None, "zero", "stagger"}
        assert {c["st_pad"] > 0 for c in mine} == {False, True} and {c["cols"] for c in mine} == {"own", "shuffled"}
        assert {c["h0"] for c in mine} == {False, True} and {c["avail"] for c in mine} == {None, "i32", "i64"}
        assert {c["counter_base"] for c in mine} == {None, 1000, 2 ** 32 - 2}
        assert {c["h_final"] for c in mine} == {False, True}
        kinds = {"greedy" if c["eps"] is None else ("ones" if set(c["eps"]) == {1.0} else "mixed") for c in mine}
        assert kinds == {"greedy", "ones", "mixed"}
        assert any(c["eps"] is not None and {0.0, 0.3, 1.0} <= set(c["eps"]) for c in mine)
        # a tile boundary inside a workgroup; several tiles per workgroup; one tile for all
        assert any(c["tile"] == 24 and c["E"] == 33 for c in mine) and any(c["tile"] == 4 and c["E"] >= 16 for c in mine)
        assert any(c["tile"] == 256 and c["E"] > 16 for c in mine)
        # the clamp: envs at or past F at entry, and envs that cross F inside the launch
        st = [c for c in mine if c["step"] == "stagger" and c["T"] >= 2]
        assert st
        for c in st:
            s0 = em.step0(c)
            assert (s0 >= c["F"]).any() and (s0 > c["F"]).any() and ((s0 < c["F"]) & (s0 + c["T"] - 1 >= c["F"])).any(), c["name"]
        assert any(c["counter_base"] == 2 ** 32 - 2 and c["eps"] is not None and c["T"] >= 2 for c in mine)     # the carry is drawn on
        shuffled = next(c for c in mine if c["cols"] == "shuffled")
        assert sorted(em.data(shuffled)["cols"]) != sorted(cols) and len(set(em.data(shuffled)["cols"])) == len(cols)
    assert {c["scale"] for c in cs} == {1.0, 4.0}
    for c in cs:
        d = em.data(c)
        assert float(np.abs(d["state"]).max()) <= c["scale"] and float(np.abs(d["positions"]).max()) <= c["scale"]
