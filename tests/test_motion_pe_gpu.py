"""Per-env moving scenarios on the GPU (include/macjd.h, macjd_motion_pe_io): the device frame compiler against its float64
model (tests/motion_pe_model.py), the per-env moving step against macjd_env_step on the gathered frames, the anchor to the
shared-frame moving step and the reference-generated fixture, the many-step launch and the masked reset, the host and
device compile paths, the runner and the driver."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import motion_cases as cases
import motion_pe_model as mpe
from _harness import REPO, random_actions
from test_env_gpu import TOL_REWARD
from test_nets_cpu import make_args, quiet

from macjd_amd.scenario import FOUR_PI_CUBED, MovingScenarioBatch, Scenario, motion_frame_dict, motion_pe_in_rows, tile_envs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
F = mpe.F_PE
E0, TILE = 19, 8
SIZES = [(2, 2), (3, 4), (6, 8), (3, 3)]   # three compiled sizes and a generic one
TOL_PD = 1e-12


def _env_class(tile):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return type(f"EnvTile{tile}", (BatchedElectromagneticEnvironment,), {"PE_TILE": tile})


def _pe_env(mb, tile=TILE, seed=11, **kw):
    return _env_class(tile)(moving_batch=mb, device=DEV, seed=seed, **kw)


def _env(sc, E, seed=11, **kw):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return BatchedElectromagneticEnvironment(scenario=sc, batch_envs=E, device=DEV, seed=seed, **kw)


def _diag(E, R, J):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    return {"out64": z(E, 4), "pd64": z(E, R), "snr64": z(E, R), "prj64": z(E, J)}


def _cuda(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _untile(a, E):
    """[n_tiles, ..., tile] -> [E, ...] (numpy)."""
    a = np.moveaxis(a, -1, 1)
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])[:E]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------
# 1. the compiler against the model
SENT_U8 = 0xAB
MARGIN = 4096   # elements of sentinel before and after every table


def _guarded(shape, dtype):
    """A sentinel-filled tensor of ``shape`` inside a sentinel-filled buffer with MARGIN elements on each side."""
    n = int(np.prod(shape))
    fill = SENT_U8 if dtype == torch.uint8 else float("nan")
    big = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device=DEV)
    return big, big[MARGIN:MARGIN + n].view(shape)


def _is_sentinel(t):
    return (t == SENT_U8) if t.dtype == torch.uint8 else torch.isnan(t)


def _run_compiler(scs, tile):
    from macjd_amd import _native
    lib = _native.load()
    sc0 = scs[0]
    E, R, J, Fr = len(scs), sc0.num_radars, sc0.num_jammers, sc0.episode_limit
    ins = [sc.motion_compile_inputs() for sc in scs]
    cols = np.stack([i["column"] for i in ins])
    weak = np.stack([i["weak"] for i in ins])
    in_t, in_w = _cuda(tile_envs(cols, tile), tile_envs(weak, tile))
    n_tiles = in_t.shape[0]
    assert tuple(in_t.shape) == (n_tiles, motion_pe_in_rows(R, J), tile)
    shapes = {"frames": ((n_tiles, Fr, mpe.pe_rows(R, J), tile), torch.float64),
              "flags": ((n_tiles, Fr, J * R, tile), torch.uint8),
              "snr_no": ((n_tiles, Fr, R, tile), torch.float64),
              "positions": ((n_tiles, Fr + 1, 2 * R + 2 * J, tile), torch.float32)}
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    d = _native.MotionPeCompileDesc()
    d.n_envs, d.n_radars, d.n_jammers, d.n_frames, d.tile = E, R, J, Fr, tile
    d.four_pi_cubed = FOUR_PI_CUBED
    d.pd_A, d.pd_c1, d.pd_denB = sc0.pd_consts
    d.in_tables, d.in_weak = in_t.data_ptr(), in_w.data_ptr()
    d.frames, d.frame_flags = bufs["frames"][1].data_ptr(), bufs["flags"][1].data_ptr()
    d.frame_snr_no, d.positions = bufs["snr_no"][1].data_ptr(), bufs["positions"][1].data_ptr()
    _native.check(lib.macjd_motion_pe_compile(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "macjd_motion_pe_compile")
    torch.cuda.synchronize()
    return bufs


def _check_compiler(scs, tile):
    E, R, J = len(scs), scs[0].num_radars, scs[0].num_jammers
    bufs = _run_compiler(scs, tile)
    want = mpe.model_tables(scs)
    sl = mpe.row_slices(R, J)
    n_pad = bufs["frames"][1].shape[0] * tile
    for k, (big, view) in bufs.items():
        # bytes past the tables are untouched, and so is every lane of the last tile's padding
        assert _is_sentinel(big[:MARGIN]).all() and _is_sentinel(big[-MARGIN:]).all(), k
        if n_pad > E:
            assert _is_sentinel(view[-1, ..., E - (n_pad - tile):]).all(), k
        got = _untile(view.cpu().numpy(), E)
        if k == "frames":
            pd_g, pd_w = got[..., sl["pd_no"]], want[k][..., sl["pd_no"]]
            rel = np.abs(pd_g - pd_w) / pd_w
            print(f"pd_no device vs model at {J}j/{R}r E={E}: max relative difference {float(rel.max()):.3e}")
            assert (pd_w > 0).all() and float(rel.max()) <= TOL_PD
            got, ref = got.copy(), want[k].copy()
            got[..., sl["pd_no"]] = 0.0
            ref[..., sl["pd_no"]] = 0.0
            bad = np.argwhere(_bits(got) != _bits(ref))
            assert bad.size == 0, (k, bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])
        else:
            bad = np.argwhere(_bits(got) != _bits(want[k]))
            assert bad.size == 0, (k, bad[:5])
    return want


@pytest.mark.parametrize("J,R", SIZES)
def test_compiler_against_the_model(J, R):
    """Every row bit-identical to the float64 model except pd_no (within 1e-12 relative: the device's exp is its own);
    padded lanes and the bytes around the tables keep their sentinels.  E = 19 in tiles of 8."""
    _, scs = mpe.case(J, R)
    want = _check_compiler(scs, TILE)
    assert (want["frames"][2, 2, mpe.row_slices(R, J)["denom"]][0] == -1.0) and want["flags"].any()


def test_compiler_against_the_model_across_tiles_of_256():
    """3j/4r at E = 260 with tile 256 (two tiles, the second almost empty) and F = 3."""
    _, scs = mpe.case(3, 4, E=260, limit=3)
    _check_compiler(scs, 256)


# ---------------------------------------------------------------------------------------------------------------
# 2. the single step against macjd_env_step on the gathered frames
def _gathered_reference(mb, E, **kw):
    """An env of env 0's static frame-0 scenario (same R, J, episode limit, r_p bounds, Pd constants in the handle) that
    steps through macjd_env_step on per-env tables; ``load(mv)`` makes env e's column ITS OWN frame f_e (tile width 1:
    [E, rows]) and copies ``mv``'s FSM bits, step counters and episode indices."""
    sc0 = mb.scenarios[0]
    cfg = mpe.config(sc0.episode_limit)
    # any static scenario of the shape will do: the handle supplies no table value on per-env tables
    static = Scenario.from_dict(motion_frame_dict(cases.moving_ring_dict(sc0.num_jammers, sc0.num_radars), 0), config=cfg)
    ref = _env(static, E, **kw)
    fr, fl = _cuda(mb.frames, mb.flags)   # [E, F, rows], [E, F, J*R]
    ar = torch.arange(E, device=DEV)

    def load(mv):
        f_e = torch.clamp(mv._step.to(torch.int64), min=0, max=fr.shape[1] - 1)
        ref._pe_tables, ref._pe_flags, ref._pe_tile = fr[ar, f_e].contiguous(), fl[ar, f_e].contiguous(), 1
        ref._track.copy_(mv._track); ref._step.copy_(mv._step); ref._episode.copy_(mv._episode)
        return f_e
    return ref, load


@pytest.mark.parametrize("mode", ["philox", "philox_diag", "uniforms_diag"])
@pytest.mark.parametrize("J,R", SIZES)
def test_step_bitwise_equal_to_the_per_env_step_on_gathered_frames(J, R, mode):
    """Production form (philox: float32 actions, no diagnostics) and the general all-float64 form (diagnostics; float32 and
    float64 actions on alternating steps; caller's uniforms), envs at staggered step counters including >= F."""
    _, scs = mpe.case(J, R)
    mb = MovingScenarioBatch(scs)
    E, S = E0, scs[0].state_dim
    mv = _pe_env(mb, seed=77, env_offset=1000)
    ref, load = _gathered_reference(mb, E, seed=77, env_offset=1000)
    assert mv.observation_is_static is False and mv._pe_tile == TILE
    mv.reset()
    # the state rows inside a NaN buffer, every non-position column at a sentinel value
    cols = scs[0].position_columns
    other = [c for c in range(S) if c not in cols]
    big = torch.full(((E + 2) * S,), float("nan"), device=DEV)
    rows = big[S:S + E * S].view(E, S)
    rows.copy_(mv._state_dyn)
    rows[:, other] = 12345.0
    mv._state_dyn = rows
    mv._motion_pe_io.state = rows.data_ptr()
    pos = torch.from_numpy(mb.positions).to(DEV)   # [E, F + 1, n_pos]
    ar = torch.arange(E, device=DEV)
    mv._step.copy_(torch.arange(E, dtype=torch.int32, device=DEV) % (F + 3))   # counters 0 .. F + 2
    rng = np.random.default_rng(31 * J + R)
    d_mv, d_ref = (_diag(E, R, J), _diag(E, R, J)) if mode != "philox" else (None, None)
    rsum_mv, rsum_ref = (torch.zeros((E, 3), device=DEV) for _ in range(2))
    snr_no_host = torch.from_numpy(mb.snr_no).to(DEV)
    for t in range(4):
        f_e = load(mv)
        k_before = mv._step.to(torch.int64).clone()
        Tn, Pn = random_actions(rng, E, J, R)
        u = torch.from_numpy(rng.random((E, R + J))).to(DEV) if mode == "uniforms_diag" else None
        if mode != "philox" and t % 2 == 0:
            Pn = Pn.astype(np.float64)
        Td, Pd = _cuda(Tn, Pn)
        rew, term, info = mv.step(Td, Pd, u, diag=d_mv, rdpj_sum=rsum_mv)
        rew_r, term_r, info_r = ref.step(Td, Pd, u, diag=d_ref, rdpj_sum=rsum_ref)
        assert torch.equal(rew, rew_r) and torch.equal(term, term_r), t
        assert torch.equal(mv._r_dpj, ref._r_dpj) and torch.equal(rsum_mv, rsum_ref), t
        assert torch.equal(mv._track, ref._track) and torch.equal(mv._step, ref._step), t
        assert torch.equal(info["radar_pds"], info_r["radar_pds"]), t
        assert torch.equal(info["snr_with_jamming"], info_r["snr_with_jamming"]), t
        assert torch.equal(info["snr_no_jamming"], snr_no_host[ar, f_e].to(torch.float32)), t
        if d_mv is not None:
            for k in d_mv:
                assert torch.equal(d_mv[k], d_ref[k]), (t, k)
        nxt = torch.clamp(k_before + 1, max=F)
        assert torch.equal(rows[:, cols], pos[ar, nxt]) and torch.equal(mv.positions, pos[ar, nxt]), t
        assert (rows[:, other] == 12345.0).all(), t
        assert torch.isnan(big[:S]).all() and torch.isnan(big[S + E * S:]).all(), t
    assert int(mv.step_count.max()) == F + 2 + 4 and int(mv.step_count.min()) == 4


# ---------------------------------------------------------------------------------------------------------------
# 3. anchor: the shared-frame moving step and the reference-generated fixture
@pytest.mark.parametrize("J,R", [(3, 4), (3, 3)])
def test_copies_of_one_scenario_equal_the_shared_frame_moving_step(J, R):
    sc, _ = cases.compiled(cases.moving_ring_dict(J, R), F)
    E = E0
    a = _env(sc, E, seed=5, env_offset=40)
    b = _pe_env(MovingScenarioBatch([sc] * E), seed=5, env_offset=40)
    a.reset(); b.reset()
    assert torch.equal(a.get_state(), b.get_state())
    rng = np.random.default_rng(R)
    for t in range(F + 2):
        if t == 3:
            m = torch.from_numpy((np.arange(E) % 3 == 0).astype(np.uint8)).to(DEV)
            a.reset(m); b.reset(m)
        Td, Pd = _cuda(*random_actions(rng, E, J, R))
        ra, ta, ia = a.step(Td, Pd)
        rb, tb, ib = b.step(Td, Pd)
        assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(a._r_dpj, b._r_dpj), t
        assert torch.equal(a._track, b._track) and torch.equal(a._step, b._step), t
        for k in ("radar_pds", "snr_with_jamming", "snr_no_jamming"):
            assert torch.equal(ia[k], ib[k]), (t, k)
        assert torch.equal(a.get_state(), b.get_state()), t


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_fixture_replay(mode):
    """tests/golden/env_3j4r_moving.npz (the reference stepped on moved positions) through the per-env moving step on three
    copies of its scenario: the assertions and tolerances of test_motion_gpu.py::test_fixture_trace_single_env on every
    copy, and bitwise equality with the shared-frame moving step."""
    cfg, g = cases.fixture()
    sc, _ = cases.compiled(cfg, None)
    R, J, E = sc.num_radars, sc.num_jammers, 3
    env = _pe_env(MovingScenarioBatch([sc] * E))
    shared = _env(sc, E)
    diag, diag_s = _diag(E, R, J), _diag(E, R, J)
    pre = f"{mode}_s42_"
    T, P, U = g[pre + "T"], g[pre + "P"], g[pre + "u"]
    rep = lambda a: np.repeat(a[:, None], E, axis=1)
    Td = torch.from_numpy(rep(T)).cuda()
    Pd = torch.from_numpy(rep(P.astype(np.float32) if mode == "f32" else P)).cuda()
    Ud = torch.from_numpy(rep(np.nan_to_num(U, nan=2.0))).cuda()
    got = {k: [] for k in ("out", "pd", "snr", "prj", "track", "term", "state", "snr_no")}
    env.reset(); shared.reset()
    assert env.get_state().cpu().numpy().tobytes() == np.repeat(g[pre + "obs_reset"][None], E, axis=0).tobytes()
    for t in range(T.shape[0]):
        _, term, info = env.step(Td[t], Pd[t], Ud[t], diag=diag)
        _, term_s, _ = shared.step(Td[t], Pd[t], Ud[t], diag=diag_s)
        for k in diag:
            assert torch.equal(diag[k], diag_s[k]), (t, k)
        assert torch.equal(env.get_state(), shared.get_state()) and torch.equal(term, term_s), t
        got["out"].append(diag["out64"].clone()); got["pd"].append(diag["pd64"].clone())
        got["snr"].append(diag["snr64"].clone()); got["prj"].append(diag["prj64"].clone())
        got["track"].append(info["radar_tracking"].clone()); got["term"].append(term.clone())
        got["state"].append(env.get_state().clone()); got["snr_no"].append(info["snr_no_jamming"].clone())
    for e in range(E):
        cat = lambda k: torch.stack([x[e] for x in got[k]]).cpu().numpy()
        np.testing.assert_array_equal(cat("track"), g[pre + "track"])
        np.testing.assert_array_equal(cat("term"), g[pre + "terminated"])
        ref = np.stack([g[pre + "reward"], g[pre + "r_d"], g[pre + "r_p"], g[pre + "r_j"]], axis=1)
        np.testing.assert_allclose(cat("out"), ref, rtol=0, atol=TOL_REWARD)
        np.testing.assert_allclose(cat("out"), ref, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(cat("pd"), g[pre + "pd"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(cat("snr"), g[pre + "snr_with"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(cat("prj"), g[pre + "prj"], rtol=1e-14, atol=0)
        assert cat("state").tobytes() == g[pre + "obs_after"].astype(np.float32).tobytes()
        np.testing.assert_array_equal(cat("snr_no"), g[pre + "snr_no"].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
# 4. many-step and reset
@pytest.mark.parametrize("J,R", [(2, 2), (3, 4), (6, 8)])
def test_step_many_equals_single_steps(J, R):
    _, scs = mpe.case(J, R)
    mb = MovingScenarioBatch(scs)
    E, n = E0, 4
    a, b = _pe_env(mb, seed=9), _pe_env(mb, seed=9)
    a.reset(); b.reset()
    stag = torch.arange(E, dtype=torch.int32, device=DEV) % 4   # counters 0..3: the 4 steps run frames up to F + 1 (clamped)
    a._step.copy_(stag); b._step.copy_(stag)
    rng = np.random.default_rng(n)
    Tn = rng.integers(-1, 2 * R + 3, size=(n, E, J)).astype(np.int32)
    Pn = rng.random((n, E, J)).astype(np.float32)
    Td, Pd = _cuda(Tn, Pn)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    rew_s, term_s, rdpj_s, sum_s = z(n, E), z(n, E, dt=torch.uint8), z(n, E, 3), z(E, 3)
    for t in range(n):
        a.step(Td[t], Pd[t], out_reward=rew_s[t], out_terminated=term_s[t], want_info=False, rdpj_sum=sum_s)
        rdpj_s[t] = a._r_dpj
    rew_m, term_m, rdpj_m, sum_m = z(n, E), z(n, E, dt=torch.uint8), z(n, E, 3), z(E, 3)
    b.step_many(Td, Pd, rew_m, term_m, rdpj_m, rdpj_sum=sum_m)
    assert torch.equal(rew_s, rew_m) and torch.equal(term_s, term_m) and torch.equal(rdpj_s, rdpj_m)
    assert torch.equal(sum_s, sum_m)
    assert torch.equal(a.track, b.track) and torch.equal(a.step_count, b.step_count)
    assert torch.equal(a.get_state(), b.get_state())
    pos = torch.from_numpy(mb.positions).to(DEV)
    ar = torch.arange(E, device=DEV)
    assert torch.equal(b.positions, pos[ar, torch.clamp(b.step_count.to(torch.int64), max=F)])
    assert term_m.any() and not term_m.all()


def test_masked_reset_and_refusals():
    _, scs = mpe.case(3, 3)   # generic size
    mb = MovingScenarioBatch(scs)
    E, J, R = E0, 3, 3
    env = _pe_env(mb)
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(2):
        env.step(*_cuda(*random_actions(rng, E, J, R)))
    before = env.get_state().clone()
    m = torch.from_numpy((np.arange(E) % 3 == 0).astype(np.uint8)).to(DEV)
    env.reset(m)
    keep = ~m.bool()
    cols = scs[0].position_columns
    pos = torch.from_numpy(mb.positions).to(DEV)
    assert torch.equal(env.get_state()[keep], before[keep])                       # only the masked envs are rewritten
    assert torch.equal(env.get_state()[m.bool()][:, cols], pos[m.bool(), 0])      # with their OWN frame-0 positions
    assert not torch.equal(pos[0, 0], pos[6, 0])
    assert torch.equal(env.step_count, torch.where(m.bool(), 0, 2).to(torch.int32))
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(Exception, match="production configuration at a compiled size"):
        env.step_many(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3))
    for name, call in (("frame_states", lambda: env.frame_states()),
                       ("time_step_kernel", lambda: env.time_step_kernel(z(E, J, dt=torch.int32), z(E, J), 2)),
                       ("time_step_many_kernel", lambda: env.time_step_many_kernel(
                           z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3), 2)),
                       ("episode_scan_args", env.episode_scan_args), ("episode_scan_pe_args", env.episode_scan_pe_args),
                       ("episode_moving_scan_args", env.episode_moving_scan_args)):
        with pytest.raises(RuntimeError, match=f"{name}: not available on a per-env moving scenario batch"):
            call()
    assert not env.step_many_has_production_form()
    assert env.table_bytes == mb.table_bytes(TILE)
    from macjd_amd.scenario import ScenarioBatch
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    static = Scenario.from_dict(motion_frame_dict(cases.moving_ring_dict(3, 3), 0), config=mpe.config())
    with pytest.raises(ValueError, match="moving_batch and scenario_batch are exclusive"):
        Env(moving_batch=mb, scenario_batch=ScenarioBatch([static] * E), device=DEV)
    with pytest.raises(ValueError, match="do not pass `scenario` too"):
        Env(moving_batch=mb, scenario=scs[1], device=DEV)
    with pytest.raises(ValueError, match=r"batch_envs \(4\) != scenarios in the moving batch"):
        Env(moving_batch=mb, batch_envs=4, device=DEV)
    with pytest.raises(ValueError, match="a moving scenario .* is not supported with per-env scenario batches"):   # the old one
        from types import SimpleNamespace   # (ScenarioBatch itself refuses a moving scenario: a stand-in whose base moves)
        Env(scenario_batch=SimpleNamespace(base=scs[0], n_envs=E), device=DEV)
    with pytest.raises(AttributeError, match="not a per-env moving batch"):
        _env(scs[0], 4).table_bytes


# ---------------------------------------------------------------------------------------------------------------
# 5. host and device compile paths
def test_host_and_device_compile_paths():
    base = cases.moving_ring_dict(3, 4)
    kw = dict(seed=3, config=mpe.config(), env_offset=100, velocity_jitter=1.0)
    E = E0
    host = MovingScenarioBatch.randomized(base, E, compile="host", **kw)
    dev = MovingScenarioBatch.randomized(base, E, compile="device", **kw)
    eh, ed = _pe_env(host, seed=21), _pe_env(dev, seed=21)
    sl = mpe.row_slices(4, 3)
    th = {k: _untile(eh._motion_keep[k].cpu().numpy(), E) for k in ("frames", "flags", "snr_no", "positions")}
    td = {k: _untile(ed._motion_keep[k].cpu().numpy(), E) for k in ("frames", "flags", "snr_no", "positions")}
    assert th["frames"].tobytes() == host.frames.tobytes()                        # the host path uploads its frames bit for bit
    assert td["positions"].tobytes() == th["positions"].tobytes() and td["flags"].tobytes() == th["flags"].tobytes()
    for name in ("Pn", "D", "rd_pen", "gr", "pmin", "pmax", "gj"):
        assert td["frames"][..., sl[name]].tobytes() == th["frames"][..., sl[name]].tobytes(), name
    rel = lambda a, b: float(np.max(np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))))
    assert rel(td["frames"][..., sl["GaPs"]], th["frames"][..., sl["GaPs"]]) <= 1e-13
    assert rel(td["frames"][..., sl["denom"]], th["frames"][..., sl["denom"]]) <= 1e-13
    assert rel(td["snr_no"], th["snr_no"]) <= 1e-13
    assert rel(td["frames"][..., sl["pd_no"]], th["frames"][..., sl["pd_no"]]) <= TOL_PD
    assert torch.equal(eh.get_state(), ed.get_state())
    # on identical uploaded tables the two envs step identically
    for k in ("frames", "flags", "snr_no", "positions"):
        ed._motion_keep[k].copy_(eh._motion_keep[k])
    eh.reset(); ed.reset()
    rng = np.random.default_rng(8)
    for t in range(F + 1):
        Td, Pd = _cuda(*random_actions(rng, E, 3, 4))
        rh, th_, ih = eh.step(Td, Pd)
        rd, td_, idv = ed.step(Td, Pd)
        assert torch.equal(rh, rd) and torch.equal(th_, td_) and torch.equal(eh._track, ed._track), t
        assert torch.equal(ih["radar_pds"], idv["radar_pds"]) and torch.equal(ih["snr_no_jamming"], idv["snr_no_jamming"]), t
        assert torch.equal(eh.get_state(), ed.get_state()), t


# ---------------------------------------------------------------------------------------------------------------
# 6. runner and driver
def _runner(mb, seed=5):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    env = _pe_env(mb, tile=256, seed=seed)
    info = env.get_env_info()
    E = mb.n_envs
    d = dict(J=info["n_agents"], A=info["n_actions"], S=info["state_shape"], H=64)
    args = make_args(d, device="cuda", use_cuda=True, episode_limit=info["episode_limit"], buffer_size=2 * E,
                     epsilon_start=0.6, epsilon_anneal_time=300)
    args.env_info = info
    torch.manual_seed(3)
    with quiet():
        mac = BasicMAC(info["obs_shape"], args)
        mac.cuda()
        buf = EpisodeReplayBuffer(args)
    return BatchedEpisodeRunner(env, mac, buf, args), buf


def test_graph_replayed_rollout_equals_eager():
    base = cases.moving_ring_dict(3, 4)
    E = 32
    mb = MovingScenarioBatch.randomized(base, E, seed=2, config=mpe.config(), velocity_jitter=1.0, compile="device")
    r_e, b_e = _runner(mb)
    r_g, b_g = _runner(mb)
    # the step loop only: no whole-episode launch, no three-launch rollout, no closed-loop launch
    assert not r_e._static and not r_e.hoist_static_obs and not r_e.fused_rollout_available()
    assert not r_e.moving_rollout_available()
    assert not r_e.closed_loop_available() and not r_e.closed_loop_pe_available() and not r_e.closed_loop_moving_available()
    r_g.enable_graph()
    for _ in range(2):
        r_e.run(sync_stats=True)
        r_g.run(sync_stats=True)
    assert b_e.obs_static is False and b_g.obs_static is False
    for k in b_e.buffers:
        assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
    # the stored state rows carry every env's own positions, frame by frame
    host = MovingScenarioBatch.randomized(base, E, seed=2, config=mpe.config(), velocity_jitter=1.0, compile="host")
    cols = host.base.position_columns
    pos = torch.from_numpy(host.positions).to(b_e.buffers["state"].device)
    st = b_e.buffers["state"][:2 * E]
    assert torch.equal(st[:E, :F][:, :, cols], pos[:, :F]) and torch.equal(st[E:, :F][:, :, cols], pos[:, :F])
    assert b_e.buffers["terminated"][:2 * E, F - 1].all()


def test_driver_trains_on_randomized_moving_scenarios(tmp_path):
    from macjd_amd.main import load_config, run
    with contextlib.redirect_stdout(io.StringIO()):
        cfg = load_config("default", os.path.join(PKG, "config"))
    E = 32
    cfg.device_request = "cuda"
    cfg.env_config = "scenario_3j4r_moving"
    cfg.sim_config_path = os.path.join(PKG, "config", "scenario_3j4r_moving.yaml")
    cfg.save_model_dir, cfg.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
    cfg.log_interval_seconds = 0
    cfg.gemm_tuning = False
    cfg.resume = None
    cfg.randomize_moving_scenarios = True
    cfg.randomize_velocity_jitter = 1.0
    for k, v in dict(batch_envs=E, buffer_size=2 * E, total_env_steps=2 * E * F, episode_limit=F, start_training_steps=0,
                     save_interval=10 ** 9, test_interval=10 ** 9, test_nepisodes=E, batch_size=8, lr=1e-4,
                     updates_per_rollout=4).items():
        setattr(cfg, k, v)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = run(cfg)
    assert res["total_steps"] == 2 * E * F and res["episodes"] == 2 * E and res["train_steps"] > 0
    assert "Training finished." in out.getvalue()
