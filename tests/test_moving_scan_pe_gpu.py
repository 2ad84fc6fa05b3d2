"""Per-env moving scenarios under scanning radars on the GPU (include/macjd.h, macjd_motion_scan_pe_io): the device compiler of
the beam frames against its float64 model (tests/moving_scan_pe_model.py), the step against macjd_env_step_scan_pe(_pattern) on
the gathered frames, against the float64 step model and against the shared-frame moving-scanning step, production against
general variant, the masked reset, every refusal of the entry points, the environment, the runner and the driver.

Bearing deviation of the device compiler from the model (the device library's atan2 is the one step IEEE 754 does not pin),
measured on the MI355X over all compiler cases of this file: worst 5.684e-14 degrees = 1.00 ulp of 360 in every case but
E = 1 (0.50 ulp); the pd_no rows within 2.7e-16 relative.  BEARING_WORST_DEG below holds the figure."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_cases
import moving_scan_cases as msc
import moving_scan_pe_model as spm
from _harness import REPO, random_actions
from test_nets_cpu import make_args, quiet

from macjd_amd.scenario import (DEG_PER_RAD, FOUR_PI_CUBED, MovingScanScenarioBatch, Scenario, ScenarioBatch, _scan_compile_inputs,
                                motion_frame_dict, motion_pe_in_rows, motion_scan_pe_in_rows, pe_scan_pattern_rows, pe_scan_rows,
                                tile_envs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
F = spm.F_PE
TILE = 8
TOL_PD = 1e-12
INFO_KEYS = ("r_d", "r_p", "r_j", "radar_tracking", "radar_pds", "snr_with_jamming", "snr_no_jamming")
# Worst circular deviation of a device bearing from the model's, measured on the MI355X over every compiler case below
# (in ulps of 360: 2^-44 degrees each).  The bar is four times that (argument ranges the cases do not visit) and may never
# exceed 1e-9 degrees: rounding cannot reach that, any formula error (swapped arguments, no wrap, radians) is far above it.
BEARING_WORST_DEG = 5.6843418860808015e-14
ULP_360 = 2.0 ** -44
BEARING_BAR_DEG = 4 * BEARING_WORST_DEG
assert BEARING_BAR_DEG <= 1e-9


def _env_class(tile):
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    return type(f"EnvTile{tile}", (BatchedElectromagneticEnvironment,), {"PE_TILE": tile})


def _ms_env(mb, tile=TILE, seed=11, **kw):
    return _env_class(tile)(moving_scan_batch=mb, device=DEV, seed=seed, **kw)


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


def _untile_t(t, E):
    """[n_tiles, F, rows, tile] -> [E, F, rows] (torch)."""
    return t.permute(0, 3, 1, 2).reshape(t.shape[0] * t.shape[3], t.shape[1], t.shape[2])[:E].contiguous()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _rel(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, r)))


def _third(E):
    return torch.from_numpy((np.arange(E) % 3 == 0).astype(np.uint8)).to(DEV)


@contextlib.contextmanager
def _options(monkeypatch, **kv):
    from macjd_amd import _native
    for k, v in kv.items():
        monkeypatch.setenv(k, v)
    _native.reload_options()
    try:
        yield
    finally:
        for k in kv:
            monkeypatch.delenv(k, raising=False)
        _native.reload_options()


def _base(J, R, L):
    return spm._scanning(motion_cases.moving_ring_dict(J, R), L)


JITTER = dict(velocity_jitter=2.0, position_jitter=20.0, azimuth_jitter=40.0)


# ---------------------------------------------------------------------------------------------------------------
# 1. the compilers against the model
MARGIN = 4096   # elements of sentinel before and after every table


def _guarded(shape, dtype):
    """A sentinel-filled tensor of ``shape`` inside a sentinel-filled buffer with MARGIN elements on each side."""
    n = int(np.prod(shape))
    fill = 0xAB if dtype == torch.uint8 else float("nan")
    big = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device=DEV)
    return big, big[MARGIN:MARGIN + n].view(shape)


def _run_compilers(scs, tile):
    """macjd_motion_pe_compile, then macjd_motion_scan_pe_compile on the same stream, every output table between sentinel
    margins.  Returns {name: (buffer, table view)} of the beam tables."""
    from macjd_amd import _native
    lib = _native.load()
    sc0 = scs[0]
    E, R, J, Fr, L = len(scs), sc0.num_radars, sc0.num_jammers, sc0.episode_limit, sc0.scan_pattern_levels
    ins = [sc.motion_compile_inputs() for sc in scs]
    in_t, in_w, sin = _cuda(tile_envs(np.stack([i["column"] for i in ins]), tile), tile_envs(np.stack([i["weak"] for i in ins]), tile),
                            tile_envs(np.stack([_scan_compile_inputs(sc) for sc in scs]), tile))
    n_tiles = in_t.shape[0]
    assert tuple(in_t.shape) == (n_tiles, motion_pe_in_rows(R, J), tile) and tuple(sin.shape) == (n_tiles, motion_scan_pe_in_rows(R, L), tile)
    shapes = {"frames": ((n_tiles, Fr, 6 * R + 3 * J + J * R, tile), torch.float64),
              "flags": ((n_tiles, Fr, J * R, tile), torch.uint8),
              "snr_no": ((n_tiles, Fr, R, tile), torch.float64),
              "positions": ((n_tiles, Fr + 1, 2 * R + 2 * J, tile), torch.float32),
              "scan_frames": ((n_tiles, Fr, pe_scan_rows(R, J), tile), torch.float64)}
    if L:
        shapes["pattern_frames"] = ((n_tiles, Fr, pe_scan_pattern_rows(R, L), tile), torch.float64)
    bufs = {k: _guarded(*v) for k, v in shapes.items()}
    stream = torch.cuda.current_stream().cuda_stream
    d = _native.MotionPeCompileDesc()
    d.n_envs, d.n_radars, d.n_jammers, d.n_frames, d.tile = E, R, J, Fr, tile
    d.four_pi_cubed = FOUR_PI_CUBED
    d.pd_A, d.pd_c1, d.pd_denB = sc0.pd_consts
    d.in_tables, d.in_weak = in_t.data_ptr(), in_w.data_ptr()
    d.frames, d.frame_flags = bufs["frames"][1].data_ptr(), bufs["flags"][1].data_ptr()
    d.frame_snr_no, d.positions = bufs["snr_no"][1].data_ptr(), bufs["positions"][1].data_ptr()
    _native.check(lib.macjd_motion_pe_compile(ctypes.byref(d), stream), "macjd_motion_pe_compile")
    s = _native.MotionScanPeCompileDesc()
    s.n_envs, s.n_radars, s.n_jammers, s.n_frames, s.tile, s.n_levels = E, R, J, Fr, tile, L
    s.deg_per_rad = DEG_PER_RAD
    s.pd_A, s.pd_c1, s.pd_denB = sc0.pd_consts
    s.in_tables, s.scan_in = in_t.data_ptr(), sin.data_ptr()
    s.frames, s.frame_snr_no = bufs["frames"][1].data_ptr(), bufs["snr_no"][1].data_ptr()
    s.scan_frames = bufs["scan_frames"][1].data_ptr()
    s.pattern_frames = bufs["pattern_frames"][1].data_ptr() if L else None
    _native.check(lib.macjd_motion_scan_pe_compile(ctypes.byref(s), stream), "macjd_motion_scan_pe_compile")
    torch.cuda.synchronize()
    return bufs


def _check_compilers(scs, tile):
    """Device against model: bit for bit on every row but the pd_no rows (1e-12 relative) and the bearing rows (circular,
    BEARING_BAR_DEG); padding lanes and the bytes around the tables keep their sentinels.  Returns the worst bearing deviation."""
    E, R, J, L = len(scs), scs[0].num_radars, scs[0].num_jammers, scs[0].scan_pattern_levels
    bufs = _run_compilers(scs, tile)
    want = spm.model_tables(scs, first="model")
    n_pad = bufs["frames"][1].shape[0] * tile
    for k, (big, view) in bufs.items():
        sent = (lambda t: t == 0xAB) if view.dtype == torch.uint8 else torch.isnan
        assert sent(big[:MARGIN]).all() and sent(big[-MARGIN:]).all(), k
        if n_pad > E:
            assert sent(view[-1, ..., E - (n_pad - tile):]).all(), k
    ss, ps = spm.scan_slices(R, J), spm.pattern_slices(R, L)
    got = _untile(bufs["scan_frames"][1].cpu().numpy(), E).copy()
    ref = want["scan_frames"].copy()
    assert not np.isnan(got).any()
    worst = 0.0
    for name in ("bear_tgt", "bear_jam"):
        assert ((got[..., ss[name]] >= 0.0) & (got[..., ss[name]] <= 360.0)).all(), name
        worst = max(worst, float(spm.circular(got[..., ss[name]], ref[..., ss[name]]).max()))
        got[..., ss[name]] = ref[..., ss[name]] = 0.0
    pd_rel = _rel(got[..., ss["pd_no_side"]], ref[..., ss["pd_no_side"]])
    got[..., ss["pd_no_side"]] = ref[..., ss["pd_no_side"]] = 0.0
    bad = np.argwhere(_bits(got) != _bits(ref))
    assert bad.size == 0, ("scan_frames", bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])
    if L:
        got = _untile(bufs["pattern_frames"][1].cpu().numpy(), E).copy()
        ref = want["pattern_frames"].copy()
        assert not np.isnan(got).any()
        pd_rel = max(pd_rel, _rel(got[..., ps["pd_no_lvl"]], ref[..., ps["pd_no_lvl"]]))
        got[..., ps["pd_no_lvl"]] = ref[..., ps["pd_no_lvl"]] = 0.0
        bad = np.argwhere(_bits(got) != _bits(ref))
        assert bad.size == 0, ("pattern_frames", bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])
    print(f"BEARING {J}j/{R}r L={L} E={E} tile={tile}: worst circular deviation {worst:.6e} deg = {worst / ULP_360:.2f} ulp(360); "
          f"pd rows max relative {pd_rel:.3e}")
    assert pd_rel <= TOL_PD
    assert worst <= BEARING_BAR_DEG, (worst, worst / ULP_360)
    return worst


@pytest.mark.parametrize("J,R,L", spm.CASES)
def test_compilers_against_the_model(J, R, L):
    """E = 19 in tiles of 4: the last tile is padded."""
    _, scs = spm.case(J, R, L)
    _check_compilers(scs, 4)


def test_compilers_against_the_model_across_tiles_of_256():
    """3j/4r, L = 4 at E = 300 with tile 256: a second tile, blocks of 256 lanes, padding lanes."""
    _, scs = spm.case(3, 4, 4, E=300)
    _check_compilers(scs, 256)


def test_compilers_against_the_model_one_env():
    _, scs = spm.case(3, 4, 4, E=1)
    _check_compilers(scs, 1)


# ---------------------------------------------------------------------------------------------------------------
# 2. the step against macjd_env_step_scan_pe(_pattern) on the gathered frames
def _batch(J, R, L, E, compiled):
    """(batch, a static scanning scenario of its shape).  host: the case table's envs; device: jittered variations whose frames
    only the two device compilers make."""
    cfg = spm.config()
    if compiled == "host":
        dicts, scs = spm.case(J, R, L, E=E)
        return MovingScanScenarioBatch(scs), Scenario.from_dict(motion_frame_dict(dicts[0], 0), config=cfg)
    base = _base(J, R, L)
    mb = MovingScanScenarioBatch.randomized(base, E, seed=5, config=cfg, env_offset=3, compile="device", **JITTER)
    return mb, Scenario.from_dict(motion_frame_dict(base, 0), config=cfg)


def _gathered_reference(mv, static, E, L, **kw):
    """A per-env scanning env of E copies of ``static`` (same R, J, episode limit, r_p bounds, Pd constants in the handle) that
    steps through macjd_env_step_scan_pe(_pattern); ``load()`` makes env e's columns ITS OWN frame f_e, read back from ``mv``'s
    device tables (tile width 1: [E, rows]), and copies ``mv``'s beams, FSM bits, step counters and episode indices."""
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment
    ref = BatchedElectromagneticEnvironment(scenario_batch=ScenarioBatch([static] * E, scan=True, pattern=bool(L)), device=DEV, **kw)
    keep = mv._motion_keep
    fr, fl, sf = (_untile_t(keep[k], E) for k in ("frames", "flags", "scan_frames"))
    pf = _untile_t(keep["pattern_frames"], E) if L else None
    sn = _untile_t(keep["snr_no"], E)
    ar = torch.arange(E, device=DEV)

    def load():
        f_e = torch.clamp(mv._step.to(torch.int64), min=0, max=fr.shape[1] - 1)
        ref._pe_tables, ref._pe_flags, ref._pe_tile = fr[ar, f_e].contiguous(), fl[ar, f_e].contiguous(), 1
        ref._scan_pe_tables = sf[ar, f_e].contiguous()
        ref._scan_pe_io.tables = ref._scan_pe_tables.data_ptr()
        if L:
            ref._scan_pe_pattern_tables = pf[ar, f_e].contiguous()
            ref._scan_pe_pattern_io.tables = ref._scan_pe_pattern_tables.data_ptr()
        ref._track.copy_(mv._track); ref._step.copy_(mv._step); ref._episode.copy_(mv._episode)
        ref._theta_a.copy_(mv._theta_a)
        return f_e
    return ref, load, sn


@pytest.mark.parametrize("compiled", ["host", "device"])
@pytest.mark.parametrize("mode", ["philox", "philox_diag", "uniforms_diag"])
@pytest.mark.parametrize("E", [1, 65, 257])
@pytest.mark.parametrize("J,R,L", [(J, R, L) for (J, R) in spm.SIZES for L in (0, 4)])
def test_step_bitwise_equal_to_the_per_env_scanning_step_on_gathered_frames(J, R, L, E, mode, compiled):
    """Production form (philox: float32 actions, no diagnostics) and the general all-float64 form (diagnostics; float32 and
    float64 actions on alternating steps; caller's uniforms), envs at staggered step counters across the F - 1 clamp."""
    mb, static = _batch(J, R, L, E, compiled)
    sc = mb.base
    S = sc.state_dim
    mv = _ms_env(mb, seed=77, env_offset=1000)
    assert mv._motion_scan_pe_io is not None and mv._motion_scan_pe_io.n_levels == L and mv.observation_is_static is False
    ref, load, snr_no = _gathered_reference(mv, static, E, L, seed=77, env_offset=1000)
    assert (ref._scan_pe_pattern_io is not None) == bool(L)
    mv.reset()
    # the state rows inside a NaN buffer, every column the step does not own at a sentinel value
    pcols, tcols = list(sc.position_columns), list(sc.theta_a_columns)
    other = [c for c in range(S) if c not in pcols and c not in tcols]
    big = torch.full(((E + 2) * S,), float("nan"), device=DEV)
    rows = big[S:S + E * S].view(E, S)
    rows.copy_(mv._state_dyn)
    rows[:, other] = 12345.0
    mv._state_dyn = rows
    mv._motion_pe_io.state = mv._scan_io.state = rows.data_ptr()
    pos = _untile_t(mv._motion_keep["positions"], E)   # [E, F + 1, n_pos]
    ar = torch.arange(E, device=DEV)
    mv._step.copy_(torch.arange(E, dtype=torch.int32, device=DEV) % (F + 3))   # counters 0 .. F + 2
    rng = np.random.default_rng(31 * J + R + E)
    d_mv, d_ref = (_diag(E, R, J), _diag(E, R, J)) if mode != "philox" else (None, None)
    rsum_mv, rsum_ref = (torch.zeros((E, 3), device=DEV) for _ in range(2))
    for t in range(3):
        f_e = load()
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
        assert torch.equal(mv._theta_a, ref._theta_a), t
        for k in INFO_KEYS:
            assert torch.equal(info[k], info_r[k]), (t, k)
        if d_mv is not None:
            for k in d_mv:
                assert torch.equal(d_mv[k], d_ref[k]), (t, k)
        nxt = torch.clamp(k_before + 1, max=F)
        assert torch.equal(rows[:, tcols], mv.beam_azimuth.to(torch.float32)), t
        assert torch.equal(rows[:, tcols], ref.get_state()[:, tcols]), t
        assert torch.equal(rows[:, pcols], pos[ar, nxt]) and torch.equal(mv.positions, pos[ar, nxt]), t
        assert (rows[:, other] == 12345.0).all(), t
        assert torch.isnan(big[:S]).all() and torch.isnan(big[S + E * S:]).all(), t
        del f_e
    assert int(mv.step_count.max()) == min(E - 1, F + 2) + 3 and int(mv.step_count.min()) == 3
    del snr_no


# ---------------------------------------------------------------------------------------------------------------
# 3. the step against the float64 model, one model per env
@pytest.mark.parametrize("J,R,L", spm.STEP_MODEL_CASES)
def test_step_vs_model(J, R, L):
    """Supplied uniforms, float64 actions, float64 diagnostics (the general variants, (3,3): the generic-size kernel) on the
    per-env model run of tests/moving_scan_pe_model.py.  Tolerances of tests/test_moving_scan_gpu.py::test_kernel_vs_model."""
    steps, _ = spm.step_model_run(J, R, L)
    E = spm.STEP_MODEL["E"]
    _, scs = spm.case(J, R, L, E=E)
    mb = MovingScanScenarioBatch(scs)
    env = _ms_env(mb)
    env.reset()
    dg = _diag(E, R, J)
    sc = mb.base
    ar = np.arange(E)
    for t, (T, P, u, o) in enumerate(steps):
        _, term, info = env.step(*_cuda(T, P, u), diag=dg)
        np.testing.assert_array_equal(info["radar_tracking"].cpu().numpy().astype(bool), o["track"])
        np.testing.assert_array_equal(term.cpu().numpy(), o["terminated"])
        assert env.beam_azimuth.cpu().numpy().tobytes() == o["theta_a"].tobytes(), t
        np.testing.assert_array_equal(info["snr_no_jamming"].cpu().numpy(), o["snr_no"].astype(np.float32))
        np.testing.assert_allclose(dg["pd64"].cpu().numpy(), o["pd"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["snr64"].cpu().numpy(), o["snr"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["prj64"].cpu().numpy(), o["prj"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dg["out64"].cpu().numpy(), o["out"], rtol=0, atol=1e-9)
        assert env.positions.cpu().numpy().tobytes() == mb.positions[ar, min(t + 1, F)].tobytes(), t
        assert env.get_state()[:, sc.theta_a_columns].cpu().numpy().tobytes() == o["theta_a"].astype(np.float32).tobytes(), t


# ---------------------------------------------------------------------------------------------------------------
# 4. copies of one scenario: the shared-frame moving-scanning step
@pytest.mark.parametrize("J,R,pattern", [(3, 4, False), (3, 4, True), (3, 3, True)])
def test_copies_of_one_scenario_equal_the_shared_frame_moving_scanning_step(J, R, pattern):
    sc = Scenario.from_dict(msc.moving_scan_dict(J, R, pattern), config=spm.config())
    E = 19
    a = _env(sc, E, seed=5, env_offset=40)
    b = _ms_env(MovingScanScenarioBatch([sc] * E), seed=5, env_offset=40)
    assert a._motion_scan_io is not None and b._motion_scan_pe_io is not None
    a.reset(); b.reset()
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.beam_azimuth, b.beam_azimuth)
    rng = np.random.default_rng(R)
    for t in range(F + 2):
        if t == 3:
            a.reset(_third(E)); b.reset(_third(E))
        Td, Pd = _cuda(*random_actions(rng, E, J, R))
        ra, ta, ia = a.step(Td, Pd)
        rb, tb, ib = b.step(Td, Pd)
        assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(a._r_dpj, b._r_dpj), t
        assert torch.equal(a._track, b._track) and torch.equal(a._step, b._step), t
        for k in INFO_KEYS:
            assert torch.equal(ia[k], ib[k]), (t, k)
        assert torch.equal(a.beam_azimuth, b.beam_azimuth) and torch.equal(a.get_state(), b.get_state()), t
    assert a.track.any()


# ---------------------------------------------------------------------------------------------------------------
# 5. production variant == general variant
@pytest.mark.parametrize("J,R,L", [(J, R, L) for (J, R) in ((2, 2), (3, 4), (6, 8)) for L in (0, 4)])
def test_production_variant_equals_general_variant(J, R, L):
    """The production (FAST) variant == the general one (selected by asking for the diagnostics), bitwise."""
    E = 65
    mb, _ = _batch(J, R, L, E, "host")
    fast, general = _ms_env(mb, seed=5, env_offset=64), _ms_env(mb, seed=5, env_offset=64)
    fast.reset(); general.reset()
    rng = np.random.default_rng(R)
    diag = _diag(E, R, J)
    for t in range(F + 2):
        if t == 3:
            fast.reset(_third(E)); general.reset(_third(E))
        Td, Pd = _cuda(*random_actions(rng, E, J, R))
        r1, t1, i1 = fast.step(Td, Pd)
        r2, t2, i2 = general.step(Td, Pd, diag=diag)
        assert torch.equal(r1, r2) and torch.equal(t1, t2), t
        for k in INFO_KEYS:
            assert torch.equal(i1[k], i2[k]), (t, k)
        assert torch.equal(fast.beam_azimuth, general.beam_azimuth) and torch.equal(fast.get_state(), general.get_state()), t
    assert fast.track.any() and not fast.track.all()


# ---------------------------------------------------------------------------------------------------------------
# 6. masked reset
def test_masked_reset_returns_only_the_masked_envs_to_their_own_frame_0():
    J, R, L, E = 3, 3, 4, 19   # generic size
    mb, _ = _batch(J, R, L, E, "host")
    sc = mb.base
    env = _ms_env(mb)
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(2):
        env.step(*_cuda(*random_actions(rng, E, J, R)))
    before, az_before = env.get_state().clone(), env.beam_azimuth.clone()
    m = _third(E)
    env.reset(m)
    sel, keep = m.bool(), ~m.bool()
    pos = torch.from_numpy(mb.positions).to(DEV)
    az0 = torch.from_numpy(np.ascontiguousarray(mb.scan_frames[:, 0, 3 * R:4 * R])).to(DEV)   # every env's own frame-0 az0
    assert torch.equal(env.get_state()[keep], before[keep]) and torch.equal(env.beam_azimuth[keep], az_before[keep])
    assert torch.equal(env.get_state()[sel][:, sc.position_columns], pos[sel, 0])
    assert torch.equal(env.beam_azimuth[sel], az0[sel])
    assert torch.equal(env.get_state()[sel][:, sc.theta_a_columns], az0[sel].to(torch.float32))
    assert not torch.equal(pos[0, 0], pos[6, 0]) and not torch.equal(az0[6], az0[9])
    assert not torch.equal(az_before[keep], az0[keep])                               # the beams had moved
    assert torch.equal(env.step_count, torch.where(sel, 0, 2).to(torch.int32))
    assert not env.track[sel].any()


# ---------------------------------------------------------------------------------------------------------------
# 7. every refusal of the entry points
def test_entry_point_refusals_leave_the_outputs_untouched():
    from macjd_amd import _native
    J, R, L, E = 3, 4, 4, 19
    mb, static = _batch(J, R, L, E, "host")
    env = _ms_env(mb)
    env.reset()
    T, P = random_actions(np.random.default_rng(0), E, J, R)
    env.step(*_cuda(T, P))                           # fills env._io with a valid call's arguments
    lib, stream = _native.load(), torch.cuda.current_stream().cuda_stream
    io_, mp, si, ms, h = env._io, env._motion_pe_io, env._scan_io, env._motion_scan_pe_io, env._handle.ptr
    ref = lambda x: ctypes.byref(x) if x is not None else None
    step = lambda io=io_, mp=mp, si=si, ms=ms, h=h: lib.macjd_env_step_moving_scan_pe(h, ref(io), ref(mp), ref(si), ref(ms), stream)
    reset = lambda si=si, ms=ms, h=h, n=E, nf=F, tile=TILE: lib.macjd_env_reset_moving_scan_pe(h, n, ref(si), ref(ms), nf, tile, None,
                                                                                            stream)
    err = lambda: lib.macjd_last_error().decode()
    copy_of = lambda x: type(x).from_buffer_copy(x)
    torch.cuda.synchronize()
    snapshot = lambda: [t.clone() for t in (env._reward, env._r_dpj, env._step, env._track, env._theta_a, env._state_dyn,
                                            env._snr_no_step, env._pd, env._terminated)]
    before = snapshot()

    def mpe(**kw):
        x = copy_of(mp)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def msio(scan=ms.scan_frames, pattern=ms.pattern_frames, n_levels=L):
        x = _native.MotionScanPeIO()
        x.scan_frames, x.pattern_frames, x.n_levels = scan, pattern, n_levels
        return x
    with torch.cuda.device(DEV):
        no_scan = _native.ScenarioHandle(Scenario.from_dict(motion_cases.moving_ring_dict(J, R), config=spm.config()))
        pat2 = _native.ScenarioHandle(Scenario.from_dict(motion_frame_dict(_base(J, R, 1), 0), config=spm.config()))
        plain = _native.ScenarioHandle(Scenario.from_dict(motion_frame_dict(_base(J, R, 0), 0), config=spm.config()))
    checks = [
        (lambda: step(io=None), "NULL"), (lambda: step(mp=None), "NULL scenario / motion io"), (lambda: step(si=None), "NULL scan io"),
        (lambda: step(ms=None), "scan_frames"), (lambda: step(ms=msio(scan=None)), "scan_frames"),
        (lambda: step(mp=mpe(frames=None)), "is NULL"), (lambda: step(mp=mpe(frame_flags=None)), "is NULL"),
        (lambda: step(mp=mpe(positions=None)), "is NULL"), (lambda: step(mp=mpe(position_columns=None)), "is NULL"),
        (lambda: step(mp=mpe(state=None)), "is NULL"),
        (lambda: step(mp=mpe(n_frames=0)), "n_frames < 1"), (lambda: step(mp=mpe(tile=0)), "tile < 1"),
        (lambda: step(mp=mpe(n_pos=2 * R + 2 * J - 1)), "n_pos must equal 2R + 2J"),
        (lambda: step(h=no_scan.ptr), "no scanning tables"), (lambda: step(h=pat2.ptr), "n_levels differs"),
        (lambda: step(ms=msio(n_levels=-1)), "n_levels outside 0..MACJD_MAX_PATTERN_LEVELS"),
        (lambda: step(ms=msio(n_levels=7)), "n_levels outside 0..MACJD_MAX_PATTERN_LEVELS"),
        (lambda: step(ms=msio(n_levels=0)), "go together"), (lambda: step(ms=msio(pattern=None)), "go together"),
        (lambda: reset(ms=None), "scan_frames"), (lambda: reset(si=None), "NULL scan io"), (lambda: reset(nf=0), "n_frames < 1"),
        (lambda: reset(tile=0), "tile < 1"), (lambda: reset(n=-1), "bad argument"), (lambda: reset(h=no_scan.ptr), "no scanning tables"),
        (lambda: reset(h=pat2.ptr), "n_levels differs"), (lambda: reset(ms=msio(n_levels=9)), "n_levels outside"),
        (lambda: reset(ms=msio(pattern=None)), "go together"),
    ]
    for i, (call, msg) in enumerate(checks):
        rc = call()
        assert rc < 0 and msg in err(), (i, rc, err())
    with_pe = copy_of(io_)
    with_pe.pe_tables, with_pe.pe_flags, with_pe.pe_stride = mp.frames, mp.frame_flags, E
    assert step(io=with_pe) == -1 and "pe_tables must be NULL" in err()
    assert step(mp=mpe(snr_no=env._snr_no_step.data_ptr(), sn_se=1, sn_sx=E)) == -1 and "motion_pe->snr_no must be NULL" in err()
    other = torch.zeros_like(env._state_dyn)
    two_states = copy_of(si)
    two_states.state = other.data_ptr()
    assert step(si=two_states) == -1 and "scan->state and motion_pe->state" in err()
    slot = copy_of(io_)
    slot.flags = _native.STEP_SLOT_KERNEL
    assert step(io=slot) == -4 and "slot" in err()
    # the compiler
    comp = lambda d: lib.macjd_motion_scan_pe_compile(ref(d), stream)
    good = _native.MotionScanPeCompileDesc()
    keep = env._motion_keep
    ins = _cuda(tile_envs(np.stack([sc.motion_compile_inputs()["column"] for sc in mb.scenarios]), TILE),
                tile_envs(np.stack([_scan_compile_inputs(sc) for sc in mb.scenarios]), TILE))
    good.n_envs, good.n_radars, good.n_jammers, good.n_frames, good.tile, good.n_levels = E, R, J, F, TILE, L
    good.deg_per_rad = DEG_PER_RAD
    good.pd_A, good.pd_c1, good.pd_denB = mb.base.pd_consts
    good.in_tables, good.scan_in = ins[0].data_ptr(), ins[1].data_ptr()
    good.frames, good.frame_snr_no = keep["frames"].data_ptr(), keep["snr_no"].data_ptr()
    out_s, out_p = torch.full_like(keep["scan_frames"], float("nan")), torch.full_like(keep["pattern_frames"], float("nan"))
    good.scan_frames, good.pattern_frames = out_s.data_ptr(), out_p.data_ptr()

    def desc(**kw):
        x = copy_of(good)
        for k, v in kw.items():
            setattr(x, k, v)
        return x
    assert comp(None) == -1 and "NULL descriptor" in err()
    for kw, msg in ((dict(n_radars=0), "out of range"), (dict(n_jammers=99), "out of range"), (dict(n_levels=7), "n_levels outside"),
                    (dict(n_levels=-1), "n_levels outside"), (dict(n_frames=0), "n_frames"), (dict(tile=0), "tile >= 1"),
                    (dict(n_envs=-1), "n_envs >= 0"), (dict(in_tables=None), "is NULL"), (dict(scan_in=None), "is NULL"),
                    (dict(frames=None), "is NULL"), (dict(frame_snr_no=None), "is NULL"), (dict(scan_frames=None), "is NULL"),
                    (dict(pattern_frames=None), "go together"), (dict(n_levels=0), "go together")):
        assert comp(desc(**kw)) == -1 and msg in err(), (kw, err())
    torch.cuda.synchronize()
    assert torch.isnan(out_s).all() and torch.isnan(out_p).all()
    for a, b in zip(before, snapshot()):
        assert torch.equal(a, b)
    # ... and the accepted variants: a pattern-free handle takes the levels from the call; the theta_a columns are optional;
    # the pattern-free step runs on the same frames; the compiler reproduces the uploaded host tables' copied rows
    assert step(h=plain.ptr) == 0
    no_state = copy_of(si)
    no_state.state = None
    assert step(si=no_state) == 0
    assert step(h=plain.ptr, ms=msio(pattern=None, n_levels=0)) == 0
    assert reset() == 0
    assert comp(good) == 0
    torch.cuda.synchronize()
    assert torch.equal(_untile_t(out_s, E)[:, :, :4 * R], _untile_t(keep["scan_frames"], E)[:, :, :4 * R])
    assert torch.isnan(out_s[-1, ..., E - (out_s.shape[0] - 1) * TILE:]).all()            # the padding lanes stay untouched
    del static


# ---------------------------------------------------------------------------------------------------------------
# 8. the environment
def test_environment_host_and_device_batches():
    J, R, L, E = 3, 4, 4, 19
    base = _base(J, R, L)
    kw = dict(seed=3, config=spm.config(), env_offset=100, **JITTER)
    host = MovingScanScenarioBatch.randomized(base, E, compile="host", **kw)
    dev = MovingScanScenarioBatch.randomized(base, E, compile="device", **kw)
    eh, ed = _ms_env(host, seed=21), _ms_env(dev, seed=21)
    assert eh.table_bytes == host.table_bytes(TILE) == ed.table_bytes == dev.table_bytes(TILE)
    names = ("frames", "flags", "snr_no", "positions", "scan_frames", "pattern_frames")
    th = {k: _untile(eh._motion_keep[k].cpu().numpy(), E) for k in names}
    td = {k: _untile(ed._motion_keep[k].cpu().numpy(), E) for k in names}
    assert th["scan_frames"].tobytes() == host.scan_frames.tobytes() and th["pattern_frames"].tobytes() == host.pattern_frames.tobytes()
    ss, ps = spm.scan_slices(R, J), spm.pattern_slices(R, L)
    for name in ("half_beam", "sweep", "sweep_mod", "az0", "gr_side"):
        assert td["scan_frames"][..., ss[name]].tobytes() == th["scan_frames"][..., ss[name]].tobytes(), name
    for name in ("bear_tgt", "bear_jam"):
        assert float(spm.circular(td["scan_frames"][..., ss[name]], th["scan_frames"][..., ss[name]]).max()) <= BEARING_BAR_DEG
    for name in ("GaPs_side", "snr_no", "snr_no_side"):   # through the first compiler's GaPs: within the project's 1e-13
        assert _rel(td["scan_frames"][..., ss[name]], th["scan_frames"][..., ss[name]]) <= 1e-13, name
    assert _rel(td["scan_frames"][..., ss["pd_no_side"]], th["scan_frames"][..., ss["pd_no_side"]]) <= TOL_PD
    assert td["pattern_frames"][..., ps["inv_width"]].tobytes() == th["pattern_frames"][..., ps["inv_width"]].tobytes()
    assert td["pattern_frames"][..., ps["gr_lvl"]].tobytes() == th["pattern_frames"][..., ps["gr_lvl"]].tobytes()
    assert _rel(td["pattern_frames"][..., ps["GaPs_lvl"]], th["pattern_frames"][..., ps["GaPs_lvl"]]) <= 1e-13
    assert _rel(td["pattern_frames"][..., ps["pd_no_lvl"]], th["pattern_frames"][..., ps["pd_no_lvl"]]) <= TOL_PD
    assert torch.equal(eh.get_state(), ed.get_state()) and torch.equal(eh.beam_azimuth, ed.beam_azimuth)
    # the device-compiled env steps; on identical tables the two envs step identically
    for k in names:
        ed._motion_keep[k].copy_(eh._motion_keep[k])
    eh.reset(); ed.reset()
    rng = np.random.default_rng(8)
    for t in range(F + 1):
        Td, Pd = _cuda(*random_actions(rng, E, J, R))
        rh, th_, ih = eh.step(Td, Pd)
        rd, td_, idv = ed.step(Td, Pd)
        assert torch.equal(rh, rd) and torch.equal(th_, td_) and torch.equal(eh._track, ed._track), t
        for k in INFO_KEYS:
            assert torch.equal(ih[k], idv[k]), (t, k)
        assert torch.equal(eh.get_state(), ed.get_state()) and torch.isfinite(rh).all(), t
    assert tuple(eh.positions.shape) == (E, 2 * R + 2 * J) and tuple(eh.beam_azimuth.shape) == (E, R)


def test_each_env_equals_a_single_scenario_environment_of_its_own_scenario(monkeypatch):
    """Same actions and uniforms; bit for bit in the all-float64 form (MACJD_ENV_PD32=0)."""
    J, R, L, E = 3, 4, 4, 6
    host = MovingScanScenarioBatch.randomized(_base(J, R, L), E, seed=9, config=spm.config(), compile="host", **JITTER)
    with _options(monkeypatch, MACJD_ENV_PD32="0"):
        env = _ms_env(host, seed=4)
        singles = [_env(sc, 1, seed=4) for sc in host.scenarios]
        env.reset()
        for s in singles:
            s.reset()
        rng = np.random.default_rng(12)
        dg, dgs = _diag(E, R, J), [_diag(1, R, J) for _ in range(E)]
        for t in range(F + 2):
            T, P = random_actions(rng, E, J, R)
            u = rng.random((E, R + J))
            Td, Pd, ud = _cuda(T, P, u)
            rew, term, info = env.step(Td, Pd, ud, diag=dg)
            for e, s in enumerate(singles):
                r1, t1, i1 = s.step(Td[e:e + 1], Pd[e:e + 1], ud[e:e + 1], diag=dgs[e])
                assert torch.equal(rew[e:e + 1], r1) and torch.equal(term[e:e + 1], t1), (t, e)
                for k in INFO_KEYS:
                    assert torch.equal(info[k][e:e + 1], i1[k]), (t, e, k)
                for k in dg:
                    assert torch.equal(dg[k][e:e + 1], dgs[e][k]), (t, e, k)
                assert torch.equal(env.beam_azimuth[e:e + 1], s.beam_azimuth), (t, e)
                assert torch.equal(env.get_state()[e:e + 1], s.get_state()), (t, e)
        assert env.track.any()


def test_environment_refusals():
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    J, R, L, E = 3, 4, 4, 19
    mb, static = _batch(J, R, L, E, "host")
    env = _ms_env(mb)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    for name, call in (("step_many", lambda: env.step_many(z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8),
                                                           z(4, E, 3))),
                       ("frame_states", lambda: env.frame_states()), ("frame_positions", lambda: env.frame_positions()),
                       ("time_step_kernel", lambda: env.time_step_kernel(z(E, J, dt=torch.int32), z(E, J), 2)),
                       ("time_step_many_kernel", lambda: env.time_step_many_kernel(
                           z(4, E, J, dt=torch.int32), z(4, E, J), z(4, E), z(4, E, dt=torch.uint8), z(4, E, 3), 2)),
                       ("episode_scan_args", env.episode_scan_args), ("episode_scan_pe_args", env.episode_scan_pe_args),
                       ("episode_moving_scan_args", env.episode_moving_scan_args),
                       ("episode_moving_pe_args", env.episode_moving_pe_args)):
        with pytest.raises(RuntimeError, match=f"{name}: not available on a per-env moving scanning scenario batch"):
            call()
    assert not env.step_many_has_production_form()
    from macjd_amd.scenario import MovingScenarioBatch
    plain = MovingScenarioBatch([Scenario.from_dict(motion_cases.moving_ring_dict(J, R), config=spm.config())] * E)
    with pytest.raises(ValueError, match="moving_scan_batch and moving_batch are exclusive"):
        Env(moving_scan_batch=mb, moving_batch=plain, device=DEV)
    with pytest.raises(ValueError, match="moving_scan_batch and scenario_batch are exclusive"):
        Env(moving_scan_batch=mb, scenario_batch=ScenarioBatch([static] * E, scan=True, pattern=True), device=DEV)
    with pytest.raises(ValueError, match="do not pass `scenario` too"):
        Env(moving_scan_batch=mb, scenario=mb.scenarios[1], device=DEV)
    with pytest.raises(ValueError, match=r"batch_envs \(4\) != scenarios in the moving scanning batch"):
        Env(moving_scan_batch=mb, batch_envs=4, device=DEV)
    with pytest.raises(AttributeError, match="not a per-env moving batch"):
        _env(mb.scenarios[0], 4).table_bytes


# ---------------------------------------------------------------------------------------------------------------
# 9. runner, learner, driver
SWITCHES = ("closed_loop_rollout", "moving_episode_rollout", "closed_loop_moving_rollout", "moving_pe_episode_rollout")
T_RUN = 6


def _runner(mb, seed=5):
    from macjd_amd.core.mac import BasicMAC
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner
    from macjd_amd.utils.replay_buffer import EpisodeReplayBuffer
    env = _ms_env(mb, tile=256, seed=seed)
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
    return BatchedEpisodeRunner(env, mac, buf, args), buf, args


def test_graph_replayed_rollout_equals_eager_with_every_switch_on_and_the_learner_trains():
    from macjd_amd.core.qmix import QMixLearner
    E = 8
    mb = MovingScanScenarioBatch.randomized(_base(3, 4, 4), E, seed=2, config=spm.config(T_RUN), compile="device", **JITTER)
    r_e, b_e, args = _runner(mb)
    r_g, b_g, _ = _runner(mb)
    r_s, b_s, _ = _runner(mb)
    for name in SWITCHES:
        setattr(r_s, name, True)                        # every rollout switch on: still the step loop
    for r in (r_e, r_s):
        assert not r._static and not r.hoist_static_obs
        assert not r.fused_rollout_available() and not r.closed_loop_available() and not r.closed_loop_pe_available()
        assert not r.closed_loop_moving_available() and not r.moving_rollout_available() and not r.moving_pe_rollout_available()
    for name in ("rollout_closed_loop", "rollout_closed_loop_pe", "rollout_closed_loop_moving", "rollout_moving", "rollout_moving_pe"):
        with pytest.raises(RuntimeError, match="not available"):
            getattr(r_s, name)()
    r_g.enable_graph()
    for _ in range(2):
        r_e.run(sync_stats=True)
        r_g.run(sync_stats=True)
        r_s.run(sync_stats=True)
    assert b_e.obs_static is False and b_g.obs_static is False
    for k in b_e.buffers:
        assert torch.equal(b_e.buffers[k], b_g.buffers[k]), k
        assert torch.equal(b_e.buffers[k], b_s.buffers[k]), k
    # the stored state rows carry every env's own positions frame by frame, and beams that moved
    env = r_e.env
    pcols, tcols = mb.base.position_columns, mb.base.theta_a_columns
    pos = _untile_t(env._motion_keep["positions"], E).to(b_e.buffers["state"].device)
    st = b_e.buffers["state"][:2 * E]
    assert torch.equal(st[:E, :T_RUN][:, :, pcols], pos[:, :T_RUN]) and torch.equal(st[E:, :T_RUN][:, :, pcols], pos[:, :T_RUN])
    assert b_e.buffers["terminated"][:2 * E, T_RUN - 1].all()
    assert torch.unique(st[:, :T_RUN, tcols[1]]).numel() > E
    with quiet():
        learner = QMixLearner(r_e.mac, args)
    stats = learner.train(b_e.sample(8), {})
    assert np.isfinite(float(stats["loss"])) and np.isfinite(float(stats["grad_norm"]))


def test_driver_trains_on_randomized_moving_scanning_scenarios_in_a_fresh_process(tmp_path):
    """``python -m macjd_amd.main --env-config scenario_3j4r_moving_scan --randomize-moving-scan-scenarios
    --randomize-velocity-jitter 1.0`` in a fresh child process: a handful of episodes, some updates, exit status 0."""
    import shutil
    import yaml
    cfg_dir = tmp_path / "config"
    cfg_dir.mkdir()
    with open(os.path.join(PKG, "config", "default.yaml")) as f:
        cfg = yaml.safe_load(f)
    E, Fd = 16, 8
    cfg.update(batch_envs=E, buffer_size=2 * E, total_env_steps=2 * E * Fd, episode_limit=Fd, start_training_steps=0, batch_size=8,
               updates_per_rollout=2, updates_per_graph=2, save_interval=10 ** 9, test_interval=0, gemm_tuning=False,
               log_interval_seconds=0, save_model_dir=str(tmp_path / "models"), results_path=str(tmp_path / "logs"), lr=1e-4)
    with open(cfg_dir / "default.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    shutil.copy(os.path.join(PKG, "config", "scenario_3j4r_moving_scan.yaml"), cfg_dir / "scenario_3j4r_moving_scan.yaml")
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-m", "macjd_amd.main", "--config-dir", str(cfg_dir), "--env-config",
                          "scenario_3j4r_moving_scan", "--randomize-moving-scan-scenarios", "--randomize-velocity-jitter", "1.0"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Training finished." in out.stdout
