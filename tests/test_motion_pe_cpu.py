"""Per-env moving scenarios without a GPU: the float64 model of the device frame compiler (tests/motion_pe_model.py) against
the definition of a frame (``Scenario.from_dict(motion_frame_dict(...))``), the layout of ``MovingScenarioBatch`` against
every scenario's own ``motion_tables``, shard invariance, the velocity draws, every refusal (the old ones included), and the
new C-ABI names."""
import contextlib
import copy
import ctypes
import io
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import motion_cases as cases
import motion_pe_model as mpe
import __graft_entry__ as entry
from _harness import REPO

from macjd_amd import _native
from macjd_amd.scenario import (MovingScenarioBatch, Scenario, ScenarioBatch, motion_frame_dict, motion_pe_in_rows,
                                randomized_moving_scenario_dict, randomized_scenario_dict, tile_envs)

PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
SIZES = [(2, 2), (3, 4), (6, 8), (3, 3)]
TOL_SNR = 1e-13   # the project's snr tolerance (tests/test_env_gpu.py: snr_with within 1e-13 relative)
TOL_PD = 1e-12    # the project's pd tolerance


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, r))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
# 1. the model against the definition of a frame
@pytest.mark.parametrize("J,R", SIZES)
def test_model_against_the_definition_of_a_frame(J, R):
    """Every case, no exclusion: positions, flags, -1.0 denominators and the copied rows bit-equal to the host's frames
    (each one a static scenario compiled at the moved positions); GaPs, snr_no and jr_denom within 1e-13 relative, pd_no
    within 1e-12.  (Observed maxima are printed; DESIGN.md 4.10 quotes them.)"""
    dicts, scs = mpe.case(J, R)
    got = mpe.model_tables(scs)
    sl = mpe.row_slices(R, J)
    worst = dict(GaPs=0.0, snr_no=0.0, denom=0.0, pd_no=0.0)
    seen_neg = seen_weak = 0
    for e, (d, sc) in enumerate(zip(dicts, scs)):
        F = sc.episode_limit
        for f in range(F + 1):
            fr = Scenario.from_dict(motion_frame_dict(d, f), config=mpe.config())
            want_pos = fr.state_vector()[sc.position_columns]
            assert got["positions"][e, f].tobytes() == want_pos.tobytes(), (e, f)
            if f == F:
                continue
            col, t = got["frames"][e, f], fr.tables
            for name, key in (("Pn", "radar_Pn"), ("D", "radar_D"), ("rd_pen", "radar_rd_pen"), ("gr", "radar_gr"),
                              ("pmin", "jam_pmin"), ("pmax", "jam_pmax"), ("gj", "jam_gj")):
                assert col[sl[name]].tobytes() == np.asarray(t[key], dtype=np.float64).tobytes(), (e, f, name)
            np.testing.assert_array_equal(got["flags"][e, f], t["jr_flags"], err_msg=f"flags env {e} frame {f}")
            den_g, den_w = col[sl["denom"]], t["jr_denom"]
            np.testing.assert_array_equal(den_g == -1.0, den_w == -1.0)
            assert (den_w[den_w < 0] == -1.0).all()
            seen_neg += int((den_w == -1.0).sum())
            seen_weak += int((t["jr_flags"] & 1).sum())
            worst["denom"] = max(worst["denom"], _rel(den_g, den_w))
            worst["GaPs"] = max(worst["GaPs"], _rel(col[sl["GaPs"]], t["radar_GaPs"]))
            worst["snr_no"] = max(worst["snr_no"], _rel(got["snr_no"][e, f], t["radar_snr_no"]))
            worst["pd_no"] = max(worst["pd_no"], _rel(col[sl["pd_no"]], t["radar_pd_no"]))
    print(f"motion_pe model vs host frames at {J}j/{R}r: max relative difference {worst}")
    assert seen_neg >= 1 and seen_weak >= 1          # the co-located frame and the weak-denominator env are in the table
    assert worst["GaPs"] <= TOL_SNR and worst["snr_no"] <= TOL_SNR and worst["denom"] <= TOL_SNR, worst
    assert worst["pd_no"] <= TOL_PD, worst


def test_the_case_table_holds_the_edge_envs():
    dicts, scs = mpe.case(3, 4)
    F = mpe.F_PE
    sl = mpe.row_slices(4, 3)
    z, t, c, w = (sc.motion_tables for sc in scs[:4])
    assert (z["frames"] == z["frames"][0]).all() and (z["positions"] == z["positions"][0]).all()     # nothing moves
    assert (t["positions"] == t["positions"][0]).all() and not (t["frames"][1] == t["frames"][0]).all()   # only the target
    den = c["frames"][:, sl["denom"]].reshape(F, 3, 4)
    assert den[2, 0, 0] == -1.0 and (den[[0, 1, 3, 4], 0, 0] > 0).all()                               # co-located in frame 2 only
    assert c["positions"][2, 0:2].tobytes() == c["positions"][2, 8:10].tobytes()                      # bit for bit
    assert (w["flags"].reshape(F, 3, 4)[:, 1, 1] == 1).all()                                           # 2e-5 m: weak in every frame
    assert len(dicts) == 19 and len({id(s) for s in scs}) == 19


def test_compile_inputs_need_no_frames():
    """``motion_compile_inputs`` of a moving scenario equals the column formed from the static scenario of frame 0 and the
    parsed motion block: no frame compile is involved."""
    from macjd_amd.scenario import _motion_compile_inputs, parse_motion
    dicts, scs = mpe.case(3, 4)
    for d, sc in zip(dicts[:6], scs[:6]):
        a = sc.motion_compile_inputs()
        sc0 = Scenario.from_dict(motion_frame_dict(d, 0), config=mpe.config())
        assert not sc0.moving and sc0.motion_tables == {}
        b = _motion_compile_inputs(sc0, parse_motion(d["environment_params"], 4, 3))
        assert a["column"].tobytes() == b["column"].tobytes() and a["weak"].tobytes() == b["weak"].tobytes()
        assert a["column"].shape == (motion_pe_in_rows(4, 3),) and a["weak"].shape == (3,)
    with pytest.raises(AttributeError, match="does not move"):
        Scenario.from_dict(motion_frame_dict(dicts[0], 0)).motion_compile_inputs()


# ---------------------------------------------------------------------------------------------------------------
# 2. the batch's layout
def test_batch_layout_equals_every_scenarios_own_motion_tables():
    """Tiles of 8 at E = 19 (last tile padded with zeros): element [tile, f, row, col] is scenario tile * 8 + col's own
    motion_tables[f, row], bit for bit, by the address formula of include/macjd.h."""
    _, scs = mpe.case(3, 4)
    mb = MovingScenarioBatch(scs)
    E, F, R, J, w = 19, mpe.F_PE, 4, 3, 8
    assert mb.n_envs == E and mb.n_frames == F and mb.host_compiled
    tl = mb.tiled(w)
    rows = mpe.pe_rows(R, J)
    assert tl["frames"].shape == (3, F, rows, w) and tl["flags"].shape == (3, F, J * R, w)
    assert tl["snr_no"].shape == (3, F, R, w) and tl["positions"].shape == (3, F + 1, 2 * R + 2 * J, w)
    assert tl["frames"].dtype == np.float64 and tl["flags"].dtype == np.uint8 and tl["positions"].dtype == np.float32
    flat = {k: v.reshape(-1) for k, v in tl.items()}
    for e, sc in enumerate(scs):
        mt = sc.motion_tables
        for key, src, nf in (("frames", "frames", F), ("flags", "flags", F), ("snr_no", "snr_no", F), ("positions", "positions", F + 1)):
            n_rows = mt[src].shape[1]
            for f in range(nf):
                idx = (((e // w) * nf + f) * n_rows + np.arange(n_rows)) * w + e % w
                assert flat[key][idx].tobytes() == np.ascontiguousarray(mt[src][f]).tobytes(), (e, key, f)
    for k, v in tl.items():   # the padding of the last tile
        assert not v[2, ..., 3:].any(), k
    assert mb.state_vectors.shape == (E, scs[0].state_dim)
    for e, sc in enumerate(scs):
        assert mb.state_vectors[e].tobytes() == sc.frame_state_rows()[0].tobytes()
    assert mb.table_bytes(w) == sum(v.nbytes for v in tl.values())
    assert MovingScenarioBatch(scs[:1]).table_bytes(1) == sum(v.nbytes for v in MovingScenarioBatch(scs[:1]).tiled(1).values())
    a = np.arange(19 * 3).reshape(19, 3)
    assert tile_envs(a, 8)[2, 1, 2] == a[18, 1] and tile_envs(a, 8).shape == (3, 3, 8)


def test_table_footprint_at_the_flagship_size():
    """3j/4r, E = 4096, F = 100 at tile 256: 45 float64 rows + 12 flag bytes + 4 float64 snr_no per env-frame (404 B) and
    14 float32 positions per env and frame 0..F — 165.5 MB + 23.2 MB = 188.6 MB."""
    _, scs = mpe.case(3, 4)
    mb = MovingScenarioBatch(scs[:1])
    mb.n_envs, mb.n_frames = 4096, 100
    assert mb.table_bytes(256) == 4096 * (100 * (45 * 8 + 12 + 4 * 8) + 101 * 14 * 4) == 188645376


# ---------------------------------------------------------------------------------------------------------------
# 3. randomised batches
def _moving_base():
    return cases.moving_ring_dict(3, 4)


def test_randomized_is_shard_invariant_and_both_compile_paths_agree_on_the_inputs():
    base = _moving_base()
    kw = dict(seed=7, config=mpe.config(), velocity_jitter=1.5)
    whole = MovingScenarioBatch.randomized(base, 6, compile="host", **kw)
    shard = MovingScenarioBatch.randomized(base, 3, env_offset=3, compile="host", **kw)
    for k in ("frames", "flags", "snr_no", "positions", "state_vectors"):
        assert getattr(whole, k)[3:].tobytes() == getattr(shard, k).tobytes(), k
    assert not (whole.positions[0] == whole.positions[1]).all()
    dev = MovingScenarioBatch.randomized(base, 6, compile="device", **kw)
    dshard = MovingScenarioBatch.randomized(base, 3, env_offset=3, compile="device", **kw)
    assert dev.frames is None and dev.positions is None and not dev.host_compiled and dev.scenarios is None
    assert dev.compile_inputs.shape == (6, motion_pe_in_rows(4, 3)) and dev.compile_weak.shape == (6, 3)
    assert dev.compile_inputs[3:].tobytes() == dshard.compile_inputs.tobytes()
    for e, sc in enumerate(whole.scenarios):   # the device path's column is the host scenario's own
        ins = sc.motion_compile_inputs()
        assert dev.compile_inputs[e].tobytes() == ins["column"].tobytes() and dev.compile_weak[e].tobytes() == ins["weak"].tobytes()
    assert dev.state_vectors.tobytes() == whole.state_vectors.tobytes()
    assert dev.n_frames == whole.n_frames == mpe.F_PE and dev.base.moving
    tl = dev.tiled_compile_inputs(4)
    assert tl["in_tables"].shape == (2, motion_pe_in_rows(4, 3), 4) and tl["in_weak"].shape == (2, 3, 4)
    assert tl["in_tables"][1, :, 1].tobytes() == dev.compile_inputs[5].tobytes() and not tl["in_tables"][1, :, 2:].any()
    with pytest.raises(RuntimeError, match="no host frames exist"):
        dev.tiled(4)
    with pytest.raises(RuntimeError, match="carries no compiler inputs"):
        whole.tiled_compile_inputs(4)
    # and the model on the device path's inputs reproduces the host path within the test-1 tolerances
    sl = mpe.row_slices(4, 3)
    for e in range(6):
        m = mpe.compile_model(dev.compile_inputs[e], dev.compile_weak[e], 4, 3, mpe.F_PE, dev.base.pd_consts)
        assert m["positions"].tobytes() == whole.positions[e].tobytes() and m["flags"].tobytes() == whole.flags[e].tobytes()
        assert _rel(m["frames"][:, sl["GaPs"]], whole.frames[e][:, sl["GaPs"]]) <= TOL_SNR
        assert _rel(m["frames"][:, sl["denom"]], whole.frames[e][:, sl["denom"]]) <= TOL_SNR


def test_velocity_draws_come_last_and_only_with_a_jitter():
    base = _moving_base()
    r0, r1, r2 = (np.random.default_rng([3, 9]) for _ in range(3))
    plain = randomized_scenario_dict(base, r0)
    same = randomized_moving_scenario_dict(base, r1)                       # jitter 0: the very dict, the very stream
    assert same == plain and r1.bit_generator.state == r0.bit_generator.state
    jit = randomized_moving_scenario_dict(base, r2, velocity_jitter=2.0)
    a, b = copy.deepcopy(jit), copy.deepcopy(plain)
    mo_j, mo_p = a["environment_params"].pop("motion"), b["environment_params"].pop("motion")
    assert a == b                                                           # everything drawn earlier is unchanged
    n = 2 * (1 + 4 + 3)
    want = np.random.default_rng([3, 9])
    randomized_scenario_dict(base, want)
    draws = [float(want.normal(0.0, 2.0)) for _ in range(n)]                # target, radars, jammers; x then y
    got = [mo_j["target_velocity"]] + mo_j["radar_velocity"] + mo_j["jammer_velocity"]
    old = [mo_p["target_velocity"]] + mo_p["radar_velocity"] + mo_p["jammer_velocity"]
    flat = lambda vs: [float(x) for v in vs for x in v]
    assert flat(got) == [o + d for o, d in zip(flat(old), draws)]
    assert mo_j["step_seconds"] == mo_p["step_seconds"]
    with pytest.raises(ValueError, match="does not move"):
        randomized_moving_scenario_dict(mpe.motion_frame_dict(base, 0), np.random.default_rng(0), velocity_jitter=1.0)


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals, old and new
def test_refusals():
    base = _moving_base()
    _, scs = mpe.case(3, 4)
    static = Scenario.from_dict(motion_frame_dict(base, 0), config=mpe.config())
    # the old ones still fire
    with pytest.raises(ValueError, match="moving scenarios are not supported in per-env scenario batches"):
        ScenarioBatch([scs[0]])
    with pytest.raises(ValueError, match="moving scenarios are not supported in per-env scenario batches"):
        ScenarioBatch.randomized(base, 2, config=mpe.config())
    # the new class
    with pytest.raises(ValueError, match="at least one scenario"):
        MovingScenarioBatch([])
    with pytest.raises(ValueError, match="scenario 1 does not move"):
        MovingScenarioBatch([scs[0], static])
    scan = copy.deepcopy(base)
    scan["environment_params"]["radar_scan"] = dict(step_seconds=0.5, sidelobe_db=-20.0)
    with pytest.raises(ValueError, match="scanning radars .*not supported on per-env batches"):
        MovingScenarioBatch([Scenario.from_dict(scan, config=mpe.config())])
    with pytest.raises(ValueError, match="scanning radars .*not supported on per-env batches"):
        MovingScenarioBatch.randomized(scan, 2, config=mpe.config())
    with pytest.raises(ValueError, match="does not move"):
        MovingScenarioBatch.randomized(motion_frame_dict(base, 0), 2, config=mpe.config())
    with pytest.raises(ValueError, match="compile must be 'device' or 'host'"):
        MovingScenarioBatch.randomized(base, 2, config=mpe.config(), compile="gpu")
    other = Scenario.from_dict(base, config=mpe.config(mpe.F_PE + 1))
    with pytest.raises(ValueError, match="differs from scenario 0 in shape / episode limit"):
        MovingScenarioBatch([scs[0], other])
    dt = copy.deepcopy(base)
    dt["environment_params"]["motion"]["step_seconds"] = 0.25
    with pytest.raises(ValueError, match="motion.step_seconds .* differs from scenario 0's"):
        MovingScenarioBatch([scs[0], Scenario.from_dict(dt, config=mpe.config())])
    with pytest.raises(ValueError, match="differs from scenario 0 in shape"):
        MovingScenarioBatch([scs[0], mpe.case(3, 3)[1][0]])


def _driver_config(tmp_path, **kw):
    from macjd_amd.main import load_config
    with contextlib.redirect_stdout(io.StringIO()):
        cfg = load_config("default", os.path.join(PKG, "config"))
    cfg.device_request = "cpu"
    cfg.save_model_dir, cfg.results_path = str(tmp_path / "models"), str(tmp_path / "logs")
    cfg.resume = None
    cfg.batch_envs = 4
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_driver_refusals(tmp_path):
    from macjd_amd.main import build_components
    moving = os.path.join(PKG, "config", "scenario_3j4r_moving.yaml")
    static = os.path.join(PKG, "config", "scenario_3j4r.yaml")

    def build(path, **kw):
        with contextlib.redirect_stdout(io.StringIO()):
            build_components(_driver_config(tmp_path, **kw), path)
    with pytest.raises(ValueError, match="--randomize-scenarios is not supported with a moving scenario"):   # the old refusal
        build(moving, randomize_scenarios=True)
    with pytest.raises(ValueError, match="--randomize-moving-scenarios needs a moving scenario"):
        build(static, randomize_moving_scenarios=True)
    with pytest.raises(ValueError, match="are exclusive"):
        build(moving, randomize_moving_scenarios=True, randomize_scenarios=True)
    with pytest.raises(ValueError, match="--randomize-velocity-jitter needs --randomize-moving-scenarios"):
        build(moving, randomize_velocity_jitter=1.0)
    with pytest.raises(ValueError, match="needs a batched run"):
        build(moving, randomize_moving_scenarios=True, batch_envs=1)
    import yaml
    with open(moving) as f:
        d = yaml.safe_load(f)
    d["environment_params"]["radar_scan"] = dict(step_seconds=d["environment_params"]["motion"]["step_seconds"], sidelobe_db=-20.0)
    p = tmp_path / "moving_scan.yaml"
    p.write_text(yaml.safe_dump(d))
    with pytest.raises(ValueError, match="--randomize-moving-scenarios is not supported with scanning radars"):
        build(str(p), randomize_moving_scenarios=True)


def test_driver_flags_parse():
    import argparse
    from macjd_amd import main as drv
    seen = {}
    orig_run, orig_load = drv.run, drv.load_config
    drv.run = lambda cfg: seen.update(vars(cfg)) or {}
    drv.load_config = lambda **kw: SimpleNamespace()
    try:
        drv.main(["--randomize-moving-scenarios", "--randomize-velocity-jitter", "1.25"])
        assert seen["randomize_moving_scenarios"] is True and seen["randomize_velocity_jitter"] == 1.25
        seen.clear()
        drv.main([])
        assert "randomize_moving_scenarios" not in seen and "randomize_velocity_jitter" not in seen
    finally:
        drv.run, drv.load_config = orig_run, orig_load
    del argparse


# ---------------------------------------------------------------------------------------------------------------
# 5. the C-ABI
@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_header_binding_and_library_agree(built):
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    names = ["macjd_env_step_moving_pe", "macjd_env_step_many_moving_pe", "macjd_env_reset_moving_pe", "macjd_motion_pe_compile"]
    lib = built
    assert "macjd_env_motion_pe.hip" in entry.HIP_SOURCES
    for n in names:
        assert re.search(rf"\bint {n}\(", hdr), n
        assert n in _native.EXPORTS
        getattr(lib, n)
    assert "#define MACJD_MOTION_PE_IN_ROWS(R, J) (12 * (R) + 10 * (J) + 4)" in hdr
    assert motion_pe_in_rows(4, 3) == 12 * 4 + 10 * 3 + 4

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            first, *rest = [p.strip() for p in decl.split(",")]
            out.append(re.search(r"(\w+)$", first).group(1))
            out += [re.search(r"(\w+)$", r).group(1) for r in rest]
        return out
    assert fields("macjd_motion_pe_io") == [f[0] for f in _native.MotionPeIO._fields_]
    assert fields("macjd_motion_pe_compile_desc") == [f[0] for f in _native.MotionPeCompileDesc._fields_]
    assert ctypes.sizeof(_native.MotionPeIO) == 5 * 8 + 4 * 4 + 5 * 8
    assert ctypes.sizeof(_native.MotionPeCompileDesc) == 8 + 4 * 4 + 4 * 8 + 6 * 8
