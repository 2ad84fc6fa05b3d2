"""Per-env moving scenarios under scanning radars without a GPU: the float64 model of the device compiler of the beam frames
(tests/moving_scan_pe_model.py) against the definition of a frame (``Scenario.motion_tables`` of host-compiled moving scanning
scenarios), what the shared case table reaches, the fairness of the step cases, the layout of ``MovingScanScenarioBatch``,
shard invariance, every refusal (the old ones included) and the new C-ABI names."""
import contextlib
import copy
import ctypes
import io
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import motion_cases
import moving_scan_pe_model as spm
import __graft_entry__ as entry
from _harness import REPO

from macjd_amd import _native
from macjd_amd.scenario import (MovingScanScenarioBatch, MovingScenarioBatch, Scenario, motion_frame_dict,
                                motion_scan_pe_in_rows, pe_scan_pattern_rows, pe_scan_rows, tile_envs)

PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
TOL_PD = 1e-12    # the project's pd tolerance
F = spm.F_PE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rel(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return float(np.nanmax(np.where(a == b, 0.0, r)))


def _host(scs, key):
    return np.stack([sc.motion_tables[key] for sc in scs])


# ---------------------------------------------------------------------------------------------------------------
# 1. the model against the definition of a frame
@pytest.mark.parametrize("J,R,L", spm.CASES)
def test_model_against_the_definition_of_a_frame(J, R, L):
    """The beam compiler's model on each scenario's host-compiled frames: every row of scan_frames / pattern_frames bit for
    bit — a * (180.0 / np.pi) against np.degrees included — except the pd_no rows (within 1e-12 relative)."""
    _, scs = spm.case(J, R, L)
    got = spm.model_tables(scs, first="host")
    ss, ps = spm.scan_slices(R, J), spm.pattern_slices(R, L)
    want = _host(scs, "scan_frames")
    assert want.shape == (spm.E0, F, pe_scan_rows(R, J)) and got["scan_frames"].shape == want.shape
    a, b = got["scan_frames"].copy(), want.copy()
    assert _rel(a[..., ss["pd_no_side"]], b[..., ss["pd_no_side"]]) <= TOL_PD
    a[..., ss["pd_no_side"]] = b[..., ss["pd_no_side"]] = 0.0
    bad = np.argwhere(_bits(a) != _bits(b))
    assert bad.size == 0, (bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
    if L:
        want = _host(scs, "pattern_frames")
        assert want.shape == (spm.E0, F, pe_scan_pattern_rows(R, L))
        a, b = got["pattern_frames"].copy(), want.copy()
        assert _rel(a[..., ps["pd_no_lvl"]], b[..., ps["pd_no_lvl"]]) <= TOL_PD
        a[..., ps["pd_no_lvl"]] = b[..., ps["pd_no_lvl"]] = 0.0
        bad = np.argwhere(_bits(a) != _bits(b))
        assert bad.size == 0, (bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
    else:
        assert "pattern_frames" not in got and "pattern_frames" not in scs[0].motion_tables


def test_the_case_table_reaches_what_it_must():
    assert {(J, R) for J, R, _ in spm.CASES} == {(2, 2), (3, 4), (6, 8), (3, 3)}
    assert {L for _, _, L in spm.CASES} == {0, 1, 4, 6}
    quadrants, near_seam, on_radar = set(), False, False
    jam_level_change = tgt_lobe_change = weak = False
    for J, R, L in spm.CASES:
        dicts, scs = spm.case(J, R, L)
        rs = [d["environment_params"]["radar_scan"] for d in dicts]
        assert len({r["sidelobe_db"] for r in rs}) == len(rs)                     # sidelobe_db differs between the envs
        if L:
            assert len({tuple(r["pattern"]["gain_db"]) for r in rs}) == len(rs)   # ... and so does every gain_db
        sf = _host(scs, "scan_frames")
        ss = spm.scan_slices(R, J)
        bears = np.concatenate([sf[..., ss["bear_tgt"]].ravel(), sf[..., ss["bear_jam"]].ravel()])
        assert ((bears >= 0.0) & (bears <= 360.0)).all()
        quadrants |= set(np.floor(bears[bears < 360.0] / 90.0).astype(int).tolist())
        near_seam |= bool(((bears > 360.0 - 1e-6) & (bears < 360.0)).any())
        on_radar |= bool((_host(scs, "frames")[..., 6 * R + 3 * J:] == -1.0).any())   # atan2(0, 0)
        weak |= bool(_host(scs, "flags").any())
        for e, sc in enumerate(scs):
            pf = sc.motion_tables["pattern_frames"] if L else None
            lt, lj = spm.search_levels(sc.motion_tables["scan_frames"], pf, R, J, L)
            tgt_lobe_change |= bool(((lt[1:] == 0) != (lt[:-1] == 0)).any())
            if L:
                jam_level_change |= bool((lj[1:] != lj[:-1]).any())
    assert quadrants == {0, 1, 2, 3} and near_seam and on_radar and weak
    assert jam_level_change and tgt_lobe_change


@pytest.mark.parametrize("J,R,L", spm.STEP_MODEL_CASES)
def test_step_cases_are_fair(J, R, L):
    """No consumed uniform of the step-vs-model run lies within the pd tolerance of its detection probability: a device pd
    within 1e-12 of the model's decides every draw as the model does."""
    steps, models = spm.step_model_run(J, R, L)
    assert len(steps) == F + 2 and len(models) == spm.STEP_MODEL["E"]
    assert min(m.min_margin for m in models) > 1e-6 > TOL_PD
    assert all(int(m.step_count[0]) == F + 2 for m in models)            # past the F - 1 clamp
    tracks = np.stack([s[3]["track"] for s in steps])
    assert tracks.any() and not tracks.all()


# ---------------------------------------------------------------------------------------------------------------
# 2. the batch
def test_batch_stacks_every_scenarios_own_tables_and_tiles_them():
    J, R, L = 3, 4, 4
    _, scs = spm.case(J, R, L)
    mb = MovingScanScenarioBatch(scs)
    E = len(scs)
    assert mb.host_compiled and mb.scan_pattern_levels == L and mb.n_frames == F
    for key, arr in (("frames", mb.frames), ("flags", mb.flags), ("snr_no", mb.snr_no), ("positions", mb.positions),
                     ("scan_frames", mb.scan_frames), ("pattern_frames", mb.pattern_frames)):
        for e, sc in enumerate(scs):
            assert arr[e].tobytes() == np.ascontiguousarray(sc.motion_tables[key]).tobytes(), (key, e)
    tile = 8
    tl = mb.tiled(tile)
    n_tiles = (E + tile - 1) // tile
    assert tl["scan_frames"].shape == (n_tiles, F, pe_scan_rows(R, J), tile)
    assert tl["pattern_frames"].shape == (n_tiles, F, pe_scan_pattern_rows(R, L), tile)
    for e, f, t in ((0, 0, 0), (9, 3, 17), (18, 4, pe_scan_rows(R, J) - 1)):   # row t of frame f of env e, by the header's formula
        flat = tl["scan_frames"].reshape(-1)
        assert flat[(((e // tile) * F + f) * pe_scan_rows(R, J) + t) * tile + e % tile] == mb.scan_frames[e, f, t]
        flat = tl["pattern_frames"].reshape(-1)
        assert flat[(((e // tile) * F + f) * pe_scan_pattern_rows(R, L) + t) * tile + e % tile] == mb.pattern_frames[e, f, t]
    assert not tl["scan_frames"][-1, ..., E - (n_tiles - 1) * tile:].any()       # the last tile's padding
    assert mb.table_bytes(tile) == sum(a.nbytes for a in tl.values())
    with pytest.raises(RuntimeError, match="carries no compiler inputs"):
        mb.tiled_compile_inputs(tile)
    # pattern-free batch: no pattern frames
    mb0 = MovingScanScenarioBatch(spm.case(J, R, 0)[1])
    assert mb0.pattern_frames is None and "pattern_frames" not in mb0.tiled(tile) and mb0.scan_pattern_levels == 0
    assert mb0.table_bytes(tile) == sum(a.nbytes for a in mb0.tiled(tile).values())


def test_table_bytes_orientation():
    """3j/4r with L = 4 at E = 4096, F = 100: the frame tables (~188.6 MB) + the scan frames (~170 MB) + the pattern frames
    (~328 MB)."""
    sc = Scenario.from_dict(spm.case(3, 4, 4)[0][4], config=spm.config(100))
    mb = object.__new__(MovingScanScenarioBatch)
    mb._init_common(sc, 4096, np.zeros((4096, sc.state_dim), dtype=np.float32))
    base = MovingScenarioBatch.table_bytes(mb, 256)
    assert round(base / 1e6, 1) == 188.6
    assert mb.table_bytes(256) - base == 4096 * 100 * (52 + 100) * 8
    assert round(4096 * 100 * 52 * 8 / 1e6) == 170 and round(4096 * 100 * 100 * 8 / 1e6) == 328


def _base(L=4):
    return spm._scanning(motion_cases.moving_ring_dict(3, 4), L)


def test_randomized_is_shard_invariant_and_carries_both_compilers_inputs():
    base = _base()
    kw = dict(seed=7, config=spm.config(), velocity_jitter=1.5, azimuth_jitter=25.0)
    whole = MovingScanScenarioBatch.randomized(base, 7, compile="host", env_offset=10, **kw)
    shard = MovingScanScenarioBatch.randomized(base, 4, compile="host", env_offset=13, **kw)
    for k in ("frames", "flags", "snr_no", "positions", "scan_frames", "pattern_frames", "state_vectors"):
        assert getattr(whole, k)[3:].tobytes() == getattr(shard, k).tobytes(), k
    az0 = whole.scan_frames[:, 0, 3 * 4:4 * 4]
    assert len({a.tobytes() for a in az0}) == 7                                 # the azimuth jitter reached every env
    dev = MovingScanScenarioBatch.randomized(base, 7, compile="device", env_offset=10, **kw)
    dshard = MovingScanScenarioBatch.randomized(base, 4, compile="device", env_offset=13, **kw)
    assert not dev.host_compiled and dev.scenarios is None and dev.scan_frames is None and dev.pattern_frames is None
    assert dev.scan_compile_inputs.shape == (7, motion_scan_pe_in_rows(4, 4)) and dev.scan_compile_inputs.dtype == np.float64
    for k in ("compile_inputs", "compile_weak", "scan_compile_inputs", "state_vectors"):
        assert getattr(dev, k)[3:].tobytes() == getattr(dshard, k).tobytes(), k
    assert dev.state_vectors.tobytes() == whole.state_vectors.tobytes()
    for e, sc in enumerate(whole.scenarios):
        # the input column is the frame-0 scanning scenario's own values
        st = Scenario.from_dict(motion_frame_dict(_dict_of(base, 7, 10 + e, kw), 0), config=spm.config()).scan_tables
        want = np.concatenate([st["half_beam"], st["sweep"], st["sweep_mod"], st["az0"], [st["rho"]], st["pat_inv_width"],
                               st["pat_rho"]])
        assert dev.scan_compile_inputs[e].tobytes() == want.tobytes(), e
        assert dev.compile_inputs[e].tobytes() == sc.motion_compile_inputs()["column"].tobytes(), e
    tl = dev.tiled_compile_inputs(4)
    assert tl["scan_in"].shape == (2, motion_scan_pe_in_rows(4, 4), 4)
    assert tl["scan_in"][1, :, 1].tobytes() == dev.scan_compile_inputs[5].tobytes() and not tl["scan_in"][1, :, 3:].any()
    assert tl["scan_in"].tobytes() == tile_envs(dev.scan_compile_inputs, 4).tobytes()
    with pytest.raises(RuntimeError, match="no host frames exist"):
        dev.tiled(4)
    assert dev.table_bytes(4) == whole.table_bytes(4)
    # the two compilers' models on the device batch's inputs give the host batch's tables (pd rows within 1e-12)
    m = spm.model_tables(whole.scenarios, first="host")
    assert m["scan_frames"][..., :5 * 4].tobytes() == whole.scan_frames[..., :5 * 4].tobytes()


def _dict_of(base, seed, index, kw):
    from macjd_amd.scenario import randomized_moving_scenario_dict
    rng = np.random.default_rng([int(kw["seed"]), int(index)])
    del seed
    return randomized_moving_scenario_dict(base, rng, velocity_jitter=kw["velocity_jitter"], azimuth_jitter=kw["azimuth_jitter"])


# ---------------------------------------------------------------------------------------------------------------
# 3. refusals, old and new
def test_batch_refusals():
    base = _base()
    _, scs = spm.case(3, 4, 4)
    cfg = spm.config()
    with pytest.raises(ValueError, match="at least one scenario"):
        MovingScanScenarioBatch([])
    plain_moving = Scenario.from_dict(motion_cases.moving_ring_dict(3, 4), config=cfg)
    with pytest.raises(ValueError, match="scenario 1 has no scanning radars"):
        MovingScanScenarioBatch([scs[0], plain_moving])
    static_scan = Scenario.from_dict(motion_frame_dict(base, 0), config=cfg)
    with pytest.raises(ValueError, match="scenario 1 does not move"):
        MovingScanScenarioBatch([scs[0], static_scan])
    with pytest.raises(ValueError, match="differs from scenario 0 in shape / episode limit"):
        MovingScanScenarioBatch([scs[0], Scenario.from_dict(base, config=spm.config(F + 1))])
    with pytest.raises(ValueError, match="differs from scenario 0 in shape"):
        MovingScanScenarioBatch([scs[0], spm.case(3, 3, 4)[1][0]])
    with pytest.raises(ValueError, match="another number of levels"):
        MovingScanScenarioBatch([scs[0], spm.case(3, 4, 6)[1][0]])
    with pytest.raises(ValueError, match="another number of levels"):
        MovingScanScenarioBatch([scs[0], spm.case(3, 4, 0)[1][0]])
    lw = copy.deepcopy(base)
    lw["environment_params"]["radar_scan"]["pattern"]["level_width"] = 2.0
    with pytest.raises(ValueError, match="level_width .* differs from scenario 0's"):
        MovingScanScenarioBatch([scs[0], Scenario.from_dict(lw, config=cfg)])
    dt = copy.deepcopy(base)
    dt["environment_params"]["motion"]["step_seconds"] = dt["environment_params"]["radar_scan"]["step_seconds"] = 0.25
    with pytest.raises(ValueError, match="motion.step_seconds .* differs from scenario 0's"):
        MovingScanScenarioBatch([scs[0], Scenario.from_dict(dt, config=cfg)])
    # one clock: any other pair is refused with the scenario compiler's own wording, on both compile paths
    two = copy.deepcopy(base)
    two["environment_params"]["radar_scan"]["step_seconds"] = 0.25
    for how in ("host", "device"):
        with pytest.raises(ValueError, match="on one clock: motion.step_seconds"):
            MovingScanScenarioBatch.randomized(two, 2, config=cfg, compile=how)
    with pytest.raises(ValueError, match="does not move"):
        MovingScanScenarioBatch.randomized(motion_frame_dict(base, 0), 2, config=cfg)
    with pytest.raises(ValueError, match="has no scanning radars"):
        MovingScanScenarioBatch.randomized(motion_cases.moving_ring_dict(3, 4), 2, config=cfg)
    with pytest.raises(ValueError, match="compile must be 'device' or 'host'"):
        MovingScanScenarioBatch.randomized(base, 2, config=cfg, compile="gpu")
    # gain_db and sidelobe_db may differ per env (spm.case makes them differ); the old class keeps refusing radar_scan
    assert MovingScanScenarioBatch(scs).n_envs == len(scs)
    with pytest.raises(ValueError, match="scanning radars .*not supported on per-env batches"):
        MovingScenarioBatch([scs[0]])
    with pytest.raises(ValueError, match="scanning radars .*not supported on per-env batches"):
        MovingScenarioBatch.randomized(base, 2, config=cfg)


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


def test_driver_refusals_and_flags(tmp_path):
    from macjd_amd import main as drv
    both = os.path.join(PKG, "config", "scenario_3j4r_moving_scan.yaml")
    moving = os.path.join(PKG, "config", "scenario_3j4r_moving.yaml")
    static = os.path.join(PKG, "config", "scenario_3j4r.yaml")

    def build(path, **kw):
        with contextlib.redirect_stdout(io.StringIO()):
            drv.build_components(_driver_config(tmp_path, **kw), path)
    for path in (moving, static):
        with pytest.raises(ValueError, match="--randomize-moving-scan-scenarios needs a scenario that both moves and scans"):
            build(path, randomize_moving_scan_scenarios=True)
    with pytest.raises(ValueError, match="are exclusive"):
        build(both, randomize_moving_scan_scenarios=True, randomize_scenarios=True)
    with pytest.raises(ValueError, match="are exclusive"):
        build(both, randomize_moving_scan_scenarios=True, randomize_moving_scenarios=True)
    with pytest.raises(ValueError, match="needs a batched run"):
        build(both, randomize_moving_scan_scenarios=True, batch_envs=1)
    with pytest.raises(ValueError, match="needs a batched run"):
        build(both, randomize_moving_scan_scenarios=True, randomize_velocity_jitter=1.0, batch_envs=1)
    import yaml
    with open(both) as f:
        d = yaml.safe_load(f)
    d["environment_params"]["radar_scan"]["step_seconds"] = 2 * float(d["environment_params"]["motion"]["step_seconds"])
    p = tmp_path / "two_clocks.yaml"
    p.write_text(yaml.safe_dump(d))
    with pytest.raises(ValueError, match="on one clock"):
        build(str(p), randomize_moving_scan_scenarios=True)
    # the old flag still refuses radar_scan; the velocity jitter still needs one of the two flags
    with pytest.raises(ValueError, match="--randomize-moving-scenarios is not supported with scanning radars"):
        build(both, randomize_moving_scenarios=True)
    with pytest.raises(ValueError, match="--randomize-velocity-jitter needs --randomize-moving-scenarios"):
        build(both, randomize_velocity_jitter=1.0)
    # with the flag on a valid config the build gets as far as the device (none here: the product has no CPU path)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            build(both, randomize_moving_scan_scenarios=True, randomize_velocity_jitter=1.0)
    seen = {}
    orig_run, orig_load = drv.run, drv.load_config
    drv.run = lambda cfg: seen.update(vars(cfg)) or {}
    from types import SimpleNamespace
    drv.load_config = lambda **kw: SimpleNamespace()
    try:
        drv.main(["--randomize-moving-scan-scenarios", "--randomize-velocity-jitter", "1.0"])
        assert seen["randomize_moving_scan_scenarios"] is True and seen["randomize_velocity_jitter"] == 1.0
        assert "randomize_moving_scenarios" not in seen
        seen.clear()
        drv.main([])
        assert "randomize_moving_scan_scenarios" not in seen
    finally:
        drv.run, drv.load_config = orig_run, orig_load


# ---------------------------------------------------------------------------------------------------------------
# 4. the C-ABI
NEW_EXPORTS = ("macjd_env_step_moving_scan_pe", "macjd_env_reset_moving_scan_pe", "macjd_motion_scan_pe_compile")


def test_new_exports_struct_sizes_and_abi_version():
    entry.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in NEW_EXPORTS:
        assert sym in _native.EXPORTS and hasattr(lib, sym) and re.search(r"\b%s\s*\(" % sym, code), sym
    assert re.search(r"#define\s+MACJD_ABI_VERSION\s+12\b", hdr) and _native.ABI_VERSION == 12
    lib.macjd_abi_version.restype = ctypes.c_int
    assert lib.macjd_abi_version() == 12
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd.h"\n'
           'int main(){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(macjd_motion_scan_pe_io), '
           'sizeof(macjd_motion_scan_pe_compile_desc), offsetof(macjd_motion_scan_pe_compile_desc, deg_per_rad), '
           'offsetof(macjd_motion_scan_pe_compile_desc, pattern_frames), offsetof(macjd_motion_scan_pe_io, n_levels), '
           'MACJD_MOTION_SCAN_PE_IN_ROWS(4, 0), MACJD_MOTION_SCAN_PE_IN_ROWS(4, 6));return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_native.MotionScanPeIO)
    assert out[1] == ctypes.sizeof(_native.MotionScanPeCompileDesc)
    assert out[2] == _native.MotionScanPeCompileDesc.deg_per_rad.offset
    assert out[3] == _native.MotionScanPeCompileDesc.pattern_frames.offset
    assert out[4] == _native.MotionScanPeIO.n_levels.offset
    assert out[5] == motion_scan_pe_in_rows(4, 0) == 17 and out[6] == motion_scan_pe_in_rows(4, 6) == 27
    from macjd_amd.scenario import DEG_PER_RAD
    assert DEG_PER_RAD == 180.0 / np.pi and np.degrees(np.float64(1.0)) == np.float64(1.0) * DEG_PER_RAD
