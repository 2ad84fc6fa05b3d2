"""Moving jammers, radars and target (sim-config ``environment_params.motion``; include/macjd.h, macjd_motion_io), host
side: validation and refusals, the per-step frame tables of ``Scenario.motion_tables``, the reference-generated fixture
tests/golden/env_3j4r_moving.npz replayed through the frame oracle (tests/motion_cases.py), and the C-ABI's declarations
and struct layout."""
import copy
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import yaml

import __graft_entry__ as entry
import motion_cases as cases
from _harness import REPO, OracleEnv

from macjd_amd import _native
from macjd_amd.scenario import (_PE_JAMMER_ROWS, _PE_RADAR_ROWS, Scenario, ScenarioBatch, motion_frame_dict, parse_motion,
                                ring_scenario_dict)

PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")


def _own_rows(sc):
    return np.concatenate([np.asarray(sc.tables[k], dtype=np.float64).reshape(-1)
                           for k in _PE_RADAR_ROWS + _PE_JAMMER_ROWS + ("jr_denom",)])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


# ---- validation and refusals -----------------------------------------------------------------------------------------
def _with_motion(**mo):
    d = ring_scenario_dict(3, 4)
    d["environment_params"]["motion"] = mo
    return d


@pytest.mark.parametrize("mo,msg", [
    ({"step_seconds": 0.5, "speed": 1.0}, r"unknown motion key\(s\) \['speed'\]"),
    ({"target_velocity": [1.0, 0.0]}, r"missing 'step_seconds'"),
    ({"step_seconds": 0.0}, r"step_seconds must be a finite number > 0"),
    ({"step_seconds": -1.0}, r"step_seconds must be a finite number > 0"),
    ({"step_seconds": float("inf")}, r"step_seconds must be a finite number > 0"),
    ({"step_seconds": True}, r"step_seconds must be a finite number > 0"),
    ({"step_seconds": "1"}, r"step_seconds must be a finite number > 0"),
    ({"step_seconds": 0.5, "target_velocity": [1.0]}, r"target_velocity must be a pair"),
    ({"step_seconds": 0.5, "target_velocity": [1.0, float("nan")]}, r"target_velocity must be a pair"),
    ({"step_seconds": 0.5, "target_velocity": [1.0, False]}, r"target_velocity must be a pair"),
    ({"step_seconds": 0.5, "radar_velocity": [[0, 0]] * 3}, r"radar_velocity must be a list of 4 "),
    ({"step_seconds": 0.5, "radar_velocity": [[0, 0]] * 5}, r"radar_velocity must be a list of 4 "),
    ({"step_seconds": 0.5, "jammer_velocity": [[0, 0]] * 4}, r"jammer_velocity must be a list of 3 "),
    ({"step_seconds": 0.5, "jammer_velocity": [[0, 0], [0, 0], [0, float("inf")]]}, r"jammer_velocity\[2\] must be a pair"),
    ({"step_seconds": 0.5, "jammer_velocity": [[0, 0], [0, True], [0, 0]]}, r"jammer_velocity\[1\] must be a pair"),
    ({"step_seconds": 0.5, "radar_velocity": 3.0}, r"radar_velocity must be a list"),
])
def test_bad_motion_blocks_raise(mo, msg):
    with pytest.raises(ValueError, match=msg):
        Scenario.from_dict(_with_motion(**mo))


def test_motion_must_be_a_mapping_and_null_means_static():
    d = ring_scenario_dict(3, 4)
    d["environment_params"]["motion"] = [1, 2]
    with pytest.raises(ValueError, match="motion must be a mapping or null"):
        Scenario.from_dict(d)
    d["environment_params"]["motion"] = None
    sc = Scenario.from_dict(d)
    assert not sc.moving and sc.motion_tables == {}
    assert parse_motion({}) is None


def test_velocities_on_the_entities_are_still_refused():
    """The velocities live under environment_params: a jammer entry with an unknown key fails like the reference's Jammer()."""
    d = ring_scenario_dict(3, 4)
    d["jammers"][0]["velocity"] = [1.0, 0.0]
    with pytest.raises(TypeError, match="unexpected keyword argument 'velocity'"):
        Scenario.from_dict(d)


def test_motion_with_radar_scan_is_refused():
    d = cases.moving_ring_dict(3, 4)
    d["environment_params"]["radar_scan"] = {"step_seconds": 0.25, "sidelobe_db": -30}
    with pytest.raises(ValueError, match="motion together with radar_scan is not supported"):
        Scenario.from_dict(d)


def test_moving_scenarios_are_refused_in_batches_and_under_randomize_scenarios(tmp_path):
    sc, _ = cases.compiled(cases.moving_ring_dict(3, 4))
    with pytest.raises(ValueError, match=r"scenario 1 moves \(environment_params.motion\)"):
        ScenarioBatch([Scenario.from_dict(ring_scenario_dict(3, 4), config=cases.config()), sc])
    with pytest.raises(ValueError, match=r"scenario 0 moves"):
        ScenarioBatch.randomized(cases.moving_ring_dict(3, 4), 2, seed=1)
    # the training driver refuses the flag before it touches a device
    from types import SimpleNamespace
    from macjd_amd.main import build_components
    args = SimpleNamespace(batch_envs=4, randomize_scenarios=True, seed=0)
    with pytest.raises(ValueError, match="--randomize-scenarios is not supported with a moving scenario"):
        build_components(args, os.path.join(PKG, "config", "scenario_3j4r_moving.yaml"))


def test_time_step_helpers_refuse_a_moving_env():
    """The refusal is the first statement of the timing helpers after the scanning one: it needs no device."""
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as B
    env = object.__new__(B)
    env._scan_io, env._motion_io = None, object()
    for call in (lambda: env.time_step_kernel(None, None, 1), lambda: env.time_step_many_kernel(None, None, None, None, None, 1)):
        with pytest.raises(RuntimeError, match="not available with a moving scenario"):
            call()


# ---- frames ----------------------------------------------------------------------------------------------------------
def test_motion_frame_dict_is_the_definition_of_a_frame():
    cfg, _ = cases.fixture()
    mo = cfg["environment_params"]["motion"]
    dt = mo["step_seconds"]
    for k in (0, 1, 20, 57, 100):
        fr = motion_frame_dict(cfg, k)
        assert "motion" not in fr["environment_params"] and "motion" in cfg["environment_params"]   # a copy
        for ents, vel in ((fr["radars"], mo["radar_velocity"]), (fr["jammers"], mo["jammer_velocity"])):
            for i, ent in enumerate(ents):
                p0 = cfg["radars" if ents is fr["radars"] else "jammers"][i]["position"]
                want = [float(p0[a]) + float(k) * (float(vel[i][a]) * dt) for a in range(2)]
                assert ent["position"] == want and all(type(x) is float for x in ent["position"])
        p0 = cfg["protected_target"]["position"]
        assert fr["protected_target"]["position"] == [float(p0[a]) + float(k) * (float(mo["target_velocity"][a]) * dt)
                                                      for a in range(2)]
        rest = lambda d: {key: v for key, v in d.items() if key != "position"}
        assert [rest(r) for r in fr["radars"]] == [rest(r) for r in cfg["radars"]]
    static = ring_scenario_dict(3, 4)
    assert motion_frame_dict(static, 7) == static


@pytest.mark.parametrize("J,R", [(3, 4), (2, 2), (3, 3), (6, 8)])
def test_every_frame_row_is_the_frame_scenarios_own_array(J, R):
    sc, frames = cases.compiled(cases.moving_ring_dict(J, R))
    F = cases.F_SHORT
    mt = sc.motion_tables
    assert sc.moving and sc.episode_limit == F
    assert mt["frames"].shape == (F, 6 * R + 3 * J + J * R) and mt["frames"].dtype == np.float64
    assert mt["flags"].shape == (F, J * R) and mt["flags"].dtype == np.uint8
    assert mt["snr_no"].shape == (F, R) and mt["snr_no"].dtype == np.float64
    assert mt["positions"].shape == (F + 1, 2 * R + 2 * J) and mt["positions"].dtype == np.float32
    assert mt["position_columns"].dtype == np.int32 and mt["position_columns"].tolist() == sc.position_columns
    assert all(a.flags["C_CONTIGUOUS"] for a in mt.values())
    cols = sc.position_columns
    rfd = sc.radar_feature_dim
    assert cols == [r * rfd + rfd - 2 + a for r in range(R) for a in range(2)] + [R * rfd + i for i in range(2 * J)]
    for f in range(F + 1):
        fr = frames[f]
        assert not fr.moving
        np.testing.assert_array_equal(_bits(mt["positions"][f]), _bits(fr.state_vector()[cols]))
        if f < F:
            np.testing.assert_array_equal(_bits(mt["frames"][f]), _bits(_own_rows(fr)))
            np.testing.assert_array_equal(mt["flags"][f], fr.tables["jr_flags"].reshape(-1))
            np.testing.assert_array_equal(_bits(mt["snr_no"][f]), _bits(fr.tables["radar_snr_no"]))
    # frame 0 is what the handle, `tables` and state_vector() carry
    np.testing.assert_array_equal(_bits(mt["frames"][0]), _bits(_own_rows(sc)))
    np.testing.assert_array_equal(mt["flags"][0], sc.tables["jr_flags"].reshape(-1))
    np.testing.assert_array_equal(_bits(mt["positions"][0]), _bits(sc.state_vector()[cols]))
    # the cases the GPU tests rely on: one co-located pair in frame 5 only, a weak denominator in frame 0 only, a moving radar
    den = mt["frames"][:, 6 * R + 3 * J:]
    assert np.argwhere(den < 0).tolist() == [[5, 0]]
    assert np.argwhere(mt["flags"] != 0).tolist() == [[0, 1 * R + 1]]
    assert (mt["positions"][0, :2 * R] != mt["positions"][F, :2 * R]).any()


def test_zero_velocities_make_every_frame_the_static_scenario():
    base = ring_scenario_dict(3, 4)
    static = Scenario.from_dict(base, config=cases.config())
    sc = Scenario.from_dict(cases.zero_velocity(base), config=cases.config())
    mt = sc.motion_tables
    assert sc.moving and sc.motion["radar_velocity"] == [[0.0, 0.0]] * 4 and sc.motion["jammer_velocity"] == [[0.0, 0.0]] * 3
    for f in range(cases.F_SHORT):
        np.testing.assert_array_equal(_bits(mt["frames"][f]), _bits(_own_rows(static)))
        np.testing.assert_array_equal(mt["flags"][f], static.tables["jr_flags"].reshape(-1))
        np.testing.assert_array_equal(_bits(mt["snr_no"][f]), _bits(static.tables["radar_snr_no"]))
    for f in range(cases.F_SHORT + 1):
        np.testing.assert_array_equal(_bits(mt["positions"][f]), _bits(static.state_vector()[sc.position_columns]))
    np.testing.assert_array_equal(_bits(sc.state_vector()), _bits(static.state_vector()))
    for k, v in static.tables.items():
        np.testing.assert_array_equal(_bits(np.asarray(sc.tables[k])), _bits(np.asarray(v)))


def test_without_the_key_nothing_changes():
    sc = Scenario.from_dict(ring_scenario_dict(3, 4))
    assert sc.motion is None and not sc.moving and sc.motion_tables == {}


# ---- the fixture: conditions the reference alone meets ---------------------------------------------------------------
def test_shipped_config_is_the_fixtures_scenario():
    cfg, _ = cases.fixture()
    with open(os.path.join(PKG, "config", "scenario_3j4r_moving.yaml")) as f:
        assert yaml.safe_load(f) == cfg
    sc = Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_moving.yaml"))
    assert sc.moving and (sc.num_jammers, sc.num_radars, sc.episode_limit) == (3, 4, 100)


def test_fixture_scenario_conditions_hold_in_the_references_own_numbers():
    cfg, g = cases.fixture()
    sc, frames = cases.compiled(cfg, None)
    R, J, F = 4, 3, 100
    # pd_no of a radar crosses 0.5 upwards and downwards between frames 10 and 90 — from the reference's recorded
    # no-jamming SNR (info['snr_no_jamming']) through the host's detection_probability, and in the compiled frames
    from macjd_amd.scenario import detection_probability
    snr_no = g["f64_s42_snr_no"]
    assert snr_no.shape == (F, R)
    pd_ref = np.array([[detection_probability(s, sc.pd_consts) for s in row] for row in snr_no])
    above = pd_ref[10:91] > 0.5
    ups = (~above[:-1] & above[1:]).any(axis=0)
    downs = (above[:-1] & ~above[1:]).any(axis=0)
    assert (ups & downs).any()
    np.testing.assert_array_equal(_bits(snr_no), _bits(sc.motion_tables["snr_no"]))   # the reference's SNR, bit for bit
    np.testing.assert_array_equal(_bits(pd_ref), _bits(sc.motion_tables["frames"][:, 3 * R:4 * R]))
    # exactly one (jammer, radar) pair is co-located, in exactly one frame; the weak-denominator bit changes between frames
    den = sc.motion_tables["frames"][:, 6 * R + 3 * J:]
    assert np.argwhere(den < 0).tolist() == [[20, 0 * R + 0]]
    fl = sc.motion_tables["flags"]
    assert fl[0].any() and not fl[1:].any()
    # a radar moves
    pos = sc.motion_tables["positions"]
    assert (pos[0, :2 * R] != pos[F, :2 * R]).any()
    assert "motion" in cfg["environment_params"]   # scenario_json carries the key


# ---- frame oracle against the reference-generated trace --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_fixture_trace_through_the_frame_oracle(mode):
    """One OracleEnv per frame scenario, track / step counter / episode carried across, the logged uniforms: FSM and
    terminated bit-exact, floats at the tolerances of test_env_gpu.py::test_golden_trace_single_env, and the recorded
    observation after step k is the state vector with positions[k + 1]."""
    cfg, g = cases.fixture()
    sc, frames = cases.compiled(cfg, None)
    pre = f"{mode}_s42_"
    T, P, U = g[pre + "T"], g[pre + "P"], np.nan_to_num(g[pre + "u"], nan=2.0)
    n = T.shape[0]
    assert n == sc.episode_limit == 100
    ora = cases.FrameOracle(frames, 1)
    ora.reset()
    out, pd, snr, prj, track, term = [], [], [], [], [], []
    for k in range(n):
        assert ora.frame_of()[0] == k
        Pk = P[k:k + 1].astype(np.float32) if mode == "f32" else P[k:k + 1]
        o = ora.step(T[k:k + 1], Pk, u=U[k:k + 1])
        out.append(o["out64"][0]); pd.append(o["pd64"][0]); snr.append(o["snr64"][0]); prj.append(o["prj64"][0])
        track.append(o["track"][0]); term.append(bool(o["terminated"][0]))
    np.testing.assert_array_equal(np.array(track), g[pre + "track"])
    np.testing.assert_array_equal(np.array(term), g[pre + "terminated"])
    ref = np.stack([g[pre + "reward"], g[pre + "r_d"], g[pre + "r_p"], g[pre + "r_j"]], axis=1)
    np.testing.assert_allclose(np.array(out), ref, rtol=0, atol=1e-5)
    np.testing.assert_allclose(np.array(out), ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.array(pd), g[pre + "pd"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.array(snr), g[pre + "snr_with"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(np.array(prj), g[pre + "prj"], rtol=1e-14, atol=0)
    # the co-located frame: the reference recorded no action of jammer 0 on radar 0 there (prj = -1), and neither did the oracle
    f20 = 20
    if 1 <= T[f20, 0] <= 2:
        assert g[pre + "prj"][f20, 0] == -1.0 and np.array(prj)[f20, 0] == -1.0
    # observations
    cols = sc.position_columns
    base = sc.state_vector()
    want = np.repeat(base[None], n, axis=0)
    want[:, cols] = sc.motion_tables["positions"][1:n + 1]
    np.testing.assert_array_equal(_bits(g[pre + "obs_after"].astype(np.float32)), _bits(want))
    assert g[pre + "obs_after"].dtype == np.float32
    want0 = base.copy()
    want0[cols] = sc.motion_tables["positions"][0]
    np.testing.assert_array_equal(_bits(g[pre + "obs_reset"]), _bits(want0))


# ---- C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_header_binding_and_library_declare_the_entry_points(built):
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int macjd_env_step_moving(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion, "
            "void* hip_stream);") in flat
    assert ("int macjd_env_step_many_moving(const macjd_scenario* s, const macjd_step_io* io, const macjd_motion_io* motion, "
            "int32_t n_steps, int64_t t_stride, void* hip_stream);") in flat
    assert ("int macjd_env_reset_moving(const macjd_scenario* s, int64_t n_envs, const macjd_motion_io* motion, "
            "const uint8_t* mask, void* hip_stream);") in flat
    for sym in ("macjd_env_step_moving", "macjd_env_step_many_moving", "macjd_env_reset_moving"):
        assert sym in _native.EXPORTS and hasattr(built, sym), sym
    assert _native.ABI_VERSION == 12 and "#define MACJD_ABI_VERSION 12" in hdr
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == 12
    assert "macjd_env_motion.hip" in entry.HIP_SOURCES
    assert os.path.exists(os.path.join(PKG, "csrc", "macjd_env_motion.hip"))


def test_motion_io_layout_matches_the_header():
    D = _native.MotionIO
    fields = [n for n, *_ in D._fields_]
    assert fields == ["frames", "frame_flags", "frame_snr_no", "positions", "position_columns", "n_frames", "n_pos", "state",
                      "st_se", "snr_no", "sn_se", "sn_sx"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd.h"\n'
           'int main(){printf("%zu %zu %zu", sizeof(macjd_motion_io), sizeof(macjd_step_io), sizeof(macjd_scan_io));\n'
           + "".join(f'printf(" %zu", offsetof(macjd_motion_io, {f}));\n' for f in fields)
           + 'printf(" %d %d", MACJD_PE_ROWS(4, 3), MACJD_PE_ROWS(8, 6));\n'
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(D)
    assert out[1] == ctypes.sizeof(_native.StepIO) and out[2] == ctypes.sizeof(_native.ScanIO)   # unchanged neighbours
    for name, off in zip(fields, out[3:3 + len(fields)]):
        assert getattr(D, name).offset == off, name
    assert out[3 + len(fields):] == [6 * 4 + 3 * 3 + 12, 6 * 8 + 3 * 6 + 48]
