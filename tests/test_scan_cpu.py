"""Scanning radars (environment_params.radar_scan): YAML parsing / validation and the host-derived tables, against the
NumPy restatement's own derivation (tests/scan_model.py).  No GPU needed."""
import copy
import json
import os

import numpy as np
import pytest

import scan_model
from _harness import GOLDEN, REPO

PKG_CONFIG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd", "config")


def _base(name="3j4r"):
    g = np.load(os.path.join(GOLDEN, f"env_{name}.npz"))
    return json.loads(str(g["scenario_json"]))


def _with_scan(d, step_seconds=0.25, sidelobe_db=-30.0):
    d = copy.deepcopy(d)
    d.setdefault("environment_params", {})["radar_scan"] = {"step_seconds": step_seconds, "sidelobe_db": sidelobe_db}
    return d


def _sc(d):
    from macjd_amd.scenario import Scenario
    return Scenario.from_dict(d)


def test_absent_or_null_key_keeps_todays_tables():
    from macjd_amd.scenario import Scenario
    for name in ("2j2r_shipped", "3j4r", "12j16r", "3j3r_edge"):
        d = _base(name)
        s0 = _sc(d)
        d2 = copy.deepcopy(d)
        d2.setdefault("environment_params", {})["radar_scan"] = None
        s1 = _sc(d2)
        assert not s0.scanning and not s1.scanning and s0.scan_tables == {} and s1.scan_tables == {}
        assert set(s0.tables) == set(s1.tables)
        for k in s0.tables:
            assert s0.tables[k].tobytes() == s1.tables[k].tobytes()
    shipped = Scenario.from_yaml(os.path.join(PKG_CONFIG, "scenario_3j4r.yaml"))
    assert not shipped.scanning


@pytest.mark.parametrize("bad", [{"step_seconds": 0.0, "sidelobe_db": -30}, {"step_seconds": -1, "sidelobe_db": -30},
                                 {"step_seconds": 0.25, "sidelobe_db": 1.0}, {"step_seconds": 0.25},
                                 {"sidelobe_db": -30}, {"step_seconds": "x", "sidelobe_db": -30},
                                 {"step_seconds": float("nan"), "sidelobe_db": -30},
                                 {"step_seconds": 0.25, "sidelobe_db": -30, "extra": 1}, [0.25, -30]])
def test_bad_radar_scan_block_raises(bad):
    d = _base()
    d.setdefault("environment_params", {})["radar_scan"] = bad
    with pytest.raises(ValueError):
        _sc(d)


@pytest.mark.parametrize("key,value", [("theta_m", 0.0), ("theta_m", -2.0), ("theta_m", 360.5), ("t_s", 0.0), ("t_s", -4.0)])
def test_bad_radar_beam_parameters_raise_only_when_scanning(key, value):
    d = _base()
    d["radars"][1][key] = value
    _sc(d)   # static beams: the values enter nothing, as today
    with pytest.raises(ValueError):
        _sc(_with_scan(d))


@pytest.mark.parametrize("name", ["2j2r_shipped", "3j4r", "6j8r", "12j16r"])
@pytest.mark.parametrize("sidelobe_db", [-30.0, -13.0])
def test_tables_match_the_restatement(name, sidelobe_db):
    sc = _sc(_with_scan(_base(name), 0.3, sidelobe_db))
    st, d = sc.scan_tables, scan_model.derive(sc)
    R, J = sc.num_radars, sc.num_jammers
    np.testing.assert_array_equal(st["half_beam"], d["half"])
    np.testing.assert_array_equal(st["sweep"], d["sweep"])
    np.testing.assert_array_equal(st["sweep_mod"], d["swm"])
    np.testing.assert_array_equal(st["full"].astype(bool), d["full"])
    np.testing.assert_array_equal(st["az0"], d["az0"])
    np.testing.assert_array_equal(st["bear_tgt"], d["bt"])
    np.testing.assert_array_equal(st["bear_jam"].reshape(J, R), d["bj"])
    for k in ("GaPs_side", "gr_side", "snr_no_side", "pd_no_side"):
        np.testing.assert_array_equal(st[k], d[k])
    assert float(st["rho"]) == d["rho"]
    assert np.all((st["az0"] >= 0) & (st["az0"] <= 360)) and np.all((st["bear_tgt"] >= 0) & (st["bear_tgt"] <= 360))
    # the state vector's theta_a columns
    v = sc.state_vector()
    assert sc.theta_a_columns == [3 + sc.max_radar_types + r * sc.radar_feature_dim for r in range(R)]
    np.testing.assert_array_equal(v[sc.theta_a_columns], np.array([r["theta_a"] for r in sc.radars], dtype=np.float32))


def test_unit_side_lobe_reproduces_the_main_tables_bitwise():
    sc = _sc(_with_scan(_base("3j4r"), 0.25, 0.0))
    st, t = sc.scan_tables, sc.tables
    assert float(st["rho"]) == 1.0
    for side, main in (("GaPs_side", "radar_GaPs"), ("gr_side", "radar_gr"), ("snr_no_side", "radar_snr_no"),
                       ("pd_no_side", "radar_pd_no")):
        assert st[side].tobytes() == t[main].tobytes(), side


def test_full_coverage_flag():
    d = _base("3j4r")
    # sweep + 2 half >= 360: a 360-degree beam, a sweep of a whole turn per step, and the exact boundary
    d["radars"][0]["theta_m"] = 360.0
    d["radars"][1]["t_s"] = 0.25                   # sweep 360 per 0.25 s step
    d["radars"][2].update(theta_m=60.0, t_s=0.3)   # sweep 300 + 60 = 360 exactly
    d["radars"][3].update(theta_m=59.0, t_s=0.3)   # 359: not full
    sc = _sc(_with_scan(d, 0.25))
    assert sc.scan_tables["full"].tolist() == [1, 1, 1, 0]
    np.testing.assert_array_equal(sc.scan_tables["full"].astype(bool), scan_model.derive(sc)["full"])
    assert sc.scan_tables["sweep_mod"][1] == 0.0


def test_wrap_and_bearings():
    from macjd_amd.scenario import bearing_degrees, wrap_degrees
    for x in (-725.0, -360.0, -0.5, 0.0, 359.75, 360.0, 721.0):
        assert wrap_degrees(x) == scan_model.wrap(x)
        assert 0.0 <= wrap_degrees(x) < 360.0
    assert bearing_degrees([0, 0], [0, 1]) == 90.0
    assert bearing_degrees([0, 0], [-1, 0]) == 180.0
    assert bearing_degrees([0, 0], [0, -1]) == 270.0


def test_shipped_scan_scenario():
    from macjd_amd.scenario import Scenario, ScenarioBatch
    sc = Scenario.from_yaml(os.path.join(PKG_CONFIG, "scenario_3j4r_scan.yaml"))
    base = Scenario.from_yaml(os.path.join(PKG_CONFIG, "scenario_3j4r.yaml"))
    assert sc.scanning and sc.radar_scan == {"step_seconds": 0.25, "sidelobe_db": -30.0}
    for k in base.tables:
        assert sc.tables[k].tobytes() == base.tables[k].tobytes()
    assert not sc.scan_tables["full"].any()
    with pytest.raises(ValueError):
        ScenarioBatch([sc, sc])


def test_restatement_takes_both_lobe_branches_on_the_shipped_scan_scenario():
    from macjd_amd.scenario import Scenario
    sc = Scenario.from_yaml(os.path.join(PKG_CONFIG, "scenario_3j4r_scan.yaml"))
    m = scan_model.ScanModel(sc, 64)
    rng = np.random.default_rng(0)
    for t in range(60):
        T = rng.integers(0, 2 * sc.num_radars + 1, size=(64, sc.num_jammers))
        m.step(T, rng.random((64, sc.num_jammers)), rng.random((64, sc.num_radars + sc.num_jammers)))
    assert m.count_target.min() > 0 and m.count_jammer.min() > 0, (m.count_target, m.count_jammer)


def test_abi_declares_the_scan_entry_points():
    from macjd_amd import _native
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    for sym in ("macjd_scenario_set_scan", "macjd_env_step_scan", "macjd_env_reset_scan"):
        assert sym in _native.EXPORTS and f"{sym}(" in hdr
    assert f"#define MACJD_ABI_VERSION {_native.ABI_VERSION}" in hdr
