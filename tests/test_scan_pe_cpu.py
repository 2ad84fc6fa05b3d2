"""Scanning radars on per-env scenario batches (include/macjd.h, macjd_scan_pe_io), host side: the stacked scan tables of
``ScenarioBatch(..., scan=True)``, its refusals, the azimuth jitter of ``randomized_scenario_dict``, the C-ABI's
declarations and struct layout, and the reference model's coverage of every lobe path on the inputs of
tests/test_scan_pe_gpu.py (tests/scan_pe_cases.py)."""
import copy
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import __graft_entry__ as entry
import scan_model
import scan_pe_cases as cases
from _harness import REPO, oracle_lib

from macjd_amd import _native
from macjd_amd.scenario import (PE_SCAN_ROWS, Scenario, ScenarioBatch, pe_scan_rows, randomized_scenario_dict,
                                ring_scenario_dict)


def _own_rows(sc):
    """Scenario ``sc``'s scan arrays in the documented row order, as one float64 vector."""
    st = sc.scan_tables
    rows = [st["half_beam"], st["sweep"], st["sweep_mod"], st["az0"], st["bear_tgt"], st["GaPs_side"],
            sc.tables["radar_snr_no"], st["snr_no_side"], st["pd_no_side"], st["gr_side"], st["bear_jam"]]
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in rows])


# ---- tables ----------------------------------------------------------------------------------------------------------
def test_scan_tables_are_the_scenarios_own_arrays_in_row_order():
    scs, b = cases.batch(3, 4, 5, seed=3)
    R, J = 4, 3
    assert b.scanning and b.scan_tables.dtype == np.float64 and b.scan_tables.flags["C_CONTIGUOUS"]
    assert b.scan_tables.shape == (10 * R + J * R, 5) == (pe_scan_rows(R, J), 5)
    assert PE_SCAN_ROWS == ("half_beam", "sweep", "sweep_mod", "az0", "bear_tgt", "GaPs_side", "snr_no", "snr_no_side",
                            "pd_no_side", "gr_side", "bear_jam")
    for e, sc in enumerate(scs):
        assert b.scan_tables[:, e].tobytes() == _own_rows(sc).tobytes(), e
        # a single-scenario environment compiles the same arrays from the same dict
        again = Scenario.from_dict(cases.scenario_dicts(3, 4, 5, seed=3)[e])
        assert _own_rows(again).tobytes() == b.scan_tables[:, e].tobytes()
        # `full` is not carried: sweep + 2 half_beam >= 360 restates it (2 half_beam is exact)
        full = b.scan_tables[R:2 * R, e] + 2.0 * b.scan_tables[0:R, e] >= 360.0
        assert (full == sc.scan_tables["full"].astype(bool)).all()
    assert len({b.scan_tables[:, e].tobytes() for e in range(5)}) == 5           # five distinct scenarios
    assert scs[cases.FULL_ENV].scan_tables["full"].all() and not scs[0].scan_tables["full"].any()
    assert scs[cases.ON_RADAR_ENV].tables["jr_denom"].reshape(J, R)[0, 0] < 0    # the jammer sits on the radar
    # what the batch carried before is unchanged
    assert b.state_vectors.shape == (5, scs[0].state_dim) and b.snr_no.shape == (5, R)
    assert b.snr_no.tobytes() == np.stack([sc.tables["radar_snr_no"] for sc in scs]).tobytes()
    plain = ScenarioBatch([Scenario.from_dict(ring_scenario_dict(3, 4))] * 2)
    assert plain.scan_tables is None and not plain.scanning


def test_tile_cycles_the_scan_columns():
    _, b = cases.batch(3, 4, 5, seed=3)
    t = b.tile(13)
    assert t.n_envs == 13 and t.scan_tables.shape == (b.scan_tables.shape[0], 13) and t.scan_tables.flags["C_CONTIGUOUS"]
    for e in range(13):
        assert t.scan_tables[:, e].tobytes() == b.scan_tables[:, e % 5].tobytes()
        assert t.tables[:, e].tobytes() == b.tables[:, e % 5].tobytes()
    assert t.scanning


def test_randomized_scanning_batch_is_shard_invariant():
    base = cases.scan_base(3, 4)
    big = ScenarioBatch.randomized(base, 9, seed=4, azimuth_jitter=45.0)
    assert big.scanning and big.base.scanning and big.scan_tables.shape == (pe_scan_rows(4, 3), 9)
    k = 4
    shard = ScenarioBatch.randomized(base, 5, seed=4, env_offset=k, azimuth_jitter=45.0)
    assert shard.scan_tables.tobytes() == np.ascontiguousarray(big.scan_tables[:, k:]).tobytes()
    assert shard.tables.tobytes() == np.ascontiguousarray(big.tables[:, k:]).tobytes()
    assert shard.state_vectors.tobytes() == big.state_vectors[k:].tobytes()
    az0 = big.scan_tables[3 * 4:4 * 4]
    assert np.unique(az0[0]).size == 9                                           # the jitter moved every env's beams
    # a base without radar_scan still gives a plain batch
    assert not ScenarioBatch.randomized(ring_scenario_dict(3, 4), 2, seed=4).scanning


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_scanning_batch_refusals():
    ds = cases.scenario_dicts(3, 4, 3, seed=3)
    scs = [Scenario.from_dict(d) for d in ds]
    with pytest.raises(ValueError, match="scan=True"):
        ScenarioBatch(scs)                                                       # the keyword is needed
    other = copy.deepcopy(ds[1])
    other["environment_params"]["radar_scan"]["sidelobe_db"] = -20.0
    with pytest.raises(ValueError, match=r"scenario 1's radar_scan .* differs"):
        ScenarioBatch([scs[0], Scenario.from_dict(other), scs[2]], scan=True)
    pat = copy.deepcopy(ds[2])
    pat["environment_params"]["radar_scan"]["pattern"] = {"level_width": 1.5, "gain_db": [-3, -12]}
    with pytest.raises(ValueError, match=r"scenario 2 has a radar_scan.pattern"):
        ScenarioBatch([scs[0], scs[1], Scenario.from_dict(pat)], scan=True)
    with pytest.raises(ValueError, match=r"scenario 0 has a radar_scan.pattern"):   # a pattern shared by all of them too
        ScenarioBatch([Scenario.from_dict(pat)] * 2, scan=True)
    static = copy.deepcopy(ds[1])
    del static["environment_params"]["radar_scan"]
    with pytest.raises(ValueError, match=r"scenario 1 has no environment_params.radar_scan"):
        ScenarioBatch([scs[0], Scenario.from_dict(static)], scan=True)


# ---- azimuth jitter --------------------------------------------------------------------------------------------------
def test_azimuth_jitter_default_changes_nothing_and_jitter_moves_only_theta_a():
    base = cases.scan_base(3, 4)
    r0, r1, r2 = (np.random.default_rng([7, 3]) for _ in range(3))
    d0 = randomized_scenario_dict(base, r0)
    d1 = randomized_scenario_dict(base, r1, azimuth_jitter=0.0)
    assert d0 == d1 and r0.bit_generator.state == r1.bit_generator.state
    d2 = randomized_scenario_dict(base, r2, azimuth_jitter=45.0)
    assert r2.bit_generator.state != r0.bit_generator.state                      # the azimuth draws come after the others
    moved = 0
    for a, b in zip(d0["radars"], d2["radars"]):
        moved += a["theta_a"] != b["theta_a"]
        assert {k: v for k, v in a.items() if k != "theta_a"} == {k: v for k, v in b.items() if k != "theta_a"}
    assert moved == 4
    assert {k: v for k, v in d0.items() if k != "radars"} == {k: v for k, v in d2.items() if k != "radars"}
    # N(0, jitter): the first draw after today's ones
    assert d2["radars"][0]["theta_a"] == base["radars"][0]["theta_a"] + float(r0.normal(0.0, 45.0))


# ---- C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_header_binding_and_library_declare_the_entry_points(built):
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int macjd_env_step_scan_pe(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan, "
            "const macjd_scan_pe_io* scan_pe, void* hip_stream);") in flat
    assert ("int macjd_env_reset_scan_pe(const macjd_scenario* s, int64_t n_envs, const macjd_scan_io* scan, "
            "const macjd_scan_pe_io* scan_pe, int32_t pe_tile, const uint8_t* mask, void* hip_stream);") in flat
    assert "#define MACJD_PE_SCAN_ROWS(R, J) (10 * (R) + (J) * (R))" in hdr
    for sym in ("macjd_env_step_scan_pe", "macjd_env_reset_scan_pe"):
        assert sym in _native.EXPORTS and hasattr(built, sym), sym
    assert f"#define MACJD_ABI_VERSION {_native.ABI_VERSION}" in hdr
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == _native.ABI_VERSION


def test_scan_pe_io_layout_and_row_macro_match_the_header():
    D = _native.ScanPeIO
    fields = [n for n, *_ in D._fields_]
    assert fields == ["tables", "stride"]
    sizes = [(2, 2), (3, 4), (5, 7), (12, 16)]   # (R, J)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd.h"\n'
           'int main(){printf("%zu %zu %zu %zu", sizeof(macjd_scan_pe_io), sizeof(macjd_step_io), sizeof(macjd_scan_desc), '
           'sizeof(macjd_scan_io));\n'
           + "".join(f'printf(" %zu", offsetof(macjd_scan_pe_io, {f}));\n' for f in fields)
           + "".join(f'printf(" %d", MACJD_PE_SCAN_ROWS({R}, {J}));\n' for R, J in sizes)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(D)
    assert out[1] == ctypes.sizeof(_native.StepIO) and out[2] == ctypes.sizeof(_native.ScanDesc)   # unchanged neighbours
    assert out[3] == ctypes.sizeof(_native.ScanIO)
    for name, off in zip(fields, out[4:6]):
        assert getattr(D, name).offset == off, name
    for (R, J), rows in zip(sizes, out[6:]):
        assert rows == pe_scan_rows(R, J) == 10 * R + J * R
        assert rows == sum(J * R if k == "bear_jam" else R for k in PE_SCAN_ROWS)


# ---- reference coverage ----------------------------------------------------------------------------------------------
def _counts(models):
    """Lobe counters (target main / side, jammer main / side) summed over the envs, the full-coverage env left out."""
    keep = [m for e, m in enumerate(models) if e != cases.FULL_ENV]
    return sum(m.count_target for m in keep), sum(m.count_jammer for m in keep)


@pytest.mark.parametrize("J,R", [(3, 4), (2, 2)])
def test_reference_model_meets_every_lobe_path_on_the_model_tests_inputs(J, R):
    """The supplied-uniform inputs of the GPU file's test against the model (33 envs x 12 steps)."""
    scs = cases.scenarios(J, R, cases.MODEL["E"], cases.MODEL["seed"])
    models = [scan_model.ScanModel(sc, 1) for sc in scs]
    tracked = 0
    for T, P, u in cases.model_actions(J, R):
        for e, m in enumerate(models):
            tracked += int(m.step(T[e:e + 1], P[e:e + 1], u[e:e + 1])["track"].sum())
    ct, cj = _counts(models)
    assert ct.min() > 0 and cj.min() > 0 and tracked > 0, (ct, cj, tracked)
    assert models[cases.FULL_ENV].count_target[1] == 0                           # that env never sees a side lobe


def test_reference_model_meets_every_lobe_path_on_the_single_env_tests_inputs():
    """The Philox-driven inputs of the GPU file's batch-equals-single-envs test (3j/4r, 40 envs x 30 steps, a masked reset
    at step 17): the model is driven with the generator's own values (the oracle's restatement of it)."""
    c = cases.SINGLES
    J, R, E = c["J"], c["R"], c["E"]
    scs = cases.scenarios(J, R, E, c["seed"], c["env_offset"])
    models = [scan_model.ScanModel(sc, 1) for sc in scs]
    lib = oracle_lib()
    episode = np.zeros(E, dtype=np.int64)
    step = np.zeros(E, dtype=np.int64)
    tracked = 0
    for t, (T, P) in enumerate(cases.singles_actions()):
        if t == c["reset_at"]:
            for e in range(0, E, 3):
                models[e].reset()
                episode[e] += 1
                step[e] = 0
        for e, m in enumerate(models):
            u = np.array([[lib.macjd_oracle_uniform(c["env_seed"], c["env_offset"] + e, int(episode[e]), int(step[e]), k)
                           for k in range(R + J)]])
            tracked += int(m.step(T[e:e + 1], P[e:e + 1], u, arith32=True)["track"].sum())
        step += 1
    ct, cj = _counts(models)
    assert ct.min() > 0 and cj.min() > 0 and tracked > 0, (ct, cj, tracked)
