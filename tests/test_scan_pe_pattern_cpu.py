"""Stepped antenna pattern on per-env scanning scenario batches (include/macjd.h, macjd_scan_pe_pattern_io), host side: the
stacked level tables of ``ScenarioBatch(..., scan=True, pattern=True)``, its refusals, the C-ABI's declarations and struct
layout, and the reference model's coverage of every level, both FSM states and a deception draw on the inputs of
tests/test_scan_pe_pattern_gpu.py (tests/scan_pe_pattern_cases.py)."""
import copy
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import __graft_entry__ as entry
import scan_pattern_model as spm
import scan_pe_pattern_cases as cases
from _harness import REPO, oracle_lib

from macjd_amd import _native
from macjd_amd import scenario as scenario_mod
from macjd_amd.scenario import PE_SCAN_ROWS, Scenario, ScenarioBatch, pe_scan_rows


def _own_rows(sc):
    """Scenario ``sc``'s level arrays in the documented row order, as one float64 vector."""
    t, st = sc.tables, sc.scan_tables
    rows = [st["pat_inv_width"],
            t["radar_GaPs"], st["pat_GaPs"], st["GaPs_side"],
            t["radar_snr_no"], st["pat_snr_no"], st["snr_no_side"],
            t["radar_pd_no"], st["pat_pd_no"], st["pd_no_side"],
            t["radar_gr"], st["pat_gr"], st["gr_side"]]
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in rows])


# ---- tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 4, 6])
def test_pattern_tables_are_the_scenarios_own_arrays_in_row_order(L):
    J, R, E = 3, 4, 5
    scs, b = cases.batch(J, R, E, seed=3, L=L)
    assert scenario_mod.PE_SCAN_PATTERN_ROWS == ("inv_width", "GaPs_lvl", "snr_no_lvl", "pd_no_lvl", "gr_lvl")
    rows = scenario_mod.pe_scan_pattern_rows(R, L)
    assert rows == R + 4 * (L + 2) * R
    pt = b.pattern_tables
    assert pt.dtype == np.float64 and pt.flags["C_CONTIGUOUS"] and pt.shape == (rows, E)
    assert b.scan_pattern_levels == L and b.scanning
    lv = (L + 2) * R
    for e, sc in enumerate(scs):
        assert pt[:, e].tobytes() == _own_rows(sc).tobytes(), e
        again = Scenario.from_dict(cases.scenario_dicts(J, R, E, seed=3, L=L)[e])   # what a single-scenario env compiles
        assert _own_rows(again).tobytes() == pt[:, e].tobytes()
        # level 0 = the env's main-lobe rows of `tables` (GaPs, pd_no, gr) and of `scan_tables` (snr_no) ...
        for k, pe_row in ((0, 0), (2, 3), (3, 5)):
            assert pt[R + k * lv:R + k * lv + R, e].tobytes() == b.tables[pe_row * R:(pe_row + 1) * R, e].tobytes(), (k, e)
        srow = {name: i for i, name in enumerate(PE_SCAN_ROWS)}
        sl = lambda name: b.scan_tables[srow[name] * R:(srow[name] + 1) * R, e]
        assert pt[R + lv:R + lv + R, e].tobytes() == sl("snr_no").tobytes() == b.snr_no[e].tobytes()
        # ... level L + 1 = its side-lobe rows of `scan_tables`
        for k, name in enumerate(("GaPs_side", "snr_no_side", "pd_no_side", "gr_side")):
            assert pt[R + k * lv + (L + 1) * R:R + (k + 1) * lv, e].tobytes() == sl(name).tobytes(), (name, e)
        # levels 1..L = the scenario's pat_* arrays, level-major; they agree with the independent restatement
        d = spm.derive(sc)
        assert pt[:R, e].tobytes() == d["inv_width"].tobytes()
        for k, mine in enumerate(("GaPs", "snr_no", "pd_no", "gr")):
            assert pt[R + k * lv:R + (k + 1) * lv, e].tobytes() == np.ascontiguousarray(d[mine]).tobytes(), (mine, e)
    assert len({pt[:, e].tobytes() for e in range(E)}) == E                       # five distinct scenarios
    assert np.unique(pt[:R, 0]).size == R                                        # inv_width differs per radar
    assert b.scan_tables.shape == (pe_scan_rows(R, J), E)                        # what the batch carried before is there


def test_batches_without_the_keyword_are_unchanged():
    import scan_pe_cases as plain
    _, b = plain.batch(3, 4, 3, seed=3)
    assert b.pattern_tables is None and b.scan_pattern_levels == 0 and b.scanning
    static = ScenarioBatch([Scenario.from_dict(plain.ring_scenario_dict(3, 4))] * 2)
    assert static.pattern_tables is None and static.scan_pattern_levels == 0
    assert static.tile(5).pattern_tables is None and b.tile(5).pattern_tables is None


def test_tile_cycles_the_pattern_columns():
    _, b = cases.batch(3, 4, 5, seed=3)
    t = b.tile(13)
    assert t.n_envs == 13 and t.pattern_tables.shape == (b.pattern_tables.shape[0], 13) and t.pattern_tables.flags["C_CONTIGUOUS"]
    for e in range(13):
        assert t.pattern_tables[:, e].tobytes() == b.pattern_tables[:, e % 5].tobytes()
        assert t.scan_tables[:, e].tobytes() == b.scan_tables[:, e % 5].tobytes()
    assert t.scan_pattern_levels == 4 and t.scanning


def test_randomized_pattern_batch_is_shard_invariant():
    base = cases.pattern_base(3, 4)
    big = ScenarioBatch.randomized(base, 9, seed=4, azimuth_jitter=45.0)
    assert big.scanning and big.scan_pattern_levels == 4
    assert big.pattern_tables.shape == (scenario_mod.pe_scan_pattern_rows(4, 4), 9)
    k = 4
    shard = ScenarioBatch.randomized(base, 5, seed=4, env_offset=k, azimuth_jitter=45.0)
    assert shard.pattern_tables.tobytes() == np.ascontiguousarray(big.pattern_tables[:, k:]).tobytes()
    assert shard.scan_tables.tobytes() == np.ascontiguousarray(big.scan_tables[:, k:]).tobytes()
    assert shard.tables.tobytes() == np.ascontiguousarray(big.tables[:, k:]).tobytes()
    assert np.unique(big.pattern_tables[4 + 2 * 4]).size == 9                     # level 2 GaPs of radar 0: jittered per env
    # bases without a pattern keep giving pattern-free batches
    assert ScenarioBatch.randomized(cases.pattern_base(3, 4, pattern=False), 2, seed=4).pattern_tables is None
    # the shipped pattern scenario goes through
    import yaml
    with open(os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd", "config",
                           "scenario_3j4r_scan_pattern.yaml")) as f:
        shipped = ScenarioBatch.randomized(yaml.safe_load(f), 3, seed=1)
    assert shipped.scan_pattern_levels == 4 and shipped.pattern_tables.shape[1] == 3


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_pattern_batch_refusals():
    ds = cases.scenario_dicts(3, 4, 3, seed=3)
    scs = [Scenario.from_dict(d) for d in ds]
    with pytest.raises(ValueError, match=r"pattern=True\) needs scan=True \(scenario 0"):
        ScenarioBatch(scs, pattern=True)
    bare = copy.deepcopy(ds[1])
    del bare["environment_params"]["radar_scan"]["pattern"]
    with pytest.raises(ValueError, match=r"scenario 1 has no radar_scan.pattern"):
        ScenarioBatch([scs[0], Scenario.from_dict(bare), scs[2]], scan=True, pattern=True)
    other = copy.deepcopy(ds[2])
    other["environment_params"]["radar_scan"]["pattern"]["gain_db"] = [-3, -12]   # another L: radar_scan is shared
    with pytest.raises(ValueError, match=r"scenario 2's radar_scan .* differs"):
        ScenarioBatch([scs[0], scs[1], Scenario.from_dict(other)], scan=True, pattern=True)
    static = copy.deepcopy(ds[1])
    del static["environment_params"]["radar_scan"]
    with pytest.raises(ValueError, match=r"scenario 1 has no environment_params.radar_scan"):
        ScenarioBatch([scs[0], Scenario.from_dict(static)], scan=True, pattern=True)
    # without the new keyword a pattern is refused as before
    with pytest.raises(ValueError, match=r"scenario 0 has a radar_scan.pattern"):
        ScenarioBatch(scs, scan=True)
    with pytest.raises(ValueError, match="scan=True"):
        ScenarioBatch(scs)


# ---- C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    entry.build()
    return ctypes.CDLL(_native.LIB_PATH)


def test_header_binding_and_library_declare_the_entry_point(built):
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int macjd_env_step_scan_pe_pattern(const macjd_scenario* s, const macjd_step_io* io, const macjd_scan_io* scan, "
            "const macjd_scan_pe_io* scan_pe, const macjd_scan_pe_pattern_io* pattern, void* hip_stream);") in flat
    assert "typedef struct macjd_scan_pe_pattern_io {" in hdr
    assert "#define MACJD_PE_SCAN_PATTERN_ROWS(R, L) ((R) + 4 * ((L) + 2) * (R))" in hdr
    sym = "macjd_env_step_scan_pe_pattern"
    assert sym in _native.EXPORTS and hasattr(built, sym)
    assert f"#define MACJD_ABI_VERSION {_native.ABI_VERSION}" in hdr and _native.ABI_VERSION >= 10
    built.macjd_abi_version.restype = ctypes.c_int
    assert built.macjd_abi_version() == _native.ABI_VERSION


def test_scan_pe_pattern_io_layout_and_row_macro_match_the_header():
    D = _native.ScanPePatternIO
    fields = [n for n, *_ in D._fields_]
    assert fields == ["tables", "stride", "n_levels", "reserved"]
    sizes = [(2, 1), (4, 4), (7, 6), (16, 4)]   # (R, L)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd.h"\n'
           'int main(){printf("%zu %zu %zu %zu", sizeof(macjd_scan_pe_pattern_io), sizeof(macjd_step_io), sizeof(macjd_scan_pe_io), '
           'sizeof(macjd_scan_io));\n'
           + "".join(f'printf(" %zu", offsetof(macjd_scan_pe_pattern_io, {f}));\n' for f in fields)
           + "".join(f'printf(" %d", MACJD_PE_SCAN_PATTERN_ROWS({R}, {L}));\n' for R, L in sizes)
           + 'printf("\\n");return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(D)
    assert out[1] == ctypes.sizeof(_native.StepIO) and out[2] == ctypes.sizeof(_native.ScanPeIO)   # unchanged neighbours
    assert out[3] == ctypes.sizeof(_native.ScanIO)
    for name, off in zip(fields, out[4:8]):
        assert getattr(D, name).offset == off, name
    for (R, L), rows in zip(sizes, out[8:]):
        assert rows == scenario_mod.pe_scan_pattern_rows(R, L) == R * (4 * L + 9)


# ---- reference coverage ----------------------------------------------------------------------------------------------
def _covered(models, tracked, searched, dec):
    ct, cj = sum(m.count_target for m in models), sum(m.count_jammer for m in models)
    assert ct.min() > 0 and cj.min() > 0, (ct, cj)                               # every level 0..L + 1 on both paths
    assert tracked > 0 and searched > 0 and dec > 0, (tracked, searched, dec)
    full = models[cases.FULL_ENV]
    assert full.count_target[1:].sum() == 0 and full.count_jammer[1:].sum() == 0   # that env only ever sees main lobes


@pytest.mark.parametrize("J,R,L", cases.MODEL_CASES)
def test_reference_model_meets_every_level_on_the_model_tests_inputs(J, R, L):
    """The supplied-uniform inputs of the GPU file's test against the model (33 envs x 12 steps), per size and L."""
    models = [spm.ScanPatternModel(sc, 1) for sc in cases.model_scenarios(J, R, L)]
    assert all(m.L == L for m in models)
    tracked = searched = dec = 0
    for T, P, u in cases.model_actions(J, R, L):
        for e, m in enumerate(models):
            dec += int(m.n_deception_draws(T[e:e + 1], P[e:e + 1]).sum())
            tracked += int(m.track.sum())                                        # FSM states at the start of the step
            searched += int((~m.track).sum())
            m.step(T[e:e + 1], P[e:e + 1], u[e:e + 1])
    _covered(models, tracked, searched, dec)


def test_reference_model_meets_every_level_on_the_single_env_tests_inputs():
    """The Philox-driven inputs of the GPU file's batch-equals-single-envs test (3j/4r, 40 envs x 30 steps, a masked reset
    at step 17): the model is driven with the generator's own values (the oracle's restatement of it)."""
    c = cases.SINGLES
    J, R, E = c["J"], c["R"], c["E"]
    models = [spm.ScanPatternModel(sc, 1) for sc in cases.scenarios(J, R, E, c["seed"], c["env_offset"], L=c["L"])]
    lib = oracle_lib()
    episode = np.zeros(E, dtype=np.int64)
    step = np.zeros(E, dtype=np.int64)
    tracked = searched = dec = 0
    for t, (T, P) in enumerate(cases.singles_actions()):
        if t == c["reset_at"]:
            for e in range(0, E, 3):
                models[e].reset()
                episode[e] += 1
                step[e] = 0
        for e, m in enumerate(models):
            u = np.array([[lib.macjd_oracle_uniform(c["env_seed"], c["env_offset"] + e, int(episode[e]), int(step[e]), k)
                           for k in range(R + J)]])
            dec += int(m.n_deception_draws(T[e:e + 1], np.nan_to_num(P[e:e + 1], nan=0.0)).sum())
            tracked += int(m.track.sum())
            searched += int((~m.track).sum())
            m.step(T[e:e + 1], P[e:e + 1], u, arith32=True)
        step += 1
    _covered(models, tracked, searched, dec)
