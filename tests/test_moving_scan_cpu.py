"""Moving scenarios with scanning radars (``environment_params.motion`` and ``radar_scan`` on one clock; include/macjd.h,
macjd_motion_scan_io), host side: acceptance and refusal, the per-frame scan / pattern tables of ``Scenario.motion_tables``,
the C-ABI's declarations and struct layout, the Python layers' refusals, and the coverage of the model run that
tests/test_moving_scan_gpu.py compares the kernels against (tests/moving_scan_cases.py, tests/moving_scan_model.py)."""
import copy
import ctypes
import os
import re
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

import __graft_entry__ as entry
import motion_cases
import moving_scan_cases as cases
from _harness import REPO

from macjd_amd import _native
from macjd_amd.scenario import (PE_SCAN_PATTERN_ROWS, PE_SCAN_ROWS, Scenario, ScenarioBatch, pe_scan_pattern_rows, pe_scan_rows)

PKG = os.path.join(REPO, "ma-cjd-cooperative-jamming-decision-making-via-marl_amd")
F = cases.F


# ---- acceptance and refusal ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [False, True])
def test_motion_with_radar_scan_on_one_clock_is_accepted(pattern):
    sc, frames = cases.case(3, 4, pattern)
    assert sc.moving and sc.scanning and sc.scan_pattern_levels == (4 if pattern else 0)
    R, J = 4, 3
    mt = sc.motion_tables
    assert mt["scan_frames"].shape == (F, pe_scan_rows(R, J)) and mt["scan_frames"].dtype == np.float64
    assert ("pattern_frames" in mt) == pattern
    if pattern:
        assert mt["pattern_frames"].shape == (F, pe_scan_pattern_rows(R, 4)) and mt["pattern_frames"].dtype == np.float64
    assert mt["frames"].shape == (F, 6 * R + 3 * J + J * R) and mt["snr_no"].shape == (F, R)   # as without radar_scan
    assert all(fr.scanning and not fr.moving for fr in frames)
    # an integer and a float spelling of the same clock are one clock
    d = cases.moving_scan_dict(3, 4, pattern)
    d["environment_params"]["motion"]["step_seconds"] = 1
    d["environment_params"]["radar_scan"]["step_seconds"] = 1.0
    assert Scenario.from_dict(d, config=motion_cases.config(3)).moving


@pytest.mark.parametrize("motion_dt,scan_dt", [(0.5, 0.25), (0.25, 0.5), (0.5, 0.5000001)])
def test_two_clocks_are_refused(motion_dt, scan_dt):
    d = cases.moving_scan_dict(3, 4, step_seconds=scan_dt)
    d["environment_params"]["motion"]["step_seconds"] = motion_dt
    with pytest.raises(ValueError, match=r": environment_params\.motion together with radar_scan is not supported.*"
                                         r"step_seconds.*must be equal"):
        Scenario.from_dict(d)


def test_scenario_batches_keep_refusing_moving_scenarios():
    sc, _ = cases.case(3, 4, True)
    with pytest.raises(ValueError, match="moving scenarios are not supported in per-env scenario batches"):
        ScenarioBatch([sc], scan=True, pattern=True)


# ---- the per-frame tables --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,R,pattern", cases.CASES)
def test_frame_rows_are_the_columns_of_a_scenario_batch_of_that_frame(J, R, pattern):
    sc, frames = cases.case(J, R, pattern)
    mt = sc.motion_tables
    changed = 0
    for f in range(F):
        b = ScenarioBatch([frames[f]], scan=True, pattern=pattern)
        assert mt["scan_frames"][f].tobytes() == np.ascontiguousarray(b.scan_tables[:, 0]).tobytes(), f
        assert mt["frames"][f].tobytes() == np.ascontiguousarray(b.tables[:, 0]).tobytes(), f
        if pattern:
            assert mt["pattern_frames"][f].tobytes() == np.ascontiguousarray(b.pattern_tables[:, 0]).tobytes(), f
        changed += mt["scan_frames"][f].tobytes() != mt["scan_frames"][0].tobytes()
    assert changed == F - 1                                       # every frame's bearings differ from frame 0's
    # rows that cannot depend on the frame: beam widths, sweeps, initial azimuths
    assert (mt["scan_frames"][:, :4 * R] == mt["scan_frames"][0, :4 * R]).all()
    assert len(PE_SCAN_ROWS) == 11 and len(PE_SCAN_PATTERN_ROWS) == 5


@pytest.mark.parametrize("pattern", [False, True])
def test_zero_velocities_give_frame_zero_everywhere(pattern):
    cfg = cases.zero_velocity(cases.moving_scan_dict(3, 4, pattern))
    sc = Scenario.from_dict(cfg, config=motion_cases.config(6))
    static = copy.deepcopy(cfg)
    del static["environment_params"]["motion"]
    b = ScenarioBatch([Scenario.from_dict(static, config=motion_cases.config(6))], scan=True, pattern=pattern)
    mt = sc.motion_tables
    for f in range(6):
        assert mt["scan_frames"][f].tobytes() == np.ascontiguousarray(b.scan_tables[:, 0]).tobytes()
        if pattern:
            assert mt["pattern_frames"][f].tobytes() == np.ascontiguousarray(b.pattern_tables[:, 0]).tobytes()


def test_shipped_config_loads():
    sc = Scenario.from_yaml(os.path.join(PKG, "config", "scenario_3j4r_moving_scan.yaml"))
    assert (sc.num_jammers, sc.num_radars, sc.episode_limit) == (3, 4, 100)
    assert sc.moving and sc.scanning and sc.scan_pattern_levels == 4
    assert sc.motion["step_seconds"] == sc.radar_scan["step_seconds"] == 0.5
    assert sc.motion_tables["pattern_frames"].shape == (100, pe_scan_pattern_rows(4, 4))


# ---- header, ctypes mirror, exports ----------------------------------------------------------------------------------
def test_abi_declares_the_entry_point_and_the_struct_layout_matches():
    entry.build()
    hdr = open(os.path.join(REPO, "include", "macjd.h")).read()
    assert re.search(r"#define MACJD_ABI_VERSION 12\b", hdr) and _native.ABI_VERSION == 12
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int macjd_env_step_moving_scan\(const macjd_scenario\* s, const macjd_step_io\* io, "
                     r"const macjd_motion_io\* motion,\s*const macjd_scan_io\* scan, const macjd_motion_scan_io\* motion_scan, "
                     r"void\* hip_stream\);", code)
    assert "macjd_env_step_moving_scan" in _native.EXPORTS
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "macjd_env_step_moving_scan")
    lib.macjd_abi_version.restype = ctypes.c_int
    assert lib.macjd_abi_version() == 12
    fields = ["scan_frames", "pattern_frames", "n_levels", "reserved"]
    assert [f[0] for f in _native.MotionScanIO._fields_] == fields
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "macjd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(macjd_motion_scan_io), ' + ", ".join(f"offsetof(macjd_motion_scan_io, {f})" for f in fields) +
           ', sizeof(macjd_motion_io), sizeof(macjd_scan_io));return 0;}\n')
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as fh:
        fh.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
    out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_native.MotionScanIO)
    assert out[1:5] == [getattr(_native.MotionScanIO, f).offset for f in fields]
    assert out[5] == ctypes.sizeof(_native.MotionIO) and out[6] == ctypes.sizeof(_native.ScanIO)   # existing structs: unchanged


# ---- the Python layers' refusals (no device needed: they are decided before anything is launched) ---------------------
def _stub_env():
    from macjd_amd.simulation.environment import BatchedElectromagneticEnvironment as Env
    env = object.__new__(Env)
    env._scan_io, env._motion_io, env._motion_scan_io = object(), object(), object()
    env._pe_tables = None
    env.num_jammers, env.num_radars = 3, 4
    return env


def test_environment_refuses_what_rests_on_the_counter_alone():
    env = _stub_env()
    with pytest.raises(RuntimeError, match="step_many: not available with scanning radars"):
        env.step_many(None, None, None, None, None)
    with pytest.raises(RuntimeError, match="frame_states: not available with scanning radars"):
        env.frame_states()
    with pytest.raises(RuntimeError, match="time_step_kernel: not available with scanning radars"):
        env.time_step_kernel(None, None, 2)
    with pytest.raises(RuntimeError, match="time_step_many_kernel: not available with scanning radars"):
        env.time_step_many_kernel(None, None, None, None, None, 2)
    with pytest.raises(RuntimeError, match="episode_scan_args: not available with a moving scenario"):
        env.episode_scan_args()
    assert env.step_many_has_production_form() is False
    env._motion_scan_io = None                    # the moving, non-scanning env of that size has the many-step launch
    assert env.step_many_has_production_form() is True


def test_runner_reports_no_whole_episode_launch():
    from macjd_amd.runners.episode_runner import BatchedEpisodeRunner as Runner
    env = _stub_env()
    env.scenario = SimpleNamespace(moving=True, scanning=True)
    env.scenario_batch, env.kernel_flags = None, 0
    stub = SimpleNamespace(env=env, device=SimpleNamespace(type="cuda"), mac=SimpleNamespace(agent=None))
    stub._closed_loop_conditions = lambda per_env: Runner._closed_loop_conditions(stub, per_env)
    assert Runner.closed_loop_available(stub) is False and Runner.closed_loop_pe_available(stub) is False
    assert Runner.moving_rollout_available(stub) is False


# ---- the model run the GPU file compares against ---------------------------------------------------------------------
@pytest.mark.parametrize("J,R,pattern", cases.CASES)
def test_model_run_covers_both_lobes_every_level_a_followed_target_and_clear_uniforms(J, R, pattern):
    steps, m = cases.model_run(J, R, pattern)
    sc, frames = cases.case(J, R, pattern)
    print(f"{J}j/{R}r pattern={pattern}: target paths per level {m.count_target.tolist()}, recorded jammer actions per level "
          f"{m.count_jammer.tolist()}, followed detections {m.followed}, min |u - pd| {m.min_margin:.3e}")
    assert m.count_target[0] > 0 and m.count_target[-1] > 0          # the target through the main and the side lobe
    assert m.count_jammer[0] > 0 and m.count_jammer[-1] > 0          # a recorded jammer action in each
    if pattern:
        assert len(m.count_jammer) == 6 and (m.count_jammer > 0).all()   # every level 0..L + 1 taken by a jammer action
    assert m.followed > 0            # a detection in a frame whose bear_tgt differs from frame 0's; theta_a == that bear_tgt
    assert m.min_margin > 1e-9       # no detection can flip within the kernel's 1e-12 relative pd error
    # one batch holds several frames, the clamp at F - 1 included
    assert any(len(set(fr.tolist())) > 1 for _, _, _, fr, _ in steps)
    counters = m.step_count
    assert counters.max() > F and sorted(set(counters.tolist())) == [cases.MODEL["steps"] - cases.MODEL["reset_at"], cases.MODEL["steps"]]
    # the bearings really move: frame 5's bear_tgt differs from frame 0's for some radar
    bt = sc.motion_tables["scan_frames"][:, 4 * R:5 * R]
    assert (bt[5].view(np.uint64) != bt[0].view(np.uint64)).any()
