"""Radar-jamming environment on MI355X.

Two classes over the same HIP kernel (csrc/macjd_env.hip, C-ABI include/macjd.h):

``BatchedElectromagneticEnvironment``
    E environments advanced per launch; actions, state and outputs stay in device tensors, no host
    synchronisation inside ``step``.  This is the hot-path object (BASELINE.json: batch_envs=4096).

``ElectromagneticEnvironment``
    Drop-in for the reference class of the same name (reference simulation/environment.py:29-573):
    same constructor ``(config, sim_config_path)``, ``reset() -> np.float32[S]``,
    ``step(list[(T_i, P_i)]) -> (obs_list, reward, terminated, info)``, ``get_state/get_obs/
    get_agent_obs/get_avail_actions/get_env_info/close`` and the same exceptions.  It runs ONE
    environment through the same kernel and, like the reference, consumes its Monte-Carlo uniforms
    from the global ``np.random`` stream (R draws for the radars, then one per valid deception action,
    environment.py:341,430), so ``np.random.seed(s)`` reproduces the reference's trajectory.

There is no CPU implementation of ``step`` in the product: both classes require a HIP device and
libmacjd_hip.so and raise otherwise.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..scenario import (DEFAULT_SIM_CONFIG_PATH, DEG_PER_RAD, FOUR_PI_CUBED, MovingScanScenarioBatch, MovingScenarioBatch,
                        Scenario, ScenarioBatch)

RADAR_STATE_SEARCH = "SEARCH"  # core/radar.py:5-7
RADAR_STATE_TRACK = "TRACK"


def _require_device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(
            "macjd_amd environment step needs a HIP device (torch.cuda.is_available() is False); "
            "there is no CPU fallback for the environment kernel.")
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"macjd_amd environment tensors must live on a HIP device, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class BatchedElectromagneticEnvironment:
    """E independent copies of the reference environment, one HIP launch per step.

    Layout in HBM (all caller-visible tensors are views of these):
      track   uint8 [R, E]   radar-major so that radar r's flags of 64 consecutive envs are one line
      step    int32 [E]
      reward  f32 [E]; r_dpj f32 [E, 3]; terminated uint8 [E]
      pd, snr f32 [R, E]     radar-major (exposed as [E, R] transposed views)
    Actions may come in any strided layout; agent-major storage ([J, E], i.e. ``T.t()`` of a
    ``[J, E]`` tensor) gives fully coalesced loads.
    """

    # The observation is a pure function of static scenario parameters (environment.py:479-510; nothing
    # in step() moves an entity), so runners may fill their obs / state / avail rows once.
    observation_is_static = True
    PE_TILE = 256            # envs per tile of the per-env tables (= the lane kernel's workgroup at streaming sizes)
    pe_tiled = True          # A/B hook: False keeps the plain [rows, E] SoA on the device
    moving_batch = None      # the per-env moving scenario batch (moving_batch=...), None otherwise
    _motion_pe_io = None     # ... and its argument block (include/macjd.h, macjd_motion_pe_io)
    moving_scan_batch = None   # the per-env moving scanning scenario batch (moving_scan_batch=...), None otherwise
    _motion_scan_pe_io = None  # ... and its beam-frame block (include/macjd.h, macjd_motion_scan_pe_io)

    def __init__(self, config: Any = None, sim_config_path: str = DEFAULT_SIM_CONFIG_PATH,
                 batch_envs: Optional[int] = None, device=None, seed: Optional[int] = None,
                 env_offset: int = 0, scenario: Optional[Scenario] = None, verbose: bool = False,
                 scenario_batch: Optional[ScenarioBatch] = None, moving_batch: Optional[MovingScenarioBatch] = None,
                 moving_scan_batch: Optional[MovingScanScenarioBatch] = None):
        """``moving_scan_batch``: one scenario that both MOVES and SCANS per env (``MovingScanScenarioBatch``; exclusive with
        ``moving_batch``, ``scenario_batch`` and ``scenario``): every env steps on its own frame tables AND its own beam frames
        (include/macjd.h, macjd_motion_pe_io + macjd_motion_scan_pe_io), uploaded from the batch's host frames or compiled on the
        device by macjd_motion_pe_compile and macjd_motion_scan_pe_compile back to back.  Single steps and resets only.

        ``moving_batch``: one MOVING scenario per env (``MovingScenarioBatch``; exclusive with ``scenario_batch``): every
        env steps on its own frame tables (include/macjd.h, macjd_motion_pe_io), uploaded from the batch's host frames or
        compiled on the device from its input columns (macjd_motion_pe_compile).

        ``scenario_batch``: one scenario PER ENV (radar / jammer positions, threat levels, powers differing
        between envs — SURVEY.md 8f-3); its tables live in HBM as an SoA that every step streams, and the
        observation becomes a per-env [E, S] tensor (still constant in time).  A scanning batch
        (``ScenarioBatch(..., scan=True)``) also streams each env's scan tables; its theta_a columns move.  With
        ``pattern=True`` each env's stepped antenna pattern tables are streamed too (macjd_env_step_scan_pe_pattern)."""
        self.scenario_batch = scenario_batch
        self.moving_batch = moving_batch
        self.moving_scan_batch = moving_scan_batch
        if moving_scan_batch is not None:
            if moving_batch is not None:
                raise ValueError("moving_scan_batch and moving_batch are exclusive (a per-env moving batch either scans or does not)")
            if scenario_batch is not None:
                raise ValueError("moving_scan_batch and scenario_batch are exclusive (a per-env batch is either static or moving)")
            if scenario is not None:
                raise ValueError("moving_scan_batch brings its own scenario (MovingScanScenarioBatch.base): do not pass `scenario` too")
            scenario = moving_scan_batch.base
            if batch_envs is None:
                batch_envs = moving_scan_batch.n_envs
            if int(batch_envs) != moving_scan_batch.n_envs:
                raise ValueError(f"batch_envs ({batch_envs}) != scenarios in the moving scanning batch ({moving_scan_batch.n_envs})")
        if moving_batch is not None:
            if scenario_batch is not None:
                raise ValueError("moving_batch and scenario_batch are exclusive (a per-env batch is either static or moving)")
            if scenario is not None and scenario is not moving_batch.base:
                raise ValueError("moving_batch brings its own scenario (MovingScenarioBatch.base): do not pass `scenario` too")
            scenario = moving_batch.base
            if batch_envs is None:
                batch_envs = moving_batch.n_envs
            if int(batch_envs) != moving_batch.n_envs:
                raise ValueError(f"batch_envs ({batch_envs}) != scenarios in the moving batch ({moving_batch.n_envs})")
        if scenario_batch is not None:
            scenario = scenario_batch.base
            if batch_envs is None:
                batch_envs = scenario_batch.n_envs
            if int(batch_envs) != scenario_batch.n_envs:
                raise ValueError(f"batch_envs ({batch_envs}) != scenarios in the batch ({scenario_batch.n_envs})")
        self.scenario = scenario if scenario is not None else Scenario.from_yaml(sim_config_path, config)
        sc = self.scenario
        pe_scan = scenario_batch is not None and getattr(scenario_batch, "scan_tables", None) is not None
        pe_pattern = pe_scan and getattr(scenario_batch, "pattern_tables", None) is not None
        if sc.scanning and scenario_batch is not None and not pe_scan:
            raise ValueError("scanning radars (environment_params.radar_scan) need a scanning per-env scenario batch "
                             "(ScenarioBatch(..., scan=True)); this batch carries no scan tables")
        if sc.moving and scenario_batch is not None:
            raise ValueError("a moving scenario (environment_params.motion) is not supported with per-env scenario batches")
        # scanning beams (environment_params.radar_scan): theta_a moves every step, so the observation does too; moving
        # entities (environment_params.motion): the position columns do
        self.observation_is_static = not sc.scanning and not sc.moving
        self.num_jammers, self.num_radars = sc.num_jammers, sc.num_radars
        self.episode_limit = sc.episode_limit
        self.state_dim = self.obs_dim = self.agent_obs_dim = sc.state_dim
        self.action_dim_discrete = sc.n_actions
        self.action_dim_continuous = 1
        if batch_envs is None:
            batch_envs = getattr(config, "batch_envs", 1)
        self.batch_envs = int(batch_envs)
        if self.batch_envs < 1:
            raise ValueError(f"batch_envs must be >= 1, got {batch_envs}")
        self.seed = int(seed if seed is not None else getattr(config, "seed", 0) or 0)
        self.env_offset = int(env_offset)
        self.device = _require_device(device)
        self._lib = _native.load()
        with torch.cuda.device(self.device):
            # a batch under a stepped pattern brings every env's level tables itself: the handle stays pattern-free, so
            # that macjd_env_reset_scan_pe (az0 per env does not depend on the pattern) takes it
            self._handle = _native.ScenarioHandle(sc, scan_pattern=not pe_pattern and moving_scan_batch is None)
        E, R, J = self.batch_envs, self.num_radars, self.num_jammers
        dev = self.device
        self._track = torch.zeros((R, E), dtype=torch.uint8, device=dev)
        self._step = torch.zeros(E, dtype=torch.int32, device=dev)
        # per-env episode index: advanced by every reset (in the reset kernel, so replayed HIP graphs advance it too)
        # and part of the in-kernel Philox counter — each episode draws fresh Monte-Carlo values like the reference's
        # np.random stream does (environment.py:341,430)
        self._episode = torch.zeros(E, dtype=torch.int32, device=dev)
        self._reward = torch.zeros(E, dtype=torch.float32, device=dev)
        self._r_dpj = torch.zeros((E, 3), dtype=torch.float32, device=dev)
        self._terminated = torch.zeros(E, dtype=torch.uint8, device=dev)
        self._pd = torch.zeros((R, E), dtype=torch.float32, device=dev)
        self._snr = torch.zeros((R, E), dtype=torch.float32, device=dev)
        self._state_vec = torch.from_numpy(sc.state_vector()).to(dev)
        self._avail = torch.ones((1, 1, sc.n_actions), dtype=torch.int32, device=dev)
        self._snr_no = torch.from_numpy(sc.tables["radar_snr_no"]).to(dev)
        self._pe_tables = self._pe_flags = self._state_vecs = None
        if scenario_batch is not None:
            # tiled (AoSoA) device form: [n_tiles, rows, PE_TILE] — a workgroup's 256 consecutive envs read one
            # contiguous block per step (the plain [rows, E] SoA is 6R+3J+JR streams E*8 bytes apart)
            self._pe_tile = self.PE_TILE if getattr(self, "pe_tiled", True) else 0
            tb, fl = scenario_batch.tables, scenario_batch.flags
            stb = scenario_batch.scan_tables if pe_scan else None
            ptb = scenario_batch.pattern_tables if pe_pattern else None
            if self._pe_tile:
                w = self._pe_tile
                n_tiles = (E + w - 1) // w
                pad = n_tiles * w - E
                tile = lambda a: np.ascontiguousarray(
                    np.pad(a, ((0, 0), (0, pad))).reshape(a.shape[0], n_tiles, w).transpose(1, 0, 2))
                tb, fl = tile(tb), tile(fl)
                stb = tile(stb) if pe_scan else None
                ptb = tile(ptb) if pe_pattern else None
            self._pe_tables = torch.from_numpy(tb).to(dev)       # f64 [rows, E] or [n_tiles, rows, w]
            self._pe_flags = torch.from_numpy(fl).to(dev)        # u8  [J*R, E] or [n_tiles, J*R, w]
            self._state_vecs = torch.from_numpy(scenario_batch.state_vectors).to(dev)   # f32 [E, S]
            self._snr_no = torch.from_numpy(scenario_batch.snr_no).to(dev)          # f64 [E, R]
        self._theta_a = self._state_dyn = self._snr_no_step = None
        self._scan_io = self._scan_pe_io = self._scan_pe_tables = None
        self._scan_pe_pattern_io = self._scan_pe_pattern_tables = None
        if pe_scan:
            # per-env scan tables (include/macjd.h, macjd_scan_pe_io) in the device form of pe_tables; beams, state rows
            # and the per-step SNR without jamming start from each env's own az0 / state vector / main-lobe snr_no
            self._scan_pe_tables = torch.from_numpy(stb).to(dev)     # f64 [10R + JR, E] or [n_tiles, 10R + JR, w]
            az0 = torch.from_numpy(np.ascontiguousarray(scenario_batch.scan_tables[3 * R:4 * R])).to(dev)   # f64 [R, E]
            self._theta_a = az0.contiguous()
            self._state_dyn = self._state_vecs.clone()
            self._state_dyn[:, sc.theta_a_columns] = az0.t().to(torch.float32)
            self._snr_no_step = self._snr_no.t().to(torch.float32).contiguous()
            sp = self._scan_pe_io = _native.ScanPeIO()
            sp.tables, sp.stride = self._scan_pe_tables.data_ptr(), E
            if pe_pattern:
                # per-env level tables (include/macjd.h, macjd_scan_pe_pattern_io), same device form
                self._scan_pe_pattern_tables = torch.from_numpy(ptb).to(dev)   # f64 [R + 4(L+2)R, E] or [n_tiles, ..., w]
                pp = self._scan_pe_pattern_io = _native.ScanPePatternIO()
                pp.tables, pp.stride, pp.n_levels = self._scan_pe_pattern_tables.data_ptr(), E, scenario_batch.scan_pattern_levels
        elif sc.scanning and moving_scan_batch is None:
            # beam azimuths f64 [R, E] (radar-major like track), the per-env state rows f32 [E, S] whose theta_a columns the
            # kernel rewrites every step (get_state / get_obs are views of it: one address for captured graphs), and the
            # per-step SNR without jamming (main or side lobe) f32 [R, E]
            az0 = torch.from_numpy(sc.scan_tables["az0"]).to(dev)
            self._theta_a = az0.view(R, 1).repeat(1, E).contiguous()
            st = torch.from_numpy(sc.state_vector()).to(dev)
            st[sc.theta_a_columns] = az0.to(torch.float32)
            self._state_dyn = st.view(1, -1).repeat(E, 1).contiguous()
            self._snr_no_step = torch.from_numpy(sc.tables["radar_snr_no"]).to(dev).to(torch.float32).view(R, 1).repeat(1, E)
            self._snr_no_step = self._snr_no_step.contiguous()
        if sc.scanning and moving_scan_batch is None:
            si = self._scan_io = _native.ScanIO()
            si.theta_a, si.a_se, si.a_sx = self._theta_a.data_ptr(), 1, E
            si.state, si.st_se = self._state_dyn.data_ptr(), self._state_dyn.stride(0)
            si.st_col0, si.st_col_step = sc.theta_a_col0, sc.theta_a_col_step
            si.snr_no, si.sn_se, si.sn_sx = self._snr_no_step.data_ptr(), 1, E
        self._motion_io = self._motion_keep = self._motion_scan_io = None
        self._motion_pe_io = self._motion_scan_pe_io = None
        if moving_scan_batch is not None:
            self._init_moving_batch(moving_scan_batch)
            self._init_moving_scan_batch(moving_scan_batch)
        elif moving_batch is not None:
            self._init_moving_batch(moving_batch)
        elif sc.moving:
            # per-step frame tables (include/macjd.h, macjd_motion_io): f64 [F, rows], u8 [F, J*R], f64 [F, R], the
            # positions f32 [F + 1, 2R + 2J] with their state columns; the per-env state rows f32 [E, S] start as frame 0
            # (get_state / get_obs are views of them: one address for captured graphs) and the per-step SNR without
            # jamming f32 [R, E] as frame 0's
            mt = sc.motion_tables
            # With scanning beams (one clock, include/macjd.h, macjd_motion_scan_io) the state rows, beams and per-step SNR
            # set up above serve both: the step rewrites their theta_a AND position columns, and the per-frame scan tables
            # f64 [F, 10R + JR] (under a stepped pattern also the level tables f64 [F, R + 4(L+2)R]) are uploaded too.
            keep = {k: torch.from_numpy(np.ascontiguousarray(mt[k])).to(dev)
                    for k in ("frames", "flags", "snr_no", "positions", "position_columns", "scan_frames", "pattern_frames")
                    if k in mt}
            self._motion_keep = keep
            self._pos_cols = keep["position_columns"].to(torch.int64)
            if self._state_dyn is None:
                st = torch.from_numpy(sc.state_vector()).to(dev)
                self._state_dyn = st.view(1, -1).repeat(E, 1).contiguous()
                self._snr_no_step = keep["snr_no"][0].to(torch.float32).view(R, 1).repeat(1, E).contiguous()
            self._state_dyn[:, self._pos_cols] = keep["positions"][0]
            mo = self._motion_io = _native.MotionIO()
            mo.frames, mo.frame_flags, mo.frame_snr_no = keep["frames"].data_ptr(), keep["flags"].data_ptr(), keep["snr_no"].data_ptr()
            mo.positions, mo.position_columns = keep["positions"].data_ptr(), keep["position_columns"].data_ptr()
            mo.n_frames, mo.n_pos = int(mt["frames"].shape[0]), int(mt["positions"].shape[1])
            mo.state, mo.st_se = self._state_dyn.data_ptr(), self._state_dyn.stride(0)
            mo.snr_no, mo.sn_se, mo.sn_sx = self._snr_no_step.data_ptr(), 1, E
            if sc.scanning:
                mo.snr_no = None   # the per-step value travels in the beam block's snr_no
                ms = self._motion_scan_io = _native.MotionScanIO()
                ms.scan_frames = keep["scan_frames"].data_ptr()
                ms.pattern_frames = keep["pattern_frames"].data_ptr() if "pattern_frames" in keep else None
                ms.n_levels = sc.scan_pattern_levels if "pattern_frames" in keep else 0
        self._io = _native.StepIO()
        self.kernel_flags = 0  # A/B hook: _native.STEP_LANE_KERNEL / STEP_SLOT_KERNEL force one kernel variant
        if verbose:
            print(f"Batched environment: {E} envs x {J} jammers / {R} radars on {dev} (from {sc.source})")

    def _init_moving_batch(self, mb: MovingScenarioBatch) -> None:
        """Per-env frame tables on the device (include/macjd.h, macjd_motion_pe_io) at env tile PE_TILE: uploaded from the
        batch's host frames, or written by ONE launch of the device frame compiler from its input columns; the per-env state
        rows f32 [E, S] start as each env's frame 0 and the per-step SNR without jamming f32 [R, E] as frame 0's."""
        E, R, J, dev = self.batch_envs, self.num_radars, self.num_jammers, self.device
        w = int(self.PE_TILE)
        F, n_pos = mb.n_frames, 2 * R + 2 * J
        n_tiles = (E + w - 1) // w
        rows = 6 * R + 3 * J + J * R
        keep = {"position_columns": torch.from_numpy(np.ascontiguousarray(mb.position_columns, dtype=np.int32)).to(dev)}
        if mb.host_compiled:
            for k, a in mb.tiled(w).items():
                keep[k] = torch.from_numpy(a).to(dev)
        else:
            ins = mb.tiled_compile_inputs(w)
            keep["in_tables"] = torch.from_numpy(ins["in_tables"]).to(dev)
            keep["in_weak"] = torch.from_numpy(ins["in_weak"]).to(dev)
            keep["frames"] = torch.zeros((n_tiles, F, rows, w), dtype=torch.float64, device=dev)
            keep["flags"] = torch.zeros((n_tiles, F, J * R, w), dtype=torch.uint8, device=dev)
            keep["snr_no"] = torch.zeros((n_tiles, F, R, w), dtype=torch.float64, device=dev)
            keep["positions"] = torch.zeros((n_tiles, F + 1, n_pos, w), dtype=torch.float32, device=dev)
            d = _native.MotionPeCompileDesc()
            d.n_envs, d.n_radars, d.n_jammers, d.n_frames, d.tile = E, R, J, F, w
            d.four_pi_cubed = FOUR_PI_CUBED
            d.pd_A, d.pd_c1, d.pd_denB = self.scenario.pd_consts
            d.in_tables, d.in_weak = keep["in_tables"].data_ptr(), keep["in_weak"].data_ptr()
            d.frames, d.frame_flags = keep["frames"].data_ptr(), keep["flags"].data_ptr()
            d.frame_snr_no, d.positions = keep["snr_no"].data_ptr(), keep["positions"].data_ptr()
            with torch.cuda.device(dev):
                _native.check(self._lib.macjd_motion_pe_compile(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                              "macjd_motion_pe_compile")
        assert tuple(keep["frames"].shape) == (n_tiles, F, rows, w) and tuple(keep["positions"].shape) == (n_tiles, F + 1, n_pos, w)
        self._motion_keep = keep
        self._pe_tile = w
        self._pos_cols = keep["position_columns"].to(torch.int64)
        untile = lambda t: t.permute(0, 2, 1).reshape(n_tiles * w, -1)[:E]      # [n_tiles, k, w] -> [E, k]
        self._state_vecs = torch.from_numpy(mb.state_vectors).to(dev)
        self._state_dyn = self._state_vecs.clone()
        self._state_dyn[:, self._pos_cols] = untile(keep["positions"][:, 0])
        self._snr_no_step = untile(keep["snr_no"][:, 0]).to(torch.float32).t().contiguous()   # f32 [R, E]
        mp = self._motion_pe_io = _native.MotionPeIO()
        mp.frames, mp.frame_flags, mp.frame_snr_no = keep["frames"].data_ptr(), keep["flags"].data_ptr(), keep["snr_no"].data_ptr()
        mp.positions, mp.position_columns = keep["positions"].data_ptr(), keep["position_columns"].data_ptr()
        mp.n_frames, mp.n_pos, mp.tile = F, n_pos, w
        mp.state, mp.st_se = self._state_dyn.data_ptr(), self._state_dyn.stride(0)
        mp.snr_no, mp.sn_se, mp.sn_sx = self._snr_no_step.data_ptr(), 1, E

    def _init_moving_scan_batch(self, mb: MovingScanScenarioBatch) -> None:
        """After ``_init_moving_batch`` (frame tables, positions, state rows): the per-env beam frames on the device
        (include/macjd.h, macjd_motion_scan_pe_io) at the same env tile — uploaded from the batch's host frames, or written by
        ONE launch of the beam-frame compiler right behind the first compiler on the same stream; beams f64 [R, E] and the
        theta_a columns of the state rows start from each env's own frame-0 az0, the per-step SNR without jamming is carried
        by the beam block (the motion block's is cleared)."""
        E, R, J, dev = self.batch_envs, self.num_radars, self.num_jammers, self.device
        sc, keep, w = self.scenario, self._motion_keep, int(self._pe_tile)
        F, L = mb.n_frames, mb.scan_pattern_levels
        n_tiles = (E + w - 1) // w
        srows, prows = 10 * R + J * R, R + 4 * (L + 2) * R
        if mb.host_compiled:
            assert "scan_frames" in keep and (("pattern_frames" in keep) == (L > 0))
        else:
            keep["scan_in"] = torch.from_numpy(mb.tiled_compile_inputs(w)["scan_in"]).to(dev)
            keep["scan_frames"] = torch.zeros((n_tiles, F, srows, w), dtype=torch.float64, device=dev)
            if L > 0:
                keep["pattern_frames"] = torch.zeros((n_tiles, F, prows, w), dtype=torch.float64, device=dev)
            d = _native.MotionScanPeCompileDesc()
            d.n_envs, d.n_radars, d.n_jammers, d.n_frames, d.tile, d.n_levels = E, R, J, F, w, L
            d.deg_per_rad = DEG_PER_RAD
            d.pd_A, d.pd_c1, d.pd_denB = sc.pd_consts
            d.in_tables, d.scan_in = keep["in_tables"].data_ptr(), keep["scan_in"].data_ptr()
            d.frames, d.frame_snr_no = keep["frames"].data_ptr(), keep["snr_no"].data_ptr()
            d.scan_frames = keep["scan_frames"].data_ptr()
            d.pattern_frames = keep["pattern_frames"].data_ptr() if L > 0 else None
            with torch.cuda.device(dev):
                _native.check(self._lib.macjd_motion_scan_pe_compile(ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream),
                              "macjd_motion_scan_pe_compile")
        assert tuple(keep["scan_frames"].shape) == (n_tiles, F, srows, w)
        assert L == 0 or tuple(keep["pattern_frames"].shape) == (n_tiles, F, prows, w)
        untile = lambda t: t.permute(0, 2, 1).reshape(n_tiles * w, -1)[:E]      # [n_tiles, k, w] -> [E, k]
        az0 = untile(keep["scan_frames"][:, 0, 3 * R:4 * R])                    # f64 [E, R]: each env's frame-0 az0
        self._theta_a = az0.t().contiguous()                                    # f64 [R, E]
        self._state_dyn[:, sc.theta_a_columns] = az0.to(torch.float32)
        si = self._scan_io = _native.ScanIO()
        si.theta_a, si.a_se, si.a_sx = self._theta_a.data_ptr(), 1, E
        si.state, si.st_se = self._state_dyn.data_ptr(), self._state_dyn.stride(0)
        si.st_col0, si.st_col_step = sc.theta_a_col0, sc.theta_a_col_step
        si.snr_no, si.sn_se, si.sn_sx = self._snr_no_step.data_ptr(), 1, E
        self._motion_pe_io.snr_no = None   # the per-step value travels in the beam block's snr_no
        ms = self._motion_scan_pe_io = _native.MotionScanPeIO()
        ms.scan_frames = keep["scan_frames"].data_ptr()
        ms.pattern_frames = keep["pattern_frames"].data_ptr() if L > 0 else None
        ms.n_levels = L

    @property
    def table_bytes(self) -> int:
        """Bytes of the per-env frame tables on the device (per-env moving batches only; with the beam frames of a per-env
        moving scanning batch)."""
        if self._motion_pe_io is None:
            raise AttributeError("table_bytes: not a per-env moving batch (moving_batch=... / moving_scan_batch=...)")
        return int(sum(self._motion_keep[k].numel() * self._motion_keep[k].element_size()
                       for k in ("frames", "flags", "snr_no", "positions", "scan_frames", "pattern_frames")
                       if k in self._motion_keep))

    def _refuse_moving_scan_batch(self, what: str) -> None:
        # theta_a depends on the detections and every env has its own frames: single steps and resets only
        if self._motion_scan_pe_io is not None:
            raise RuntimeError(f"{what}: not available on a per-env moving scanning scenario batch (moving_scan_batch=...)")

    def _refuse_moving_batch(self, what: str) -> None:
        if self._motion_pe_io is not None:
            raise RuntimeError(f"{what}: not available on a per-env moving scenario batch (moving_batch=...)")

    # ---- reference-shaped getters, broadcast views (never materialised per env) ----
    def get_state(self) -> torch.Tensor:
        """f32 [E, S] expanded view of the static state vector (environment.py:479-510); with scanning beams the per-env
        state rows, whose theta_a columns every step / reset rewrites in place (a moving scenario: its position columns)."""
        if self._state_dyn is not None:
            return self._state_dyn
        if self._state_vecs is not None:
            return self._state_vecs
        return self._state_vec.unsqueeze(0).expand(self.batch_envs, -1)

    def get_obs(self) -> torch.Tensor:
        """f32 [E, J, S] expanded view: every agent observes the global state (environment.py:512-522)."""
        if self._state_dyn is not None:
            return self._state_dyn.unsqueeze(1).expand(-1, self.num_jammers, -1)
        if self._state_vecs is not None:
            return self._state_vecs.unsqueeze(1).expand(-1, self.num_jammers, -1)
        return self._state_vec.view(1, 1, -1).expand(self.batch_envs, self.num_jammers, -1)

    def get_avail_actions(self) -> torch.Tensor:
        """int32 [E, J, A] expanded view of ones (environment.py:539-551)."""
        return self._avail.expand(self.batch_envs, self.num_jammers, -1)

    def get_env_info(self) -> Dict[str, int]:
        return self.scenario.env_info()

    @property
    def track(self) -> torch.Tensor:
        """uint8 [E, R] view, 1 = TRACK."""
        return self._track.t()

    @property
    def beam_azimuth(self) -> torch.Tensor:
        """f64 [E, R] view of the beam azimuths in degrees (scanning beams only)."""
        if self._theta_a is None:
            raise AttributeError("beam_azimuth: the scenario's beams do not scan (no environment_params.radar_scan)")
        return self._theta_a.t()

    @property
    def positions(self) -> torch.Tensor:
        """f32 [E, 2R + 2J]: the current position columns of the state rows in state order (per radar x, y; then per jammer
        x, y), gathered from them (moving scenarios only)."""
        if self._motion_io is None and self._motion_pe_io is None:
            raise AttributeError("positions: the scenario does not move (no environment_params.motion)")
        return self._state_dyn[:, self._pos_cols]

    def frame_states(self) -> torch.Tensor:
        """f32 [F + 1, S] on the device (moving scenarios only): row k is the state row every env shows at step counter k —
        the scenario's state vector with the position columns of frame k (``Scenario.frame_state_rows``), i.e. the bits
        the moving step writes.  Built once."""
        self._refuse_moving_scan_batch("frame_states")
        self._refuse_moving_batch("frame_states")   # every env has its own frames
        if self._motion_io is None:
            raise AttributeError("frame_states: the scenario does not move (no environment_params.motion)")
        if self._motion_scan_io is not None:   # the theta_a columns depend on the detections, not on the counter alone
            raise RuntimeError("frame_states: not available with scanning radars (environment_params.radar_scan): the state "
                               "rows of a moving scanning scenario depend on the detections")
        if getattr(self, "_frame_states", None) is None:
            self._frame_states = torch.from_numpy(self.scenario.frame_state_rows()).to(self.device)
        return self._frame_states

    @property
    def step_count(self) -> torch.Tensor:
        return self._step

    @property
    def episode_index(self) -> torch.Tensor:
        """int32 [E]: number of resets each env has seen (keys the in-kernel Monte-Carlo stream)."""
        return self._episode

    def reset(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """All (or the masked) envs back to SEARCH / step 0 (environment.py:208-219).  Returns the
        [E, S] state view."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        mptr = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mptr = mask.data_ptr()
        with torch.cuda.device(self.device):
            _native.check(self._lib.macjd_env_reset(self._handle.ptr, self.batch_envs, self._track.data_ptr(),
                                                    1, self.batch_envs, self._step.data_ptr(), mptr,
                                                    self._episode.data_ptr(), stream),
                          "macjd_env_reset")
            if self._motion_scan_pe_io is not None:   # beam part on each env's own frame 0 (the position part follows)
                mp = self._motion_pe_io
                _native.check(self._lib.macjd_env_reset_moving_scan_pe(
                    self._handle.ptr, self.batch_envs, ctypes.byref(self._scan_io), ctypes.byref(self._motion_scan_pe_io),
                    int(mp.n_frames), int(mp.tile), mptr, stream), "macjd_env_reset_moving_scan_pe")
            elif self._scan_pe_io is not None:
                _native.check(self._lib.macjd_env_reset_scan_pe(self._handle.ptr, self.batch_envs, ctypes.byref(self._scan_io),
                                                                ctypes.byref(self._scan_pe_io), self._pe_tile, mptr, stream),
                              "macjd_env_reset_scan_pe")
            elif self._scan_io is not None:
                _native.check(self._lib.macjd_env_reset_scan(self._handle.ptr, self.batch_envs, ctypes.byref(self._scan_io),
                                                             mptr, stream), "macjd_env_reset_scan")
            if self._motion_pe_io is not None:
                _native.check(self._lib.macjd_env_reset_moving_pe(self._handle.ptr, self.batch_envs,
                                                                  ctypes.byref(self._motion_pe_io), mptr, stream),
                              "macjd_env_reset_moving_pe")
            if self._motion_io is not None:   # (next to the beam reset when the scenario also scans)
                _native.check(self._lib.macjd_env_reset_moving(self._handle.ptr, self.batch_envs, ctypes.byref(self._motion_io),
                                                               mptr, stream), "macjd_env_reset_moving")
        self._keep_mask = mask
        return self.get_state()

    # ---- the hot call ----
    def _fill_io(self, T: torch.Tensor, P: torch.Tensor, u: Optional[torch.Tensor], arith_f64: bool,
                 reward: Optional[torch.Tensor], terminated: Optional[torch.Tensor], want_info: bool,
                 diag: Optional[Dict[str, torch.Tensor]], rdpj_sum: Optional[torch.Tensor] = None) -> _native.StepIO:
        E, R, J = self.batch_envs, self.num_radars, self.num_jammers
        if T.dim() == 3:
            T = T.squeeze(-1)
        if P.dim() == 3:
            P = P.squeeze(-1)
        if tuple(T.shape) != (E, J) or tuple(P.shape) != (E, J):
            raise ValueError(f"Received actions of shape {tuple(T.shape)} / {tuple(P.shape)}, but expected ({E}, {J})")
        if T.dtype != torch.int32:
            T = T.to(torch.int32)
        if P.dtype not in (torch.float32, torch.float64):
            P = P.to(torch.float32)
        if T.device != self.device or P.device != self.device:
            raise ValueError("actions must live on the environment's device")
        io = self._io
        io.n_envs, io.env_offset, io.seed = E, self.env_offset, self.seed
        io.flags = (_native.STEP_ARITH_F64 if arith_f64 else 0) | self.kernel_flags
        io.T, io.T_se, io.T_sx = T.data_ptr(), T.stride(0), T.stride(1)
        if P.dtype == torch.float32:
            io.P32, io.P64 = P.data_ptr(), None
        else:
            io.P32, io.P64 = None, P.data_ptr()
        io.P_se, io.P_sx = P.stride(0), P.stride(1)
        if u is not None:
            if tuple(u.shape) != (E, R + J) or u.dtype != torch.float64 or u.device != self.device:
                raise ValueError(f"uniforms must be float64 [{E}, {R + J}] on {self.device}")
            io.u, io.u_se, io.u_sx = u.data_ptr(), u.stride(0), u.stride(1)
        else:
            io.u, io.u_se, io.u_sx = None, 0, 0
        io.episode = self._episode.data_ptr()
        io.track, io.k_se, io.k_sx = self._track.data_ptr(), 1, E
        io.step = self._step.data_ptr()
        rew = self._reward if reward is None else reward
        ter = self._terminated if terminated is None else terminated
        for name, t, dt in (("reward", rew, torch.float32), ("terminated", ter, torch.uint8)):
            if t.dtype != dt and not (dt == torch.uint8 and t.dtype == torch.bool):
                raise ValueError(f"{name} output must be {dt}")
            if t.numel() != E or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} output must be a contiguous [{E}] tensor on {self.device}")
        io.reward, io.terminated = rew.data_ptr(), ter.data_ptr()
        io.r_dpj = self._r_dpj.data_ptr()
        if want_info:
            io.pd, io.pd_se, io.pd_sx = self._pd.data_ptr(), 1, E
            io.snr_with, io.sw_se, io.sw_sx = self._snr.data_ptr(), 1, E
        else:
            io.pd, io.pd_se, io.pd_sx = None, 0, 0
            io.snr_with, io.sw_se, io.sw_sx = None, 0, 0
        for k in ("out64", "pd64", "snr64", "prj64"):
            setattr(io, k, diag[k].data_ptr() if diag is not None else None)
        io.r_dpj_sum = rdpj_sum.data_ptr() if rdpj_sum is not None else None
        if self._pe_tables is not None:
            io.pe_tables, io.pe_flags, io.pe_stride = self._pe_tables.data_ptr(), self._pe_flags.data_ptr(), E
            io.pe_tile = self._pe_tile
        # keep converted tensors alive until the launch has been enqueued (same-stream ordering
        # keeps their storage valid for the kernel: the caching allocator is stream-ordered)
        self._keep = (T, P, u, rew, ter, diag)
        return io

    def step(self, actions_T: torch.Tensor, actions_P: torch.Tensor, uniforms: Optional[torch.Tensor] = None,
             *, arith_f64: bool = False, out_reward: Optional[torch.Tensor] = None,
             out_terminated: Optional[torch.Tensor] = None, want_info: bool = True,
             diag: Optional[Dict[str, torch.Tensor]] = None, rdpj_sum: Optional[torch.Tensor] = None
             ) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """One step of all E envs (batched environment.py:221-477).

        actions_T  int   [E, J] or [E, J, 1]  discrete action index T_i (int32 avoids a cast kernel)
        actions_P  f32/f64 [E, J] or [E, J, 1] normalised power P_i
        uniforms   f64 [E, R+J] or None (None -> Philox in-kernel, keyed by seed / env / step)

        Returns ``(reward f32[E], terminated bool[E], info)``; the tensors are views of buffers that
        the next ``step`` overwrites (pass ``out_reward`` / ``out_terminated`` to write elsewhere,
        e.g. straight into a replay row).  No host synchronisation happens here.
        """
        if rdpj_sum is not None and not (rdpj_sum.dtype == torch.float32 and rdpj_sum.is_contiguous()
                                         and tuple(rdpj_sum.shape) == (self.batch_envs, 3) and rdpj_sum.device == self.device):
            raise ValueError(f"rdpj_sum must be a contiguous float32 [{self.batch_envs}, 3] tensor on {self.device}")
        io = self._fill_io(actions_T, actions_P, uniforms, arith_f64, out_reward, out_terminated, want_info, diag,
                           rdpj_sum)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if self._motion_scan_pe_io is not None:
                si = self._scan_io
                si.snr_no = self._snr_no_step.data_ptr() if want_info else None
                _native.check(self._lib.macjd_env_step_moving_scan_pe(
                    self._handle.ptr, ctypes.byref(io), ctypes.byref(self._motion_pe_io), ctypes.byref(si),
                    ctypes.byref(self._motion_scan_pe_io), stream), "macjd_env_step_moving_scan_pe")
            elif self._motion_scan_io is not None:
                si = self._scan_io
                si.snr_no = self._snr_no_step.data_ptr() if want_info else None
                _native.check(self._lib.macjd_env_step_moving_scan(
                    self._handle.ptr, ctypes.byref(io), ctypes.byref(self._motion_io), ctypes.byref(si),
                    ctypes.byref(self._motion_scan_io), stream), "macjd_env_step_moving_scan")
            elif self._scan_pe_pattern_io is not None:
                _native.check(self._lib.macjd_env_step_scan_pe_pattern(
                    self._handle.ptr, ctypes.byref(io), ctypes.byref(self._scan_io), ctypes.byref(self._scan_pe_io),
                    ctypes.byref(self._scan_pe_pattern_io), stream), "macjd_env_step_scan_pe_pattern")
            elif self._scan_pe_io is not None:
                _native.check(self._lib.macjd_env_step_scan_pe(self._handle.ptr, ctypes.byref(io), ctypes.byref(self._scan_io),
                                                               ctypes.byref(self._scan_pe_io), stream), "macjd_env_step_scan_pe")
            elif self._scan_io is not None:
                _native.check(self._lib.macjd_env_step_scan(self._handle.ptr, ctypes.byref(io), ctypes.byref(self._scan_io),
                                                            stream), "macjd_env_step_scan")
            elif self._motion_pe_io is not None:
                mp = self._motion_pe_io
                mp.snr_no = self._snr_no_step.data_ptr() if want_info else None
                _native.check(self._lib.macjd_env_step_moving_pe(self._handle.ptr, ctypes.byref(io), ctypes.byref(mp), stream),
                              "macjd_env_step_moving_pe")
            elif self._motion_io is not None:
                mo = self._motion_io
                mo.snr_no = self._snr_no_step.data_ptr() if want_info else None
                _native.check(self._lib.macjd_env_step_moving(self._handle.ptr, ctypes.byref(io), ctypes.byref(mo), stream),
                              "macjd_env_step_moving")
            else:
                _native.check(self._lib.macjd_env_step(self._handle.ptr, ctypes.byref(io), stream), "macjd_env_step")
        rew = self._reward if out_reward is None else out_reward
        ter = self._terminated if out_terminated is None else out_terminated
        info = {"r_d": self._r_dpj[:, 0], "r_p": self._r_dpj[:, 1], "r_j": self._r_dpj[:, 2],
                "radar_tracking": self._track.t(), "step_count": self._step}
        if want_info:
            info["radar_pds"] = self._pd.t()
            info["snr_with_jamming"] = self._snr.t()
            info["snr_no_jamming"] = self._snr_no if self._snr_no_step is None else self._snr_no_step.t()
        return rew, (ter.view(torch.bool) if ter.dtype == torch.uint8 else ter), info

    def step_many(self, actions_T: torch.Tensor, actions_P: torch.Tensor, out_reward: torch.Tensor,
                  out_terminated: torch.Tensor, out_rdpj: torch.Tensor, rdpj_sum: Optional[torch.Tensor] = None) -> None:
        """All n steps of an episode batch in ONE launch (+ a tiny one that advances the counters), given the actions of
        all steps: ``actions_T`` int32 / ``actions_P`` float32 [n, E, J(,1)] contiguous (the runner's staging tensors);
        ``out_reward`` float32 [n, E(,1)], ``out_terminated`` bool / uint8 [n, E(,1)], ``out_rdpj`` float32 [n, E, 3] —
        all contiguous.  Legal because a step's outcome depends on the env's past only through the step counter (the
        FSM's next state equals `detected`, core/radar.py:102-117) — see include/macjd.h, macjd_env_step_many; meant for
        actions that do not depend on the env's outputs (static observation).  Philox uniforms, no pd / snr outputs."""
        self._refuse_moving_scan_batch("step_many")
        self._refuse_scanning("step_many")
        E, J = self.batch_envs, self.num_jammers
        n = actions_T.shape[0]
        for name, t, dt in (("actions_T", actions_T, torch.int32), ("actions_P", actions_P, torch.float32),
                            ("out_reward", out_reward, torch.float32), ("out_rdpj", out_rdpj, torch.float32)):
            if t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} must be a contiguous {dt} tensor on {self.device}")
        if actions_T.numel() != n * E * J or actions_P.numel() != n * E * J or out_reward.numel() != n * E \
                or out_terminated.numel() != n * E or out_rdpj.numel() != n * E * 3 or not out_terminated.is_contiguous():
            raise ValueError("step_many: tensor sizes do not match [n, E, J] / [n, E] / [n, E, 3]")
        if out_terminated.dtype not in (torch.uint8, torch.bool):
            raise ValueError("out_terminated must be uint8 or bool")
        io = self._fill_io(actions_T[0].view(E, J), actions_P[0].view(E, J), None, False, out_reward.view(-1)[:E],
                           out_terminated.view(-1)[:E], False, None, rdpj_sum)
        io.r_dpj = out_rdpj.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if self._motion_pe_io is not None:   # the same on each env's own frames
                mp = self._motion_pe_io
                mp.snr_no = None
                _native.check(self._lib.macjd_env_step_many_moving_pe(self._handle.ptr, ctypes.byref(io), ctypes.byref(mp), int(n),
                                                                      int(E * J), stream), "macjd_env_step_many_moving_pe")
            elif self._motion_io is not None:   # item (t, e) runs frame min(step[e] + t, F - 1); state rows end as after step n
                mo = self._motion_io
                mo.snr_no = None
                _native.check(self._lib.macjd_env_step_many_moving(self._handle.ptr, ctypes.byref(io), ctypes.byref(mo), int(n),
                                                                   int(E * J), stream), "macjd_env_step_many_moving")
            else:
                _native.check(self._lib.macjd_env_step_many(self._handle.ptr, ctypes.byref(io), int(n), int(E * J), stream),
                              "macjd_env_step_many")
        io.r_dpj = self._r_dpj.data_ptr()
        self._keep = (actions_T, actions_P, out_reward, out_terminated, out_rdpj)

    def time_step_many_kernel(self, actions_T, actions_P, out_reward, out_terminated, out_rdpj, iters: int) -> float:
        """bench.py helper: average milliseconds per launch of the many-step kernel (n x E work items), ``iters``
        launches replayed from a HIP graph and bracketed by HIP events on the replay stream (macjd_env_step_many_timed)."""
        self._refuse_moving_scan_batch("time_step_many_kernel")
        self._refuse_scanning("time_step_many_kernel")
        self._refuse_moving("time_step_many_kernel")
        self._refuse_moving_batch("time_step_many_kernel")
        E, J = self.batch_envs, self.num_jammers
        n = actions_T.shape[0]
        io = self._fill_io(actions_T[0].view(E, J), actions_P[0].view(E, J), None, False, out_reward.view(-1)[:E],
                           out_terminated.view(-1)[:E], False, None, None)
        io.r_dpj = out_rdpj.data_ptr()
        ms = ctypes.c_float(0.0)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            _native.check(self._lib.macjd_env_step_many_timed(self._handle.ptr, ctypes.byref(io), int(n), int(E * J), int(iters),
                                                              stream, ctypes.byref(ms)), "macjd_env_step_many_timed")
        io.r_dpj = self._r_dpj.data_ptr()
        return float(ms.value)

    def time_step_kernel(self, actions_T: torch.Tensor, actions_P: torch.Tensor, iters: int,
                         uniforms: Optional[torch.Tensor] = None, want_info: bool = True) -> float:
        """bench.py helper: average milliseconds per env_step launch over ``iters`` back-to-back
        launches, measured with HIP events recorded on the launch stream (macjd_env_step_timed)."""
        self._refuse_moving_scan_batch("time_step_kernel")
        self._refuse_scanning("time_step_kernel")
        self._refuse_moving("time_step_kernel")
        self._refuse_moving_batch("time_step_kernel")
        io = self._fill_io(actions_T, actions_P, uniforms, False, None, None, want_info, None)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ms = ctypes.c_float(0.0)
        with torch.cuda.device(self.device):
            _native.check(self._lib.macjd_env_step_timed(self._handle.ptr, ctypes.byref(io), int(iters), stream,
                                                         ctypes.byref(ms)), "macjd_env_step_timed")
        return float(ms.value)

    def episode_scan_args(self) -> Dict[str, Any]:
        """What the closed-loop episode launch (``ops.agent_env_episode_scan``) needs from a scanning environment: the
        scenario handle, the beam / state-row block, the FSM bits, step counters and episode indices it reads and leaves
        as T single steps would, and the Monte-Carlo stream's seed and env offset."""
        self._refuse_moving_scan_batch("episode_scan_args")
        self._refuse_moving_batch("episode_scan_args")
        if self._scan_io is None:
            raise RuntimeError("episode_scan_args: the scenario's beams do not scan (no environment_params.radar_scan)")
        if self._pe_tables is not None:
            raise RuntimeError("episode_scan_args: per-env scenario tables are not supported with scanning radars")
        if self._motion_io is not None:
            raise RuntimeError("episode_scan_args: not available with a moving scenario (environment_params.motion): the "
                               "closed-loop launch reads the handle's frame-0 tables")
        return {"handle": self._handle.ptr, "scan_io": self._scan_io, "track": self._track, "step": self._step,
                "episode": self._episode, "seed": self.seed, "env_offset": self.env_offset, "n_radars": self.num_radars,
                "pe_tables": None}

    def episode_scan_pe_args(self) -> Dict[str, Any]:
        """What the closed-loop episode launch on per-env tables (``ops.agent_env_episode_scan_pe``) needs from a per-env
        scanning scenario batch: the entries of ``episode_scan_args`` plus the batch's scenario tables and flag bytes
        with their tile width, ``n_envs`` (the plain layout's row stride), the per-env scan block and, under a stepped
        pattern, the per-env level tables (else None)."""
        self._refuse_moving_scan_batch("episode_scan_pe_args")
        self._refuse_moving_batch("episode_scan_pe_args")
        if self._scan_pe_io is None:
            raise RuntimeError("episode_scan_pe_args: needs a per-env scanning scenario batch (ScenarioBatch(..., scan=True)); "
                               "episode_scan_args serves shared scenario tables")
        return {"handle": self._handle.ptr, "scan_io": self._scan_io, "track": self._track, "step": self._step,
                "episode": self._episode, "seed": self.seed, "env_offset": self.env_offset, "n_radars": self.num_radars,
                "pe_tables": self._pe_tables.data_ptr(), "pe_flags": self._pe_flags.data_ptr(), "pe_tile": self._pe_tile,
                "n_envs": self.batch_envs, "scan_pe_io": self._scan_pe_io, "scan_pe_pattern_io": self._scan_pe_pattern_io}

    def episode_moving_scan_args(self) -> Dict[str, Any]:
        """What the closed-loop episode launch on a moving scanning scenario (``ops.agent_env_episode_moving_scan``) needs:
        the entries of ``episode_scan_args`` plus the motion block (frame tables, positions and their state columns) and the
        motion-scan block (per-frame beam tables, under a stepped pattern the per-frame level tables)."""
        self._refuse_moving_scan_batch("episode_moving_scan_args")
        self._refuse_moving_batch("episode_moving_scan_args")
        if self._motion_io is None or self._motion_scan_io is None:
            raise RuntimeError("episode_moving_scan_args: needs a scenario that both moves and scans (environment_params.motion "
                               "and environment_params.radar_scan); episode_scan_args serves a static scanning scenario")
        self._scan_io.snr_no = self._snr_no_step.data_ptr()   # (a step with want_info=False clears it)
        return {"handle": self._handle.ptr, "scan_io": self._scan_io, "motion_io": self._motion_io,
                "motion_scan_io": self._motion_scan_io, "track": self._track, "step": self._step, "episode": self._episode,
                "seed": self.seed, "env_offset": self.env_offset, "n_radars": self.num_radars, "pe_tables": None}

    def episode_moving_scan_pe_args(self) -> Dict[str, Any]:
        """What the closed-loop episode launch on a per-env moving scanning scenario batch
        (``ops.agent_env_episode_moving_scan_pe``) needs: the entries of ``episode_scan_args`` plus the per-env motion block
        (tiled frame tables, positions and their state columns, tile width) and the per-env motion-scan block (tiled beam
        frames, under a stepped pattern the tiled level frames)."""
        if self._motion_scan_pe_io is None:
            raise RuntimeError("episode_moving_scan_pe_args: needs a per-env moving scanning scenario batch "
                               "(moving_scan_batch=...); episode_moving_scan_args serves shared frame tables")
        self._scan_io.snr_no = self._snr_no_step.data_ptr()   # (a step with want_info=False clears it)
        return {"handle": self._handle.ptr, "scan_io": self._scan_io, "motion_pe_io": self._motion_pe_io,
                "motion_scan_pe_io": self._motion_scan_pe_io, "track": self._track, "step": self._step,
                "episode": self._episode, "seed": self.seed, "env_offset": self.env_offset, "n_radars": self.num_radars,
                "pe_tables": None}

    def _need_moving_batch(self, what: str) -> None:
        if self._motion_pe_io is None:
            raise RuntimeError(f"{what}: needs a per-env moving scenario batch (moving_batch=...)")

    def episode_moving_pe_args(self) -> Dict[str, Any]:
        """What the agent's episode launch on per-env moving frames (``ops.agent_episode_moving_pe``) needs from a per-env
        moving scenario batch: every env's own state row (the position columns are ignored), the step counters, the tiled
        positions table f32 [n_tiles, F + 1, n_pos, tile] with its state columns, F, n_pos and the tile width."""
        self._refuse_moving_scan_batch("episode_moving_pe_args")
        self._need_moving_batch("episode_moving_pe_args")
        keep, mp = self._motion_keep, self._motion_pe_io
        return {"state": self._state_dyn, "step": self._step, "positions": keep["positions"],
                "position_columns": keep["position_columns"], "n_frames": int(mp.n_frames), "n_pos": int(mp.n_pos),
                "tile": int(mp.tile), "n_radars": self.num_radars}

    def frame_positions(self) -> torch.Tensor:
        """f32 [E, F + 1, n_pos] on the device (per-env moving batches only): env e's position columns at step counter k in
        state order, untiled from the positions table — the bits the per-env moving step writes.  Built once."""
        self._refuse_moving_scan_batch("frame_positions")
        self._need_moving_batch("frame_positions")
        if getattr(self, "_frame_positions", None) is None:
            pos = self._motion_keep["positions"]                    # [n_tiles, F + 1, n_pos, tile]
            n_tiles, F1, n_pos, w = pos.shape
            self._frame_positions = pos.permute(0, 3, 1, 2).reshape(n_tiles * w, F1, n_pos)[:self.batch_envs].contiguous()
        return self._frame_positions

    MANY_STEP_MOVING_SIZES = ((2, 2), (3, 4), (6, 8))   # (J, R) of csrc/macjd_env_motion.hip, motion_size_compiled

    def step_many_has_production_form(self) -> bool:
        """A moving env's ``step_many`` exists in the production form only (the lane kernel at a compiled size; any other
        size is refused by the launch): True when this env moves — on shared frames or as a per-env moving batch, whose
        many-step launch is compiled at the same sizes — and its size is one of them."""
        return ((self._motion_io is not None or self._motion_pe_io is not None) and self._motion_scan_io is None
                and self._motion_scan_pe_io is None
                and (self.num_jammers, self.num_radars) in self.MANY_STEP_MOVING_SIZES)

    def _refuse_scanning(self, what: str) -> None:
        # macjd_env_step_many rests on "a step's outcome depends on the past only through the step counter" (include/
        # macjd.h), which the beam azimuth breaks; the timing helper runs the non-scanning launch
        if self._scan_io is not None:
            raise RuntimeError(f"{what}: not available with scanning radars (environment_params.radar_scan)")

    def _refuse_moving(self, what: str) -> None:
        # the timing helpers run the static launch on the handle's (frame-0) tables: not what a moving env steps with
        if self._motion_io is not None:
            raise RuntimeError(f"{what}: not available with a moving scenario (environment_params.motion)")

    @property
    def scenario_regular(self) -> bool:
        """The shared scenario's tables are regular (include/macjd.h, macjd_scenario_is_regular): the production lane
        kernel runs its short-division form.  Per-env scenario batches have no shared handle: False."""
        h = getattr(self, "_handle", None)
        return bool(h is not None and self._lib.macjd_scenario_is_regular(h.ptr) == 1)

    def close(self) -> None:
        self._handle.close()


class ElectromagneticEnvironment:
    """Single-environment drop-in for the reference class (simulation/environment.py:29-573)."""

    def __init__(self, config, sim_config_path: str = DEFAULT_SIM_CONFIG_PATH):
        self._batched = BatchedElectromagneticEnvironment(config, sim_config_path, batch_envs=1,
                                                          device=getattr(config, "env_device", None))
        sc = self.scenario = self._batched.scenario
        self.sim_config_path = sim_config_path
        self.num_jammers, self.num_radars = sc.num_jammers, sc.num_radars
        self.episode_limit = sc.episode_limit
        self.max_radar_types = sc.max_radar_types
        self.rd_min_penalty, self.rd_max_penalty = sc.rd_min, sc.rd_max
        self.rp_min_penalty, self.rp_max_penalty = sc.rp_min, sc.rp_max
        self.action_dim_discrete = sc.n_actions
        self.action_dim_continuous = 1
        self.state_dim = self.obs_dim = self.agent_obs_dim = sc.state_dim
        self.protected_target_config = {"position": sc.target_position, "rcs": sc.target_rcs}
        self._step_count = 0
        self._last_actions = np.zeros((self.num_jammers, 2))
        dynamic = sc.scanning or sc.moving
        self._state = sc.state_vector() if not dynamic else self._batched.get_state()[0].cpu().numpy().copy()
        dev = self._batched.device
        R, J = self.num_radars, self.num_jammers
        self._diag = {"out64": torch.zeros((1, 4), dtype=torch.float64, device=dev),
                      "pd64": torch.zeros((1, R), dtype=torch.float64, device=dev),
                      "snr64": torch.zeros((1, R), dtype=torch.float64, device=dev),
                      "prj64": torch.zeros((1, J), dtype=torch.float64, device=dev)}
        # same one-time summary the reference prints (environment.py:115-121)
        rfd = sc.radar_feature_dim
        print(f"Environment Initialized: {J} Jammers, {R} Radars (from {sim_config_path})")
        print(f"State Dimension: {self.state_dim} (Radar features: {rfd}, Jammer features: 2, "
              f"Max Radar Types: {self.max_radar_types})")
        print(f"Observation Dimension (per agent): {self.agent_obs_dim}")
        print(f"Action Dimension (Discrete): {self.action_dim_discrete}")
        print(f"Protected Target: Pos={sc.target_position}, RCS={sc.target_rcs}")
        print(f"Episode Limit: {self.episode_limit}")
        print(f"Reward Params: rd=[{sc.rd_min}, {sc.rd_max}], rp=[{sc.rp_min}, {sc.rp_max}]")

    def reset(self) -> np.ndarray:
        self._batched.reset()
        if self._batched._scan_io is not None or self._batched._motion_io is not None:
            self._state = self._batched.get_state()[0].cpu().numpy().copy()
        self._step_count = 0
        self._last_actions.fill(0)
        return self.get_state()

    def _host_actions(self, actions: Sequence[Tuple[Any, Any]]):
        """Decode on the host only what decides HOW MANY uniforms the reference would draw, using the
        same NumPy expressions on the caller's own scalar types (environment.py:249-284)."""
        sc = self.scenario
        R, J = self.num_radars, self.num_jammers
        T = np.zeros(J, dtype=np.int32)
        all_f32 = all(isinstance(a[1], np.float32) for a in actions)
        P = np.zeros(J, dtype=np.float32 if all_f32 else np.float64)
        powers: List[Any] = []
        n_dec = 0
        denom = sc.tables["jr_denom"].reshape(J, R)
        if sc.moving:   # the frame this step runs on (self._step_count is already advanced: the counter before is one less)
            mt = sc.motion_tables
            f = min(self._step_count - 1, mt["frames"].shape[0] - 1)
            denom = mt["frames"][f, 6 * R + 3 * J:].reshape(J, R)
        for i, (t_i, p_i) in enumerate(actions):
            t_i = int(t_i)
            p_c = np.clip(p_i, 0.0, 1.0)
            pmin, pmax = sc.jammers[i]["power_min"], sc.jammers[i]["power_max"]
            actual = pmin + p_c * (pmax - pmin)
            powers.append(actual)
            T[i] = max(min(t_i, 2 ** 31 - 1), -(2 ** 31))
            P[i] = p_i
            if 1 <= t_i <= 2 * R:
                tgt = (t_i + 1) // 2 - 1
                if actual > 0 and denom[i, tgt] >= 0.0 and t_i % 2 == 0:
                    n_dec += 1
            elif t_i > 0:
                print(f"Warning: Jammer {i} chose invalid discrete action T_i={t_i}")  # environment.py:268
        return T, P, all_f32, powers, n_dec

    def step(self, actions):
        if len(actions) != self.num_jammers:  # environment.py:232-233
            raise ValueError(f"Received {len(actions)} actions, but expected {self.num_jammers}")
        self._step_count += 1
        sc, b = self.scenario, self._batched
        R, J = self.num_radars, self.num_jammers
        T, P, all_f32, powers, n_dec = self._host_actions(actions)
        u = np.full(R + J, 2.0)  # slots the reference would not draw can never compare as hits
        for k in range(R + n_dec):  # same consumption of the global stream as environment.py:341,430
            u[k] = np.random.rand()
        dev = b.device
        T_d = torch.from_numpy(T).to(dev).view(1, J)
        P_d = torch.from_numpy(P).to(dev).view(1, J)
        u_d = torch.from_numpy(u).to(dev).view(1, R + J)
        _, term, _ = b.step(T_d, P_d, u_d, diag=self._diag)
        out = self._diag["out64"].cpu().numpy()[0]
        pd = self._diag["pd64"].cpu().numpy()[0].copy()
        snr = self._diag["snr64"].cpu().numpy()[0].copy()
        prj = self._diag["prj64"].cpu().numpy()[0]
        tracking = b.track.cpu().numpy()[0].astype(bool)
        terminated = bool(self._step_count >= self.episode_limit)
        self._last_actions = np.array([[T[i], np.clip(actions[i][1], 0.0, 1.0)] for i in range(J)], dtype=np.float64)

        jammer_actions = []
        for i in range(J):
            if prj[i] >= 0.0:  # recorded in the reference's jammer_actions_details (environment.py:288-295)
                jammer_actions.append({"jammer_idx": i, "target_idx": (int(T[i]) + 1) // 2 - 1, "type": int(T[i]) % 2,
                                       "power": powers[i], "received_power": np.float64(prj[i])})
        radar_states = []
        for r in range(R):
            radar_states.append({  # core/radar.py:121-130
                "state": RADAR_STATE_TRACK if tracking[r] else RADAR_STATE_SEARCH,
                "threat": sc.radars[r]["threat_level"],
                "is_tracking": bool(tracking[r]),
                "locked_target": self.protected_target_config if tracking[r] else None,
            })
        if b._scan_io is not None:
            # the kernel reports which lobe's no-jamming SNR applied (float32); hand out that table's float64 value
            snr32 = b._snr_no_step.t().cpu().numpy()[0]
            main, side = sc.tables["radar_snr_no"], sc.scan_tables["snr_no_side"]
            levels = sc.scan_tables["pat_snr_no"] if sc.scan_pattern_levels else None
            if b._motion_scan_io is not None:   # a moving scenario: the tables of the frame this step ran on
                mt, L = sc.motion_tables, sc.scan_pattern_levels
                f = min(self._step_count - 1, mt["scan_frames"].shape[0] - 1)
                main, side = mt["scan_frames"][f, 6 * R:7 * R], mt["scan_frames"][f, 7 * R:8 * R]
                if L:   # snr_no_lvl block of the pattern row: [L + 2, R] behind inv_width and GaPs_lvl
                    levels = mt["pattern_frames"][f, R + (L + 2) * R:R + 2 * (L + 2) * R].reshape(L + 2, R)[1:L + 1]
            snr_no = np.where(main.astype(np.float32) == snr32, main, side).astype(np.float64)
            if sc.scan_pattern_levels:
                # stepped pattern: the matching level's value (equal gains give equal values: any of them will do)
                for lvl in levels[::-1]:
                    snr_no = np.where((lvl.astype(np.float32) == snr32) & (main.astype(np.float32) != snr32), lvl, snr_no)
            self._state = b.get_state()[0].cpu().numpy().copy()
        elif b._motion_io is not None:
            mt = sc.motion_tables
            snr_no = mt["snr_no"][min(self._step_count - 1, mt["snr_no"].shape[0] - 1)].copy()
            self._state = b.get_state()[0].cpu().numpy().copy()
        else:
            snr_no = sc.tables["radar_snr_no"].copy()
        info = {
            "radar_pds": pd,
            "radar_states": radar_states,
            "snr_no_jamming": snr_no,
            "snr_with_jamming": snr,
            "r_d": out[1], "r_p": out[2], "r_j": out[3],
            "jammer_actions": jammer_actions,
        }
        if b._scan_io is not None:
            info["radar_beam_azimuth"] = b.beam_azimuth.cpu().numpy()[0].copy()
        return self.get_obs(), np.float64(out[0]), terminated, info

    def get_state(self) -> np.ndarray:
        return self._state.copy()

    def get_obs(self) -> List[np.ndarray]:
        s = self.get_state()
        return [s for _ in range(self.num_jammers)]

    def get_agent_obs(self, agent_id: int) -> np.ndarray:
        if not (0 <= agent_id < self.num_jammers):  # environment.py:535-536
            raise ValueError(f"Invalid agent_id {agent_id} for {self.num_jammers} jammers.")
        return self.get_state()

    def get_avail_actions(self) -> List[np.ndarray]:
        return [np.ones(self.action_dim_discrete, dtype=np.int32) for _ in range(self.num_jammers)]

    def get_env_info(self) -> Dict[str, int]:
        return self.scenario.env_info()

    def close(self) -> None:
        print("Closing Electromagnetic Environment.")
        self._batched.close()
