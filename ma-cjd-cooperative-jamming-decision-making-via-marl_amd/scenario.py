"""Scenario compiler: sim-config YAML -> static float64 tables for the HIP env-step kernel.

The reference rebuilds Radar/Jammer objects on every reset and recomputes echo power, distances and
the no-jamming SNR on every step (reference simulation/environment.py:123-206, 316-333;
core/radar.py:10-60; core/jammer.py:24-54; utils/math_utils.py:3-8,40-42).  Nothing in step() moves
an entity (environment.py:237-238 is a TODO), so all of it is a pure function of the YAML.  This
module evaluates those quantities ONCE, on the host, with the same Python/NumPy expression forms the
reference uses (so the table entries are bit-identical to what the reference computes per step) and
hands them to the native library as a ``macjd_scenario_desc`` (include/macjd.h).

Opt-in, ``environment_params.motion`` moves target, radars and jammers on straight lines that do not depend on the
actions: the same compiler then runs once per step of an episode on the moved positions (``motion_frame_dict``) and the
tables become per-step frames (``Scenario.motion_tables``; include/macjd.h, ``macjd_motion_io``).  Together with
``radar_scan`` on one clock (equal ``step_seconds``) the beams' scan and pattern tables become frames as well
(``motion_tables["scan_frames"]`` / ``["pattern_frames"]``; ``macjd_motion_scan_io``).
``MovingScenarioBatch`` is the per-env batch of moving scenarios (``macjd_motion_pe_io``): every env's own frame tables,
stacked from host compiles or written by the device frame compiler from one input column per env
(``Scenario.motion_compile_inputs``; ``macjd_motion_pe_compile``).  ``MovingScanScenarioBatch`` is the same for scenarios
that both move and scan (``macjd_motion_scan_pe_io``): the beam frames per env too, from the host or from a second device
compiler (``macjd_motion_scan_pe_compile``).

Validation and error behaviour follow environment.py:44-79 and :133-199 (same exception types and
messages for the cases the reference checks).
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import yaml

DEFAULT_SIM_CONFIG_PATH = "config/simulation_config.yaml"  # environment.py:11

MAX_RADARS = 32   # MACJD_MAX_RADARS
MAX_JAMMERS = 32  # MACJD_MAX_JAMMERS
MAX_PATTERN_LEVELS = 6  # MACJD_MAX_PATTERN_LEVELS

_REQUIRED_RADAR_PARAMS = [  # environment.py:136-140
    "pt", "gt", "gr", "wavelength", "rcs", "loss", "latm", "pn",
    "type_id", "position", "theta_m", "theta_a", "t_s",
    "pulse_compression_gain", "anti_jamming_factor",
]
_REQUIRED_JAMMER_PARAMS = ["gj", "loss", "latm", "bj", "position"]  # environment.py:179
_JAMMER_INIT_KEYS = {"power", "gj", "loss", "latm", "bj", "position"}  # jammer.py:24


def db_to_linear(db_value):
    """dB -> linear power ratio (utils/math_utils.py:3-8)."""
    return 10 ** (db_value / 10.0)


def detection_probability_constants(prfa=1e-6, m=10):
    """The three constants of Radar.detection_probability (core/radar.py:67-77), evaluated with the
    reference's own expression forms: A = ln(0.62/prfa); c1 = 5 log10(m) / (6.2 + 4.54/sqrt(m) + 0.44);
    denB = 1.7 + 0.12 A."""
    safe_prfa = max(prfa, 1e-18)
    A = np.log(0.62 / safe_prfa)
    safe_m = max(m, 1)
    log10_m = np.log10(safe_m) if safe_m > 0 else 0
    c1 = (5 * log10_m) / (6.2 + 4.54 / np.sqrt(safe_m) + 0.44)
    den_b = 1.7 + 0.12 * A
    return float(A), float(c1), float(den_b)


def detection_probability(snr, consts=None):
    """Host evaluation of core/radar.py:67-82 (used only for the static no-jamming Pd table)."""
    A, c1, den_b = consts if consts is not None else detection_probability_constants()
    snr_linear = max(snr, 0.0)
    Z = snr_linear + c1
    if abs(den_b) < 1e-9:
        return 0.0
    B = (10 * Z - A) / den_b
    if B > 700:
        return 1.0
    if B < -700:
        return 0.0
    return 1 / (1 + np.exp(-B))


def wrap_degrees(x):
    """x - 360 floor(x / 360) in float64: an angle in [0, 360) (include/macjd.h, macjd_scan_desc)."""
    x = np.float64(x)
    return np.float64(x - 360.0 * np.floor(x / 360.0))


def bearing_degrees(frm, to):
    """wrap(degrees(atan2(to_y - from_y, to_x - from_x))) in float64."""
    f = np.asarray(frm, dtype=np.float64).reshape(-1)
    t = np.asarray(to, dtype=np.float64).reshape(-1)
    return wrap_degrees(np.degrees(np.arctan2(t[1] - f[1], t[0] - f[0])))


def parse_radar_scan(env_params: dict, source: str = "<dict>") -> Optional[Dict[str, float]]:
    """``environment_params.radar_scan`` -> {'step_seconds', 'sidelobe_db'} or None (absent / null: static beams); with the
    optional stepped antenna pattern also 'pattern': {'level_width': float, 'gain_db': [float] * L}."""
    rs = env_params.get("radar_scan")
    if rs is None:
        return None
    if not isinstance(rs, dict):
        raise ValueError(f"{source}: environment_params.radar_scan must be a mapping or null")
    unknown = set(rs) - {"step_seconds", "sidelobe_db", "pattern"}
    if unknown:
        raise ValueError(f"{source}: unknown radar_scan key(s) {sorted(unknown)}")
    out = {}
    for key in ("step_seconds", "sidelobe_db"):
        if key not in rs:
            raise ValueError(f"{source}: radar_scan is missing '{key}'")
        v = rs[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError(f"{source}: radar_scan.{key} must be a finite number, got {v!r}")
        out[key] = float(v)
    if not out["step_seconds"] > 0.0:
        raise ValueError(f"{source}: radar_scan.step_seconds must be > 0, got {out['step_seconds']}")
    if not out["sidelobe_db"] <= 0.0:
        raise ValueError(f"{source}: radar_scan.sidelobe_db must be <= 0, got {out['sidelobe_db']}")
    if "pattern" in rs:
        out["pattern"] = _parse_scan_pattern(rs["pattern"], source)
    return out


def _parse_scan_pattern(pat, source: str) -> Dict[str, Any]:
    """``radar_scan.pattern`` (include/macjd.h, macjd_scan_pattern_desc): exactly ``level_width`` (finite, > 0, in half beam
    widths) and ``gain_db`` (1..MAX_PATTERN_LEVELS finite one-way gains <= 0)."""
    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float)) and bool(np.isfinite(v))
    if not isinstance(pat, dict):
        raise ValueError(f"{source}: radar_scan.pattern must be a mapping")
    if set(pat) != {"level_width", "gain_db"}:
        raise ValueError(f"{source}: radar_scan.pattern must have exactly the keys 'level_width' and 'gain_db', "
                         f"got {sorted(map(str, pat))}")
    lw, gains = pat["level_width"], pat["gain_db"]
    if not number(lw) or not lw > 0.0:
        raise ValueError(f"{source}: radar_scan.pattern.level_width must be a finite number > 0, got {lw!r}")
    if not isinstance(gains, (list, tuple)) or not 1 <= len(gains) <= MAX_PATTERN_LEVELS:
        raise ValueError(f"{source}: radar_scan.pattern.gain_db must be a list of 1..{MAX_PATTERN_LEVELS} numbers, got {gains!r}")
    for g in gains:
        if not number(g) or not g <= 0.0:
            raise ValueError(f"{source}: radar_scan.pattern.gain_db entries must be finite numbers <= 0, got {g!r}")
    return {"level_width": float(lw), "gain_db": [float(g) for g in gains]}


_MOTION_KEYS = ("step_seconds", "target_velocity", "radar_velocity", "jammer_velocity")


def parse_motion(env_params: dict, num_radars: Optional[int] = None, num_jammers: Optional[int] = None,
                 source: str = "<dict>") -> Optional[Dict[str, Any]]:
    """``environment_params.motion`` -> {'step_seconds', 'target_velocity': [vx, vy], 'radar_velocity': [[vx, vy]] * R,
    'jammer_velocity': [[vx, vy]] * J} or None (absent / null: nothing moves).  Velocities are metres per second; a missing
    list means zeros.  With ``num_radars`` / ``num_jammers`` (the entities the scenario uses) the lists must have exactly
    that many pairs; without them (None) the lengths are taken as given."""
    mo = env_params.get("motion")
    if mo is None:
        return None
    if not isinstance(mo, dict):
        raise ValueError(f"{source}: environment_params.motion must be a mapping or null")
    unknown = set(mo) - set(_MOTION_KEYS)
    if unknown:
        raise ValueError(f"{source}: unknown motion key(s) {sorted(map(str, unknown))}")

    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float)) and bool(np.isfinite(v))

    def pair(v, what):
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(number(x) for x in v):
            raise ValueError(f"{source}: motion.{what} must be a pair of finite numbers [vx, vy], got {v!r}")
        return [float(v[0]), float(v[1])]

    if "step_seconds" not in mo:
        raise ValueError(f"{source}: motion is missing 'step_seconds'")
    dt = mo["step_seconds"]
    if not number(dt) or not dt > 0.0:
        raise ValueError(f"{source}: motion.step_seconds must be a finite number > 0, got {dt!r}")
    out: Dict[str, Any] = {"step_seconds": float(dt), "target_velocity": pair(mo.get("target_velocity", [0, 0]), "target_velocity")}
    for key, n in (("radar_velocity", num_radars), ("jammer_velocity", num_jammers)):
        v = mo.get(key)
        if v is None:
            out[key] = None if n is None else [[0.0, 0.0] for _ in range(n)]
            continue
        if not isinstance(v, (list, tuple)) or (n is not None and len(v) != n):
            raise ValueError(f"{source}: motion.{key} must be a list of {'' if n is None else str(n) + ' '}[vx, vy] pairs "
                             f"(one per {key.split('_')[0]} used), got {v!r}")
        out[key] = [pair(x, f"{key}[{i}]") for i, x in enumerate(v)]
    return out


def motion_frame_dict(sim_config: dict, k: int) -> dict:
    """Frame ``k`` of a moving scenario as an ordinary (static) sim-config dict: a deep copy of ``sim_config`` in which
    every position is, per axis a and in Python floats, ``float(p0[a]) + float(k) * (float(v[a]) * dt)``, and from which
    ``environment_params.motion`` is removed.  THE definition of a frame: the compiler (``Scenario.motion_tables``), the
    tests and the fixture generator all go through it.  A config without ``motion`` comes back as a plain deep copy."""
    import copy
    d = copy.deepcopy(sim_config)
    env_params = d.get("environment_params") or {}
    mo = parse_motion(env_params)
    if mo is None:
        return d
    del env_params["motion"]
    dt = mo["step_seconds"]

    def moved(p0, v):
        p0 = np.array(p0).flatten()
        return [float(p0[a]) + float(k) * (float(v[a]) * dt) for a in range(2)]

    d["protected_target"]["position"] = moved(d["protected_target"]["position"], mo["target_velocity"])
    for key, ents in (("radar_velocity", d.get("radars") or []), ("jammer_velocity", d.get("jammers") or [])):
        vel = mo[key]
        if vel is None:
            vel = [[0.0, 0.0]] * len(ents)
        if len(vel) > len(ents):
            raise ValueError(f"motion.{key} has {len(vel)} pairs, but the scenario defines only {len(ents)} entities")
        for ent, v in zip(ents, vel):
            ent["position"] = moved(ent["position"], v)
    return d


class _Desc(ctypes.Structure):
    """ctypes mirror of ``macjd_scenario_desc`` (include/macjd.h)."""
    _fields_ = [
        ("n_radars", ctypes.c_int32), ("n_jammers", ctypes.c_int32),
        ("episode_limit", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("rp_min", ctypes.c_double), ("rp_max", ctypes.c_double),
        ("pd_A", ctypes.c_double), ("pd_c1", ctypes.c_double), ("pd_denB", ctypes.c_double),
        ("radar_GaPs", ctypes.c_void_p), ("radar_Pn", ctypes.c_void_p), ("radar_D", ctypes.c_void_p),
        ("radar_pd_no", ctypes.c_void_p), ("radar_snr_no", ctypes.c_void_p),
        ("radar_rd_pen", ctypes.c_void_p), ("radar_gr", ctypes.c_void_p),
        ("jam_pmin", ctypes.c_void_p), ("jam_pmax", ctypes.c_void_p), ("jam_gj", ctypes.c_void_p),
        ("jr_denom", ctypes.c_void_p), ("jr_flags", ctypes.c_void_p),
    ]


@dataclass
class Scenario:
    """Validated scenario + its static tables.  Build with :meth:`from_yaml` / :meth:`from_dict`."""
    num_radars: int
    num_jammers: int
    episode_limit: int
    max_radar_types: int
    rd_min: float
    rd_max: float
    rp_min: float
    rp_max: float
    radars: List[Dict[str, Any]]
    jammers: List[Dict[str, Any]]
    target_position: np.ndarray
    target_rcs: float
    tables: Dict[str, np.ndarray] = field(default_factory=dict)
    pd_consts: tuple = (0.0, 0.0, 0.0)
    source: str = "<dict>"
    radar_scan: Optional[Dict[str, Any]] = None     # environment_params.radar_scan; None = static beams
    scan_tables: Dict[str, np.ndarray] = field(default_factory=dict)
    motion: Optional[Dict[str, Any]] = None         # environment_params.motion; None = nothing moves
    motion_tables: Dict[str, np.ndarray] = field(default_factory=dict)

    @property
    def moving(self) -> bool:
        """Entities move (environment_params.motion given): the tables are per-step frames, the observation is dynamic."""
        return self.motion is not None

    @property
    def position_columns(self) -> List[int]:
        """Columns of the position entries in the state vector, in state order: per radar (x, y), then per jammer (x, y)."""
        rfd, R = self.radar_feature_dim, self.num_radars
        cols = [r * rfd + rfd - 2 + a for r in range(R) for a in range(2)]
        return cols + [R * rfd + 2 * j + a for j in range(self.num_jammers) for a in range(2)]

    @property
    def scanning(self) -> bool:
        """The beams scan (environment_params.radar_scan given): theta_a changes every step, the observation is dynamic."""
        return self.radar_scan is not None

    @property
    def theta_a_col0(self) -> int:
        """Column of radar 0's theta_a in the state vector (see :meth:`state_vector`)."""
        return 3 + self.max_radar_types

    @property
    def theta_a_col_step(self) -> int:
        return self.radar_feature_dim

    @property
    def theta_a_columns(self) -> List[int]:
        return [self.theta_a_col0 + r * self.theta_a_col_step for r in range(self.num_radars)]

    # ---- derived dims (environment.py:91-101) ----
    @property
    def n_actions(self) -> int:
        return 2 * self.num_radars + 1

    @property
    def radar_feature_dim(self) -> int:
        return 1 + 1 + 1 + self.max_radar_types + 1 + 2

    @property
    def state_dim(self) -> int:
        return self.num_radars * self.radar_feature_dim + self.num_jammers * 2

    # ---- construction ----
    @classmethod
    def from_yaml(cls, sim_config_path: str = DEFAULT_SIM_CONFIG_PATH, config: Any = None) -> "Scenario":
        try:  # environment.py:45-55
            with open(sim_config_path, "r") as f:
                sim_config = yaml.safe_load(f)
        except FileNotFoundError:
            print(f"Error: Simulation configuration file not found at {sim_config_path}")
            raise
        except yaml.YAMLError as e:
            print(f"Error parsing simulation configuration file {sim_config_path}: {e}")
            raise
        return cls.from_dict(sim_config, config=config, source=sim_config_path)

    @classmethod
    def from_dict(cls, sim_config: Optional[dict], config: Any = None, source: str = "<dict>") -> "Scenario":
        if not sim_config or "radars" not in sim_config or "jammers" not in sim_config:  # :48-49
            raise ValueError(f"Simulation config file {source} is missing required 'radars' or 'jammers' keys.")
        if "protected_target" not in sim_config:  # :58-59
            raise ValueError(f"Simulation config file {source} is missing required 'protected_target' key.")
        target = sim_config["protected_target"]
        if "position" not in target or "rcs" not in target:  # :61-62
            raise ValueError("Protected target config must contain 'position' and 'rcs'.")
        target_position = np.array(target["position"])  # :64
        target_rcs = target["rcs"]

        env_params = sim_config.get("environment_params", {}) or {}  # :67-73
        max_radar_types = env_params.get("max_radar_types", 4)
        reward_params = env_params.get("rewards", {}) or {}
        radar_scan = parse_radar_scan(env_params, source)
        rd_min = reward_params.get("rd_min", -1.2)
        rd_max = reward_params.get("rd_max", -0.8)
        rp_min = reward_params.get("rp_min", -0.1)
        rp_max = reward_params.get("rp_max", -0.01)
        if rd_min >= rd_max:  # :76-79 (warnings only)
            print(f"Warning: rd_min ({rd_min}) should be less than rd_max ({rd_max}) in config.")
        if rp_min >= rp_max:
            print(f"Warning: rp_min ({rp_min}) should be less than rp_max ({rp_max}) in config.")

        radar_cfgs_all = sim_config.get("radars", []) or []
        jammer_cfgs_all = sim_config.get("jammers", []) or []
        num_jammers = getattr(config, "num_jammers", len(jammer_cfgs_all))  # :82-84
        num_radars = getattr(config, "num_radars", len(radar_cfgs_all))
        episode_limit = getattr(config, "episode_limit", 100)

        radar_cfgs = radar_cfgs_all[:num_radars]  # :129-131
        jammer_cfgs = jammer_cfgs_all[:num_jammers]  # :172-174
        if len(radar_cfgs) < num_radars or len(jammer_cfgs) < num_jammers:
            # The reference only warns here and then indexes past the end of its entity lists as
            # soon as such an entity is addressed; the batched kernel needs rectangular tables.
            raise ValueError(
                f"Requested {num_radars} radars / {num_jammers} jammers, but the scenario defines only "
                f"{len(radar_cfgs)} / {len(jammer_cfgs)}.")
        if not (1 <= num_radars <= MAX_RADARS and 1 <= num_jammers <= MAX_JAMMERS):
            raise ValueError(f"Scenario size {num_jammers}j/{num_radars}r outside the supported range "
                             f"1..{MAX_JAMMERS} / 1..{MAX_RADARS}.")
        motion = parse_motion(env_params, num_radars, num_jammers, source)
        if motion is not None and radar_scan is not None and float(motion["step_seconds"]) != float(radar_scan["step_seconds"]):
            # one env step is one dt for the beams and for the entities: the scan tables become per-step frames too
            raise ValueError(f"{source}: environment_params.motion together with radar_scan is not supported unless both run "
                             f"on one clock: motion.step_seconds ({motion['step_seconds']!r}) and radar_scan.step_seconds "
                             f"({radar_scan['step_seconds']!r}) must be equal")

        radars: List[Dict[str, Any]] = []
        for i, params in enumerate(radar_cfgs):  # :133-169
            try:
                for p_name in _REQUIRED_RADAR_PARAMS:
                    if p_name not in params:
                        raise KeyError(f"Radar config {i} missing required parameter: {p_name}")
                if not (0 <= params.get("type_id", -1) < max_radar_types):
                    raise ValueError(f"Radar config {i} invalid type_id")
            except KeyError as e:
                print(f"Error initializing radar {i}: Missing parameter {e} in simulation_config.yaml")
                raise
            except ValueError as e:
                print(f"Error initializing radar {i}: Invalid value - {e}")
                raise
            if radar_scan is not None:
                tm, ts = params["theta_m"], params["t_s"]
                if isinstance(tm, bool) or not isinstance(tm, (int, float)) or not (0.0 < tm <= 360.0):
                    raise ValueError(f"Radar config {i}: theta_m must lie in (0, 360] when radar_scan is on, got {tm!r}")
                if isinstance(ts, bool) or not isinstance(ts, (int, float)) or not (ts > 0.0) or not np.isfinite(ts):
                    raise ValueError(f"Radar config {i}: t_s must be > 0 when radar_scan is on, got {ts!r}")
                ta = params["theta_a"]
                if isinstance(ta, bool) or not isinstance(ta, (int, float)) or not np.isfinite(ta):
                    raise ValueError(f"Radar config {i}: theta_a must be a finite number when radar_scan is on, got {ta!r}")
                if "pattern" in radar_scan and not radar_scan["pattern"]["level_width"] * (float(tm) / 2) >= 1e-3:
                    # keeps q = x / (level_width half_beam) below 3.6e5 (x < 360): far inside the int32 conversion's range
                    raise ValueError(f"Radar config {i}: radar_scan.pattern.level_width * theta_m / 2 must be >= 1e-3, "
                                     f"got {radar_scan['pattern']['level_width']} * {tm} / 2")
            r = dict(params)
            r["threat_level"] = params.get("threat_level", 1.0)
            radars.append(r)

        jammers: List[Dict[str, Any]] = []
        for i, params in enumerate(jammer_cfgs):  # :176-199
            try:
                for p_name in _REQUIRED_JAMMER_PARAMS:
                    if p_name not in params:
                        raise KeyError(f"Jammer config {i} missing required parameter: {p_name}")
            except KeyError as e:
                print(f"Error initializing jammer {i}: Missing parameter {e} in simulation_config.yaml")
                raise
            extra = set(params) - _JAMMER_INIT_KEYS - {"power_max", "power_min"}
            if extra:  # Jammer(**init_params) in the reference, environment.py:186-190
                k = sorted(extra)[0]
                print(f"Error initializing jammer {i}: Jammer.__init__() got an unexpected keyword argument '{k}'")
                raise TypeError(f"Jammer.__init__() got an unexpected keyword argument '{k}'")
            j = dict(params)
            j["power_max"] = params.get("power_max", 100.0)
            j["power_min"] = params.get("power_min", 0.0)
            jammers.append(j)

        sc = cls(num_radars=num_radars, num_jammers=num_jammers, episode_limit=int(episode_limit),
                 max_radar_types=max_radar_types, rd_min=rd_min, rd_max=rd_max, rp_min=rp_min, rp_max=rp_max,
                 radars=radars, jammers=jammers, target_position=target_position, target_rcs=target_rcs,
                 source=source, radar_scan=radar_scan, motion=motion)
        sc._compile()
        if radar_scan is not None:
            sc._compile_scan()
        if motion is not None:
            sc._compile_motion(sim_config, config)
        return sc

    # ---- per-step frame tables of a moving scenario (include/macjd.h, macjd_motion_io) ----
    def _compile_motion(self, sim_config: dict, config: Any) -> None:
        """Frame f = the static scenario ``motion_frame_dict(sim_config, f)``, compiled by :meth:`from_dict` itself; its
        arrays are COPIED into row f, so every value has the bits a static scenario of that frame would have (the
        ``d <= 1e-6`` negative denominators and the weak-denominator flags included)."""
        R, J, F = self.num_radars, self.num_jammers, self.episode_limit
        if F < 1:
            raise ValueError(f"{self.source}: a moving scenario needs episode_limit >= 1, got {F}")
        cols = self.position_columns
        frames = np.zeros((F, 6 * R + 3 * J + J * R), dtype=np.float64)
        flags = np.zeros((F, J * R), dtype=np.uint8)
        snr_no = np.zeros((F, R), dtype=np.float64)
        positions = np.zeros((F + 1, len(cols)), dtype=np.float32)
        scan_frs = []   # the frames' compiled scenarios (scanning: their scan / pattern columns are copied below)
        for f in range(F + 1):
            fr = Scenario.from_dict(motion_frame_dict(sim_config, f), config=config, source=f"{self.source}[frame {f}]")
            positions[f] = fr.state_vector()[cols]
            if f < F:
                scan_frs.append(fr)
                frames[f] = np.concatenate([np.asarray(fr.tables[key], dtype=np.float64).reshape(-1)
                                            for key in _PE_RADAR_ROWS + _PE_JAMMER_ROWS + ("jr_denom",)])
                flags[f] = fr.tables["jr_flags"].reshape(-1)
                snr_no[f] = fr.tables["radar_snr_no"]
        self.motion_tables = {"frames": frames, "flags": flags, "snr_no": snr_no, "positions": positions,
                              "position_columns": np.asarray(cols, dtype=np.int32)}
        if self.scanning:   # the beams' tables per frame too (include/macjd.h, macjd_motion_scan_io)
            self.motion_tables["scan_frames"] = np.stack([_scan_column(fr) for fr in scan_frs])
            if self.scan_pattern_levels:
                self.motion_tables["pattern_frames"] = np.stack([_pattern_column(fr) for fr in scan_frs])

    def motion_compile_inputs(self) -> Dict[str, np.ndarray]:
        """Input column of the device frame compiler (include/macjd.h, macjd_motion_pe_compile_desc) for this moving
        scenario: ``{"column": float64 [MACJD_MOTION_PE_IN_ROWS(R, J)], "weak": uint8 [J]}``.  Needs only the static compile
        at the start positions (``self.tables``, frame 0) and the parsed ``motion`` block: no frame is compiled."""
        if not self.moving:
            raise AttributeError("motion_compile_inputs: the scenario does not move (no environment_params.motion)")
        return _motion_compile_inputs(self, self.motion)

    # ---- static tables ----
    def _compile(self) -> None:
        R, J = self.num_radars, self.num_jammers
        consts = detection_probability_constants()
        self.pd_consts = consts
        GaPs = np.zeros(R); Pn = np.zeros(R); D = np.zeros(R); pd_no = np.zeros(R)
        snr_no = np.zeros(R); rd_pen = np.zeros(R); gr_lin = np.zeros(R); Ps_tab = np.zeros(R)
        radar_pos = []
        for r, p in enumerate(self.radars):
            pt = float(p["pt"])                       # radar.py:11
            gt = db_to_linear(p["gt"])                # radar.py:12-13
            gr = db_to_linear(p["gr"])
            lam = p["wavelength"]
            loss = db_to_linear(p["loss"])            # radar.py:16-17
            latm = db_to_linear(p["latm"])
            pn_watts = 10 ** ((p["pn"] - 30) / 10)    # radar.py:19
            position = np.array(p["position"])
            radar_pos.append(position)
            # echo power of the PROTECTED TARGET at this radar, radar.py:35-60
            distance = np.linalg.norm(position - self.target_position)
            safe_distance = max(distance, 1e-6)
            numerator = pt * gt * gr * (lam ** 2) * self.target_rcs
            denominator = ((4 * np.pi) ** 3) * (safe_distance ** 4) * loss * latm
            Ps = 0.0 if denominator <= 1e-18 else numerator / denominator
            Ga = p["pulse_compression_gain"]
            ga_ps = Ga * Ps                           # environment.py:326
            s_no = ga_ps / pn_watts if pn_watts > 1e-18 else 0.0
            s_no = max(0.0, s_no)                     # environment.py:327
            Ps_tab[r] = Ps
            GaPs[r] = ga_ps
            Pn[r] = pn_watts
            D[r] = p["anti_jamming_factor"]
            snr_no[r] = s_no
            pd_no[r] = detection_probability(s_no, consts)           # environment.py:385
            rd_pen[r] = np.clip(-p["threat_level"], self.rd_min, self.rd_max)  # environment.py:362-365
            gr_lin[r] = gr                            # get_antenna_gain, radar.py:84-85

        pmin = np.zeros(J); pmax = np.zeros(J); gj_lin = np.zeros(J)
        denom = np.zeros((J, R)); flags = np.zeros((J, R), dtype=np.uint8)
        for j, p in enumerate(self.jammers):
            gj = db_to_linear(p["gj"])                # jammer.py:44-46
            loss = db_to_linear(p["loss"])
            latm = db_to_linear(p["latm"])
            bj = p["bj"]
            pmin[j] = p["power_min"]
            pmax[j] = p["power_max"]
            gj_lin[j] = gj
            jpos = np.array(p["position"])
            for r in range(R):
                distance = np.linalg.norm(np.array(jpos) - np.array(radar_pos[r]))  # math_utils.py:40-42
                if not (distance > 1e-6):             # environment.py:284
                    denom[j, r] = -1.0
                    continue
                distance_sq = max(1e-9, distance ** 2)    # jammer.py:83
                effective_bj = max(1e-9, bj)              # jammer.py:87
                den = distance_sq * loss * latm * effective_bj  # jammer.py:88
                denom[j, r] = den
                if not isinstance(den, np.floating):
                    # Python-float denominator: with a float32 numerator NumPy-2 keeps the division
                    # in float32 (weak scalar promotion)
                    flags[j, r] |= 1
        self.tables = {
            "radar_GaPs": GaPs, "radar_Pn": Pn, "radar_D": D, "radar_pd_no": pd_no,
            "radar_snr_no": snr_no, "radar_rd_pen": rd_pen, "radar_gr": gr_lin, "radar_Ps": Ps_tab,
            "jam_pmin": pmin, "jam_pmax": pmax, "jam_gj": gj_lin,
            "jr_denom": np.ascontiguousarray(denom.reshape(-1)),
            "jr_flags": np.ascontiguousarray(flags.reshape(-1)),
        }

    # ---- scanning-beam tables (include/macjd.h, macjd_scan_desc) ----
    def _compile_scan(self) -> None:
        R, J = self.num_radars, self.num_jammers
        dt = self.radar_scan["step_seconds"]
        rho = 10 ** (self.radar_scan["sidelobe_db"] / 10)
        t = self.tables
        half = np.zeros(R); sweep = np.zeros(R); swm = np.zeros(R); full = np.zeros(R, dtype=np.uint8)
        az0 = np.zeros(R); bt = np.zeros(R); bj = np.zeros((J, R))
        GaPs_side = np.zeros(R); snr_no_side = np.zeros(R); pd_no_side = np.zeros(R); gr_side = np.zeros(R)
        for r, p in enumerate(self.radars):
            half[r] = float(p["theta_m"]) / 2
            sweep[r] = 360.0 * dt / float(p["t_s"])
            swm[r] = np.fmod(sweep[r], 360.0)
            full[r] = 1 if sweep[r] + 2 * half[r] >= 360.0 else 0
            az0[r] = wrap_degrees(float(p["theta_a"]))
            bt[r] = bearing_degrees(p["position"], self.target_position)
            for j, q in enumerate(self.jammers):
                bj[j, r] = bearing_degrees(p["position"], q["position"])
            # side lobe: received jamming one-way (gr rho), the target's echo two-way (GaPs rho^2); the no-jamming SNR
            # and Pd from GaPs_side through the same host expressions as the main tables (_compile)
            gr_side[r] = t["radar_gr"][r] * rho
            ga_ps = t["radar_GaPs"][r] * (rho * rho)
            pn_watts = t["radar_Pn"][r]
            s_no = ga_ps / pn_watts if pn_watts > 1e-18 else 0.0
            s_no = max(0.0, s_no)
            GaPs_side[r] = ga_ps
            snr_no_side[r] = s_no
            pd_no_side[r] = detection_probability(s_no, self.pd_consts)
        self.scan_tables = {
            "half_beam": half, "sweep": sweep, "sweep_mod": swm, "full": full, "az0": az0, "bear_tgt": bt,
            "bear_jam": np.ascontiguousarray(bj.reshape(-1)), "GaPs_side": GaPs_side, "snr_no_side": snr_no_side,
            "pd_no_side": pd_no_side, "gr_side": gr_side, "rho": np.float64(rho),
        }
        pat = self.radar_scan.get("pattern")
        if pat is not None:
            # stepped antenna pattern (include/macjd.h, macjd_scan_pattern_desc): per level k = 1..L the side-lobe
            # expressions above with rho_k in place of rho
            L = len(pat["gain_db"])
            inv_width = np.zeros(R); pat_rho = np.zeros(L)
            pat_GaPs = np.zeros((L, R)); pat_gr = np.zeros((L, R)); pat_snr_no = np.zeros((L, R)); pat_pd_no = np.zeros((L, R))
            for r in range(R):
                inv_width[r] = 1.0 / (pat["level_width"] * half[r])
            for k, g_db in enumerate(pat["gain_db"]):
                rho_k = 10 ** (g_db / 10)
                pat_rho[k] = rho_k
                for r in range(R):
                    pat_gr[k, r] = t["radar_gr"][r] * rho_k
                    ga_ps = t["radar_GaPs"][r] * (rho_k * rho_k)
                    pn_watts = t["radar_Pn"][r]
                    s_no = ga_ps / pn_watts if pn_watts > 1e-18 else 0.0
                    s_no = max(0.0, s_no)
                    pat_GaPs[k, r] = ga_ps
                    pat_snr_no[k, r] = s_no
                    pat_pd_no[k, r] = detection_probability(s_no, self.pd_consts)
            self.scan_tables.update({"pat_inv_width": inv_width, "pat_rho": pat_rho, "pat_GaPs": pat_GaPs, "pat_gr": pat_gr,
                                     "pat_snr_no": pat_snr_no, "pat_pd_no": pat_pd_no})

    @property
    def scan_pattern_levels(self) -> int:
        """L of the stepped antenna pattern (``radar_scan.pattern.gain_db``), 0 without one."""
        return len(self.radar_scan["pattern"]["gain_db"]) if self.radar_scan and "pattern" in self.radar_scan else 0

    def c_scan_pattern_desc(self):
        """Returns (``_native.ScanPatternDesc`` instance, keepalive list) for a scenario with ``radar_scan.pattern``."""
        from ._native import ScanPatternDesc
        if not self.scan_pattern_levels:
            raise ValueError("c_scan_pattern_desc: the scenario has no radar_scan.pattern")
        st = self.scan_tables
        d = ScanPatternDesc()
        d.n_radars, d.n_levels = self.num_radars, self.scan_pattern_levels
        keep = []
        for name, key in (("inv_width", "pat_inv_width"), ("GaPs_lvl", "pat_GaPs"), ("snr_no_lvl", "pat_snr_no"),
                          ("pd_no_lvl", "pat_pd_no"), ("gr_lvl", "pat_gr")):
            a = np.ascontiguousarray(st[key], dtype=np.float64).reshape(-1)
            keep.append(a)
            setattr(d, name, a.ctypes.data)
        return d, keep

    def c_scan_desc(self):
        """Returns (``_native.ScanDesc`` instance, keepalive list).  Pointers reference ``self.scan_tables`` arrays."""
        from ._native import ScanDesc
        st = self.scan_tables
        d = ScanDesc()
        d.n_radars, d.n_jammers = self.num_radars, self.num_jammers
        keep = []
        for name, src in (("half_beam", st["half_beam"]), ("sweep", st["sweep"]), ("sweep_mod", st["sweep_mod"]),
                          ("az0", st["az0"]), ("bear_tgt", st["bear_tgt"]), ("bear_jam", st["bear_jam"]),
                          ("GaPs_side", st["GaPs_side"]), ("snr_no", self.tables["radar_snr_no"]),
                          ("snr_no_side", st["snr_no_side"]), ("pd_no_side", st["pd_no_side"]), ("gr_side", st["gr_side"])):
            a = np.ascontiguousarray(src, dtype=np.float64)
            keep.append(a)
            setattr(d, name, a.ctypes.data)
        f = np.ascontiguousarray(st["full"], dtype=np.uint8)
        keep.append(f)
        d.full = f.ctypes.data
        return d, keep

    # ---- observation pieces (static; environment.py:479-565) ----
    def state_vector(self) -> np.ndarray:
        """f32[S]: per radar [pt, theta_m, t_s, onehot(type_id), theta_a, x, y], then per jammer [x, y]
        (environment.py:479-510; utils/state_utils.py:3-27)."""
        feats: List[Any] = []
        for p in self.radars:
            feats.append(float(p["pt"]))
            feats.append(p["theta_m"])
            feats.append(p["t_s"])
            type_id = p["type_id"]
            if not isinstance(type_id, int):
                raise TypeError(f"Index must be an integer, got {type(type_id)}")
            onehot = np.zeros(self.max_radar_types, dtype=np.float32)
            onehot[type_id] = 1.0
            feats.extend(onehot)
            feats.append(p["theta_a"])
            feats.extend(np.array(p["position"]).flatten())
        for p in self.jammers:
            feats.extend(np.array(p["position"]).flatten())
        return np.array(feats, dtype=np.float32)

    def frame_state_rows(self) -> np.ndarray:
        """f32[F + 1, S] of a moving scenario: row k is ``state_vector()`` with ``position_columns`` replaced by
        ``motion_tables["positions"][k]`` — the state row every env shows at step counter k (the bits the moving step
        writes), equal to the state vector of the static scenario of frame k (``motion_frame_dict``)."""
        if not self.moving:
            raise AttributeError("frame_state_rows: the scenario does not move (no environment_params.motion)")
        pos = self.motion_tables["positions"]
        rows = np.repeat(self.state_vector()[None, :], pos.shape[0], axis=0)
        rows[:, self.motion_tables["position_columns"]] = pos
        return np.ascontiguousarray(rows, dtype=np.float32)

    def env_info(self) -> Dict[str, int]:
        """environment.py:553-565."""
        return {"state_shape": self.state_dim, "obs_shape": self.state_dim, "n_actions": self.n_actions,
                "n_agents": self.num_jammers, "episode_limit": self.episode_limit}

    # ---- native description ----
    def c_desc(self):
        """Returns (``_Desc`` instance, keepalive list).  Pointers reference ``self.tables`` arrays."""
        t = self.tables
        d = _Desc()
        d.n_radars, d.n_jammers, d.episode_limit, d.reserved = self.num_radars, self.num_jammers, self.episode_limit, 0
        d.rp_min, d.rp_max = float(self.rp_min), float(self.rp_max)
        d.pd_A, d.pd_c1, d.pd_denB = self.pd_consts
        keep = []
        for name in ("radar_GaPs", "radar_Pn", "radar_D", "radar_pd_no", "radar_snr_no", "radar_rd_pen",
                     "radar_gr", "jam_pmin", "jam_pmax", "jam_gj", "jr_denom"):
            a = np.ascontiguousarray(t[name], dtype=np.float64)
            keep.append(a)
            setattr(d, name, a.ctypes.data)
        f = np.ascontiguousarray(t["jr_flags"], dtype=np.uint8)
        keep.append(f)
        d.jr_flags = f.ctypes.data
        return d, keep


# Row order of the per-env SoA table (include/macjd.h, macjd_step_io.pe_tables)
_PE_RADAR_ROWS = ("radar_GaPs", "radar_Pn", "radar_D", "radar_pd_no", "radar_rd_pen", "radar_gr")
_PE_JAMMER_ROWS = ("jam_pmin", "jam_pmax", "jam_gj")
# Row order of the per-env scan SoA (include/macjd.h, macjd_scan_pe_io): R rows each, then bear_jam's J*R (j-major).
# "snr_no" is the main-lobe row of Scenario.tables; the others are Scenario.scan_tables arrays.
PE_SCAN_ROWS = ("half_beam", "sweep", "sweep_mod", "az0", "bear_tgt", "GaPs_side", "snr_no", "snr_no_side", "pd_no_side",
                "gr_side", "bear_jam")


# Row order of the per-env pattern SoA (include/macjd.h, macjd_scan_pe_pattern_io): inv_width's R rows, then four level
# tables of (L + 2) R rows each, level-major (level k of radar r at row k * R + r of its block).  Per table: (level 0 =
# the main-lobe array of Scenario.tables, levels 1..L = the Scenario.scan_tables array [L, R], level L + 1 = the side-lobe
# array of Scenario.scan_tables).
PE_SCAN_PATTERN_ROWS = ("inv_width", "GaPs_lvl", "snr_no_lvl", "pd_no_lvl", "gr_lvl")
_PE_PATTERN_LEVEL_SOURCES = {
    "GaPs_lvl": ("radar_GaPs", "pat_GaPs", "GaPs_side"), "snr_no_lvl": ("radar_snr_no", "pat_snr_no", "snr_no_side"),
    "pd_no_lvl": ("radar_pd_no", "pat_pd_no", "pd_no_side"), "gr_lvl": ("radar_gr", "pat_gr", "gr_side"),
}


def pe_scan_rows(n_radars: int, n_jammers: int) -> int:
    """MACJD_PE_SCAN_ROWS(R, J) of include/macjd.h."""
    return 10 * n_radars + n_jammers * n_radars


def pe_scan_pattern_rows(n_radars: int, n_levels: int) -> int:
    """MACJD_PE_SCAN_PATTERN_ROWS(R, L) of include/macjd.h."""
    return n_radars + 4 * (n_levels + 2) * n_radars


def _scan_column(sc: "Scenario") -> np.ndarray:
    """Scenario ``sc``'s own arrays in the row order ``PE_SCAN_ROWS``, as one float64 vector (copied, not recomputed)."""
    return np.concatenate([np.asarray(sc.tables["radar_snr_no"] if key == "snr_no" else sc.scan_tables[key],
                                      dtype=np.float64).reshape(-1) for key in PE_SCAN_ROWS])


def _pattern_column(sc: "Scenario") -> np.ndarray:
    """Scenario ``sc``'s own arrays in the row order ``PE_SCAN_PATTERN_ROWS``, as one float64 vector (copied, not recomputed)."""
    parts = [sc.scan_tables["pat_inv_width"]]
    for key in PE_SCAN_PATTERN_ROWS[1:]:
        main, levels, side = _PE_PATTERN_LEVEL_SOURCES[key]
        parts += [sc.tables[main], sc.scan_tables[levels], sc.scan_tables[side]]
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in parts])


def motion_pe_in_rows(n_radars: int, n_jammers: int) -> int:
    """MACJD_MOTION_PE_IN_ROWS(R, J) of include/macjd.h."""
    return 12 * n_radars + 10 * n_jammers + 4


FOUR_PI_CUBED = float((4 * np.pi) ** 3)   # as Scenario._compile evaluates it (radar.py:35-60)


def _motion_compile_inputs(sc: "Scenario", motion: Dict[str, Any]) -> Dict[str, np.ndarray]:
    """The device frame compiler's input column from ``sc`` — a scenario compiled at the START positions (a moving scenario's
    own static tables, or the static scenario of frame 0) — and the parsed motion block.  Row order of include/macjd.h,
    macjd_motion_pe_compile_desc; every per-entity factor is formed with the expressions of ``Scenario._compile``."""
    R, J = sc.num_radars, sc.num_jammers
    t = sc.tables
    dt = motion["step_seconds"]
    num = np.zeros(R); rloss = np.zeros(R); rlatm = np.zeros(R); ga = np.zeros(R)
    for r, p in enumerate(sc.radars):
        pt = float(p["pt"])
        gt = db_to_linear(p["gt"])
        gr = db_to_linear(p["gr"])
        lam = p["wavelength"]
        num[r] = pt * gt * gr * (lam ** 2) * sc.target_rcs
        rloss[r] = db_to_linear(p["loss"])
        rlatm[r] = db_to_linear(p["latm"])
        ga[r] = p["pulse_compression_gain"]
    jloss = np.zeros(J); jlatm = np.zeros(J); bj_eff = np.zeros(J); weak = np.zeros(J, dtype=np.uint8)
    for j, p in enumerate(sc.jammers):
        loss = db_to_linear(p["loss"])
        latm = db_to_linear(p["latm"])
        effective_bj = max(1e-9, p["bj"])
        jloss[j], jlatm[j], bj_eff[j] = loss, latm, effective_bj
        # the host's denominator max(1e-9, d^2) * loss * latm * bj is a Python float exactly when d^2 <= 1e-9 (the max
        # then returns its Python-float argument) and these three factors are Python floats too
        weak[j] = 0 if isinstance(1e-9 * loss * latm * effective_bj, np.floating) else 1

    def p0(pos):
        q = np.array(pos).flatten()
        return [float(q[0]), float(q[1])]

    def vdt(v):
        return [float(v[0]) * dt, float(v[1]) * dt]

    pos_rows = p0(sc.target_position) + vdt(motion["target_velocity"])
    pos_rows += [x for p in sc.radars for x in p0(p["position"])]
    pos_rows += [x for v in motion["radar_velocity"] for x in vdt(v)]
    pos_rows += [x for p in sc.jammers for x in p0(p["position"])]
    pos_rows += [x for v in motion["jammer_velocity"] for x in vdt(v)]
    col = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in (
        t["radar_Pn"], t["radar_D"], t["radar_rd_pen"], t["radar_gr"], num, rloss, rlatm, ga,
        t["jam_pmin"], t["jam_pmax"], t["jam_gj"], jloss, jlatm, bj_eff, pos_rows)])
    assert col.shape == (motion_pe_in_rows(R, J),)
    return {"column": col, "weak": weak}


def tile_envs(a: np.ndarray, tile: int) -> np.ndarray:
    """[E, ...] -> [n_tiles, ..., tile]: the tiled per-env layout with the env index split into (tile, column) and the
    column innermost; the last tile is zero-padded."""
    E = a.shape[0]
    n_tiles = (E + tile - 1) // tile
    padded = np.zeros((n_tiles * tile,) + a.shape[1:], dtype=a.dtype)
    padded[:E] = a
    padded = padded.reshape((n_tiles, tile) + a.shape[1:])
    return np.ascontiguousarray(np.moveaxis(padded, 1, -1))


def randomized_moving_scenario_dict(base: dict, rng: np.random.Generator, velocity_jitter: float = 0.0,
                                    num_radars: Optional[int] = None, num_jammers: Optional[int] = None, **jitter) -> dict:
    """``randomized_scenario_dict`` plus N(0, velocity_jitter) metres per second per axis on every velocity of the
    ``motion`` block (target, then radars, then jammers; a missing list counts as zeros for the ``num_radars`` /
    ``num_jammers`` entities used, default all defined).  The velocity draws come after all the others and only when the
    jitter is > 0: without it the dict and the generator's state afterwards are ``randomized_scenario_dict``'s."""
    d = randomized_scenario_dict(base, rng, **jitter)
    if velocity_jitter > 0:
        env_params = d.get("environment_params") or {}
        nr = len(d["radars"]) if num_radars is None else int(num_radars)
        nj = len(d["jammers"]) if num_jammers is None else int(num_jammers)
        mo = parse_motion(env_params, nr, nj)
        if mo is None:
            raise ValueError("randomized_moving_scenario_dict: the scenario does not move (no environment_params.motion)")
        draw = lambda v: [v[0] + float(rng.normal(0.0, velocity_jitter)), v[1] + float(rng.normal(0.0, velocity_jitter))]
        mo["target_velocity"] = draw(mo["target_velocity"])
        mo["radar_velocity"] = [draw(v) for v in mo["radar_velocity"]]
        mo["jammer_velocity"] = [draw(v) for v in mo["jammer_velocity"]]
        env_params["motion"] = mo
    return d


class MovingScenarioBatch:
    """E MOVING, non-scanning scenarios of one shape (same R, J, episode limit F, r_p bounds, Pd constants and
    ``motion.step_seconds``): every env has its own trajectory and so its own frame tables (include/macjd.h,
    macjd_motion_pe_io).  ``ScenarioBatch`` keeps refusing moving scenarios; this class is their per-env batch.

    Host path (``MovingScenarioBatch(scenarios)``): every scenario's own ``motion_tables`` stacked, bit for bit —
    ``frames`` f64 [E, F, rows], ``flags`` u8 [E, F, J*R], ``snr_no`` f64 [E, F, R], ``positions`` f32 [E, F + 1, n_pos];
    ``tiled(tile)`` gives them in the device layout.  Device path (``randomized(..., compile="device")``): only the input
    columns of the device frame compiler exist (``compile_inputs`` f64 [E, in_rows], ``compile_weak`` u8 [E, J]) and
    ``frames`` is None; the environment runs macjd_motion_pe_compile."""

    def __init__(self, scenarios: List[Scenario]):
        if not scenarios:
            raise ValueError("MovingScenarioBatch needs at least one scenario")
        for i, sc in enumerate(scenarios):
            if not sc.moving:
                raise ValueError(f"MovingScenarioBatch: scenario {i} does not move (no environment_params.motion); "
                                 f"ScenarioBatch takes static scenarios")
            if sc.scanning:
                raise ValueError(f"MovingScenarioBatch: scenario {i} has scanning radars (environment_params.radar_scan); "
                                 f"motion together with scanning is not supported on per-env batches")
        self._check_shared(scenarios, [sc.motion["step_seconds"] for sc in scenarios])
        self._init_common(scenarios[0], len(scenarios), np.stack([sc.state_vector() for sc in scenarios]))
        self.scenarios = list(scenarios)
        mt = [sc.motion_tables for sc in scenarios]
        self.frames = np.ascontiguousarray(np.stack([m["frames"] for m in mt]), dtype=np.float64)
        self.flags = np.ascontiguousarray(np.stack([m["flags"] for m in mt]), dtype=np.uint8)
        self.snr_no = np.ascontiguousarray(np.stack([m["snr_no"] for m in mt]), dtype=np.float64)
        self.positions = np.ascontiguousarray(np.stack([m["positions"] for m in mt]), dtype=np.float32)
        self.state_vectors[:, self.position_columns] = self.positions[:, 0]
        self.compile_inputs = self.compile_weak = None

    @staticmethod
    def _check_shared(scenarios: List[Scenario], step_seconds: List[float]) -> None:
        s0 = scenarios[0]
        for i, sc in enumerate(scenarios):
            same = (sc.num_radars == s0.num_radars and sc.num_jammers == s0.num_jammers
                    and sc.episode_limit == s0.episode_limit and sc.max_radar_types == s0.max_radar_types
                    and sc.rp_min == s0.rp_min and sc.rp_max == s0.rp_max and sc.pd_consts == s0.pd_consts)
            if not same:
                raise ValueError(f"MovingScenarioBatch: scenario {i} differs from scenario 0 in shape / episode limit / "
                                 f"r_p bounds / Pd constants (these are shared by the whole batch)")
            if step_seconds[i] != step_seconds[0]:
                raise ValueError(f"MovingScenarioBatch: scenario {i}'s motion.step_seconds ({step_seconds[i]!r}) differs from "
                                 f"scenario 0's ({step_seconds[0]!r}) (it is shared by the whole batch)")

    def _init_common(self, base: Scenario, n_envs: int, state_vectors: np.ndarray) -> None:
        self.base = base
        self.n_envs = int(n_envs)
        self.n_frames = int(base.episode_limit)
        if self.n_frames < 1:
            raise ValueError(f"MovingScenarioBatch: a moving scenario needs episode_limit >= 1, got {self.n_frames}")
        self.position_columns = np.asarray(base.position_columns, dtype=np.int32)
        self.state_vectors = np.ascontiguousarray(state_vectors, dtype=np.float32)

    @property
    def host_compiled(self) -> bool:
        """The frame tables exist on the host (built from scenarios' own ``motion_tables``)."""
        return self.frames is not None

    def tiled(self, tile: int) -> Dict[str, np.ndarray]:
        """The four tables in the device layout of include/macjd.h, macjd_motion_pe_io: ``frames`` [n_tiles, F, rows, tile],
        ``flags`` [n_tiles, F, J*R, tile], ``snr_no`` [n_tiles, F, R, tile], ``positions`` [n_tiles, F + 1, n_pos, tile]; the
        last tile is zero-padded.  Host-compiled batches only."""
        if not self.host_compiled:
            raise RuntimeError("MovingScenarioBatch.tiled: this batch was made for the device frame compiler "
                               "(compile='device'): no host frames exist")
        return {"frames": tile_envs(self.frames, tile), "flags": tile_envs(self.flags, tile),
                "snr_no": tile_envs(self.snr_no, tile), "positions": tile_envs(self.positions, tile)}

    def tiled_compile_inputs(self, tile: int) -> Dict[str, np.ndarray]:
        """The device frame compiler's input in its layout: ``in_tables`` f64 [n_tiles, in_rows, tile], ``in_weak`` u8
        [n_tiles, J, tile]."""
        if self.compile_inputs is None:
            raise RuntimeError("MovingScenarioBatch.tiled_compile_inputs: this batch carries no compiler inputs")
        return {"in_tables": tile_envs(self.compile_inputs, tile), "in_weak": tile_envs(self.compile_weak, tile)}

    def table_bytes(self, tile: int) -> int:
        """Bytes of the four device tables at env tile ``tile`` (the padded last tile included)."""
        R, J, F = self.base.num_radars, self.base.num_jammers, self.n_frames
        n_pad = ((self.n_envs + tile - 1) // tile) * tile
        return n_pad * (F * ((6 * R + 3 * J + J * R) * 8 + J * R + R * 8) + (F + 1) * (2 * R + 2 * J) * 4)

    @classmethod
    def randomized(cls, base_dict: dict, n_envs: int, seed: int = 0, config: Any = None, env_offset: int = 0,
                   velocity_jitter: float = 0.0, compile: str = "device", **jitter) -> "MovingScenarioBatch":
        """``n_envs`` random variations of the moving ``base_dict`` (``randomized_moving_scenario_dict``); env e of the batch
        is variation number ``env_offset + e`` of the stream keyed by ``seed`` (shard-invariant like
        ``ScenarioBatch.randomized``).  ``compile="host"`` compiles every frame of every env on the host (the yardstick, and
        fine for small batches); ``compile="device"`` compiles only each env's start positions and carries the device frame
        compiler's input columns: no host frames exist."""
        if compile not in ("device", "host"):
            raise ValueError(f"MovingScenarioBatch.randomized: compile must be 'device' or 'host', got {compile!r}")
        env_params = (base_dict or {}).get("environment_params") or {}
        if parse_motion(env_params) is None:
            raise ValueError("MovingScenarioBatch.randomized: the base scenario does not move (no environment_params.motion); "
                             "ScenarioBatch.randomized takes static scenarios")
        if parse_radar_scan(env_params) is not None:
            raise ValueError("MovingScenarioBatch.randomized: the base scenario has scanning radars "
                             "(environment_params.radar_scan); motion together with scanning is not supported on per-env batches")
        nr = getattr(config, "num_radars", None)
        nj = getattr(config, "num_jammers", None)
        dicts = []
        for e in range(n_envs):
            rng = np.random.default_rng([int(seed), int(env_offset) + e])
            dicts.append(randomized_moving_scenario_dict(base_dict, rng, velocity_jitter=velocity_jitter, num_radars=nr,
                                                         num_jammers=nj, **jitter))
        if compile == "host":
            return cls([Scenario.from_dict(d, config=config, source=f"<randomized moving {seed}:{env_offset + e}>")
                        for e, d in enumerate(dicts)])
        # device: the static scenario of frame 0 (the start positions) + the parsed motion block per env
        starts, motions = [], []
        for e, d in enumerate(dicts):
            sc0 = Scenario.from_dict(motion_frame_dict(d, 0), config=config, source=f"<randomized moving {seed}:{env_offset + e}>[frame 0]")
            starts.append(sc0)
            motions.append(parse_motion(d["environment_params"], sc0.num_radars, sc0.num_jammers))
        cls._check_shared(starts, [m["step_seconds"] for m in motions])
        out = object.__new__(cls)
        # the shared handle and shape come from a moving Scenario of env 0 (its own frames: one scenario's host compile)
        base = Scenario.from_dict(dicts[0], config=config, source=f"<randomized moving {seed}:{env_offset}>")
        out._init_common(base, n_envs, np.stack([sc0.state_vector() for sc0 in starts]))
        out.scenarios = None
        out.frames = out.flags = out.snr_no = out.positions = None
        ins = [_motion_compile_inputs(sc0, m) for sc0, m in zip(starts, motions)]
        out.compile_inputs = np.ascontiguousarray(np.stack([i["column"] for i in ins]))
        out.compile_weak = np.ascontiguousarray(np.stack([i["weak"] for i in ins]))
        return out


DEG_PER_RAD = float(180.0 / np.pi)   # np.degrees multiplies by this constant


def motion_scan_pe_in_rows(n_radars: int, n_levels: int) -> int:
    """MACJD_MOTION_SCAN_PE_IN_ROWS(R, L) of include/macjd.h."""
    return 4 * n_radars + 1 + (n_radars + n_levels if n_levels > 0 else 0)


def _scan_compile_inputs(sc: "Scenario") -> np.ndarray:
    """The beam-frame compiler's input column (include/macjd.h, macjd_motion_scan_pe_compile_desc) from ``sc``, a SCANNING
    scenario compiled at the start positions: half_beam | sweep | sweep_mod | az0 | rho | inv_width | rho_lvl, every value
    ``Scenario._compile_scan``'s own (copied from its ``scan_tables``)."""
    st = sc.scan_tables
    parts = [st["half_beam"], st["sweep"], st["sweep_mod"], st["az0"], [st["rho"]]]
    if sc.scan_pattern_levels:
        parts += [st["pat_inv_width"], st["pat_rho"]]
    col = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in parts])
    assert col.shape == (motion_scan_pe_in_rows(sc.num_radars, sc.scan_pattern_levels),)
    return col


class MovingScanScenarioBatch(MovingScenarioBatch):
    """E scenarios of one shape that both MOVE and SCAN on one clock (``float(motion.step_seconds) ==
    float(radar_scan.step_seconds)``): the per-env batch of ``config/scenario_3j4r_moving_scan.yaml``-like scenarios
    (include/macjd.h, macjd_motion_pe_io + macjd_motion_scan_pe_io).  ``MovingScenarioBatch`` keeps refusing ``radar_scan``.

    Shared by the batch: everything ``MovingScenarioBatch`` shares, the pattern's ``level_width`` and its number of levels L;
    ``sidelobe_db`` and the pattern's ``gain_db`` may differ per env (their values travel in each env's own columns).

    Host path (``MovingScanScenarioBatch(scenarios)``): every scenario's own ``motion_tables`` stacked, bit for bit —
    ``MovingScenarioBatch``'s four arrays plus ``scan_frames`` f64 [E, F, 10R + JR] and, L > 0, ``pattern_frames`` f64
    [E, F, R + 4(L+2)R].  Device path (``randomized(..., compile="device")``): ``compile_inputs`` / ``compile_weak`` of the first
    compiler plus ``scan_compile_inputs`` f64 [E, MACJD_MOTION_SCAN_PE_IN_ROWS(R, L)]; the environment runs
    macjd_motion_pe_compile, then macjd_motion_scan_pe_compile."""

    def __init__(self, scenarios: List[Scenario]):
        if not scenarios:
            raise ValueError("MovingScanScenarioBatch needs at least one scenario")
        for i, sc in enumerate(scenarios):
            if not sc.moving:
                raise ValueError(f"MovingScanScenarioBatch: scenario {i} does not move (no environment_params.motion); "
                                 f"ScenarioBatch(..., scan=True) takes static scanning scenarios")
            if not sc.scanning:
                raise ValueError(f"MovingScanScenarioBatch: scenario {i} has no scanning radars (no environment_params.radar_scan); "
                                 f"MovingScenarioBatch takes moving scenarios without them")
        self._check_shared(scenarios, [sc.motion["step_seconds"] for sc in scenarios])
        self._check_scan_shared([sc.radar_scan for sc in scenarios])
        self._init_common(scenarios[0], len(scenarios), np.stack([sc.state_vector() for sc in scenarios]))
        self.scenarios = list(scenarios)
        mt = [sc.motion_tables for sc in scenarios]
        self.frames = np.ascontiguousarray(np.stack([m["frames"] for m in mt]), dtype=np.float64)
        self.flags = np.ascontiguousarray(np.stack([m["flags"] for m in mt]), dtype=np.uint8)
        self.snr_no = np.ascontiguousarray(np.stack([m["snr_no"] for m in mt]), dtype=np.float64)
        self.positions = np.ascontiguousarray(np.stack([m["positions"] for m in mt]), dtype=np.float32)
        self.scan_frames = np.ascontiguousarray(np.stack([m["scan_frames"] for m in mt]), dtype=np.float64)
        self.pattern_frames = (np.ascontiguousarray(np.stack([m["pattern_frames"] for m in mt]), dtype=np.float64)
                               if self.scan_pattern_levels else None)
        self.state_vectors[:, self.position_columns] = self.positions[:, 0]
        self.compile_inputs = self.compile_weak = self.scan_compile_inputs = None

    @staticmethod
    def _check_scan_shared(scans: List[Dict[str, Any]]) -> None:
        """``scans``: every env's parsed ``radar_scan`` block."""
        p0 = scans[0].get("pattern")
        for i, rs in enumerate(scans):
            p = rs.get("pattern")
            if (p is None) != (p0 is None) or (p is not None and len(p["gain_db"]) != len(p0["gain_db"])):
                raise ValueError(f"MovingScanScenarioBatch: scenario {i}'s stepped antenna pattern has another number of levels "
                                 f"than scenario 0's (L is shared by the whole batch)")
            if p is not None and float(p["level_width"]) != float(p0["level_width"]):
                raise ValueError(f"MovingScanScenarioBatch: scenario {i}'s radar_scan.pattern.level_width ({p['level_width']!r}) "
                                 f"differs from scenario 0's ({p0['level_width']!r}) (it is shared by the whole batch)")

    @property
    def scan_pattern_levels(self) -> int:
        """L of the batch's stepped antenna pattern, 0 without one."""
        return int(self.base.scan_pattern_levels)

    def tiled(self, tile: int) -> Dict[str, np.ndarray]:
        """``MovingScenarioBatch.tiled`` plus ``scan_frames`` [n_tiles, F, 10R + JR, tile] and, L > 0, ``pattern_frames``
        [n_tiles, F, R + 4(L+2)R, tile] (include/macjd.h, macjd_motion_scan_pe_io).  Host-compiled batches only."""
        out = super().tiled(tile)
        out["scan_frames"] = tile_envs(self.scan_frames, tile)
        if self.pattern_frames is not None:
            out["pattern_frames"] = tile_envs(self.pattern_frames, tile)
        return out

    def tiled_compile_inputs(self, tile: int) -> Dict[str, np.ndarray]:
        """``MovingScenarioBatch.tiled_compile_inputs`` plus ``scan_in`` f64 [n_tiles, scan_in_rows, tile]."""
        out = super().tiled_compile_inputs(tile)
        out["scan_in"] = tile_envs(self.scan_compile_inputs, tile)
        return out

    def table_bytes(self, tile: int) -> int:
        """Bytes of the device tables at env tile ``tile``: ``MovingScenarioBatch``'s four plus the scan and pattern frames."""
        R, J, F, L = self.base.num_radars, self.base.num_jammers, self.n_frames, self.scan_pattern_levels
        n_pad = ((self.n_envs + tile - 1) // tile) * tile
        beam_rows = pe_scan_rows(R, J) + (pe_scan_pattern_rows(R, L) if L else 0)
        return super().table_bytes(tile) + n_pad * F * beam_rows * 8

    @classmethod
    def randomized(cls, base_dict: dict, n_envs: int, seed: int = 0, config: Any = None, env_offset: int = 0,
                   velocity_jitter: float = 0.0, compile: str = "device", **jitter) -> "MovingScanScenarioBatch":
        """``MovingScenarioBatch.randomized`` for a base that both moves and scans on one clock (``azimuth_jitter`` among the
        jitters moves every radar's initial beam azimuth); env e is variation ``env_offset + e`` of the stream keyed by
        ``seed``.  ``compile="device"`` compiles only the static scanning scenario of frame 0 per env and carries the two
        compilers' input columns."""
        if compile not in ("device", "host"):
            raise ValueError(f"MovingScanScenarioBatch.randomized: compile must be 'device' or 'host', got {compile!r}")
        env_params = (base_dict or {}).get("environment_params") or {}
        mo0, rs0 = parse_motion(env_params), parse_radar_scan(env_params)
        if mo0 is None:
            raise ValueError("MovingScanScenarioBatch.randomized: the base scenario does not move (no environment_params.motion); "
                             "ScenarioBatch.randomized takes static scenarios")
        if rs0 is None:
            raise ValueError("MovingScanScenarioBatch.randomized: the base scenario has no scanning radars (no "
                             "environment_params.radar_scan); MovingScenarioBatch.randomized takes moving scenarios without them")
        nr = getattr(config, "num_radars", None)
        nj = getattr(config, "num_jammers", None)
        dicts = []
        for e in range(n_envs):
            rng = np.random.default_rng([int(seed), int(env_offset) + e])
            dicts.append(randomized_moving_scenario_dict(base_dict, rng, velocity_jitter=velocity_jitter, num_radars=nr,
                                                         num_jammers=nj, **jitter))
        if compile == "host":
            return cls([Scenario.from_dict(d, config=config, source=f"<randomized moving scan {seed}:{env_offset + e}>")
                        for e, d in enumerate(dicts)])
        # the shared handle and shape come from a moving scanning Scenario of env 0 (one scenario's host compile; it also
        # applies the one-clock rule with the existing wording)
        base = Scenario.from_dict(dicts[0], config=config, source=f"<randomized moving scan {seed}:{env_offset}>")
        starts, motions = [], []
        for e, d in enumerate(dicts):
            sc0 = Scenario.from_dict(motion_frame_dict(d, 0), config=config,
                                     source=f"<randomized moving scan {seed}:{env_offset + e}>[frame 0]")
            starts.append(sc0)
            motions.append(parse_motion(d["environment_params"], sc0.num_radars, sc0.num_jammers))
        cls._check_shared(starts, [m["step_seconds"] for m in motions])
        cls._check_scan_shared([sc0.radar_scan for sc0 in starts])
        out = object.__new__(cls)
        out._init_common(base, n_envs, np.stack([sc0.state_vector() for sc0 in starts]))
        out.scenarios = None
        out.frames = out.flags = out.snr_no = out.positions = out.scan_frames = out.pattern_frames = None
        ins = [_motion_compile_inputs(sc0, m) for sc0, m in zip(starts, motions)]
        out.compile_inputs = np.ascontiguousarray(np.stack([i["column"] for i in ins]))
        out.compile_weak = np.ascontiguousarray(np.stack([i["weak"] for i in ins]))
        out.scan_compile_inputs = np.ascontiguousarray(np.stack([_scan_compile_inputs(sc0) for sc0 in starts]))
        return out


def randomized_scenario_dict(base: dict, rng: np.random.Generator, position_jitter: float = 60.0,
                             threat_jitter: float = 0.15, power_jitter: float = 0.2, azimuth_jitter: float = 0.0) -> dict:
    """One random variation of a scenario dict in the reference's schema: radar and jammer
    positions moved by N(0, position_jitter) metres per axis, threat levels by N(0, threat_jitter), radar peak
    power ``pt`` and jammer ``power_max`` scaled by exp(N(0, power_jitter)); with ``azimuth_jitter`` > 0 every radar's
    initial beam azimuth ``theta_a`` moved by N(0, azimuth_jitter) degrees (scanning radars).  Everything else is kept.
    The azimuth draws come after all the others and only when the jitter is > 0: without it the dict and the
    generator's state afterwards are what they were before the option existed."""
    import copy
    d = copy.deepcopy(base)
    for r in d["radars"]:
        x, y = (float(v) for v in np.array(r["position"]).flatten()[:2])
        r["position"] = [x + float(rng.normal(0.0, position_jitter)), y + float(rng.normal(0.0, position_jitter))]
        r["threat_level"] = float(r.get("threat_level", 1.0) + rng.normal(0.0, threat_jitter))
        r["pt"] = float(r["pt"] * np.exp(rng.normal(0.0, power_jitter)))
    for j in d["jammers"]:
        x, y = (float(v) for v in np.array(j["position"]).flatten()[:2])
        j["position"] = [x + float(rng.normal(0.0, position_jitter)), y + float(rng.normal(0.0, position_jitter))]
        j["power_max"] = float(j.get("power_max", 100.0) * np.exp(rng.normal(0.0, power_jitter)))
    if azimuth_jitter > 0:
        for r in d["radars"]:
            r["theta_a"] = float(r.get("theta_a", 0.0)) + float(rng.normal(0.0, azimuth_jitter))
    return d


class ScenarioBatch:
    """E scenarios of one shape (same R, J, episode limit, r_p bounds, Pd constants), compiled one by one with
    :class:`Scenario` (so each env's tables are exactly what a single-scenario environment would use) and stacked
    as the per-env SoA the step kernel streams: ``tables`` float64 [6R + 3J + JR, E], ``flags`` uint8 [JR, E],
    plus the per-env observation vectors ``state_vectors`` f32 [E, S] and ``snr_no`` f64 [E, R].

    ``scan=True`` makes a batch of SCANNING scenarios: all of them scan with one ``radar_scan`` dict (shared by the batch
    like the r_p bounds) and no stepped antenna pattern; their scan tables are stacked as ``scan_tables`` float64
    [10R + JR, E] in the row order ``PE_SCAN_ROWS`` (include/macjd.h, macjd_scan_pe_io), column e bit-identical to
    scenario e's own arrays.  ``full`` is not carried (the device recomputes sweep + 2 half_beam >= 360 with the same
    bits).  Without ``scan`` a scanning scenario is refused and ``scan_tables`` is None.

    ``scan=True, pattern=True`` makes a scanning batch under a stepped antenna pattern: every scenario has a
    ``radar_scan.pattern`` (part of the shared ``radar_scan`` dict, so ``level_width``, ``gain_db`` and L are the batch's),
    and the level tables are stacked as ``pattern_tables`` float64 [R + 4 (L + 2) R, E] in the row order
    ``PE_SCAN_PATTERN_ROWS`` (include/macjd.h, macjd_scan_pe_pattern_io), column e again scenario e's own arrays bit for bit.
    Without ``pattern`` a scenario that has one is refused and ``pattern_tables`` is None."""

    def __init__(self, scenarios: List[Scenario], *, scan: bool = False, pattern: bool = False):
        if not scenarios:
            raise ValueError("ScenarioBatch needs at least one scenario")
        if pattern and not scan:
            i = next((k for k, sc in enumerate(scenarios) if sc.scan_pattern_levels), 0)
            raise ValueError(f"ScenarioBatch(pattern=True) needs scan=True (scenario {i}: the stepped antenna pattern belongs "
                             f"to scanning radars)")
        for i, sc in enumerate(scenarios):
            if sc.moving:
                raise ValueError(f"ScenarioBatch: scenario {i} moves (environment_params.motion); moving scenarios are not "
                                 f"supported in per-env scenario batches")
        s0 = scenarios[0]
        for i, sc in enumerate(scenarios):
            same = (sc.num_radars == s0.num_radars and sc.num_jammers == s0.num_jammers
                    and sc.episode_limit == s0.episode_limit and sc.max_radar_types == s0.max_radar_types
                    and sc.rp_min == s0.rp_min and sc.rp_max == s0.rp_max and sc.pd_consts == s0.pd_consts)
            if not same:
                raise ValueError(f"ScenarioBatch: scenario {i} differs from scenario 0 in shape / episode limit / "
                                 f"r_p bounds / Pd constants (these are shared by the whole batch)")
        if not scan and any(sc.scanning for sc in scenarios):
            raise ValueError("ScenarioBatch: scanning radars (environment_params.radar_scan) are not supported with per-env "
                             "scenario batches unless the batch is built with scan=True")
        for i, sc in enumerate(scenarios if scan else ()):
            if not sc.scanning:
                raise ValueError(f"ScenarioBatch(scan=True): scenario {i} has no environment_params.radar_scan (every "
                                 f"scenario of a scanning batch must scan)")
            if pattern and "pattern" not in sc.radar_scan:
                raise ValueError(f"ScenarioBatch(scan=True, pattern=True): scenario {i} has no radar_scan.pattern (every "
                                 f"scenario of such a batch must have the stepped antenna pattern)")
            if not pattern and "pattern" in sc.radar_scan:
                raise ValueError(f"ScenarioBatch(scan=True): scenario {i} has a radar_scan.pattern (the stepped antenna "
                                 f"pattern is not supported with per-env scenario batches unless the batch is built "
                                 f"with pattern=True)")
            if sc.radar_scan != s0.radar_scan:
                raise ValueError(f"ScenarioBatch(scan=True): scenario {i}'s radar_scan {sc.radar_scan} differs from scenario "
                                 f"0's {s0.radar_scan} (it is shared by the whole batch)")
        self.scenarios = list(scenarios)
        self.base = s0
        self.n_envs = len(scenarios)
        rows = []
        for key in _PE_RADAR_ROWS + _PE_JAMMER_ROWS + ("jr_denom",):
            rows.append(np.stack([np.asarray(sc.tables[key], dtype=np.float64).reshape(-1) for sc in scenarios], axis=1))
        self.tables = np.ascontiguousarray(np.concatenate(rows, axis=0))                     # [rows, E]
        self.flags = np.ascontiguousarray(np.stack([sc.tables["jr_flags"].reshape(-1) for sc in scenarios], axis=1)
                                          .astype(np.uint8))                                  # [J*R, E]
        self.state_vectors = np.stack([sc.state_vector() for sc in scenarios]).astype(np.float32)
        self.snr_no = np.stack([sc.tables["radar_snr_no"] for sc in scenarios]).astype(np.float64)
        R, J = s0.num_radars, s0.num_jammers
        assert self.tables.shape == (6 * R + 3 * J + J * R, self.n_envs)
        self.scan_tables = None
        if scan:
            self.scan_tables = np.ascontiguousarray(np.stack([_scan_column(sc) for sc in scenarios], axis=1))   # [10R + JR, E]
            assert self.scan_tables.shape == (pe_scan_rows(R, J), self.n_envs)
        self.pattern_tables = None
        if pattern:
            self.pattern_tables = np.ascontiguousarray(np.stack([_pattern_column(sc) for sc in scenarios], axis=1))
            assert self.pattern_tables.shape == (pe_scan_pattern_rows(R, s0.scan_pattern_levels), self.n_envs)

    @property
    def scanning(self) -> bool:
        """The batch carries per-env scan tables (built with ``scan=True``)."""
        return self.scan_tables is not None

    @property
    def scan_pattern_levels(self) -> int:
        """L of the batch's stepped antenna pattern (built with ``pattern=True``), 0 without one."""
        return self.base.scan_pattern_levels if self.pattern_tables is not None else 0

    def tile(self, n_envs: int) -> "ScenarioBatch":
        """A batch of ``n_envs`` envs that cycles through this batch's scenarios (env e runs scenario e mod E) —
        for streaming-size measurements, where compiling millions of distinct scenarios on the host is pointless."""
        reps = (int(n_envs) + self.n_envs - 1) // self.n_envs
        out = object.__new__(ScenarioBatch)
        out.scenarios = None                       # too many to keep per-env objects; ``base`` carries the shape
        out.base, out.n_envs = self.base, int(n_envs)
        out.tables = np.ascontiguousarray(np.tile(self.tables, (1, reps))[:, :n_envs])
        out.flags = np.ascontiguousarray(np.tile(self.flags, (1, reps))[:, :n_envs])
        out.state_vectors = np.ascontiguousarray(np.tile(self.state_vectors, (reps, 1))[:n_envs])
        out.snr_no = np.ascontiguousarray(np.tile(self.snr_no, (reps, 1))[:n_envs])
        out.scan_tables = (None if self.scan_tables is None
                           else np.ascontiguousarray(np.tile(self.scan_tables, (1, reps))[:, :n_envs]))
        out.pattern_tables = (None if self.pattern_tables is None
                              else np.ascontiguousarray(np.tile(self.pattern_tables, (1, reps))[:, :n_envs]))
        return out

    @classmethod
    def randomized(cls, base_dict: dict, n_envs: int, seed: int = 0, config: Any = None, env_offset: int = 0,
                   **jitter) -> "ScenarioBatch":
        """``n_envs`` random variations of ``base_dict``; env e of the batch is variation number ``env_offset + e``
        of the stream keyed by ``seed`` (shard-invariant: a rank's shard of a bigger batch is the same scenarios).  A base
        with ``environment_params.radar_scan`` gives a scanning batch (``scan=True``), one with ``radar_scan.pattern`` a
        scanning batch under that pattern (``pattern=True``)."""
        scs = []
        for e in range(n_envs):
            rng = np.random.default_rng([int(seed), int(env_offset) + e])
            scs.append(Scenario.from_dict(randomized_scenario_dict(base_dict, rng, **jitter), config=config,
                                          source=f"<randomized {seed}:{env_offset + e}>"))
        return cls(scs, scan=scs[0].scanning, pattern=scs[0].scan_pattern_levels > 0)


def ring_scenario_dict(n_jammers: int, n_radars: int) -> dict:
    """Build-authored ring scenarios in the reference's YAML schema for sizes the reference does not
    ship (it ships 2 jammers / 2 radars only, config/simulation_config.yaml).  Definition from
    SURVEY.md section 8(d): radar r of R at 400*(cos, sin)(2 pi r / R) m, theta_a = deg(2 pi r / R),
    other radar parameters alternating between the two shipped radar parameter sets, type_id = r mod 4,
    threat_level = 0.8 + 0.4 r / (R-1); jammer j of J at 70*(cos, sin)(2 pi j / J + 0.3) m with the shipped
    jammer parameters (power_max defaults to 100 W, power_min to 0); protected target at the origin."""
    import math
    tmpl = [
        dict(pt=300.0, gt=30, gr=30, wavelength=0.03, rcs=1.0, loss=10, latm=2, pn=3, theta_m=2.0, t_s=5.0,
             pulse_compression_gain=100.0, anti_jamming_factor=10.0),
        dict(pt=180.0, gt=25, gr=25, wavelength=0.03, rcs=1.0, loss=10, latm=2, pn=3, theta_m=1.8, t_s=4.0,
             pulse_compression_gain=120.0, anti_jamming_factor=15.0),
    ]
    radars = []
    for r in range(n_radars):
        ang = 2.0 * math.pi * r / n_radars
        p = dict(tmpl[r % 2])
        p.update(type_id=r % 4, position=[400.0 * math.cos(ang), 400.0 * math.sin(ang)],
                 theta_a=math.degrees(ang),
                 threat_level=0.8 + 0.4 * r / (n_radars - 1) if n_radars > 1 else 1.0)
        radars.append(p)
    jammers = []
    for j in range(n_jammers):
        ang = 2.0 * math.pi * j / n_jammers + 0.3
        jammers.append(dict(power=1000, gj=20, loss=5, latm=2, bj=10,
                            position=[70.0 * math.cos(ang), 70.0 * math.sin(ang)]))
    return dict(radars=radars, jammers=jammers, protected_target=dict(position=[0, 0], rcs=1.0),
                environment_params=dict(max_radar_types=4,
                                        rewards=dict(rd_min=-1.2, rd_max=-0.8, rp_min=-0.1, rp_max=-0.01)))
