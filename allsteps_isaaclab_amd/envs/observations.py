"""Device state of an env's observation manager (``cfg.observations``) and the ``env.observation_manager`` view of it.

``DirectRLEnv`` builds an :class:`EnvObservations` once the subclass has its device state and launches
``as_observations_step`` last in ``step`` -- after the step and its in-kernel reset, the contact timers, the commands
and the interval events, the reference's order (manager_based_rl_env.py step) -- once per group, on the env's stream
(csrc/observation_kernels.h; semantics and Philox stream: csrc/allsteps_observations.h).  Everything the kernel reads
and writes -- the term descriptors, the column table, the output map, the output rows that hold the history, the push
counts and the per-env stream counters -- lives in fixed device tensors, so a step captured in a HIP graph replays
with fresh draws and a moving history, and ``set_term_cfg`` takes effect in a graph that is already captured.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from .. import _native
from ..utils import commands as CM
from ..utils import noise as NZ
from ..utils import observations as OB
from ..utils import sensors as SN
from ..utils.observations import resolve_joint_ids  # noqa: F401  (re-exported)
from ._manager import DeviceState, cfg_items, is_number, u8

_SRC = {name: k for k, name in enumerate(_native.OBS_SOURCES)}
_NOISE = {NZ.constant_noise: (_native.NOISE_CONSTANT, ("bias", None)),
          NZ.uniform_noise: (_native.NOISE_UNIFORM, ("n_min", "n_max")),
          NZ.gaussian_noise: (_native.NOISE_GAUSSIAN, ("mean", "std"))}


def _unsupported(group: str, term: str | None, detail: str) -> "_native.NativeError":
    where = f"cfg.observations group {group!r}" + ("" if term is None else f" term {term!r}")
    return _native.NativeError(f"{where}: {detail}.  The observations are assembled in a HIP kernel (no host "
                               f"fallback); supported: {OB.SUPPORTED}")


@dataclass
class ObsContext:
    """What the terms of an env can read -- the host facts the parser checks a cfg against (no device needed)."""

    joint_names: list
    default_joint_pos: np.ndarray  # (joints,) float32
    default_joint_vel: np.ndarray  # (joints,) float32
    soft_joint_pos_limits: np.ndarray  # (joints, 2) float32
    action_cols: int
    clamp_actions: bool = False  # the env's `actions` clamps to [-1, 1]
    command_names: list = field(default_factory=list)
    ray_sensors: dict = field(default_factory=dict)  # scene name -> rays
    imu_names: list = field(default_factory=list)


@dataclass
class TermSpec:
    """One parsed term: what the descriptor row and the column table's entries are made from."""

    name: str
    cfg: object
    kind: int
    source: int
    rows: list  # source row of every column
    a: np.ndarray
    b: np.ndarray
    noise_kind: int
    noise_op: int
    p0: np.ndarray
    p1: np.ndarray
    clip: tuple | None
    scale: np.ndarray
    history_length: int
    flatten: bool
    flags: int = 0

    width = property(lambda self: len(self.rows))
    slots = property(lambda self: max(1, self.history_length))

    @property
    def dims(self) -> tuple:
        if self.history_length > 0:
            return (self.slots * self.width,) if self.flatten else (self.slots, self.width)
        return (self.width,)


def _asset(params: dict, key: str, default: str, g: str, t: str) -> object:
    cfg = params.get(key, None)
    if cfg is None:
        return OB.SceneEntityCfg(default)
    if not hasattr(cfg, "name"):
        raise _unsupported(g, t, f"params[{key!r}] = {cfg!r} is not a SceneEntityCfg")
    return cfg


def _params(params: dict, allowed: tuple, g: str, t: str) -> None:
    extra = sorted(set(params) - set(allowed))
    if extra:
        raise _unsupported(g, t, f"params {extra} are not parameters of the term function (it takes {list(allowed)})")


def _term_source(func, params: dict, ctx: ObsContext, g: str, t: str):
    """(kind, source, rows, a, b, flags) of a term function on the env of ``ctx``."""
    f32 = np.float32
    G, S = _native.OBS_GATHER, _SRC
    zeros = lambda k: np.zeros(k, f32)  # noqa: E731
    name = getattr(func, "__name__", repr(func))
    root = {OB.base_pos_z: ("root_pos", [2]), OB.root_pos_w: ("root_pos", [0, 1, 2]),
            OB.root_lin_vel_w: ("root_lin", [0, 1, 2]), OB.root_ang_vel_w: ("root_ang", [0, 1, 2])}
    rotated = {OB.base_lin_vel: "root_lin", OB.base_ang_vel: "root_ang", OB.projected_gravity: "gravity"}
    joints = {OB.joint_pos: "q", OB.joint_pos_rel: "q", OB.joint_pos_limit_normalized: "q", OB.joint_vel: "qd",
              OB.joint_vel_rel: "qd"}
    imus = {SN.imu_orientation: 3, SN.imu_ang_vel: 10, SN.imu_lin_acc: 13}
    if func in root or func in rotated or func is OB.root_quat_w:
        _params(params, ("asset_cfg", "make_quat_unique") if func is OB.root_quat_w else ("asset_cfg",), g, t)
        asset = _asset(params, "asset_cfg", "robot", g, t)
        if asset.name != "robot":
            raise _unsupported(g, t, f"asset_cfg.name = {asset.name!r} is not 'robot' (the env's articulation)")
        if func in root:
            src, rows = root[func]
            return G, S[src], rows, zeros(len(rows)), zeros(len(rows)), 0
        if func in rotated:
            return _native.OBS_ROTATE_INVERSE, S[rotated[func]], [0, 1, 2], zeros(3), zeros(3), 0
        kind = _native.OBS_QUAT_UNIQUE if params.get("make_quat_unique", False) else G
        return kind, S["root_quat"], [0, 1, 2, 3], zeros(4), zeros(4), 0
    if func in joints:
        _params(params, ("asset_cfg",), g, t)
        asset = _asset(params, "asset_cfg", "robot", g, t)
        if asset.name != "robot":
            raise _unsupported(g, t, f"asset_cfg.name = {asset.name!r} is not 'robot' (the env's articulation)")
        try:
            ids = resolve_joint_ids(asset, ctx.joint_names, "asset_cfg")
        except ValueError as e:
            raise _unsupported(g, t, str(e)) from None
        ids = list(range(len(ctx.joint_names))) if ids is None else ids
        if not ids:
            raise _unsupported(g, t, "asset_cfg selects no joint")
        a, b, kind = zeros(len(ids)), zeros(len(ids)), G
        if func is OB.joint_pos_rel:
            a = ctx.default_joint_pos.astype(f32)[ids]
        elif func is OB.joint_vel_rel:
            a = ctx.default_joint_vel.astype(f32)[ids]
        elif func is OB.joint_pos_limit_normalized:  # math.py scale_transform's two tensors, float32 as torch's
            lo, hi = ctx.soft_joint_pos_limits.astype(f32)[ids, 0], ctx.soft_joint_pos_limits.astype(f32)[ids, 1]
            a, b, kind = (lo + hi) * f32(0.5), hi - lo, _native.OBS_LIMIT_NORM
        return kind, S[joints[func]], ids, a, b, 0
    if func is OB.last_action:
        _params(params, ("action_name",), g, t)
        if params.get("action_name", None) is not None:
            raise _unsupported(g, t, f"action_name = {params['action_name']!r}: the env has one action term (None)")
        k = ctx.action_cols
        return _native.OBS_LAST_ACTION, S["actions"], list(range(k)), zeros(k), zeros(k), int(ctx.clamp_actions)
    if func is CM.generated_commands:
        _params(params, ("command_name",), g, t)
        cname = params.get("command_name", None)
        if cname not in ctx.command_names:
            raise _unsupported(g, t, f"command_name = {cname!r} names no command term of cfg.commands "
                                     f"({ctx.command_names})")
        k = ctx.command_names.index(cname)
        return G, S["commands"], [3 * k, 3 * k + 1, 3 * k + 2], zeros(3), zeros(3), 0
    if func is SN.height_scan:
        _params(params, ("sensor_cfg", "offset"), g, t)
        sensor = params.get("sensor_cfg", None)
        sname = getattr(sensor, "name", None)
        if sname not in ctx.ray_sensors:
            raise _unsupported(g, t, f"sensor_cfg names the sensor {sname!r}; the env's cfg has the ray casters "
                                     f"{sorted(ctx.ray_sensors)} (cfg.height_scanner)")
        offset = params.get("offset", 0.5)
        if not is_number(offset):
            raise _unsupported(g, t, f"offset = {offset!r} is not a number")
        R = int(ctx.ray_sensors[sname])
        return (_native.OBS_HEIGHT_SCAN, S["ray_hits"], [2 * R + r for r in range(R)], np.full(R, f32(offset), f32),
                zeros(R), 0)
    if func in imus:
        _params(params, ("asset_cfg",), g, t)
        asset = _asset(params, "asset_cfg", "imu", g, t)
        if asset.name not in ctx.imu_names:
            raise _unsupported(g, t, f"asset_cfg names the sensor {asset.name!r}; the env's cfg has the IMUs "
                                     f"{ctx.imu_names} (cfg.imu)")
        s, ns, r0 = ctx.imu_names.index(asset.name), len(ctx.imu_names), imus[func]
        k = 4 if func is SN.imu_orientation else 3
        return G, S["imu"], [(r0 + j) * ns + s for j in range(k)], zeros(k), zeros(k), 0
    if func is SN.image or func is OB.image_features or name in ("image", "image_features"):
        raise _unsupported(g, t, f"{name} is an image term (rank above 2): read the camera's data instead")
    if func is OB.body_incoming_wrench or name == "body_incoming_wrench":
        raise _unsupported(g, t, "body_incoming_wrench: the step keeps no joint reaction wrenches")
    raise _unsupported(g, t, f"func = {name!r} is not a served term function")


def _per_column(x, width: int, g: str, t: str, what: str) -> np.ndarray:
    """A noise parameter -- a float, or per-column values (tuple, array or tensor) -- as float32 [width]."""
    if is_number(x):
        return np.full(width, np.float32(x), np.float32)
    try:
        v = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise _unsupported(g, t, f"{what} = {x!r} is neither a float nor per-column values") from None
    if v.size not in (1, width):
        raise _unsupported(g, t, f"{what} has {v.size} values for a term of {width} columns")
    return np.broadcast_to(v, (width,)).astype(np.float32)


def _noise(cfg, width: int, g: str, t: str):
    f32 = np.float32
    z = np.zeros(width, f32)
    if cfg is None:
        return _native.NOISE_NONE, 0, z, z
    if isinstance(cfg, NZ.NoiseModelCfg):
        raise _unsupported(g, t, f"noise is a {type(cfg).__name__}: a noise model keeps per-env state; only the "
                                 f"stateless NoiseCfg terms are served here")
    func = getattr(cfg, "func", None)
    if func not in _NOISE:
        raise _unsupported(g, t, f"noise.func = {getattr(func, '__name__', func)!r} is not a built-in noise term")
    kind, (n0, n1) = _NOISE[func]
    op = getattr(cfg, "operation", None)
    if op not in _native.NOISE_OPS:
        raise _unsupported(g, t, f"noise.operation = {op!r}")
    x0 = getattr(cfg, n0)
    x1 = getattr(cfg, n1) if n1 else 0.0
    if kind == _native.NOISE_UNIFORM:  # w = n_max - n_min as torch forms it: in double for two floats
        if is_number(x0) and is_number(x1):
            w = np.full(width, f32(float(x1) - float(x0)), f32)
        else:
            w = _per_column(x1, width, g, t, "noise.n_max") - _per_column(x0, width, g, t, "noise.n_min")
        return kind, _native.NOISE_OPS[op], _per_column(x0, width, g, t, "noise.n_min"), w
    return (kind, _native.NOISE_OPS[op], _per_column(x0, width, g, t, f"noise.{n0}"),
            _per_column(x1, width, g, t, f"noise.{n1}"))


def parse_term(g: str, t: str, cfg, group_cfg, ctx: ObsContext) -> TermSpec:
    f32 = np.float32
    if cfg.func is OB.MISSING or not callable(cfg.func):
        raise _unsupported(g, t, f"func = {cfg.func!r} is not callable")
    if cfg.modifiers is not None:
        raise _unsupported(g, t, "modifiers are host callables; they are not served")
    if not isinstance(cfg.params, dict):
        raise _unsupported(g, t, f"params = {cfg.params!r} is not a dict")
    kind, source, rows, a, b, flags = _term_source(cfg.func, cfg.params, ctx, g, t)
    width = len(rows)
    enable = _get(group_cfg, "enable_corruption", False)
    nk, nop, p0, p1 = _noise(cfg.noise if enable else None, width, g, t)
    clip = None
    if cfg.clip:
        try:
            lo, hi = cfg.clip
            clip = (float(f32(lo)), float(f32(hi)))
        except (TypeError, ValueError):
            raise _unsupported(g, t, f"clip = {cfg.clip!r} is not a (lo, hi) pair") from None
    scale = np.ones(width, f32)
    if cfg.scale is not None:
        s = cfg.scale.tolist() if torch.is_tensor(cfg.scale) else cfg.scale
        if isinstance(s, list):
            s = tuple(s)
        if not isinstance(s, (float, int, tuple)) or isinstance(s, bool):
            raise TypeError(f"Scale for observation term '{t}' in group '{g}' is not of type float, int or tuple. "
                            f"Received: '{type(cfg.scale)}'.")
        if isinstance(s, tuple) and len(s) != width:
            raise ValueError(f"Scale for observation term '{t}' in group '{g}' does not match the dimensions of the "
                             f"observation. Expected: {width} but received: {len(s)}.")
        scale = np.broadcast_to(np.asarray(s, dtype=f32), (width,)).copy()  # torch.tensor(scale, dtype=torch.float)
    gh = _get(group_cfg, "history_length", None)
    hist = int(cfg.history_length if gh is None else gh)
    flatten = bool(cfg.flatten_history_dim if gh is None else _get(group_cfg, "flatten_history_dim", True))
    if hist < 0:
        raise _unsupported(g, t, f"history_length = {hist} is negative")
    concat = bool(_get(group_cfg, "concatenate_terms", True))
    if hist > 0 and not flatten and concat:
        raise _unsupported(g, t, "flatten_history_dim=False gives a term of rank 3, which concatenate_terms=True "
                                 "cannot join with terms of rank 2: set concatenate_terms=False")
    return TermSpec(t, cfg, kind, source, [int(r) for r in rows], a.astype(f32), b.astype(f32), nk, nop, p0, p1,
                    clip, scale, hist, flatten, flags)


def _get(cfg, key: str, default):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class GroupSpec:
    """One parsed group: its terms, the layout of its output and the device tables as host arrays."""

    def __init__(self, name: str, cfg, ctx: ObsContext):
        self.name, self.cfg = name, cfg
        self.concatenate = bool(_get(cfg, "concatenate_terms", True))
        self.terms = [parse_term(name, tname, tcfg, cfg, ctx)
                      for tname, tcfg in cfg_items(cfg, OB.ObservationTermCfg, ignore=OB.GROUP_SETTINGS)]
        if not self.terms:
            raise _unsupported(name, None, "the group has no terms")
        if len(self.terms) > _native.MAX_OBS_TERMS:
            raise _unsupported(name, None, f"{len(self.terms)} terms; a group takes at most AS_MAX_OBS_TERMS = "
                                           f"{_native.MAX_OBS_TERMS}")
        self.build()

    def build(self) -> None:
        """The descriptor rows, the column table and the output map from the term specs as they stand."""
        f32, i32 = np.float32, np.int32
        d0 = sum(t.width for t in self.terms)
        out_cols = sum(t.width * t.slots for t in self.terms)
        if d0 > _native.MAX_OBS_COLS or out_cols > _native.MAX_OBS_OUT_COLS:
            raise _unsupported(self.name, None, f"{d0} columns, {out_cols} with the history; a group takes at most "
                                                f"AS_MAX_OBS_COLS = {_native.MAX_OBS_COLS} and AS_MAX_OBS_OUT_COLS = "
                                                f"{_native.MAX_OBS_OUT_COLS}")
        rows = np.zeros((len(self.terms), _native.OBS_TERM_WORDS), f32)
        cols = np.zeros((_native.OBS_COL_ROWS, _native.MAX_OBS_COLS), f32)
        cols[5] = 1.0
        omap = np.zeros(out_cols, i32)
        self.term_col, self.term_out_col = [], []
        c = oc = 0
        for k, t in enumerate(self.terms):
            w, H = t.width, t.slots
            ints = rows[k].view(i32)
            ints[:9] = (t.kind, t.source, w, c, oc, H, t.noise_kind, t.noise_op, 0 if t.clip is None else 1)
            if t.clip is not None:
                rows[k, 9:11] = t.clip
            ints[11] = t.flags
            cols[0, c:c + w] = np.asarray(t.rows, i32).view(f32)
            cols[1, c:c + w], cols[2, c:c + w] = t.a, t.b
            cols[3, c:c + w], cols[4, c:c + w], cols[5, c:c + w] = t.p0, t.p1, t.scale
            for s in range(H):
                omap[oc + s * w: oc + (s + 1) * w] = (np.arange(c, c + w) | (int(s == H - 1) << 8) | (w << 9))
            self.term_col.append(c)
            self.term_out_col.append(oc)
            c += w
            oc += w * H
        self.d0, self.out_cols, self.rows, self.cols, self.omap = d0, out_cols, rows, cols, omap

    names = property(lambda self: [t.name for t in self.terms])
    term_dims = property(lambda self: [t.dims for t in self.terms])

    @property
    def dim(self):
        """group_obs_dim's entry: one tuple for a concatenated group, else the list of the terms' shapes."""
        return (self.out_cols,) if self.concatenate else self.term_dims

    def layout(self) -> list:
        return [(t.width, t.slots) for t in self.terms]

    def sources(self) -> set:
        used = {_native.OBS_SOURCES[t.source] for t in self.terms}
        if any(t.kind == _native.OBS_ROTATE_INVERSE for t in self.terms):
            used.add("root_quat")
        if any(t.kind == _native.OBS_HEIGHT_SCAN for t in self.terms):
            used.add("ray_pose")
        return used


def _not_a_group(name: str, cfg) -> TypeError:
    return TypeError(f"Observation group '{name}' is not of type 'ObservationGroupCfg'. Received: '{type(cfg)}'.")


class ObservationGroups:
    """The host side of cfg.observations: groups in cfg order, checked (no device needed)."""

    def __init__(self, observations, ctx: ObsContext):
        self.ctx = ctx
        self.groups: list[GroupSpec] = []
        for gname, gcfg in cfg_items(observations, (OB.ObservationGroupCfg, dict), error=_not_a_group):
            if gname == "policy":
                raise _unsupported(gname, None, "'policy' is the task's own observation, which stays as it is: give "
                                                "the group another name")
            self.groups.append(GroupSpec(gname, gcfg, ctx))
        if len(self.groups) > _native.MAX_OBS_GROUPS:
            raise _native.NativeError(f"cfg.observations has {len(self.groups)} groups ({self.names}); the observation "
                                      f"kernel takes at most AS_MAX_OBS_GROUPS = {_native.MAX_OBS_GROUPS}")

    names = property(lambda self: [g.name for g in self.groups])

    def group(self, name: str) -> GroupSpec:
        for g in self.groups:
            if g.name == name:
                return g
        raise ValueError(f"Unable to find the group '{name}' in the observation manager. Available groups are: "
                         f"{self.names}")

    def set_term(self, group_name: str, term_name: str, cfg) -> GroupSpec:
        g = self.group(group_name)
        if term_name not in g.names:
            raise ValueError(f"Observation term '{term_name}' not found in group '{group_name}'.")
        k = g.names.index(term_name)
        new = parse_term(group_name, term_name, cfg, g.cfg, self.ctx)
        old = g.terms[k]
        if (new.width, new.slots, new.dims) != (old.width, old.slots, old.dims):
            raise _unsupported(group_name, term_name, f"the new cfg changes the term's shape from {old.dims} to "
                                                      f"{new.dims}; the group's width is fixed at construction")
        g.terms[k] = new
        g.build()
        return g

    def table(self) -> str:
        """ObservationManager.__str__: one table per group, in the reference's form."""
        msg = f"<ObservationManager> contains {len(self.groups)} groups.\n"
        for g in self.groups:
            title = f"Active Observation Terms in Group: '{g.name}'"
            if g.concatenate:
                title += f" (shape: {g.dim})"
            rows = [(str(i), t.name, str(tuple(t.dims))) for i, t in enumerate(g.terms)]
            head = ("Index", "Name", "Shape")
            w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
            extra = len(title) - (sum(w) + 6)  # a title wider than the columns widens them, as PrettyTable does
            if extra > 0:
                for j in range(3):
                    w[j] += extra // 3 + (1 if j < extra % 3 else 0)
            line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
            total = len(line) - 3
            fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), r[2].center(w[2]))) + " |\n"  # noqa: E731
            msg += "+" + "-" * total + "+\n" + "|" + title.center(total) + "|\n"
            msg += line + "| " + " | ".join(h.center(x) for h, x in zip(head, w)) + " |\n" + line
            msg += "".join(fmt(r) for r in rows) + line
        return msg


class EnvObservations(DeviceState):
    """The observations side of a DirectRLEnv: per group the device tables, the output rows (which hold the
    history), the push counts and the stream counter."""

    STATE_PREFIX = "observation_"

    def __init__(self, cfg, env, n: int, device, seed: int):
        self.n, self.device, self.seed = n, device, int(seed)
        self._env = env
        self.spec = ObservationGroups(cfg.observations, env._observations_context())
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
        G = len(self.spec.groups)
        self.t = z(G, n, dtype=torch.int32)
        self.count = z(G, n, dtype=torch.int32)
        self.out = [z(n, g.out_cols) for g in self.spec.groups]
        self.desc = [torch.as_tensor(g.rows.copy(), device=device) for g in self.spec.groups]
        self.cols = [torch.as_tensor(g.cols.copy(), device=device) for g in self.spec.groups]
        self.omap = [torch.as_tensor(g.omap.copy(), device=device) for g in self.spec.groups]
        self._all = torch.ones(n, dtype=torch.uint8, device=device)
        self._find_sensors()
        self.buffer: dict | None = None  # the reference's _obs_buffer
        self.launches = 0

    def _find_sensors(self) -> None:
        """Which sensors the step brings up to date before the launch: those a term of any group reads, as the
        terms now stand (set_term_cfg may replace a term by one of the same shape on another source)."""
        used = set().union(*(g.sources() for g in self.spec.groups)) if self.spec.groups else set()
        self.needs_height_scan = "ray_hits" in used
        self.needs_imu = "imu" in used

    @staticmethod
    def wanted(cfg) -> bool:
        return getattr(cfg, "observations", None) is not None

    # ---- launches
    def _refresh_sensors(self) -> None:
        """Bring the sensors the terms read up to date: the launch that reading their data causes."""
        env = self._env
        if self.needs_height_scan:
            env.height_scanner.data  # noqa: B018  (launches when the scene changed since the last launch)
        if self.needs_imu:
            env._imus.refresh()

    def _result(self, k: int):
        g, out = self.spec.groups[k], self.out[k]
        if g.concatenate:
            return out
        res = {}
        for t, oc in zip(g.terms, g.term_out_col):
            v = out[:, oc:oc + t.width * t.slots]
            res[t.name] = v.unflatten(1, (t.slots, t.width)) if (t.history_length > 0 and not t.flatten) else v
        return res

    def launch_group(self, k: int, reset=None, reset2=None, draws=None):
        env, g = self._env, self.spec.groups[k]
        src = _native.make_observation_sources(env._observations_sources())
        _native.observations_step(self.desc[k], self.cols[k], self.omap[k], g.d0, g.out_cols, k, src, self.out[k],
                                  self.count[k], self.t[k], reset=reset, reset2=reset2, draws=draws, seed=self.seed,
                                  env_offset=env._noise_offset(), stream=env._noise_stream())
        self.launches += 1
        return self._result(k)

    def compute(self, reset=None, reset2=None) -> dict:
        """Every group, one launch each; the result is cached (``buffer``).  reset / reset2: the step's dones."""
        self._refresh_sensors()
        self.buffer = {g.name: self.launch_group(k, reset, reset2) for k, g in enumerate(self.spec.groups)}
        return self.buffer

    def compute_all_reset(self) -> dict:
        """``env.reset()``: every env counts as reset (its last action reads 0, its history fills)."""
        return self.compute(self._all, None)

    def reset(self, mask) -> None:
        """ObservationManager.reset(env_ids) for the envs of a uint8 / bool mask (None: all): no compute."""
        if mask is not None:
            mask = u8(mask.to(self.device).reshape(self.n))
        for k in range(len(self.spec.groups)):
            _native.observations_reset(self.out[k], self.count[k], mask=mask, stream=self._env._noise_stream())
            self.launches += 1

    def set_term_cfg(self, group_name: str, term_name: str, cfg) -> None:
        g = self.spec.set_term(group_name, term_name, cfg)
        k = self.spec.groups.index(g)
        self.desc[k].copy_(torch.as_tensor(g.rows.copy()))
        self.cols[k].copy_(torch.as_tensor(g.cols.copy()))
        self.omap[k].copy_(torch.as_tensor(g.omap.copy()))
        self._find_sensors()  # (a graph captured before keeps the sensor launches it was captured with)

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        d = {"observation_t": self.t, "observation_count": self.count}
        d.update({f"observation_history_{g.name}": self.out[k] for k, g in enumerate(self.spec.groups)})
        return d


class ObservationManagerView:
    """``env.observation_manager``: the caller-visible surface of the reference's ``ObservationManager``
    (observation_manager.py:106-335) over the device state."""

    def __init__(self, obs: EnvObservations):
        self._o = obs

    active_terms = property(lambda self: {g.name: g.names for g in self._o.spec.groups})
    group_obs_dim = property(lambda self: {g.name: g.dim for g in self._o.spec.groups})
    group_obs_term_dim = property(lambda self: {g.name: g.term_dims for g in self._o.spec.groups})
    group_obs_concatenate = property(lambda self: {g.name: g.concatenate for g in self._o.spec.groups})

    def get_term_cfg(self, group_name: str, term_name: str):
        g = self._o.spec.group(group_name)
        if term_name not in g.names:
            raise ValueError(f"Observation term '{term_name}' not found in group '{group_name}'.")
        return g.terms[g.names.index(term_name)].cfg

    def set_term_cfg(self, group_name: str, term_name: str, cfg) -> None:
        """Replace a term's cfg.  The new constants are written into the device tables, so they hold from the next
        launch on, in a captured graph too; a cfg that changes the term's shape is refused."""
        self._o.set_term_cfg(group_name, term_name, cfg)

    def compute(self) -> dict:
        """ObservationManager.compute: every group on the env's state as it stands -- one launch per group, a push
        into every history -- cached as the reference caches ``_obs_buffer``."""
        return self._o.compute()

    def compute_group(self, group_name: str):
        k = self._o.spec.groups.index(self._o.spec.group(group_name))
        self._o._refresh_sensors()
        return self._o.launch_group(k)

    def reset(self, env_ids=None) -> dict:
        """ObservationManager.reset(env_ids): the envs' histories are cleared; nothing to log."""
        mask = None
        if env_ids is not None:
            mask = torch.zeros(self._o.n, dtype=torch.uint8, device=self._o.device)
            mask[torch.as_tensor(env_ids, device=self._o.device).long()] = 1
        self._o.reset(mask)
        return {}

    def __str__(self) -> str:
        return self._o.spec.table()
