"""The articulation and contact-sensor surface of the native envs (``env.robot``, ``env.sensor*``): views of a
``NativeDirectEnv``'s SoA state and of its opt-in contact report, shared by the walker and the quadruped."""

from __future__ import annotations

import torch

from .. import _native
from ..model import joint_limits_cfg


class _RobotData:
    """The ``ArticulationData`` views (articulation_data.py:364-601).  Ring 1 -- what the task reads --
    as zero-copy (N, k) views of the SoA state (k-major storage, so rows are strided).  Ring 2 -- the
    body views of every MJCF body (``body_names``: the walker's 17, document order) -- computed on demand
    by the ``as_body_state`` HIP kernel (the step kernel's own FK of the state as it stands) each time one
    is read; the step never computes them (include/allsteps.h)."""

    def __init__(self, env, default_joint_pos: torch.Tensor | None = None, init_root_pos=None):
        """``default_joint_pos``: (nd,) -- the quadruped's stand pose; None: zero, the walker's.  ``init_root_pos``:
        the default root position, None: the origin."""
        self._env = env
        s = env.state
        n = env.num_envs
        self.joint_names = list(env.model["dof_names"])
        self.body_names = list(env.model["body_names"])
        self.num_bodies = len(self.body_names)
        self._body_table = _native.make_body_table(env.model)
        self._body_out = None
        nd = self._nd = int(env.model["num_hinges"])
        lim = torch.as_tensor(joint_limits_cfg(env.model), device=env._device)
        self.joint_pos_limits = lim.unsqueeze(0).expand(n, -1, -1)
        self.default_joint_pos = (torch.zeros(n, nd, device=env._device) if default_joint_pos is None
                                  else default_joint_pos.reshape(1, nd).expand(n, nd).clone())
        self.default_joint_vel = torch.zeros(n, nd, device=env._device)
        self.default_root_state = torch.zeros(n, 13, device=env._device)
        if init_root_pos is not None:
            self.default_root_state[:, :3] = torch.tensor(init_root_pos, device=env._device)
        self.default_root_state[:, 3] = 1.0
        self._s = s

    root_pos_w = property(lambda self: self._s["root_pos"].T)
    root_quat_w = property(lambda self: self._s["root_quat"].T)
    root_lin_vel_w = property(lambda self: self._s["root_lin"].T)
    root_ang_vel_w = property(lambda self: self._s["root_ang"].T)
    joint_pos = property(lambda self: self._s["q"][: self._nd].T)  # the state's rows past the model's hinges unused
    joint_vel = property(lambda self: self._s["qd"][: self._nd].T)
    # the soft limits the env keeps (the quadruped's, by its soft_joint_pos_limit_factor), else the hard ones
    soft_joint_pos_limits = property(lambda self: getattr(self._env, "soft_joint_pos_limits", self.joint_pos_limits))

    # The base-frame quantities of articulation_data.py -- torch expressions over the views, the reference's
    # quat_rotate_inverse / quat_apply (math.py:546-564, 606-625); the kernels compute the same from the same rows.
    @staticmethod
    def _rotate_inverse(q: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        q_w, q_vec = q[..., 0], q[..., 1:]
        a = v * (2.0 * q_w**2 - 1.0).unsqueeze(-1)
        b = torch.cross(q_vec, v, dim=-1) * q_w.unsqueeze(-1) * 2.0
        c = q_vec * torch.bmm(q_vec.reshape(q.shape[0], 1, 3), v.reshape(q.shape[0], 3, 1)).squeeze(-1) * 2.0
        return a - b + c

    @property
    def root_lin_vel_b(self) -> torch.Tensor:
        return self._rotate_inverse(self.root_quat_w, self.root_lin_vel_w)

    @property
    def root_ang_vel_b(self) -> torch.Tensor:
        return self._rotate_inverse(self.root_quat_w, self.root_ang_vel_w)

    @property
    def projected_gravity_b(self) -> torch.Tensor:
        g = torch.tensor((0.0, 0.0, -1.0), device=self._s["root_quat"].device).repeat(self._s["root_quat"].shape[1], 1)
        return self._rotate_inverse(self.root_quat_w, g)

    @property
    def heading_w(self) -> torch.Tensor:
        q = self.root_quat_w
        v = torch.tensor((1.0, 0.0, 0.0), device=q.device).repeat(q.shape[0], 1)
        xyz = q[:, 1:]
        t = xyz.cross(v, dim=-1) * 2
        fwd = v + q[:, 0:1] * t + xyz.cross(t, dim=-1)
        return torch.atan2(fwd[:, 1], fwd[:, 0])

    @property
    def joint_acc(self) -> torch.Tensor:
        """(N, nd) joint accelerations: the last physics substep's finite difference (joint_vel - the velocity
        at that substep's start) / sim.dt (articulation_data.py:78-83, 547-556), from the contact report's
        qd_prev -- cfg.contact_forces only.  An env the step reset shows its reset velocity against the old one."""
        rep = self._env._report_or_raise("robot.data.joint_acc")
        return (self.joint_vel - rep.qd_prev[: self._nd].T) / self._env.cfg.sim.dt

    @property
    def root_state_w(self) -> torch.Tensor:
        s = self._s
        return torch.cat([s["root_pos"], s["root_quat"], s["root_lin"], s["root_ang"]], 0).T.contiguous()

    def _bodies(self) -> torch.Tensor:
        """(16, B, N) as_body_state rows of the current state: pos 3 | quat 4 | frame lin vel 3 | ang vel 3 |
        COM lin vel 3 (one launch on the env's stream)."""
        env = self._env
        if self._body_out is None:
            self._body_out = torch.empty(_native.BODY_STATE_ROWS, self.num_bodies, env.num_envs, device=env._device)
        env._native.body_state(self._body_table, self._body_out, stream=env._stream())
        return self._body_out

    def _rows(self, lo: int, hi: int) -> torch.Tensor:
        return self._bodies()[lo:hi].permute(2, 1, 0).contiguous()

    @property
    def body_pos_w(self) -> torch.Tensor:
        """(N, B, 3) body (link-frame) positions, all bodies; rows torso / right_foot / left_foot equal the
        state's body_pos (the step's FK after the last substep) bit for bit."""
        return self._rows(0, 3)

    @property
    def body_quat_w(self) -> torch.Tensor:
        """(N, B, 4) body orientations (w, x, y, z)."""
        return self._rows(3, 7)

    @property
    def body_lin_vel_w(self) -> torch.Tensor:
        """(N, B, 3) linear velocities of the bodies' centres of mass (PhysX link velocities)."""
        return self._rows(13, 16)

    @property
    def body_ang_vel_w(self) -> torch.Tensor:
        return self._rows(10, 13)

    @property
    def body_state_w(self) -> torch.Tensor:
        """(N, B, 13) [pos, quat, lin_vel, ang_vel]: link-frame pose, centre-of-mass velocity
        (articulation_data.py:430-447)."""
        b = self._bodies()
        return torch.cat([b[0:7], b[13:16], b[10:13]], 0).permute(2, 1, 0).contiguous()

    @property
    def body_link_state_w(self) -> torch.Tensor:
        """(N, B, 13) link-frame pose and the link frame's own velocity (articulation_data.py:449-470)."""
        return self._rows(0, 13)

    @property
    def body_link_pos_w(self) -> torch.Tensor:
        return self._rows(0, 3)

    @property
    def body_link_vel_w(self) -> torch.Tensor:
        return self._rows(7, 13)

    @property
    def body_com_pos_w(self) -> torch.Tensor:
        """(N, B, 3) the bodies' own centres of mass (as_body_table_t.com, from the MJCF geoms)."""
        b = self._bodies()
        q = b[3:7].permute(2, 1, 0)
        com = torch.as_tensor(self._env.model["body_com"][: self.num_bodies], device=b.device)
        w, v = q[..., :1], q[..., 1:]
        c = com.expand_as(v)
        t = 2.0 * torch.linalg.cross(v, c, dim=-1)
        return b[0:3].permute(2, 1, 0) + c + w * t + torch.linalg.cross(v, t, dim=-1)


class _SensorData:
    def __init__(self, sensor: "_FootSensor"):
        self._sensor = sensor

    @property
    def force_matrix_w(self) -> torch.Tensor | None:
        """(N, B, 20, 3) FLAG-VALUED force matrix of the stones (filter_prim_paths_expr = the 20 steps):
        (0, 0, 1) N where the foot pushed on that stone with |F| > 1e-4 N in the env step's last
        substep (contact_sensor.py:341 with the contact solve's impulse / dt), 0 elsewhere.  The force
        itself is not kept by the step (only the flag the task reads: allsteps_env.py:421-425 tests
        ``vector_norm(force_matrix_w) > EPSILON``, which this view answers exactly).  None for the
        unfiltered two-foot sensor, as in the reference.

        With ``cfg.contact_forces`` the real thing: the normal contact force (N, world frame) of each stone on
        each foot in the env step's last substep, the contact report's impulses / sim.dt summed per (foot,
        stone) by ``as_contact_forces`` -- the sum whose norm the step tested for the flag."""
        return self._sensor._force_matrix()

    @property
    def net_forces_w(self) -> torch.Tensor:
        """(N, B, 3) net normal contact force on each sensor body in the last substep (contact_sensor.py:329-335):
        stones and self-contacts.  ``cfg.contact_forces`` only; without it the step keeps no forces."""
        return self._sensor._net_forces()[:, 0]

    @property
    def net_forces_w_history(self) -> torch.Tensor:
        """(N, T, B, 3) net forces of the env step's last T = decimation substeps, index 0 the latest (the
        reference's history_length = 4 at one sensor update per physics step)."""
        return self._sensor._net_forces()

    # ``cfg.contact_air_time`` (the reference's track_air_time, contact_sensor_data.py:68-101): (N, B) zero-copy
    # views of the env's one set of timers, which k_contact_timers advances by `decimation` sensor updates in
    # every ``env.step``; None when the feature is off, as in the reference
    @property
    def current_air_time(self) -> torch.Tensor | None:
        """(N, B) time (s) spent in the air since the last detach."""
        return self._sensor._timer(0)

    @property
    def last_air_time(self) -> torch.Tensor | None:
        """(N, B) time (s) spent in the air before the last contact."""
        return self._sensor._timer(1)

    @property
    def current_contact_time(self) -> torch.Tensor | None:
        """(N, B) time (s) spent in contact since the last contact."""
        return self._sensor._timer(2)

    @property
    def last_contact_time(self) -> torch.Tensor | None:
        """(N, B) time (s) spent in contact before the last detach."""
        return self._sensor._timer(3)


class _FootSensor:
    """The reference's foot ContactSensors (allsteps_env_cfg.py:119-130; contact_sensor.py:320-343):
    ``sensor_right`` / ``sensor_left`` (one foot, filtered by the 20 stones) and ``sensor`` (both feet,
    unfiltered), over the state's per-foot stone bitmasks (contact_mask)."""

    def __init__(self, env, feet: list, names: list, filtered: bool):
        self._env, self._feet, self._filtered = env, feet, filtered
        self.body_names = list(names)
        self.num_bodies = len(feet)
        self.data = _SensorData(self)

    def _force_matrix(self):
        if not self._filtered:
            return None
        env = self._env
        ns = env.cfg.num_steps
        if env._report is not None:
            fm, _ = env._report.forces()  # (T, 4, 20, 3, N) impulses
            return fm[0, self._feet, :ns].permute(3, 0, 1, 2) / env.cfg.sim.dt
        m = env._contact_masks()  # (feet, N) int32, bit s = stone s
        bits = torch.arange(ns, device=m.device, dtype=torch.int32)
        f = torch.zeros(env.num_envs, self.num_bodies, ns, 3, device=m.device)
        for k, foot in enumerate(self._feet):
            f[:, k, :, 2] = ((m[foot].unsqueeze(1) >> bits) & 1).float()
        return f

    def _net_forces(self) -> torch.Tensor:
        """(N, T, B, 3) net contact forces of the sensor's bodies over the stored substeps."""
        rep = self._env._report_or_raise("ContactSensor.data.net_forces_w")
        _, net = rep.forces()  # (T, bodies, 3, N) impulses
        return net[:, [rep.foot_body[f] for f in self._feet]].permute(3, 0, 1, 2) / self._env.cfg.sim.dt

    def _timer(self, row: int) -> torch.Tensor | None:
        """(N, B) view of timer `row` of this sensor's bodies (its feet are consecutive in sensor order)."""
        tm = self._env._contact_timers
        return None if tm is None else tm.timers[row, self._feet[0]: self._feet[-1] + 1].T

    def _timers_or_raise(self) -> None:
        # the reference's message (contact_sensor.py:201-205, 236-240); its track_air_time is cfg.contact_air_time
        if self._env._contact_timers is None:
            raise RuntimeError("The contact sensor is not configured to track contact time."
                               "Please enable the 'track_air_time' in the sensor configuration.")

    def compute_first_contact(self, dt: float, abs_tol: float = 1.0e-8) -> torch.Tensor:
        """(N, B) bool: the bodies that established contact within the last ``dt`` seconds
        (contact_sensor.py:175-209).  ``cfg.contact_air_time`` only."""
        self._timers_or_raise()
        currently_in_contact = self.data.current_contact_time > 0.0
        less_than_dt_in_contact = self.data.current_contact_time < (dt + abs_tol)
        return currently_in_contact * less_than_dt_in_contact

    def compute_first_air(self, dt: float, abs_tol: float = 1.0e-8) -> torch.Tensor:
        """(N, B) bool: the bodies that broke contact within the last ``dt`` seconds (contact_sensor.py:211-244).
        ``cfg.contact_air_time`` only."""
        self._timers_or_raise()
        currently_detached = self.data.current_air_time > 0.0
        less_than_dt_detached = self.data.current_air_time < (dt + abs_tol)
        return currently_detached * less_than_dt_detached


class _ContactReport:
    """The opt-in contact report of an env (``cfg.contact_forces``; include/allsteps.h ABI 6): the device buffers
    k_step fills for the last ``depth`` substeps of every step, and the dense sums ``as_contact_forces`` makes of
    them, launched on the env's stream at most once per step however many views are read."""

    def __init__(self, env, depth: int):
        n, dev = env.num_envs, env._device
        self._env, self.depth = env, depth
        self.count = torch.zeros(depth, n, dtype=torch.int32, device=dev)
        self.records = torch.zeros(depth, _native.REPORT_WORDS, _native.MAXC, n, dtype=torch.int32, device=dev)
        self.qd_prev = torch.zeros(21, n, dtype=torch.float32, device=dev)
        env._native.set_contact_report(depth, self.count, self.records, self.qd_prev)
        m = env.model
        self._table = _native.make_body_table(m)
        nb, ng = int(m["num_bodies"]), int(m["num_geoms"])
        body_link = [int(x) for x in m["body_link"][:nb]]
        # sensor foot -> the body its geoms' link carries
        self.foot_body = {int(m["geom_foot"][g]): body_link.index(int(m["geom_link"][g])) for g in range(ng)
                          if int(m["geom_foot"][g]) >= 0}
        self._matrix = torch.empty(depth, _native.REPORT_FEET, _native.NUM_STONES, 3, n, device=dev)
        self._net = torch.empty(depth, nb, 3, n, device=dev)
        self._stamp = None

    def forces(self):
        """(force matrix (T, 4, 20, 3, N), net (T, bodies, 3, N)) impulses in N s of the last step."""
        env = self._env
        stamp = (env.common_step_counter, env._sim_step_counter, env._launches)
        if stamp != self._stamp:
            env._native.contact_forces(self._table, self._matrix, self._net, stream=env._stream())
            self._stamp = stamp
        return self._matrix, self._net


class _ContactSensorData:
    def __init__(self, sensor: "_ContactSensor"):
        self._sensor = sensor

    @property
    def net_forces_w_history(self) -> torch.Tensor:
        """(N, T, B, 3) net normal contact force on every body of the robot over the env step's last T = decimation
        substeps, index 0 the latest: the contact report's net impulses / sim.dt, as the foot sensors form theirs."""
        return self._sensor._report.forces()[1].permute(3, 0, 1, 2) / self._sensor._env.cfg.sim.dt

    @property
    def net_forces_w(self) -> torch.Tensor:
        """(N, B, 3) the net forces of the last substep."""
        return self.net_forces_w_history[:, 0]


class _ContactSensor:
    """``env.scene.sensors["contact_forces"]`` of an env with ``cfg.contact_forces``: a contact sensor over every
    body of the robot (``body_names``: the articulation's, in its order), the view the velocity task's
    ``illegal_contact`` on the base reads.  It is built over the contact report's dense net impulses
    (``_ContactReport.forces()[1]``, one launch per step however many views read it) and launches nothing itself."""

    def __init__(self, env, report: "_ContactReport"):
        self._env, self._report = env, report
        self.body_names = list(env.model["body_names"])[: int(env.model["num_bodies"])]
        self.num_bodies = len(self.body_names)
        self.data = _ContactSensorData(self)

    def find_bodies(self, name_keys, preserve_order: bool = False):
        """(indices, names) of the bodies whose whole name matches one of the regular expressions ``name_keys`` (a
        string or a list), in body order, or in the order of the keys with ``preserve_order``
        (contact_sensor.py ``find_bodies``); a key that matches nothing is a ValueError."""
        import re

        keys = [name_keys] if isinstance(name_keys, str) else list(name_keys)
        hit = [[k for k, bn in enumerate(self.body_names) if re.fullmatch(p, bn)] for p in keys]
        missing = [p for p, h in zip(keys, hit) if not h]
        if missing:
            raise ValueError(f"find_bodies: {missing} match no body of {self.body_names}")
        flat = [k for h in hit for k in h]
        ids = list(dict.fromkeys(flat)) if preserve_order else sorted(set(flat))
        return ids, [self.body_names[k] for k in ids]


class _ContactTimers:
    """The air / contact timers of an env (``cfg.contact_air_time``; the reference's ContactSensor with
    track_air_time = True, contact_sensor.py:351-379): device state of ``as_contact_timers`` over the env's contact
    report.  One set serves every sensor of the env: body k is sensor foot k (walker: right, left; quadruped: RF,
    LF, RH, LH).  ``update`` runs after every ``env.step`` (``decimation`` sensor updates, then the reset of the
    envs the step reset), ``reset`` in the env's reset paths; both are one launch on the env's stream."""

    STATE_KEYS = ("contact_timers", "contact_timestamp")

    def __init__(self, env, report: _ContactReport, force_threshold: float):
        n, dev = env.num_envs, env._device
        self._env, self._depth = env, report.depth
        self.force_threshold = float(force_threshold)
        feet = sorted(report.foot_body)
        if feet != list(range(len(feet))):
            raise _native.NativeError(f"contact_air_time: the model's sensor feet {feet} are not 0 .. {len(feet) - 1}")
        body_link = [int(x) for x in env.model["body_link"]]
        self._table = _native.AsBodyTable()
        self._table.num_bodies = len(feet)
        for f in feet:
            self._table.link[f] = body_link[report.foot_body[f]]
        self.num_bodies = len(feet)
        self.timers = torch.zeros(_native.TIMER_ROWS, len(feet), n, dtype=torch.float32, device=dev)
        self.timestamp = torch.zeros(n, dtype=torch.float32, device=dev)

    def update(self, terminated: torch.Tensor, truncated: torch.Tensor) -> None:
        env = self._env
        env._native.contact_timers(self._table, self.timers, self.timestamp, self.force_threshold, self._depth,
                                   terminated, truncated, stream=env._stream())

    def reset(self, mask: torch.Tensor | None) -> None:
        """ContactSensor.reset(env_ids) for the envs of a uint8 / bool mask (None: all)."""
        env = self._env
        env._native.contact_timers(self._table, self.timers, self.timestamp, self.force_threshold, 0, mask, None,
                                   stream=env._stream())

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {"contact_timers": self.timers, "contact_timestamp": self.timestamp}

    def get_state(self) -> dict:
        return {k: v.clone() for k, v in self.tensors().items()}

    def set_state(self, state: dict) -> None:
        for k, v in self.tensors().items():
            if k in state:
                v.copy_(torch.as_tensor(state[k]).to(v.device, v.dtype).reshape(v.shape))


class _RayCasterData:
    """``RayCasterData`` (ray_caster_data.py): zero-copy strided views of the sensor's env-minor device buffers, as
    the last launch left them."""

    def __init__(self, sensor: "_RayCaster"):
        self._s = sensor

    ray_hits_w = property(lambda self: self._s.hits.permute(2, 1, 0))  # (N, R, 3), env-local frame; +inf: a miss
    pos_w = property(lambda self: self._s.pose[:3].T)  # (N, 3) the root position the rays were cast from
    quat_w = property(lambda self: self._s.pose[3:].T)  # (N, 4) (w, x, y, z)
    # extension: (N, R) int8, the stone hit, -1 the ground, -2 a miss
    ray_hit_surface = property(lambda self: self._s.surface.T)


class _RayCaster:
    """The ray-caster height scanner of an env (``cfg.height_scanner``; the reference's ``RayCaster``,
    ray_caster.py:201-260, attached to the robot's root body): the local rays of the cfg's pattern and the device
    buffers of ``as_ray_cast``, which casts them from every env's root frame against the ground plane and the env's
    stones as they stand.  Lazy like the reference's sensors: reading ``data`` launches only when the env has marked
    the scene changed since the last launch (``mark_dirty``: step, graph-replay accounting, every reset path,
    set_state, the robot view's writers, stone regeneration); ``update(force_recompute=True)`` always launches, on
    the env's current stream -- the call to put inside a captured graph.  The sensor carries no state and draws
    nothing: no get_state keys, nothing to reset."""

    def __init__(self, env, cfg):
        from .ray_caster import RayCasterSpec

        n, dev = env.num_envs, env._device
        root = list(env.model["body_names"])[0]
        spec = RayCasterSpec(cfg, root_body=root, step_dt=env.step_dt,
                             step_paths=tuple(getattr(env.cfg, "step_paths", ()) or ()))
        self._env, self.cfg, self._spec = env, cfg, spec
        self._native_cfg = spec.native_cfg()
        self.num_rays = spec.num_rays
        self.rays = spec.rays.to(dev)  # (6, R): a device tensor, so a captured graph sees later edits
        self.hits = torch.zeros(3, self.num_rays, n, dtype=torch.float32, device=dev)
        self.surface = torch.full((self.num_rays, n), _native.RAY_MISS, dtype=torch.int8, device=dev)
        self.pose = torch.zeros(7, n, dtype=torch.float32, device=dev)
        self._data = _RayCasterData(self)
        self._dirty = True
        self.launches = 0  # as_ray_cast launches so far

    def __str__(self) -> str:
        n, surfaces = self._env.num_envs, self._spec.surface_names()
        return (f"Ray-caster @ '{self.cfg.prim_path}': \n"
                f"\tview type            : {_RobotView}\n"
                f"\tupdate period (s)    : {self.cfg.update_period}\n"
                f"\tnumber of meshes     : {len(surfaces)} ({', '.join(surfaces)})\n"
                f"\tnumber of sensors    : {n}\n"
                f"\tnumber of rays/sensor: {self.num_rays}\n"
                f"\ttotal number of rays : {self.num_rays * n}")

    num_instances = property(lambda self: self._env.num_envs)
    device = property(lambda self: self._env.device)

    def mark_dirty(self) -> None:
        self._dirty = True

    def _launch(self) -> None:
        env = self._env
        env._native.ray_cast(self._native_cfg, self.rays, self.hits, self.surface, self.pose, stream=env._stream())
        self.launches += 1
        self._dirty = False

    @property
    def data(self) -> _RayCasterData:
        if self._dirty:
            self._launch()
        return self._data

    def update(self, dt: float = 0.0, force_recompute: bool = False) -> None:
        """SensorBase.update: with ``force_recompute`` one launch now; otherwise the next read of ``data`` decides."""
        if force_recompute:
            self._launch()

    def reset(self, env_ids=None) -> None:
        """SensorBase.reset: nothing is kept per env but the outdated flag."""
        self._dirty = True


class _CameraData:
    """``CameraData`` (camera_data.py) of a ray-cast camera: views of the sensor's device buffers, as the last launch
    left them.  Positions are env-local, like every other view here (envs/scene.py)."""

    def __init__(self, sensor: "_RayCasterCamera"):
        self._s = sensor
        self.image_shape = sensor.image_shape
        h, w = sensor.image_shape
        # (N, H, W, C): zero-copy views of the env-major buffers
        self.output = {name: buf.view(-1, h, w, 3 if name == "normals" else 1) for name, buf in sensor.images.items()}
        self.info = [{name: None for name in sensor.images}] * sensor.num_instances

    pos_w = property(lambda self: self._s.pose[:3].T)  # (N, 3) the camera's position
    quat_w_world = property(lambda self: self._s.pose[3:].T)  # (N, 4) (w, x, y, z), forward +X, up +Z
    intrinsic_matrices = property(lambda self: self._s.intrinsic_matrices)  # (N, 3, 3)

    @property
    def quat_w_ros(self) -> torch.Tensor:
        """(N, 4) the orientation in the ROS convention (forward +Z, up -Y): torch on the device."""
        from .ray_camera import quat_from_world_torch

        return quat_from_world_torch(self.quat_w_world, "ros")

    @property
    def quat_w_opengl(self) -> torch.Tensor:
        """(N, 4) the orientation in the OpenGL / USD convention (forward -Z, up +Y): torch on the device."""
        from .ray_camera import quat_from_world_torch

        return quat_from_world_torch(self.quat_w_world, "opengl")


class _RayCasterCamera:
    """A ray-cast depth camera of an env (``cfg.camera``; the reference's ``RayCasterCamera``,
    ray_caster_camera.py, attached to the robot's root body): the pixels' local directions, the per-env offsets and
    the device buffers of ``as_ray_camera``, which casts them from every env's camera pose against the ground plane
    and the env's stones as they stand and writes the requested images env-major.  Lazy like the height scanner:
    reading ``data`` launches only when the env has marked the scene changed since the last launch (``mark_dirty``:
    step, graph-replay accounting, every reset path, set_state, the robot view's writers, stone regeneration) or
    the camera itself was moved or re-focused; ``update(force_recompute=True)`` always launches, on the env's
    current stream -- the call to put inside a captured graph.  No get_state keys: the images are a function of the
    state, the offsets and intrinsics are configuration.

    ``frame`` counts launches per env and ``reset(env_ids)`` zeroes it for those envs.  One deviation from the
    reference: after a masked reset that follows a read in the same step the reference recomputes and counts only
    the reset envs; here every env is recomputed (the same state gives the same bits) and every env's count moves."""

    def __init__(self, env, cfg, name: str = "camera"):
        from .ray_camera import RayCameraSpec

        n, dev = env.num_envs, env._device
        root = list(env.model["body_names"])[0]
        spec = RayCameraSpec(cfg, root_body=root, step_dt=env.step_dt,
                             step_paths=tuple(getattr(env.cfg, "step_paths", ()) or ()), name=name)
        self._env, self.cfg, self._spec, self.name = env, cfg, spec, name
        self._native_cfg = spec.native_cfg()
        self.num_rays = R = spec.num_rays
        self.image_shape = (spec.height, spec.width)
        # device tensors, so a captured graph sees later set_world_poses / set_intrinsic_matrices edits
        self.dirs = torch.from_numpy(spec.dirs).to(dev)  # (3, R)
        self.offset = torch.from_numpy(spec.offset).to(dev).reshape(7, 1).repeat(1, n).contiguous()  # (7, N)
        self.intrinsic_matrices = torch.from_numpy(spec.intrinsics).to(dev).repeat(n, 1, 1)  # (N, 3, 3)
        self.pose = torch.zeros(7, n, dtype=torch.float32, device=dev)
        self.images = {t: torch.zeros(n, R, 3 if t == "normals" else 1, dtype=torch.float32, device=dev)
                       for t in spec.data_types}
        self.frame = torch.zeros(n, dtype=torch.long, device=dev)
        self._ALL_INDICES = torch.arange(n, dtype=torch.long, device=dev)
        self._focal_length = spec.pattern.focal_length
        self._data = _CameraData(self)
        self._dirty = True
        self.launches = 0  # as_ray_camera launches so far

    def __str__(self) -> str:
        n, surfaces = self._env.num_envs, self._spec.surface_names()
        return (f"Ray-Caster-Camera @ '{self.cfg.prim_path}': \n"
                f"\tview type            : {_RobotView}\n"
                f"\tupdate period (s)    : {self.cfg.update_period}\n"
                f"\tnumber of meshes     : {len(surfaces)} ({', '.join(surfaces)})\n"
                f"\tnumber of sensors    : {n}\n"
                f"\tnumber of rays/sensor: {self.num_rays}\n"
                f"\ttotal number of rays : {self.num_rays * n}\n"
                f"\timage shape          : {self.image_shape}")

    num_instances = property(lambda self: self._env.num_envs)
    device = property(lambda self: self._env.device)

    def mark_dirty(self) -> None:
        self._dirty = True

    def _launch(self) -> None:
        env, im = self._env, self.images
        env._native.ray_camera(self._native_cfg, self.dirs, self.offset, self.pose, im.get("distance_to_image_plane"),
                               im.get("distance_to_camera"), im.get("normals"), stream=env._stream())
        self.frame += 1  # on the current stream as well: capturable
        self.launches += 1
        self._dirty = False

    @property
    def data(self) -> _CameraData:
        if self._dirty:
            self._launch()
        return self._data

    def update(self, dt: float = 0.0, force_recompute: bool = False) -> None:
        """SensorBase.update: with ``force_recompute`` one launch now; otherwise the next read of ``data`` decides."""
        if force_recompute:
            self._launch()

    def reset(self, env_ids=None) -> None:
        """RayCasterCamera.reset (ray_caster_camera.py:142-154): the frame count of the envs becomes zero and the
        sensor outdated; the pose rows are rewritten by the next launch, before they can be read."""
        if env_ids is None:
            self.frame.zero_()
        else:
            ids = torch.as_tensor(env_ids, device=self.frame.device)
            if ids.dtype == torch.bool:
                self.frame.masked_fill_(ids, 0)
            else:
                self.frame[ids.long()] = 0
        self._dirty = True

    def set_intrinsic_matrices(self, matrices: torch.Tensor, focal_length: float = 1.0, env_ids=None) -> None:
        """ray_caster_camera.py:121-140, for all envs at once with equal matrices -- the kernel takes one table of
        directions: ``matrices`` is (3, 3) or (N, 3, 3) with N equal rows.  Rewrites the device directions in
        place."""
        m = torch.as_tensor(matrices, dtype=torch.float32).detach().cpu()
        n = self._env.num_envs
        if env_ids is not None and sorted(int(i) for i in torch.as_tensor(env_ids).reshape(-1).tolist()) \
                != list(range(n)):
            raise _native.NativeError("camera.set_intrinsic_matrices: env_ids selects some of the envs; per-env "
                                      "intrinsics are not served (one HIP launch takes one table of ray directions)")
        if m.shape == (3, 3):
            m = m.reshape(1, 3, 3)
        if m.ndim != 3 or m.shape[1:] != (3, 3) or m.shape[0] not in (1, n) or bool((m != m[:1]).any()):
            raise _native.NativeError(f"camera.set_intrinsic_matrices: matrices of shape {tuple(m.shape)} are not one "
                                      f"(3, 3) matrix or ({n}, 3, 3) equal ones; per-env intrinsics are not served "
                                      f"(one HIP launch takes one table of ray directions)")
        dirs = self._spec.directions(m[0].numpy())
        self.dirs.copy_(torch.from_numpy(dirs))
        self.intrinsic_matrices.copy_(m[:1].to(self.intrinsic_matrices.device).expand(n, 3, 3))
        self._focal_length = focal_length
        self._dirty = True

    def set_world_poses(self, positions=None, orientations=None, env_ids=None, convention: str = "ros") -> None:
        """ray_caster_camera.py:156-206: place the cameras of ``env_ids`` in the world (env-local frame) by rewriting
        their offsets against the root poses as they stand; torch on the device."""
        from .ray_camera import world_pose_offsets

        dev = self.offset.device
        ids = self._ALL_INDICES if env_ids is None else torch.as_tensor(env_ids, device=dev).long()
        s = self._env.state
        f32 = lambda t: None if t is None else torch.as_tensor(t, dtype=torch.float32, device=dev)  # noqa: E731
        off_pos, off_quat = world_pose_offsets(s["root_pos"][:, ids].T, s["root_quat"][:, ids].T, f32(positions),
                                               f32(orientations), convention)
        if off_pos is not None:
            self.offset[:3, ids] = off_pos.T
        if off_quat is not None:
            self.offset[3:, ids] = off_quat.T
        self._dirty = True

    def set_world_poses_from_view(self, eyes, targets, env_ids=None) -> None:
        raise NotImplementedError("camera.set_world_poses_from_view is not served: build the orientation and call "
                                  "set_world_poses")


class _ImuData:
    """``ImuData`` (imu_data.py) of one sensor: zero-copy strided views of the env-minor device buffer, as the last
    launch left them.  Positions are env-local, like every other view here (envs/scene.py)."""

    def __init__(self, group: "_ImuSet", s: int):
        self._g, self._i = group, s

    pos_w = property(lambda self: self._g.data[0:3, self._i].T)  # (N, 3)
    quat_w = property(lambda self: self._g.data[3:7, self._i].T)  # (N, 4) (w, x, y, z)
    lin_vel_b = property(lambda self: self._g.data[7:10, self._i].T)  # (N, 3) sensor frame
    ang_vel_b = property(lambda self: self._g.data[10:13, self._i].T)
    lin_acc_b = property(lambda self: self._g.data[13:16, self._i].T)
    ang_acc_b = property(lambda self: self._g.data[16:19, self._i].T)


class _Imu:
    """One IMU of an env (the reference's ``Imu``, imu.py): sensor ``index`` of the env's ``_ImuSet``, which owns
    the buffers and the launch."""

    STATE_KEYS = ("imu_prev_lin_vel", "imu_prev_ang_vel")

    def __init__(self, group: "_ImuSet", index: int, name: str, cfg):
        self._g, self.index, self.name, self.cfg = group, index, name, cfg
        self._data = _ImuData(group, index)

    def __str__(self) -> str:
        return (f"Imu sensor @ '{self.cfg.prim_path}': \n"
                f"\tview type         : {_RobotView}\n"
                f"\tupdate period (s) : {self.cfg.update_period}\n"
                f"\tnumber of sensors : {self.num_instances}\n")

    num_instances = property(lambda self: self._g._env.num_envs)
    device = property(lambda self: self._g._env.device)
    launches = property(lambda self: self._g.launches)  # as_imu launches so far (one serves all the env's IMUs)

    @property
    def data(self) -> _ImuData:
        """The sensor's buffers, after one launch if an env is outdated (every env after ``env.step``, graph-replay
        accounting, ``env.reset()`` and ``set_state``; the envs of a masked reset); a second read launches nothing.
        The accelerations are the change of velocity since the env's previous update over ``dt`` -- the ``dt`` of
        the last ``update(dt)``, which ``env.step`` sets to ``physics_dt`` as the reference's does.  So a sensor read
        once per env step reports the velocity change of the whole env step over ONE physics step: ``decimation``
        times the step's mean acceleration.  That is the reference's behaviour for this task;
        ``env.imu.update(env.step_dt, force_recompute=True)`` after each step gives the mean acceleration."""
        self._g.refresh()
        return self._data

    def update(self, dt: float, force_recompute: bool = False) -> None:
        """Imu.update (imu.py:105-109): ``dt`` becomes the divisor of the next updates (of all the env's IMUs: they
        share the launch); with ``force_recompute`` one launch now, on the env's current stream -- the call to put
        inside a captured graph -- which recomputes exactly the outdated envs.  Otherwise the next read decides."""
        self._g.update(dt, force_recompute)

    def reset(self, env_ids=None) -> None:
        """Imu.reset(env_ids) (imu.py:92-103): the envs become outdated (None: all).  The previous velocities are
        not cleared, as in the reference; the outdated flag is the env's, shared by its IMUs."""
        self._g.reset(env_ids)


class _ImuSet:
    """The IMUs of an env (``cfg.imu``): the device buffers of ``as_imu`` (csrc/allsteps_imu.h) and the one launch
    that serves every sensor.  ``outdated`` is the reference's per-env ``_is_outdated`` on the device; "every env"
    is a host flag that the launch passes by value (``all``), so marking all envs launches nothing."""

    STATE_KEYS = _Imu.STATE_KEYS

    def __init__(self, env, cfg):
        from .imu import ImuSpec

        n, dev = env.num_envs, env._device
        spec = ImuSpec(cfg, model=env.model, step_dt=env.step_dt)
        self._env, self._spec = env, spec
        self._table = spec.table()
        S = self.num_sensors = spec.num_sensors
        self.data = torch.zeros(_native.IMU_DATA_ROWS, S, n, dtype=torch.float32, device=dev)
        self.data[3] = 1.0  # quat_w = identity before the first update (imu.py:188-189)
        self.prev = torch.zeros(_native.IMU_PREV_ROWS, S, n, dtype=torch.float32, device=dev)
        self.outdated = torch.ones(n, dtype=torch.uint8, device=dev)
        self.dt = float(env.physics_dt)  # the reference's self._dt: set before the first read (imu.py:145)
        self._all = self._dirty = True
        self.launches = 0
        self.sensors = {name: _Imu(self, s, name, c) for s, (name, c) in enumerate(zip(spec.names, spec.cfgs))}

    def mark_all(self, dt: float | None = None) -> None:
        """Every env is outdated (a host flag only); ``dt``: the step's ``update(physics_dt)``."""
        if dt is not None:
            self.dt = float(dt)
        self._all = self._dirty = True

    def mark(self, mask: torch.Tensor | None) -> None:
        """The envs of a uint8 / bool mask are outdated (None: all)."""
        if mask is None:
            return self.mark_all()
        self.outdated.logical_or_(mask)
        self._dirty = True

    def reset(self, env_ids=None) -> None:
        if env_ids is None:
            return self.mark_all()
        ids = torch.as_tensor(env_ids, device=self.outdated.device)
        if ids.dtype == torch.bool:
            return self.mark(ids)
        self.outdated[ids.long()] = 1
        self._dirty = True

    def _launch(self) -> None:
        env = self._env
        env._native.imu(self._table, self.dt, self._all, self.outdated, self.data, self.prev, stream=env._stream())
        self.launches += 1
        self._all = self._dirty = False

    def refresh(self) -> None:
        if self._dirty:
            self._launch()

    def update(self, dt: float, force_recompute: bool = False) -> None:
        self.dt = float(dt)
        if force_recompute:
            self._launch()

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {"imu_prev_lin_vel": self.prev[0:3], "imu_prev_ang_vel": self.prev[3:6]}  # (3, S, N) each

    def get_state(self) -> dict:
        return {k: v.clone() for k, v in self.tensors().items()}

    def set_state(self, state: dict) -> None:
        for k, v in self.tensors().items():
            if k in state:
                v.copy_(torch.as_tensor(state[k]).to(v.device, v.dtype).reshape(v.shape))
        self.mark_all()


class _FrameTransformerData:
    """``FrameTransformerData`` (frame_transformer_data.py) of one sensor: zero-copy strided views of the env-minor
    device buffers, as the last launch left them.  Positions are env-local, like every other view here
    (envs/scene.py); the poses in the source frame do not depend on that."""

    def __init__(self, group: "_FrameTransformerSet", s: int, frames: slice, names: list):
        self._g, self._i, self._f = group, s, frames
        self.target_frame_names = names  # the order of envs/frame_transformer.py

    source_pos_w = property(lambda self: self._g.source[0:3, self._i].T)  # (N, 3)
    source_quat_w = property(lambda self: self._g.source[3:7, self._i].T)  # (N, 4) (w, x, y, z)
    target_pos_w = property(lambda self: self._g.target[0:3, self._f].permute(2, 1, 0))  # (N, F_s, 3)
    target_quat_w = property(lambda self: self._g.target[3:7, self._f].permute(2, 1, 0))  # (N, F_s, 4)
    target_pos_source = property(lambda self: self._g.target[7:10, self._f].permute(2, 1, 0))
    target_quat_source = property(lambda self: self._g.target[10:14, self._f].permute(2, 1, 0))


class _FrameTransformer:
    """One frame transformer of an env (the reference's ``FrameTransformer``, frame_transformer.py): sensor
    ``index`` of the env's ``_FrameTransformerSet``, which owns the buffers and the launch."""

    def __init__(self, group: "_FrameTransformerSet", index: int, name: str, cfg):
        self._g, self.index, self.name, self.cfg = group, index, name, cfg
        spec = group._spec
        self._data = _FrameTransformerData(group, index, spec.slices[index], list(spec.frame_names[index]))
        self._source_body = spec.sources[index][2]
        self._target_bodies = list(dict.fromkeys(body[2] for body, _, _ in spec.frames[index]))

    def __str__(self) -> str:
        names = self._data.target_frame_names
        return (f"FrameTransformer @ '{self.cfg.prim_path}': \n"
                f"\ttracked body frames: {[self._source_body] + self._target_bodies} \n"
                f"\tnumber of envs: {self.num_instances}\n"
                f"\tsource body frame: {self._source_body}\n"
                f"\ttarget frames (count: {names}): {len(names)}\n")

    num_instances = property(lambda self: self._g._env.num_envs)
    device = property(lambda self: self._g._env.device)
    launches = property(lambda self: self._g.launches)  # as_frame_transformer launches so far (one serves all)

    @property
    def data(self) -> _FrameTransformerData:
        """The sensor's buffers, after one launch if the scene changed since the last one; a second read launches
        nothing."""
        self._g.refresh()
        return self._data

    def update(self, dt: float = 0.0, force_recompute: bool = False) -> None:
        """SensorBase.update: with ``force_recompute`` one launch now, on the env's current stream -- the call to
        put inside a captured graph; otherwise the next read of ``data`` decides."""
        if force_recompute:
            self._g._launch()

    def reset(self, env_ids=None) -> None:
        """SensorBase.reset: nothing is kept per env but the outdated flag, which here is the set's."""
        self._g.mark_dirty()


class _FrameTransformerSet:
    """The frame transformers of an env (``cfg.frame_transformer``): the device buffers of ``as_frame_transformer``
    (csrc/allsteps_frame_transformer.h) and the one launch that serves every sensor.  Lazy like the height scanner:
    a read of any sensor's ``data`` launches only when the env has marked the scene changed since the last launch
    (``mark_dirty``: step, graph-replay accounting, every reset path, set_state, the robot view's writers, stone
    regeneration); ``update(dt, force_recompute=True)`` always launches.  The sensors keep nothing between updates:
    recomputing an env that the reference would have left alone gives the same bits from the same state, so there is
    no per-env outdated buffer, and there are no get_state keys."""

    def __init__(self, env, cfg):
        from .frame_transformer import FrameTransformerSpec

        n, dev = env.num_envs, env._device
        spec = FrameTransformerSpec(cfg, model=env.model, num_steps=int(env.cfg.num_steps), step_dt=env.step_dt)
        self._env, self._spec = env, spec
        self._table = spec.table()
        self.num_sensors, self.num_frames = spec.num_sensors, spec.num_frames
        # zeros before the first update, as the reference's buffers (frame_transformer.py:315-320)
        self.source = torch.zeros(_native.FRAME_SOURCE_ROWS, self.num_sensors, n, dtype=torch.float32, device=dev)
        self.target = torch.zeros(_native.FRAME_TARGET_ROWS, self.num_frames, n, dtype=torch.float32, device=dev)
        self._dirty = True
        self.launches = 0
        self.sensors = {name: _FrameTransformer(self, s, name, c)
                        for s, (name, c) in enumerate(zip(spec.names, spec.cfgs))}

    def mark_dirty(self) -> None:
        self._dirty = True

    def _launch(self) -> None:
        env = self._env
        env._native.frame_transformer(self._table, self.source, self.target, stream=env._stream())
        self.launches += 1
        self._dirty = False

    def refresh(self) -> None:
        if self._dirty:
            self._launch()


class _RobotView:
    """Minimal ``Articulation`` surface: ``data`` plus the state writers used on reset (each tells the env that the
    scene changed: a lazy sensor recomputes on its next read)."""

    def __init__(self, env, default_joint_pos: torch.Tensor | None = None, init_root_pos=None):
        self._env = env
        self.data = _RobotData(env, default_joint_pos, init_root_pos)
        self._ALL_INDICES = torch.arange(env.num_envs, dtype=torch.long, device=env._device)

    def write_root_pose_to_sim(self, root_pose: torch.Tensor, env_ids=None):
        ids = self._ALL_INDICES if env_ids is None else env_ids
        s = self._env.state
        s["root_pos"][:, ids] = root_pose[:, :3].T.to(s["root_pos"].dtype)
        s["root_quat"][:, ids] = root_pose[:, 3:7].T.to(s["root_quat"].dtype)
        self._env._scene_changed()

    def write_root_velocity_to_sim(self, root_velocity: torch.Tensor, env_ids=None):
        ids = self._ALL_INDICES if env_ids is None else env_ids
        s = self._env.state
        s["root_lin"][:, ids] = root_velocity[:, :3].T.float()
        s["root_ang"][:, ids] = root_velocity[:, 3:6].T.float()
        self._env._scene_changed()

    def write_joint_state_to_sim(self, position, velocity, joint_ids=None, env_ids=None):
        ids = self._ALL_INDICES if env_ids is None else env_ids
        s = self._env.state
        s["q"][:, ids] = position.T.float()
        s["qd"][:, ids] = velocity.T.float()
        self._env._scene_changed()


def __getattr__(name: str):
    """``RewardManagerView`` (``env.reward_manager``, the view of cfg.rewards' device state) lives in envs/rewards.py
    and is loaded on first use, so the default path never imports it."""
    if name == "RewardManagerView":
        from .rewards import RewardManagerView

        return RewardManagerView
    if name == "TerminationManagerView":  # (``env.termination_manager``, envs/terminations.py: the same)
        from .terminations import TerminationManagerView

        return TerminationManagerView
    if name == "ActionManagerView":  # (``env.action_manager``, envs/actions.py: the same)
        from .actions import ActionManagerView

        return ActionManagerView
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
