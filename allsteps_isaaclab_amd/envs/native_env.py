"""``NativeDirectEnv`` -- what the direct-workflow envs on the HIP step library share: the SoA state, the
``NativeEnv`` handle over it, the opt-in contact report, state save / restore, rendering and shutdown.  The task
envs (``AllstepsEnv``, ``AnymalCStonesEnv``) add their own ``_step_impl`` / ``_reset_impl`` and task buffers."""

from __future__ import annotations

import torch

from .. import _native
from .direct_rl_env import DirectRLEnv
from .state import alloc_state
from .views import (_ContactReport, _ContactSensor, _ContactTimers, _FootSensor, _FrameTransformerSet, _ImuSet,
                    _RayCaster, _RayCasterCamera)


class NativeDirectEnv(DirectRLEnv):
    _native = None  # the NativeEnv handle: None before _init_native and after close
    _contact_timers = None  # the _ContactTimers of cfg.contact_air_time, or None: nothing allocated or launched
    _frame_transformers = None  # the _FrameTransformerSet of cfg.frame_transformer, or None: the same

    def _init_native(self, model: dict, *, hind: bool = False, feet: bool = False, env_id_offset: int = 0,
                     contact_forces: bool | None = None) -> None:
        """After ``DirectRLEnv.__init__``: the zeroed device state (``alloc_state(n, device, hind=, feet=)``), the
        handle over it, seeded with ``cfg.seed``, and the contact report when ``cfg.contact_forces`` (or the
        constructor's override ``contact_forces``) or ``cfg.contact_air_time`` asks for one -- the timers read the
        report, so they bring it (and with it the force views) whether or not the forces were asked for.
        With ``cfg.height_scanner`` it also builds the ray-caster sensor (``env.height_scanner``,
        ``env.scene.sensors["height_scanner"]``), with ``cfg.camera`` the ray-cast cameras (``env.scene.sensors[name]``;
        ``env.camera`` for a single cfg), with ``cfg.imu`` the IMUs (``env.scene.sensors[name]``; ``env.imu``
        for a single cfg), with ``cfg.frame_transformer`` the frame transformers (``env.scene.sensors[name]``;
        ``env.frame_transformer`` for a single cfg); with ``cfg.contact_forces`` the all-body contact sensor
        (``env.scene.sensors["contact_forces"]``).  Env-specific initial values are the caller's."""
        dev = self._device
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _native.NativeError(f"{type(self).__name__} runs on the HIP backend only (device={dev}, HIP device "
                                      f"available: {torch.cuda.is_available()}); there is no CPU fallback")
        self.model = model
        self.state = alloc_state(self.num_envs, dev, hind=hind, feet=feet)  # SoA, resident in HBM ([field][env])
        self.env_id_offset = int(env_id_offset)
        with torch.cuda.device(dev):
            self._native = _native.NativeEnv(self.num_envs, model, self.cfg, self.state, int(self.cfg.seed or 0),
                                             dev.index if dev.index is not None else torch.cuda.current_device(),
                                             self.env_id_offset)
            self._launches = 0  # launches that change the report (the views' cache key beside the step counters)
            on = self.cfg.contact_forces if contact_forces is None else contact_forces
            air = bool(getattr(self.cfg, "contact_air_time", False))
            self._report = _ContactReport(self, int(self.cfg.decimation)) if on or air else None
            self._contact_timers = (_ContactTimers(self, self._report, self.cfg.contact_force_threshold)
                                    if air else None)
            self._sensors = self._contact_timers  # DirectRLEnv.step / reset drive them
            if on:  # the net forces of every body of the robot, over the report's one launch per step
                self.scene.sensors["contact_forces"] = _ContactSensor(self, self._report)
            hs = getattr(self.cfg, "height_scanner", None)
            if hs is not None:  # lazy: launched by reads of its data (or update(force_recompute=True)), never by step
                self.height_scanner = self.scene.sensors["height_scanner"] = _RayCaster(self, hs)
                self._add_lazy_sensor(self.height_scanner)
            cam = getattr(self.cfg, "camera", None)
            if cam is not None:  # lazy as well; each camera has its own buffers and its own launch
                from .ray_camera import named_cfgs

                cams = named_cfgs(cam)
                taken = sorted(set(cams) & set(self.scene.sensors))
                if taken:
                    raise _native.NativeError(f"cfg.camera: the sensor names {taken} are already registered in the "
                                              f"scene")
                for name, c in cams.items():
                    self.scene.sensors[name] = _RayCasterCamera(self, c, name)
                    self._add_lazy_sensor(self.scene.sensors[name], camera=True)
                if not isinstance(cam, dict):
                    self.camera = self.scene.sensors["camera"]
            imu = getattr(self.cfg, "imu", None)
            if imu is not None:  # lazy too, and one launch serves them all
                self._imus = _ImuSet(self, imu)
                taken = sorted(set(self._imus.sensors) & set(self.scene.sensors))
                if taken:
                    raise _native.NativeError(f"cfg.imu: the sensor names {taken} are already registered in the scene")
                self.scene.sensors.update(self._imus.sensors)
                if not isinstance(imu, dict):
                    self.imu = self._imus.sensors["imu"]
            ft = getattr(self.cfg, "frame_transformer", None)
            if ft is not None:  # lazy like the height scanner; one launch serves them all
                self._frame_transformers = _FrameTransformerSet(self, ft)
                taken = sorted(set(self._frame_transformers.sensors) & set(self.scene.sensors))
                if taken:
                    raise _native.NativeError(f"cfg.frame_transformer: the sensor names {taken} are already registered "
                                              f"in the scene")
                self.scene.sensors.update(self._frame_transformers.sensors)
                self._add_lazy_sensor(self._frame_transformers)
                if not isinstance(ft, dict):
                    self.frame_transformer = self._frame_transformers.sensors["frame_transformer"]
            self._events_start()

    episode_length_buf = property(lambda self: self.state["ep_len"])

    def _stream(self) -> int:
        return torch.cuda.current_stream(self._device).cuda_stream

    _noise_stream = _stream

    def _events_root_velocity(self):
        return self.state["root_lin"], self.state["root_ang"]

    def _commands_root_state(self):
        return self.state["root_quat"], self.state["root_lin"], self.state["root_ang"]

    _actions_clamped = False  # the env's `actions` clamps the last action to [-1, 1] (the walker's)

    def _observations_context(self):
        from .observations import ObsContext

        d = self.robot.data
        hs = self.height_scanner
        return ObsContext(
            joint_names=list(d.joint_names),
            default_joint_pos=d.default_joint_pos[0].detach().cpu().numpy(),
            default_joint_vel=d.default_joint_vel[0].detach().cpu().numpy(),
            soft_joint_pos_limits=d.soft_joint_pos_limits[0].detach().cpu().numpy(),
            action_cols=int(self.cfg.action_space),
            # (with cfg.actions last_action is the manager's `action`, which is not clamped)
            clamp_actions=self._actions_clamped and self._action_terms is None,
            command_names=[] if self._commands is None else list(self._commands.terms.names),
            ray_sensors={} if hs is None else {"height_scanner": int(hs.num_rays)},
            imu_names=[] if self._imus is None else list(self._imus.sensors))

    def _observations_sources(self) -> dict:
        s, hs, im, cm = self.state, self.height_scanner, self._imus, self._commands
        a = self._actions
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = self._actions = a.float().contiguous()
        return {"root_pos": s["root_pos"], "root_quat": s["root_quat"], "root_lin": s["root_lin"],
                "root_ang": s["root_ang"], "q": s["q"], "qd": s["qd"], "actions": a,
                "commands": None if cm is None or not len(cm.terms.names) else cm.vel,
                "imu": None if im is None else im.data,
                "ray_hits": None if hs is None else hs.hits, "ray_pose": None if hs is None else hs.pose}

    def _foot_sensor_infos(self) -> dict:
        """{name: SensorInfo} of the env's foot sensors, under their attribute names: what the reward and the
        termination terms resolve a sensor_cfg against."""
        from ._manager import SensorInfo

        rep = self._report
        return {name: SensorInfo(list(s.body_names), [0 if rep is None else rep.foot_body[f] for f in s._feet],
                                 list(s._feet))
                for name, s in vars(self).items() if isinstance(s, _FootSensor)}

    def _rewards_context(self):
        from .rewards import RewContext

        d = self.robot.data
        rep, tm = self._report, self._contact_timers
        return RewContext(
            joint_names=list(d.joint_names),
            default_joint_pos=d.default_joint_pos[0].detach().cpu().numpy(),
            soft_joint_pos_limits=d.soft_joint_pos_limits[0].detach().cpu().numpy(),
            action_cols=int(self.cfg.action_space), step_dt=self.step_dt,
            command_names=[] if self._commands is None else list(self._commands.terms.names),
            sensors=self._foot_sensor_infos(), contact_forces=rep is not None, contact_air_time=tm is not None)

    def _rewards_sources(self, net: bool = False) -> dict:
        s, cm, rep, tm = self.state, self._commands, self._report, self._contact_timers
        a = self._actions
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = self._actions = a.float().contiguous()
        nd = int(self.model["num_hinges"])
        return {"root_pos": s["root_pos"], "root_quat": s["root_quat"], "root_lin": s["root_lin"],
                "root_ang": s["root_ang"], "q": s["q"][:nd], "qd": s["qd"][:nd], "actions": a,
                "qd_prev": None if rep is None else rep.qd_prev[:nd],
                "commands": None if cm is None or not len(cm.terms.names) else cm.vel.view(-1, self.num_envs),
                "net": rep.forces()[1] if (net and rep is not None) else None,
                "timers": None if tm is None else tm.timers}

    def _actions_context(self):
        from .actions import ActContext

        d = self.robot.data
        act = getattr(self._native, "_act", None)  # (set_actuator's; the walker never calls it: torque)
        return ActContext(
            joint_names=list(d.joint_names),
            default_joint_pos=d.default_joint_pos[0].detach().cpu().numpy(),
            soft_joint_pos_limits=d.soft_joint_pos_limits[0].detach().cpu().numpy(),
            actuator=_native.ACT_TORQUE if act is None else int(act.mode),
            action_space=int(self.cfg.action_space))

    def _actions_joint_pos(self) -> torch.Tensor:
        return self.state["q"][: int(self.model["num_hinges"])]

    def _actions_attach(self, cmd: torch.Tensor) -> None:
        self._native.set_joint_commands(cmd)

    def _terminations_context(self):
        from .terminations import SensorInfo, TermContext

        d = self.robot.data
        rep = self._report
        sensors = self._foot_sensor_infos()
        for name, s in self.scene.sensors.items():  # and the all-body contact sensor of cfg.contact_forces
            if isinstance(s, _ContactSensor):
                sensors[name] = SensorInfo(list(s.body_names), list(range(s.num_bodies)))
        return TermContext(
            joint_names=list(d.joint_names),
            soft_joint_pos_limits=d.soft_joint_pos_limits[0].detach().cpu().numpy(),
            step_dt=self.step_dt, max_episode_length=self.max_episode_length,
            command_names=[] if self._commands is None else list(self._commands.terms.names),
            sensors=sensors, contact_forces=rep is not None)

    def _terminations_sources(self, net: bool = False) -> dict:
        s, cm, rep = self.state, self._commands, self._report
        nd = int(self.model["num_hinges"])
        has_cm = cm is not None and len(cm.terms.names)
        return {"root_pos": s["root_pos"], "root_quat": s["root_quat"], "q": s["q"][:nd], "qd": s["qd"][:nd],
                "ep_len": s["ep_len"],
                "time_left": cm.time_left if has_cm else None, "command_counter": cm.counter if has_cm else None,
                "net": rep.forces()[1] if (net and rep is not None) else None}

    def _report_or_raise(self, what: str) -> _ContactReport:
        if self._report is None:
            raise _native.NativeError(
                f"{what} is not available: the MI355X step keeps the per-stone contact flags of each foot "
                f"(force_matrix_w, flag-valued), not contact forces or joint accelerations, unless the env is built "
                f"with cfg.contact_forces = True (INTEGRATION.md §C3)")
        return self._report

    def _contact_masks(self) -> torch.Tensor:
        """(feet, N) stone bitmasks of the sensor feet in the last substep: two rows, four with the hind pair."""
        s = self.state
        return torch.cat([s["contact_mask"], s["contact_mask_hind"]]) if "contact_mask_hind" in s else s["contact_mask"]

    def _render_rgb(self, env_id: int):
        from .render import render_frame

        st = {k: self.state[k][..., env_id].detach().cpu().numpy() for k in ("root_pos", "root_quat", "q", "stones")}
        half = [0.5 * v for v in self.cfg.step_size]
        return render_frame(self.model, st["root_pos"], st["root_quat"], st["q"], st["stones"].reshape(-1, 3), half,
                            target=int(self.state["idx"][env_id]))

    def get_state(self) -> dict:
        """Copy of the full SoA state (field -> (rows, N) tensor); with a noise model, also the noise
        stream's counter and biases (noise_t, noise_action_bias, noise_obs_bias); with cfg.events, the event
        streams' counter and timers (event_t, event_time_left); with cfg.contact_air_time, the sensors' timers and
        timestamp (contact_timers (4, B, N), contact_timestamp (N,)); with cfg.imu, the IMUs' previous world
        velocities (imu_prev_lin_vel, imu_prev_ang_vel, (3, S, N) each); with cfg.commands, the command streams'
        counter and the terms' state (command_t, command_time_left, command_vel_b, command_heading_target,
        command_flags, command_counter, command_metrics, command_last_metrics); with cfg.observations, the observation
        streams' counters, the push counts and each group's output rows, which hold its history (observation_t,
        observation_count, (groups, N) each; observation_history_<group>, (N, columns)); with cfg.rewards, the
        reward manager's episodic sums, step values and last episode's sums ((terms, N) each) and its previous
        actions (reward_episode_sums, reward_step, reward_last_episode_sums, reward_prev_actions); with
        cfg.terminations, the termination manager's flags (termination_term_dones, termination_last_episode_dones,
        (terms, N); termination_time_outs, termination_terminated, termination_dones, termination_reset_request,
        (N,); uint8); with cfg.actions, the action manager's buffers (action_action, action_prev_action,
        action_processed, action_prev_applied, (N, columns); action_commands, (N, joints))."""
        tm, im = self._contact_timers, self._imus
        return {**{k: v.clone() for k, v in self.state.items()}, **self._parts_get_state(),
                **({} if tm is None else tm.get_state()),
                **({} if im is None else im.get_state())}

    def set_state(self, state: dict):
        self._scene_changed()
        if self._contact_timers is not None:
            self._contact_timers.set_state(state)
        if self._imus is not None:  # (and every env is outdated)
            self._imus.set_state(state)
        state = {k: v for k, v in state.items() if k not in _ContactTimers.STATE_KEYS + _ImuSet.STATE_KEYS}
        for k, v in self._parts_set_state(state).items():
            self.state[k].copy_(torch.as_tensor(v).to(self.state[k].device, self.state[k].dtype).reshape(
                self.state[k].shape))

    def _reseed(self, seed: int):
        super()._reseed(seed)
        self._native.set_seed(int(seed))

    def close(self):
        if self._native is not None:
            self._native.close()
            self._native = None
        super().close()
