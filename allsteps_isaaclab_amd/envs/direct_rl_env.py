"""``DirectRLEnv`` -- the direct-workflow env contract of the reference, MI355X-native.

Mirrors the caller-visible surface of ``isaaclab/envs/direct_rl_env.py`` (``step``, ``reset``,
``seed``, ``close``, spaces, counters; SURVEY.md §8b ring 2).  Unlike the reference there is no
Omniverse simulation context: a subclass owns a native step backend and implements
``_step_impl`` / ``_reset_impl``; the base class keeps the bookkeeping (episode counters, spaces,
``extras``, device placement) so that wrappers written for the reference run unchanged.
"""

from __future__ import annotations

import math
from functools import partialmethod
from typing import Any

import torch

from .scene import SceneView
from .spaces import Box, Dict, batch_box


def _part_classes() -> dict:
    """{attribute of the env: class} of every part of an env that carries device state from step to step, in the
    order of get_state's keys (the parts are built in another order: the actions ahead of the observations)."""
    from .actions import EnvActions
    from .commands import EnvCommands
    from .events import EnvEvents
    from .noise import EnvNoise
    from .observations import EnvObservations
    from .rewards import EnvRewards
    from .terminations import EnvTerminations

    return {"_noise": EnvNoise, "_events": EnvEvents, "_commands": EnvCommands, "_observations": EnvObservations,
            "_rewards": EnvRewards, "_terminations": EnvTerminations, "_action_terms": EnvActions}


class DirectRLEnv:
    """Base class of direct-workflow environments (direct_rl_env.py:53-670)."""

    is_vector_env = True
    metadata: dict = {"render_modes": [None, "rgb_array"], "isaac_sim_version": None}
    env_id_offset = 0  # a shard's first global env id (it enters the noise models' Philox key)
    # Sensors that carry state from step to step (the contact sensors' air / contact timers), set by the subclass
    # that owns them: an object with update(terminated, truncated) -- the step's sensor updates, then the reset of
    # the envs the step reset -- and reset(mask).  None: step() launches nothing for it.
    _sensors = None
    # A lazy sensor (the ray-caster height scanner of cfg.height_scanner), set by the subclass that owns it: an
    # object with mark_dirty().  It is launched by reads of its data, never by step().  None: nothing to mark.
    height_scanner = None
    # Every lazy sensor of the env -- the height scanner and the ray-cast cameras of cfg.camera -- as the subclass
    # that owns them registered them (_add_lazy_sensor): objects with mark_dirty().  Empty: nothing to mark.
    _lazy_sensors: tuple = ()
    # The cameras among them (views._RayCasterCamera): a reset also zeroes their frame counters.  Empty: none.
    _cameras: tuple = ()
    # The IMUs of cfg.imu (views._ImuSet), set by the subclass that owns them: lazy like the height scanner, but
    # outdated by time and by reset only, env by env (a recompute moves their previous velocities).  None: nothing
    # to mark.
    _imus = None
    # cfg.action_noise_model / cfg.observation_noise_model, cfg.events, cfg.commands: the device state of their
    # kernels, built by the constructor.  None: step() launches nothing for them and nothing is allocated.
    _noise = _events = _commands = None
    # cfg.observations (the reference's ObservationManager): the device state of the observation kernel, built by
    # _observations_start once the subclass has its views.  None: step() launches nothing for it.
    _observations = None
    # cfg.rewards (the reference's RewardManager): the device state of the reward kernel, built by _rewards_start
    # once the subclass has its views.  None: step() launches nothing for it.
    _rewards = None
    # cfg.terminations (the reference's TerminationManager): the device state of the termination kernel, built by
    # _terminations_start once the subclass has its views.  None: step() launches nothing for it.
    _terminations = None
    # cfg.actions (the reference's ActionManager): the device state of the action kernels, built by _actions_start
    # once the subclass has its views and actuator.  None: step() launches nothing for it.
    _action_terms = None

    def __init__(self, cfg, render_mode: str | None = None, **kwargs):
        self.cfg = cfg
        self.render_mode = render_mode
        self._is_closed = False
        if cfg.seed is not None:
            cfg.seed = self.seed(cfg.seed)
        self._device = torch.device(cfg.sim.device)
        self.num_envs = int(cfg.scene.num_envs)
        self.scene = SceneView(cfg.scene, self._device)  # env_origins: the reference's world offsets
        self.common_step_counter = 0
        self._sim_step_counter = 0
        self.extras: dict = {}
        self._configure_gym_env_spaces()
        # cfg.action_noise_model / cfg.observation_noise_model (direct_rl_env.py:188-195): device state of the
        # noise kernels, or None -- then step() issues exactly the subclass's launches
        from .noise import EnvNoise

        self._noise = (EnvNoise(cfg, self.num_envs, self._device, cfg.seed if cfg.seed is not None else 0)
                       if EnvNoise.wanted(cfg) else None)
        # cfg.events (direct_rl_env.py:148-149): device state of the interval-event kernel and env.event_manager,
        # or None -- then step() launches nothing for it and nothing is allocated
        from .events import EnvEvents, EventManagerView

        self._events = (EnvEvents(cfg, self.num_envs, self._device, cfg.seed if cfg.seed is not None else 0,
                                  self.step_dt) if EnvEvents.wanted(cfg) else None)
        if self._events is not None:
            self.event_manager = EventManagerView(self._events)
        # cfg.commands (the reference's CommandManager): device state of the command kernel and
        # env.command_manager, or None -- then step() launches nothing for it and nothing is allocated
        from .commands import EnvCommands

        self._commands = (EnvCommands(cfg, self.num_envs, self._device, cfg.seed if cfg.seed is not None else 0,
                                      self.step_dt) if EnvCommands.wanted(cfg) else None)
        if self._commands is not None:
            from .commands import CommandManagerView

            self.command_manager = CommandManagerView(self._commands, self)

    # ------------------------------------------------------------------ properties
    @property
    def device(self) -> str:
        return str(self._device)

    @property
    def physics_dt(self) -> float:
        return self.cfg.sim.dt

    @property
    def step_dt(self) -> float:
        return self.cfg.sim.dt * self.cfg.decimation

    @property
    def max_episode_length_s(self) -> float:
        return self.cfg.episode_length_s

    @property
    def max_episode_length(self) -> int:
        # direct_rl_env.py:247-250
        return math.ceil(self.max_episode_length_s / (self.cfg.sim.dt * self.cfg.decimation))

    @property
    def unwrapped(self) -> "DirectRLEnv":
        return self

    # ------------------------------------------------------------------ spaces (direct_rl_env.py:523-561)
    def _configure_gym_env_spaces(self):
        inf = math.inf
        self.single_observation_space = Dict()
        self.single_observation_space["policy"] = Box(-inf, inf, (int(self.cfg.observation_space),))
        self.single_action_space = Box(-inf, inf, (int(self.cfg.action_space),))
        # direct_rl_env.py:551-552: the batched observation space is the policy Box, not a Dict
        self.observation_space = batch_box(self.single_observation_space["policy"], self.num_envs)
        self.action_space = batch_box(self.single_action_space, self.num_envs)
        self.state_space = None
        if getattr(self.cfg, "state_space", 0):
            self.single_observation_space["critic"] = Box(-inf, inf, (int(self.cfg.state_space),))
            self.state_space = batch_box(self.single_observation_space["critic"], self.num_envs)

    # ------------------------------------------------------------------ operations
    def reset(self, seed: int | None = None, options: dict[str, Any] | None = None):
        """direct_rl_env.py:256-294: reset all envs and return (observations, extras)."""
        if seed is not None:
            self.seed(seed)
            self._reseed(seed)
        obs = self._reset_impl()
        self._scene_changed()
        self._sensors_reset(None)
        self._noise_reset(None)  # the returned observation is not noised (direct_rl_env.py:294)
        if self._observations is not None:  # every history was reset (_sensors_reset); one compute fills them
            obs.update(self._observations.compute_all_reset())
        return obs, self.extras

    def step(self, action: torch.Tensor):
        """direct_rl_env.py:296-383: one env step (decimation physics substeps inside).  With noise models:
        the action model's output is what the step, ``env.actions`` and the action cost see (:322-323); the
        envs the step reset get new biases (:578-581) and the policy observation is noised in place (:379-380).
        With cfg.events: the interval terms run after the step and before the observation noise (:370-372); a
        push is first seen by the next step's physics, as in the reference, where the observation, reward and
        dones of the firing step are made from values cached before it.  With stateful sensors (the contact
        sensors' air / contact timers): their update for the step's substeps and the reset of the envs the step
        reset (:347, :361) follow the step directly.  Only ``step`` drives them -- a subclass's bare physics or
        task launches do not.  With cfg.commands: the command terms' reset of the envs the step reset, then their
        compute(step_dt), follow the step and the sensors and precede the interval events
        (manager_based_rl_env.py:220-239); the commands read the root state and write only their own buffers, so
        the step's outputs are those of an env without them.  With cfg.imu: every env's IMUs become outdated and their ``dt`` the physics step's, as
        after the reference's sensor updates (:347); nothing is launched until a sensor's data is read.  With
        cfg.observations: the term groups are assembled last, one launch per group, after the sensors their terms
        read were brought up to date (manager_based_rl_env.py step: the observations follow the reset, the commands
        and the interval events); they join the returned observation dict under their group names and write only
        their own buffers.  With cfg.rewards: the reward terms are computed in one launch after the sensors, the
        commands and the events and before the observation manager, on the state as the step left it (an env the
        step reset shows its post-reset state); the task's own reward is returned unless
        cfg.rewards_replace_task_reward.  With cfg.terminations: the done terms are computed in one launch directly
        after the step (after the once-per-step contact-force sums where a term reads them) and before everything
        above -- the reference's order, terminations first -- on the state as the step left it; they fill the
        manager's own buffers only, unless cfg.terminations_reset: then the envs the manager ends are reset by one
        masked reset, their observation rows and flags join the step's, and every later stage of this step sees the
        merged flags, so those envs are reset once, in the usual places.  With cfg.actions: the action terms are
        processed in one launch after the action noise model and before the physics, which reads their joint commands
        in place of the actuator's own action formula; the manager's reset of the envs the step reset (and of those
        cfg.terminations_reset ended) follows the step, on the device flags."""
        action = action.to(self._device)
        self._sim_step_counter += self.cfg.decimation
        nz = self._noise
        if nz is not None and nz.action is not None:
            action = nz.apply_actions(action, self._noise_offset(), self._noise_stream())
        if self._action_terms is not None:
            action = self._action_terms.process(action)
        out = self._step_impl(action)
        if self._terminations is not None:
            out = self._terminations.apply(out)
        if self._action_terms is not None:
            self._action_terms.reset(out[2], out[3])
        for sensor in self._lazy_sensors:  # (empty by default: the default step calls nothing)
            sensor.mark_dirty()
        if self._imus is not None:  # the step's sensor updates pass physics_dt (direct_rl_env.py:347)
            self._imus.mark_all(self.physics_dt)
        if self._sensors is not None:  # before the events, as a fixed order: the two touch disjoint buffers
            self._sensors.update(out[2], out[3])
        if self._commands is not None:
            self._commands.apply(*self._commands_root_state(), out[2], out[3], self._noise_offset(),
                                 self._noise_stream())
        if self._events is not None:
            self._events.apply(*self._events_root_velocity(), self._noise_offset(), self._noise_stream())
        if nz is not None:
            nz.post(out[0]["policy"], out[2], out[3], self._noise_offset(), self._noise_stream())
        if self._rewards is not None:
            rew = self._rewards.compute(self.step_dt, out[2], out[2], out[3])
            if self._rewards.replace_task_reward:
                out = (out[0], rew, *out[2:])
        if self._observations is not None:
            out[0].update(self._observations.compute(out[2], out[3]))
        self.common_step_counter += 1
        return out

    # ------------------------------------------------------------------ noise models
    def _noise_stream(self) -> int:
        return torch.cuda.current_stream(self._device).cuda_stream

    def _noise_offset(self) -> int:
        return self.env_id_offset

    def _noise_reset(self, mask: torch.Tensor | None) -> None:
        """NoiseModel.reset(env_ids) of both models (direct_rl_env.py:578-581) for the envs of a uint8 mask
        (None: all) -- the subclass's reset paths call it after their own reset."""
        if self._noise is not None:
            self._noise.post(None, mask, None, self._noise_offset(), self._noise_stream())

    # ------------------------------------------------------------------ state of the parts
    def _part_get_state(self, attr: str) -> dict:
        """The state keys of the part under ``attr`` (a key of _part_classes); none where the env has no such part."""
        part = getattr(self, attr)
        return {} if part is None else part.get_state()

    def _part_set_state(self, attr: str, state: dict) -> dict:
        """Load the part's keys of a set_state dict; returns the dict without the keys the part's class owns --
        whether or not the env has the part, so a key of a manager the env was built without is dropped."""
        part, owns = getattr(self, attr), _part_classes()[attr].owns
        if part is not None:
            part.set_state(state)
        return {k: v for k, v in state.items() if not owns(k)}

    def _parts_get_state(self) -> dict:
        """The state of every part the env has, merged."""
        out = {}
        for attr in _part_classes():
            out.update(self._part_get_state(attr))
        return out

    def _parts_set_state(self, state: dict) -> dict:
        """Hand every part the env has a set_state dict; returns the dict without the keys of any part class."""
        for attr in _part_classes():
            state = self._part_set_state(attr, state)
        return state

    # One part's half of the two calls above, under the per-manager names that callers outside this class use.
    _events_get_state = partialmethod(_part_get_state, "_events")
    _commands_get_state = partialmethod(_part_get_state, "_commands")
    _commands_set_state = partialmethod(_part_set_state, "_commands")
    _rewards_get_state = partialmethod(_part_get_state, "_rewards")
    _rewards_set_state = partialmethod(_part_set_state, "_rewards")
    _terminations_get_state = partialmethod(_part_get_state, "_terminations")
    _terminations_set_state = partialmethod(_part_set_state, "_terminations")
    _actions_get_state = partialmethod(_part_get_state, "_action_terms")
    _actions_set_state = partialmethod(_part_set_state, "_action_terms")

    # ------------------------------------------------------------------ lazy sensors
    def _add_lazy_sensor(self, sensor, camera: bool = False) -> None:
        self._lazy_sensors = (*self._lazy_sensors, sensor)
        if camera:
            self._cameras = (*self._cameras, sensor)

    def _scene_changed(self) -> None:
        """Every path that changes what a lazy sensor sees (root pose, stones) calls this, or does what it does:
        the sensors are marked outdated (a host flag only: nothing is launched)."""
        for sensor in self._lazy_sensors:
            sensor.mark_dirty()

    def _time_advanced(self, dt: float | None = None) -> None:
        """Every path other than ``step`` that advances the simulation (graph-replay accounting, a subclass's bare
        step launches) calls this: the IMUs are outdated by time, every env (a host flag only)."""
        if self._imus is not None:
            self._imus.mark_all(self.physics_dt if dt is None else dt)

    # ------------------------------------------------------------------ stateful sensors
    def _sensors_reset(self, mask: torch.Tensor | None) -> None:
        """Sensor.reset(env_ids) for the envs of a uint8 mask (None: all) -- reset() calls it, and the subclass's
        other reset paths after their own reset."""
        if self._sensors is not None:
            self._sensors.reset(mask)
        if self._imus is not None:  # Imu.reset(env_ids): the envs become outdated, nothing is cleared or launched
            self._imus.mark(mask)
        for camera in self._cameras:  # RayCasterCamera.reset(env_ids): the envs' frame counters become zero
            camera.reset(None if mask is None else mask.bool())
        if self._commands is not None:  # CommandManager.reset(env_ids) of _reset_idx: no compute
            self._commands.reset(mask, self._noise_offset(), self._noise_stream())
        if self._observations is not None:  # ObservationManager.reset(env_ids): the histories, no compute
            self._observations.reset(mask)
        if self._rewards is not None:  # RewardManager.reset(env_ids): the episodic sums and prev_actions
            self._rewards.reset(mask)
        if self._action_terms is not None:  # ActionManager.reset(env_ids): the action history, prev_applied
            self._action_terms.reset(mask)

    # ------------------------------------------------------------------ interval events
    def _events_root_velocity(self):
        """(root_lin, root_ang): the (3, num_envs) device rows the push terms write (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not expose a root velocity for cfg.events")

    def _events_start(self) -> None:
        """Draw the initial timers once the subclass knows its stream and env_id_offset."""
        if self._events is not None:
            self._events.start(self._noise_offset(), self._noise_stream())

    # ------------------------------------------------------------------ command manager
    def _commands_root_state(self):
        """(root_quat (4, n), root_lin (3, n), root_ang (3, n)): the device rows the command terms read (subclass
        hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not expose a root state for cfg.commands")

    # ------------------------------------------------------------------ observation manager
    def _observations_start(self) -> None:
        """Build the observation manager of cfg.observations once the subclass has its state, views and sensors
        (the last line of its constructor); raises NativeError for a cfg the kernel does not serve."""
        from .observations import EnvObservations, ObservationManagerView

        if EnvObservations.wanted(self.cfg):
            self._observations = EnvObservations(self.cfg, self, self.num_envs, self._device,
                                                 self.cfg.seed if self.cfg.seed is not None else 0)
            self.observation_manager = ObservationManagerView(self._observations)

    def _observations_context(self):
        """The ObsContext of the env: what its terms can read (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.observations")

    def _observations_sources(self) -> dict:
        """{source name: device tensor} of the rows the terms read (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.observations")

    # ------------------------------------------------------------------ reward manager
    def _rewards_start(self) -> None:
        """Build the reward manager of cfg.rewards once the subclass has its state, views and sensors (its
        constructor calls it beside _observations_start); raises NativeError for a cfg the kernel does not serve."""
        from .rewards import EnvRewards, RewardManagerView

        if EnvRewards.wanted(self.cfg):
            self._rewards = EnvRewards(self.cfg, self, self.num_envs, self._device)
            self.reward_manager = RewardManagerView(self._rewards)

    def _rewards_context(self):
        """The RewContext of the env: what its terms can read (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.rewards")

    def _rewards_sources(self, net: bool = False) -> dict:
        """{source name: device tensor} of the rows the terms read; net: the contact report's dense net impulses
        are wanted, brought up to date (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.rewards")

    # ------------------------------------------------------------------ action manager
    def _actions_start(self) -> None:
        """Build the action manager of cfg.actions once the subclass has its views and actuator (its constructor
        calls it ahead of _observations_start); raises NativeError for a cfg the kernels do not serve."""
        from .actions import ActionManagerView, EnvActions

        if EnvActions.wanted(self.cfg):
            self._action_terms = EnvActions(self.cfg, self, self.num_envs, self._device)
            self.action_manager = ActionManagerView(self._action_terms)
            self._actions_attach(self._action_terms.cmd)
            self._action_terms.reset(None)  # the envs stand reset: prev_applied = their joint positions

    def _actions_context(self):
        """The ActContext of the env: what its terms resolve against (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.actions")

    def _actions_joint_pos(self) -> torch.Tensor:
        """(joints, num_envs) the device rows of the joint positions, cfg dof order (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.actions")

    def _actions_attach(self, cmd: torch.Tensor) -> None:
        """Make the physics read its joint commands from ``cmd`` (N, joints) (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.actions")

    # ------------------------------------------------------------------ termination manager
    def _terminations_start(self) -> None:
        """Build the termination manager of cfg.terminations once the subclass has its state, views and sensors (its
        constructor calls it beside _rewards_start); raises NativeError for a cfg the kernel does not serve."""
        from .terminations import EnvTerminations, TerminationManagerView

        self._terminations_check_reset()
        if EnvTerminations.wanted(self.cfg):
            self._terminations = EnvTerminations(self.cfg, self, self.num_envs, self._device)
            self.termination_manager = TerminationManagerView(self._terminations)

    def _terminations_check_reset(self) -> None:
        """Raise NativeError where the env cannot serve cfg.terminations_reset (subclass hook)."""
        if getattr(self.cfg, "terminations_reset", False):
            from .. import _native

            raise _native.NativeError(f"cfg.terminations_reset: {type(self).__name__} has no masked reset")

    def _terminations_context(self):
        """The TermContext of the env: what its terms can read (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.terminations")

    def _terminations_sources(self, net: bool = False) -> dict:
        """{source name: device tensor} of the rows the terms read; net: the contact report's dense net impulses
        are wanted, brought up to date (subclass hook)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.terminations")

    def _terminations_reset_mask(self, mask: torch.Tensor, obs: torch.Tensor) -> None:
        """Reset the envs of a device uint8 mask and write every env's observation row into ``obs``: one
        stream-ordered masked reset, no host read (subclass hook of cfg.terminations_reset)."""
        raise NotImplementedError(f"{type(self).__name__} does not serve cfg.terminations_reset")

    @staticmethod
    def seed(seed: int = -1) -> int:
        """direct_rl_env.py:390-407: seed torch / numpy / random (no replicator here)."""
        import random

        import numpy as np

        if seed == -1:
            seed = np.random.randint(0, 10_000)
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        return seed

    def render(self, recompute: bool = False):
        """``rgb_array``: an (H, W, 3) uint8 frame of env 0 (envs/render.py; direct_rl_env.py:508-548
        returns the viewport capture there).  None without a render mode."""
        if self.render_mode is None:
            return None
        if self.render_mode != "rgb_array":
            raise NotImplementedError(f"render_mode={self.render_mode!r}: only 'rgb_array' is supported (headless)")
        return self._render_rgb(0)

    def _render_rgb(self, env_id: int):
        raise NotImplementedError(f"{type(self).__name__} has no renderer")

    def close(self):
        self._is_closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ subclass hooks
    def _reseed(self, seed: int):
        """Re-seed the device streams (subclasses extend it): here the Philox key of the noise models, of
        the interval events (whose timers stay as they are: DirectRLEnv never resets the event manager), of the
        command terms and of the observation terms' noise."""
        for attr in _part_classes():
            part = getattr(self, attr)
            if hasattr(part, "seed"):  # (the rewards, terminations and actions draw nothing)
                part.seed = int(seed)

    def _reset_impl(self):
        raise NotImplementedError

    def _step_impl(self, action: torch.Tensor):
        raise NotImplementedError
