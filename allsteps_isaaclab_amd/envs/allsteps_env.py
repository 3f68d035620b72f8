"""``AllstepsEnv`` -- the Allsteps-v0 stepping-stone task on the MI355X-native step kernels.

Drop-in for ``isaaclab_tasks/direct/allsteps/allsteps_env.py:34-567`` (``AllstepsEnv``): same
constructor (``cfg, render_mode``), same ``step``/``reset`` results (policy obs (N, 59), reward,
terminated, truncated, extras), same task buffers (``curr_target_index``, ``swing_leg``,
``potentials`` ...), same mirror indices and symmetry functions.  Underneath, the whole
``DirectRLEnv.step`` -- actuation, 4 physics substeps, contacts, foot-state machine, rewards,
dones, resets, observations -- is two HIP kernels (``liballsteps_hip.so``) over a struct-of-arrays
state that stays resident in HBM; there is no PhysX, no Python per-step logic and no host sync.
"""

from __future__ import annotations

from typing import Tuple

import torch

from .. import _native
from ..model import load_model
from .allsteps_env_cfg import AllstepsEnvCfg
from .native_env import NativeDirectEnv
from .views import _FootSensor, _RobotView

RIGHT_FOOT = 0
LEFT_FOOT = 1
EPSILON = 1e-4


class AllstepsEnv(NativeDirectEnv):
    cfg: AllstepsEnvCfg

    def __init__(self, cfg: AllstepsEnvCfg | None = None, render_mode: str | None = None, *,
                 env_id_offset: int = 0, model: dict | None = None, contact_forces: bool | None = None, **kwargs):
        cfg = cfg if cfg is not None else AllstepsEnvCfg()
        super().__init__(cfg, render_mode, **kwargs)
        self._init_native(model if model is not None else load_model(), env_id_offset=env_id_offset,
                          contact_forces=contact_forces)
        n = self.num_envs
        dev = self._device
        self.state["root_quat"][0] = 1.0
        self.state["idx"][:] = 1
        self.state["next"][:] = 2
        with torch.cuda.device(dev):
            # footsteps generated once at init (allsteps_env.py:71), curriculum level 0 by default
            self._native.generate_stones(int(cfg.initial_stone_curriculum), stream=self._stream())
        # ---- DirectRLEnv buffers (direct_rl_env.py:179-185)
        self.reset_terminated = torch.zeros(n, dtype=torch.bool, device=dev)
        self.reset_time_outs = torch.zeros(n, dtype=torch.bool, device=dev)
        self.reward_buf = torch.zeros(n, dtype=torch.float32, device=dev)
        self.obs_buf = {"policy": torch.zeros(n, cfg.observation_space, device=dev)}
        self._actions = torch.zeros(n, cfg.action_space, device=dev)
        # ---- task constants / names (allsteps_env.py:41-92)
        self.num_steps = cfg.num_steps
        self.step_radius = cfg.step_radius
        self.stop_frames = cfg.stop_frames
        self.max_curriculum = torch.tensor(cfg.max_curriculum, dtype=torch.int64, device=dev)
        self.termination_curriculum = torch.as_tensor(_native.linspace_f32(0.75, 0.45, cfg.max_curriculum + 1),
                                                      device=dev)
        self.applied_gain_curriculum = torch.as_tensor(_native.linspace_f32(1.2, 1.2, cfg.max_curriculum + 1),
                                                       device=dev)
        self.joint_gears = torch.tensor(cfg.joint_gears, dtype=torch.float32, device=dev)
        self.robot = _RobotView(self, init_root_pos=cfg.init_root_pos)
        # foot contact sensors (allsteps_env.py:224-226): right = sensor foot 0, left = 1
        self.sensor_right = _FootSensor(self, [0], ["right_foot"], True)
        self.sensor_left = _FootSensor(self, [1], ["left_foot"], True)
        self.sensor = _FootSensor(self, [0, 1], ["right_foot", "left_foot"], False)
        jn = self.robot.data.joint_names
        self.foot_names = list(cfg.foot_names)
        self.foot_indices = [self.robot.data.body_names.index(x) for x in self.foot_names]
        self.torso_index = self.robot.data.body_names.index(cfg.torso_name)
        L = lambda names: torch.tensor([jn.index(x) for x in names], dtype=torch.int64, device=dev)  # noqa: E731
        self.hip_y_index = L(cfg.hip_y_names)
        self.right_body_indices = L(cfg.right_body_names)
        self.left_body_indices = L(cfg.left_body_names)
        self.negation_body_indices = L(cfg.negation_body_names)
        self._actions_start()
        self._observations_start()
        self._rewards_start()
        self._terminations_start()

    _actions_clamped = True  # `actions` below

    def _terminations_check_reset(self) -> None:
        pass  # cfg.terminations_reset is served: as_reset_mask takes a device mask

    def _terminations_reset_mask(self, mask: torch.Tensor, obs: torch.Tensor) -> None:
        """cfg.terminations_reset: as_reset_mask on the manager's device mask.  As in _reset_idx, the curriculum
        gate and the second foot-state tick run for every env when any env of the mask is reset, as the reference's
        _reset_idx does; an all-zero mask leaves the state as it is.  The managers are not reset here: the step
        hands the merged flags to them."""
        self._native.reset_mask(mask, obs, None, stream=self._stream())

    # ------------------------------------------------------------------ task buffers (views)
    curr_target_index = property(lambda self: self.state["idx"])
    prev_target_index = property(lambda self: self.state["prev"])
    next_target_index = property(lambda self: self.state["next"])
    target_reach_count = property(lambda self: self.state["count"])
    swing_leg = property(lambda self: self.state["swing"])
    potentials = property(lambda self: self.state["pot"])
    old_potentials = property(lambda self: self.state["old_pot"])
    foot_contact = property(lambda self: self.state["foot_contact"].T)

    @property
    def curriculum(self) -> torch.Tensor:
        """Per-env curriculum level (all envs share one level in the reference, allsteps_env.py:472)."""
        return self.state["curriculum"].expand(self.num_envs)

    @property
    def steps_pos(self) -> torch.Tensor:
        """(N, 20, 3) stepping-stone centres, env-local frame."""
        return self.state["stones"].view(self.num_steps, 3, -1).permute(2, 0, 1)

    @property
    def actions(self) -> torch.Tensor:
        return torch.clamp(self._actions, -1.0, 1.0)

    @property
    def reset_buf(self) -> torch.Tensor:
        return self.reset_terminated | self.reset_time_outs

    @property
    def targets_w(self) -> torch.Tensor:
        """(N, 3, 3) previous / current / next target stone (allsteps_env.py:459-467)."""
        sp = self.steps_pos
        ar = torch.arange(self.num_envs, device=self._device)
        idx = [self.state[k].long() for k in ("prev", "idx", "next")]
        return torch.stack([sp[ar, i] for i in idx], 1)

    # ------------------------------------------------------------------ native backend
    def _reset_impl(self, reset_draws: torch.Tensor | None = None):
        obs = torch.empty(self.num_envs, self.cfg.observation_space, device=self._device)
        self._native.reset_all(obs, reset_draws, stream=self._stream())
        self.obs_buf = {"policy": obs}
        return self.obs_buf

    def _reset_idx(self, env_ids, reset_draws: torch.Tensor | None = None):
        """AllstepsEnv._reset_idx(env_ids) (allsteps_env.py:469-567): reset the given envs (curriculum
        gate and second foot-state tick for all envs, as the reference does), then refresh the
        observation buffer.  ``env_ids``: indices, a bool mask, or None (all envs)."""
        self._scene_changed()
        if env_ids is None:
            obs = self._reset_impl(reset_draws)
            self._sensors_reset(None)
            self._noise_reset(None)
            return obs
        ids = torch.as_tensor(env_ids, device=self._device)
        if ids.dtype == torch.bool:
            if ids.shape != (self.num_envs,):
                raise ValueError(f"env_ids mask must be ({self.num_envs},), got {tuple(ids.shape)}")
            mask = ids.to(torch.uint8).contiguous()
        else:
            ids = ids.long().reshape(-1)
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.num_envs):
                raise IndexError(f"env_ids out of range [0, {self.num_envs})")
            mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self._device)
            mask[ids] = 1
        obs = torch.empty(self.num_envs, self.cfg.observation_space, device=self._device)
        d = None if reset_draws is None else reset_draws.to(self._device).float().contiguous()
        self._native.reset_mask(mask, obs, d, stream=self._stream())
        self._sensors_reset(mask)
        self._noise_reset(mask)
        self.obs_buf = {"policy": obs}
        return self.obs_buf

    def _step_impl(self, action: torch.Tensor, reset_draws: torch.Tensor | None = None):
        a = action if (action.dtype == torch.float32 and action.is_contiguous()) else action.float().contiguous()
        if a.shape != (self.num_envs, self.cfg.action_space):
            raise ValueError(f"actions must be ({self.num_envs}, {self.cfg.action_space}), got {tuple(a.shape)}")
        obs = torch.empty(self.num_envs, self.cfg.observation_space, device=self._device)
        rew = torch.empty(self.num_envs, device=self._device)
        self._native.step(a, obs, rew, self.reset_terminated, self.reset_time_outs, reset_draws,
                          stream=self._stream())
        self._launches += 1
        self._actions = a
        self.obs_buf = {"policy": obs}
        self.reward_buf = rew
        return self.obs_buf, rew, self.reset_terminated, self.reset_time_outs, self.extras

    # ---- HIP-graph capture of step() (trainer rollout graphs)
    graph_safe_step = True  # step() launches only stream-ordered work with no host synchronisation

    def set_graph_capture(self, on: bool = True) -> None:
        """Make ``step`` replayable from a captured HIP graph (as_set_graph_safe: fixed counter bank,
        cleared by a memset node per call)."""
        self._native.set_graph_safe(on)

    def account_steps(self, k: int = 1) -> None:
        """Advance the host-side step counters for ``k`` steps replayed from a graph (the replay runs
        the device work of ``step`` but not its Python bookkeeping)."""
        self._sim_step_counter += self.cfg.decimation * k
        self.common_step_counter += k
        self._scene_changed()
        self._time_advanced()

    def step_with_draws(self, action: torch.Tensor, reset_draws: torch.Tensor):
        """``step`` with injected reset draws ((N, 22) U[0,1): mirror, 21 joint noise) -- parity tests."""
        self._sim_step_counter += self.cfg.decimation
        action = action.to(self._device)
        if self._action_terms is not None:  # as step(): process, the step, the manager's reset on the step's flags
            action = self._action_terms.process(action)
        out = self._step_impl(action, reset_draws.to(self._device).float().contiguous())
        if self._action_terms is not None:
            self._action_terms.reset(out[2], out[3])
        self._scene_changed()
        self._time_advanced()
        self.common_step_counter += 1
        return out

    def reset_with_draws(self, reset_draws: torch.Tensor):
        self._scene_changed()
        if self._imus is not None:
            self._imus.mark(None)
        return self._reset_impl(reset_draws.to(self._device).float().contiguous()), self.extras

    def task_step(self, action: torch.Tensor, reset_draws: torch.Tensor | None = None):
        """Post-physics half of ``step`` on the current state (body_pos / contact_mask as written)."""
        a = action.to(self._device).float().contiguous()
        obs = torch.empty(self.num_envs, self.cfg.observation_space, device=self._device)
        rew = torch.empty(self.num_envs, device=self._device)
        d = None if reset_draws is None else reset_draws.to(self._device).float().contiguous()
        self._native.task_step(a, obs, rew, self.reset_terminated, self.reset_time_outs, d, stream=self._stream())
        self._scene_changed()
        self._time_advanced()
        return {"policy": obs}, rew, self.reset_terminated, self.reset_time_outs, self.extras

    def physics_step(self, action: torch.Tensor):
        """Physics only (4 substeps, no task logic) -- known-answer tests / profiling."""
        a = action.to(self._device).float().contiguous()
        if self._action_terms is not None:  # the physics reads the manager's commands
            a = self._action_terms.process(a)
        self._native.physics_step(a, stream=self._stream())
        self._launches += 1
        self._scene_changed()
        self._time_advanced()

    def generate_foot_steps(self, level: int, draws: torch.Tensor | None = None):
        """_generate_foot_steps_allsteps at `level` for every env (allsteps_env.py:106-174)."""
        d = None if draws is None else draws.to(self._device).float().contiguous()
        self._native.generate_stones(int(level), d, stream=self._stream())
        self._scene_changed()

    def dropped_contacts(self) -> int:
        """Contacts the constraint budget (AS_MAX_CONTACTS contacts, AS_MAX_ROWS rows incl. the joint
        limits) cut in the last step, over all envs and substeps -- PhysX keeps every contact
        (simulation_cfg.py:110), so this is the step's deviation from it in contact count.  Reads the
        device counter (as_step_counters word 3): synchronises the env's stream."""
        return int(self._native.counters_host(self._stream())[3])


# ------------------------------------------------------------------------------------------------
# mirror augmentation (allsteps_env.py:570-660)

def _mirror_indices(env, obs_dim: int, act_dim: int, device):
    uw = env.unwrapped
    right, left, neg = uw.right_body_indices, uw.left_body_indices, uw.negation_body_indices
    K = 2 if obs_dim == 56 else 3
    steps_neg = torch.tensor([K * i + 1 for i in range(3)], dtype=torch.int64, device=device)
    root_neg = torch.tensor([1, 4], dtype=torch.int64, device=device)
    r_obs = torch.cat((right + 6, right + 6 + act_dim, torch.tensor([6 + act_dim * 2], device=device)))
    l_obs = torch.cat((left + 6, left + 6 + act_dim, torch.tensor([6 + act_dim * 2 + 1], device=device)))
    n_obs = torch.cat((root_neg, 6 + neg, 6 + act_dim + neg, 6 + act_dim * 2 + 2 + steps_neg))
    return right, left, neg, r_obs, l_obs, n_obs


def _mirror(x, right, left, neg):
    y = x.clone()
    y[:, right] = x[:, left]
    y[:, left] = x[:, right]
    y[:, neg] = -x[:, neg]
    return y


def get_symmetric_states_rsl_rl(obs, actions, env, is_critic: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    uw = env.unwrapped
    dev = uw.right_body_indices.device
    right, left, neg, r_obs, l_obs, n_obs = _mirror_indices(env, uw.observation_space.shape[1],
                                                            uw.action_space.shape[1], dev)
    ro = None if obs is None else torch.vstack((obs, _mirror(obs, r_obs, l_obs, n_obs)))
    ra = None if actions is None else torch.vstack((actions, _mirror(actions, right, left, neg)))
    return ro, ra


def get_symmetric_states_rl_games(obs, actions, env, is_critic: bool, mus):
    ro, ra = get_symmetric_states_rsl_rl(obs, actions, env, is_critic)
    if mus is None:
        return ro, ra, None
    uw = env.unwrapped
    rm = torch.vstack((mus, _mirror(mus, uw.right_body_indices, uw.left_body_indices, uw.negation_body_indices)))
    return ro, ra, rm
