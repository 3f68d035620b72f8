"""``AnymalCStonesEnv`` -- BASELINE C5 behind the direct-workflow env surface (registered as
``Allsteps-AnymalC-v0``), so ``RlGamesVecEnvWrapper``, ``train.py`` and ``play.py`` drive it like Allsteps-v0.

One ``step(actions)`` is ``as_quad_step`` on the HIP device: ``decimation`` substeps of ``k_step<18>``
(6 + 12 generalized velocities) with IsaacLab's DC motor evaluated in every substep on the position targets
``default_q + action_scale * a`` (anymal_c_env.py:73-78), four foot sensors, then ``k_quad``: target
stones, potentials, rewards, dones, in-kernel resets of done envs (stand pose + Philox joint noise, actions
observed as zero: anymal_c_env.py:171-172) and the 64-float observation.  Simulation settings are ANYmal-C's
(``AnymalCStonesEnvCfg``: dt 1/200, friction 1.0 multiply, max depenetration velocity 1.0).  There is no
CPU fallback: without the HIP library or a gfx950 device the constructor raises ``NativeError``.
"""

from __future__ import annotations

import torch

from .. import _native
from ..model import ANYMAL_C_JSON, load_model
from .anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
from .native_env import NativeDirectEnv
from .quadruped import level0_stones, stand_pose
from .views import _FootSensor, _RobotView


class AnymalCStonesEnv(NativeDirectEnv):
    """The C5 task env: ``reset() -> ({"policy": obs}, extras)``, ``step(a) -> ({"policy": obs}, reward,
    terminated, truncated, extras)``; every buffer on the device."""

    cfg: AnymalCStonesEnvCfg

    def __init__(self, cfg: AnymalCStonesEnvCfg | None = None, render_mode: str | None = None, *,
                 env_id_offset: int = 0, contact_forces: bool | None = None, **kwargs):
        cfg = cfg or AnymalCStonesEnvCfg()
        super().__init__(cfg, render_mode, **kwargs)
        model = load_model(ANYMAL_C_JSON)
        if not cfg.robot.enabled_self_collisions:  # ArticulationRootPropertiesCfg.enabled_self_collisions
            model = dict(model, num_self_pairs=0, self_pair=[0] * len(model["self_pair"]))
        self.num_dof = model["num_hinges"]
        if self.num_dof != cfg.action_space:
            raise ValueError(f"model has {self.num_dof} hinges, cfg.action_space = {cfg.action_space}")
        # the opt-in contact report (cfg.contact_forces) comes with the handle
        # env_id_offset: a shard's first global env id, the key of the reset draws (as AllstepsEnv's)
        self._init_native(model, hind=True, feet=True, env_id_offset=env_id_offset, contact_forces=contact_forces)
        n, dev = self.num_envs, self._device
        self.state["stones"][:] = torch.as_tensor(level0_stones(n, cfg.num_steps), device=dev)
        self.default_joint_pos = torch.as_tensor(stand_pose(model["dof_names"], cfg.robot.init_joint_pos), device=dev)
        self._native.set_actuator(_native.ACT_DC_MOTOR, action_scale=cfg.action_scale,
                                  default_q=self.default_joint_pos.cpu().tolist(), **cfg.actuator())
        self._native.set_quad_task(**cfg.quad_task())
        # the four-foot contact sensor (sensor order RF, LF, RH, LH; filtered by the stones): flag-valued
        # force_matrix_w without the contact report, as the walker's
        body_link = [int(x) for x in self.model["body_link"][: int(self.model["num_bodies"])]]
        ng = int(self.model["num_geoms"])
        foot_link = {int(f): int(l) for f, l in zip(self.model["geom_foot"][:ng], self.model["geom_link"][:ng])
                     if int(f) >= 0}
        self.sensor = _FootSensor(self, [0, 1, 2, 3],
                                  [self.model["body_names"][body_link.index(foot_link[f])] for f in range(4)], True)
        # articulation.py:1262-1266: mean -+ 0.5 range * factor (data only, as in IsaacLab)
        lo = torch.tensor([self.model["lower"][self.model["cfg_dof_link"][k]] for k in range(self.num_dof)])
        hi = torch.tensor([self.model["upper"][self.model["cfg_dof_link"][k]] for k in range(self.num_dof)])
        mean, rng = (lo + hi) / 2, hi - lo
        f = cfg.robot.soft_joint_pos_limit_factor
        self.soft_joint_pos_limits = torch.stack([mean - 0.5 * rng * f, mean + 0.5 * rng * f], -1).to(dev)
        self.soft_joint_pos_limits = self.soft_joint_pos_limits.unsqueeze(0).expand(n, -1, -1)
        self.obs_buf = torch.zeros((n, _native.QUAD_OBS_DIM), dtype=torch.float32, device=dev)
        self.reward_buf = torch.zeros(n, dtype=torch.float32, device=dev)
        # k_quad writes 0 / 1 bytes straight into the bool buffers (torch.bool is one byte, as AllstepsEnv)
        self.reset_terminated = torch.zeros(n, dtype=torch.bool, device=dev)
        self.reset_time_outs = torch.zeros(n, dtype=torch.bool, device=dev)
        # persistent reset_buf (DirectRLEnv keeps one): filled from terminated | truncated on the first
        # access after a step, so in-place writes (env.reset_buf[ids] = 1) stick until the next step
        self._reset_buf = torch.zeros(n, dtype=torch.bool, device=dev)
        self._reset_buf_stale = False
        self.extras = {}
        self._native.quad_reset_all(self.obs_buf, stream=self._stream())
        # the ArticulationData views (ring 1 zero-copy, ring 2 -- the 13 MJCF bodies -- by as_body_state on
        # demand), as the walker's env serves them (envs/views.py)
        self.robot = _RobotView(self, default_joint_pos=self.default_joint_pos)
        self._actions = torch.zeros(n, self.num_dof, dtype=torch.float32, device=dev)
        self._actions_start()
        self._observations_start()
        self._rewards_start()
        self._terminations_start()

    def _terminations_check_reset(self) -> None:
        if getattr(self.cfg, "terminations_reset", False):
            raise _native.NativeError("cfg.terminations_reset is not served by the quadruped: k_quad resets the envs "
                                      "its own dones end and has no masked reset (DESIGN.md §9); leave it False -- "
                                      "the termination manager then fills its own buffers")

    @property
    def actions(self) -> torch.Tensor:
        """The last step's actions as the step took them (anymal_c_env.py keeps them unclamped)."""
        return self._actions

    @property
    def target_index(self) -> torch.Tensor:
        return self.state["idx"]

    @property
    def reset_buf(self) -> torch.Tensor:
        """terminated | truncated of the last step: one persistent buffer, formed on the first access after
        a step (no kernel in the step itself); writes into it persist until the next step."""
        if self._reset_buf_stale:
            torch.logical_or(self.reset_terminated, self.reset_time_outs, out=self._reset_buf)
            self._reset_buf_stale = False
        return self._reset_buf

    @reset_buf.setter
    def reset_buf(self, value) -> None:
        self._reset_buf.copy_(torch.as_tensor(value, device=self._reset_buf.device).to(torch.bool).expand_as(
            self._reset_buf))
        self._reset_buf_stale = False

    @property
    def foot_targets(self) -> torch.Tensor:
        """(N, 4) target stone of each sensor foot (RF, LF, RH, LH); target_index is the front pair's min"""
        return self.state["feet"][:4].T

    @property
    def contact_mask(self) -> torch.Tensor:
        """(N, 4) stone bitmasks of the four sensor feet (RF, LF, RH, LH) in the last substep."""
        return self._contact_masks().T

    def _reset_impl(self):
        self._native.quad_reset_all(self.obs_buf, stream=self._stream())
        self._launches += 1
        self._reset_buf_stale = True
        return {"policy": self.obs_buf}

    def _reset_idx(self, env_ids):
        """AnymalCEnv._reset_idx(env_ids) (anymal_c_env.py:163-182): reset the given envs -- ``as_quad_reset_mask``
        on a device mask, one launch, no physics -- and rewrite their rows of ``obs_buf`` in place; the other
        envs keep their state and the last step's observation.  ``env_ids``: indices, a bool mask of shape
        (num_envs,), or None (all envs).  The stateful sensors, the managers and the noise models reset the same
        envs; ``reset_terminated`` / ``reset_time_outs`` and ``reset_buf`` stay as they are."""
        self._scene_changed()
        if env_ids is None:
            obs = self._reset_impl()
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
        self._native.quad_reset_mask(mask, self.obs_buf, stream=self._stream())
        self._launches += 1  # (the masked envs' report counts were cleared)
        self._sensors_reset(mask)
        self._noise_reset(mask)
        return {"policy": self.obs_buf}

    def _step_impl(self, action: torch.Tensor):
        if action.shape != (self.num_envs, self.num_dof):
            raise ValueError(f"actions must be ({self.num_envs}, {self.num_dof}), got {tuple(action.shape)}")
        a = action.to(torch.float32).contiguous()
        self._native.quad_step(a, self.obs_buf, self.reward_buf, self.reset_terminated, self.reset_time_outs,
                               stream=self._stream())
        self._launches += 1
        self._actions = a
        self._reset_buf_stale = True
        return {"policy": self.obs_buf}, self.reward_buf, self.reset_terminated, self.reset_time_outs, self.extras
