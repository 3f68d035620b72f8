"""Event configuration -- ``EventTermCfg`` / ``SceneEntityCfg`` of ``isaaclab.managers`` and the event function
``push_by_setting_velocity`` of ``isaaclab.envs.mdp``, same names, fields and defaults, for ``cfg.events`` of the
envs.

The events themselves run on the device (``k_events_interval``, csrc/event_kernels.h): ``func`` names which of
the built-in event functions a term asks for, and the env raises at construction for anything it does not
serve.  The function below is that name; there is no host implementation behind it.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable

from .noise import MISSING

VELOCITY_KEYS = ("x", "y", "z", "roll", "pitch", "yaw")


def push_by_setting_velocity(env, env_ids, velocity_range=None, asset_cfg=None):
    """events.py ``push_by_setting_velocity``: the term the HIP event kernel applies for this cfg."""
    raise NotImplementedError(
        "push_by_setting_velocity names an event term of the device kernel (cfg.events of an env); it has no "
        "host implementation")


@dataclass
class SceneEntityCfg:
    """scene_entity_cfg.py ``SceneEntityCfg``: the asset a term acts on.  The fields that select a part of the
    asset are carried so that the env can refuse them; the defaults mean the whole asset."""

    name: str = MISSING
    joint_names: Any = None
    joint_ids: Any = slice(None)
    fixed_tendon_names: Any = None
    fixed_tendon_ids: Any = slice(None)
    body_names: Any = None
    body_ids: Any = slice(None)
    object_collection_names: Any = None
    object_collection_ids: Any = slice(None)
    preserve_order: bool = False

    def whole(self) -> bool:
        """No joint / body / tendon / object selection: the term acts on the whole asset."""
        return all(getattr(self, k) is None for k in ("joint_names", "fixed_tendon_names", "body_names",
                                                      "object_collection_names")) and \
            all(getattr(self, k) == slice(None) for k in ("joint_ids", "fixed_tendon_ids", "body_ids",
                                                          "object_collection_ids"))


@dataclass
class EventTermCfg:
    """manager_term_cfg.py ``EventTermCfg`` (with ``ManagerTermBaseCfg``'s ``func`` / ``params``)."""

    func: Callable = MISSING
    params: dict = field(default_factory=dict)
    mode: str = MISSING  # "startup" | "reset" | "interval"
    interval_range_s: tuple | None = None
    is_global_time: bool = False
    min_step_count_between_reset: int = 0


SUPPORTED = ("EventTermCfg(func=push_by_setting_velocity, mode='interval', interval_range_s=(lo, hi), "
             "is_global_time=False, params={'velocity_range': {x y z roll pitch yaw: (lo, hi)}, "
             "'asset_cfg': SceneEntityCfg('robot')})")
