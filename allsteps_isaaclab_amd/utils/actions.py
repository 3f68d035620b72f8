"""Action configuration -- ``ActionTermCfg`` of ``isaaclab.managers`` and the action term cfgs of
``isaaclab.envs.mdp.actions``, same names, fields and defaults, for ``cfg.actions`` of the envs.

The terms themselves run on the device (``k_actions_process``, csrc/action_kernels.h): a term's class names which of
the built-in joint terms it asks for, and the env raises at construction for anything it does not serve.  The cfg
classes of the terms that are not served are here as well, so that a cfg written for the reference imports and is
then refused with its reason.  ``class_type`` of a served cfg is the term view of envs/actions.py, resolved lazily.

``resolve_matching_names`` / ``resolve_matching_names_values`` are ``isaaclab.utils.string``'s: the joints a list of
regular expressions (or the keys of a dict) selects, with the reference's errors for a name matched twice and for an
expression that matches nothing.
"""

from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Any

from .noise import MISSING


# ---- name resolution (isaaclab/utils/string.py)
def _resolve(keys: list, values: list, names: list, preserve_order: bool):
    found = [None] * len(names)  # the expression that matched each name
    per_key = [[] for _ in keys]
    hits = []  # (name index, key index) in name order
    for i, name in enumerate(names):
        for k, key in enumerate(keys):
            if re.fullmatch(key, name):
                if found[i]:
                    raise ValueError(f"Multiple matches for '{name}': '{found[i]}' and '{key}'!")
                found[i] = key
                hits.append((i, k))
                per_key[k].append(name)
    if preserve_order:  # the order of the expressions, names of one expression in name order
        hits.sort(key=lambda h: h[1])
    if not all(per_key):
        msg = "\n" + "".join(f"\t{key}: {m}\n" for key, m in zip(keys, per_key)) + f"Available strings: {names}\n"
        raise ValueError("Not all regular expressions are matched! Please check that the regular expressions are "
                         f"correct: {msg}")
    return [i for i, _ in hits], [names[i] for i, _ in hits], [values[k] for _, k in hits]


def resolve_matching_names(keys, list_of_strings, preserve_order: bool = False):
    """(indices, names) of the strings that fully match one of the regular expressions ``keys``, in the order of the
    strings, or in the order of the expressions with ``preserve_order``."""
    keys = [keys] if isinstance(keys, str) else list(keys)
    ids, names, _ = _resolve(keys, [None] * len(keys), list(list_of_strings), preserve_order)
    return ids, names


def resolve_matching_names_values(data: dict, list_of_strings, preserve_order: bool = False):
    """(indices, names, values) of the strings that fully match one of the regular-expression keys of ``data``."""
    if not isinstance(data, dict):
        raise TypeError(f"Input argument `data` should be a dictionary. Received: {data}")
    return _resolve(list(data.keys()), list(data.values()), list(list_of_strings), preserve_order)


# ---- cfg classes
class _TermType:
    """``class_type`` of a served cfg: the term view of envs/actions.py, imported on first use."""

    def __get__(self, obj, owner):
        from ..envs.actions import ActionTermView

        return ActionTermView


@dataclass
class ActionTermCfg:
    """manager_term_cfg.py ``ActionTermCfg``."""

    asset_name: str = MISSING
    debug_vis: bool = False
    clip: Any = None  # dict of regular expressions -> (lo, hi), or None
    class_type = None  # (not a field)


@dataclass
class JointActionCfg(ActionTermCfg):
    """actions_cfg.py ``JointActionCfg``: processed = raw * scale + offset over the selected joints."""

    joint_names: Any = MISSING
    scale: Any = 1.0  # float or dict of regular expressions -> float
    offset: Any = 0.0
    preserve_order: bool = False


@dataclass
class JointPositionActionCfg(JointActionCfg):
    """Joint position targets; ``use_default_offset`` replaces ``offset`` by the default joint positions."""

    use_default_offset: bool = True
    class_type = _TermType()


@dataclass
class JointEffortActionCfg(JointActionCfg):
    """Joint efforts."""

    class_type = _TermType()


@dataclass
class JointPositionToLimitsActionCfg(ActionTermCfg):
    """Joint position targets rescaled from [-1, 1] to the soft joint position limits."""

    joint_names: Any = MISSING
    scale: Any = 1.0
    rescale_to_limits: bool = True
    class_type = _TermType()


@dataclass
class EMAJointPositionToLimitsActionCfg(JointPositionToLimitsActionCfg):
    """The same with an exponential moving average: applied = alpha * processed + (1 - alpha) * previous applied."""

    alpha: Any = 1.0  # float or dict of regular expressions -> float, each in [0, 1]


# ---- the reference's terms that are not served (envs/actions.py refuses them with REFUSED's reason)
@dataclass
class RelativeJointPositionActionCfg(JointActionCfg):
    use_zero_offset: bool = True


@dataclass
class JointVelocityActionCfg(JointActionCfg):
    use_default_offset: bool = True


@dataclass
class BinaryJointActionCfg(ActionTermCfg):
    joint_names: Any = MISSING
    open_command_expr: Any = MISSING
    close_command_expr: Any = MISSING


@dataclass
class BinaryJointPositionActionCfg(BinaryJointActionCfg):
    pass


@dataclass
class BinaryJointVelocityActionCfg(BinaryJointActionCfg):
    pass


@dataclass
class NonHolonomicActionCfg(ActionTermCfg):
    body_name: str = MISSING
    x_joint_name: str = MISSING
    y_joint_name: str = MISSING
    yaw_joint_name: str = MISSING
    scale: tuple = (1.0, 1.0)
    offset: tuple = (0.0, 0.0)


@dataclass
class DifferentialInverseKinematicsActionCfg(ActionTermCfg):
    joint_names: Any = MISSING
    body_name: str = MISSING
    body_offset: Any = None
    scale: Any = 1.0
    controller: Any = MISSING


@dataclass
class OperationalSpaceControllerActionCfg(ActionTermCfg):
    joint_names: Any = MISSING
    body_name: str = MISSING
    body_offset: Any = None
    task_frame_rel_path: Any = None
    controller_cfg: Any = MISSING
    position_scale: float = 1.0
    orientation_scale: float = 1.0
    wrench_scale: float = 1.0
    stiffness_scale: float = 1.0
    damping_ratio_scale: float = 1.0
    nullspace_joint_pos_target: str = "none"


REFUSED = {
    "RelativeJointPositionActionCfg": "its target is re-formed from joint_pos in every physics substep, inside the "
                                      "step kernel's substep loop, which the command buffer does not reach",
    "JointVelocityActionCfg": "the DC motor tracks kd * (0 - qd) and has no velocity target",
    "BinaryJointPositionActionCfg": "binary joint terms are not served",
    "BinaryJointVelocityActionCfg": "binary joint terms are not served",
    "BinaryJointActionCfg": "binary joint terms are not served",
    "NonHolonomicActionCfg": "non-holonomic terms are not served (the robots have no dummy base joints)",
    "DifferentialInverseKinematicsActionCfg": "task-space terms are not served (no controller runs on the device)",
    "OperationalSpaceControllerActionCfg": "task-space terms are not served (no controller runs on the device)",
}
SERVED = ("JointPositionActionCfg", "JointEffortActionCfg", "JointPositionToLimitsActionCfg",
          "EMAJointPositionToLimitsActionCfg")
SUPPORTED = ", ".join(SERVED) + " on asset_name 'robot', commanding every joint exactly once"

__all__ = ["ActionTermCfg", "JointActionCfg", *SERVED, *[k for k in REFUSED], "resolve_matching_names",
           "resolve_matching_names_values"]
