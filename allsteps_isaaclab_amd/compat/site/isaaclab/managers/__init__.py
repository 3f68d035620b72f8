"""Shim of ``isaaclab.managers``: the event cfg classes, served by the device event kernel, the command term
cfg base class, served by the device command kernel, the observation term and group cfg classes, served by the
device observation kernel, the reward term cfg class, served by the device reward kernel, the termination term
cfg class, served by the device termination kernel, and the action term cfg base class, served by the device action
kernels.  The manager-based workflow itself is out of scope."""

from allsteps_isaaclab_amd.utils.actions import ActionTermCfg  # noqa: F401
from allsteps_isaaclab_amd.utils.commands import CommandTermCfg  # noqa: F401
from allsteps_isaaclab_amd.utils.events import EventTermCfg, SceneEntityCfg  # noqa: F401
from allsteps_isaaclab_amd.utils.observations import ObservationGroupCfg, ObservationTermCfg  # noqa: F401
from allsteps_isaaclab_amd.utils.rewards import RewardTermCfg  # noqa: F401
from allsteps_isaaclab_amd.utils.terminations import TerminationTermCfg  # noqa: F401

__all__ = ["EventTermCfg", "SceneEntityCfg", "CommandTermCfg", "ObservationGroupCfg", "ObservationTermCfg",
           "RewardTermCfg", "TerminationTermCfg", "ActionTermCfg"]
