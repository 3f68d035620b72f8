"""envs/_manager.py: the cfg walk, the state mixin and u8 that the env managers share.  CPU only, no device.

The walk's expectations are what the managers' own copies of it gave before they were merged: their orders, their
skips and their TypeError texts, asked of ``cfg_items`` directly and of every manager through its own entry point."""

import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allsteps_isaaclab_amd.envs._manager import DeviceState, cfg_items, is_number, u8  # noqa: E402
from allsteps_isaaclab_amd.utils import actions as AC  # noqa: E402
from allsteps_isaaclab_amd.utils import commands as CM  # noqa: E402
from allsteps_isaaclab_amd.utils import events as E  # noqa: E402
from allsteps_isaaclab_amd.utils import noise as NZ  # noqa: E402
from allsteps_isaaclab_amd.utils import observations as OB  # noqa: E402
from allsteps_isaaclab_amd.utils import rewards as RW  # noqa: E402
from allsteps_isaaclab_amd.utils import terminations as TM  # noqa: E402


class Term:
    def __init__(self, tag=""):
        self.tag = tag


def _names(obj, **kw):
    return [k for k, _ in cfg_items(obj, Term, **kw)]


# ------------------------------------------------------------------ the walk itself
def test_a_dict_keeps_its_order_and_loses_its_none_entries():
    d = {"z": Term(), "a": Term(), "off": None, "m": Term()}
    assert _names(d) == ["z", "a", "m"]
    assert [v for _, v in cfg_items(d, Term)] == [d["z"], d["a"], d["m"]]


def _classes():
    class Base:
        b_first = Term("base.b_first")
        shared = Term("base.shared")
        off = None
        _hidden = Term()
        number = 3  # (a class attribute of another type is no entry and no error)

    class Derived(Base):
        d_term = Term("derived.d_term")
        shared = Term("derived.shared")

    return Base, Derived


def test_class_level_terms_come_base_classes_first_each_name_once():
    Base, Derived = _classes()
    assert _names(Base()) == ["b_first", "shared"]
    assert _names(Derived()) == ["b_first", "shared", "d_term"]
    # the name is met in the base class first, and the first one met is the one taken -- as every copy of the walk did
    assert dict(cfg_items(Derived(), Term))["shared"].tag == "base.shared"


def test_instance_level_terms_come_first_and_hide_class_level_ones_of_their_name():
    Base, Derived = _classes()
    only = SimpleNamespace(y=Term(), x=Term(), gone=None)
    assert _names(only) == ["y", "x"]
    both = Derived()
    both.inst, both.d_term, both.gone = Term("inst"), Term("inst.d_term"), None
    assert _names(both) == ["inst", "d_term", "b_first", "shared"]
    assert dict(cfg_items(both, Term))["d_term"].tag == "inst.d_term"
    assert _names(both, class_attrs=False) == ["inst", "d_term"]


def test_private_names_are_skipped_or_kept_by_argument():
    obj = SimpleNamespace(a=Term(), _p=Term())
    d = {"a": Term(), "_p": Term()}
    assert _names(obj) == ["a"] and _names(d) == ["a"]  # "skip", the default
    assert _names(obj, private="attrs") == ["a"] and _names(d, private="attrs") == ["a", "_p"]
    assert _names(obj, private="keep") == ["a", "_p"] and _names(d, private="keep") == ["a", "_p"]
    # a skipped name is not type-checked; a kept one is
    assert _names({"a": Term(), "_n": 3}) == ["a"]
    with pytest.raises(TypeError, match="'_n'"):
        _names({"a": Term(), "_n": 3}, private="attrs")
    Base, _ = _classes()
    assert "_hidden" not in _names(Base(), private="keep")  # a class's private attributes never count


def test_ignored_names_and_the_error_hook_and_the_laziness_of_the_walk():
    d = {"setting": True, "a": Term(), "bad": 3, "b": Term()}
    with pytest.raises(TypeError) as e:
        _names(d)
    assert str(e.value) == "Configuration for the term 'setting' is not of type Term. Received: '<class 'bool'>'."
    walk = cfg_items(d, Term, ignore=("setting",), error=lambda k, v: KeyError(f"{k}={v}"))
    assert next(walk)[0] == "a"  # the entries ahead of a wrong one are yielded before it raises
    with pytest.raises(KeyError, match="bad=3"):
        next(walk)
    # term_type may be a tuple of types
    assert [k for k, _ in cfg_items({"g": {}, "t": Term()}, (Term, dict))] == ["g", "t"]


# ------------------------------------------------------------------ every manager through its own entry point
def _event():
    return E.EventTermCfg(func=E.push_by_setting_velocity, mode="interval", interval_range_s=(1.0, 2.0),
                          params={"velocity_range": {"x": (-1.0, 1.0)}})


def _command():
    U = CM.UniformVelocityCommandCfg
    return U(asset_name="robot", resampling_time_range=(1.0, 2.0), heading_command=False,
             ranges=U.Ranges(lin_vel_x=(0.0, 1.0), lin_vel_y=(0.0, 1.0), ang_vel_z=(0.0, 1.0)))


def _reward():
    return RW.RewardTermCfg(func=RW.is_alive, weight=1.0)


def _termination():
    return TM.TerminationTermCfg(func=TM.time_out, time_out=True)


def _observation():
    return OB.ObservationTermCfg(func=OB.base_lin_vel)


def _action():
    return AC.JointEffortActionCfg(asset_name="robot", joint_names=[".*"])


JOINTS = ["hip", "knee"]
LIMITS = np.array([[-1.0, 1.0], [-2.0, 2.0]], np.float32)


def _events(cfg):
    from allsteps_isaaclab_amd.envs.events import EventTerms

    return EventTerms(cfg).names


def _commands(cfg):
    from allsteps_isaaclab_amd.envs.commands import CommandTerms

    return CommandTerms(cfg, 0.02).names


def _rew_ctx():
    from allsteps_isaaclab_amd.envs.rewards import RewContext

    return RewContext(joint_names=JOINTS, default_joint_pos=np.zeros(2, np.float32), soft_joint_pos_limits=LIMITS,
                      action_cols=2, step_dt=0.02)


def _rewards(cfg):
    from allsteps_isaaclab_amd.envs.rewards import RewardTerms

    return RewardTerms(cfg, _rew_ctx()).names


def _term_ctx():
    from allsteps_isaaclab_amd.envs.terminations import TermContext

    return TermContext(joint_names=JOINTS, soft_joint_pos_limits=LIMITS, step_dt=0.02, max_episode_length=10)


def _terminations(cfg):
    from allsteps_isaaclab_amd.envs.terminations import TerminationTerms

    return TerminationTerms(cfg, _term_ctx()).names


def _obs_ctx():
    from allsteps_isaaclab_amd.envs.observations import ObsContext

    return ObsContext(joint_names=JOINTS, default_joint_pos=np.zeros(2, np.float32),
                      default_joint_vel=np.zeros(2, np.float32), soft_joint_pos_limits=LIMITS, action_cols=2)


def _observation_groups(cfg):
    from allsteps_isaaclab_amd.envs.observations import ObservationGroups

    return ObservationGroups(cfg, _obs_ctx()).names


def _observation_terms(cfg):
    from allsteps_isaaclab_amd.envs.observations import ObservationGroups

    return ObservationGroups({"g": cfg}, _obs_ctx()).groups[0].names


def _actions(cfg):
    from allsteps_isaaclab_amd.envs.actions import named_terms

    return [k for k, _ in named_terms(cfg)]


TERM = "Configuration for the term 'a' is not of type {}. Received: '<class 'int'>'."


@pytest.mark.parametrize("build, text", [
    (_events, TERM.format("EventTermCfg")), (_commands, TERM.format("CommandTermCfg")),
    (_rewards, TERM.format("RewardTermCfg")), (_terminations, TERM.format("TerminationTermCfg")),
    (_observation_terms, TERM.format("ObservationTermCfg")), (_actions, TERM.format("ActionTermCfg")),
    (_observation_groups, "Observation group 'a' is not of type 'ObservationGroupCfg'. Received: '<class 'int'>'."),
], ids=["events", "commands", "rewards", "terminations", "observation_terms", "actions", "observation_groups"])
def test_a_non_term_entry_raises_the_managers_type_error(build, text):
    with pytest.raises(TypeError) as e:
        build({"a": 3})
    assert str(e.value) == text


def _object(term, base=object):
    class Base(base):
        b_first = term()
        shared = term()
        off = None
        _hidden = term()

    class Derived(Base):
        d_term = term()
        shared = term()

        def __init__(self):
            self.inst = term()
            self.inst_none = None
            self._private = term()

    return Derived()


@pytest.mark.parametrize("build, term, base", [
    (_events, _event, object), (_commands, _command, object), (_rewards, _reward, object),
    (_terminations, _termination, object), (_observation_terms, _observation, OB.ObservationGroupCfg),
], ids=["events", "commands", "rewards", "terminations", "observation_terms"])
def test_the_managers_walk_a_cfg_object_alike(build, term, base):
    assert build(_object(term, base)) == ["inst", "b_first", "shared", "d_term"]


def test_the_differences_between_the_managers_that_are_kept():
    # a dict key that begins with "_": the rewards and the terminations take it as a term, the others pass over it
    assert _rewards({"a": _reward(), "_b": _reward()}) == ["a", "_b"]
    assert _terminations({"a": _termination(), "_b": _termination()}) == ["a", "_b"]
    assert _events({"a": _event(), "_b": _event()}) == ["a"]
    assert _commands({"a": _command(), "_b": _command()}) == ["a"]
    assert _observation_terms({"a": _observation(), "_b": _observation()}) == ["a"]
    # the actions read neither class attributes nor pass over private names
    assert _actions(_object(_action)) == ["inst", "_private"]
    assert _actions({"a": _action(), "_b": _action(), "c": None}) == ["a", "_b"]
    # a group's settings are no terms, in a dict or on an object
    assert _observation_terms({"enable_corruption": False, "history_length": 2, "a": _observation()}) == ["a"]


# ------------------------------------------------------------------ is_number, u8
def test_is_number_and_u8():
    assert all(is_number(x) for x in (1, 2.5, np.float32(1), np.int64(3)))
    assert not any(is_number(x) for x in (True, "1", None, (1,), np.bool_(True)))
    assert u8(None) is None
    b = torch.tensor([True, False, True])
    assert u8(b).dtype == torch.uint8 and u8(b).data_ptr() == b.data_ptr()  # a view, no copy
    i = torch.tensor([0, 2, 1], dtype=torch.int32)
    assert u8(i).dtype == torch.uint8 and u8(i).tolist() == [0, 2, 1]
    strided = torch.zeros(4, 2, dtype=torch.bool)[:, 0]
    assert not strided.is_contiguous() and u8(strided).is_contiguous()
    c = torch.zeros(5, dtype=torch.uint8)
    assert u8(c) is c


# ------------------------------------------------------------------ the state mixin
class Part(DeviceState):
    STATE_KEYS = ("p_a", "p_b", "p_absent")

    def __init__(self):
        self.a = torch.zeros(2, 3, dtype=torch.float32)
        self.b = torch.zeros(4, dtype=torch.int32)

    def tensors(self):
        return {"p_a": self.a, "p_b": self.b}


def test_set_state_loads_what_it_is_given_into_the_tensors_in_place():
    p = Part()
    a_ptr, b_ptr = p.a.data_ptr(), p.b.data_ptr()
    st = p.get_state()
    assert sorted(st) == ["p_a", "p_b"] and st["p_a"].data_ptr() != a_ptr  # clones
    # another dtype, another shape, and not a tensor of the part's device at all (numpy, a list)
    assert p.set_state({"p_a": torch.arange(6, dtype=torch.float64), "p_b": np.array([[1, 2], [3, 4]], np.int64)})
    assert p.a.dtype == torch.float32 and p.a.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    assert p.b.dtype == torch.int32 and p.b.tolist() == [1, 2, 3, 4]
    assert p.set_state({"p_b": [7, 7, 7, 7], "root_pos": 0}) and p.b.tolist() == [7, 7, 7, 7]
    assert (p.a.data_ptr(), p.b.data_ptr()) == (a_ptr, b_ptr)
    # a missing key leaves its tensor alone; nothing of the part in the dict: nothing loaded
    assert p.a.tolist()[1] == [3.0, 4.0, 5.0]
    assert p.set_state({"root_pos": 0, "p_absent": 1}) is False
    with pytest.raises(RuntimeError):
        p.set_state({"p_b": torch.zeros(5)})  # a size that cannot be the tensor's is an error, not a truncation


def test_owns_by_keys_and_by_prefix():
    class ByPrefix(DeviceState):
        STATE_PREFIX = "thing_"

    assert Part.owns("p_a") and Part.owns("p_absent") and not Part.owns("p_other") and not Part.owns("q")
    assert ByPrefix.owns("thing_x") and ByPrefix.owns("thing_") and not ByPrefix.owns("thin") and not ByPrefix.owns("q")
    assert not DeviceState.owns("anything")
    with pytest.raises(NotImplementedError):
        DeviceState().get_state()


def _cpu_env_cfg():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.sim.device, cfg.scene.num_envs, cfg.seed = "cpu", 4, 3
    bias = NZ.NoiseModelWithAdditiveBiasCfg(noise_cfg=NZ.GaussianNoiseCfg(mean=0.0, std=0.1),
                                            bias_noise_cfg=NZ.GaussianNoiseCfg(mean=0.0, std=0.1))
    cfg.action_noise_model = cfg.observation_noise_model = bias
    cfg.events, cfg.commands = {"push": _event()}, {"vel": _command()}
    cfg.observations = {"g": {"a": _observation()}, "h": {"a": _observation()}}
    cfg.rewards, cfg.terminations, cfg.actions = {"a": _reward()}, {"a": _termination()}, {"a": _action()}
    return cfg


# what told a manager's keys from the others before DeviceState.owns: STATE_KEYS membership or is_state_key
OLD_RULES = {
    "_noise": lambda k: k in ("noise_t", "noise_action_bias", "noise_obs_bias"),
    "_events": lambda k: k in ("event_t", "event_time_left"),
    "_commands": lambda k: k in ("command_t", "command_time_left", "command_vel_b", "command_heading_target",
                                 "command_flags", "command_counter", "command_metrics", "command_last_metrics"),
    "_observations": lambda k: k.startswith("observation_"),
    "_rewards": lambda k: k.startswith("reward_"),
    "_terminations": lambda k: k.startswith("termination_"),
    "_action_terms": lambda k: k.startswith("action_") and k[len("action_"):] in (
        "action", "prev_action", "processed", "prev_applied", "commands"),
}


def test_owns_agrees_with_the_old_rules_and_the_env_merges_and_filters_by_it():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.actions import ActContext
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv, _part_classes

    class Env(DirectRLEnv):  # the hooks the managers ask, from host facts alone
        _actions_clamped = False

        def _observations_context(self):
            return _obs_ctx()

        def _rewards_context(self):
            return _rew_ctx()

        def _terminations_context(self):
            return _term_ctx()

        def _actions_context(self):
            return ActContext(joint_names=JOINTS, default_joint_pos=np.zeros(2, np.float32),
                              soft_joint_pos_limits=LIMITS, actuator=_native.ACT_TORQUE)

    env = Env(_cpu_env_cfg())
    env._observations_start(), env._rewards_start(), env._terminations_start()
    from allsteps_isaaclab_amd.envs.actions import EnvActions

    env._action_terms = EnvActions(env.cfg, env, env.num_envs, env._device)  # (_actions_start also launches a reset)
    classes = _part_classes()
    assert list(classes) == list(OLD_RULES)
    emitted = {attr: list(getattr(env, attr).tensors()) for attr in classes}
    assert all(emitted.values())
    everything = [k for keys in emitted.values() for k in keys] + ["root_pos", "contact_timers", "action_other"]
    for attr, cls in classes.items():
        for k in everything:
            assert cls.owns(k) == OLD_RULES[attr](k), (attr, k)
        assert all(cls.owns(k) for k in emitted[attr])
    # get_state's part: every part's keys, in the order of the classes
    st = env._parts_get_state()
    assert list(st) == [k for keys in emitted.values() for k in keys]
    # set_state's part: loaded in place, the parts' keys taken out, the rest handed back in their order
    st["reward_episode_sums"] = st["reward_episode_sums"] + 2
    st["noise_t"] = st["noise_t"].double() + 5
    rest = env._parts_set_state({"root_pos": 1, **st, "action_other": 2, "q": 3})
    assert list(rest) == ["root_pos", "action_other", "q"]
    assert bool((env._rewards.episode_sums == 2).all()) and env._noise.t.tolist() == [5] * 4
    assert env._events.started
    # an env built without the managers drops their keys all the same
    bare = DirectRLEnv.__new__(DirectRLEnv)
    assert bare._parts_get_state() == {} and bare._parts_set_state({"root_pos": 1, **st}) == {"root_pos": 1}
    # _reseed: the parts that draw, and only those
    env._reseed(11)
    assert [a for a in classes if hasattr(getattr(env, a), "seed")] == ["_noise", "_events", "_commands",
                                                                       "_observations"]
    assert all(getattr(env, a).seed == 11 for a in ("_noise", "_events", "_commands", "_observations"))
