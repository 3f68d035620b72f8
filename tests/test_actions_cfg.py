"""cfg.actions on the host: what envs/actions.py makes of the reference's action term cfgs, and what it refuses.

No GPU: the parsing (ActionTerms over an ActContext), the reference's name resolution with its errors, the column
order and constants of the device table, every refusal with its reason, the manager's table string, the shim exports,
and that the default cfgs add nothing."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

from allsteps_isaaclab_amd import _native  # noqa: E402
from allsteps_isaaclab_amd.envs.actions import (KIND_EFFORT, KIND_EMA, KIND_POSITION, KIND_TO_LIMITS,  # noqa: E402
                                                ActContext, ActionTerms, EnvActions)
from allsteps_isaaclab_amd.utils import actions as AC  # noqa: E402

NAMES = [f"{leg}_{j}" for j in ("HAA", "HFE", "KFE") for leg in ("LF", "LH", "RF", "RH")]
DEFAULT = np.linspace(-0.4, 0.7, 12).astype(np.float32)
LIMITS = np.stack([np.linspace(-1.5, -1.0, 12), np.linspace(1.0, 1.6, 12)], -1).astype(np.float32)
W = {k: i for i, k in enumerate(("joint", "kind", "rescale", "term", "scale", "offset", "clip_lo", "clip_hi", "lim_lo",
                                 "lim_hi", "alpha", "one_minus_alpha"))}


def ctx(actuator=_native.ACT_DC_MOTOR, names=NAMES, action_space=12):
    k = len(names)
    return ActContext(joint_names=list(names), default_joint_pos=np.resize(DEFAULT, k),
                      soft_joint_pos_limits=np.resize(LIMITS, (k, 2)),
                      actuator=actuator, action_space=action_space)


def col(spec, name):
    rows = spec.rows
    return rows.view(np.int32)[:, W[name]] if W[name] < 4 else rows[:, W[name]]


def pos(**kw):
    return AC.JointPositionActionCfg(asset_name="robot", **{"joint_names": [".*"], **kw})


# ------------------------------------------------------------------------------------------------ name resolution
def test_name_resolution_is_the_reference_s():
    names = ["a", "b", "c", "d", "e"]
    assert AC.resolve_matching_names(["a|c", "b"], names) == ([0, 1, 2], ["a", "b", "c"])
    assert AC.resolve_matching_names(["a|c", "b"], names, preserve_order=True) == ([0, 2, 1], ["a", "c", "b"])
    assert AC.resolve_matching_names("d", names) == ([3], ["d"])
    data = {"a|d|e": 1, "b|c": 2}
    assert AC.resolve_matching_names_values(data, names) == ([0, 1, 2, 3, 4], names, [1, 2, 2, 1, 1])
    assert AC.resolve_matching_names_values(data, names, True) == ([0, 3, 4, 1, 2], ["a", "d", "e", "b", "c"],
                                                                   [1, 1, 1, 2, 2])
    with pytest.raises(ValueError, match=r"Multiple matches for 'a': 'a\|c' and '\.\*'!"):
        AC.resolve_matching_names(["a|c", ".*"], names)
    with pytest.raises(ValueError, match="Not all regular expressions are matched!") as e:
        AC.resolve_matching_names(["a", "x.*"], names)
    assert "\tx.*: []\n" in str(e.value) and "\ta: ['a']\n" in str(e.value) and f"Available strings: {names}" in str(e.value)
    with pytest.raises(TypeError, match="should be a dictionary"):
        AC.resolve_matching_names_values(["a"], names)
    assert AC.resolve_matching_names(["a"], ["ab", "a"]) == ([1], ["a"])  # a full match, not a prefix


def test_term_errors_of_the_reference_are_kept():
    with pytest.raises(ValueError, match="Not all regular expressions are matched"):
        ActionTerms({"p": pos(joint_names=["nothing_.*"])}, ctx())
    with pytest.raises(ValueError, match="Multiple matches for 'LF_HAA'"):
        ActionTerms({"p": pos(joint_names=["LF_.*", ".*_HAA", ".*"])}, ctx())
    with pytest.raises(ValueError, match="Not all regular expressions are matched"):
        ActionTerms({"p": pos(scale={"wrong": 1.0})}, ctx())
    with pytest.raises(ValueError, match="Unsupported scale type: <class 'str'>. Supported types are float and dict."):
        ActionTerms({"p": pos(scale="1")}, ctx())
    with pytest.raises(ValueError, match="Unsupported offset type"):
        ActionTerms({"p": pos(offset=[0.0], use_default_offset=False)}, ctx())
    with pytest.raises(ValueError, match="Unsupported clip type: <class 'tuple'>. Supported types are dict."):
        ActionTerms({"p": pos(clip=(-1.0, 1.0))}, ctx())
    ema = lambda a: AC.EMAJointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".*"], alpha=a)  # noqa: E731
    with pytest.raises(ValueError, match=r"Moving average weight must be in the range \[0, 1\]. Got 1.5."):
        ActionTerms({"e": ema(1.5)}, ctx())
    with pytest.raises(ValueError, match=r"Moving average weight must be in the range \[0, 1\]. Got -0.1 for joint "
                                         r"LF_HAA."):
        ActionTerms({"e": ema({"LF_HAA": -0.1})}, ctx())
    with pytest.raises(ValueError, match="Unsupported moving average weight type: <class 'int'>"):
        ActionTerms({"e": ema(1)}, ctx())
    with pytest.raises(TypeError, match="Configuration for the term 'p' is not of type ActionTermCfg"):
        ActionTerms({"p": {"scale": 1.0}}, ctx())
    with pytest.raises(ValueError, match="cfg.action_space = 11 but the terms of cfg.actions take 12 columns"):
        ActionTerms({"p": pos()}, ctx(action_space=11))


# ------------------------------------------------------------------------------------------------ the table
def test_velocity_task_term_and_column_constants():
    spec = ActionTerms({"joint_pos": pos(scale=0.5, use_default_offset=True)}, ctx())
    assert spec.names == ["joint_pos"] and spec.dims == [12] and spec.total == 12 and spec.starts == [0]
    assert spec.rows.shape == (12, _native.ACTION_COLUMN_WORDS) and spec.rows.dtype == np.float32
    assert list(col(spec, "joint")) == list(range(12)) and set(col(spec, "kind")) == {KIND_POSITION}
    assert np.array_equal(col(spec, "scale"), np.full(12, 0.5, np.float32))
    assert np.array_equal(col(spec, "offset"), DEFAULT)
    assert np.all(col(spec, "clip_lo") == -np.inf) and np.all(col(spec, "clip_hi") == np.inf)
    assert np.array_equal(col(spec, "lim_lo"), LIMITS[:, 0]) and np.array_equal(col(spec, "lim_hi"), LIMITS[:, 1])
    # a Python float enters as torch takes it: rounded to float32
    spec = ActionTerms({"p": pos(scale=0.1, offset=0.3, use_default_offset=False)}, ctx())
    assert col(spec, "scale")[0] == np.float32(0.1) and col(spec, "offset")[3] == np.float32(0.3)


def test_dicts_preserve_order_and_two_terms():
    p = pos(joint_names=[".*_KFE", "LF_HAA"], preserve_order=True, scale={".*_KFE": 0.25, "LF_HAA": 2},
            offset={"RF_KFE": -0.5}, use_default_offset=False, clip={"L._KFE": (-0.7, 0.4)})
    rest = [n for n in NAMES if not (n.endswith("_KFE") or n == "LF_HAA")]
    spec = ActionTerms({"first": p, "skipped": None, "rest": AC.JointPositionToLimitsActionCfg(
        asset_name="robot", joint_names=rest, scale=0.9, rescale_to_limits=False)}, ctx())
    assert spec.names == ["first", "rest"] and spec.dims == [5, 7] and spec.starts == [0, 5]
    first = spec.terms[0]
    assert first.joint_names == ["LF_KFE", "LH_KFE", "RF_KFE", "RH_KFE", "LF_HAA"]  # the order of the expressions
    assert first.joint_ids == [8, 9, 10, 11, 0]
    assert list(col(spec, "joint")) == [8, 9, 10, 11, 0] + [NAMES.index(n) for n in rest]
    assert list(col(spec, "term")) == [0] * 5 + [1] * 7
    assert list(col(spec, "scale")[:5]) == [0.25, 0.25, 0.25, 0.25, 2.0]
    assert list(col(spec, "offset")[:5]) == [0.0, 0.0, -0.5, 0.0, 0.0]
    assert list(col(spec, "clip_lo")[:5]) == [np.float32(-0.7), np.float32(-0.7), -np.inf, -np.inf, -np.inf]
    assert list(col(spec, "clip_hi")[:5]) == [np.float32(0.4), np.float32(0.4), np.inf, np.inf, np.inf]
    assert set(col(spec, "kind")[5:]) == {KIND_TO_LIMITS} and not col(spec, "rescale").any()
    # without preserve_order: the order of the joints
    q = pos(joint_names=[".*_KFE", "LF_HAA"], use_default_offset=False)
    assert ActionTerms({"first": q, "rest": spec.terms[1].cfg}, ctx()).terms[0].joint_ids == [0, 8, 9, 10, 11]
    # a configclass-like object in place of the dict: its attributes in order
    ns = type("ActionsCfg", (), {})()
    ns.first, ns.none, ns.rest = q, None, spec.terms[1].cfg
    assert ActionTerms(ns, ctx()).names == ["first", "rest"]


def test_ema_constants_are_formed_as_torch_forms_them():
    e = AC.EMAJointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".*"], alpha=0.8)
    spec = ActionTerms({"e": e}, ctx())
    assert set(col(spec, "kind")) == {KIND_EMA} and col(spec, "rescale").all()
    assert np.all(col(spec, "alpha") == np.float32(0.8))
    assert np.all(col(spec, "one_minus_alpha") == np.float32(1.0 - 0.8))  # a Python scalar: 1 - alpha in double
    e = AC.EMAJointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".*"], alpha={".*_HAA": 0.8})
    spec = ActionTerms({"e": e}, ctx())
    assert list(col(spec, "alpha")[:5]) == [np.float32(0.8)] * 4 + [1.0]
    assert col(spec, "one_minus_alpha")[0] == np.float32(1.0) - np.float32(0.8)  # a tensor: 1 - alpha in float32
    assert np.float32(1.0) - np.float32(0.8) != np.float32(1.0 - 0.8)  # (the two differ, so the test tells them apart)
    assert col(spec, "one_minus_alpha")[4] == 0.0


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("cls, kw, reason", [
    ("RelativeJointPositionActionCfg", {"joint_names": [".*"]}, "re-formed from joint_pos in every physics substep"),
    ("JointVelocityActionCfg", {"joint_names": [".*"]}, r"kd \* \(0 - qd\) and has no velocity target"),
    ("BinaryJointPositionActionCfg", {"joint_names": [".*"]}, "binary joint terms are not served"),
    ("BinaryJointVelocityActionCfg", {"joint_names": [".*"]}, "binary joint terms are not served"),
    ("NonHolonomicActionCfg", {}, "non-holonomic terms are not served"),
    ("DifferentialInverseKinematicsActionCfg", {"joint_names": [".*"]}, "task-space terms are not served"),
    ("OperationalSpaceControllerActionCfg", {"joint_names": [".*"]}, "task-space terms are not served"),
])
def test_refused_term_classes(cls, kw, reason):
    with pytest.raises(_native.NativeError, match=f"cfg.actions term 'bad': {cls} is not served: .*{reason}"):
        ActionTerms({"bad": getattr(AC, cls)(asset_name="robot", **kw)}, ctx())


def test_other_refusals():
    R = _native.NativeError
    with pytest.raises(R, match="cfg.actions term 'p': debug_vis = True"):
        ActionTerms({"p": pos(debug_vis=True)}, ctx())
    with pytest.raises(R, match="cfg.actions term 'p': asset_name = 'arm' is not 'robot'"):
        ActionTerms({"p": AC.JointPositionActionCfg(asset_name="arm", joint_names=[".*"])}, ctx())
    with pytest.raises(R, match="term 'p': a joint position term needs the DC-motor actuator .*kp = kd = 0"):
        ActionTerms({"p": pos()}, ctx(actuator=_native.ACT_TORQUE))
    for cls in (AC.JointPositionToLimitsActionCfg, AC.EMAJointPositionToLimitsActionCfg):
        with pytest.raises(R, match="a joint position term needs the DC-motor actuator"):
            ActionTerms({"p": cls(asset_name="robot", joint_names=[".*"])}, ctx(actuator=_native.ACT_TORQUE))
    eff = AC.JointEffortActionCfg(asset_name="robot", joint_names=[".*"])
    with pytest.raises(R, match="term 'e': a joint effort term needs the torque actuator"):
        ActionTerms({"e": eff}, ctx())
    assert set(col(ActionTerms({"e": eff}, ctx(actuator=_native.ACT_TORQUE)), "kind")) == {KIND_EFFORT}
    with pytest.raises(R, match=r"every joint of the robot exactly once: not commanded \['LH_HAA', 'RF_HAA', "
                                r"'RH_HAA'\], commanded more than once \[\]"):
        ActionTerms({"p": pos(joint_names=[".*_HFE", ".*_KFE", "LF_HAA"])}, ctx(action_space=9))
    with pytest.raises(R, match=r"not commanded \[\], commanded more than once \['LF_HAA'\]"):
        ActionTerms({"p": pos(), "q": pos(joint_names=["LF_HAA"])}, ctx(action_space=13))
    many = [f"j{k:02d}" for k in range(22)]
    with pytest.raises(R, match="cfg.actions has 22 columns .* at most AS_ACT_DIM = 21"):
        ActionTerms({"p": pos(use_default_offset=False)}, ctx(names=many, action_space=22))
    with pytest.raises(R, match="a clip bound is NaN"):
        ActionTerms({"p": pos(clip={".*": (float("nan"), 1.0)})}, ctx())

    class Custom(AC.ActionTermCfg):
        pass

    with pytest.raises(R, match="term 'c': Custom is not one of the served term cfgs"):
        ActionTerms({"c": Custom(asset_name="robot")}, ctx())

    class MyRelative(AC.RelativeJointPositionActionCfg):  # a subclass of a refused cfg is refused with its reason
        pass

    with pytest.raises(R, match="RelativeJointPositionActionCfg is not served"):
        ActionTerms({"r": MyRelative(asset_name="robot", joint_names=[".*"])}, ctx())


# ------------------------------------------------------------------------------------------------ the manager's surface
def test_table_string():
    spec = ActionTerms({"joint_pos": pos()}, ctx())
    assert spec.table_str() == (
        "<ActionManager> contains 1 active terms.\n"
        "+---------------------------------+\n"
        "| Active Action Terms (shape: 12) |\n"
        "+-------+-----------+-------------+\n"
        "| Index | Name      |   Dimension |\n"
        "+-------+-----------+-------------+\n"
        "|   0   | joint_pos |          12 |\n"
        "+-------+-----------+-------------+\n")
    e = AC.JointEffortActionCfg
    two = ActionTerms({"the_legs_of_the_robot": e(asset_name="robot", joint_names=[".*_HAA", ".*_HFE"]),
                       "knees": e(asset_name="robot", joint_names=[".*_KFE"])}, ctx(actuator=_native.ACT_TORQUE))
    assert two.table_str() == (
        "<ActionManager> contains 2 active terms.\n"
        "+-------------------------------------------+\n"
        "|      Active Action Terms (shape: 12)      |\n"
        "+-------+-----------------------+-----------+\n"
        "| Index | Name                  | Dimension |\n"
        "+-------+-----------------------+-----------+\n"
        "|   0   | the_legs_of_the_robot |         8 |\n"
        "|   1   | knees                 |         4 |\n"
        "+-------+-----------------------+-----------+\n")


def test_cfg_classes_have_the_reference_s_fields_and_defaults():
    fields = lambda c: list(c.__dataclass_fields__)  # noqa: E731
    assert fields(AC.ActionTermCfg) == ["asset_name", "debug_vis", "clip"]
    assert fields(AC.JointPositionActionCfg) == ["asset_name", "debug_vis", "clip", "joint_names", "scale", "offset",
                                                 "preserve_order", "use_default_offset"]
    assert fields(AC.JointEffortActionCfg) == fields(AC.JointActionCfg)
    assert fields(AC.EMAJointPositionToLimitsActionCfg) == ["asset_name", "debug_vis", "clip", "joint_names", "scale",
                                                            "rescale_to_limits", "alpha"]
    p = AC.JointPositionActionCfg(asset_name="robot", joint_names=[".*"])
    assert (p.scale, p.offset, p.preserve_order, p.use_default_offset, p.clip, p.debug_vis) == \
        (1.0, 0.0, False, True, None, False)
    e = AC.EMAJointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".*"])
    assert (e.scale, e.rescale_to_limits, e.alpha) == (1.0, True, 1.0)
    assert AC.RelativeJointPositionActionCfg().use_zero_offset is True
    from allsteps_isaaclab_amd.envs.actions import ActionTermView

    assert p.class_type is ActionTermView and e.class_type is ActionTermView


def test_cfg_classes_default_to_none_and_add_nothing():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.actions is None and not EnvActions.wanted(cfg)
    assert DirectRLEnv._action_terms is None and not hasattr(DirectRLEnv, "action_manager")
    env = DirectRLEnv.__new__(DirectRLEnv)
    assert env._actions_get_state() == {}
    assert env._actions_set_state({"q": 1, "action_action": 2, "action_commands": 3, "reward_step": 4,
                                   "action_other": 5}) == {"q": 1, "reward_step": 4, "action_other": 5}


def test_compat_exports():
    code = """
import isaaclab.envs.mdp as mdp
import isaaclab.managers as managers
from isaaclab.managers import ActionTermCfg, TerminationTermCfg, SceneEntityCfg
from allsteps_isaaclab_amd.utils import actions as AC
for name in AC.SERVED + tuple(AC.REFUSED) + ("JointActionCfg",):
    assert getattr(mdp, name) is getattr(AC, name) and name in mdp.__all__, name
assert ActionTermCfg is AC.ActionTermCfg and "ActionTermCfg" in managers.__all__
for name in ("is_alive", "joint_pos", "generated_commands", "height_scan", "push_by_setting_velocity", "time_out"):
    assert hasattr(mdp, name), name  # every name that was there stays
t = mdp.JointPositionActionCfg(asset_name="robot", joint_names=[".*"], scale=0.5, use_default_offset=True)
assert isinstance(t, ActionTermCfg) and t.scale == 0.5
print("ok")
"""
    from allsteps_isaaclab_amd import compat

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([compat.SITE, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_action_kernels_use_no_scratch_and_no_lds(tmp_path):
    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "--cuda-device-only", "-S", "-o", str(tmp_path / "k.s"),
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(_native.CSRC, "allsteps_kernels.hip")],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?):\s+(\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    mine = {k: v for k, v in res.items() if "k_actions_" in k}
    assert len(mine) == 2, sorted(res)
    for name, v in mine.items():
        print(name, v)
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (name, v)
        assert v["Dynamic Stack"] == "False" and int(v["LDS Size [bytes/block]"]) == 0, (name, v)
