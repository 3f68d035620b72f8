"""cfg.rewards on the host: the parser, the resolution of ids and constants, every refusal with its message, the
reference's TypeError cases, the device tables, the compat exports (envs/rewards.py, utils/rewards.py), and the
compiled kernels' resources.  No device."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from allsteps_isaaclab_amd import _native  # noqa: E402
from allsteps_isaaclab_amd.envs.rewards import RewContext, RewardTerms, SensorInfo  # noqa: E402
from allsteps_isaaclab_amd.utils import rewards as RW  # noqa: E402
from allsteps_isaaclab_amd.utils.events import SceneEntityCfg  # noqa: E402

T = RW.RewardTermCfg
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def ctx(**over) -> RewContext:
    j = 12
    lim = np.stack([np.linspace(-1.0, -0.5, j), np.linspace(0.75, 1.25, j)], -1).astype(np.float32)
    base = dict(joint_names=[f"LF_{k}" if k < 6 else f"RH_{k}" for k in range(j)],
                default_joint_pos=np.linspace(-0.5, 0.5, j).astype(np.float32), soft_joint_pos_limits=lim,
                action_cols=12, step_dt=4.0 / 240.0, command_names=["base_velocity", "second"],
                sensors={"sensor": SensorInfo(["RF_FOOT", "LF_FOOT", "RH_FOOT", "LH_FOOT"], [4, 7, 10, 13],
                                              [0, 1, 2, 3])},
                contact_forces=True, contact_air_time=True)
    base.update(over)
    return RewContext(**base)


def fields(row: np.ndarray) -> dict:
    i = row.view(np.int32)
    return {"kind": _native.REW_KINDS[i[0]], "weight": row[1], "num_ids": int(i[2]), "cmd_row": int(i[3]),
            "p0": row[4], "p1": row[5]}


def test_limits_mirror_the_header():
    h = open(os.path.join(ROOT, "include", "allsteps.h")).read()
    for name, value in (("AS_MAX_REW_TERMS", _native.MAX_REW_TERMS), ("AS_MAX_REW_IDS", _native.MAX_REW_IDS),
                        ("AS_REW_TABLE_ROWS", _native.REW_TABLE_ROWS)):
        assert int(re.search(rf"#define {name} (\d+)", h).group(1)) == value
    assert _native.MAX_REW_TERMS == 32
    enum = re.search(r"enum \{\s*AS_REW_IS_ALIVE = 0,(.*?)AS_REW_NUM_KINDS", h, re.S).group(0)
    kinds = [k.lower()[len("as_rew_"):] for k in re.findall(r"AS_REW_[A-Z0-9_]+(?= =|,)", enum)]
    assert kinds == [k.replace("feet_air_time_positive_biped", "feet_air_time_biped").replace("yaw_frame", "yaw")
                     for k in _native.REW_KINDS]
    assert len(kinds) == 21
    assert "as_rewards_step" in _native.EXPORTED_SYMBOLS and "as_rewards_reset" in _native.EXPORTED_SYMBOLS
    assert "#define AS_ABI_VERSION 6" in h or _native.ABI_VERSION == 6


def test_resolution_of_ids_and_constants():
    c = ctx()
    r = RewardTerms({
        "alive": T(func=RW.is_alive, weight=1),
        "skipped": None,
        "height": T(func=RW.base_height_l2, weight=-1.5, params={"target_height": 0.6}),
        "dev": T(func=RW.joint_deviation_l1, weight=-0.1,
                 params={"asset_cfg": SceneEntityCfg("robot", joint_names=["RH_.*"])}),
        "lim": T(func=RW.joint_pos_limits, weight=-1.0,
                 params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[11, 2])}),
        "jv": T(func=RW.joint_vel_l2, weight=-0.001),
        "hits": T(func=RW.undesired_contacts, weight=-1.0,
                  params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("sensor", body_names=".*H_FOOT")}),
        "air": T(func=RW.feet_air_time, weight=0.125,
                 params={"threshold": 0.5, "command_name": "second", "sensor_cfg": SceneEntityCfg("sensor")}),
        "track": T(func=RW.track_lin_vel_xy_exp, weight=1.0, params={"std": 0.3, "command_name": "base_velocity"}),
    }, c)
    assert r.names == ["alive", "height", "dev", "lim", "jv", "hits", "air", "track"]  # None entries are skipped
    assert r.rows.shape == (8, _native.REW_TERM_WORDS) and r.table.shape == (3, 32, 32)
    f = [fields(row) for row in r.rows]
    assert [x["kind"] for x in f] == ["is_alive", "base_height_l2", "joint_deviation_l1", "joint_pos_limits",
                                      "joint_vel_l2", "undesired_contacts", "feet_air_time", "track_lin_vel_xy_exp"]
    assert f[0]["weight"] == np.float32(1.0) and f[1]["p0"] == np.float32(0.6) and f[1]["num_ids"] == 0
    ids = r.table[0].view(np.int32)
    assert ids[2, :6].tolist() == [6, 7, 8, 9, 10, 11] and f[2]["num_ids"] == 6
    assert np.array_equal(r.table[1, 2, :6], c.default_joint_pos[6:])
    assert ids[3, :2].tolist() == [11, 2]  # joint_ids keep their order
    assert np.array_equal(r.table[1, 3, :2], c.soft_joint_pos_limits[[11, 2], 0])
    assert np.array_equal(r.table[2, 3, :2], c.soft_joint_pos_limits[[11, 2], 1])
    assert ids[4, :12].tolist() == list(range(12)) and f[4]["num_ids"] == 12
    assert ids[5, :2].tolist() == [10, 13]  # the sensor's bodies 2, 3 as rows of the net forces
    assert ids[6, :4].tolist() == [0, 1, 2, 3] and f[6]["cmd_row"] == 3  # timer rows; the second command term
    assert f[6]["p1"] == np.float32(4.0 / 240.0 + 1.0e-8) and f[6]["p0"] == np.float32(0.5)
    assert f[7]["p0"] == np.float32(0.3 ** 2)  # std**2 in double, then cast
    assert r.kinds == sum(1 << _native.REW_KINDS.index(x["kind"]) for x in f)


def test_configclass_like_objects_and_set_term():
    class Rewards:
        alive = T(func=RW.is_alive, weight=1.0)
        act = T(func=RW.action_rate_l2, weight=-0.01)

    r = RewardTerms(Rewards(), ctx())
    assert r.names == ["alive", "act"] and r.index("act") == 1
    with pytest.raises(ValueError, match="Reward term 'nope' not found."):
        r.index("nope")
    s = r.table_str()
    assert "<RewardManager> contains 2 active terms." in s and "Active Reward Terms" in s and "-0.01" in s


def test_served_functions_are_the_issues_twenty_one():
    assert len(RW.SERVED) == 21 and "track_lin_vel_xy_yaw_frame_exp" in RW.SERVED
    r = RewardTerms({"yaw": T(func=RW.track_lin_vel_xy_yaw_frame_exp, weight=1.0,
                              params={"std": 0.5, "command_name": "second"})}, ctx())
    f = fields(r.rows[0])
    assert f["kind"] == "track_lin_vel_xy_yaw_frame_exp" and f["cmd_row"] == 3 and f["p0"] == np.float32(0.25)


REFUSALS = [
    (T(func=RW.joint_torques_l2, weight=1.0), "joint_torques_l2: the step keeps no applied torque"),
    (T(func=RW.applied_torque_limits, weight=1.0), "applied_torque_limits: the step keeps no applied torque"),
    (T(func=RW.joint_vel_limits, weight=1.0, params={"soft_ratio": 0.9}), "joint_vel_limits: the views have no soft"),
    (T(func=RW.body_lin_acc_l2, weight=1.0), "body_lin_acc_l2"),
    (T(func=RW.feet_slide, weight=1.0), "feet_slide"),
    (T(func=RW.is_terminated_term, weight=1.0), "is_terminated_term: there is no termination manager"),
    (T(func=RW.base_height_l2, weight=1.0, params={"target_height": 0.5, "sensor_cfg": SceneEntityCfg("height_scanner")}),
     "base_height_l2 with a sensor_cfg"),
    (T(func=lambda env: None, weight=1.0), "is not a served term function"),
    (T(func=RW.joint_vel_l2, weight=1.0, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[12])}),
     r"joint_ids \[12\] outside"),
    (T(func=RW.joint_vel_l2, weight=1.0, params={"asset_cfg": SceneEntityCfg("cube")}), "is not 'robot'"),
    (T(func=RW.base_height_l2, weight=1.0, params={"target_height": "high"}), "target_height = 'high' is not a number"),
    (T(func=RW.base_height_l2, weight=1.0), r"needs params \['target_height'\]"),
    (T(func=RW.is_alive, weight=1.0, params={"extra": 1}), r"params \['extra'\] are not parameters"),
    (T(func=RW.undesired_contacts, weight=1.0, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("other")}),
     "names the sensor 'other'"),
    (T(func=RW.track_ang_vel_z_exp, weight=1.0, params={"std": 0.5, "command_name": "nope"}),
     "command_name = 'nope' names no command term of cfg.commands"),
]


@pytest.mark.parametrize("cfg, message", REFUSALS, ids=[m[:24] for _, m in REFUSALS])
def test_refusals_name_the_term_and_the_reason(cfg, message):
    with pytest.raises(_native.NativeError, match=message) as e:
        RewardTerms({"bad_term": cfg}, ctx())
    assert "cfg.rewards term 'bad_term'" in str(e.value) and "no host fallback" in str(e.value)


def test_terms_whose_sensor_or_command_is_not_configured_name_the_field():
    hits = T(func=RW.contact_forces, weight=1.0, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("sensor")})
    air = T(func=RW.feet_air_time_positive_biped, weight=1.0,
            params={"threshold": 0.4, "command_name": "base_velocity", "sensor_cfg": SceneEntityCfg("sensor")})
    track = T(func=RW.track_ang_vel_z_world_exp, weight=1.0, params={"std": 0.5, "command_name": "base_velocity"})
    acc = T(func=RW.joint_acc_l2, weight=1.0)
    for cfg, over, field in ((hits, {"contact_forces": False}, "cfg.contact_forces"),
                             (acc, {"contact_forces": False}, "cfg.contact_forces"),
                             (air, {"contact_air_time": False}, "cfg.contact_air_time"),
                             (track, {"command_names": []}, "cfg.commands")):
        with pytest.raises(_native.NativeError, match=field):
            RewardTerms({"t": cfg}, ctx(**over))
        RewardTerms({"t": cfg}, ctx())  # served once the field is set


def test_limits_are_refused():
    many = {f"t{k}": T(func=RW.is_alive, weight=1.0) for k in range(_native.MAX_REW_TERMS + 1)}
    with pytest.raises(_native.NativeError, match="33 terms; the reward kernel takes at most AS_MAX_REW_TERMS = 32"):
        RewardTerms(many, ctx())
    RewardTerms(dict(list(many.items())[:32]), ctx())
    j = _native.MAX_REW_IDS + 1
    wide = ctx(joint_names=[f"j{k}" for k in range(j)], default_joint_pos=np.zeros(j, np.float32),
               soft_joint_pos_limits=np.zeros((j, 2), np.float32))
    with pytest.raises(_native.NativeError, match="selects 33 joints or bodies; the index table holds"):
        RewardTerms({"t": T(func=RW.joint_vel_l1, weight=1.0)}, wide)
    with pytest.raises(_native.NativeError, match="there are no terms"):
        RewardTerms({"t": None}, ctx())


def test_type_errors_are_the_references():
    with pytest.raises(TypeError, match="Configuration for the term 'x' is not of type RewardTermCfg. Received: "
                                        "'<class 'dict'>'."):
        RewardTerms({"x": {"func": RW.is_alive}}, ctx())
    with pytest.raises(TypeError, match="Weight for the term 'x' is not of type float or int. Received: "
                                        "'<class 'str'>'."):
        RewardTerms({"x": T(func=RW.is_alive, weight="1")}, ctx())
    with pytest.raises(TypeError, match="Weight for the term 'x'"):
        RewardTerms({"x": T(func=RW.is_alive)}, ctx())  # MISSING
    RewardTerms({"x": T(func=RW.is_alive, weight=2)}, ctx())  # an int is a weight


def test_compat_exports():
    code = """
import isaaclab.envs.mdp as mdp
from isaaclab.managers import RewardTermCfg, SceneEntityCfg
from allsteps_isaaclab_amd.utils import rewards as RW
for name in RW.SERVED + tuple(RW.REFUSED):
    assert getattr(mdp, name) is getattr(RW, name), name
assert RewardTermCfg is RW.RewardTermCfg
t = RewardTermCfg(func=mdp.is_alive, weight=1.0)
assert t.params == {} and [f for f in t.__dataclass_fields__] == ["func", "params", "weight"]
print("ok")
"""
    from allsteps_isaaclab_amd import compat

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([compat.SITE, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_cfg_classes_default_to_none_and_add_nothing():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.envs.rewards import EnvRewards

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.rewards is None and cfg.rewards_replace_task_reward is False
        assert not EnvRewards.wanted(cfg)
    assert DirectRLEnv._rewards is None and not hasattr(DirectRLEnv, "reward_manager")
    env = DirectRLEnv.__new__(DirectRLEnv)
    assert env._rewards_get_state() == {} and env._rewards_set_state({"q": 1, "reward_step": 2}) == {"q": 1}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_reward_kernels_use_no_scratch_and_spill_no_vgpr(tmp_path):
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
    mine = {k: v for k, v in res.items() if "k_rewards_step" in k or "k_rewards_reset" in k}
    assert len(mine) == 2, sorted(res)
    for name, v in mine.items():
        print(name, v)
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (name, v)
        assert v["Dynamic Stack"] == "False", (name, v)
