"""cfg.terminations on the host: the parser, the resolution of ids and constants, every refusal with its message, the
reference's TypeError, the device tables, set_term_cfg's rules, the quadruped's refusal of terminations_reset, the
compat exports (envs/terminations.py, utils/terminations.py), and the compiled kernel's resources.  No device."""

import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from allsteps_isaaclab_amd import _native  # noqa: E402
from allsteps_isaaclab_amd.envs.terminations import (  # noqa: E402
    EnvTerminations, SensorInfo, TermContext, TerminationManagerView, TerminationTerms)
from allsteps_isaaclab_amd.utils import terminations as TM  # noqa: E402
from allsteps_isaaclab_amd.utils.events import SceneEntityCfg  # noqa: E402

T = TM.TerminationTermCfg
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def ctx(**over) -> TermContext:
    j = 12
    lim = np.stack([np.linspace(-1.0, -0.5, j), np.linspace(0.75, 1.25, j)], -1).astype(np.float32)
    base = dict(joint_names=[f"LF_{k}" if k < 6 else f"RH_{k}" for k in range(j)], soft_joint_pos_limits=lim,
                step_dt=4.0 / 240.0, max_episode_length=1200, command_names=["base_velocity", "second"],
                sensors={"sensor": SensorInfo(["RF_FOOT", "LF_FOOT", "RH_FOOT", "LH_FOOT"], [4, 7, 10, 13]),
                         "contact_forces": SensorInfo(["base", "LF_HIP", "LF_THIGH"], [0, 1, 2])},
                contact_forces=True)
    base.update(over)
    return TermContext(**base)


def fields(row: np.ndarray) -> dict:
    i = row.view(np.int32)
    return {"kind": _native.TERMINATION_KINDS[i[0]], "time_out": int(i[1]), "num_ids": int(i[2]), "row": int(i[3]),
            "p0": row[4], "p1": row[5], "i0": int(i[6])}


def test_limits_mirror_the_header():
    h = open(os.path.join(ROOT, "include", "allsteps.h")).read()
    for name, value in (("AS_MAX_TERMINATION_TERMS", _native.MAX_TERMINATION_TERMS),
                        ("AS_MAX_TERMINATION_IDS", _native.MAX_TERMINATION_IDS),
                        ("AS_TERMINATION_TABLE_ROWS", _native.TERMINATION_TABLE_ROWS)):
        assert int(re.search(rf"#define {name} (\d+)", h).group(1)) == value
    assert _native.MAX_TERMINATION_TERMS == 16 and _native.MAX_TERMINATION_IDS == 32
    enum = re.search(r"enum \{\s*AS_TERMINATION_TIME_OUT = 0,(.*?)AS_TERMINATION_NUM_KINDS", h, re.S).group(0)
    kinds = [k.lower()[len("as_termination_"):] for k in re.findall(r"AS_TERMINATION_[A-Z0-9_]+(?= =|,)", enum)]
    assert kinds == list(_native.TERMINATION_KINDS) == list(TM.SERVED) and len(kinds) == 8
    assert "as_terminations_step" in _native.EXPORTED_SYMBOLS
    assert "#define AS_ABI_VERSION 6" in h or _native.ABI_VERSION == 6


def test_resolution_of_ids_and_constants():
    c = ctx()
    r = TerminationTerms({
        "time_out": T(func=TM.time_out, time_out=True),
        "skipped": None,
        "resample": T(func=TM.command_resample, params={"command_name": "second", "num_resamples": 3}),
        "tilt": T(func=TM.bad_orientation, params={"limit_angle": 0.7}),
        "low": T(func=TM.root_height_below_minimum, params={"minimum_height": 0.3, "asset_cfg": SceneEntityCfg("robot")}),
        "lim": T(func=TM.joint_pos_out_of_limit, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[11, 2])}),
        "manual": T(func=TM.joint_pos_out_of_manual_limit,
                    params={"bounds": (-1.3, 1.4), "asset_cfg": SceneEntityCfg("robot", joint_names=["RH_.*"])}),
        "vel": T(func=TM.joint_vel_out_of_manual_limit, params={"max_velocity": 30}),
        "base_contact": T(func=TM.illegal_contact,
                          params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("contact_forces", body_names="base")}),
        "feet": T(func=TM.illegal_contact,
                  params={"threshold": 500.0, "sensor_cfg": SceneEntityCfg("sensor", body_names=".*H_FOOT")}),
    }, c)
    assert r.names == ["time_out", "resample", "tilt", "low", "lim", "manual", "vel", "base_contact", "feet"]
    assert r.rows.shape == (9, _native.TERMINATION_TERM_WORDS) and r.table.shape == (3, 16, 32)
    f = [fields(row) for row in r.rows]
    assert [x["kind"] for x in f] == ["time_out", "command_resample", "bad_orientation", "root_height_below_minimum",
                                      "joint_pos_out_of_limit", "joint_pos_out_of_manual_limit",
                                      "joint_vel_out_of_manual_limit", "illegal_contact", "illegal_contact"]
    assert [x["time_out"] for x in f] == [1] + [0] * 8
    assert f[0]["i0"] == 1200
    assert f[1]["row"] == 1 and f[1]["i0"] == 3 and f[1]["p0"] == np.float32(4.0 / 240.0)  # the second command term
    assert f[2]["p0"] == np.float32(0.7) and f[3]["p0"] == np.float32(0.3)  # Python scalars enter as float32
    ids = r.table[0].view(np.int32)
    assert ids[4, :2].tolist() == [11, 2] and f[4]["num_ids"] == 2  # joint_ids keep their order
    assert np.array_equal(r.table[1, 4, :2], c.soft_joint_pos_limits[[11, 2], 0])
    assert np.array_equal(r.table[2, 4, :2], c.soft_joint_pos_limits[[11, 2], 1])
    assert ids[5, :6].tolist() == [6, 7, 8, 9, 10, 11] and f[5]["p0"] == np.float32(-1.3) and f[5]["p1"] == np.float32(1.4)
    assert ids[6, :12].tolist() == list(range(12)) and f[6]["num_ids"] == 12 and f[6]["p0"] == np.float32(30.0)
    assert ids[7, :1].tolist() == [0] and f[7]["num_ids"] == 1  # the all-body sensor's base
    assert ids[8, :2].tolist() == [10, 13]  # the foot sensor's bodies 2, 3 as rows of the net forces
    assert r.kinds == sum(1 << k for k in {_native.TERMINATION_KINDS.index(x["kind"]) for x in f})
    assert r.uses("illegal_contact") and not TerminationTerms({"t": T(func=TM.time_out)}, c).uses("illegal_contact")


def test_configclass_like_objects_and_the_table():
    class Terminations:
        time_out = T(func=TM.time_out, time_out=True)
        base_contact = T(func=TM.illegal_contact,
                         params={"sensor_cfg": SceneEntityCfg("contact_forces", body_names="base"), "threshold": 1.0})

    r = TerminationTerms(Terminations(), ctx())
    assert r.names == ["time_out", "base_contact"] and r.index("base_contact") == 1
    with pytest.raises(ValueError, match="Termination term 'nope' not found."):
        r.index("nope")
    s = r.table_str()
    assert "<TerminationManager> contains 2 active terms." in s and "Active Termination Terms" in s
    assert "Time Out" in s and "True" in s and "False" in s


class _Klass:
    def __init__(self, cfg=None, env=None):
        pass

    def __call__(self, env):
        return None

    def reset(self, env_ids=None):
        pass


REFUSALS = [
    (T(func=TM.joint_effort_out_of_limit), "joint_effort_out_of_limit: the step keeps no applied torque"),
    (T(func=TM.joint_vel_out_of_limit), "joint_vel_out_of_limit: the views have no soft joint velocity limits"),
    (T(func=_Klass), "is a class-based term"),
    (T(func=_Klass()), "is a class-based term"),
    (T(func=lambda env: None), "is not a served term function"),
    (T(), "func = .* is not callable"),  # MISSING
    (T(func=3), "func = 3 is not callable"),
    (T(func=TM.time_out, params=[1]), r"params = \[1\] is not a dict"),
    (T(func=TM.bad_orientation, params={"limit_angle": 0.5, "asset_cfg": "robot"}),
     r"params\['asset_cfg'\] = 'robot' is not a SceneEntityCfg"),
    (T(func=TM.joint_pos_out_of_limit, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[])}),
     "asset_cfg selects no joint"),
    (T(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("sensor", body_ids=[])}),
     "sensor_cfg selects no body"),
    (T(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("sensor", body_ids=[4])}),
     r"body_ids \[4\] outside"),
    (T(func=TM.command_resample, params={"command_name": "second", "num_resamples": True}),
     "num_resamples = True is not an int"),
    (T(func=TM.joint_pos_out_of_manual_limit, params={"bounds": (None, 1.0)}), r"bounds\[0\] = None is not a number"),
    (T(func=TM.illegal_contact, params={"sensor_cfg": SceneEntityCfg("sensor")}), r"needs params \['threshold'\]"),
    (T(func=TM.time_out, time_out=1), "time_out = 1 is not a bool"),
    (T(func=TM.time_out, params={"extra": 1}), r"params \['extra'\] are not parameters"),
    (T(func=TM.bad_orientation), r"needs params \['limit_angle'\]"),
    (T(func=TM.bad_orientation, params={"limit_angle": "steep"}), "limit_angle = 'steep' is not a number"),
    (T(func=TM.root_height_below_minimum, params={"minimum_height": 0.3, "asset_cfg": SceneEntityCfg("cube")}),
     "is not 'robot'"),
    (T(func=TM.joint_pos_out_of_manual_limit, params={"bounds": 1.0}), r"bounds = 1.0 is not a \(lower, upper\) pair"),
    (T(func=TM.joint_vel_out_of_manual_limit,
       params={"max_velocity": 1.0, "asset_cfg": SceneEntityCfg("robot", joint_ids=[12])}), r"joint_ids \[12\] outside"),
    (T(func=TM.joint_pos_out_of_limit, params={"asset_cfg": SceneEntityCfg("robot", joint_names=["nope"])}),
     r"joint_names \['nope'\] match no joint"),
    (T(func=TM.command_resample, params={"command_name": "nope"}),
     "command_name = 'nope' names no command term of cfg.commands"),
    (T(func=TM.command_resample, params={"command_name": "second", "num_resamples": 1.5}),
     "num_resamples = 1.5 is not an int"),
    (T(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("other")}),
     "names the sensor 'other'"),
    (T(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("sensor", body_names="trunk")}),
     r"body_names \['trunk'\] match no body"),
]


@pytest.mark.parametrize("cfg, message", REFUSALS, ids=[m[:24] for _, m in REFUSALS])
def test_refusals_name_the_term_and_the_reason(cfg, message):
    with pytest.raises(_native.NativeError, match=message) as e:
        TerminationTerms({"bad_term": cfg}, ctx())
    assert "cfg.terminations term 'bad_term'" in str(e.value) and "no host fallback" in str(e.value)


def test_terms_whose_sensor_or_command_is_not_configured_name_the_field():
    hit = T(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("contact_forces")})
    again = T(func=TM.command_resample, params={"command_name": "base_velocity"})
    for cfg, over, field in ((hit, {"contact_forces": False}, "set cfg.contact_forces"),
                             (again, {"command_names": []}, "set cfg.commands")):
        with pytest.raises(_native.NativeError, match=field):
            TerminationTerms({"t": cfg}, ctx(**over))
        TerminationTerms({"t": cfg}, ctx())  # served once the field is set


def test_limits_are_refused():
    many = {f"t{k}": T(func=TM.time_out) for k in range(_native.MAX_TERMINATION_TERMS + 1)}
    with pytest.raises(_native.NativeError, match="17 terms; the termination kernel takes at most "
                                                  "AS_MAX_TERMINATION_TERMS = 16"):
        TerminationTerms(many, ctx())
    TerminationTerms(dict(list(many.items())[:16]), ctx())
    j = _native.MAX_TERMINATION_IDS + 1
    wide = ctx(joint_names=[f"j{k}" for k in range(j)], soft_joint_pos_limits=np.zeros((j, 2), np.float32))
    with pytest.raises(_native.NativeError, match="selects 33 joints or bodies; the index table holds"):
        TerminationTerms({"t": T(func=TM.joint_pos_out_of_limit)}, wide)
    with pytest.raises(_native.NativeError, match="there are no terms"):
        TerminationTerms({"t": None}, ctx())


def test_sources_take_a_row_count_from_whichever_source_is_there():
    import torch

    q, qd = torch.zeros(12, 4), torch.zeros(10, 4)
    left, count = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32)
    make = _native.make_termination_sources
    assert make({"q": q, "qd": qd}, 0.005).joint_rows == 10
    s = make({"q": q}, 0.005)
    assert s.joint_rows == 12 and s.q == q.data_ptr() and not s.qd
    assert make({"qd": qd}, 0.005).joint_rows == 10 and make({}, 0.005).joint_rows == 0
    assert make({"time_left": left, "command_counter": count}, 0.005).command_terms == 2
    assert make({"time_left": left}, 0.005).command_terms == 2 and make({}, 0.005).command_terms == 0


def test_type_error_is_the_references():
    with pytest.raises(TypeError, match="Configuration for the term 'x' is not of type TerminationTermCfg. Received: "
                                        "'<class 'dict'>'."):
        TerminationTerms({"x": {"func": TM.time_out}}, ctx())


def _host_manager(terms: dict):
    env = types.SimpleNamespace(_terminations_context=ctx)
    cfg = types.SimpleNamespace(terminations=terms, terminations_reset=False)
    return EnvTerminations(cfg, env, 4, "cpu")


def test_set_term_cfg_rewrites_in_place_and_refuses_another_function():
    t = _host_manager({"low": T(func=TM.root_height_below_minimum, params={"minimum_height": 0.3}),
                       "time_out": T(func=TM.time_out, time_out=True)})
    view = TerminationManagerView(t)
    desc, table = t.desc.data_ptr(), t.table.data_ptr()
    new = T(func=TM.root_height_below_minimum, params={"minimum_height": 0.5}, time_out=True)
    view.set_term_cfg("low", new)
    assert view.get_term_cfg("low") is new and view.active_terms == ["low", "time_out"]
    f = fields(t.desc[0].numpy())
    assert f["p0"] == np.float32(0.5) and f["time_out"] == 1
    assert (t.desc.data_ptr(), t.table.data_ptr()) == (desc, table)  # the same device memory: a captured graph sees it
    with pytest.raises(_native.NativeError, match="changes the term's function from root_height_below_minimum to "
                                                  "bad_orientation; the terms' functions are fixed at construction"):
        view.set_term_cfg("low", T(func=TM.bad_orientation, params={"limit_angle": 0.5}))
    with pytest.raises(ValueError, match="Termination term 'nope' not found."):
        view.set_term_cfg("nope", new)
    with pytest.raises(_native.NativeError, match="minimum_height = None is not a number"):
        view.set_term_cfg("low", T(func=TM.root_height_below_minimum, params={"minimum_height": None}))
    assert fields(t.desc[0].numpy())["p0"] == np.float32(0.5)  # a refused cfg changes nothing
    assert view.reset([0, 2]) == {"Episode_Termination/low": 0, "Episode_Termination/time_out": 0}
    t.term_dones[0, 2] = 1
    assert view.reset([0, 2])["Episode_Termination/low"] == 1 and view.reset()["Episode_Termination/low"] == 1
    assert view.get_active_iterable_terms(2) == [("low", [1.0]), ("time_out", [0.0])]
    assert view.get_term("low").dtype.is_floating_point is False and bool(view.get_term("low")[2])
    assert sorted(t.get_state()) == sorted("termination_" + k for k in (
        "term_dones", "time_outs", "terminated", "dones", "last_episode_dones", "reset_request"))


def test_the_quadruped_refuses_terminations_reset_and_the_walker_serves_it():
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    quad = AnymalCStonesEnv.__new__(AnymalCStonesEnv)
    quad.cfg = AnymalCStonesEnvCfg()
    quad._terminations_start()  # nothing asked for: nothing built
    assert quad._terminations is None
    quad.cfg.terminations_reset = True
    with pytest.raises(_native.NativeError, match="terminations_reset is not served by the quadruped: k_quad .* has no "
                                                  "masked reset"):
        quad._terminations_start()
    walker = AllstepsEnv.__new__(AllstepsEnv)
    walker.cfg = AllstepsEnvCfg()
    walker.cfg.terminations_reset = True
    walker._terminations_start()
    assert walker._terminations is None


def test_cfg_classes_default_to_none_and_add_nothing():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.terminations is None and cfg.terminations_reset is False
        assert not EnvTerminations.wanted(cfg)
    assert DirectRLEnv._terminations is None and not hasattr(DirectRLEnv, "termination_manager")
    env = DirectRLEnv.__new__(DirectRLEnv)
    assert env._terminations_get_state() == {}
    assert env._terminations_set_state({"q": 1, "termination_dones": 2, "reward_step": 3}) == {"q": 1, "reward_step": 3}


def test_compat_exports():
    code = """
import isaaclab.envs.mdp as mdp
import isaaclab.managers as managers
from isaaclab.managers import TerminationTermCfg, RewardTermCfg, SceneEntityCfg
from allsteps_isaaclab_amd.utils import terminations as TM
for name in TM.SERVED + tuple(TM.REFUSED):
    assert getattr(mdp, name) is getattr(TM, name) and name in mdp.__all__, name
assert TerminationTermCfg is TM.TerminationTermCfg and "TerminationTermCfg" in managers.__all__
for name in ("is_alive", "joint_pos", "generated_commands", "height_scan", "push_by_setting_velocity"):
    assert hasattr(mdp, name), name  # every name that was there stays
t = TerminationTermCfg(func=mdp.time_out, time_out=True)
assert t.params == {} and [f for f in t.__dataclass_fields__] == ["func", "params", "time_out"]
assert TerminationTermCfg(func=mdp.time_out).time_out is False
try:
    mdp.joint_effort_out_of_limit(None)
except NotImplementedError as e:
    assert "the step keeps no applied torque" in str(e)
print("ok")
"""
    from allsteps_isaaclab_amd import compat

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([compat.SITE, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_termination_kernel_uses_no_scratch_and_spills_no_vgpr(tmp_path):
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
    mine = {k: v for k, v in res.items() if "k_terminations_step" in k}
    assert len(mine) == 1, sorted(res)
    for name, v in mine.items():
        print(name, v)
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (name, v)
        assert v["Dynamic Stack"] == "False", (name, v)
        assert int(v["LDS Size [bytes/block]"]) == 16 * 64, (name, v)
