"""cfg.observations on the host: parsing, layout, the device tables as host arrays, the refusals, the table and the
compat exports (envs/observations.py, utils/observations.py).  No device."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from allsteps_isaaclab_amd import _native  # noqa: E402
from allsteps_isaaclab_amd.envs.observations import ObsContext, ObservationGroups, resolve_joint_ids  # noqa: E402
from allsteps_isaaclab_amd.utils import commands as CM  # noqa: E402
from allsteps_isaaclab_amd.utils import noise as NZ  # noqa: E402
from allsteps_isaaclab_amd.utils import observations as OB  # noqa: E402
from allsteps_isaaclab_amd.utils import sensors as SN  # noqa: E402
from allsteps_isaaclab_amd.utils.events import SceneEntityCfg  # noqa: E402

Term, Group = OB.ObservationTermCfg, OB.ObservationGroupCfg
J = 12


def ctx(**kw):
    d = dict(joint_names=[f"{leg}_{j}" for leg in ("LF", "RF", "LH", "RH") for j in ("HAA", "HFE", "KFE")],
             default_joint_pos=np.linspace(-0.4, 0.7, J).astype(np.float32),
             default_joint_vel=np.zeros(J, np.float32),
             soft_joint_pos_limits=np.stack([np.full(J, -2.0, np.float32), np.full(J, 1.0, np.float32)], -1),
             action_cols=12, clamp_actions=True, command_names=["base_velocity"],
             ray_sensors={"height_scanner": 187}, imu_names=["imu", "imu_hind"])
    d.update(kw)
    return ObsContext(**d)


class PolicyCfg(Group):
    """The reference velocity task's PolicyCfg (velocity_env_cfg.py), written as a subclass with class attributes."""

    base_lin_vel = Term(func=OB.base_lin_vel, noise=NZ.UniformNoiseCfg(n_min=-0.1, n_max=0.1))
    base_ang_vel = Term(func=OB.base_ang_vel, noise=NZ.UniformNoiseCfg(n_min=-0.2, n_max=0.2))
    projected_gravity = Term(func=OB.projected_gravity, noise=NZ.UniformNoiseCfg(n_min=-0.05, n_max=0.05))
    velocity_commands = Term(func=CM.generated_commands, params={"command_name": "base_velocity"})
    joint_pos = Term(func=OB.joint_pos_rel, noise=NZ.UniformNoiseCfg(n_min=-0.01, n_max=0.01))
    joint_vel = Term(func=OB.joint_vel_rel, noise=NZ.UniformNoiseCfg(n_min=-1.5, n_max=1.5))
    actions = Term(func=OB.last_action)
    height_scan = Term(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")},
                       noise=NZ.UniformNoiseCfg(n_min=-0.1, n_max=0.1), clip=(-1.0, 1.0))
    skipped = None


class ObservationsCfg:
    def __init__(self, **kw):
        self.obs = PolicyCfg(enable_corruption=True, **kw)


def test_velocity_task_group_fits_with_history_five():
    g = ObservationGroups(ObservationsCfg(), ctx()).groups[0]
    assert g.names == ["base_lin_vel", "base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos",
                       "joint_vel", "actions", "height_scan"]  # cfg order, the None entry skipped
    assert (g.d0, g.out_cols) == (48 + 187, 48 + 187) and g.dim == (235,)
    h = ObservationGroups(ObservationsCfg(history_length=5), ctx()).groups[0]
    assert (h.d0, h.out_cols) == (235, 1175) and h.dim == (1175,)
    assert h.term_dims == [(15,), (15,), (15,), (15,), (60,), (60,), (60,), (935,)]
    assert h.out_cols <= _native.MAX_OBS_OUT_COLS and h.d0 <= _native.MAX_OBS_COLS
    assert (_native.MAX_OBS_GROUPS, _native.MAX_OBS_TERMS, _native.MAX_OBS_COLS, _native.MAX_OBS_OUT_COLS) == \
        (4, 16, 256, 1280)


def test_limits_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "allsteps.h")).read()
    for name, value in (("AS_MAX_OBS_GROUPS", _native.MAX_OBS_GROUPS), ("AS_MAX_OBS_TERMS", _native.MAX_OBS_TERMS),
                        ("AS_MAX_OBS_COLS", _native.MAX_OBS_COLS), ("AS_MAX_OBS_OUT_COLS", _native.MAX_OBS_OUT_COLS),
                        ("AS_OBS_COL_ROWS", _native.OBS_COL_ROWS)):
        assert f"#define {name} {value} " in text or f"#define {name} {value}\n" in text, name
    assert "AS_OBS_SRC_" + _native.OBS_SOURCES[0].upper() + " = 0" in text
    assert len(_native.OBS_SOURCES) == 12
    tag = open(os.path.join(ROOT, "allsteps_isaaclab_amd", "csrc", "allsteps_observations.h")).read()
    assert f"kObsTag = 0x{_native.OBS_TAG:08x}u" in tag


def test_dict_cfgs_and_group_order():
    cfg = {"critic": {"concatenate_terms": True, "z": Term(func=OB.base_pos_z), "none": None,
                      "q": Term(func=OB.joint_pos)},
           "skip": None,
           "extra": Group(concatenate_terms=False)}
    cfg["extra"].w = Term(func=OB.root_quat_w, params={"make_quat_unique": True}, history_length=2,
                          flatten_history_dim=False)
    cfg["extra"].v = Term(func=OB.root_lin_vel_w, history_length=1)
    groups = ObservationGroups(cfg, ctx())
    assert groups.names == ["critic", "extra"]
    assert groups.groups[0].names == ["z", "q"] and groups.groups[0].dim == (13,)
    assert groups.groups[1].dim == [(2, 4), (3,)] and not groups.groups[1].concatenate
    assert groups.groups[1].terms[0].kind == _native.OBS_QUAT_UNIQUE


def test_group_history_overrides_the_terms_and_corruption_off_drops_noise():
    g = Group(history_length=3, flatten_history_dim=True)
    g.a = Term(func=OB.base_lin_vel, history_length=7, flatten_history_dim=False,
               noise=NZ.GaussianNoiseCfg(mean=0.0, std=1.0))
    g.b = Term(func=OB.base_pos_z)
    spec = ObservationGroups({"g": g}, ctx()).groups[0]
    assert [t.slots for t in spec.terms] == [3, 3] and spec.term_dims == [(9,), (3,)]
    assert spec.terms[0].noise_kind == _native.NOISE_NONE  # enable_corruption defaults to False
    g.enable_corruption = True
    assert ObservationGroups({"g": g}, ctx()).groups[0].terms[0].noise_kind == _native.NOISE_GAUSSIAN


def test_descriptor_rows_column_table_and_output_map():
    g = Group(enable_corruption=True)
    g.jp = Term(func=OB.joint_pos_rel, params={"asset_cfg": SceneEntityCfg("robot", joint_names=[".*_KFE"])},
                noise=NZ.UniformNoiseCfg(n_min=-0.1, n_max=0.3, operation="scale"), clip=(-0.5, 0.1),
                scale=(1.0, 2.0, 3.0, 0.1), history_length=2)
    g.hs = Term(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner"), "offset": 0.3},
                noise=NZ.ConstantNoiseCfg(bias=0.1))
    g.act = Term(func=OB.last_action)
    g.imu = Term(func=SN.imu_ang_vel, params={"asset_cfg": SceneEntityCfg("imu_hind")})
    g.lim = Term(func=OB.joint_pos_limit_normalized, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[1, 4])})
    spec = ObservationGroups({"g": g}, ctx(ray_sensors={"height_scanner": 9})).groups[0]
    ints = spec.rows.view(np.int32)
    S = _native.OBS_SOURCES.index
    # kind, source, width, col, out_col, history, noise_kind, noise_op, clip
    assert ints[0, :9].tolist() == [_native.OBS_GATHER, S("q"), 4, 0, 0, 2, _native.NOISE_UNIFORM, 1, 1]
    assert spec.rows[0, 9:11].tolist() == [np.float32(-0.5), np.float32(0.1)]
    assert ints[1, :9].tolist() == [_native.OBS_HEIGHT_SCAN, S("ray_hits"), 9, 4, 8, 1, _native.NOISE_CONSTANT, 0, 0]
    assert ints[2, :6].tolist() == [_native.OBS_LAST_ACTION, S("actions"), 12, 13, 17, 1] and ints[2, 11] == 1
    assert ints[3, :6].tolist() == [_native.OBS_GATHER, S("imu"), 3, 25, 29, 1]
    assert ints[4, :6].tolist() == [_native.OBS_LIMIT_NORM, S("q"), 2, 28, 32, 1]
    cols = spec.cols
    assert cols[0].view(np.int32)[:4].tolist() == [2, 5, 8, 11]  # the KFE joints
    assert np.array_equal(cols[1, :4], ctx().default_joint_pos[[2, 5, 8, 11]])
    assert cols[3, :4].tolist() == [np.float32(-0.1)] * 4
    assert cols[4, :4].tolist() == [np.float32(0.3 - -0.1)] * 4  # w = n_max - n_min in double, then float32
    assert cols[5, :4].tolist() == [1.0, 2.0, 3.0, np.float32(0.1)]
    assert cols[0].view(np.int32)[4:13].tolist() == [18 + r for r in range(9)]  # the hits' z rows of 9 rays
    assert cols[1, 4:13].tolist() == [np.float32(0.3)] * 9 and cols[3, 4:13].tolist() == [np.float32(0.1)] * 9
    assert cols[0].view(np.int32)[25:28].tolist() == [(10 + j) * 2 + 1 for j in range(3)]  # ang_vel_b of IMU 1 of 2
    assert cols[1, 28:30].tolist() == [-0.5, -0.5] and cols[2, 28:30].tolist() == [3.0, 3.0]  # centre, range
    assert cols[5, 4:30].tolist() == [1.0] * 26
    # the output map: jp's two slots (old, then last), then one slot each
    m = spec.omap
    assert (m[:4] & 255).tolist() == [0, 1, 2, 3] and ((m[:4] >> 8) & 1).tolist() == [0] * 4
    assert (m[4:8] & 255).tolist() == [0, 1, 2, 3] and ((m[4:8] >> 8) & 1).tolist() == [1] * 4
    assert (m[:8] >> 9).tolist() == [4] * 8 and (m[8:17] & 255).tolist() == list(range(4, 13))
    assert spec.out_cols == 34 and len(m) == 34 and ((m[8:] >> 8) & 1).all()


def test_per_column_noise_parameters():
    import torch

    g = Group(enable_corruption=True)
    g.a = Term(func=OB.root_pos_w, noise=NZ.UniformNoiseCfg(n_min=torch.tensor([-0.1, -0.2, -0.3]),
                                                           n_max=torch.tensor([0.4, 0.3, 0.2])))
    g.b = Term(func=OB.root_ang_vel_w, noise=NZ.GaussianNoiseCfg(mean=0.5, std=(0.1, 0.2, 0.3), operation="abs"))
    spec = ObservationGroups({"g": g}, ctx()).groups[0]
    f = np.float32
    assert spec.cols[3, :3].tolist() == [f(-0.1), f(-0.2), f(-0.3)]
    assert spec.cols[4, :3].tolist() == [f(0.4) - f(-0.1), f(0.3) - f(-0.2), f(0.2) - f(-0.3)]  # in float32
    assert spec.cols[3, 3:6].tolist() == [0.5] * 3 and spec.cols[4, 3:6].tolist() == [f(0.1), f(0.2), f(0.3)]
    assert spec.rows.view(np.int32)[1, 6:8].tolist() == [_native.NOISE_GAUSSIAN, 2]


def test_joint_selection():
    names = ctx().joint_names
    assert resolve_joint_ids(SceneEntityCfg("robot"), names, "x") is None
    assert resolve_joint_ids(SceneEntityCfg("robot", joint_names=["RF_.*", "LF_HAA"]), names, "x") == [0, 3, 4, 5]
    assert resolve_joint_ids(SceneEntityCfg("robot", joint_names=["RF_HAA", "LF_HAA"], preserve_order=True), names,
                             "x") == [3, 0]
    assert resolve_joint_ids(SceneEntityCfg("robot", joint_ids=slice(0, 3)), names, "x") == [0, 1, 2]


def _refuse(group_or_cfg, match, context=None, name="obs"):
    cfg = group_or_cfg if isinstance(group_or_cfg, dict) and name is None else {name: group_or_cfg}
    with pytest.raises(_native.NativeError, match=match) as e:
        ObservationGroups(cfg, context or ctx())
    return str(e.value)


def _one(term, **group):
    g = Group(**group)
    g.t = term
    return g


def test_refusals_name_the_group_the_term_and_the_reason():
    msg = _refuse(_one(Term(func=OB.base_lin_vel, modifiers=[object()])), "modifiers")
    assert "group 'obs' term 't'" in msg and "no host fallback" in msg
    model = NZ.NoiseModelWithAdditiveBiasCfg(noise_cfg=NZ.GaussianNoiseCfg(), bias_noise_cfg=NZ.GaussianNoiseCfg())
    assert "group 'obs' term 't'" in _refuse(_one(Term(func=OB.base_lin_vel, noise=model), enable_corruption=True),
                                             "NoiseModelWithAdditiveBiasCfg")
    assert "term 't'" in _refuse(_one(Term(func=SN.image, params={"sensor_cfg": SceneEntityCfg("camera")})), "image")
    _refuse(_one(Term(func=OB.image_features)), "image_features")
    _refuse(_one(Term(func=OB.body_incoming_wrench, params={"asset_cfg": SceneEntityCfg("robot")})),
            "body_incoming_wrench")
    _refuse(_one(Term(func=lambda env: None)), "not a served term function")
    _refuse(_one(Term(func=OB.joint_pos, history_length=2, flatten_history_dim=False)), "concatenate_terms=False")
    assert "group 'policy'" in _refuse(_one(Term(func=OB.base_lin_vel)), "task's own observation", name="policy")
    # a sensor or command the env's cfg does not have
    _refuse(_one(Term(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")})),
            "cfg.height_scanner", ctx(ray_sensors={}))
    _refuse(_one(Term(func=SN.imu_lin_acc)), "cfg.imu", ctx(imu_names=[]))
    _refuse(_one(Term(func=SN.imu_lin_acc, params={"asset_cfg": SceneEntityCfg("imu_front")})), "imu_front")
    _refuse(_one(Term(func=CM.generated_commands, params={"command_name": "pose"})), "cfg.commands")
    _refuse(_one(Term(func=CM.generated_commands, params={"command_name": "base_velocity"})), "cfg.commands",
            ctx(command_names=[]))
    # parameters the function does not take, selections that match nothing
    _refuse(_one(Term(func=OB.base_lin_vel, params={"offset": 1.0})), "not parameters")
    _refuse(_one(Term(func=OB.joint_pos, params={"asset_cfg": SceneEntityCfg("robot", joint_names=["nope"])})),
            "match no joint")
    _refuse(_one(Term(func=OB.last_action, params={"action_name": "legs"})), "one action term")
    _refuse(_one(Term(func=OB.base_lin_vel, noise=NZ.UniformNoiseCfg(operation="mul")), enable_corruption=True),
            "operation")


def test_limits_are_refused():
    wide = Group()
    wide.a = Term(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")})
    wide.b = Term(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")})
    assert "AS_MAX_OBS_COLS = 256" in _refuse(wide, "374 columns")
    deep = PolicyCfg(history_length=6)
    assert "AS_MAX_OBS_OUT_COLS = 1280" in _refuse(deep, "1410 with the history")
    many = Group()
    for k in range(17):
        setattr(many, f"t{k}", Term(func=OB.base_pos_z))
    _refuse(many, "AS_MAX_OBS_TERMS = 16")
    with pytest.raises(_native.NativeError, match="AS_MAX_OBS_GROUPS = 4"):
        ObservationGroups({f"g{k}": _one(Term(func=OB.base_pos_z)) for k in range(5)}, ctx())
    _refuse(Group(), "no terms")


def test_scale_checks_are_the_references():
    with pytest.raises(ValueError, match="Expected: 3 but received: 2"):
        ObservationGroups({"g": _one(Term(func=OB.base_lin_vel, scale=(1.0, 2.0)))}, ctx())
    with pytest.raises(TypeError, match="not of type float, int or tuple"):
        ObservationGroups({"g": _one(Term(func=OB.base_lin_vel, scale="2"))}, ctx())
    with pytest.raises(TypeError, match="not of type ObservationTermCfg"):
        g = Group()
        g.t = 3.0
        ObservationGroups({"g": g}, ctx())
    with pytest.raises(TypeError, match="not of type 'ObservationGroupCfg'"):
        ObservationGroups({"g": 3.0}, ctx())


def test_set_term_keeps_the_layout():
    groups = ObservationGroups(ObservationsCfg(), ctx())
    new = Term(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")}, clip=(-0.5, 0.5))
    g = groups.set_term("obs", "height_scan", new)
    assert g.rows[7, 9:11].tolist() == [-0.5, 0.5] and g.terms[7].noise_kind == _native.NOISE_NONE
    with pytest.raises(_native.NativeError, match="changes the term's shape"):
        groups.set_term("obs", "height_scan", Term(func=OB.base_lin_vel))
    with pytest.raises(_native.NativeError, match="changes the term's shape"):
        groups.set_term("obs", "actions", Term(func=OB.last_action, history_length=2))
    with pytest.raises(ValueError, match="not found"):
        groups.set_term("obs", "nope", new)
    with pytest.raises(ValueError, match="Unable to find the group"):
        groups.group("nope")


def test_table_is_the_references_form():
    g = Group()
    g.base_lin_vel = Term(func=OB.base_lin_vel)
    g.joint_pos = Term(func=OB.joint_pos, history_length=2)
    s = ObservationGroups({"obs": g, "split": _one(Term(func=OB.base_pos_z), concatenate_terms=False)}, ctx()).table()
    lines = s.splitlines()
    assert lines[0] == "<ObservationManager> contains 2 groups."
    assert lines[2].strip("|").strip() == "Active Observation Terms in Group: 'obs' (shape: (27,))"
    assert [c.strip() for c in lines[4].strip("|").split("|")] == ["Index", "Name", "Shape"]
    assert [c.strip() for c in lines[6].strip("|").split("|")] == ["0", "base_lin_vel", "(3,)"]
    assert [c.strip() for c in lines[7].strip("|").split("|")] == ["1", "joint_pos", "(24,)"]
    assert lines[7].split("|")[2].startswith(" joint_pos ")  # names left-aligned
    assert len({len(x) for x in lines[1:9]}) == 1 and lines[1].startswith("+-") and lines[8].startswith("+-")
    assert "Active Observation Terms in Group: 'split'" in s and "'split' (shape" not in s


def test_compat_exports():
    code = """
import isaaclab.envs.mdp as mdp
from isaaclab.managers import ObservationGroupCfg, ObservationTermCfg, SceneEntityCfg
from allsteps_isaaclab_amd.utils import observations as OB
for name in ("base_pos_z", "base_lin_vel", "base_ang_vel", "projected_gravity", "root_pos_w", "root_quat_w",
             "root_lin_vel_w", "root_ang_vel_w", "joint_pos", "joint_pos_rel", "joint_pos_limit_normalized",
             "joint_vel", "joint_vel_rel", "last_action", "generated_commands", "height_scan", "imu_orientation",
             "imu_ang_vel", "imu_lin_acc", "image", "image_features", "body_incoming_wrench"):
    assert callable(getattr(mdp, name)), name
assert ObservationTermCfg is OB.ObservationTermCfg and ObservationGroupCfg is OB.ObservationGroupCfg
t = ObservationTermCfg(func=mdp.base_lin_vel)
assert (t.params, t.modifiers, t.noise, t.clip, t.scale, t.history_length, t.flatten_history_dim) == \\
    ({}, None, None, None, None, 0, True)
g = ObservationGroupCfg()
assert (g.concatenate_terms, g.enable_corruption, g.history_length, g.flatten_history_dim) == (True, False, None, True)
print("ok")
"""
    from allsteps_isaaclab_amd import compat

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([compat.SITE, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_cfg_classes_default_to_none():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    assert AllstepsEnvCfg().observations is None and AnymalCStonesEnvCfg().observations is None
