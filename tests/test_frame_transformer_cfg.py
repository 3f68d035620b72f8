"""The frame transformer's Python surface and build, no GPU: FrameTransformerCfg / OffsetCfg with the reference's
fields and defaults, both forms of cfg.frame_transformer, the frame order on both robots and the stones, the two
offset switches at the allclose edges, every refusal with the field it names, the launch table's contents, the
compat shim, the lazy rule of views._FrameTransformerSet on a fake env and every path that marks it, the
feature-off env (no sensor, no state keys), the C ABI's new name and the refusals it makes before any device call,
and the kernel's compiled resource figures."""

import ctypes as C
import dataclasses
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NS = "/World/envs/env_.*"
TILTED = (0.8, 0.3, -0.4, 0.2)  # (not normalised: an offset's rot is used as given)


def _frame(leaf, name=None, robot=True, **offset):
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg, OffsetCfg

    path = f"{NS}/Robot/{leaf}" if robot else f"{NS}/{leaf}"
    return FrameTransformerCfg.FrameCfg(prim_path=path, name=name, offset=OffsetCfg(**offset))


def _cfg(targets=None, source="torso", **kw):
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg

    base = dict(prim_path=f"{NS}/Robot/{source}", target_frames=[_frame(".*_foot")] if targets is None else targets)
    base.update(kw)
    return FrameTransformerCfg(**base)


def _walker():
    from allsteps_isaaclab_amd.model import load_model

    return load_model()


def _quadruped():
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    return load_model(ANYMAL_C_JSON)


def _spec(cfg, **kw):
    from allsteps_isaaclab_amd.envs.frame_transformer import FrameTransformerSpec

    args = dict(model=_walker(), num_steps=20, step_dt=4 / 240)
    args.update(kw)
    return FrameTransformerSpec(cfg, **args)


def test_cfg_classes_have_the_reference_fields_and_defaults():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.utils.noise import MISSING
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg, OffsetCfg

    assert [f.name for f in dataclasses.fields(OffsetCfg)] == ["pos", "rot"]
    assert (OffsetCfg().pos, OffsetCfg().rot) == ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    assert [f.name for f in dataclasses.fields(FrameTransformerCfg)] == [
        "prim_path", "update_period", "history_length", "debug_vis", "source_frame_offset", "target_frames",
        "visualizer_cfg"]
    c = FrameTransformerCfg()
    assert c.prim_path is MISSING and c.target_frames is MISSING
    assert (c.update_period, c.history_length, c.debug_vis) == (0.0, 0, False)
    assert c.source_frame_offset == OffsetCfg() and c.source_frame_offset is not FrameTransformerCfg().source_frame_offset
    assert [f.name for f in dataclasses.fields(FrameTransformerCfg.FrameCfg)] == ["prim_path", "name", "offset"]
    f = FrameTransformerCfg.FrameCfg()
    assert f.prim_path is MISSING and f.name is None and f.offset == OffsetCfg()
    assert f.offset is not FrameTransformerCfg.FrameCfg().offset
    assert AllstepsEnvCfg().frame_transformer is None and AnymalCStonesEnvCfg().frame_transformer is None


def test_both_cfg_forms_and_the_frame_order():
    one = _spec(_cfg())
    assert one.names == ["frame_transformer"] and one.num_sensors == 1 and one.num_frames == 2
    assert one.frame_names == [["left_foot", "right_foot"]] and one.sources[0][2] == "torso"
    # cfg order does not matter between bodies; {ENV_REGEX_NS} is the env namespace too
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg as FT

    swapped = _spec(_cfg([_frame("right_foot"), FT.FrameCfg(prim_path="{ENV_REGEX_NS}/Robot/left_foot"),
                          _frame("head")]))
    assert swapped.frame_names == [["head", "left_foot", "right_foot"]]
    # two frames on one body come in cfg order (the reference iterates a set here: the decided deviation)
    two = _spec(_cfg([_frame("left_foot", name="toe", pos=(0.1, 0.0, 0.0)), _frame("left_foot", name="heel"),
                      _frame("head")]))
    assert two.frame_names == [["head", "toe", "heel"]]
    flipped = _spec(_cfg([_frame("left_foot", name="heel"), _frame("head"),
                          _frame("left_foot", name="toe", pos=(0.1, 0.0, 0.0))]))
    assert flipped.frame_names == [["head", "heel", "toe"]]
    # one name over several bodies; the same frame listed twice is one frame
    assert _spec(_cfg([_frame(".*_foot", name="foot"), _frame("left_foot", name="foot")])).frame_names == [
        ["foot", "foot"]]
    # the source is among the targets only if a target path matches it
    assert "torso" not in one.frame_names[0]
    everything = _spec(_cfg([_frame(".*")]))
    assert everything.frame_names == [sorted(_walker()["body_names"])] and "torso" in everything.frame_names[0]
    # robot bodies before stones, stones as strings: step_10 before step_2
    mixed = _spec(_cfg([_frame("step_.*", robot=False), _frame("right_foot")]), num_steps=12)
    names = mixed.frame_names[0]
    assert names[0] == "right_foot" and names[1:4] == ["step_0", "step_1", "step_10"] and len(names) == 13
    assert names.index("step_11") < names.index("step_2") < names.index("step_9")
    assert [b[:2] for b, _, _ in mixed.frames[0]][:4] == [("robot", 7), ("stone", 0), ("stone", 1), ("stone", 10)]
    # a stone as the source
    on_stone = _spec(FT(prim_path=f"{NS}/step_3", target_frames=[_frame(".*_foot")]))
    assert on_stone.sources[0][:2] == ("stone", 3)
    # the quadruped: upper case before lower case, LF_SHANK before base
    q = _spec(_cfg([_frame("base"), _frame(".*_SHANK")], source="LF_HIP"), model=_quadruped(), step_dt=0.02)
    assert q.frame_names == [["LF_SHANK", "LH_SHANK", "RF_SHANK", "RH_SHANK", "base"]]
    # the dict form: several sensors, their frames side by side in the launch
    many = _spec({"feet": _cfg(), "stones": _cfg([_frame("step_.*", robot=False)], source="left_foot")})
    assert many.names == ["feet", "stones"] and many.num_frames == 22
    assert many.slices == [slice(0, 2), slice(2, 22)]


def test_both_switches_are_the_reference_allclose_test():
    from allsteps_isaaclab_amd.envs.frame_transformer import is_identity_pose

    assert is_identity_pose((0, 0, 0), (1, 0, 0, 0))
    assert is_identity_pose((0, 0, 0), (1 - 5e-6, 0, 0, 0))  # inside rtol 1e-5 of 1
    assert not is_identity_pose((0, 0, 0), (1 - 2e-5, 0, 0, 0))
    assert is_identity_pose((1e-8, 0, 0), (1, 0, 0, 0)) and not is_identity_pose((2e-8, 0, 0), (1, 0, 0, 0))  # atol 1e-8
    assert not is_identity_pose((0, 0, 0), (1, 0, 2e-8, 0))
    s = _spec(_cfg())
    assert s.apply_source == [False] and s.apply_target == [False]
    s = _spec(_cfg(source_frame_offset=_frame("x", rot=(1 - 5e-6, 0.0, 0.0, 0.0)).offset))
    assert s.apply_source == [False] and list(s.table().source[0].offset_rot)[0] == float(np.float32(1 - 5e-6))
    s = _spec(_cfg(source_frame_offset=_frame("x", pos=(2e-8, 0.0, 0.0)).offset))
    assert s.apply_source == [True] and s.apply_target == [False]
    # the target switch is the sensor's: one frame off the identity turns it on for every frame
    s = _spec(_cfg([_frame("left_foot"), _frame("right_foot", pos=(2e-8, 0.0, 0.0))]))
    assert s.apply_source == [False] and s.apply_target == [True]
    s = _spec({"a": _cfg([_frame("left_foot", rot=TILTED)]), "b": _cfg()})
    assert s.apply_target == [True, False]
    t = s.table()
    assert list(t.apply_target_offset) == [1, 0, 0, 0] and list(t.apply_source_offset) == [0, 0, 0, 0]


def test_table_contents():
    from allsteps_isaaclab_amd import _native

    m = _walker()
    f = lambda xs: [float(np.float32(x)) for x in xs]  # noqa: E731
    s = _spec({"feet": _cfg([_frame(".*_foot"), _frame("left_foot", name="toe", pos=(0.12, 0.0, -0.03), rot=TILTED)]),
               "stones": _cfg([_frame("step_.*", robot=False)], source="left_foot",
                              source_frame_offset=_frame("x", pos=(0.0, 0.0, -0.05)).offset)})
    t = s.table()
    assert isinstance(t, _native.AsFrameTable) and (t.num_sensors, t.num_frames) == (2, 23)
    assert list(t.sensor)[:23] == [0] * 3 + [1] * 20
    for entry, body in ((t.source[0], "torso"), (t.source[1], "left_foot"), (t.target[0], "left_foot"),
                        (t.target[1], "left_foot"), (t.target[2], "right_foot")):
        b = m["body_names"].index(body)
        assert entry.link == int(m["body_link"][b]) and entry.stone == -1
        assert list(entry.body_offset_pos) == f(m["body_offset_pos"][b])
        assert list(entry.body_offset_quat) == f(m["body_offset_quat"][b])
    assert list(t.target[1].offset_pos) == f((0.12, 0.0, -0.03)) and list(t.target[1].offset_rot) == f(TILTED)
    assert list(t.target[0].offset_pos) == [0, 0, 0] and list(t.target[0].offset_rot) == [1, 0, 0, 0]
    assert list(t.source[1].offset_pos) == f((0.0, 0.0, -0.05)) and list(t.source[0].offset_rot) == [1, 0, 0, 0]
    order = [int(x.split("_")[1]) for x in s.frame_names[1]]
    assert order[:4] == [0, 1, 10, 11] and sorted(order) == list(range(20))
    for k, stone in enumerate(order):
        e = t.target[3 + k]
        assert (e.link, e.stone) == (-1, stone) and list(e.body_offset_quat) == [1, 0, 0, 0]
        assert list(e.offset_rot) == [1, 0, 0, 0]
    assert max(e.link for e in list(t.target)[:3]) < m["num_links"]


def test_every_refusal_names_its_field():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg as FT
    from allsteps_isaaclab_amd.utils.sensors import OffsetCfg

    nan, inf = float("nan"), float("inf")
    refused = [
        ("prim_path", dict(prim_path=f"{NS}/Robot/tail")),                                  # matches nothing
        ("prim_path", dict(prim_path=f"{NS}/Robot/.*_foot")),                               # a source on two bodies
        ("prim_path", dict(prim_path=f"{NS}/Robot")),                                       # not a body or a stone
        ("prim_path", dict(prim_path="/World/ground/plane")),
        ("prim_path", dict(prim_path=f"{NS}/step_20")),                                     # past num_steps
        ("prim_path", dict(prim_path=FT().prim_path)),                                      # left MISSING
        (r"target_frames\[0\]\.prim_path", dict(target_frames=[_frame("tail")])),
        (r"target_frames\[1\]\.prim_path", dict(target_frames=[_frame("head"), _frame("step_2.", robot=False)])),
        (r"target_frames\[1\]\.offset", dict(target_frames=[_frame("head", name="a"),
                                                            _frame("waist", name="a", pos=(0.1, 0.0, 0.0))])),
        (r"target_frames\[0\]\.offset", dict(target_frames=[_frame("head", pos=(0.0, inf, 0.0))])),
        (r"target_frames\[0\]\.offset", dict(target_frames=[_frame("head", rot=(1.0, 0.0, nan, 0.0))])),
        (r"target_frames\[0\]\.offset", dict(target_frames=[_frame("head", rot=(1.0, 0.0, 0.0))])),
        ("target_frames", dict(target_frames=[])),
        ("target_frames", dict(target_frames=FT().target_frames)),                          # left MISSING
        ("source_frame_offset", dict(source_frame_offset=OffsetCfg(pos=(nan, 0.0, 0.0)))),
        ("source_frame_offset", dict(source_frame_offset=OffsetCfg(rot=(inf, 0.0, 0.0, 0.0)))),
        ("debug_vis", dict(debug_vis=True)),
        ("history_length", dict(history_length=3)),
        ("update_period", dict(update_period=0.1)),                                         # > step_dt
    ]
    for field, kw in refused:
        with pytest.raises(_native.NativeError, match=rf"cfg\.frame_transformer\.{field}:") as e:
            _spec(_cfg(**kw))
        assert "HIP kernel" in str(e.value)
        with pytest.raises(_native.NativeError, match=rf"cfg\.frame_transformer\['feet'\]\.{field}:"):
            _spec({"torso": _cfg(), "feet": _cfg(**kw)})
    with pytest.raises(_native.NativeError, match=r"cfg\.frame_transformer: 5 sensors.*AS_MAX_FRAME_TRANSFORMERS = 4"):
        _spec({f"ft_{k}": _cfg() for k in range(5)})
    with pytest.raises(_native.NativeError, match=r"cfg\.frame_transformer: 34 target frames.*AS_MAX_FRAMES = 32"):
        _spec({"bodies": _cfg([_frame(".*")]), "again": _cfg([_frame(".*")])})
    with pytest.raises(_native.NativeError, match=r"cfg\.frame_transformer: an empty dict"):
        _spec({})
    full = _spec({"bodies": _cfg([_frame(".*")]), "more": _cfg([_frame("step_1.", robot=False), _frame(".*_hand"),
                                                                 _frame(".*_foot"), _frame("head")])})
    assert full.num_frames == 32 and full.table().num_frames == 32
    assert _spec({f"ft_{k}": _cfg() for k in range(4)}).table().num_sensors == 4
    _spec(_cfg(update_period=4 / 240))  # one env step is not stale
    assert (_native.MAX_FRAME_TRANSFORMERS, _native.MAX_FRAMES) == (4, 32)


def test_compat_shim_imports_the_reference_names():
    site = os.path.join(ROOT, "allsteps_isaaclab_amd", "compat", "site")
    code = ("from isaaclab.sensors import FrameTransformerCfg, OffsetCfg, ImuCfg, RayCasterCfg\n"
            "import isaaclab.sensors, allsteps_isaaclab_amd.utils.sensors as S\n"
            "assert FrameTransformerCfg is S.FrameTransformerCfg and OffsetCfg is S.OffsetCfg\n"
            "assert {'FrameTransformerCfg', 'OffsetCfg'} <= set(isaaclab.sensors.__all__)\n"
            "c = FrameTransformerCfg(prim_path='{ENV_REGEX_NS}/Robot/base', target_frames=[\n"
            "    FrameTransformerCfg.FrameCfg(prim_path='{ENV_REGEX_NS}/Robot/LF_SHANK', name='LF_FOOT',\n"
            "                                 offset=OffsetCfg(pos=(0.0, 0.0, -0.3)))])\n"
            "print(c.target_frames[0].name, c.target_frames[0].offset.pos[2], c.source_frame_offset.rot[0])\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([site, ROOT]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split() == ["LF_FOOT", "-0.3", "1.0"]


def _fake_env(n=5):
    calls = []

    def frame_transformer(table, source, target, stream=None):
        calls.append((table.num_sensors, table.num_frames, tuple(source.shape), tuple(target.shape)))

    nat = types.SimpleNamespace(frame_transformer=frame_transformer)
    from allsteps_isaaclab_amd.envs.scene import SceneView

    env = types.SimpleNamespace(num_envs=n, _device=torch.device("cpu"), device="cpu", step_dt=4 / 240,
                                physics_dt=1 / 240, _native=nat, model=_walker(), _stream=lambda: None,
                                cfg=types.SimpleNamespace(num_steps=20),
                                scene=SceneView(types.SimpleNamespace(num_envs=n, env_spacing=4.0), "cpu"))
    return env, calls


def test_views_are_zero_copy_and_lazy_on_a_fake_env():
    """_FrameTransformerSet over a fake env whose handle records the launches: strided views of the env-minor
    buffers, one launch per dirty read however many sensors and reads, a forced update always."""
    from allsteps_isaaclab_amd.envs.views import _FrameTransformerSet

    env, calls = _fake_env()
    g = _FrameTransformerSet(env, {"feet": _cfg([_frame(".*_foot"), _frame("left_foot", name="toe", rot=TILTED)]),
                                   "stones": _cfg([_frame("step_.*", robot=False)], source="left_foot")})
    a, b = g.sensors["feet"], g.sensors["stones"]
    assert (g.num_sensors, g.num_frames) == (2, 23) and g.source.shape == (7, 2, 5) and g.target.shape == (14, 23, 5)
    assert not g.source.any() and not g.target.any() and a.launches == 0 and calls == []
    d = a.data
    assert calls == [(2, 23, (7, 2, 5), (14, 23, 5))] and a.launches == b.launches == 1
    assert d.target_frame_names == ["left_foot", "toe", "right_foot"] and len(b.data.target_frame_names) == 20
    g.target.copy_(torch.arange(14 * 23 * 5, dtype=torch.float32).reshape(14, 23, 5))
    g.source.copy_(torch.arange(7 * 2 * 5, dtype=torch.float32).reshape(7, 2, 5))
    for sensor, s, lo, count in ((a, 0, 0, 3), (b, 1, 3, 20)):
        x = sensor.data
        assert x.source_pos_w.shape == (5, 3) and x.source_pos_w.data_ptr() == g.source[0, s].data_ptr()
        assert x.source_quat_w.shape == (5, 4) and x.source_quat_w.data_ptr() == g.source[3, s].data_ptr()
        assert torch.equal(x.source_quat_w, g.source[3:7, s].T)
        for name, row, width in (("target_pos_w", 0, 3), ("target_quat_w", 3, 4), ("target_pos_source", 7, 3),
                                 ("target_quat_source", 10, 4)):
            v = getattr(x, name)
            assert v.shape == (5, count, width) and v.data_ptr() == g.target[row, lo].data_ptr()
            assert torch.equal(v, g.target[row:row + width, lo:lo + count].permute(2, 1, 0))
            g.target[row + 1, lo + count - 1, 3] = -7.5
            assert float(getattr(sensor.data, name)[3, count - 1, 1]) == -7.5
    assert a.launches == 1  # all those reads: no launch
    g.mark_dirty()
    assert a.launches == 1
    b.data, a.data
    assert a.launches == 2
    a.update(4 / 240)  # not forced: the next read decides, and nothing is dirty
    a.data
    assert a.launches == 2
    a.update(4 / 240, force_recompute=True)
    b.update(4 / 240, force_recompute=True)
    assert a.launches == 4 and len(calls) == 4
    b.reset([2])
    a.data
    a.reset()
    b.data
    assert a.launches == 6
    assert not hasattr(g, "get_state") and not hasattr(g, "outdated")  # a function of the state: nothing to keep
    text = str(a)
    assert text.startswith(f"FrameTransformer @ '{NS}/Robot/torso': \n")
    assert "\ttracked body frames: ['torso', 'left_foot', 'right_foot'] \n" in text
    assert "\tnumber of envs: 5\n\tsource body frame: torso\n" in text
    assert text.endswith("\ttarget frames (count: ['left_foot', 'toe', 'right_foot']): 3\n")
    assert a.num_instances == 5 and a.device == "cpu" and a.cfg is g._spec.cfgs[0]


def test_every_env_path_marks_the_sensors():
    """DirectRLEnv's own paths on a bare base env with a recording lazy sensor: step, reset and _scene_changed (what
    _reset_idx, set_state, account_steps, stone regeneration and the robot view's writers call) each mark it."""
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.envs.views import _FrameTransformerSet, _RobotView

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = 5

    class Env(DirectRLEnv):
        def _step_impl(self, action):
            return {"policy": action}, None, None, None, {}

        def _reset_impl(self):
            return {"policy": None}

    env = Env(cfg)
    assert env._lazy_sensors == ()
    fake, calls = _fake_env()
    env._native, env.model, env._stream = fake._native, fake.model, fake._stream
    g = _FrameTransformerSet(env, _cfg())
    env._add_lazy_sensor(g)
    ft = g.sensors["frame_transformer"]

    def launched_by(what):
        ft.data
        before = g.launches
        what()
        assert g.launches == before  # marking launches nothing
        ft.data
        ft.data
        return g.launches - before

    assert launched_by(lambda: None) == 0
    assert launched_by(lambda: env.step(torch.zeros(5, cfg.action_space))) == 1
    assert launched_by(env.reset) == 1
    assert launched_by(env._scene_changed) == 1
    # the three writers of the robot view go through _scene_changed
    env.state = {"root_pos": torch.zeros(3, 5), "root_quat": torch.zeros(4, 5), "root_lin": torch.zeros(3, 5),
                 "root_ang": torch.zeros(3, 5), "q": torch.zeros(21, 5), "qd": torch.zeros(21, 5)}
    view = object.__new__(_RobotView)
    view._env, view._ALL_INDICES = env, torch.arange(5)
    assert launched_by(lambda: view.write_root_pose_to_sim(torch.zeros(5, 7))) == 1
    assert launched_by(lambda: view.write_root_velocity_to_sim(torch.zeros(5, 6))) == 1
    assert launched_by(lambda: view.write_joint_state_to_sim(torch.zeros(5, 21), torch.zeros(5, 21))) == 1
    # and the env subclasses' paths call _scene_changed
    import inspect

    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.native_env import NativeDirectEnv

    for fn in (AllstepsEnv._reset_idx, AllstepsEnv.account_steps, AllstepsEnv.generate_foot_steps,
               NativeDirectEnv.set_state):
        assert "self._scene_changed()" in inspect.getsource(fn), fn.__name__


def test_feature_off_env_has_no_sensor_no_state_keys_and_nothing_to_launch():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.native_env import NativeDirectEnv
    from allsteps_isaaclab_amd.envs.state import alloc_state

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = 4
    env = NativeDirectEnv(cfg)  # no handle: the state paths alone
    assert env._frame_transformers is None and not hasattr(env, "frame_transformer")
    assert env.scene.sensors == {} and env._lazy_sensors == ()
    env.state = alloc_state(4, torch.device("cpu"))
    before = set(env.get_state())
    assert before == set(env.state) and not any("frame" in k for k in before)
    env._scene_changed()
    env._sensors_reset(None)
    env.set_state(env.get_state())
    assert set(env.get_state()) == before


def test_abi_exports_the_entry_point_and_refuses_before_any_device_call():
    from allsteps_isaaclab_amd import _native

    assert "as_frame_transformer" in _native.EXPORTED_SYMBOLS
    with open(os.path.join(_native.INCLUDE, "allsteps.h")) as f:
        header = f.read()
    assert re.search(r"#define AS_ABI_VERSION 6\b", header)
    assert re.search(r"#define AS_MAX_FRAME_TRANSFORMERS 4\b", header) and re.search(r"#define AS_MAX_FRAMES 32\b", header)
    assert re.search(r"int as_frame_transformer\(as_env_t\* env, const as_frame_table_t\* host, float\* source, "
                     r"float\* target, void\* stream\);", header)
    assert C.sizeof(_native.AsFrameBody) == 4 * (2 + 3 + 4 + 3 + 4)
    assert C.sizeof(_native.AsFrameTable) == 4 * (2 + 4 + 4) + 64 * (4 + 32) + 4 * 32 < 4096 - 512  # a kernel argument
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def table(S=2, F=3, sensor=(0, 0, 1)):
        t = _native.AsFrameTable()
        t.num_sensors, t.num_frames = S, F
        for f, s in enumerate(sensor):
            t.sensor[f] = s
        return t

    def call(t, source, target, env=None):
        rc = L.as_frame_transformer(env, None if t is None else C.byref(t), source, target, None)
        return rc, L.as_last_error().decode()

    # nothing here ever reaches a device call: there is no handle, and that is the last thing asked for
    assert call(None, p, p) == (-1, "as_frame_transformer: null argument host")
    assert call(table(), None, p) == (-1, "as_frame_transformer: null argument source")
    assert call(table(), p, None) == (-1, "as_frame_transformer: null argument target")
    for count in (0, -1, 5):
        rc, msg = call(table(S=count), p, p)
        assert rc == -1 and f"num_sensors {count} outside [1, AS_MAX_FRAME_TRANSFORMERS = 4]" in msg
    for count in (0, -1, 33):
        rc, msg = call(table(F=count), p, p)
        assert rc == -1 and f"num_frames {count} outside [1, AS_MAX_FRAMES = 32]" in msg
    for bad in ((0, 2, 1), (0, -1, 1)):
        rc, msg = call(table(sensor=bad), p, p)
        assert rc == -1 and f"frame 1 sensor {bad[1]} outside [0, 2)" in msg
    for bad in ((1, 1, 1), (0, 1, 0), (0, 0, 0)):  # not from 0, not grouped, a sensor without a frame
        rc, msg = call(table(sensor=bad), p, p)
        assert rc == -1 and "out of order" in msg, (bad, msg)
    assert call(table(), p, p) == (-1, "as_frame_transformer: null argument env")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_compiles_without_scratch_or_spills(tmp_path):
    """k_frame_transformer with the package's own flags (_native.STEP_FLAGS): no scratch, no VGPR or SGPR spill, no
    AGPRs -- both body rows, the offsets and the 21 outputs live in registers, and body_row's velocity chain falls
    away; its LDS is k_body_state's (the step's FK scratch); the VGPR ceiling is k_imu's test's."""
    from allsteps_isaaclab_amd import _native

    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "-I", _native.CSRC, "--cuda-device-only", "-S", "-o",
                        str(tmp_path / "kernels.s"), "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(_native.CSRC, "allsteps_kernels.hip")],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = {}
    for name in ("k_frame_transformer", "k_body_state"):
        m = re.search(rf"Function Name: _ZN2as\d+{name}E.*?(?=Function Name:|\Z)", r.stderr, re.S)
        assert m, name
        res[name] = dict(re.findall(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?):\s+(\S+) \[-Rpass", m.group(0)))
    print(res)
    k, b = res["k_frame_transformer"], res["k_body_state"]
    assert int(k["ScratchSize [bytes/lane]"]) == 0, k
    assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0 and int(k["AGPRs"]) == 0, k
    assert int(k["LDS Size [bytes/block]"]) == int(b["LDS Size [bytes/block]"]), (k, b)
    assert int(k["VGPRs"]) <= 128, k  # four waves per SIMD at least
