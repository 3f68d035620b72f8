"""cfg.camera without a device: the cfg classes and their defaults, the spec's refusals by field name, the compat
shims, mdp.image, the sensor's views and laziness over a fake env, the C ABI's entry point and its refusals before any
device call, and the kernel's resource usage."""

import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TYPES = ["distance_to_image_plane", "distance_to_camera", "normals"]


def _cfg(**kw):
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCameraCfg, patterns

    base = dict(prim_path="/World/envs/env_.*/Robot/base", mesh_prim_paths=["/World/ground"],
                pattern_cfg=patterns.PinholeCameraPatternCfg(width=19, height=13))
    base.update(kw)
    return RayCasterCameraCfg(**base)


def _spec(cfg, root_body="base", step_dt=0.02, **kw):
    from allsteps_isaaclab_amd.envs.ray_camera import RayCameraSpec

    return RayCameraSpec(cfg, root_body=root_body, step_dt=step_dt, **kw)


def test_cfg_defaults_are_the_reference_ones():
    from allsteps_isaaclab_amd.utils.noise import MISSING
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCameraCfg, RayCasterCfg, patterns

    c = RayCasterCameraCfg()
    assert isinstance(c, RayCasterCfg)
    assert c.prim_path is MISSING and c.mesh_prim_paths is MISSING and c.pattern_cfg is MISSING
    assert (c.update_period, c.history_length, c.debug_vis, c.max_distance, c.drift_range) == (0.0, 0, False, 1e6,
                                                                                              (0.0, 0.0))
    assert c.data_types == ["distance_to_image_plane"] and c.depth_clipping_behavior == "none"
    assert c.attach_yaw_only is False  # __post_init__
    assert RayCasterCameraCfg(attach_yaw_only=True).attach_yaw_only is False
    assert (c.offset.pos, c.offset.rot, c.offset.convention) == ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), "ros")
    assert c.data_types is not RayCasterCameraCfg().data_types  # no shared default
    p = patterns.PinholeCameraPatternCfg(width=4, height=3)
    assert (p.focal_length, p.horizontal_aperture, p.vertical_aperture, p.horizontal_aperture_offset,
            p.vertical_aperture_offset) == (24.0, 20.955, None, 0.0, 0.0)
    assert p.func is patterns.pinhole_camera_pattern and issubclass(type(p), patterns.PatternBaseCfg)
    assert patterns.PinholeCameraPatternCfg().width is MISSING
    q = patterns.PinholeCameraPatternCfg.from_intrinsic_matrix([300.0, 0, 8.0, 0, 200.0, 6.0, 0, 0, 1], 16, 12)
    assert (q.focal_length, q.width, q.height) == (24.0, 16, 12)
    assert q.horizontal_aperture == 16 * 24.0 / 300.0 and q.vertical_aperture == 12 * 24.0 / 200.0
    assert q.horizontal_aperture_offset == 0.0 and q.vertical_aperture_offset == 0.0
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    assert AllstepsEnvCfg().camera is None and AnymalCStonesEnvCfg().camera is None


def test_pinhole_pattern_serves_a_batch_of_cameras():
    from allsteps_isaaclab_amd.envs.ray_camera import intrinsic_matrix
    from allsteps_isaaclab_amd.utils.sensors import patterns

    p = patterns.PinholeCameraPatternCfg(width=5, height=4)
    k = torch.from_numpy(intrinsic_matrix(p))
    assert p.vertical_aperture == 20.955 * 4 / 5  # filled in, as the reference does
    k2 = k.clone()
    k2[0, 0] *= 2
    starts, dirs = patterns.pinhole_camera_pattern(p, torch.stack([k, k2]), "cpu")
    assert starts.shape == dirs.shape == (2, 20, 3) and not bool(starts.any()) and dirs.dtype == torch.float32
    assert torch.allclose(dirs.norm(dim=-1), torch.ones(2, 20), atol=1e-6)
    assert float(dirs[1, 0, 1]) < float(dirs[0, 0, 1])  # twice the focal length: a narrower view
    with pytest.raises(ValueError, match=r"\(N, 3, 3\)"):
        patterns.pinhole_camera_pattern(p, k, "cpu")


def test_spec_of_a_plain_cfg():
    from allsteps_isaaclab_amd import _native

    s = _spec(_cfg(mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_3"], data_types=list(TYPES),
                   depth_clipping_behavior="max", max_distance=7.5),
              step_paths=[f"/World/envs/env_.*/step_{i}" for i in range(20)])
    assert (s.width, s.height, s.num_rays, s.surfaces, s.clipping) == (19, 13, 247, 3, _native.CAM_CLIP_MAX)
    assert s.surface_names() == ["ground", "stones"] and s.data_types == TYPES
    c = s.native_cfg()
    assert (c.width, c.height, c.surfaces, c.clipping, c.max_distance, c.ground_z) == (19, 13, 3, 1, 7.5, 0.0)
    assert s.dirs.shape == (3, 247) and s.dirs.dtype == np.float32 and s.offset.shape == (7,)
    assert s.offset.tolist() in ([0, 0, 0, 0.5, 0.5, -0.5, 0.5], [0, 0, 0, -0.5, -0.5, 0.5, -0.5])  # identity "ros"
    assert _spec(_cfg(mesh_prim_paths=["/World/envs/env_.*/step_.*"])).surfaces == 2
    assert _spec(_cfg(depth_clipping_behavior="zero")).clipping == _native.CAM_CLIP_ZERO
    _spec(_cfg(update_period=4 / 200))  # one env step is not stale
    _spec(_cfg(prim_path="/World/envs/env_.*/Robot/walker3d"), root_body="walker3d")
    big = _spec(_cfg(pattern_cfg=_pinhole(128, 128)))
    assert big.num_rays == _native.MAX_CAMERA_RAYS == 16384


def _pinhole(w, h, **kw):
    from allsteps_isaaclab_amd.utils.sensors import patterns

    return patterns.PinholeCameraPatternCfg(width=w, height=h, **kw)


def test_every_refusal_names_its_field():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCameraCfg, patterns

    def offset_starts(cfg, k, device):
        starts, dirs = patterns.pinhole_camera_pattern(cfg, k, device)
        return starts + 0.01, dirs

    Off = RayCasterCameraCfg.OffsetCfg
    refused = [
        ("prim_path", dict(prim_path="/World/envs/env_.*/Robot/LF_FOOT")),      # not the root body
        ("prim_path", dict(prim_path="")),
        ("mesh_prim_paths", dict(mesh_prim_paths=["/World/terrain"])),
        ("mesh_prim_paths", dict(mesh_prim_paths=["/World/ground", "/World/envs/env_.*/Robot"])),
        ("mesh_prim_paths", dict(mesh_prim_paths=[])),
        ("data_types", dict(data_types=[])),
        ("data_types", dict(data_types="normals")),
        ("depth_clipping_behavior", dict(depth_clipping_behavior="clip")),
        (r"offset\.convention", dict(offset=Off(convention="usd"))),
        ("offset", dict(offset=Off(pos=(0.0, float("inf"), 0.0)))),
        ("offset", dict(offset=Off(rot=(0.0, 0.0, 0.0, 0.0)))),
        ("pattern_cfg", dict(pattern_cfg=patterns.GridPatternCfg(resolution=0.1, size=[1.6, 1.0]))),  # not a pinhole
        ("pattern_cfg", dict(pattern_cfg=_pinhole(0, 4))),
        ("pattern_cfg", dict(pattern_cfg=_pinhole(4, -1))),
        ("pattern_cfg", dict(pattern_cfg=_pinhole(4.0, 4))),
        ("pattern_cfg", dict(pattern_cfg=_pinhole(True, 4))),
        ("pattern_cfg", dict(pattern_cfg=_pinhole(129, 128))),                  # more than AS_MAX_CAMERA_RAYS
        ("pattern_cfg", dict(pattern_cfg=_pinhole(4, 4, func=offset_starts))),  # starts that are not all zero
        ("pattern_cfg", dict(pattern_cfg=_pinhole(4, 4, focal_length=float("nan")))),
        ("pattern_cfg", dict(pattern_cfg=_pinhole(4, 4, horizontal_aperture=0.0))),
        ("update_period", dict(update_period=0.1)),                              # > step_dt = 0.02
        ("history_length", dict(history_length=2)),
        ("debug_vis", dict(debug_vis=True)),
        ("drift_range", dict(drift_range=(-0.1, 0.1))),
        ("max_distance", dict(max_distance=0.0)),
        ("max_distance", dict(max_distance=float("inf"))),
        ("max_distance", dict(max_distance=float("nan"))),
    ]
    for field, kw in refused:
        with pytest.raises(_native.NativeError, match=rf"cfg\.camera\.{field}:") as e:
            _spec(_cfg(**kw))
        assert "HIP kernel" in str(e.value), field
    with pytest.raises(_native.NativeError, match="AS_MAX_CAMERA_RAYS = 16384"):
        _spec(_cfg(pattern_cfg=_pinhole(129, 128)))
    with pytest.raises(_native.NativeError, match=r"cfg\.camera\['front'\]\.max_distance:"):
        _spec(_cfg(max_distance=-1.0), name="front")
    # a regex in the leaf: the reference's own error (ray_caster.py:61-67)
    with pytest.raises(RuntimeError, match="Invalid prim path for the ray-caster sensor: .*\n\tHint: Please ensure "
                                           "that the prim path does not contain any regex patterns in the leaf."):
        _spec(_cfg(prim_path="/World/envs/env_.*/Robot/.*"))
    # the reference's own ValueErrors (ray_caster_camera.py:331-342, :366)
    with pytest.raises(ValueError, match="RayCasterCamera class does not support the following sensor types: "
                                         r"\{'rgb'\}"):
        _spec(_cfg(data_types=["distance_to_camera", "rgb"]))
    with pytest.raises(ValueError, match="RayCasterCamera class does not support"):
        _spec(_cfg(data_types=["semantic_segmentation"]))
    with pytest.raises(ValueError, match="Received unknown data type: depth. Please check the configuration."):
        _spec(_cfg(data_types=["depth"]))


def test_named_cfgs():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.ray_camera import named_cfgs

    one = _cfg()
    assert named_cfgs(one) == {"camera": one}
    assert list(named_cfgs({"front": one, "down": one})) == ["front", "down"]
    for bad in ({}, {"": one}, {3: one}, {str(i): one for i in range(5)}):
        with pytest.raises(_native.NativeError, match=r"cfg\.camera:"):
            named_cfgs(bad)


def test_compat_shims_import_the_reference_names():
    site = os.path.join(ROOT, "allsteps_isaaclab_amd", "compat", "site")
    code = ("from isaaclab.sensors import RayCasterCameraCfg, RayCasterCfg, patterns\n"
            "from isaaclab.sensors.patterns import PinholeCameraPatternCfg, pinhole_camera_pattern\n"
            "from isaaclab.envs import mdp\n"
            "from isaaclab.managers import SceneEntityCfg\n"
            "import allsteps_isaaclab_amd.utils.sensors as S\n"
            "assert RayCasterCameraCfg is S.RayCasterCameraCfg and issubclass(RayCasterCameraCfg, RayCasterCfg)\n"
            "assert PinholeCameraPatternCfg is S.patterns.PinholeCameraPatternCfg is patterns.PinholeCameraPatternCfg\n"
            "assert pinhole_camera_pattern is S.patterns.pinhole_camera_pattern and mdp.image is S.image\n"
            "c = RayCasterCameraCfg(prim_path='{ENV_REGEX_NS}/Robot/base', mesh_prim_paths=['/World/ground'],\n"
            "                       offset=RayCasterCameraCfg.OffsetCfg(pos=(0.3, 0.0, 0.2), convention='world'),\n"
            "                       data_types=['distance_to_image_plane'], max_distance=10.0,\n"
            "                       pattern_cfg=patterns.PinholeCameraPatternCfg(width=32, height=24))\n"
            "print(c.pattern_cfg.width * c.pattern_cfg.height, c.attach_yaw_only, SceneEntityCfg('camera').name)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([site, ROOT]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split() == ["768", "False", "camera"]


def _fake_env(n=6, calls=None):
    def ray_camera(cfg, dirs, offset, pose, plane=None, camera=None, normals=None, stream=None):
        calls.append((cfg.width * cfg.height, plane is not None, camera is not None, normals is not None))

    nat = types.SimpleNamespace(ray_camera=ray_camera)
    state = {"root_pos": torch.zeros(3, n), "root_quat": torch.zeros(4, n)}
    state["root_quat"][0] = 1.0
    return types.SimpleNamespace(num_envs=n, _device=torch.device("cpu"), device="cpu", step_dt=0.02, _native=nat,
                                 model={"body_names": ["base", "LF_HIP"]}, cfg=types.SimpleNamespace(),
                                 _stream=lambda: None, state=state)


def test_data_views_are_zero_copy_and_lazy_on_a_fake_env():
    """_RayCasterCamera over a fake env whose handle counts the launches: zero-copy (N, H, W, C) views of the
    env-major buffers, one launch per change however often the data is read, update(force_recompute=True) always,
    the frame counter, set_world_poses and set_intrinsic_matrices."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.views import _RayCasterCamera

    calls = []
    env = _fake_env(6, calls)
    s = _RayCasterCamera(env, _cfg(mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_.*"],
                                   data_types=list(TYPES)))
    assert s.num_rays == 247 and s.image_shape == (13, 19) and s.launches == 0 and calls == []
    assert s.num_instances == 6 and s.device == "cpu" and s.frame.dtype == torch.int64 and s.frame.shape == (6,)
    d = s.data
    assert calls == [(247, True, True, True)] and s.launches == 1 and s.frame.tolist() == [1] * 6
    assert d.image_shape == (13, 19) and set(d.output) == set(TYPES) and d.info == [{t: None for t in TYPES}] * 6
    assert d.output["distance_to_image_plane"].shape == d.output["distance_to_camera"].shape == (6, 13, 19, 1)
    assert d.output["normals"].shape == (6, 13, 19, 3)
    for t in TYPES:
        assert d.output[t].data_ptr() == s.images[t].data_ptr() and d.output[t].is_contiguous()
    assert d.pos_w.shape == (6, 3) and d.pos_w.data_ptr() == s.pose.data_ptr()
    assert d.quat_w_world.shape == (6, 4) and d.quat_w_world.data_ptr() == s.pose[3].data_ptr()
    assert d.intrinsic_matrices.shape == (6, 3, 3) and float(d.intrinsic_matrices[4, 2, 2]) == 1.0
    s.pose[3] = 1.0  # identity "world" orientation: looking along +x with z up
    assert torch.allclose(d.quat_w_ros, torch.tensor([0.5, -0.5, 0.5, -0.5]).expand(6, 4))
    assert torch.allclose(d.quat_w_opengl, torch.tensor([0.5, 0.5, -0.5, -0.5]).expand(6, 4))
    s.images["distance_to_camera"][4, 19 * 2 + 5, 0] = 7.0
    assert float(s.data.output["distance_to_camera"][4, 2, 5, 0]) == 7.0 and s.launches == 1  # a second read: no launch
    s.update(0.02)
    s.mark_dirty()
    s.update(0.02)
    assert s.launches == 1  # lazy: the read decides
    s.data, s.data
    assert s.launches == 2
    s.update(0.0, force_recompute=True)
    s.update(0.0, force_recompute=True)
    assert s.launches == 4 and s.frame.tolist() == [4] * 6
    s.reset([1, 2])
    assert s.frame.tolist() == [4, 0, 0, 4, 4, 4]
    s.data
    assert s.launches == 5 and s.frame.tolist() == [5, 1, 1, 5, 5, 5]
    s.reset(torch.tensor([True, False, False, False, False, True]))
    assert s.frame.tolist() == [0, 1, 1, 5, 5, 0]
    s.reset()
    assert s.frame.tolist() == [0] * 6
    # set_world_poses: the roots are at the origin with the identity orientation, so the offset is the pose itself
    s.data
    before = s.offset.clone()
    s.set_world_poses(torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), torch.tensor([[1.0, 0, 0, 0]] * 2), [0, 3],
                      convention="world")
    assert s.offset[:, 0].tolist() == [1, 2, 3, 1, 0, 0, 0] and s.offset[:, 3].tolist() == [4, 5, 6, 1, 0, 0, 0]
    assert torch.equal(s.offset[:, [1, 2, 4, 5]], before[:, [1, 2, 4, 5]])
    launches = s.launches
    s.data
    assert s.launches == launches + 1  # moved: outdated
    s.set_world_poses(orientations=torch.tensor([[1.0, 0, 0, 0]]), env_ids=[1])  # "ros"
    assert torch.allclose(s.offset[3:, 1].abs(), torch.full((4,), 0.5)) and torch.equal(s.offset[:3, 1], before[:3, 1])
    with pytest.raises(ValueError, match="convention"):
        s.set_world_poses(orientations=torch.tensor([[1.0, 0, 0, 0]]), env_ids=[1], convention="usd")
    with pytest.raises(NotImplementedError):
        s.set_world_poses_from_view(torch.zeros(6, 3), torch.ones(6, 3))
    # set_intrinsic_matrices: all envs, equal matrices; the device directions are rewritten in place
    ptr, old = s.dirs.data_ptr(), s.dirs.clone()
    k = s.data.intrinsic_matrices[0].clone()
    k[0, 0] *= 2
    launches = s.launches
    s.set_intrinsic_matrices(k.expand(6, 3, 3), focal_length=2.0)
    assert s.dirs.data_ptr() == ptr and not torch.equal(s.dirs, old) and torch.equal(s.intrinsic_matrices[5], k)
    s.data
    assert s.launches == launches + 1
    s.set_intrinsic_matrices(k, env_ids=list(range(6)))
    per_env = k.repeat(6, 1, 1)
    per_env[2, 0, 0] += 1
    for kw in (dict(matrices=per_env), dict(matrices=k, env_ids=[0, 1])):
        with pytest.raises(_native.NativeError, match="per-env intrinsics are not served"):
            s.set_intrinsic_matrices(**kw)
    text = str(s)
    assert text.startswith("Ray-Caster-Camera @ '/World/envs/env_.*/Robot/base': \n")
    assert "\tnumber of meshes     : 2 (ground, stones)\n" in text and "\tnumber of sensors    : 6\n" in text
    assert "\tnumber of rays/sensor: 247\n" in text and "\ttotal number of rays : 1482\n" in text
    assert text.endswith("\timage shape          : (13, 19)") and "\tupdate period (s)    : 0.0\n" in text


def test_only_the_requested_data_types_are_allocated_and_launched():
    from allsteps_isaaclab_amd.envs.views import _RayCasterCamera

    calls = []
    s = _RayCasterCamera(_fake_env(3, calls), _cfg(pattern_cfg=_pinhole(8, 6)))
    assert set(s.data.output) == {"distance_to_image_plane"} and calls == [(48, True, False, False)]
    s = _RayCasterCamera(_fake_env(3, calls), _cfg(pattern_cfg=_pinhole(8, 6), data_types=["normals"]))
    assert set(s.data.output) == {"normals"} and calls[-1] == (48, False, False, True)


def test_image_is_the_reference_function():
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg
    from allsteps_isaaclab_amd.utils.sensors import image

    depth = torch.rand(3, 4, 5, 1)
    depth[1, 2, 3, 0] = float("inf")
    plane = torch.rand(3, 4, 5, 1)
    plane[0, 0, 0, 0] = float("nan")
    sensor = types.SimpleNamespace(data=types.SimpleNamespace(
        output={"distance_to_camera": depth, "distance_to_image_plane": plane, "normals": torch.ones(3, 4, 5, 3)}))
    env = types.SimpleNamespace(scene=types.SimpleNamespace(sensors={"camera": sensor}))
    cfg = SceneEntityCfg("camera")
    raw = image(env, cfg, "distance_to_camera", normalize=False)
    assert torch.equal(raw, depth) and raw.data_ptr() != depth.data_ptr() and float(raw[1, 2, 3, 0]) == float("inf")
    got = image(env, cfg, "distance_to_camera")
    assert float(got[1, 2, 3, 0]) == 0.0 and float(depth[1, 2, 3, 0]) == 0.0  # in place on the sensor's buffer
    assert got.data_ptr() != depth.data_ptr()
    assert bool(torch.isnan(image(env, cfg, "distance_to_image_plane")[0, 0, 0, 0]))  # only inf is replaced
    assert torch.equal(image(env, cfg, "normals"), torch.ones(3, 4, 5, 3))
    with pytest.raises(ValueError, match="rgb"):
        image(env, cfg)
    with pytest.raises(NotImplementedError, match="convert_perspective_to_orthogonal"):
        image(env, cfg, "distance_to_camera", convert_perspective_to_orthogonal=True)


def test_feature_off_env_has_no_camera_and_nothing_to_mark():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.envs.native_env import NativeDirectEnv

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = 4
    base = DirectRLEnv(cfg)
    assert base._lazy_sensors == () and base._cameras == () and base.scene.sensors == {}
    env = NativeDirectEnv(cfg)
    assert not hasattr(env, "camera") and env._lazy_sensors == ()
    marks = []
    env._add_lazy_sensor(types.SimpleNamespace(mark_dirty=lambda: marks.append("a")))
    env._add_lazy_sensor(types.SimpleNamespace(mark_dirty=lambda: marks.append("b"),
                                               reset=lambda ids: marks.append(("reset", ids))), camera=True)
    env._scene_changed()
    env._sensors_reset(None)
    assert marks == ["a", "b", ("reset", None)] and DirectRLEnv._lazy_sensors == ()  # per instance


def test_abi_exports_the_entry_point_and_refuses_before_any_device_call():
    from allsteps_isaaclab_amd import _native

    assert "as_ray_camera" in _native.EXPORTED_SYMBOLS
    with open(os.path.join(_native.INCLUDE, "allsteps.h")) as f:
        header = f.read()
    assert re.search(r"#define AS_ABI_VERSION 6\b", header)
    assert re.search(r"#define AS_MAX_CAMERA_RAYS 16384\b", header)
    for name, value in (("NONE", 0), ("MAX", 1), ("ZERO", 2)):
        assert re.search(rf"#define AS_CAM_CLIP_{name} {value}\b", header)
    assert re.search(r"int as_ray_camera\(as_env_t\* env, const as_ray_camera_t\* cfg_host, const float\* dirs, "
                     r"const float\* offset,\s+float\* pose, float\* plane, float\* camera, float\* normals, "
                     r"void\* stream\);", header)
    assert re.search(r"int32_t width;\s+int32_t height;\s+int32_t surfaces;[^}]*int32_t clipping;[^}]*"
                     r"float max_distance;\s+float ground_z;\s+} as_ray_camera_t;", header)
    assert _native.MAX_CAMERA_RAYS == 16384 and C.sizeof(_native.AsRayCamera) == 24
    assert (_native.CAM_CLIP_NONE, _native.CAM_CLIP_MAX, _native.CAM_CLIP_ZERO) == (0, 1, 2)
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    good = dict(width=4, height=3, surfaces=3, clipping=0, max_distance=10.0, ground_z=0.0)

    def call(env=None, cfg=good, dirs=p, offset=p, pose=p, plane=p, camera=None, normals=None):
        c = None if cfg is None else C.byref(_native.AsRayCamera(**cfg))
        rc = L.as_ray_camera(env, c, dirs, offset, pose, plane, camera, normals, None)
        return rc, L.as_last_error().decode()

    # no handle anywhere: nothing here ever reaches a device call
    assert call() == (-1, "as_ray_camera: null argument env")
    for kw, text in ((dict(cfg=None), "null argument cfg"), (dict(dirs=None), "null argument dirs"),
                     (dict(offset=None), "null argument offset"), (dict(pose=None), "null argument pose"),
                     (dict(plane=None), "all null"),
                     (dict(cfg=dict(good, width=0)), "image 0 x 3"), (dict(cfg=dict(good, height=-2)), "image 4 x -2"),
                     (dict(cfg=dict(good, width=129, height=128)), "AS_MAX_CAMERA_RAYS = 16384"),
                     (dict(cfg=dict(good, width=65536, height=65536)), "AS_MAX_CAMERA_RAYS = 16384"),
                     (dict(cfg=dict(good, surfaces=0)), "surfaces 0"), (dict(cfg=dict(good, surfaces=4)), "surfaces 4"),
                     (dict(cfg=dict(good, clipping=3)), "clipping 3"),
                     (dict(cfg=dict(good, clipping=-1)), "clipping -1"),
                     (dict(cfg=dict(good, max_distance=0.0)), "max_distance"),
                     (dict(cfg=dict(good, max_distance=float("inf"))), "max_distance"),
                     (dict(cfg=dict(good, max_distance=float("nan"))), "max_distance"),
                     (dict(cfg=dict(good, ground_z=float("nan"))), "ground_z")):
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("as_ray_camera: ") and text in err, (kw, err)
    assert call(plane=None, normals=p)[1] == "as_ray_camera: null argument env"  # one image is enough


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_compiles_without_scratch_or_spills(tmp_path):
    """k_ray_camera with the package's own flags (_native.STEP_FLAGS): no scratch, no VGPR or SGPR spill, no LDS; the
    env's pose, offset and stones are uniform, so the lanes keep one pixel each in a few dozen VGPRs."""
    from allsteps_isaaclab_amd import _native

    src = tmp_path / "camera.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "allsteps.h"\n#include "allsteps_device.h"\n'
                   '#include "ray_camera_kernels.h"\n')
    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "-I", _native.CSRC, "--cuda-device-only", "-S", "-o",
                        str(tmp_path / "camera.s"), "-Rpass-analysis=kernel-resource-usage", str(src)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Function Name: _ZN2as12k_ray_camera" in r.stderr
    res = dict(re.findall(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?):\s+(\S+) \[-Rpass", r.stderr))
    print(res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0 and int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0 and int(res["AGPRs"]) == 0, res
    assert int(res["VGPRs"]) <= 64, res  # 33 as written: eight waves per SIMD
    assert int(res["Occupancy [waves/SIMD]"]) == 8, res
