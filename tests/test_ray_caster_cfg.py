"""The ray caster's Python surface and build, no GPU: the cfg classes with the reference's fields and defaults, the grid
pattern bit-equal to the fixture's local rays, every refusal with the field it names, the compat shims, height_scan's
formula, the feature-off env (no sensor, no state keys), the C ABI's new name and its refusals made before any device
call, and the kernel's compiled resource figures."""

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


def _cfg(**kw):
    """The velocity task's height scanner (velocity_env_cfg.py:66-73) on the quadruped's base."""
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg, patterns

    base = dict(prim_path="/World/envs/env_.*/Robot/base", offset=RayCasterCfg.OffsetCfg(pos=(0.0, 0.0, 20.0)),
                attach_yaw_only=True, pattern_cfg=patterns.GridPatternCfg(resolution=0.1, size=[1.6, 1.0]),
                debug_vis=False, mesh_prim_paths=["/World/ground"])
    base.update(kw)
    return RayCasterCfg(**base)


def _spec(cfg, **kw):
    from allsteps_isaaclab_amd.envs.ray_caster import RayCasterSpec

    args = dict(root_body="base", step_dt=4 / 200, step_paths=())
    args.update(kw)
    return RayCasterSpec(cfg, **args)


def test_cfg_classes_have_the_reference_fields_and_defaults():
    from allsteps_isaaclab_amd.utils.noise import MISSING
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg, patterns

    f = {x.name: x for x in dataclasses.fields(RayCasterCfg)}
    assert list(f) == ["prim_path", "update_period", "history_length", "debug_vis", "mesh_prim_paths", "offset",
                       "attach_yaw_only", "pattern_cfg", "max_distance", "drift_range"]
    c = RayCasterCfg()
    assert c.prim_path is MISSING and c.mesh_prim_paths is MISSING and c.attach_yaw_only is MISSING
    assert c.pattern_cfg is MISSING
    assert (c.update_period, c.history_length, c.debug_vis, c.max_distance, c.drift_range) == \
        (0.0, 0, False, 1e6, (0.0, 0.0))
    assert c.offset == RayCasterCfg.OffsetCfg() and c.offset is not RayCasterCfg().offset
    assert (c.offset.pos, c.offset.rot) == ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    g = patterns.GridPatternCfg()
    assert [x.name for x in dataclasses.fields(g)] == ["func", "resolution", "size", "direction", "ordering"]
    assert g.func is patterns.grid_pattern and g.resolution is MISSING and g.size is MISSING
    assert g.direction == (0.0, 0.0, -1.0) and g.ordering == "xy"
    assert issubclass(patterns.GridPatternCfg, patterns.PatternBaseCfg)
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    assert AllstepsEnvCfg().height_scanner is None and AnymalCStonesEnvCfg().height_scanner is None


def test_grid_pattern_is_bit_equal_to_the_reference_local_rays():
    """The fixture's local rays are the reference's grid_pattern + offset; cases y (xy), f (xy, rotated offset) and d
    (yx, slanted direction)."""
    from _ray_caster_cases import load_cases

    from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg, patterns

    for c in load_cases():
        k = c["cfg"]
        pat = patterns.GridPatternCfg(resolution=k["resolution"], size=k["size"], direction=tuple(k["direction"]),
                                      ordering=k["ordering"])
        starts, dirs = patterns.grid_pattern(pat, "cpu")
        assert starts.shape == dirs.shape == (c["num_rays"], 3) and starts.dtype == torch.float32
        if k["offset_rot"] == [1.0, 0.0, 0.0, 0.0]:  # bare pattern: start + offset pos is all that happens
            want = c["rays"][:3].T - np.asarray(k["offset_pos"], np.float32)
            assert np.array_equal((starts.numpy() + np.asarray(k["offset_pos"], np.float32)).view(np.uint32),
                                  c["rays"][:3].T.copy().view(np.uint32)), (c["name"], want[:2])
        spec = _spec(_cfg(offset=RayCasterCfg.OffsetCfg(pos=tuple(k["offset_pos"]), rot=tuple(k["offset_rot"])),
                          attach_yaw_only=k["attach_yaw_only"], pattern_cfg=pat))
        assert spec.num_rays == c["num_rays"] and spec.rays.shape == (6, c["num_rays"])
        assert np.array_equal(spec.rays.numpy().view(np.uint32), c["rays"].view(np.uint32)), c["name"]
    # the orderings differ in which index runs fastest
    xy = patterns.grid_pattern(patterns.GridPatternCfg(resolution=0.5, size=[1.0, 0.5]), "cpu")[0]
    yx = patterns.grid_pattern(patterns.GridPatternCfg(resolution=0.5, size=[1.0, 0.5], ordering="yx"), "cpu")[0]
    assert xy[:3, 0].tolist() == [-0.5, 0.0, 0.5] and yx[:2, 1].tolist() == [-0.25, 0.25] and len(xy) == len(yx) == 6


def test_grid_pattern_raises_the_reference_value_errors():
    from allsteps_isaaclab_amd.utils.sensors import patterns

    with pytest.raises(ValueError, match="Ordering must be 'xy' or 'yx'. Received: 'zz'."):
        patterns.grid_pattern(patterns.GridPatternCfg(resolution=0.1, size=[1, 1], ordering="zz"), "cpu")
    with pytest.raises(ValueError, match="Resolution must be greater than 0. Received: '0'."):
        patterns.grid_pattern(patterns.GridPatternCfg(resolution=0, size=[1, 1]), "cpu")


def test_any_pattern_function_of_the_reference_protocol_is_accepted():
    def three(cfg, device):
        return torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], device=device), torch.tensor([[0.0, 0, -1]] * 3)

    spec = _spec(_cfg(pattern_cfg=types.SimpleNamespace(func=three), mesh_prim_paths=["/World/envs/env_.*/step_.*"]))
    assert spec.num_rays == 3 and spec.surfaces == 2 and spec.rays[2].tolist() == [20.0, 20.0, 20.0]
    both = _spec(_cfg(mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_3"]),
                 step_paths=[f"/World/envs/env_.*/step_{i}" for i in range(20)])
    assert both.surfaces == 3 and both.surface_names() == ["ground", "stones"]
    c = both.native_cfg()
    assert (c.num_rays, c.attach_yaw_only, c.surfaces, c.max_distance, c.ground_z) == (187, 1, 3, 1e6, 0.0)


def test_every_refusal_names_its_field():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg, patterns

    def many(cfg, device):
        return torch.zeros(_native.MAX_RAYS + 1, 3), torch.zeros(_native.MAX_RAYS + 1, 3)

    def bad_shape(cfg, device):
        return torch.zeros(4, 2), torch.zeros(4, 2)

    nan_dir = patterns.GridPatternCfg(resolution=0.1, size=[0.2, 0.2], direction=(0.0, float("nan"), -1.0))
    refused = [
        ("prim_path", dict(prim_path="/World/envs/env_.*/Robot/LF_FOOT")),      # not the root body
        ("mesh_prim_paths", dict(mesh_prim_paths=["/World/terrain"])),
        ("mesh_prim_paths", dict(mesh_prim_paths=["/World/ground", "/World/envs/env_.*/Robot"])),
        ("mesh_prim_paths", dict(mesh_prim_paths=[])),
        ("drift_range", dict(drift_range=(-0.1, 0.1))),
        ("update_period", dict(update_period=0.1)),                              # > step_dt = 0.02
        ("debug_vis", dict(debug_vis=True)),
        ("pattern_cfg", dict(pattern_cfg=types.SimpleNamespace(func=many))),    # more than AS_MAX_RAYS
        ("pattern_cfg", dict(pattern_cfg=types.SimpleNamespace(func=bad_shape))),
        ("pattern_cfg", dict(pattern_cfg=nan_dir)),                             # a non-finite pattern
        ("offset", dict(offset=RayCasterCfg.OffsetCfg(pos=(0.0, float("inf"), 0.0)))),
        ("max_distance", dict(max_distance=0.0)),
        ("attach_yaw_only", dict(attach_yaw_only=RayCasterCfg().attach_yaw_only)),  # left MISSING
    ]
    for field, kw in refused:
        with pytest.raises(_native.NativeError, match=rf"cfg\.height_scanner\.{field}:") as e:
            _spec(_cfg(**kw))
        assert "HIP kernel" in str(e.value)
    with pytest.raises(_native.NativeError, match="AS_MAX_RAYS = 1024"):
        _spec(_cfg(pattern_cfg=types.SimpleNamespace(func=many)))
    # a regex in the leaf: the reference's own error (ray_caster.py:61-67)
    with pytest.raises(RuntimeError, match="Invalid prim path for the ray-caster sensor: .*\n\tHint: Please ensure "
                                           "that the prim path does not contain any regex patterns in the leaf."):
        _spec(_cfg(prim_path="/World/envs/env_.*/Robot/.*"))
    _spec(_cfg(update_period=4 / 200))  # one env step is not stale
    _spec(_cfg(prim_path="/World/envs/env_.*/Robot/walker3d"), root_body="walker3d")


def test_compat_shims_import_the_reference_names():
    site = os.path.join(ROOT, "allsteps_isaaclab_amd", "compat", "site")
    code = ("from isaaclab.sensors import RayCasterCfg, patterns\n"
            "from isaaclab.sensors.patterns import GridPatternCfg, grid_pattern\n"
            "from isaaclab.envs import mdp\n"
            "from isaaclab.managers import SceneEntityCfg\n"
            "import allsteps_isaaclab_amd.utils.sensors as S\n"
            "assert RayCasterCfg is S.RayCasterCfg and patterns.GridPatternCfg is S.patterns.GridPatternCfg\n"
            "assert GridPatternCfg is patterns.GridPatternCfg and grid_pattern is S.patterns.grid_pattern\n"
            "assert mdp.height_scan is S.height_scan and callable(mdp.push_by_setting_velocity)\n"
            "c = RayCasterCfg(prim_path='{ENV_REGEX_NS}/Robot/base', offset=RayCasterCfg.OffsetCfg(pos=(0.0, 0.0, 20.0)),\n"
            "                 attach_yaw_only=True, pattern_cfg=patterns.GridPatternCfg(resolution=0.1, size=[1.6, 1.0]),\n"
            "                 debug_vis=False, mesh_prim_paths=['/World/ground'])\n"
            "print(len(c.pattern_cfg.func(c.pattern_cfg, 'cpu')[0]), SceneEntityCfg('height_scanner').name)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([site, ROOT]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split() == ["187", "height_scanner"]


def test_height_scan_is_the_reference_formula():
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg
    from allsteps_isaaclab_amd.utils.sensors import height_scan

    n, R = 3, 5
    pos = torch.rand(n, 3) + 20.0
    hits = torch.rand(n, R, 3)
    hits[1, 2] = float("inf")
    sensor = types.SimpleNamespace(data=types.SimpleNamespace(pos_w=pos, ray_hits_w=hits))
    env = types.SimpleNamespace(scene=types.SimpleNamespace(sensors={"height_scanner": sensor}))
    for offset in (0.5, 0.0):
        kw = {} if offset == 0.5 else {"offset": offset}
        got = height_scan(env, SceneEntityCfg("height_scanner"), **kw)
        assert got.shape == (n, R)
        assert torch.equal(got, pos[:, 2].unsqueeze(1) - hits[..., 2] - offset)
    assert got[1, 2] == -float("inf")


def test_data_views_are_zero_copy_and_lazy_on_a_fake_env():
    """_RayCaster over a fake env whose handle counts the launches: strided views of the env-minor buffers, one
    launch per change of the scene however often the data is read, and update(force_recompute=True) always."""
    from allsteps_isaaclab_amd.envs.views import _RayCaster

    calls = []
    nat = types.SimpleNamespace(ray_cast=lambda cfg, rays, hits, surface, pose, stream=None: calls.append(cfg.num_rays))
    env = types.SimpleNamespace(num_envs=6, _device=torch.device("cpu"), device="cpu", step_dt=0.02, _native=nat,
                                model={"body_names": ["base", "LF_HIP"]}, cfg=types.SimpleNamespace(),
                                _stream=lambda: None)
    s = _RayCaster(env, _cfg(mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_.*"]))
    assert s.num_rays == 187 and s.launches == 0 and calls == []
    d = s.data
    assert calls == [187] and s.launches == 1
    assert d.ray_hits_w.shape == (6, 187, 3) and d.pos_w.shape == (6, 3) and d.quat_w.shape == (6, 4)
    assert d.ray_hit_surface.shape == (6, 187) and d.ray_hit_surface.dtype == torch.int8
    assert d.ray_hits_w.data_ptr() == s.hits.data_ptr() and d.pos_w.data_ptr() == s.pose.data_ptr()
    assert d.quat_w.data_ptr() == s.pose[3].data_ptr() and d.ray_hit_surface.data_ptr() == s.surface.data_ptr()
    s.hits[2, 5, 4] = 7.0
    assert float(s.data.ray_hits_w[4, 5, 2]) == 7.0 and s.launches == 1  # a second read: no launch
    s.update(0.02)
    assert s.launches == 1
    s.mark_dirty()
    s.update(0.02)
    assert s.launches == 1  # lazy: the read decides
    s.data, s.data
    assert s.launches == 2
    s.update(0.0, force_recompute=True)
    s.update(0.0, force_recompute=True)
    assert s.launches == 4
    s.reset([1, 2])
    s.data
    assert s.launches == 5
    text = str(s)
    assert text.startswith("Ray-caster @ '/World/envs/env_.*/Robot/base': \n")
    assert "\tnumber of meshes     : 2 (ground, stones)\n" in text and "\tnumber of sensors    : 6\n" in text
    assert "\tnumber of rays/sensor: 187\n" in text and text.endswith("\ttotal number of rays : 1122")
    assert "\tupdate period (s)    : 0.0\n" in text


def test_feature_off_env_has_no_sensor_no_state_keys_and_nothing_to_launch():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.envs.native_env import NativeDirectEnv
    from allsteps_isaaclab_amd.envs.state import alloc_state

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = 4
    base = DirectRLEnv(cfg)
    assert base.scene.sensors == {} and base._scene_changed() is None
    env = NativeDirectEnv(cfg)  # no handle: the state paths alone
    assert env.height_scanner is None and env.scene.sensors == {}
    env.state = alloc_state(4, torch.device("cpu"))
    before = set(env.get_state())
    assert before == set(env.state)
    env._scene_changed()  # nothing to mark, no handle is touched
    env.set_state(env.get_state())
    assert set(env.get_state()) == before


def test_abi_exports_the_entry_point_and_refuses_before_any_device_call():
    from allsteps_isaaclab_amd import _native

    assert "as_ray_cast" in _native.EXPORTED_SYMBOLS
    with open(os.path.join(_native.INCLUDE, "allsteps.h")) as f:
        header = f.read()
    assert re.search(r"#define AS_ABI_VERSION 6\b", header)
    assert re.search(r"int as_ray_cast\(as_env_t\* env, const as_ray_caster_t\* cfg_host, const float\* rays, "
                     r"float\* hits, int8_t\* surface,\s+float\* pose, void\* stream\);", header)
    assert re.search(r"int32_t num_rays;\s+int32_t attach_yaw_only;\s+int32_t surfaces;[^}]*float max_distance;\s+"
                     r"float ground_z;\s+} as_ray_caster_t;", header)
    with open(os.path.join(_native.CSRC, "allsteps_consts.h")) as f:
        assert re.search(r"#define AS_MAX_RAYS 1024\b", f.read())
    assert _native.MAX_RAYS == 1024 and C.sizeof(_native.AsRayCaster) == 20
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    cfg = _native.AsRayCaster(4, 1, 3, 1e6, 0.0)
    # no handle: refused by name, whatever else is passed -- nothing here ever reaches a device call
    assert L.as_ray_cast(None, C.byref(cfg), p, p, None, None, None) == -1
    assert b"as_ray_cast: null argument env" in L.as_last_error()
    assert L.as_ray_cast(None, None, None, None, None, None, None) == -1
    assert b"as_ray_cast: null argument env" in L.as_last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_compiles_without_scratch_or_spills(tmp_path):
    """k_ray_cast with the package's own flags (_native.STEP_FLAGS): no scratch, no VGPR or SGPR spill, no LDS --
    the pose, the 60 stone coordinates and the ray in flight all live in registers."""
    from allsteps_isaaclab_amd import _native

    src = tmp_path / "rays.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "allsteps.h"\n#include "allsteps_device.h"\n'
                   '#include "ray_caster_kernels.h"\n')
    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "-I", _native.CSRC, "--cuda-device-only", "-S", "-o",
                        str(tmp_path / "rays.s"), "-Rpass-analysis=kernel-resource-usage", str(src)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Function Name: _ZN2as10k_ray_cast" in r.stderr
    res = dict(re.findall(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?):\s+(\S+) \[-Rpass", r.stderr))
    print(res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0 and int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0 and int(res["AGPRs"]) == 0, res
    assert int(res["VGPRs"]) <= 168, res  # 152 as written: three waves per SIMD
