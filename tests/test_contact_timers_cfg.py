"""The contact timers' Python surface and build, no GPU: the cfg fields with the reference's defaults, the sensor
data and methods with the feature off (None, RuntimeError, no state keys) and over hand-set timers, the C ABI's new
name and its refusals made before any device call, the kernel's compiled resource figures, and the fixture's
regeneration where a reference checkout is given (ALLSTEPS_REFERENCE)."""

import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _env_stub(timers=None):
    """What _FootSensor reads of its env for the timer views."""
    tm = None if timers is None else types.SimpleNamespace(timers=timers)
    return types.SimpleNamespace(_contact_timers=tm)


def _sensors(env):
    from allsteps_isaaclab_amd.envs.views import _FootSensor

    return (_FootSensor(env, [0], ["right_foot"], True), _FootSensor(env, [1], ["left_foot"], True),
            _FootSensor(env, [0, 1], ["right_foot", "left_foot"], False))


def test_cfg_fields_exist_with_the_reference_defaults():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.contact_air_time is False  # ContactSensorCfg.track_air_time
        assert cfg.contact_force_threshold == 1.0  # ContactSensorCfg.force_threshold
        assert cfg.contact_forces is False


def test_feature_off_data_is_none_and_the_methods_raise():
    for s in _sensors(_env_stub()):
        for name in ("current_air_time", "last_air_time", "current_contact_time", "last_contact_time"):
            assert getattr(s.data, name) is None
        for fn in (s.compute_first_contact, s.compute_first_air):
            with pytest.raises(RuntimeError, match="not configured to track contact time"):
                fn(1 / 60)


def test_feature_off_env_has_no_timers_no_state_keys_and_nothing_to_launch():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.envs.native_env import NativeDirectEnv
    from allsteps_isaaclab_amd.envs.state import alloc_state

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = 4
    base = DirectRLEnv(cfg)
    assert base._sensors is None and base._sensors_reset(None) is None
    env = NativeDirectEnv(cfg)  # no handle: the state paths alone
    assert env._contact_timers is None and env._sensors is None
    env.state = alloc_state(4, torch.device("cpu"))
    keys = set(env.get_state())
    assert keys == set(env.state) and not any(k.startswith("contact_t") for k in keys)
    env._sensors_reset(None)  # nothing to launch: no handle is touched


def test_views_are_zero_copy_transposes_of_the_one_set_of_timers():
    n = 5
    timers = torch.arange(4 * 2 * n, dtype=torch.float32).reshape(4, 2, n)
    right, left, both = _sensors(_env_stub(timers))
    names = ("current_air_time", "last_air_time", "current_contact_time", "last_contact_time")
    for row, name in enumerate(names):
        for s, lo, hi in ((right, 0, 1), (left, 1, 2), (both, 0, 2)):
            v = getattr(s.data, name)
            assert v.shape == (n, hi - lo) and torch.equal(v, timers[row, lo:hi].T)
            assert v.data_ptr() == timers[row, lo].data_ptr()  # a view, not a copy
    timers[2, 1, 3] = 77.0
    assert float(left.data.current_contact_time[3, 0]) == 77.0 == float(both.data.current_contact_time[3, 1])
    # a quadruped's four-foot sensor
    from allsteps_isaaclab_amd.envs.views import _FootSensor

    t4 = torch.rand(4, 4, n)
    quad = _FootSensor(_env_stub(t4), [0, 1, 2, 3], ["RF", "LF", "RH", "LH"], True)
    assert torch.equal(quad.data.last_air_time, t4[1].T)


def test_compute_first_contact_and_air_are_the_reference_formulas():
    dt = 4 / 240
    cur = torch.tensor([0.0, 1 / 240, dt, dt + 5e-9, dt + 1 / 240, 3.0])
    timers = torch.zeros(4, 2, cur.numel())
    timers[2, 0], timers[0, 1] = cur, cur  # foot 0: contact times, foot 1: air times
    right, left, both = _sensors(_env_stub(timers))
    want = (cur > 0.0) * (cur < (dt + 1.0e-8))
    assert want.tolist() == [False, True, True, True, False, False]
    assert torch.equal(right.compute_first_contact(dt)[:, 0], want)
    assert torch.equal(left.compute_first_air(dt)[:, 0], want)
    assert not right.compute_first_air(dt).any() and not left.compute_first_contact(dt).any()
    assert torch.equal(both.compute_first_contact(dt), torch.stack([want, torch.zeros_like(want)], 1))
    assert torch.equal(right.compute_first_contact(dt, abs_tol=0.0)[:, 0], (cur > 0.0) * (cur < dt))


def test_state_keys_round_trip_on_the_host():
    from allsteps_isaaclab_amd.envs.views import _ContactTimers

    assert _ContactTimers.STATE_KEYS == ("contact_timers", "contact_timestamp")
    tm = object.__new__(_ContactTimers)
    tm.timers, tm.timestamp = torch.rand(4, 2, 3), torch.rand(3)
    st = tm.get_state()
    assert set(st) == set(_ContactTimers.STATE_KEYS) and st["contact_timers"] is not tm.timers
    tm.timers.zero_(), tm.timestamp.zero_()
    tm.set_state({**st, "q": torch.zeros(1)})
    assert torch.equal(tm.timers, st["contact_timers"]) and torch.equal(tm.timestamp, st["contact_timestamp"])


def test_abi_exports_the_entry_point_and_refuses_before_any_device_call():
    from allsteps_isaaclab_amd import _native

    assert "as_contact_timers" in _native.EXPORTED_SYMBOLS
    with open(os.path.join(_native.INCLUDE, "allsteps.h")) as f:
        header = f.read()
    assert re.search(r"#define AS_ABI_VERSION 6\b", header)
    assert re.search(r"int as_contact_timers\(as_env_t\* env, const as_body_table_t\* bodies_host, float\* timers",
                     header)
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    table = _native.AsBodyTable()
    table.num_bodies = 2
    # no handle: refused as a null argument, as are null timers / timestamp / bodies with any handle value
    assert L.as_contact_timers(None, None, p, p, 1.0, 0, None, None, None) == -1
    assert b"as_contact_timers: null argument" in L.as_last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_compiles_without_scratch_or_spills(tmp_path):
    """k_contact_timers with the package's own flags (_native.STEP_FLAGS): no scratch, no VGPR or SGPR spill, no
    LDS -- the kernel's timers, links and a slot's records all live in registers."""
    from allsteps_isaaclab_amd import _native

    src = tmp_path / "timers.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "allsteps.h"\n#include "allsteps_device.h"\n'
                   '#include "contact_timer_kernels.h"\n')
    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "-I", _native.CSRC, "--cuda-device-only", "-S", "-o",
                        str(tmp_path / "timers.s"), "-Rpass-analysis=kernel-resource-usage", str(src)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Function Name: _ZN2as16k_contact_timers" in r.stderr
    res = dict(re.findall(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?):\s+(\S+) \[-Rpass", r.stderr))
    print(res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0 and int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0 and int(res["AGPRs"]) == 0, res
    assert int(res["VGPRs"]) <= 128, res  # 70 as written: four waves per SIMD or more


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_contact_timers.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
