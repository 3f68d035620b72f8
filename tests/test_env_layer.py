"""The host-side env layer, no GPU: the one state allocator (envs/state.py), the direction of the imports between
the env modules, the import names kept for tests / scripts / INTEGRATION.md, and the refusal of a CPU device."""

import importlib
import os
import subprocess
import sys

import pytest
import torch

from allsteps_isaaclab_amd import _native
from allsteps_isaaclab_amd.envs.state import alloc_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f": torch.float32, "i": torch.int32}


@pytest.mark.parametrize("n", [3, 66])
def test_alloc_state_layout(n):
    s = alloc_state(n, torch.device("cpu"))
    assert list(s) == [name for name, _, _ in _native.STATE_LAYOUT] + ["curriculum"]
    for name, rows, t in _native.STATE_LAYOUT:
        assert s[name].shape == ((rows, n) if rows > 1 else (n,)) and s[name].dtype == DTYPES[t], name
        assert s[name].is_contiguous()
    for t in DTYPES:  # one slab per dtype: each field starts where the one before it ends
        fields = [(name, rows) for name, rows, k in _native.STATE_LAYOUT if k == t]
        for (a, rows), (b, _) in zip(fields, fields[1:]):
            assert s[b].data_ptr() - s[a].data_ptr() == rows * n * 4, (a, b)
    assert s["curriculum"].shape == (1,) and s["curriculum"].dtype == torch.int32
    assert all(not bool(v.any()) for v in s.values())


@pytest.mark.parametrize("hind,feet", [(True, False), (False, True), (True, True)])
def test_alloc_state_quadruped_extras(hind, feet):
    n = 66
    s = alloc_state(n, torch.device("cpu"), hind=hind, feet=feet)
    assert ("contact_mask_hind" in s) == hind and ("feet" in s) == feet
    for name, rows, on in (("contact_mask_hind", 2, hind), ("feet", 8, feet)):
        if on:
            assert s[name].shape == (rows, n) and s[name].dtype == torch.int32 and not bool(s[name].any())
    # the extras are allocations of their own: the walker's slabs are what they are without them
    base = alloc_state(n, torch.device("cpu"))
    for name in base:
        assert s[name].shape == base[name].shape and s[name].stride() == base[name].stride()
    assert s["contact_mask"].data_ptr() - s["episode"].data_ptr() == n * 4


def test_quadruped_task_env_does_not_import_the_walker_env():
    code = ("import sys, allsteps_isaaclab_amd.envs.anymal_c_stones_env as m; "
            "assert 'allsteps_isaaclab_amd.envs.allsteps_env' not in sys.modules; "
            "assert 'allsteps_isaaclab_amd.envs.views' in sys.modules; print('ok', m.AnymalCStonesEnv.set_state)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("module,names", [
    ("envs.anymal_c_stones_env", ["level0_stones", "AnymalCStonesEnv"]),
    ("envs.quadruped", ["STAND_ROOT", "level0_stones", "stand_pose", "QuadrupedStonesEnv"]),
    ("envs.allsteps_env", ["AllstepsEnv", "get_symmetric_states_rsl_rl", "get_symmetric_states_rl_games"]),
])
def test_old_import_names_resolve(module, names):
    m = importlib.import_module("allsteps_isaaclab_amd." + module)
    for name in names:
        assert hasattr(m, name), f"{module}.{name}"


def test_registry_entry_points_resolve():
    from allsteps_isaaclab_amd import registry

    for task, cls in (("Allsteps-v0", "AllstepsEnv"), ("Allsteps-AnymalC-v0", "AnymalCStonesEnv")):
        module, _, name = registry.spec(task).entry_point.partition(":")
        assert name == cls and getattr(importlib.import_module(module), name).__name__ == cls


def test_quadruped_helpers_are_the_same_objects_and_values():
    import numpy as np

    from allsteps_isaaclab_amd.envs import anymal_c_stones_env, quadruped
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    assert anymal_c_stones_env.level0_stones is quadruped.level0_stones
    names = load_model(ANYMAL_C_JSON)["dof_names"]
    np.testing.assert_array_equal(quadruped.stand_pose(names), quadruped.stand_pose(names, quadruped.STAND_Q))
    st = quadruped.level0_stones(3)
    assert st.shape == (60, 3) and st.dtype == np.float32 and (st[3] == 0.75).all() and (st[1::3] == 0).all()


def test_quadruped_task_env_refuses_a_cpu_device():
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = 4
    cfg.sim.device = "cpu"
    with pytest.raises(_native.NativeError, match="AnymalCStonesEnv runs on the HIP backend only.*no CPU fallback"):
        AnymalCStonesEnv(cfg)
