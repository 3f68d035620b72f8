"""The noise models' Python surface, no GPU: the cfg fields, the reference-named cfg classes through the
compat import, the refusal of anything the device kernels do not implement, and the C ABI's new names."""

import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cfg_fields_default_to_none():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.action_noise_model is None and cfg.observation_noise_model is None


def test_cfg_classes_carry_the_reference_fields_and_defaults():
    from allsteps_isaaclab_amd.utils import noise as N

    assert N.NoiseCfg().operation == "add" and N.NoiseCfg().func is N.MISSING
    c, u, g = N.ConstantNoiseCfg(), N.UniformNoiseCfg(), N.GaussianNoiseCfg()
    assert (c.func, c.operation, c.bias) == (N.constant_noise, "add", 0.0)
    assert (u.func, u.operation, u.n_min, u.n_max) == (N.uniform_noise, "add", -1.0, 1.0)
    assert (g.func, g.operation, g.mean, g.std) == (N.gaussian_noise, "add", 0.0, 1.0)
    m, b = N.NoiseModelCfg(), N.NoiseModelWithAdditiveBiasCfg()
    assert m.class_type is N.NoiseModel and m.noise_cfg is N.MISSING
    assert b.class_type is N.NoiseModelWithAdditiveBias and b.noise_cfg is N.MISSING and b.bias_noise_cfg is N.MISSING
    with pytest.raises(NotImplementedError, match="no host implementation"):
        g.func(torch.zeros(2, 2), g)


def test_reference_style_construction_through_the_compat_import():
    """A reference cfg's noise block, written against isaaclab.utils.noise, builds the env's device state (on
    the CPU here: tensors only, the kernels are not launched)."""
    code = """
from allsteps_isaaclab_amd import compat
compat.install()
import torch
from isaaclab.utils.noise import GaussianNoiseCfg, NoiseModelWithAdditiveBiasCfg, UniformNoiseCfg, NoiseModelCfg
from isaaclab.utils.noise import AdditiveGaussianNoiseCfg, AdditiveUniformNoiseCfg, ConstantBiasNoiseCfg  # noqa: F401
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
from allsteps_isaaclab_amd.envs.noise import EnvNoise
from allsteps_isaaclab_amd import _native
cfg = AllstepsEnvCfg()
cfg.action_noise_model = NoiseModelWithAdditiveBiasCfg(
    noise_cfg=GaussianNoiseCfg(mean=0.0, std=0.05, operation="add"),
    bias_noise_cfg=GaussianNoiseCfg(mean=0.0, std=0.015, operation="abs"))
cfg.observation_noise_model = NoiseModelCfg(
    noise_cfg=UniformNoiseCfg(n_min=torch.full((59,), -0.25), n_max=0.5, operation="scale"))
assert EnvNoise.wanted(cfg) and not EnvNoise.wanted(AllstepsEnvCfg())
nz = EnvNoise(cfg, 8, torch.device("cpu"), 42)
a, o = nz.action.desc, nz.obs.desc
assert (a.kind, a.op, a.bias_kind, a.bias_op) == (_native.NOISE_GAUSSIAN, 0, _native.NOISE_GAUSSIAN, 2)
assert nz.action.p1.shape == (21,) and float(nz.action.p1[3]) == float(torch.tensor(0.05))
assert (o.kind, o.op, o.bias_kind) == (_native.NOISE_UNIFORM, 1, _native.NOISE_NONE)
assert torch.equal(nz.obs.p1, torch.full((59,), 0.75)) and nz.obs.bias is None
assert sorted(nz.get_state()) == ["noise_action_bias", "noise_t"]
assert nz.noisy_actions.shape == (8, 21) and nz.t.shape == (8,)
print("compat noise ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "compat noise ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_uniform_width_follows_torch_for_floats_and_tensors():
    """w = n_max - n_min is formed in double for two Python floats and in float32 with a tensor, as torch
    forms it in rand * (n_max - n_min)."""
    import numpy as np

    from allsteps_isaaclab_amd.envs.noise import NoiseModelState
    from allsteps_isaaclab_amd.utils import noise as N

    lo, hi = -0.3 - 0.011, 0.7 + 0.013
    cpu = torch.device("cpu")
    st = NoiseModelState(N.NoiseModelCfg(noise_cfg=N.UniformNoiseCfg(n_min=lo, n_max=hi)), 4, 5, cpu, "m")
    assert float(st.p1[0]) == float(np.float32(hi - lo))
    tl = torch.tensor([lo] * 5)
    st = NoiseModelState(N.NoiseModelCfg(noise_cfg=N.UniformNoiseCfg(n_min=tl, n_max=hi)), 4, 5, cpu, "m")
    assert torch.equal(st.p1, hi - tl)


def _custom(data, cfg):
    return data


@pytest.mark.parametrize("what", ["func", "class_type", "bias func", "operation", "missing term", "columns"])
def test_unsupported_models_raise_at_construction(what):
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.utils import noise as N

    class Custom(N.NoiseModel):
        pass

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = 4
    good = N.GaussianNoiseCfg(std=0.1)
    err, match = _native.NativeError, "supported"
    if what == "func":
        model = N.NoiseModelCfg(noise_cfg=N.NoiseCfg(func=_custom))
    elif what == "class_type":
        model = N.NoiseModelCfg(class_type=Custom, noise_cfg=good)
    elif what == "bias func":
        model = N.NoiseModelWithAdditiveBiasCfg(noise_cfg=good, bias_noise_cfg=N.NoiseCfg(func=_custom))
    elif what == "operation":
        model = N.NoiseModelCfg(noise_cfg=N.GaussianNoiseCfg(operation="mul"))
    elif what == "missing term":
        model, err, match = N.NoiseModelCfg(), ValueError, "noise_cfg is not set"
    else:
        model, err, match = N.NoiseModelCfg(noise_cfg=N.GaussianNoiseCfg(std=torch.ones(7))), ValueError, "broadcast"
    cfg.observation_noise_model = model
    with pytest.raises(err, match=match):
        DirectRLEnv(cfg)
    cfg.observation_noise_model = None
    assert DirectRLEnv(cfg)._noise is None


def test_abi_exports_the_noise_entry_points():
    from allsteps_isaaclab_amd import _native

    assert {"as_noise_actions", "as_noise_post"} <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    assert hasattr(L, "as_noise_actions") and hasattr(L, "as_noise_post")


def test_noise_calls_validate_their_arguments():
    """Every refusal is made before any device call: kind / op ranges, cols, null pointers."""
    import numpy as np

    from allsteps_isaaclab_amd import _native

    L = _native.load()
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data

    def model(**kw):
        m = _native.AsNoiseModel()
        m.kind, m.op, m.p0, m.p1 = _native.NOISE_UNIFORM, 0, p, p
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def actions(m, src=p, out=p + 2048, n=4, cols=21, t=p):
        return L.as_noise_actions(None if m is None else C.byref(m), src, out, n, cols, t, None, 0, 0, None)

    def post(am, om, obs=p, n=4, cols=59, t=p, reset=None, reset2=None):
        return L.as_noise_post(None if am is None else C.byref(am), None if om is None else C.byref(om), obs, n, cols,
                               t, reset, reset2, None, None, None, 0, 0, None)

    refusals = [
        (lambda: actions(None), b"null"),
        (lambda: actions(model(), src=None), b"null"),
        (lambda: actions(model(), t=None), b"null"),
        (lambda: actions(model(), out=p), b"out of place"),
        (lambda: actions(model(kind=0)), b"kind"),
        (lambda: actions(model(kind=4)), b"kind"),
        (lambda: actions(model(op=3)), b"op 3"),
        (lambda: actions(model(op=-1)), b"op -1"),
        (lambda: actions(model(p0=None)), b"null parameter"),
        (lambda: actions(model(p1=None)), b"null parameter"),
        (lambda: actions(model(bias_kind=5)), b"bias_kind"),
        (lambda: actions(model(bias_kind=2, bias_op=7)), b"bias_op"),
        (lambda: actions(model(bias_kind=2)), b"null bias"),
        (lambda: actions(model(), cols=257), b"cols 257"),
        (lambda: actions(model(), cols=0), b"cols 0"),
        (lambda: actions(model(), n=0), b"n 0"),
        (lambda: post(None, model(), t=None), b"null"),
        (lambda: post(None, model(), cols=300), b"cols 300"),
        (lambda: post(model(kind=9), None), b"action model: kind"),
        (lambda: post(None, model(op=5)), b"observation model: op"),
        (lambda: post(None, model(), reset2=p), b"reset2 without reset"),
    ]
    for call, msg in refusals:
        rc = call()
        assert rc == -1, msg
        assert msg in L.as_last_error(), (msg, L.as_last_error())
