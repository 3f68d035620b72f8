"""Noise model configuration -- the cfg classes of ``isaaclab/utils/noise/noise_cfg.py``, same names, fields
and defaults, for ``cfg.action_noise_model`` / ``cfg.observation_noise_model`` of the envs.

The noise itself runs on the device (``k_noise_actions`` / ``k_noise_post``, csrc/noise_kernels.h): ``func``
and ``class_type`` name which of the built-in terms and models a cfg asks for, and the env raises at
construction for anything else.  The functions and classes below are those names; there is no host
implementation behind them.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable


class _Missing:
    """The reference's ``dataclasses.MISSING`` default of a configclass field: must be set by the user."""

    def __repr__(self) -> str:
        return "MISSING"


MISSING = _Missing()


def _device_only(name: str):
    def fn(data, cfg):
        raise NotImplementedError(
            f"{name} names a noise term of the device kernels (cfg.action_noise_model / "
            f"cfg.observation_noise_model of an env); it has no host implementation")

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"noise_model.py ``{name}``: the term the HIP noise kernels apply for this cfg."
    return fn


constant_noise = _device_only("constant_noise")
uniform_noise = _device_only("uniform_noise")
gaussian_noise = _device_only("gaussian_noise")


class NoiseModel:
    """noise_model.py ``NoiseModel``: the term alone (names the model; the env builds the device state)."""


class NoiseModelWithAdditiveBias(NoiseModel):
    """noise_model.py ``NoiseModelWithAdditiveBias``: the term plus a per-env bias re-drawn on reset."""


@dataclass
class NoiseCfg:
    func: Callable = MISSING
    operation: str = "add"  # "add" | "scale" | "abs"


@dataclass
class ConstantNoiseCfg(NoiseCfg):
    func: Callable = constant_noise
    bias: Any = 0.0  # float or tensor


@dataclass
class UniformNoiseCfg(NoiseCfg):
    func: Callable = uniform_noise
    n_min: Any = -1.0
    n_max: Any = 1.0


@dataclass
class GaussianNoiseCfg(NoiseCfg):
    func: Callable = gaussian_noise
    mean: Any = 0.0
    std: Any = 1.0


@dataclass
class NoiseModelCfg:
    class_type: type = NoiseModel
    noise_cfg: NoiseCfg = MISSING


@dataclass
class NoiseModelWithAdditiveBiasCfg(NoiseModelCfg):
    class_type: type = NoiseModelWithAdditiveBias
    bias_noise_cfg: NoiseCfg = MISSING


# backward-compatible names of the reference (isaaclab/utils/noise/__init__.py)
ConstantBiasNoiseCfg = ConstantNoiseCfg
AdditiveUniformNoiseCfg = UniformNoiseCfg
AdditiveGaussianNoiseCfg = GaussianNoiseCfg

SUPPORTED = ("ConstantNoiseCfg / UniformNoiseCfg / GaussianNoiseCfg terms (func = constant_noise / uniform_noise / "
             "gaussian_noise, operation 'add' / 'scale' / 'abs') in a NoiseModelCfg or a "
             "NoiseModelWithAdditiveBiasCfg (class_type = NoiseModel / NoiseModelWithAdditiveBias)")
