"""Shim of ``isaaclab.utils.noise``: the noise cfg classes, served by the device noise kernels."""

from allsteps_isaaclab_amd.utils.noise import (  # noqa: F401
    AdditiveGaussianNoiseCfg,
    AdditiveUniformNoiseCfg,
    ConstantBiasNoiseCfg,
    ConstantNoiseCfg,
    GaussianNoiseCfg,
    NoiseCfg,
    NoiseModel,
    NoiseModelCfg,
    NoiseModelWithAdditiveBias,
    NoiseModelWithAdditiveBiasCfg,
    UniformNoiseCfg,
    constant_noise,
    gaussian_noise,
    uniform_noise,
)
