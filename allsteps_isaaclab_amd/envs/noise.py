"""Device state of an env's noise models (``cfg.action_noise_model`` / ``cfg.observation_noise_model``).

``DirectRLEnv`` builds an :class:`EnvNoise` at construction when either field is set and launches
``as_noise_actions`` before the step and ``as_noise_post`` after it on the env's stream
(csrc/noise_kernels.h; formulas and Philox stream: csrc/allsteps_noise.h).  Everything the kernels read --
the per-env step counter ``t``, the per-env biases, the per-column parameter vectors, the noisy-action
buffer -- lives in fixed device tensors, so a step captured in a HIP graph replays with fresh noise.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..utils import noise as N
from ._manager import DeviceState, is_number

_TERMS = {N.constant_noise: (_native.NOISE_CONSTANT, ("bias", None)),
          N.uniform_noise: (_native.NOISE_UNIFORM, ("n_min", "n_max")),
          N.gaussian_noise: (_native.NOISE_GAUSSIAN, ("mean", "std"))}


def _unsupported(what: str, detail: str) -> "_native.NativeError":
    return _native.NativeError(f"{what}: {detail}.  The noise runs in HIP kernels (no host fallback); supported: "
                               f"{N.SUPPORTED}")


def _term(cfg, what: str):
    """(kind, op, p0, p1) of a NoiseCfg: the AS_NOISE_* codes and its two parameters as given."""
    func = getattr(cfg, "func", None)
    if func is N.MISSING or func not in _TERMS:
        raise _unsupported(what, f"func = {getattr(func, '__name__', func)!r} is not a built-in noise term")
    kind, names = _TERMS[func]
    op = getattr(cfg, "operation", None)
    if op not in _native.NOISE_OPS:
        raise _unsupported(what, f"operation = {op!r}")
    try:
        p0 = getattr(cfg, names[0])
        p1 = getattr(cfg, names[1]) if names[1] else 0.0
    except AttributeError as e:
        raise _unsupported(what, f"the cfg of {func.__name__} lacks field {e.name!r}") from None
    return kind, _native.NOISE_OPS[op], p0, p1


def _vector(x, cols: int, device, what: str) -> torch.Tensor:
    """A parameter (float or tensor broadcastable to a row) as a float32 device vector [cols]."""
    if is_number(x):
        return torch.full((cols,), float(np.float32(x)), dtype=torch.float32, device=device)
    if not torch.is_tensor(x):
        raise _unsupported(what, f"parameter of type {type(x).__name__} (float or tensor expected)")
    v = x.detach().to(device=device, dtype=torch.float32)
    if v.dim() > 1 and all(s == 1 for s in v.shape[:-1]):
        v = v.reshape(v.shape[-1])
    if v.dim() > 1 or v.numel() not in (1, cols):
        raise ValueError(f"{what}: parameter of shape {tuple(x.shape)} does not broadcast over a row of {cols}")
    return v.reshape(-1).expand(cols).contiguous()


def _params(kind: int, p0, p1, cols: int, device, what: str):
    """The kernels' [cols] vectors.  Uniform: (n_min, w = n_max - n_min), w formed once as torch forms it --
    in double for two Python floats (rounded to float32 where it meets the data), in float32 with a tensor."""
    if kind == _native.NOISE_UNIFORM:
        if is_number(p0) and is_number(p1):
            w = float(p1) - float(p0)
        else:
            w = _vector(p1, cols, device, what) - _vector(p0, cols, device, what)
        return _vector(p0, cols, device, what), _vector(w, cols, device, what)
    return _vector(p0, cols, device, what), _vector(p1, cols, device, what)


def _scalar(x, what: str) -> float:
    if torch.is_tensor(x) and x.numel() == 1:
        return float(x.detach().float().reshape(()).cpu())
    if not is_number(x):
        raise ValueError(f"{what}: the bias term's parameters are one value per model (the bias is (num_envs, 1)), "
                         f"got {type(x).__name__}" + (f" of shape {tuple(x.shape)}" if torch.is_tensor(x) else ""))
    return float(x)


class NoiseModelState:
    """One model on the device: the as_noise_model_t descriptor and the tensors it points at."""

    def __init__(self, model_cfg, n: int, cols: int, device, what: str):
        if cols < 1 or cols > _native.NOISE_MAX_COLS:
            raise _native.NativeError(f"{what}: rows of {cols} columns; the noise kernels take 1 .. "
                                      f"{_native.NOISE_MAX_COLS}")
        ct = getattr(model_cfg, "class_type", None)
        if ct not in (N.NoiseModel, N.NoiseModelWithAdditiveBias):
            raise _unsupported(what, f"class_type = {getattr(ct, '__name__', ct)!r} is not a built-in noise model")
        term = getattr(model_cfg, "noise_cfg", N.MISSING)
        if term is N.MISSING or term is None:
            raise ValueError(f"{what}: noise_cfg is not set")
        kind, op, p0, p1 = _term(term, f"{what}.noise_cfg")
        self.p0, self.p1 = _params(kind, p0, p1, cols, device, f"{what}.noise_cfg")
        self.cols = cols
        self.bias = None
        d = _native.AsNoiseModel()
        d.kind, d.op, d.p0, d.p1 = kind, op, self.p0.data_ptr(), self.p1.data_ptr()
        d.bias_kind = _native.NOISE_NONE
        if ct is N.NoiseModelWithAdditiveBias:
            bterm = getattr(model_cfg, "bias_noise_cfg", N.MISSING)
            if bterm is N.MISSING or bterm is None:
                raise ValueError(f"{what}: bias_noise_cfg is not set")
            bkind, bop, b0, b1 = _term(bterm, f"{what}.bias_noise_cfg")
            b0, b1 = _scalar(b0, f"{what}.bias_noise_cfg"), _scalar(b1, f"{what}.bias_noise_cfg")
            if bkind == _native.NOISE_UNIFORM:
                b1 = b1 - b0
            self.bias = torch.zeros(n, dtype=torch.float32, device=device)  # NoiseModelWithAdditiveBias.__init__
            d.bias_kind, d.bias_op, d.bias_p0, d.bias_p1, d.bias = bkind, bop, b0, b1, self.bias.data_ptr()
        self.desc = d


class EnvNoise(DeviceState):
    """The noise side of a DirectRLEnv: both models, the stream counter and the noisy-action buffer."""

    STATE_KEYS = ("noise_t", "noise_action_bias", "noise_obs_bias")

    def __init__(self, cfg, n: int, device, seed: int):
        self.n, self.device, self.seed = n, device, int(seed)
        am, om = getattr(cfg, "action_noise_model", None), getattr(cfg, "observation_noise_model", None)
        self.action = None if am is None else NoiseModelState(am, n, int(cfg.action_space), device,
                                                               "cfg.action_noise_model")
        self.obs = None if om is None else NoiseModelState(om, n, int(cfg.observation_space), device,
                                                           "cfg.observation_noise_model")
        self.t = torch.zeros(n, dtype=torch.int32, device=device)
        self.noisy_actions = (None if self.action is None
                              else torch.zeros(n, self.action.cols, dtype=torch.float32, device=device))

    @staticmethod
    def wanted(cfg) -> bool:
        return (getattr(cfg, "action_noise_model", None) is not None
                or getattr(cfg, "observation_noise_model", None) is not None)

    def _desc(self, m):
        return None if m is None else m.desc

    def apply_actions(self, action: torch.Tensor, env_offset: int, stream) -> torch.Tensor:
        """The action model of ``action`` in the env's noisy-action buffer (the caller's tensor is not written)."""
        m = self.action
        if action.shape != (self.n, m.cols):
            raise ValueError(f"actions must be ({self.n}, {m.cols}), got {tuple(action.shape)}")
        a = action if (action.dtype == torch.float32 and action.is_contiguous()) else action.float().contiguous()
        _native.noise_actions(m.desc, a, self.noisy_actions, self.t, seed=self.seed, env_offset=env_offset,
                              stream=stream)
        return self.noisy_actions

    def post(self, obs, reset, reset2, env_offset: int, stream) -> None:
        """After a step (obs noised in place, biases of reset | reset2 re-drawn) or, with obs None, after a
        reset of the envs in ``reset`` (None: all): advances the stream counter either way."""
        if obs is not None and self.obs is not None:
            if obs.shape != (self.n, self.obs.cols) or obs.dtype != torch.float32 or not obs.is_contiguous():
                raise ValueError(f"policy observations must be contiguous float32 ({self.n}, {self.obs.cols}), got "
                                 f"{obs.dtype} {tuple(obs.shape)}")
        else:
            obs = None
        _native.noise_post(self._desc(self.action), self._desc(self.obs), obs, self.t, reset, reset2,
                           seed=self.seed, env_offset=env_offset, stream=stream)

    # ---- state (get_state / set_state of the envs): keys only for what exists
    def tensors(self) -> dict:
        d = {"noise_t": self.t}
        if self.action is not None and self.action.bias is not None:
            d["noise_action_bias"] = self.action.bias
        if self.obs is not None and self.obs.bias is not None:
            d["noise_obs_bias"] = self.obs.bias
        return d
