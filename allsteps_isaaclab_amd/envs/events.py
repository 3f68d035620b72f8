"""Device state of an env's interval events (``cfg.events``) and the ``env.event_manager`` view of it.

``DirectRLEnv`` builds an :class:`EnvEvents` at construction when ``cfg.events`` is set and launches
``as_events_interval`` after the step on the env's stream (csrc/event_kernels.h; semantics and Philox stream:
csrc/allsteps_events.h).  Everything the kernel reads -- the per-(term, env) timers ``time_left``, the per-env
stream counter ``t``, the term descriptors -- lives in fixed device tensors, so a step captured in a HIP graph
replays with fresh pushes, and ``set_term_cfg`` takes effect in a graph that is already captured.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _native
from ..utils import events as E
from ._manager import DeviceState, RowTerms, is_number


def _unsupported(term: str, detail: str) -> "_native.NativeError":
    return _native.NativeError(f"cfg.events term {term!r}: {detail}.  The events run in a HIP kernel (no host "
                               f"fallback); supported: {E.SUPPORTED}")


def _pair(x, term: str, what: str) -> tuple[float, float]:
    try:
        lo, hi = x
    except (TypeError, ValueError):
        raise _unsupported(term, f"{what} = {x!r} is not a (lo, hi) pair") from None
    if not (is_number(lo) and is_number(hi)):
        raise _unsupported(term, f"{what} = {x!r} is not a pair of numbers")
    return float(lo), float(hi)


def term_row(name: str, cfg) -> np.ndarray:
    """The as_event_term_t of a term as 14 float32 (interval_lo, interval_w, vel_lo[6], vel_w[6]); raises
    NativeError, naming the term and the reason, for a term the kernel does not serve.

    The two widths are formed as the reference forms them: the interval's from two Python floats -- in double,
    rounded to float32 where it meets the draw (event_manager.py:221) -- the velocity's through a float32 tensor
    (events.py:703-704), a float32 subtraction."""
    mode = getattr(cfg, "mode", E.MISSING)
    if mode == "startup":
        raise _unsupported(name, "mode = 'startup' randomises physical parameters per env, which needs per-env model "
                                 "tables where the step kernel reads one constants block")
    if mode == "reset":
        raise _unsupported(name, "mode = 'reset': the task's own reset overwrites root pose, root velocity and joints "
                                 "after the reset events have run (allsteps_env.py:563-565), and parameter "
                                 "randomisation needs per-env model tables")
    if mode != "interval":
        raise _unsupported(name, f"mode = {mode!r}")
    func = getattr(cfg, "func", E.MISSING)
    fname = getattr(func, "__name__", repr(func))
    if fname == "apply_external_force_torque":
        raise _unsupported(name, "func = apply_external_force_torque acts inside the physics substeps of the fused "
                                 "step kernel, not between steps")
    if func is not E.push_by_setting_velocity:
        raise _unsupported(name, f"func = {fname} is not a served event function")
    if getattr(cfg, "is_global_time", False):
        raise _unsupported(name, "is_global_time = True: the reference calls the term with env_ids = None, which is "
                                 "not a usable path for push_by_setting_velocity")
    rng = getattr(cfg, "interval_range_s", None)
    if rng is None:
        raise _unsupported(name, "mode = 'interval' but interval_range_s is not specified")
    lo, hi = _pair(rng, name, "interval_range_s")
    if hi < lo:
        raise _unsupported(name, f"interval_range_s = {rng!r} has hi < lo")
    params = dict(getattr(cfg, "params", None) or {})
    if "velocity_range" not in params:
        raise _unsupported(name, "params lack 'velocity_range'")
    extra = sorted(set(params) - {"velocity_range", "asset_cfg"})
    if extra:
        raise _unsupported(name, f"params {extra} are not arguments of push_by_setting_velocity")
    asset = params.get("asset_cfg", E.SceneEntityCfg("robot"))
    if getattr(asset, "name", None) != "robot" or not (hasattr(asset, "whole") and asset.whole()):
        raise _unsupported(name, f"asset_cfg = {asset!r} is not the whole 'robot' (the push sets the root velocity of "
                                 f"the env's articulation)")
    vr = params["velocity_range"]
    if not isinstance(vr, dict):
        raise _unsupported(name, f"velocity_range of type {type(vr).__name__} (dict expected)")
    row = np.zeros(_native.EVENT_TERM_FLOATS, np.float32)
    row[0] = np.float32(lo)
    row[1] = np.float32(hi - lo)
    for k, key in enumerate(E.VELOCITY_KEYS):
        vlo, vhi = _pair(vr.get(key, (0.0, 0.0)), name, f"velocity_range[{key!r}]")
        row[2 + k] = np.float32(vlo)
        row[8 + k] = np.float32(vhi) - np.float32(vlo)
    if not np.isfinite(row).all():
        raise _unsupported(name, "a range is not finite in float32")
    return row


class EventTerms(RowTerms):
    """The host side of cfg.events: names, cfgs and descriptor rows, checked (no device needed).  None entries are
    skipped (event_manager.py:337-338)."""

    NOUN, TERM_TYPE, WORDS = "event", E.EventTermCfg, _native.EVENT_TERM_FLOATS
    LIMIT = ("AS_MAX_EVENT_TERMS", _native.MAX_EVENT_TERMS)

    def row(self, name: str, cfg) -> np.ndarray:
        return term_row(name, cfg)


class EnvEvents(DeviceState):
    """The events side of a DirectRLEnv: term descriptors, timers, stream counter and the fired mask."""

    STATE_KEYS = ("event_t", "event_time_left")

    def __init__(self, cfg, n: int, device, seed: int, step_dt: float):
        self.n, self.device, self.seed = n, device, int(seed)
        self.dt = float(np.float32(step_dt))
        self.terms = EventTerms(cfg.events)
        k = len(self.terms.names)
        self.started = k == 0  # without terms there is nothing to launch
        self.desc = torch.as_tensor(self.terms.rows.copy(), device=device)
        self.time_left = torch.zeros(k, n, dtype=torch.float32, device=device)
        self.t = torch.zeros(n, dtype=torch.int32, device=device)
        self.fired = torch.zeros(k, n, dtype=torch.uint8, device=device)

    @staticmethod
    def wanted(cfg) -> bool:
        return getattr(cfg, "events", None) is not None

    def start(self, env_offset: int, stream) -> None:
        """The initial timers, one draw per (term, env) (event_manager.py:383-385); once, before the first step."""
        if not self.started:
            _native.events_init(self.desc, self.time_left, self.t, seed=self.seed, env_offset=env_offset,
                                stream=stream)
            self.started = True

    def apply(self, root_lin: torch.Tensor, root_ang: torch.Tensor, env_offset: int, stream) -> None:
        """EventManager.apply(mode="interval", dt=step_dt) on the root velocity rows (3, n) of the state."""
        if not len(self.terms.names):
            return
        self.start(env_offset, stream)
        _native.events_interval(self.desc, root_lin, root_ang, self.time_left, self.t, self.dt, fired=self.fired,
                                seed=self.seed, env_offset=env_offset, stream=stream)

    def set_term_cfg(self, term_name: str, cfg) -> None:
        k = self.terms.set(term_name, cfg)
        self.desc[k].copy_(torch.as_tensor(self.terms.rows[k].copy()))

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {"event_t": self.t, "event_time_left": self.time_left}

    def set_state(self, state: dict) -> bool:
        loaded = super().set_state(state)
        self.started = self.started or loaded  # (loaded timers are not drawn again)
        return loaded


class EventManagerView:
    """``env.event_manager``: the caller-visible surface of the reference's ``EventManager``
    (event_manager.py:73-118, 275-315) over the device state."""

    def __init__(self, events: EnvEvents):
        self._ev = events

    @property
    def active_terms(self) -> dict[str, list[str]]:
        return {"interval": list(self._ev.terms.names)} if self._ev.terms.names else {}

    @property
    def available_modes(self) -> list[str]:
        return list(self.active_terms.keys())

    def get_term_cfg(self, term_name: str):
        return self._ev.terms.cfgs[self._ev.terms.index(term_name)]

    def set_term_cfg(self, term_name: str, cfg) -> None:
        """Replace a term's cfg.  The new ranges are written into the device descriptors, so they hold from the
        next step on, in a captured graph too; the running timers are kept, as the reference keeps them."""
        self._ev.set_term_cfg(term_name, cfg)

    @property
    def last_triggered(self) -> torch.Tensor:
        """(terms, num_envs) bool view of the device mask: which terms fired in which envs in the last step."""
        return self._ev.fired.view(torch.bool)

    def __str__(self) -> str:
        names = self._ev.terms.names
        msg = f"<EventManager> contains {1 if names else 0} active terms.\n"
        if names:
            rows = [(str(i), k, str(c.interval_range_s)) for i, (k, c) in enumerate(zip(names, self._ev.terms.cfgs))]
            head = ("Index", "Name", "Interval time range (s)")
            w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
            line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
            fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), r[2].center(w[2]))) + " |\n"  # noqa: E731
            msg += "Active Event Terms in Mode: 'interval'\n" + line + fmt(head) + line
            msg += "".join(fmt(r) for r in rows) + line
        return msg
