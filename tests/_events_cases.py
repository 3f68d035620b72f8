"""The cases of tests/golden/events.npz (gen_events.py: the reference's EventManager.apply and
push_by_setting_velocity on recorded draws) as the event kernel takes them -- shared by the host and GPU event
tests -- and a float32 numpy restatement of one env step from given uniforms."""

from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 66


def term_cfg(term: dict):
    """A fixture term as a user writes it: utils.events cfg objects with Python floats."""
    from allsteps_isaaclab_amd.utils import events as E

    return E.EventTermCfg(func=E.push_by_setting_velocity, mode="interval",
                          interval_range_s=tuple(term["interval_range_s"]),
                          params={"velocity_range": {k: tuple(v) for k, v in term["velocity_range"].items()},
                                  "asset_cfg": E.SceneEntityCfg("robot")})


def load_cases() -> list[dict]:
    """Every fixture case: its descriptor rows (terms, 14) built by the env's own host code (envs/events.py: the
    two widths), dt as float32, and its arrays in the kernel's field-major layouts: vel0 (6, n), time_left0
    (terms, n), and per step iv_draws (terms, n), push_draws (terms, 6, n), time_left (terms, n), fired
    (terms, n), vel (6, n).  Case a also has init_draws (terms, n)."""
    from allsteps_isaaclab_amd.envs.events import EventTerms

    z = np.load(os.path.join(GOLDEN, "events.npz"), allow_pickle=False)
    out = []
    for case in json.loads(str(z["cases"])):
        name = case["name"]
        terms = EventTerms({t["name"]: term_cfg(t) for t in case["terms"]})
        c = {"name": name, "rows": terms.rows, "dt": np.float32(case["dt"]), "steps": case["steps"],
             "vel0": np.ascontiguousarray(z[f"{name}_vel0"].T), "time_left0": z[f"{name}_time_left0"],
             "iv_draws": z[f"{name}_iv_draws"],
             "push_draws": np.ascontiguousarray(z[f"{name}_push_draws"].transpose(0, 1, 3, 2)),
             "time_left": z[f"{name}_time_left"], "fired": z[f"{name}_fired"],
             "vel": np.ascontiguousarray(z[f"{name}_vel"].transpose(0, 2, 1))}
        if f"{name}_init_draws" in z.files:
            c["init_draws"] = z[f"{name}_init_draws"]
        out.append(c)
    return out


def host_step(rows, dt, time_left, vel, iv_u, push_u):
    """One env step of every term in float32 numpy, each operation rounded on its own (csrc/allsteps_events.h):
    rows (terms, 14), time_left (terms, n), vel (6, n), iv_u (terms, n), push_u (terms, 6, n).  Returns new
    (time_left, vel, fired (terms, n) uint8)."""
    f = np.float32
    time_left, vel = time_left.astype(f).copy(), vel.astype(f).copy()
    fired = np.zeros(time_left.shape, np.uint8)
    for k in range(rows.shape[0]):
        tl = time_left[k] - f(dt)
        fire = tl < f(1e-6)
        lo, w, vlo, vw = rows[k, 0], rows[k, 1], rows[k, 2:8], rows[k, 8:14]
        time_left[k] = np.where(fire, iv_u[k].astype(f) * w + lo, tl)
        for a in range(6):
            vel[a] = np.where(fire, vel[a] + (push_u[k, a].astype(f) * vw[a] + vlo[a]), vel[a])
        fired[k] = fire
    return time_left, vel, fired
