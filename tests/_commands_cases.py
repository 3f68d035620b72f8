"""The cases of tests/golden/commands.npz (gen_commands.py: the reference's CommandManager.reset / compute with its
velocity terms on recorded draws) as the command kernels take them -- shared by the host and GPU command tests --
and a float32 numpy restatement of one env step from given draws."""

from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 66
DRAWS = 11
STATE = ("vel", "heading_target", "flags", "time_left", "counter", "metrics")

# The heading tolerance (rad/s per unit of |heading_control_stiffness|): 2 x the largest difference between the
# host header (as_atan2f) and the reference fixture (torch.atan2) in the heading envs' yaw command and in
# error_vel_yaw, as tests/commands_check.cpp measures it on the fixture (test_commands_host.py asserts that the
# measurement stays at or below MEASURED_HEADING_DIFF, and MEASURED_HEADING_DIFF below the derived bound
# 8 * 2**-22: as_atan2f <= 2.5 ulp and a libm atan2f <= 1 ulp, both at ulp(pi) = 2**-22, plus the roundings of the
# subtraction and the wrap).
MEASURED_HEADING_DIFF = 4.0 * 2.0 ** -22  # rad, per unit stiffness (9.53674316e-07): two steps of ulp(2 pi)
MEASURED_ERR_YAW_DIFF = 2.0 ** -22  # error_vel_yaw's largest difference when the yaw commands are carried along
HEADING_TOL = 2.0 * MEASURED_HEADING_DIFF
ERR_YAW_TOL = 2.0 * MEASURED_ERR_YAW_DIFF
HEADING_BOUND = 8.0 * 2.0 ** -22


def term_cfg(term: dict):
    """A fixture term as a user writes it: utils.commands cfg objects with Python floats."""
    from allsteps_isaaclab_amd.utils import commands as CM

    r = {k: (tuple(v) if v is not None else None) for k, v in term["ranges"].items()}
    if term["kind"] == "normal":
        return CM.NormalVelocityCommandCfg(asset_name="robot", resampling_time_range=tuple(term["resampling_time_range"]),
                                           rel_standing_envs=term.get("rel_standing_envs", 0.0),
                                           ranges=CM.NormalVelocityCommandCfg.Ranges(**r))
    return CM.UniformVelocityCommandCfg(
        asset_name="robot", resampling_time_range=tuple(term["resampling_time_range"]),
        heading_command=term.get("heading_command", False),
        heading_control_stiffness=term.get("heading_control_stiffness", 1.0),
        rel_standing_envs=term.get("rel_standing_envs", 0.0), rel_heading_envs=term.get("rel_heading_envs", 1.0),
        ranges=CM.UniformVelocityCommandCfg.Ranges(**r))


def _spread(a: np.ndarray, slots: list[int], axis: int) -> np.ndarray:
    """The fixture's used draw slots spread to the kernel's DRAWS rows (the others zero)."""
    shape = list(a.shape)
    shape[axis] = DRAWS
    out = np.zeros(shape, np.float32)
    idx = [slice(None)] * a.ndim
    idx[axis] = slots
    out[tuple(idx)] = a
    return out


def load_cases() -> list[dict]:
    """Every fixture case: its descriptor rows (terms, 21) built by the env's own host code (envs/commands.py), dt
    as float32, the initial state ``<key>0`` and per step the inputs root_quat (4, n), root_lin / root_ang (3, n),
    reset (n,), draws (2, terms, 11, n) (phase 0 zero in a step without a reset) and the reference's state after
    the step, every array in the kernel's layout; ``resampled`` (steps, 2, terms, n); init_draws (terms, 11, n)."""
    from allsteps_isaaclab_amd.envs.commands import CommandTerms

    z = np.load(os.path.join(GOLDEN, "commands.npz"), allow_pickle=False)
    out = []
    for case in json.loads(str(z["cases"])):
        name, steps, slots = case["name"], case["steps"], case["slots"]
        terms = CommandTerms({t["name"]: term_cfg(t) for t in case["terms"]}, case["dt"])
        K = len(case["terms"])
        draws = np.zeros((steps, 2, K, DRAWS, N), np.float32)
        draws[:, 1] = _spread(z[f"{name}_draws"], slots, 2)
        draws[z[f"{name}_reset_steps"], 0] = _spread(z[f"{name}_reset_draws"], slots, 2)
        c = {"name": name, "rows": terms.rows, "terms": case["terms"], "dt": np.float32(case["dt"]), "steps": steps,
             "draws": draws, "init_draws": _spread(z[f"{name}_init_draws"], slots, 1),
             "root_quat": z[f"{name}_root_quat"], "root_lin": z[f"{name}_root_lin"], "root_ang": z[f"{name}_root_ang"],
             "reset": z[f"{name}_reset"], "resampled": z[f"{name}_resampled"],
             "last_metrics": z[f"{name}_last_metrics"]}
        for key in STATE:
            c[key] = z[f"{name}_{key}"]
            c[key + "0"] = z[f"{name}_{key}0"]
        out.append(c)
    return out


def heading_rows(c: dict) -> np.ndarray:
    """(terms,) bool: the terms of a case whose yaw command can come from atan2."""
    return np.array([t["kind"] != "normal" and bool(t.get("heading_command")) for t in c["terms"]])


def fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) elementwise on float32 values: the product is exact in double; where the double sum lands on
    the midpoint of two float32 values its own rounding may have put it there, and the element is redone in
    rationals."""
    from fractions import Fraction

    a, b, c = (np.array(x, np.float32) for x in np.broadcast_arrays(np.asarray(a, np.float32),
                                                                     np.asarray(b, np.float32),
                                                                     np.asarray(c, np.float32)))
    r64 = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = r64.astype(np.float32)
    tie = (r64.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    for i in zip(*np.nonzero(tie)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((np.nextafter(out[i], np.float32(-np.inf)), np.nextafter(out[i], np.float32(np.inf))))
        out[i] = min((lo, out[i], hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
    return out


def _cross(a, b):
    return [fma32(a[1], b[2], -(a[2] * b[1])), fma32(a[2], b[0], -(a[0] * b[2])), fma32(a[0], b[1], -(a[1] * b[0]))]


def _rotate_inverse(q, u):
    f = np.float32
    qw, xyz = q[0], [q[1], q[2], q[3]]
    s = f(2) * (qw * qw) - f(1)
    x = _cross(xyz, u)
    dot = (xyz[0] * u[0] + xyz[1] * u[1]) + xyz[2] * u[2]
    return [(u[k] * s - (x[k] * qw) * f(2)) + (xyz[k] * dot) * f(2) for k in range(3)]


def _forward(q):
    f = np.float32
    n = q.shape[1]
    xyz = [q[1], q[2], q[3]]
    v = [np.ones(n, f), np.zeros(n, f), np.zeros(n, f)]
    t = [c * f(2) for c in _cross(xyz, v)]
    x = _cross(xyz, t)
    return [(v[k] + q[0] * t[k]) + x[k] for k in range(3)]


def _wrap_to_pi(a):
    f = np.float32
    pi, two_pi = f(np.pi), f(2) * f(np.pi)
    m = np.fmod(a + pi, two_pi)
    m = np.where((m != 0) & (m < 0), m + two_pi, m)
    return np.where((m == 0) & (a > 0), pi, m - pi).astype(f)


def row_fields(row: np.ndarray) -> dict:
    """An as_command_term_t row (21 words) by field."""
    ints = row[:2].view(np.int32)
    return {"kind": int(ints[0]), "heading": int(ints[1]), "time_lo": row[2], "time_w": row[3], "lo": row[4:8],
            "w": row[8:12], "clip_lo": row[12], "clip_hi": row[13], "stiffness": row[14], "p_heading": row[15],
            "p_standing": row[16], "p_zero": row[17:20], "max_command_step": row[20]}


def host_step(rows, dt, state, atan2, root=None, reset=None, draws=None, compute=True):
    """One launch of k_commands_step (compute) or k_commands_reset in float32 numpy, each operation rounded on its
    own but for the fused sample (csrc/allsteps_commands.h).  state: dict of STATE arrays + last_metrics, in the
    kernel's layouts, not modified; root = (root_quat (4, n), root_lin (3, n), root_ang (3, n)); reset (n,) bool;
    draws (phases, terms, 11, n); atan2(y, x) -> float32 array, the header's as_atan2f.  Returns the new state and
    resampled (2, terms, n)."""
    f = np.float32
    st = {k: np.array(v) for k, v in state.items()}
    K, n = st["time_left"].shape
    reset = np.zeros(n, bool) if reset is None else np.asarray(reset).astype(bool)
    resampled = np.zeros((2, K, n), bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            c = row_fields(rows[k])
            vel, flags = st["vel"][k], st["flags"][k]

            def resample(m, d):
                st["time_left"][k] = np.where(m, fma32(d[0], c["time_w"], c["time_lo"]), st["time_left"][k])
                st["counter"][k] += m.astype(np.int32)
                if c["kind"] == 1:
                    for a in range(3):
                        v = fma32(d[1 + a], c["w"][a], c["lo"][a]) * np.where(d[4 + a] <= f(0.5), f(1), f(-1))
                        vel[a] = np.where(m, v, vel[a])
                        flags[2 + a] = np.where(m, d[7 + a] <= c["p_zero"][a], flags[2 + a])
                    flags[1] = np.where(m, d[10] <= c["p_standing"], flags[1])
                else:
                    for a in range(3):
                        vel[a] = np.where(m, fma32(d[1 + a], c["w"][a], c["lo"][a]), vel[a])
                    if c["heading"]:
                        st["heading_target"][k] = np.where(m, fma32(d[4], c["w"][3], c["lo"][3]),
                                                           st["heading_target"][k])
                        flags[0] = np.where(m, d[5] <= c["p_heading"], flags[0])
                    flags[1] = np.where(m, d[6] <= c["p_standing"], flags[1])

            if reset.any():
                st["last_metrics"][k][:, reset] = st["metrics"][k][:, reset]
                st["metrics"][k][:, reset] = 0
                st["counter"][k][reset] = 0
                resample(reset, draws[0, k].astype(f))
                resampled[0, k] = reset
            if not compute:
                continue
            q, lin, ang = (np.asarray(x, f) for x in root)
            lin_b, ang_b = _rotate_inverse(q, lin), _rotate_inverse(q, ang)
            dx, dy = vel[0] - lin_b[0], vel[1] - lin_b[1]
            st["metrics"][k][0] = st["metrics"][k][0] + np.sqrt(fma32(dy, dy, dx * dx)) / c["max_command_step"]
            st["metrics"][k][1] = st["metrics"][k][1] + np.abs(vel[2] - ang_b[2]) / c["max_command_step"]
            st["time_left"][k] = st["time_left"][k] - f(dt)
            m = st["time_left"][k] <= 0
            if m.any():
                resample(m, draws[-1, k].astype(f))
                resampled[1, k] = m
            if c["kind"] == 0 and c["heading"]:
                fwd = _forward(q)
                e = _wrap_to_pi(st["heading_target"][k] - atan2(fwd[1], fwd[0]))
                w = np.minimum(np.maximum(c["stiffness"] * e, c["clip_lo"]), c["clip_hi"])
                vel[2] = np.where(flags[0] != 0, w, vel[2])
            vel[:, flags[1] != 0] = 0
            if c["kind"] == 1:
                for a in range(3):
                    vel[a] = np.where(flags[2 + a] != 0, f(0), vel[a])
    return st, resampled


def oracle_atan2(orc):
    """as_atan2f of include/as_detmath.h through the oracle library."""
    import ctypes as C

    def atan2(y, x):
        y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
        out = np.empty_like(y)
        fp = C.POINTER(C.c_float)
        orc.L.or_detmath_eval(C.c_int(0), C.c_int(len(y)), y.ctypes.data_as(fp), x.ctypes.data_as(fp),
                              out.ctypes.data_as(fp))
        return out

    return atan2
