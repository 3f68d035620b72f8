"""The cases of tests/golden/terminations.npz as this project's cfg objects, and what the host and GPU tests (and the
fixture's generator) share: the parsed terms (envs/terminations.py) with their device tables as host arrays, the
fixture's arrays, the band inside which bad_orientation is not held to the reference, and a NumPy restatement of
csrc/allsteps_terminations.h (host_step), held equal to the header bit for bit by tests/test_terminations_host.py."""

import ctypes as C
import json
import os

import numpy as np

from _commands_cases import _rotate_inverse, fma32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "terminations.npz")
SOURCES = ("root_pos", "root_quat", "q", "qd", "time_left", "command_counter", "net", "ep_len")
BUFFERS = ("term_dones", "time_outs", "terminated", "dones", "last_episode_dones", "reset_request")

# ---- the band of bad_orientation
# angle = |acos(x)|, x = -g[2], g = quat_rotate_inverse(q, (0, 0, -1)).  With u = (0, 0, -1) the rotation's third
# component is -(2 qw qw - 1) - 2 qz qz: four roundings (qw qw, the - 1, qz qz, the last sum; the doublings and the
# products with 0 and -1 are exact) of values of size at most 2 |q|^2, each within 2^-24 of its size: x is within
# DX = 8 2^-24 max(1, |q|^2) of the exact value for the float32 quaternion.  torch's kernels and
# allsteps_base_frame.h make x with the same operations, so both carry this error, the same one.
# term_acosf(x) = as_atan2f(s, x), s = sqrtf((1 - x)(1 + x)): one of 1 - x, 1 + x is exact (Sterbenz) or both are within
# 2^-24, the product and the root add one rounding each (the root halves what came before): s is within 2.5 2^-24 s
# of the exact root, and atan2 moves by x s times a relative error of s, at most half of it; as_atan2f itself is
# within 2.5 ulp of an angle of at most pi (include/as_detmath.h), 2.5 2^-22.  Together ACOS_ERR = 3 2^-22 rad.
# tests/test_terminations_host.py measures the function against float64 over a sweep of [-1, 1] and holds it under
# this figure.  torch's own float32 acos is within 2 ulp, inside the same figure.
ACOS_ERR = 3.0 * 2.0 ** -22


def orientation_dx(quat64: np.ndarray) -> np.ndarray:
    """DX above, per env, for (4, n) float64 copies of the float32 quaternions."""
    return 8.0 * 2.0 ** -24 * np.maximum(1.0, (quat64 ** 2).sum(0))


def orientation_angle64(quat: np.ndarray):
    """(x, angle) in float64 on (4, n) float32 quaternions: x = -projected_gravity_b[2], angle = |acos(x)| (NaN
    outside [-1, 1])."""
    q = quat.astype(np.float64)
    x = (2.0 * q[0] * q[0] - 1.0) + 2.0 * q[3] * q[3]
    with np.errstate(invalid="ignore"):
        return x, np.abs(np.arccos(x))


def orientation_band(quat: np.ndarray) -> np.ndarray:
    """B per env: how far the float32 angle -- the header's or torch's -- may lie from the float64 one.  The angle
    moves by at most max |acos(x +- DX) - acos(x)| (acos is monotone; x +- DX is clipped to [-1, 1]) plus ACOS_ERR.
    Past the ends the float32 x may exceed 1 in size, and the angle is then a NaN, whose flag is clear.  Above +1 that
    is the flag of the angle 0, which the clipping already covers: such an env is held like any other.  Below -1 it
    is not the flag of the angle pi: an env whose x may pass -1, or whose float64 angle is itself a NaN, is
    infinitely wide."""
    x, ang = orientation_angle64(quat)
    dx = orientation_dx(quat.astype(np.float64))
    with np.errstate(invalid="ignore"):
        lo, hi = np.arccos(np.clip(x + dx, -1.0, 1.0)), np.arccos(np.clip(x - dx, -1.0, 1.0))
        band = np.maximum(np.abs(lo - ang), np.abs(hi - ang)) + ACOS_ERR
    return np.where((x - dx < -1.0) | np.isnan(ang), np.inf, band)


def orientation_held(quat: np.ndarray, limit: float) -> np.ndarray:
    """The envs whose bad_orientation flag is held to the float64 flag (and so to the reference's): the float64 angle
    is farther from float32(limit) than B."""
    _, ang = orientation_angle64(quat)
    with np.errstate(invalid="ignore"):
        return np.abs(ang - float(np.float32(limit))) > orientation_band(quat)


# ---- the fixture
def load_fixture():
    z = np.load(FIXTURE)
    return z, json.loads(bytes(z["meta"]).decode())


def context(z, meta, case):
    from allsteps_isaaclab_amd.envs.terminations import SensorInfo, TermContext

    bodies = list(range(meta["bodies"]))
    return TermContext(joint_names=[f"joint_{k}" for k in range(meta["joints"])],
                       soft_joint_pos_limits=z["soft_joint_pos_limits"], step_dt=case["step_dt"],
                       max_episode_length=meta["max_episode_length"], command_names=["base_velocity"],
                       sensors={"contact": SensorInfo([f"body_{k}" for k in bodies], bodies)}, contact_forces=True)


def term_cfgs(terms: list, time_outs: dict | None = None) -> dict:
    """The fixture case's terms in this project's cfg classes and term functions."""
    from allsteps_isaaclab_amd.utils import terminations as TM
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    cfgs = {}
    for t in terms:
        p = dict(t["params"])
        params = {}
        if "joint_ids" in p:
            params["asset_cfg"] = SceneEntityCfg("robot", joint_ids=p.pop("joint_ids"))
        if "body_ids" in p:
            ids = p.pop("body_ids")
            params["sensor_cfg"] = SceneEntityCfg("contact") if ids is None else SceneEntityCfg("contact", body_ids=ids)
        if "bounds" in p:
            p["bounds"] = tuple(p["bounds"])
        params.update(p)
        to = t["time_out"] if time_outs is None or t["name"] not in time_outs else time_outs[t["name"]]
        cfgs[t["name"]] = TM.TerminationTermCfg(func=getattr(TM, t["func"]), params=params, time_out=to)
    return cfgs


def load_cases() -> list:
    """Per case: name, steps, sim_dt, the parsed TerminationTerms per step (the time_out edits applied), inputs
    {source: (steps, ...)} and the reference's flags (steps, terms, n), time_outs / terminated / dones (steps, n),
    last (steps, terms, n), the float64 angle of bad_orientation (steps, n) and the by-hand resets' counts."""
    from allsteps_isaaclab_amd.envs.terminations import TerminationTerms

    z, meta = load_fixture()
    cases = []
    for c in meta["cases"]:
        ctx = context(z, meta, c)
        steps, names = c["steps"], [t["name"] for t in c["terms"]]
        specs, time_outs = [], {}
        for s in range(steps):
            for e in c["edits"]:
                if e["step"] == s:
                    time_outs[e["term"]] = e["time_out"]
            specs.append(TerminationTerms(term_cfgs(c["terms"], time_outs), ctx))
        x = {k: z[f"in_{c['name']}_{k}"][:steps] for k in SOURCES}
        out = {"name": c["name"], "steps": steps, "n": meta["n"], "sim_dt": c["sim_dt"], "step_dt": c["step_dt"],
               "terms": c["terms"], "names": names, "specs": specs, "inputs": x, "resets": c["resets"],
               "band_words": c["band_words"]}
        out.update({k: z[f"{c['name']}_{k}"] for k in ("flags", "time_outs", "terminated", "dones", "last",
                                                       "angle64")})
        cases.append(out)
    return cases


def step_inputs(case: dict, s: int) -> dict:
    return {k: v[s] for k, v in case["inputs"].items()}


# ---- the NumPy restatement of the header
def oracle_atan2(orc):
    """as_atan2f of include/as_detmath.h through the oracle library."""
    fp = C.POINTER(C.c_float)

    def atan2(y, x):
        y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
        out = np.empty_like(y)
        orc.L.or_detmath_eval(C.c_int(0), C.c_int(y.size), y.ctypes.data_as(fp), x.ctypes.data_as(fp),
                              out.ctypes.data_as(fp))
        return out

    return atan2


def acosf(x, atan2):
    """term_acosf of the header."""
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) <= f(1)
        xs = np.where(ok, x, f(0)).astype(f)
        out = atan2(np.sqrt((f(1) - xs) * (f(1) + xs)), xs)
    return np.where(ok, out, f(np.nan)).astype(f)


def orientation_angle(quat, atan2):
    """term_orientation_angle of the header on (4, n) rows."""
    n = quat.shape[1]
    f = np.float32
    o = _rotate_inverse([quat[k] for k in range(4)], [np.zeros(n, f), np.zeros(n, f), np.full(n, -1, f)])
    return np.abs(acosf(-o[2], atan2))


def _contact_max(net, b, sdt):
    m = None
    for d in range(net.shape[0]):
        x, y, z = (net[d, b, c] / sdt for c in range(3))
        w = np.sqrt(fma32(z, z, fma32(y, y, x * x)))
        m = w if m is None else np.where(~np.isnan(m) & ((w > m) | np.isnan(w)), w, m)
    return m


def term_flags(spec, x: dict, sim_dt: float, atan2, step_truncated=None) -> np.ndarray:
    """f of every term of a parsed TerminationTerms on one step's rows: (terms, n) uint8."""
    from allsteps_isaaclab_amd import _native

    f = np.float32
    sdt = f(sim_dt)
    n = x["root_quat"].shape[-1]
    out = np.zeros((len(spec.terms), n), np.uint8)
    with np.errstate(all="ignore"):
        for k, t in enumerate(spec.terms):
            kind = _native.TERMINATION_KINDS[t.kind]
            ids = list(t.ids)
            v = np.zeros(n, bool)
            if kind == "time_out":
                v = x["ep_len"] >= t.i0
                if step_truncated is not None:
                    v = v | (step_truncated != 0)
            elif kind == "command_resample":
                v = (x["time_left"][t.row] <= t.p0) & (x["command_counter"][t.row] == t.i0)
            elif kind == "bad_orientation":
                v = orientation_angle(x["root_quat"], atan2) > t.p0
            elif kind == "root_height_below_minimum":
                v = x["root_pos"][2] < t.p0
            elif kind == "joint_pos_out_of_limit":
                for i, j in enumerate(ids):
                    v = v | (x["q"][j] > t.b[i]) | (x["q"][j] < t.a[i])
            elif kind == "joint_pos_out_of_manual_limit":
                for j in ids:
                    v = v | (x["q"][j] > t.p1) | (x["q"][j] < t.p0)
            elif kind == "joint_vel_out_of_manual_limit":
                for j in ids:
                    v = v | (np.abs(x["qd"][j]) > t.p0)
            else:  # illegal_contact
                for b in ids:
                    v = v | (_contact_max(x["net"], b, sdt) > t.p0)
            out[k] = v
    return out


def host_step(spec, x: dict, state: dict, sim_dt: float, atan2, step_terminated=None, step_truncated=None):
    """One launch of k_terminations_step in numpy.  state: the BUFFERS, not modified.  Returns the new state."""
    flags = term_flags(spec, x, sim_dt, atan2, step_truncated)
    n = flags.shape[1]
    to = np.zeros(n, bool)
    te = np.zeros(n, bool)
    for k, t in enumerate(spec.terms):
        if t.time_out:
            to |= flags[k] != 0
        else:
            te |= flags[k] != 0
    stepped = np.zeros(n, bool)
    for m in (step_terminated, step_truncated):
        if m is not None:
            stepped |= m != 0
    u8 = lambda a: a.astype(np.uint8)  # noqa: E731
    return {"term_dones": flags, "time_outs": u8(to), "terminated": u8(te), "dones": u8(to | te),
            "last_episode_dones": np.where((to | te | stepped)[None], flags, state["last_episode_dones"]),
            "reset_request": u8((to | te) & ~stepped)}


def zero_state(terms: int, n: int) -> dict:
    z = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    return {"term_dones": z(terms, n), "time_outs": z(n), "terminated": z(n), "dones": z(n),
            "last_episode_dones": z(terms, n), "reset_request": z(n)}
