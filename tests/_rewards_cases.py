"""The cases of tests/golden/rewards.npz as this project's cfg objects, and what the host and GPU tests share: the
parsed terms (envs/rewards.py) with their device tables as host arrays, the fixture's arrays, and a NumPy restatement
of csrc/allsteps_rewards.h (host_step), held equal to the header bit for bit by tests/test_rewards_host.py."""

import ctypes as C
import json
import os

import numpy as np

from _commands_cases import _rotate_inverse, fma32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "rewards.npz")
SOURCES = ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "qd_prev", "commands", "net", "timers",
           "actions", "terminated")
EXP_FUNCS = ("track_lin_vel_xy_exp", "track_ang_vel_z_exp", "track_ang_vel_z_world_exp")
YAW_FUNC = "track_lin_vel_xy_yaw_frame_exp"  # an exp term whose argument goes through the library's atan2 / sincos
# the kinds that reduce over more than two rounded addends: the case-b rule applies to them
REDUCTIONS = ("joint_vel_l1", "joint_vel_l2", "joint_deviation_l1", "joint_pos_limits", "joint_acc_l2", "action_l2",
              "action_rate_l2", "contact_forces", "feet_air_time")


def load_fixture():
    z = np.load(FIXTURE)
    return z, json.loads(bytes(z["meta"]).decode())


def context(z, meta, case):
    from allsteps_isaaclab_amd.envs.rewards import RewContext, SensorInfo

    feet = list(range(meta["feet"]))
    return RewContext(joint_names=[f"joint_{k}" for k in range(meta["joints"])],
                      default_joint_pos=z["default_joint_pos"], soft_joint_pos_limits=z["soft_joint_pos_limits"],
                      action_cols=meta["actions"], step_dt=case["step_dt"], command_names=["base_velocity"],
                      sensors={"contact": SensorInfo([f"foot_{k}" for k in feet], feet, feet)},
                      contact_forces=True, contact_air_time=True)


def term_cfgs(terms: list, weights: dict | None = None) -> dict:
    """The fixture case's terms in this project's cfg classes and term functions."""
    from allsteps_isaaclab_amd.utils import rewards as RW
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    cfgs = {}
    for t in terms:
        p = dict(t["params"])
        params = {}
        if "joint_ids" in p:
            params["asset_cfg"] = SceneEntityCfg("robot", joint_ids=p.pop("joint_ids"))
        if "body_ids" in p:
            params["sensor_cfg"] = SceneEntityCfg("contact", body_ids=p.pop("body_ids"))
        params.update(p)
        w = t["weight"] if weights is None or t["name"] not in weights else weights[t["name"]]
        cfgs[t["name"]] = RW.RewardTermCfg(func=getattr(RW, t["func"]), params=params, weight=w)
    return cfgs


def load_cases() -> list:
    """Per case: name, steps, dt / sim_dt, the parsed RewardTerms per step (the weight edits applied), inputs {source:
    (steps, ...)}, reset (steps, n) uint8 and the reference's f / f64 / reward / sums / step / last; case a0 takes
    its term arrays from case a."""
    from allsteps_isaaclab_amd.envs.rewards import RewardTerms

    z, meta = load_fixture()
    cases = []
    for c in meta["cases"]:
        ctx = context(z, meta, c)
        steps, names = c["steps"], [t["name"] for t in c["terms"]]
        specs, weights = [], {}
        for s in range(steps):
            for e in c["edits"]:
                if e["step"] == s:
                    weights[e["term"]] = e["weight"]
            specs.append(RewardTerms(term_cfgs(c["terms"], weights), ctx))
        x = {k: z[f"in_{c['inputs']}_{k}"][:steps] for k in SOURCES}
        out = {"name": c["name"], "steps": steps, "n": meta["n"], "dt": c["dt"], "sim_dt": c["sim_dt"],
               "terms": c["terms"], "names": names, "specs": specs, "inputs": x,
               "reset": z[f"in_{c['inputs']}_reset"][:steps], "reward": z[f"{c['name']}_reward"]}
        if c["name"] == "a0":
            a = next(k for k in cases if k["name"] == "a")
            idx = [a["names"].index(k) for k in names]
            out.update({k: a[k][:, idx] for k in ("f", "f64", "sums", "step", "last")})
        else:
            out.update({k: z[f"{c['name']}_{k}"] for k in ("f", "f64", "sums", "step", "last")})
        cases.append(out)
    return cases


def oracle_exp(orc):
    """as_expf of include/as_detmath.h through the oracle library; its attributes atan2, sin and cos are as_atan2f
    and the two halves of as_sincosf."""
    fp = C.POINTER(C.c_float)

    def call(fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        b = a if b is None else np.ascontiguousarray(b, np.float32)
        out = np.empty_like(a)
        orc.L.or_detmath_eval(C.c_int(fn), C.c_int(a.size), a.ctypes.data_as(fp), b.ctypes.data_as(fp),
                              out.ctypes.data_as(fp))
        return out

    def exp(x):
        return call(2, x)

    exp.atan2, exp.sin, exp.cos = (lambda y, x: call(0, y, x)), (lambda a: call(3, a)), (lambda a: call(4, a))
    return exp


def _yaw_quat(q, m):
    """rew_yaw_quat of the header; m: the oracle's math (oracle_exp)."""
    f = np.float32
    qw, qx, qy, qz = q
    yaw = m.atan2(f(2) * (qw * qz + qx * qy), f(1) - f(2) * (qy * qy + qz * qz))
    s, c = m.sin(yaw / f(2)), m.cos(yaw / f(2))
    nrm = np.maximum(np.sqrt(fma32(s, s, c * c)), f(1e-9))
    zero = np.zeros_like(c)
    return [c / nrm, zero / nrm, zero / nrm, s / nrm]


def yaw_frame_f64(x: dict, cmd_row: int, std: float):
    """(argument, value) of track_lin_vel_xy_yaw_frame_exp in float64 numpy on one step's rows."""
    q = x["root_quat"].astype(np.float64)
    v = x["root_lin"].astype(np.float64)
    yaw = np.arctan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] * q[2] + q[3] * q[3]))
    c, s = np.cos(yaw / 2), np.sin(yaw / 2)
    vx, vy = (c * c - s * s) * v[0] + 2 * c * s * v[1], -2 * c * s * v[0] + (c * c - s * s) * v[1]
    cmd = x["commands"].astype(np.float64)
    arg = -((cmd[cmd_row] - vx) ** 2 + (cmd[cmd_row + 1] - vy) ** 2) / std ** 2
    return arg, np.exp(arg)


def yaw_frame_bounds(x: dict, cmd_row: int, std: float):
    """How far the header's argument and value of track_lin_vel_xy_yaw_frame_exp may lie from the float64 ones, per
    env: (argument bound, value bound).  yaw = atan2(num, den): num and den carry four roundings each of terms of
    size at most 2 |q|^2, so the point (num, den) is off by at most 8 2^-24 |q|^2 and the angle by that over r =
    |(num, den)| (the yaw is ill-conditioned where r is small, at a pitch near +-90 degrees); as_atan2f adds 2.5 ulp
    of an angle of at most pi, 2.5 2^-22.  Halved for yaw / 2; as_sincosf adds 2 2^-24 to each of c and s and the
    normalisation three roundings: the yaw quaternion's components are within eq = dyaw / 2 + 5 2^-24.
    quat_rotate_inverse is quadratic in the unit quaternion with coefficients that sum to at most 4 |v|, and its own
    fifteen roundings add at most 16 2^-24 |v|: the rotated velocity is within ev = (4 eq + 2^-20) |v| per component.
    Then e = dx^2 + dy^2 moves by at most 2 (|dx| + |dy|) ev + 2 ev^2 + 4 2^-24 e with |dx| + |dy| <= sqrt(2 e), the
    argument -e / std^2 by that over std^2 plus 2 2^-24 |arg|, and the value by the factor exp(that), plus as_expf's
    2 ulp and one rounding (and 2^-126: as_expf gives +0 below the normal range)."""
    arg, val = yaw_frame_f64(x, cmd_row, std)
    q, v = x["root_quat"].astype(np.float64), x["root_lin"].astype(np.float64)
    num, den = 2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] * q[2] + q[3] * q[3])
    r = np.sqrt(num ** 2 + den ** 2)
    dyaw = 2.5 * 2.0 ** -22 + 8 * 2.0 ** -24 * np.maximum(1.0, (q ** 2).sum(0)) / r
    eq = dyaw / 2 + 5 * 2.0 ** -24
    ev = (4 * eq + 2.0 ** -20) * np.sqrt((v ** 2).sum(0))
    e = -arg * std ** 2
    de = 2 * np.sqrt(2 * e) * ev + 2 * ev ** 2 + 4 * 2.0 ** -24 * e
    darg = de / std ** 2 + 2 * 2.0 ** -24 * np.abs(arg)
    return darg, val * np.expm1(darg) + 3 * 2.0 ** -24 * val + 2.0 ** -126


def _clip_max(x, hi):  # torch's clip(max=hi): a NaN passes
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.where(x > hi, hi, x)).astype(np.float32)


def _clip_min(x, lo):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.where(x < lo, lo, x)).astype(np.float32)


def _add(acc, comp, v):
    """rew_add of the header: the compensated sum's step; returns (acc, comp)."""
    y = v - comp
    t = acc + y
    comp = np.where(np.isfinite(t), (t - acc) - y, np.float32(0)).astype(np.float32)
    return t, comp


def _norm3(x, y, z):
    return np.sqrt(fma32(z, z, fma32(y, y, x * x)))


def _gate(cmd, row):
    x, y = cmd[row], cmd[row + 1]
    return (np.sqrt(fma32(y, y, x * x)) > np.float32(0.1)).astype(np.float32)


def term_values(spec, x: dict, prev: np.ndarray, sim_dt: float, exp, clamp: bool = False, exp_args: dict | None = None):
    """f of every term of a parsed RewardTerms on one step's rows (float32, the header's order of operations):
    (terms, n).  exp_args, a dict, receives the exp terms' arguments by term index."""
    from allsteps_isaaclab_amd import _native

    f = np.float32
    sdt = f(sim_dt)
    n = x["root_quat"].shape[-1]
    q = [x["root_quat"][k] for k in range(4)]
    act = np.clip(x["actions"], -1, 1).astype(f) if clamp else x["actions"]
    out = np.zeros((len(spec.terms), n), f)
    with np.errstate(all="ignore"):
        for k, t in enumerate(spec.terms):
            kind = _native.REW_KINDS[t.kind]
            ids = list(t.ids)
            acc, comp = np.zeros(n, f), np.zeros(n, f)
            if kind in ("is_alive", "is_terminated"):
                term = x["terminated"].astype(bool)
                v = (term if kind == "is_terminated" else ~term).astype(f)
            elif kind in ("lin_vel_z_l2", "ang_vel_xy_l2", "flat_orientation_l2", "track_lin_vel_xy_exp",
                          "track_ang_vel_z_exp", YAW_FUNC):
                if kind == "flat_orientation_l2":
                    u = [np.zeros(n, f), np.zeros(n, f), np.full(n, -1, f)]
                else:
                    lin = kind in ("lin_vel_z_l2", "track_lin_vel_xy_exp", YAW_FUNC)
                    src = x["root_lin"] if lin else x["root_ang"]
                    u = [src[j] for j in range(3)]
                o = _rotate_inverse(_yaw_quat(q, exp) if kind == YAW_FUNC else q, u)
                if kind == "lin_vel_z_l2":
                    v = o[2] * o[2]
                elif kind in ("track_lin_vel_xy_exp", YAW_FUNC):
                    dx, dy = x["commands"][t.cmd_row] - o[0], x["commands"][t.cmd_row + 1] - o[1]
                    arg = -(dx * dx + dy * dy) / t.p0
                    v = exp(arg)
                elif kind == "track_ang_vel_z_exp":
                    d = x["commands"][t.cmd_row + 2] - o[2]
                    arg = -(d * d) / t.p0
                    v = exp(arg)
                else:
                    v = o[0] * o[0] + o[1] * o[1]
                if exp_args is not None and kind.endswith("_exp"):
                    exp_args[k] = arg
            elif kind == "track_ang_vel_z_world_exp":
                d = x["commands"][t.cmd_row + 2] - x["root_ang"][2]
                arg = -(d * d) / t.p0
                v = exp(arg)
                if exp_args is not None:
                    exp_args[k] = arg
            elif kind == "base_height_l2":
                d = x["root_pos"][2] - t.p0
                v = d * d
            elif kind.startswith("joint_"):
                for i, j in enumerate(ids):
                    if kind == "joint_vel_l1":
                        w = np.abs(x["qd"][j])
                    elif kind == "joint_vel_l2":
                        w = x["qd"][j] * x["qd"][j]
                    elif kind == "joint_deviation_l1":
                        w = np.abs(x["q"][j] - t.a[i])
                    elif kind == "joint_pos_limits":
                        w = -_clip_max(x["q"][j] - t.a[i], f(0)) + _clip_min(x["q"][j] - t.b[i], f(0))
                    else:
                        a = (x["qd"][j] - x["qd_prev"][j]) / sdt
                        w = a * a
                    acc, comp = _add(acc, comp, w)
                v = acc
            elif kind in ("action_l2", "action_rate_l2"):
                for j in range(act.shape[1]):
                    u = act[:, j] - prev[:, j] if kind == "action_rate_l2" else act[:, j]
                    acc, comp = _add(acc, comp, u * u)
                v = acc
            elif kind in ("undesired_contacts", "contact_forces"):
                count = np.zeros(n, np.int64)
                for b in ids:
                    m = None
                    for d in range(x["net"].shape[0]):
                        w = _norm3(*(x["net"][d, b, c] / sdt for c in range(3)))
                        m = w if m is None else np.where(~np.isnan(m) & ((w > m) | np.isnan(w)), w, m)
                    if kind == "undesired_contacts":
                        count += m > t.p0
                    else:
                        acc, comp = _add(acc, comp, _clip_min(m - t.p0, f(0)))
                v = count.astype(f) if kind == "undesired_contacts" else acc
            elif kind == "feet_air_time":
                for b in ids:
                    cc = x["timers"][2, b]
                    first = ((cc > 0) & (cc < t.p1)).astype(f)
                    acc, comp = _add(acc, comp, (x["timers"][1, b] - t.p0) * first)
                v = acc * _gate(x["commands"], t.cmd_row)
            else:  # feet_air_time_positive_biped
                cc = np.stack([x["timers"][2, b] for b in ids])
                air = np.stack([x["timers"][0, b] for b in ids])
                single = (cc > 0).sum(0) == 1
                mode = np.where(single[None], np.where(cc > 0, cc, air), f(0)).astype(f)
                m = mode[0]
                for i in range(1, len(ids)):
                    w = mode[i]
                    m = np.where(~np.isnan(m) & ((w < m) | np.isnan(w)), w, m)
                v = _clip_max(m, t.p0) * _gate(x["commands"], t.cmd_row)
            out[k] = v
    return out


def step_inputs(case: dict, s: int) -> dict:
    return {k: v[s] for k, v in case["inputs"].items()}


def host_step(spec, x: dict, state: dict, done: np.ndarray, dt: float, sim_dt: float, exp, clamp: bool = False):
    """One launch of k_rewards_step in float32 numpy.  state: episode_sums / step_reward / last_episode_sums (terms,
    n) and prev_actions (n, A), not modified.  Returns (reward, new state, f)."""
    f = np.float32
    dt = f(dt)
    fv = term_values(spec, x, state["prev_actions"], sim_dt, exp, clamp)
    st = {k: v.copy() for k, v in state.items()}
    total = np.zeros(fv.shape[1], f)
    done = done.astype(bool)
    with np.errstate(all="ignore"):
        for k, t in enumerate(spec.terms):
            if t.weight == 0:
                continue
            value = (fv[k] * t.weight) * dt
            total = total + value
            st["episode_sums"][k] = st["episode_sums"][k] + value
            st["step_reward"][k] = value / dt
    st["last_episode_sums"] = np.where(done[None], st["episode_sums"], st["last_episode_sums"])
    st["episode_sums"] = np.where(done[None], f(0), st["episode_sums"]).astype(f)
    act = np.clip(x["actions"], -1, 1).astype(f) if clamp else x["actions"]
    st["prev_actions"] = np.where(done[:, None], f(0), act).astype(f)
    return total, st, fv


def zero_state(terms: int, n: int, actions: int) -> dict:
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    return {"episode_sums": z(terms, n), "step_reward": z(terms, n), "last_episode_sums": z(terms, n),
            "prev_actions": z(n, actions)}


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """|a - b| in units of the last place of b (float32, finite values of one sign)."""
    ai = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    bi = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ai - bi)
