"""Shared by the action manager's tests: the cases of tests/golden/actions.npz with the column tables
envs/actions.py makes of their cfgs, and a NumPy restatement of csrc/allsteps_actions.h (every float32 operation on
its own, in the header's order) that tests/test_actions_host.py holds to the header bit for bit."""

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "actions.npz")
BUFFERS = ("action", "prev_action", "processed", "prev_applied")
KIND_POSITION, KIND_EFFORT, KIND_TO_LIMITS, KIND_EMA = range(4)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(a, b) -> bool:
    return np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b) -> bool:
    """Bit for bit, except for which NaN a NaN is: a NaN an operation makes (inf - inf, 0 * inf) carries the sign the
    machine gives it (x86 and gfx950 differ), and torch.clamp's vector loop replaces a NaN's payload.  Where both are
    NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(bits(a)[~both], bits(b)[~both])


def build_cfgs(terms: list) -> dict:
    from allsteps_isaaclab_amd.utils import actions as AC

    return {t["name"]: getattr(AC, t["cls"])(asset_name="robot", **t["fields"]) for t in terms}


def context(z, meta: dict, joints: int, actuator: int):
    from allsteps_isaaclab_amd.envs.actions import ActContext

    return ActContext(joint_names=list(meta[f"joints{joints}"]), default_joint_pos=z[f"default_joint_pos_{joints}"],
                      soft_joint_pos_limits=z[f"soft_joint_pos_limits_{joints}"], actuator=actuator,
                      action_space=joints)


def load_cases() -> list:
    """The fixture's cases: name, n, steps, joints, spec (envs.actions.ActionTerms), inputs raw / joint_pos, the
    reference's arrays, resets {step: env ids}."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.actions import ActionTerms

    z = np.load(FIXTURE)
    meta = json.loads(bytes(z["meta"]).decode())
    out = []
    for c in meta["cases"]:
        effort = c["terms"][0]["cls"] == "JointEffortActionCfg"
        ctx = context(z, meta, c["joints"], _native.ACT_TORQUE if effort else _native.ACT_DC_MOTOR)
        spec = ActionTerms(build_cfgs(c["terms"]), ctx)
        name = c["name"]
        ref = {k: z[f"{name}_{k}"] for k in ("action", "prev_action", "raw", "processed", "prev_applied", "targets",
                                             "post_action", "post_prev_action", "post_raw", "post_prev_applied")}
        out.append({"name": name, "n": meta["n"], "steps": meta["steps"], "joints": c["joints"], "spec": spec,
                    "meta": c, "raw": z[f"in_{name}_raw"], "joint_pos": z[f"in_{name}_joint_pos"], "ref": ref,
                    "resets": {int(k): v for k, v in c["resets"].items()}})
    return out


def zero_state(n: int, cols: int, joints: int) -> dict:
    z = lambda k: np.zeros((n, k), np.float32)  # noqa: E731
    return {"action": z(cols), "prev_action": z(cols), "processed": z(cols), "prev_applied": z(cols),
            "cmd": z(joints)}


def clamp(x, lo, hi):
    """torch.clamp per element with std::max / std::min's comparisons; a NaN passes."""
    m = np.where(x < lo, lo, x)
    return np.where(np.isnan(x), x, np.where(hi < m, hi, m)).astype(np.float32)


def host_process(rows: np.ndarray, inp: np.ndarray, st: dict) -> None:
    """actions_process_one over every (env, column); rows (cols, 12) float32 words of as_action_column_t."""
    I = np.ascontiguousarray(rows, np.float32).view(np.int32)
    F = np.ascontiguousarray(rows, np.float32)
    joint, kind, rescale = I[:, 0], I[:, 1], I[:, 2]
    scale, offset, clo, chi, lo, hi, alpha, oma = (F[:, k] for k in range(4, 12))
    half = np.float32(0.5)
    inp = np.asarray(inp, np.float32)
    with np.errstate(all="ignore"):
        st["prev_action"][:] = st["action"]
        st["action"][:] = inp
        affine = kind <= KIND_EFFORT
        p = inp * scale
        p = np.where(affine, p + offset, p)
        p = clamp(p, clo, chi)
        x = clamp(p, np.float32(-1.0), np.float32(1.0))
        r = ((x * (hi - lo)) * half) + ((lo + hi) * half)
        p = np.where(~affine & (rescale != 0), r, p)
        e = alpha * p
        e = e + oma * st["prev_applied"]
        ema = kind == KIND_EMA
        p = np.where(ema, clamp(e, lo, hi), p).astype(np.float32)
    st["processed"][:] = p
    st["prev_applied"][:] = np.where(ema, p, st["prev_applied"])
    ok = (joint >= 0) & (joint < st["cmd"].shape[1])
    st["cmd"][:, joint[ok]] = p[:, ok]


def host_reset(rows: np.ndarray, st: dict, q: np.ndarray, mask=None) -> None:
    """actions_reset_one over the envs of mask ((n,) bool; None: all); q (joints, n)."""
    I = np.ascontiguousarray(rows, np.float32).view(np.int32)
    joint, kind = I[:, 0], I[:, 1]
    n = st["action"].shape[0]
    m = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    st["action"][m] = 0.0
    st["prev_action"][m] = 0.0
    ema = (kind == KIND_EMA) & (joint >= 0) & (joint < q.shape[0])
    jp = np.asarray(q, np.float32).T[:, np.clip(joint, 0, q.shape[0] - 1)]  # (n, cols)
    st["prev_applied"][:] = np.where(m[:, None] & ema[None, :], jp, st["prev_applied"])
