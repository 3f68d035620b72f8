"""Generate tests/golden/actions.npz from the reference's own action code.

Loads ``isaaclab/managers/action_manager.py``, ``isaaclab/envs/mdp/actions/joint_actions.py``,
``joint_actions_to_limits.py``, ``isaaclab/utils/string.py`` and ``isaaclab/utils/math.py`` of a reference checkout BY
PATH, with stub modules of this file's own for the Isaac / Omniverse packages they import, and drives the real
``ActionManager.process_action()``, ``apply_action()`` and ``reset(env_ids)`` on the CPU over a stub env and a stub
articulation.  The stub articulation serves ``find_joints`` (over the reference's ``resolve_matching_names``),
``data.default_joint_pos``, ``data.soft_joint_pos_limits`` and ``data.joint_pos`` (recorded arrays) and records what
``set_joint_position_target`` / ``set_joint_effort_target`` hand it.  The manager's and the terms' base classes are
stubs that keep the cfg and the env; the term cfg classes are this project's (same fields), their ``class_type`` set
to the reference's term classes here.

Per case and step the file holds the inputs ``in_<case>_raw`` (steps, n, columns) and ``in_<case>_joint_pos`` (steps,
n, joints), and after ``process_action`` + ``apply_action``: ``action``, ``prev_action``, ``raw`` and ``processed``
(the terms' tensors side by side in cfg order), ``prev_applied`` (the EMA terms' ``_prev_applied_actions``, zero
columns for the other terms) and ``targets`` (n, joints), what the articulation was handed.  A step listed in the
case's ``resets`` is followed by ``reset(env_ids)`` on that step's joint positions; ``post_action``,
``post_prev_action``, ``post_raw`` and ``post_prev_applied`` hold the state after it (after the step where there is no
reset).  The first step of every case runs on the freshly built manager (no reset before it).

``reset(env_ids)`` of an EMA term over a SUBSET of the joints cannot run in the reference: its reset indexes
``_prev_applied_actions[env_ids[:, None], :]`` (k, 1, joints of the term) against ``joint_pos[env_ids[:, None],
joint_ids]`` (k, joints of the term), which raises for every input (and the manager hands a slice for env_ids = None,
which ``[:, None]`` rejects).  Cases c and d therefore run without resets -- ``check_subset_reset_cannot_run`` asserts
that the reference still raises, so that a fixed reference is noticed -- and case f, an EMA term over all joints, has
them.

Cases (n = 16; steps 5; where a case has resets: after steps 1 and 3, of envs 1, 4, 7, 12):

  a   12 joints, the velocity task's JointPositionActionCfg(joint_names=[".*"], scale=0.5, use_default_offset=True)
  b   12 joints, JointPositionActionCfg with preserve_order over three expressions, dict scale, dict offset
      (use_default_offset off) and a dict clip on some joints
  c   12 joints, two terms splitting the joints: JointPositionToLimitsActionCfg (dict scale, dict clip, rescale on) on
      the front legs, EMAJointPositionToLimitsActionCfg (alpha 0.8, where float32(1 - alpha) formed in
      double and 1 - float32(alpha) differ; rescale off) on the hind legs; no resets
  d   12 joints, three EMA terms: alpha 0.0 (rescale on), alpha 1.0 (rescale off, float scale), alpha a dict (rescale
      on) with a joint the dict leaves at 1; no resets
  e   21 joints, two JointEffortActionCfg terms: a dict scale with a float offset, and a float scale with a clip
  f   12 joints, one EMA term over all joints: alpha a dict with 0, 1 and interior values, dict scale, rescale on

Raw actions: normal draws times 1.2 (many beyond +-1); in steps 0 and 2 the envs 0..7 hold +0, -0, +-1.5, +-3e38 (the
scaled value overflows), +-inf and NaN in every column.

    python tests/golden/gen_actions.py --reference DIR [--check]

--check regenerates into memory and compares with the committed file byte for byte.
"""

from __future__ import annotations

import argparse
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "actions.npz")
PKG = os.path.join("source", "isaaclab", "isaaclab")
N, STEPS = 16, 5
RESETS = {1: [1, 4, 7, 12], 3: [1, 4, 7, 12]}

for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGS = ("LF", "LH", "RF", "RH")
JOINTS12 = [f"{leg}_{j}" for j in ("HAA", "HFE", "KFE") for leg in LEGS]
JOINTS21 = ["abdomen_z", "abdomen_y", "abdomen_x"] + \
           [f"{s}_{j}" for s in ("right", "left") for j in ("hip_x", "hip_z", "hip_y", "knee", "ankle_y", "ankle_x")] + \
           [f"{s}_{j}" for s in ("right", "left") for j in ("shoulder_x", "shoulder_y", "elbow")]
assert len(JOINTS12) == 12 and len(JOINTS21) == 21


class _Any:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Any()

    def __call__(self, *a, **k):
        return _Any()


class _ManagerTermBase:
    """manager_base.py ``ManagerTermBase`` as far as ActionTerm needs it."""

    def __init__(self, cfg, env):
        self.cfg, self._env = cfg, env

    num_envs = property(lambda self: self._env.num_envs)
    device = property(lambda self: self._env.device)


class _ManagerBase:
    """manager_base.py ``ManagerBase`` as far as ActionManager needs it."""

    def __init__(self, cfg, env):
        self.cfg, self._env = cfg, env
        self._prepare_terms()

    num_envs = property(lambda self: self._env.num_envs)
    device = property(lambda self: self._env.device)


def _mod(name: str, **attrs) -> types.ModuleType:
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def _load(name: str, path: str, package: str):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    m.__package__ = package
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    spec.loader.exec_module(m)
    return m


def load_reference(root: str):
    """(action_manager, joint_actions, joint_actions_to_limits, string modules) of the reference at ``root``."""
    from allsteps_isaaclab_amd.utils.actions import ActionTermCfg

    pkg = os.path.join(root, PKG)
    for name in ("omni", "omni.kit", "carb", "isaaclab", "isaaclab.utils", "isaaclab.envs", "isaaclab.envs.mdp",
                 "isaaclab.envs.mdp.actions", "isaaclab.managers"):
        _mod(name)
    _mod("omni.log", info=lambda *a, **k: None, warn=lambda *a, **k: None)
    _mod("omni.kit.app")
    _mod("prettytable", PrettyTable=_Any)
    _mod("isaaclab.assets", AssetBase=_Any, Articulation=_Any)
    _mod("isaaclab.assets.articulation", Articulation=_Any)
    _mod("isaaclab.managers.manager_base", ManagerBase=_ManagerBase, ManagerTermBase=_ManagerTermBase)
    _mod("isaaclab.managers.manager_term_cfg", ActionTermCfg=ActionTermCfg)
    string_mod = _load("isaaclab.utils.string", os.path.join(pkg, "utils", "string.py"), "isaaclab.utils")
    _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    am = _load("isaaclab.managers.action_manager", os.path.join(pkg, "managers", "action_manager.py"),
               "isaaclab.managers")
    ja = _load("isaaclab.envs.mdp.actions.joint_actions", os.path.join(pkg, "envs", "mdp", "actions",
                                                                       "joint_actions.py"),
               "isaaclab.envs.mdp.actions")
    jl = _load("isaaclab.envs.mdp.actions.joint_actions_to_limits",
               os.path.join(pkg, "envs", "mdp", "actions", "joint_actions_to_limits.py"), "isaaclab.envs.mdp.actions")
    return am, ja, jl, string_mod


# ------------------------------------------------------------------------------------------------ the stubs
class StubArticulation:
    """The asset the terms see: the reference's name resolution over ``joint_names``, recorded data, and a record
    of the targets it is handed."""

    def __init__(self, string_mod, names: list, default: np.ndarray, limits: np.ndarray):
        self._string = string_mod
        self.joint_names, self.num_joints = list(names), len(names)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
        self.data = types.SimpleNamespace(
            default_joint_pos=t(default).unsqueeze(0).repeat(N, 1), default_joint_vel=torch.zeros(N, len(names)),
            soft_joint_pos_limits=t(limits).unsqueeze(0).repeat(N, 1, 1), joint_pos=torch.zeros(N, len(names)))
        self.targets = torch.zeros(N, len(names))
        self.handed = {"position": 0, "effort": 0}

    def find_joints(self, name_keys, joint_subset=None, preserve_order: bool = False):
        return self._string.resolve_matching_names(name_keys, self.joint_names, preserve_order)

    def _take(self, kind, target, joint_ids):
        self.targets[:, slice(None) if joint_ids is None else joint_ids] = target
        self.handed[kind] += 1

    def set_joint_position_target(self, target, joint_ids=None, env_ids=None):
        self._take("position", target, joint_ids)

    def set_joint_effort_target(self, target, joint_ids=None, env_ids=None):
        self._take("effort", target, joint_ids)


class StubEnv:
    device = "cpu"
    num_envs = N

    def __init__(self, asset):
        self.scene = {"robot": asset}


# ------------------------------------------------------------------------------------------------ cases
def _q8(x):
    return (np.round(np.asarray(x, np.float64) * 256.0) / 256.0).astype(np.float32)


def robot_data(joints: int):
    """(default_joint_pos (J,), soft_joint_pos_limits (J, 2)) of the stub robots: off-grid float32 values."""
    rng = np.random.default_rng(1000 + joints)
    lo = (-1.6 + 0.5 * rng.uniform(0, 1, joints)).astype(np.float32)
    hi = (0.9 + 0.8 * rng.uniform(0, 1, joints)).astype(np.float32)
    default = (0.5 * rng.uniform(-1, 1, joints)).astype(np.float32)
    return default, np.stack([lo, hi], -1)


def case_specs() -> list:
    """The cases as plain data (JSON): per term its cfg class of utils/actions.py and its fields."""
    T = lambda name, cls, **fields: {"name": name, "cls": cls, "fields": fields}  # noqa: E731
    cases = _case_list(T)
    for c in cases:
        c["resets"] = {str(k): v for k, v in RESETS.items()} if c["name"] not in ("c", "d") else {}
    return cases


def _case_list(T) -> list:
    return [
        {"name": "a", "joints": 12, "terms": [
            T("joint_pos", "JointPositionActionCfg", joint_names=[".*"], scale=0.5, use_default_offset=True)]},
        {"name": "b", "joints": 12, "terms": [
            T("joint_pos", "JointPositionActionCfg", joint_names=[".*_KFE", ".*_HAA", ".*_HFE"], preserve_order=True,
              scale={".*_HAA": 0.3, ".*_HFE": 1.7, "L._KFE": 0.25}, offset={"R.*": -0.1, "LF_HFE": 0.45},
              use_default_offset=False, clip={".*_KFE": [-0.7, 0.4], "LH_HAA": [-0.05, 0.05]})]},
        {"name": "c", "joints": 12, "terms": [
            T("front", "JointPositionToLimitsActionCfg", joint_names=[".F_.*"], scale={".*": 0.9, },
              clip={"LF_.*": [-0.8, 0.6]}, rescale_to_limits=True),
            T("hind", "EMAJointPositionToLimitsActionCfg", joint_names=[".H_.*"], scale=0.6, alpha=0.8,
              rescale_to_limits=False)]},
        {"name": "d", "joints": 12, "terms": [
            T("haa", "EMAJointPositionToLimitsActionCfg", joint_names=[".*_HAA"], alpha=0.0, rescale_to_limits=True),
            T("hfe", "EMAJointPositionToLimitsActionCfg", joint_names=[".*_HFE"], scale=1.3, alpha=1.0,
              rescale_to_limits=False),
            T("kfe", "EMAJointPositionToLimitsActionCfg", joint_names=[".*_KFE"], scale={"R.*": 0.7},
              alpha={"L._KFE": 0.1, "RF_KFE": 0.85}, clip={"RH_KFE": [-0.5, 2.0]}, rescale_to_limits=True)]},
        {"name": "e", "joints": 21, "terms": [
            T("legs", "JointEffortActionCfg", joint_names=[".*_hip_.*", ".*_knee", ".*_ankle_.*"],
              scale={".*_hip_.*": 45.0, ".*_knee": 80.5, ".*_ankle_.*": 21.3}, offset=0.125),
            T("upper", "JointEffortActionCfg", joint_names=["abdomen_.*", ".*_shoulder_.*", ".*_elbow"], scale=33.3,
              clip={"abdomen_.*": [-20.0, 25.5]})]},
        {"name": "f", "joints": 12, "terms": [
            T("ema", "EMAJointPositionToLimitsActionCfg", joint_names=[".*"], scale={".*_HFE": 0.8, ".*_KFE": 1.1},
              alpha={".*_HAA": 0.0, "L._HFE": 1.0, "R._HFE": 0.85, ".*_KFE": 0.2}, rescale_to_limits=True)]},
    ]


def build_cfgs(terms: list) -> dict:
    """{name: cfg} of utils/actions.py from a case's term list."""
    from allsteps_isaaclab_amd.utils import actions as AC

    return {t["name"]: getattr(AC, t["cls"])(asset_name="robot", **t["fields"]) for t in terms}


def make_inputs(rng, joints: int, cols: int) -> dict:
    raw = (1.2 * rng.standard_normal((STEPS, N, cols))).astype(np.float32)
    edge = np.array([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, np.inf, -np.inf], np.float32)
    for s in (0, 2):
        half = cols // 2  # +-0, +-1.5, ... in both orders across the columns
        raw[s, :8, :half] = edge[:, None]
        raw[s, :8, half:] = edge[[1, 0, 3, 2, 5, 4, 7, 6], None]
        raw[s, 7, ::2] = np.nan
    lo_hi = robot_data(joints)[1]
    jp = (lo_hi[:, 0] + (lo_hi[:, 1] - lo_hi[:, 0]) * rng.uniform(0, 1, (STEPS, N, joints))).astype(np.float32)
    return {"raw": raw, "joint_pos": jp}


def run_case(ref, spec: dict, x: dict) -> dict:
    am, ja, jl, string_mod = ref
    classes = {"JointPositionActionCfg": ja.JointPositionAction, "JointEffortActionCfg": ja.JointEffortAction,
               "JointPositionToLimitsActionCfg": jl.JointPositionToLimitsAction,
               "EMAJointPositionToLimitsActionCfg": jl.EMAJointPositionToLimitsAction}
    names = JOINTS12 if spec["joints"] == 12 else JOINTS21
    default, limits = robot_data(spec["joints"])
    asset = StubArticulation(string_mod, names, default, limits)
    env = StubEnv(asset)
    cfgs = build_cfgs(spec["terms"])
    for t in spec["terms"]:
        cfgs[t["name"]].class_type = classes[t["cls"]]
    mgr = am.ActionManager(types.SimpleNamespace(**cfgs), env)
    assert mgr.active_terms == [t["name"] for t in spec["terms"]]
    terms = [mgr.get_term(k) for k in mgr.active_terms]

    def side_by_side(get):
        return torch.cat([get(t) for t in terms], 1).numpy().copy()

    def applied(t):
        return t._prev_applied_actions if hasattr(t, "_prev_applied_actions") else torch.zeros_like(t.raw_actions)

    keys = ("action", "prev_action", "raw", "processed", "prev_applied", "targets", "post_action", "post_prev_action",
            "post_raw", "post_prev_applied")
    out = {k: [] for k in keys}
    for s in range(STEPS):
        asset.data.joint_pos = torch.from_numpy(x["joint_pos"][s].copy())
        mgr.process_action(torch.from_numpy(x["raw"][s].copy()))
        mgr.apply_action()
        out["action"].append(mgr.action.numpy().copy())
        out["prev_action"].append(mgr.prev_action.numpy().copy())
        out["raw"].append(side_by_side(lambda t: t.raw_actions))
        out["processed"].append(side_by_side(lambda t: t.processed_actions))
        out["prev_applied"].append(side_by_side(applied))
        out["targets"].append(asset.targets.numpy().copy())
        if str(s) in spec["resets"]:
            assert mgr.reset(torch.tensor(spec["resets"][str(s)])) == {}
        out["post_action"].append(mgr.action.numpy().copy())
        out["post_prev_action"].append(mgr.prev_action.numpy().copy())
        out["post_raw"].append(side_by_side(lambda t: t.raw_actions))
        out["post_prev_applied"].append(side_by_side(applied))
    res = {k: np.stack(v) for k, v in out.items()}
    # raw_actions and the manager's action are equal at every point, as the term views of this project assume
    assert np.array_equal(res["raw"].view(np.uint32), res["action"].view(np.uint32))
    assert np.array_equal(res["post_raw"].view(np.uint32), res["post_action"].view(np.uint32))
    if not spec["resets"]:
        check_subset_reset_cannot_run(mgr)
    info = {"dims": list(mgr.action_term_dim), "total": int(mgr.total_action_dim),
            "term_joints": [list(t._joint_names) for t in terms],
            "handed": dict(asset.handed)}
    return res, info


def check_subset_reset_cannot_run(mgr) -> None:
    """The reference's reset of an EMA term over a subset of the joints still raises (see the module docstring)."""
    for env_ids in (torch.tensor([1, 4]), None):
        try:
            mgr.reset(env_ids)
        except (RuntimeError, TypeError):
            continue
        raise AssertionError("the reference's EMA reset over a joint subset now runs: give cases c and d resets")


def generate(reference: str) -> dict:
    ref = load_reference(reference)
    rng = np.random.default_rng(20261101)
    out, cases = {}, []
    for spec in case_specs():
        spec = json.loads(json.dumps(spec))  # the cfgs are built from what the file will hold
        x = make_inputs(rng, spec["joints"], spec["joints"])  # every case commands every joint once
        res, info = run_case(ref, spec, x)
        assert info["total"] == spec["joints"], spec["name"]
        for k, v in x.items():
            out[f"in_{spec['name']}_{k}"] = v
        for k, v in res.items():
            out[f"{spec['name']}_{k}"] = v
        # what the cases must exercise
        p = res["processed"]
        assert np.isnan(p).any() and np.isfinite(p).any(), spec["name"]
        assert np.isnan(x["raw"]).any() and np.isposinf(x["raw"]).any() and np.isneginf(x["raw"]).any()
        assert (np.abs(x["raw"][np.isfinite(x["raw"])]) > 1).any()
        assert np.signbit(x["raw"][x["raw"] == 0]).any() and not np.signbit(x["raw"][x["raw"] == 0]).all()
        cases.append({**spec, **info})
    meta = {"n": N, "steps": STEPS, "cases": cases, "joints12": JOINTS12, "joints21": JOINTS21}
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    for j in (12, 21):
        out[f"default_joint_pos_{j}"], out[f"soft_joint_pos_limits_{j}"] = robot_data(j)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ALLSTEPS_REFERENCE"), required=False)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or ALLSTEPS_REFERENCE) names the reference checkout")
    torch.set_num_threads(1)
    arrays = generate(args.reference)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    data = buf.getvalue()
    if args.check:
        with open(OUT, "rb") as f:
            same = f.read() == data
        print("actions.npz:", "identical" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT}: {len(data)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
