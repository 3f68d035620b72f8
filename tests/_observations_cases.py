"""The cases of tests/golden/observations.npz as this project's cfg objects, and what the host and GPU tests share:
the parsed groups (envs/observations.py) with their device tables as host arrays, and the fixture's arrays."""

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "observations.npz")
SOURCES = ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "commands", "imu", "ray_hits", "ray_pose",
           "actions")


def load_fixture():
    z = np.load(FIXTURE)
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def context(z, meta):
    from allsteps_isaaclab_amd.envs.observations import ObsContext

    return ObsContext(joint_names=[f"joint_{k}" for k in range(meta["joints"])],
                      default_joint_pos=z["default_joint_pos"], default_joint_vel=z["default_joint_vel"],
                      soft_joint_pos_limits=z["soft_joint_pos_limits"], action_cols=meta["actions"],
                      clamp_actions=False, command_names=["base_velocity"],
                      ray_sensors={"height_scanner": meta["rays"]}, imu_names=["imu"])


def _noise_cfg(nz):
    import torch

    from allsteps_isaaclab_amd.utils import noise as N

    if nz is None:
        return None
    val = lambda v: torch.tensor(v, dtype=torch.float32) if isinstance(v, list) else v  # noqa: E731
    if nz["kind"] == "constant":
        return N.ConstantNoiseCfg(operation=nz["operation"], bias=val(nz["p0"]))
    if nz["kind"] == "uniform":
        return N.UniformNoiseCfg(operation=nz["operation"], n_min=val(nz["p0"]), n_max=val(nz["p1"]))
    return N.GaussianNoiseCfg(operation=nz["operation"], mean=val(nz["p0"]), std=val(nz["p1"]))


def group_cfg(case: dict):
    """The fixture case's group in this project's cfg classes and term functions."""
    from allsteps_isaaclab_amd.utils import commands as CM
    from allsteps_isaaclab_amd.utils import observations as OB
    from allsteps_isaaclab_amd.utils import sensors as SN
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    funcs = {**{k: getattr(OB, k) for k in dir(OB)}, "generated_commands": CM.generated_commands,
             "height_scan": SN.height_scan, "imu_orientation": SN.imu_orientation, "imu_ang_vel": SN.imu_ang_vel,
             "imu_lin_acc": SN.imu_lin_acc}
    group = OB.ObservationGroupCfg(concatenate_terms=case["concatenate_terms"],
                                   enable_corruption=case["enable_corruption"],
                                   history_length=case["history_length"],
                                   flatten_history_dim=case["flatten_history_dim"])
    for t in case["terms"]:
        p = dict(t["params"])
        params = {}
        if "joint_ids" in p:
            params["asset_cfg"] = SceneEntityCfg("robot", joint_ids=p.pop("joint_ids"))
        if "sensor" in p:
            params["sensor_cfg"] = SceneEntityCfg(p.pop("sensor"))
        if "imu" in p:
            params["asset_cfg"] = SceneEntityCfg(p.pop("imu"))
        params.update(p)
        scale = tuple(t["scale"]) if isinstance(t["scale"], list) else t["scale"]
        setattr(group, t["name"], OB.ObservationTermCfg(
            func=funcs[t["func"]], params=params, noise=_noise_cfg(t["noise"]),
            clip=None if t["clip"] is None else tuple(t["clip"]), scale=scale, history_length=t["history_length"],
            flatten_history_dim=t["flatten_history_dim"]))
    return group


def load_cases() -> list:
    """Per case: name, steps, the parsed GroupSpec (tables as host arrays), inputs {source: (steps, ...)}, draws
    (steps, d0, n), reset (steps, n) uint8 and the reference's out (steps, n, out_cols)."""
    from allsteps_isaaclab_amd.envs.observations import ObservationGroups

    z, meta = load_fixture()
    ctx = context(z, meta)
    cases = []
    for c in meta["cases"]:
        spec = ObservationGroups({c["name"]: group_cfg(c)}, ctx).groups[0]
        steps = c["steps"]
        cases.append({"name": c["name"], "steps": steps, "n": meta["n"], "spec": spec,
                      "inputs": {k: z[f"in_{c['inputs']}_{k}"][:steps] for k in SOURCES},
                      "draws": z[f"{c['draws']}_draws"][:steps], "reset": z[f"{c['name']}_reset"],
                      "out": z[f"{c['name']}_out"]})
    return cases


def source_rows(inputs: dict) -> list:
    """Rows of every source in AS_OBS_SRC_* order (the gravity constant has none)."""
    rows = []
    for k in SOURCES:
        a = inputs[k][0]
        rows.append(a.shape[1] if k == "actions" else int(np.prod(a.shape[:-1])))
    return rows + [0]
