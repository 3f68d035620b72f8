"""The cases of tests/golden/noise.npz (gen_noise.py: the reference's outputs from recorded draws) as the
noise kernels take them -- shared by the host and GPU noise tests."""

from __future__ import annotations

import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 66


def model_cfg(case: dict, z):
    """The case's model as a user writes it: utils.noise cfg objects with Python floats or tensors."""
    from allsteps_isaaclab_amd.utils import noise as N_

    def term(kind, op, p0, p1):
        if kind == "constant":
            return N_.ConstantNoiseCfg(operation=op, bias=p0)
        if kind == "uniform":
            return N_.UniformNoiseCfg(operation=op, n_min=p0, n_max=p1)
        return N_.GaussianNoiseCfg(operation=op, mean=p0, std=p1)

    if case["p"] is None:
        p0, p1 = (torch.from_numpy(z[f"{case['name']}_p{i}"].copy()) for i in (0, 1))
    else:
        p0, p1 = case["p"]
    t = term(case["kind"], case["op"], p0, p1)
    b = case["bias"]
    if b is None:
        return N_.NoiseModelCfg(noise_cfg=t)
    return N_.NoiseModelWithAdditiveBiasCfg(noise_cfg=t, bias_noise_cfg=term(b["kind"], b["op"], *b["p"]))


def load_cases(device="cpu") -> list[dict]:
    """Every fixture case with its model built on `device` by the env's own host code (envs/noise.py: the
    scalar broadcast and the uniform width) and its arrays: x, draws (zeros for the constant term), and per
    step the reset mask, the bias draws and the reference's bias and output."""
    from allsteps_isaaclab_amd.envs.noise import NoiseModelState

    z = np.load(os.path.join(GOLDEN, "noise.npz"), allow_pickle=False)
    out = []
    for case in json.loads(str(z["cases"])):
        cols, name = case["cols"], case["name"]
        st = NoiseModelState(model_cfg(case, z), N, cols, torch.device(device), name)
        draws = {"constant": np.zeros((N, cols), np.float32), "uniform": z[f"u{cols}"],
                 "gaussian": z[f"z{cols}"]}[case["kind"]]
        steps = []
        for s in range(case["steps"]):
            if case["bias"] is None:
                zero = np.zeros(N, np.float32)
                steps.append((np.zeros(N, np.uint8), zero, zero, z[f"{name}_out{s}"]))
            else:
                steps.append(tuple(z[f"{name}_{k}{s}"] for k in ("mask", "bdraw", "bias", "out")))
        out.append({"name": name, "cols": cols, "state": st, "x": z[f"x{cols}"], "draws": draws, "steps": steps,
                    "random": case["kind"] != "constant"})
    return out
