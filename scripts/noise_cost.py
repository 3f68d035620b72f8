"""Cost of the noise models (cfg.action_noise_model / cfg.observation_noise_model) on one GPU.

Allsteps-v0 at 4096 envs, stone level 0, random actions: HIP-event-timed windows of 400 env steps (after 100
warm-up steps) of a clean env, an env with an observation model and an env with both models (Gaussian term,
Gaussian `abs` bias), interleaved over 5 rounds; then each noise kernel alone, launched back to back.  Prints
one JSON line (profiles/noise_cost.log; DESIGN.md §3 "Noise models").

    python scripts/noise_cost.py
"""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils import noise as N  # noqa: E402

DEV = "cuda:0"
ENVS, STEPS, ROUNDS = 4096, 400, 5


def make(obs, act):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = ENVS
    cfg.sim.device = DEV
    cfg.observation_noise_model, cfg.action_noise_model = obs, act
    env = AllstepsEnv(cfg)
    env.reset()
    return env


def model(std):
    return N.NoiseModelWithAdditiveBiasCfg(noise_cfg=N.GaussianNoiseCfg(std=std),
                                           bias_noise_cfg=N.GaussianNoiseCfg(std=std / 2, operation="abs"))


def timed(fn, k):
    """us per call of fn over k back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(k):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / k


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    envs = {"clean": make(None, None), "obs": make(model(0.05), None), "both": make(model(0.05), model(0.02))}
    gen = torch.Generator(device=DEV).manual_seed(1)
    acts = [torch.rand(ENVS, 21, device=DEV, generator=gen) * 2 - 1 for _ in range(16)]
    for env in envs.values():
        timed(lambda i: env.step(acts[i & 15]), 100)
    res = {k: [] for k in envs}
    for _ in range(ROUNDS):
        for k, env in envs.items():
            res[k].append(timed(lambda i: env.step(acts[i & 15]), STEPS))
    nz = envs["both"]._noise
    obs = torch.zeros(ENVS, 59, device=DEV)
    done = torch.zeros(ENVS, dtype=torch.bool, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    kernels = {}
    for name, fn in (("k_noise_actions", lambda i: nz.apply_actions(acts[0], 0, s)),
                     ("k_noise_post", lambda i: nz.post(obs, done, done, 0, s))):
        timed(fn, 100)
        kernels[name] = [timed(fn, 2000) for _ in range(3)]
    out = {"envs": ENVS, "steps_per_window": STEPS, "us_per_step": res,
           "median_us": {k: median(v) for k, v in res.items()}, "kernel_alone_us_back_to_back": kernels}
    out["delta_obs_us"] = out["median_us"]["obs"] - out["median_us"]["clean"]
    out["delta_both_us"] = out["median_us"]["both"] - out["median_us"]["clean"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
