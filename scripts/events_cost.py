"""Cost of the interval events (cfg.events) on one GPU.

Allsteps-v0 at 4096 envs, stone level 0, random actions: HIP-event-timed windows of 400 env steps (after 100
warm-up steps) of a clean env and an env with one push_by_setting_velocity term (intervals of 0.05 - 0.2 s, so
about one env in eight fires per step), interleaved over 5 rounds; then the event kernel alone, launched back to
back, with that term and with a term that fires in every env in every step.  Prints one JSON line
(profiles/events_cost.log; DESIGN.md §3 "Interval events").

    python scripts/events_cost.py
"""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils import events as E  # noqa: E402

DEV = "cuda:0"
ENVS, STEPS, ROUNDS = 4096, 400, 5


def push(interval):
    return {"push_robot": E.EventTermCfg(func=E.push_by_setting_velocity, mode="interval", interval_range_s=interval,
                                         params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})}


def make(events):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = ENVS
    cfg.sim.device = DEV
    cfg.events = events
    env = AllstepsEnv(cfg)
    env.reset()
    return env


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
    envs = {"clean": make(None), "push": make(push((0.05, 0.2)))}
    gen = torch.Generator(device=DEV).manual_seed(1)
    acts = [torch.rand(ENVS, 21, device=DEV, generator=gen) * 2 - 1 for _ in range(16)]
    for env in envs.values():
        timed(lambda i: env.step(acts[i & 15]), 100)
    res = {k: [] for k in envs}
    for _ in range(ROUNDS):
        for k, env in envs.items():
            res[k].append(timed(lambda i: env.step(acts[i & 15]), STEPS))
    s = torch.cuda.current_stream().cuda_stream
    kernels = {}
    always = make(push((0.0, 0.01)))  # below one env step: every env fires at every launch
    for name, env in (("k_events_interval", envs["push"]), ("k_events_interval_all_fire", always)):
        ev, lin, ang = env._events, env.state["root_lin"].clone(), env.state["root_ang"].clone()
        fn = lambda i: ev.apply(lin, ang, 0, s)  # noqa: E731
        timed(fn, 100)
        kernels[name] = [timed(fn, 2000) for _ in range(3)]
        kernels[name + "_fired_fraction"] = float(ev.fired.float().mean())
    out = {"envs": ENVS, "steps_per_window": STEPS, "us_per_step": res,
           "median_us": {k: median(v) for k, v in res.items()}, "kernel_alone_us_back_to_back": kernels}
    out["delta_push_us"] = out["median_us"]["push"] - out["median_us"]["clean"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
