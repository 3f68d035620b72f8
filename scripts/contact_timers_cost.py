"""Cost of the contact sensors' air / contact timers (cfg.contact_air_time) on one GPU.

Allsteps-v0 at 4096 envs, stone level 0, random actions, with bench.py's protocol for the step loop -- a pre-heat,
the construction state restored, reset, 50 warm-up steps, then 1000 ``env.step`` calls between two device
synchronisations, timed on the host -- for an env with ``contact_forces = True`` alone (the contact report without
the timers: the baseline) and an env with ``contact_air_time = True`` (the report and one k_contact_timers launch
per step), alternating, three repetitions each; then the timer kernel alone, launched back to back.  Prints one
JSON line (DESIGN.md §3 "Contact timers").

    python scripts/contact_timers_cost.py
"""

import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg  # noqa: E402

DEV = "cuda:0"
ENVS, STEPS, WARMUP, REPS, PREHEAT_S = 4096, 1000, 50, 3, 0.25


def make(air: bool):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = ENVS
    cfg.sim.device = DEV
    cfg.contact_forces = True
    cfg.contact_air_time = air
    return AllstepsEnv(cfg)


def run(air: bool, actions) -> float:
    """ms per env.step over the timed window of one fresh env."""
    env = make(air)
    s_init = env.get_state()
    env.reset()
    k, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < PREHEAT_S:
        for _ in range(10):
            env.step(actions[k % (STEPS + WARMUP)])
            k += 1
        torch.cuda.synchronize()
    env.set_state(s_init)
    env.reset()
    for t in range(WARMUP):
        env.step(actions[STEPS + t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(STEPS):
        env.step(actions[t])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    env.close()
    return el * 1e3 / STEPS


def kernel_alone() -> list:
    """us per launch of k_contact_timers over the report a stepped env left, back to back, by device events."""
    env = make(True)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(20):
        env.step(torch.rand(ENVS, 21, device=DEV, generator=gen) * 2 - 1)
    tm = env._contact_timers
    out = []
    for rep in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(2000):
            tm.update(env.reset_terminated, env.reset_time_outs)
        e1.record()
        e1.synchronize()
        if rep:  # the first window warms up
            out.append(e0.elapsed_time(e1) * 1e3 / 2000)
    env.close()
    return out


def main():
    gen = torch.Generator(device=DEV).manual_seed(1000)
    actions = torch.rand(STEPS + WARMUP, ENVS, 21, device=DEV, generator=gen) * 2.0 - 1.0
    res = {"contact_forces": [], "contact_air_time": []}
    for _ in range(REPS):
        res["contact_forces"].append(run(False, actions))
        res["contact_air_time"].append(run(True, actions))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    out = {"envs": ENVS, "steps": STEPS, "warmup": WARMUP, "ms_per_step": res, "median_ms": med,
           "delta_us": (med["contact_air_time"] - med["contact_forces"]) * 1e3,
           "kernel_alone_us_back_to_back": kernel_alone()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
