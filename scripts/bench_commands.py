"""Cost of the command kernel (cfg.commands) on one GPU, at 4096 envs.

The walker (Allsteps) after 20 steps of random actions.  By device events over windows of back-to-back launches,
three windows after a discarded one, the kernels taking turns window by window:

  commands1_us          one k_commands_step launch, one uniform term with heading_command (resampling every 10 s)
  commands4_us          one k_commands_step launch, four terms (two uniform with heading, one uniform, one normal)
  commands1_resample_us the one-term launch with resampling_time_range = (0, 0): every env resamples in every launch
  events_interval_us    one k_events_interval launch with one push term, on the same run, for scale

The kernel is launch- and latency-bound: one thread an env, a few dozen words an env and term.  Writes the result as
JSON to --out and prints it (DESIGN.md §3 "Command manager").  A record, not a threshold.

    python scripts/bench_commands.py [--sizes 4096] [--out profiles/commands_cost.json]
"""

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils import events as E  # noqa: E402
from allsteps_isaaclab_amd.utils.commands import NormalVelocityCommandCfg, UniformVelocityCommandCfg  # noqa: E402

DEV = "cuda:0"
WINDOWS = 4  # the first is discarded


def uniform(heading: bool, time=(10.0, 10.0)):
    return UniformVelocityCommandCfg(
        asset_name="robot", resampling_time_range=time, heading_command=heading, heading_control_stiffness=0.5,
        rel_standing_envs=0.02, rel_heading_envs=1.0,
        ranges=UniformVelocityCommandCfg.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-1.0, 1.0), ang_vel_z=(-1.0, 1.0),
                                                heading=(-math.pi, math.pi) if heading else None))


def normal():
    return NormalVelocityCommandCfg(
        asset_name="robot", resampling_time_range=(5.0, 10.0), rel_standing_envs=0.02,
        ranges=NormalVelocityCommandCfg.Ranges(mean_vel=(0.5, 0.0, 0.0), std_vel=(0.3, 0.2, 0.4),
                                               zero_prob=(0.1, 0.3, 0.3)))


def make(n: int, commands: dict, events=None):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.commands = commands
    cfg.events = events
    env = AllstepsEnv(cfg)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(20):
        env.step(torch.rand(n, 21, device=DEV, generator=gen) * 2 - 1)
    return env


def window_us(fn, launches: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def measure(n: int) -> dict:
    push = {"push": E.EventTermCfg(func=E.push_by_setting_velocity, mode="interval", interval_range_s=(10.0, 15.0),
                                   params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})}
    envs = {"commands1_us": make(n, {"base_velocity": uniform(True)}, push),
            "commands4_us": make(n, {"a": uniform(True), "b": uniform(True), "c": uniform(False), "d": normal()}),
            "commands1_resample_us": make(n, {"base_velocity": uniform(True, (0.0, 0.0))})}

    def launch(env):
        s = env.state
        return lambda: env._commands.apply(s["root_quat"], s["root_lin"], s["root_ang"], None, None, 0, env._stream())

    fns = {k: launch(e) for k, e in envs.items()}
    first = envs["commands1_us"]
    fns["events_interval_us"] = lambda: first._events.apply(first.state["root_lin"], first.state["root_ang"], 0,
                                                            first._stream())
    launches = 2000 if n <= 4096 else 500
    out = {k: [] for k in fns}
    for w in range(WINDOWS):
        for k, fn in fns.items():
            us = window_us(fn, launches)
            if w:
                out[k].append(us)
    res = {"launches_per_window": launches, **out, "median_us": {k: sorted(v)[len(v) // 2] for k, v in out.items()}}
    for e in envs.values():
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commands_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_commands.py measures on the HIP device; none is available")
    out = {"device": torch.cuda.get_device_name(0), "windows": WINDOWS - 1,
           "sizes": {str(n): measure(n) for n in (int(x) for x in a.sizes.split(","))}}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
