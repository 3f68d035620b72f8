"""Cost of the IMU kernel (cfg.imu) on one GPU, at 4096 and 32768 envs.

The walker (Allsteps) after 20 steps of random actions.  Per size, by device events over windows of back-to-back
launches, three windows after a discarded one, the three kernels taking turns window by window:

  imu1_us        one k_imu launch with one sensor (the torso), every env recomputed (`all` = 1)
  imu3_us        one k_imu launch with three sensors (torso, left foot under a tilted offset, right thigh)
  body_state_us  one k_body_state launch (as_body_state: the same FK, 16 rows of 17 bodies stored)

k_imu runs k_body_state's FK and stores 25 floats per sensor where k_body_state stores 16 x 17 per env, so the
expectation is that it is no slower in the same run.  Writes the result as JSON to --out and prints it
(DESIGN.md §3 "IMU").

    python scripts/bench_imu.py [--sizes 4096,32768] [--out profiles/imu_cost.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils.sensors import ImuCfg  # noqa: E402

DEV = "cuda:0"
WINDOWS = 4  # the first is discarded


def make(n: int, sensors: int):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    path = "/World/envs/env_.*/Robot/"
    imus = {"imu": ImuCfg(prim_path=path + "torso"),
            "foot_imu": ImuCfg(prim_path=path + "left_foot",
                               offset=ImuCfg.OffsetCfg(pos=(0.1, -0.05, 0.2), rot=(0.8, 0.3, -0.4, 0.2))),
            "thigh_imu": ImuCfg(prim_path=path + "right_thigh", gravity_bias=(0.0, 0.0, 0.0))}
    cfg.imu = dict(list(imus.items())[:sensors])
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
    one, three = make(n, 1), make(n, 3)

    def imu(env):
        g = env._imus
        return lambda: env._native.imu(g._table, g.dt, True, g.outdated, g.data, g.prev, stream=env._stream())

    fns = {"imu1_us": imu(one), "imu3_us": imu(three), "body_state_us": lambda: three.robot.data._bodies()}
    launches = 2000 if n <= 4096 else 500
    out = {k: [] for k in fns}
    for w in range(WINDOWS):
        for k, fn in fns.items():
            us = window_us(fn, launches)
            if w:
                out[k].append(us)
    res = {"launches_per_window": launches, **out,
           "median_us": {k: sorted(v)[len(v) // 2] for k, v in out.items()}}
    one.close(), three.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096,32768")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imu_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imu.py measures on the HIP device; none is available")
    out = {"device": torch.cuda.get_device_name(0), "windows": WINDOWS - 1,
           "sizes": {str(n): measure(n) for n in (int(x) for x in a.sizes.split(","))}}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
