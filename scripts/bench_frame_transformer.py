"""Cost of the frame-transformer kernel (cfg.frame_transformer) on one GPU, at 4096 envs.

The walker (Allsteps) after 20 steps of random actions, two sensors: the feet in the torso frame (2 frames) and the
20 stones in the left foot's frame under a source offset (20 frames).  By device events over windows of
back-to-back launches, three windows after a discarded one, the three kernels taking turns window by window:

  frame_transformer_us  one k_frame_transformer launch serving both sensors (22 lanes an env)
  imu1_us               one k_imu launch with one sensor (the torso), every env recomputed -- the same launch shape
  body_state_us         one k_body_state launch (as_body_state: the same FK, 16 rows of 17 bodies stored)

Writes the result as JSON to --out and prints it (DESIGN.md §3 "Frame transformer").  A record, not a threshold.

    python scripts/bench_frame_transformer.py [--sizes 4096] [--out profiles/frame_transformer_cost.json]
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
from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg, ImuCfg, OffsetCfg  # noqa: E402

DEV = "cuda:0"
WINDOWS = 4  # the first is discarded


def make(n: int):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    ns = "{ENV_REGEX_NS}"
    frame = FrameTransformerCfg.FrameCfg
    cfg.frame_transformer = {
        "feet": FrameTransformerCfg(prim_path=f"{ns}/Robot/torso", target_frames=[frame(prim_path=f"{ns}/Robot/.*_foot")]),
        "stones": FrameTransformerCfg(prim_path=f"{ns}/Robot/left_foot",
                                      source_frame_offset=OffsetCfg(pos=(0.0, 0.0, -0.05)),
                                      target_frames=[frame(prim_path=f"{ns}/step_.*")])}
    cfg.imu = ImuCfg(prim_path=f"{ns}/Robot/torso")
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
    env = make(n)
    g, i = env._frame_transformers, env._imus
    assert (g.num_sensors, g.num_frames) == (2, 22)
    fns = {"frame_transformer_us": g._launch,
           "imu1_us": lambda: env._native.imu(i._table, i.dt, True, i.outdated, i.data, i.prev, stream=env._stream()),
           "body_state_us": lambda: env.robot.data._bodies()}
    launches = 2000 if n <= 4096 else 500
    out = {k: [] for k in fns}
    for w in range(WINDOWS):
        for k, fn in fns.items():
            us = window_us(fn, launches)
            if w:
                out[k].append(us)
    res = {"launches_per_window": launches, "sensors": g.num_sensors, "frames": g.num_frames, **out,
           "median_us": {k: sorted(v)[len(v) // 2] for k, v in out.items()}}
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_transformer_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_transformer.py measures on the HIP device; none is available")
    out = {"device": torch.cuda.get_device_name(0), "windows": WINDOWS - 1,
           "sizes": {str(n): measure(n) for n in (int(x) for x in a.sizes.split(","))}}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
