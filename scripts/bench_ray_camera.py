"""Cost of the ray-cast camera kernel (cfg.camera) on one GPU, at 4096 envs.

The walker (Allsteps) after 20 steps of random actions, a camera on the root pitched 0.2 rad down, ground + stones.
By device events over windows of back-to-back launches, three windows after a discarded one, the kernels taking
turns window by window:

  camera_32x32_all_us    one k_ray_camera launch at 32 x 32 with all three outputs
  camera_32x32_plane_us  one k_ray_camera launch at 32 x 32 with distance_to_image_plane only
  ray_cast_1024_us       one k_ray_cast launch (the height scanner's kernel) fed the same 1024 local rays with
                         attach_yaw_only = False
  camera_64x48_all_us    one k_ray_camera launch at 64 x 48 with all three outputs

The yardstick is ray_cast_1024_us from the same run: camera_32x32_plane_us traces the same rays against the same
boxes and stores a third of the floats, so the expectation is that it is no slower.  No threshold is fixed here.
Writes the result as JSON to --out and prints it (DESIGN.md §3 "Ray-cast camera").

    python scripts/bench_ray_camera.py [--num-envs 4096] [--out profiles/ray_camera_cost.json]
"""

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from allsteps_isaaclab_amd import _native  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils.sensors import RayCasterCameraCfg, patterns  # noqa: E402

DEV = "cuda:0"
WINDOWS = 4  # the first is discarded
TYPES = ["distance_to_image_plane", "distance_to_camera", "normals"]


def camera_cfg(width: int, height: int, data_types) -> RayCasterCameraCfg:
    return RayCasterCameraCfg(
        prim_path="/World/envs/env_.*/Robot/walker3d", mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_.*"],
        offset=RayCasterCameraCfg.OffsetCfg(pos=(0.2, 0.0, 0.3), rot=(math.cos(0.1), 0.0, math.sin(0.1), 0.0),
                                            convention="world"),
        data_types=list(data_types), pattern_cfg=patterns.PinholeCameraPatternCfg(width=width, height=height))


def make(n: int):
    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.camera = {"all32": camera_cfg(32, 32, TYPES), "plane32": camera_cfg(32, 32, TYPES[:1]),
                  "all64": camera_cfg(64, 48, TYPES)}
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
    nat, stream = env._native, env._stream()

    def camera(name):
        c = env.scene.sensors[name]
        im = c.images
        return lambda: nat.ray_camera(c._native_cfg, c.dirs, c.offset, c.pose, im.get(TYPES[0]), im.get(TYPES[1]),
                                      im.get(TYPES[2]), stream=stream)

    # k_ray_cast on the same rays: the camera's 1024 local directions turned by its offset, every start the offset's
    # position, the full root orientation
    cam = env.scene.sensors["all32"]
    off = cam.offset[:, 0]
    w, u = off[3], off[4:7]
    d = cam.dirs.T
    t = torch.linalg.cross(u.expand_as(d), d, dim=-1) * 2
    d = (d + w * t) + torch.linalg.cross(u.expand_as(d), t, dim=-1)
    rays = torch.cat([off[:3].reshape(3, 1).expand(3, 1024), d.T]).contiguous()
    hits = torch.zeros(3, 1024, n, device=DEV)
    scan_cfg = _native.AsRayCaster(1024, 0, 3, 1e6, 0.0)

    fns = {"camera_32x32_all_us": camera("all32"), "camera_32x32_plane_us": camera("plane32"),
           "ray_cast_1024_us": lambda: nat.ray_cast(scan_cfg, rays, hits, None, None, stream=stream),
           "camera_64x48_all_us": camera("all64")}
    launches = 300
    out = {k: [] for k in fns}
    for wdw in range(WINDOWS):
        for k, fn in fns.items():
            us = window_us(fn, launches)
            if wdw:
                out[k].append(us)
    torch.cuda.synchronize()
    # the two kernels looked at the same scene: where both hit, the scanner's hit distance is the camera's (up to the
    # rounding of the direction, formed by two rotations there and by one here; a ray next to an edge may differ)
    dist = (hits - (cam.pose[:3].reshape(3, 1, n))).norm(dim=0).T  # (n, 1024); the directions are unit vectors
    depth = cam.images[TYPES[1]].reshape(n, 1024)
    both = torch.isfinite(depth) & torch.isfinite(dist)
    diff = (dist[both] - depth[both]).abs()
    res = {"launches_per_window": launches, **out,
           "median_us": {k: sorted(v)[len(v) // 2] for k, v in out.items()},
           "pixels_hit_share": float(torch.isfinite(depth).float().mean()),
           "scanner_minus_camera_median_m": float(diff.median()),
           "scanner_within_1mm_of_camera_share": float((diff < 1e-3).float().mean())}
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_camera_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_camera.py measures on the HIP device; none is available")
    out = {"device": torch.cuda.get_device_name(0), "windows": WINDOWS - 1, "num_envs": a.num_envs,
           **measure(a.num_envs)}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
