"""Cost of the quadruped's masked reset (as_quad_reset_mask, k_quad<true>), 1 GPU.

    python scripts/bench_quad_reset.py [--num_envs 16384] [--launches 2000] [--samples 7] [--out profiles/quad_reset_cost.json]

One launch resets the envs of a device mask; timed here at 1 %, 50 % and 100 % of the envs masked (seeded random
masks), with as_quad_reset_all -- the same reset of every env, plus the wave-map rebuild -- beside it as the
yardstick.  The envs are first stepped 100 times with random actions, so the state the resets read is a used one.
Each sample is a window of `launches` back-to-back launches between two device events (after a warm-up window of
the same call), so a figure is the steady cost of one launch in a queue, launch gaps included; the median of the
windows is reported with all of them.  Prints one JSON line and, with --out, writes the same as a file.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def window_us(fn, launches: int, samples: int) -> list:
    for _ in range(launches):  # warm-up: code objects loaded, clocks up
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(launches):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / launches)
    return out


def measure(num_envs: int = 16384, launches: int = 2000, samples: int = 7, device: str = "cuda:0") -> dict:
    from allsteps_isaaclab_amd import registry

    cfg = registry.load_cfg_from_registry("Allsteps-AnymalC-v0", "env_cfg_entry_point")
    cfg.scene.num_envs = num_envs
    cfg.sim.device = device
    env = registry.make("Allsteps-AnymalC-v0", cfg=cfg)
    env.reset()
    gen = torch.Generator(device=device).manual_seed(7)
    for _ in range(100):
        env.step(torch.rand(num_envs, 12, device=device, generator=gen) * 2 - 1)
    torch.cuda.synchronize(device)
    nat, obs = env._native, env.obs_buf
    stream = torch.cuda.current_stream(device).cuda_stream
    res = {}
    for name, frac in (("mask_1pct", 0.01), ("mask_50pct", 0.5), ("mask_100pct", 1.0)):
        mask = (torch.rand(num_envs, device=device, generator=gen) < frac).to(torch.uint8)
        w = window_us(lambda: nat.quad_reset_mask(mask, obs, stream=stream), launches, samples)
        res[name] = {"masked_envs": int(mask.sum()), "window_us": w, "median_us": statistics.median(w)}
    w = window_us(lambda: nat.quad_reset_all(obs, stream=stream), launches, samples)
    res["reset_all"] = {"masked_envs": num_envs, "window_us": w, "median_us": statistics.median(w)}
    env.close()
    return {"device": torch.cuda.get_device_name(device), "n": num_envs, "launches_per_window": launches,
            "unit": "us per launch (device events around a window of back-to-back launches)",
            "kernels": {"mask_*": "k_quad<true>", "reset_all": "k_quad<false>, reset_all = 1"}, "results": res}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--num_envs", type=int, default=16384)
    p.add_argument("--launches", type=int, default=2000)
    p.add_argument("--samples", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    r = measure(a.num_envs, a.launches, a.samples)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
