"""Cost of the ray-caster height scanner (cfg.height_scanner) on one GPU, at 4096 and 32768 envs x 187 rays.

The quadruped (Allsteps-AnymalC-v0) with the velocity task's scanner -- 187 rays, yaw only, 20 m above the base --
cast against the ground and the stones.  Per size, one JSON field each:

  scan_us        one k_ray_cast launch: windows of back-to-back launches over the state a stepped env left, by
                 device events, the first window discarded
  torch_scan_us  the obvious alternative on the same device and state: a plain-torch (N, R, 20) broadcast slab test
                 of the same scan (same frame, surfaces and tie rules), timed the same way; its hits are compared
                 with the kernel's before any timing
  step_ms        env.step without and with a scan every step (``height_scanner.update(force_recompute=True)``), a
                 host clock around steps that end in a device synchronise, fresh envs, alternating

Prints one JSON line (DESIGN.md §3 "Ray caster").

    python scripts/bench_ray_caster.py [--sizes 4096,32768] [--steps 1000]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg, patterns  # noqa: E402

DEV = "cuda:0"
WARMUP, REPS = 50, 3


def make(n: int, scanner: bool):
    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    if scanner:
        cfg.height_scanner = RayCasterCfg(
            prim_path="/World/envs/env_.*/Robot/base", offset=RayCasterCfg.OffsetCfg(pos=(0.0, 0.0, 20.0)),
            attach_yaw_only=True, pattern_cfg=patterns.GridPatternCfg(resolution=0.1, size=[1.6, 1.0]),
            mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_.*"])
    return AnymalCStonesEnv(cfg)


def torch_scan(env, rays):
    """The scan in plain torch: hits (N, R, 3) and surface (N, R) of the yaw-attached rays against ground and stones."""
    s = env.state
    pos, q = s["root_pos"].T, s["root_quat"].T  # (N, 3), (N, 4)
    yaw = torch.atan2(2 * (q[:, 0] * q[:, 3] + q[:, 1] * q[:, 2]), 1 - 2 * (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))
    c, sn = torch.cos(yaw)[:, None], torch.sin(yaw)[:, None]
    lx, ly, lz = rays[0][None], rays[1][None], rays[2][None]
    o = torch.stack([c * lx - sn * ly, sn * lx + c * ly, lz.expand(len(pos), -1)], -1) + pos[:, None, :]  # (N, R, 3)
    d = rays[3:].T[None]  # (1, R, 3)
    inv = 1.0 / d
    centres = s["stones"].view(20, 3, -1).permute(2, 0, 1)[:, None]  # (N, 1, 20, 3)
    half = torch.tensor([0.5 * v for v in env.cfg.step_size], device=pos.device)
    oo, dd, ii = o[:, :, None, :], d[:, :, None, :], inv[:, :, None, :]
    lo, hi = centres - half, centres + half
    t1, t2 = (lo - oo) * ii, (hi - oo) * ii
    par = (dd == 0).expand_as(t1)
    inside = (oo >= lo) & (oo <= hi)
    inf = torch.full_like(t1, float("inf"))
    near = torch.where(par, torch.where(inside, -inf, inf), torch.minimum(t1, t2)).amax(-1)
    far = torch.where(par, torch.where(inside, inf, -inf), torch.maximum(t1, t2)).amin(-1)
    t = torch.where(near >= 0, near, far)
    t = torch.where((near <= far) & (far >= 0), t, torch.full_like(t, float("inf")))  # (N, R, 20)
    tg = (0.0 - o[..., 2]) * inv[..., 2]
    tg = torch.where((d[..., 2] < 0) & (tg >= 0), tg, torch.full_like(tg, float("inf")))
    tall = torch.cat([tg[..., None], t], -1)  # the ground first: argmin takes the first of equal values
    best, idx = tall.min(-1)
    hit = torch.where(torch.isfinite(best)[..., None], o + best[..., None] * d, torch.full_like(o, float("inf")))
    return hit, (idx - 1).to(torch.int8)


def events_us(fn, launches: int, windows: int = 4) -> list:
    out = []
    for w in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        if w:  # the first window warms up
            out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return out


def scans(n: int) -> dict:
    env = make(n, True)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(20):
        env.step(torch.rand(n, 12, device=DEV, generator=gen) * 2 - 1)
    s = env.height_scanner
    hits = s.data.ray_hits_w
    t_hits, t_surf = torch_scan(env, s.rays)
    torch.cuda.synchronize()
    agree = float((t_surf == s.data.ray_hit_surface).float().mean())
    err = float((t_hits - hits)[torch.isfinite(hits) & (t_surf == s.data.ray_hit_surface)[..., None]].abs().max())
    stone_share = float((s.data.ray_hit_surface >= 0).float().mean())
    kernel = events_us(lambda: s.update(0.0, force_recompute=True), 2000 if n <= 4096 else 500)
    plain = events_us(lambda: torch_scan(env, s.rays), 40 if n <= 4096 else 8)
    env.close()
    return {"scan_us": kernel, "torch_scan_us": plain, "torch_surface_agreement": agree, "torch_max_abs_diff_m": err,
            "stone_hit_share": stone_share}


def step_ms(n: int, scanner: bool, actions, steps: int) -> float:
    env = make(n, scanner)
    env.reset()
    for t in range(WARMUP):
        env.step(actions[steps + t])
        if scanner:
            env.height_scanner.update(0.0, force_recompute=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        env.step(actions[t])
        if scanner:
            env.height_scanner.update(0.0, force_recompute=True)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    env.close()
    return el * 1e3 / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096,32768")
    ap.add_argument("--steps", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_caster.py measures on the HIP device; none is available")
    out = {"rays": 187, "warmup": WARMUP, "sizes": {}}
    for n in (int(x) for x in a.sizes.split(",")):
        steps = a.steps if n <= 4096 else max(a.steps // 4, 100)
        gen = torch.Generator(device=DEV).manual_seed(1000)
        actions = torch.rand(steps + WARMUP, n, 12, device=DEV, generator=gen) * 2.0 - 1.0
        res = scans(n)
        ms = {"step": [], "step_and_scan": []}
        for _ in range(REPS):
            ms["step"].append(step_ms(n, False, actions, steps))
            ms["step_and_scan"].append(step_ms(n, True, actions, steps))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        res.update(steps=steps, step_ms=ms, median_step_ms=med,
                   scan_per_step_us=(med["step_and_scan"] - med["step"]) * 1e3)
        out["sizes"][str(n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
