"""Cost of the observation kernel (cfg.observations) on one GPU, at 4096 envs, against the same group composed from
the torch callables on the views.

The quadruped (12 joints) with the velocity task's policy group -- base_lin_vel, base_ang_vel, projected_gravity,
generated_commands, joint_pos_rel, joint_vel_rel, last_action, height_scan over 17 x 11 rays: 48 + 187 = 235 columns
-- after 20 steps of random actions, with uniform noise on as the task has it, without history and with group
history_length = 5 (1175 columns).

  --mode kernel   `iters` launches of k_observations per variant (the sensors are not refreshed: the launch alone)
  --mode torch    `iters` compositions per variant: per term the callable, torch.rand_like noise, clip, then for the
                  history variant a shift of the term's (N, 5, d) buffer, then torch.cat -- what a user writes by
                  hand without the manager
  --variant       plain | history | both

Run under ``rocprofv3 --kernel-trace --stats`` the kernel statistics give the device time; run at two values of
--iters, the difference of the summed kernel durations divided by the difference of the iterations is the device
time of one composition, whatever the set-up launched.  By itself the script times windows of back-to-back
iterations with device events (launch overhead included) and prints one JSON line; --out also writes it.  A record,
not a threshold (DESIGN.md §3 "Observation manager").

    python scripts/bench_observations.py --mode kernel [--iters 2000] [--n 4096] [--out profiles/observations_cost.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv  # noqa: E402
from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg  # noqa: E402
from allsteps_isaaclab_amd.utils import commands as CM  # noqa: E402
from allsteps_isaaclab_amd.utils import noise as NZ  # noqa: E402
from allsteps_isaaclab_amd.utils import observations as OB  # noqa: E402
from allsteps_isaaclab_amd.utils import sensors as SN  # noqa: E402
from allsteps_isaaclab_amd.utils.events import SceneEntityCfg  # noqa: E402

DEV = "cuda:0"
HISTORY = 5


def policy(history=None):
    T = OB.ObservationTermCfg
    u = lambda a: NZ.UniformNoiseCfg(n_min=-a, n_max=a)  # noqa: E731
    g = OB.ObservationGroupCfg(enable_corruption=True, history_length=history)
    g.base_lin_vel = T(func=OB.base_lin_vel, noise=u(0.1))
    g.base_ang_vel = T(func=OB.base_ang_vel, noise=u(0.2))
    g.projected_gravity = T(func=OB.projected_gravity, noise=u(0.05))
    g.velocity_commands = T(func=CM.generated_commands, params={"command_name": "base_velocity"})
    g.joint_pos = T(func=OB.joint_pos_rel, noise=u(0.01))
    g.joint_vel = T(func=OB.joint_vel_rel, noise=u(1.5))
    g.actions = T(func=OB.last_action)
    g.height_scan = T(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")}, noise=u(0.1),
                      clip=(-1.0, 1.0))
    return g


def make(n: int):
    U = CM.UniformVelocityCommandCfg
    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.commands = {"base_velocity": U(asset_name="robot", resampling_time_range=(10.0, 10.0),
                                       ranges=U.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-1.0, 1.0),
                                                       ang_vel_z=(-1.0, 1.0)))}
    cfg.height_scanner = SN.RayCasterCfg(
        prim_path="/World/envs/env_.*/Robot/base", offset=SN.RayCasterCfg.OffsetCfg(pos=(0.0, 0.0, 20.0)),
        attach_yaw_only=True, pattern_cfg=SN.patterns.GridPatternCfg(resolution=0.1, size=[1.6, 1.0]), debug_vis=False,
        mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_.*"])
    cfg.observations = {"plain": policy(), "history": policy(HISTORY)}
    env = AnymalCStonesEnv(cfg)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(20):
        env.step(torch.rand(n, 12, device=DEV, generator=gen) * 2 - 1)
    torch.cuda.synchronize()
    return env


def torch_composition(env, group, history: bool):
    """One composition by hand: the callables, noise, clip, the history shift, the concatenation."""
    names = [k for k, v in vars(group).items() if isinstance(v, OB.ObservationTermCfg)]
    terms = [getattr(group, k) for k in names]
    hist = [None] * len(terms)

    def compose():
        parts = []
        for k, t in enumerate(terms):
            v = t.func(env, **t.params)
            if t.noise is not None:
                v = v + torch.rand_like(v) * (t.noise.n_max - t.noise.n_min) + t.noise.n_min
            if t.clip:
                v = v.clip(min=t.clip[0], max=t.clip[1])
            if history:
                h = hist[k]
                h = v.unsqueeze(1).repeat(1, HISTORY, 1) if h is None else torch.cat((h[:, 1:], v.unsqueeze(1)), 1)
                hist[k] = h
                v = h.reshape(h.shape[0], -1)
            parts.append(v)
        return torch.cat(parts, dim=-1)

    return compose


def source_words(g) -> int:
    """Distinct source words one env's launch of a parsed group reads: every (source, row) a term names, the root
    quaternion for the rotated terms and the caster's height for height_scan."""
    from allsteps_isaaclab_amd import _native

    words = {(t.source, r) for t in g.terms for r in t.rows if _native.OBS_SOURCES[t.source] != "gravity"}
    if any(t.kind == _native.OBS_ROTATE_INVERSE for t in g.terms):
        words |= {(_native.OBS_SOURCES.index("root_quat"), k) for k in range(4)}
    if any(t.kind == _native.OBS_HEIGHT_SCAN for t in g.terms):
        words.add((_native.OBS_SOURCES.index("ray_pose"), 2))
    return len(words)


def window_us(fn, iters: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("kernel", "torch"), default="kernel")
    ap.add_argument("--variant", choices=("plain", "history", "both"), default="both")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_observations.py measures on the HIP device; none is available")
    env = make(a.n)
    obs = env._observations
    variants = ("plain", "history") if a.variant == "both" else (a.variant,)
    res = {"device": torch.cuda.get_device_name(0), "mode": a.mode, "n": a.n, "iters": a.iters, "variants": {}}
    for name in variants:
        k = obs.spec.names.index(name)
        g = obs.spec.groups[k]
        if a.mode == "kernel":
            fn = lambda k=k: obs.launch_group(k)  # noqa: E731
        else:
            fn = torch_composition(env, env.cfg.observations[name], name == "history")
            assert fn().shape == (a.n, g.out_cols)
        fn()
        torch.cuda.synchronize()
        us = [window_us(fn, a.iters) for _ in range(a.windows)]
        # bytes one launch moves: the source words it reads, the output it writes, the history it reads back
        src_words = source_words(g)
        nbytes = 4 * a.n * (src_words + g.out_cols + (g.out_cols - g.d0))
        res["variants"][name] = {"columns": g.out_cols, "window_us": us, "median_us": sorted(us)[len(us) // 2],
                                 "bytes_per_launch": nbytes}
    env.close()
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
