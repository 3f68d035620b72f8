"""Cost of the reward kernel (cfg.rewards) on one GPU, at 4096 envs, against the same terms composed from the torch
callables on the views.

The quadruped (12 joints, four feet) with the reference velocity task's RewardsCfg minus its torque term, which is
refused -- track_lin_vel_xy_exp, track_ang_vel_z_exp, lin_vel_z_l2, ang_vel_xy_l2, joint_acc_l2, action_rate_l2,
feet_air_time, undesired_contacts, flat_orientation_l2 and joint_pos_limits (the last two at weight 0 as the task has
them, so both sides skip them) -- after 20 steps of random actions.

  --mode kernel   `iters` launches of k_rewards_step (the sensors are not refreshed: the launch alone)
  --mode torch    `iters` compositions: per term of non-zero weight the callable, times weight and dt, added to the
                  total, to the term's episodic sum and written to the step buffer -- RewardManager.compute as the
                  reference writes it
  --mode both     the two alternating, window by window, in one process

The script times windows of back-to-back iterations with device events (launch overhead included), and profiles one
iteration of each mode with torch.profiler for the number of device kernels and their summed device time; it prints
one JSON line, and --out also writes it.  A record, not a threshold (DESIGN.md §3 "Reward manager").

    python scripts/bench_rewards.py [--mode both] [--iters 2000] [--n 4096] [--out profiles/rewards_cost.json]
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
from allsteps_isaaclab_amd.utils import rewards as RW  # noqa: E402
from allsteps_isaaclab_amd.utils.events import SceneEntityCfg  # noqa: E402

DEV = "cuda:0"


def rewards() -> dict:
    T = RW.RewardTermCfg
    feet, cmd = SceneEntityCfg("sensor"), {"command_name": "base_velocity"}
    return {
        "track_lin_vel_xy_exp": T(func=RW.track_lin_vel_xy_exp, weight=1.0, params={"std": 0.25 ** 0.5, **cmd}),
        "track_ang_vel_z_exp": T(func=RW.track_ang_vel_z_exp, weight=0.5, params={"std": 0.25 ** 0.5, **cmd}),
        "lin_vel_z_l2": T(func=RW.lin_vel_z_l2, weight=-2.0),
        "ang_vel_xy_l2": T(func=RW.ang_vel_xy_l2, weight=-0.05),
        "dof_acc_l2": T(func=RW.joint_acc_l2, weight=-2.5e-7),
        "action_rate_l2": T(func=RW.action_rate_l2, weight=-0.01),
        "feet_air_time": T(func=RW.feet_air_time, weight=0.125, params={"sensor_cfg": feet, "threshold": 0.5, **cmd}),
        "undesired_contacts": T(func=RW.undesired_contacts, weight=-1.0, params={"sensor_cfg": feet, "threshold": 1.0}),
        "flat_orientation_l2": T(func=RW.flat_orientation_l2, weight=0.0),
        "dof_pos_limits": T(func=RW.joint_pos_limits, weight=0.0),
    }


def make(n: int):
    U = CM.UniformVelocityCommandCfg
    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.commands = {"base_velocity": U(asset_name="robot", resampling_time_range=(10.0, 10.0),
                                       ranges=U.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-1.0, 1.0),
                                                       ang_vel_z=(-1.0, 1.0)))}
    cfg.contact_forces = cfg.contact_air_time = True
    cfg.rewards = rewards()
    env = AnymalCStonesEnv(cfg)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(20):
        env.step(torch.rand(n, 12, device=DEV, generator=gen) * 2 - 1)
    torch.cuda.synchronize()
    return env


def torch_composition(env):
    """RewardManager.compute by hand over the callables."""
    terms = list(env.cfg.rewards.items())
    n = env.num_envs
    total = torch.zeros(n, device=DEV)
    sums = {k: torch.zeros(n, device=DEV) for k, _ in terms}
    step = torch.zeros(n, len(terms), device=DEV)
    dt = env.step_dt

    def compose():
        total[:] = 0.0
        for i, (k, t) in enumerate(terms):
            if t.weight == 0.0:
                continue
            value = t.func(env, **t.params) * t.weight * dt
            total.add_(value)
            sums[k] += value
            step[:, i] = value / dt
        return total

    return compose


def kernel_launch(env):
    r = env._rewards
    env._report.forces()  # the dense net impulses, once: the launches below read them as they stand
    return lambda: r.compute(env.step_dt)


def window_us(fn, iters: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def profile_once(fn) -> dict:
    """Device kernels of one iteration and their summed device time (us), or nulls where the profiler is not there."""
    try:
        from torch.profiler import ProfilerActivity, profile

        reps = 20
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return {"kernels": len(ev) / reps, "device_us": sum(e.device_time for e in ev) / reps}
    except Exception as e:  # noqa: BLE001
        return {"kernels": None, "device_us": None, "profiler": repr(e)[:200]}


def bytes_per_launch(env) -> int:
    """Distinct words one env's launch reads and writes, times 4 n: the root state (13), qd and qd_prev, the actions
    and prev_actions read and prev_actions written, the command (3), the timers' two rows and the net impulses of the
    four feet, the flags; per live term the episodic sum read and written and the step value, and the reward."""
    spec = env._rewards.spec
    live = sum(1 for t in spec.terms if t.weight != 0)
    A = env._rewards.prev_actions.shape[1]
    nd = int(env.model["num_hinges"])
    feet, depth = env.sensor.num_bodies, env._report.depth
    words = 13 + 2 * nd + 3 * A + 3 + 2 * feet + depth * feet * 3 + 1 + 3 * live + 1
    return 4 * env.num_envs * words


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("kernel", "torch", "both"), default="both")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rewards.py measures on the HIP device; none is available")
    env = make(a.n)
    fns = {"kernel": kernel_launch(env), "torch": torch_composition(env)}
    modes = ("kernel", "torch") if a.mode == "both" else (a.mode,)
    res = {"device": torch.cuda.get_device_name(0), "n": a.n, "iters": a.iters, "terms": len(env.cfg.rewards),
           "live_terms": sum(1 for t in env.cfg.rewards.values() if t.weight != 0), "modes": {}}
    us = {m: [] for m in modes}
    for m in modes:
        fns[m]()
    torch.cuda.synchronize()
    for _ in range(a.windows):
        for m in modes:
            us[m].append(window_us(fns[m], a.iters if m == "kernel" else max(1, a.iters // 10)))
    for m in modes:
        res["modes"][m] = {"window_us": us[m], "median_us": sorted(us[m])[len(us[m]) // 2], **profile_once(fns[m])}
    res["bytes_per_launch"] = bytes_per_launch(env)
    env.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
