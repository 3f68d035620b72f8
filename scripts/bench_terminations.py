"""Cost of the termination kernel (cfg.terminations) on one GPU, at 4096 envs, against the same terms composed from
the torch callables on the views.

The quadruped after 20 steps of random actions with the reference velocity task's terms -- time_out and
base_contact = illegal_contact on the base through the all-body contact sensor -- plus bad_orientation and
root_height_below_minimum.

  --mode kernel   `iters` launches of k_terminations_step (the contact forces are not refreshed: the launch alone)
  --mode torch    `iters` compositions: TerminationManager.compute as the reference writes it -- both buffers
                  cleared, per term the callable, ORed into its buffer and copied to the term's flags, then the union
  --mode both     the two alternating, window by window, in one process

The script times windows of back-to-back iterations with device events (launch overhead included), and profiles one
iteration of each mode with torch.profiler for the number of device kernels and their summed device time; it prints
one JSON line, and --out also writes it.  A record, not a threshold (DESIGN.md §3 "Termination manager").

    python scripts/bench_terminations.py [--mode both] [--iters 2000] [--n 4096] [--out profiles/terminations_cost.json]
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
from allsteps_isaaclab_amd.utils import terminations as TM  # noqa: E402
from allsteps_isaaclab_amd.utils.events import SceneEntityCfg  # noqa: E402

DEV = "cuda:0"


def terminations() -> dict:
    T = TM.TerminationTermCfg
    return {
        "time_out": T(func=TM.time_out, time_out=True),
        "base_contact": T(func=TM.illegal_contact,
                          params={"sensor_cfg": SceneEntityCfg("contact_forces", body_names="base"), "threshold": 1.0}),
        "bad_orientation": T(func=TM.bad_orientation, params={"limit_angle": 0.7}),
        "base_height": T(func=TM.root_height_below_minimum, params={"minimum_height": 0.3}),
    }


def make(n: int):
    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.contact_forces = True
    cfg.terminations = terminations()
    env = AnymalCStonesEnv(cfg)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(20):
        env.step(torch.rand(n, 12, device=DEV, generator=gen) * 2 - 1)
    torch.cuda.synchronize()
    return env


def torch_composition(env):
    """TerminationManager.compute by hand over the callables."""
    terms = list(env.cfg.terminations.items())
    n = env.num_envs
    truncated = torch.zeros(n, dtype=torch.bool, device=DEV)
    terminated = torch.zeros(n, dtype=torch.bool, device=DEV)
    term_dones = {k: torch.zeros(n, dtype=torch.bool, device=DEV) for k, _ in terms}

    def compose():
        truncated[:] = False
        terminated[:] = False
        for k, t in terms:
            value = t.func(env, **t.params)
            if t.time_out:
                truncated.__ior__(value)
            else:
                terminated.__ior__(value)
            term_dones[k][:] = value
        return truncated | terminated

    return compose


def kernel_launch(env):
    t = env._terminations
    env._report.forces()  # the dense net impulses, once: the launches below read them as they stand
    return lambda: t.compute(env.reset_terminated, env.reset_time_outs)


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
    """Distinct bytes one env's launch reads and writes, times n: the quaternion (4 words), the root height, the
    episode length, the net impulses of the base over the history (3 depth words); the two step flags read, and per
    term its flag written, the three unions and the reset request (bytes)."""
    terms = len(env._terminations.spec.terms)
    words = 4 + 1 + 1 + 3 * env._report.depth
    return env.num_envs * (4 * words + 2 + terms + 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("kernel", "torch", "both"), default="both")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_terminations.py measures on the HIP device; none is available")
    env = make(a.n)
    fns = {"kernel": kernel_launch(env), "torch": torch_composition(env)}
    modes = ("kernel", "torch") if a.mode == "both" else (a.mode,)
    res = {"device": torch.cuda.get_device_name(0), "n": a.n, "iters": a.iters, "terms": len(env.cfg.terminations),
           "modes": {}}
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
