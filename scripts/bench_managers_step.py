"""Wall clock of env.step on the quadruped with every manager on: what the managers' host code costs per step.

The env is the one of tests/test_gpu_state_roundtrip.py (noise models, events, commands, observations, rewards,
terminations, actions, contact report and timers) at --n envs.  After --warmup steps, --windows windows of --iters
steps each are timed with time.perf_counter: `issue_us` until the last step returned (the host's share, the launches
are asynchronous), `step_us` until the device was idle.  Prints one JSON line; --out writes it to a file too.

    python scripts/bench_managers_step.py [--root OTHER_TREE] [--n 4096] [--iters 300] [--windows 5] [--out FILE]

--root: import the package from another checkout (a parent commit exported beside this one), for an A/B.
"""

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(args.root))

    import torch

    import test_gpu_state_roundtrip as T
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv

    T.N = args.n
    env = AnymalCStonesEnv(T._cfg())
    env.reset()
    g = torch.Generator(device=T.DEV).manual_seed(7)
    acts = [(torch.rand(args.n, 12, device=T.DEV, generator=g) * 2.4 - 1.2).contiguous() for _ in range(16)]
    for k in range(args.warmup):
        env.step(acts[k % 16])
    torch.cuda.synchronize()
    issue, whole = [], []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for k in range(args.iters):
            env.step(acts[k % 16])
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        issue.append((t1 - t0) / args.iters * 1e6)
        whole.append((t2 - t0) / args.iters * 1e6)
    env.close()
    res = {"root": os.path.relpath(os.path.abspath(args.root), HERE), "device": torch.cuda.get_device_name(0),
           "n": args.n, "iters": args.iters, "issue_us": issue, "step_us": whole,
           "median_issue_us": statistics.median(issue), "median_step_us": statistics.median(whole)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
