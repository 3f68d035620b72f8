"""Cost of the action kernel (cfg.actions) on one GPU, at 4096 envs x 12 and x 21 columns, against the same terms
composed in torch as the reference's ActionManager.process_action + apply_action write them.

  12 columns   two terms splitting a quadruped's joints: JointPositionToLimitsActionCfg (rescale on) on the front
               legs and EMAJointPositionToLimitsActionCfg (alpha a dict) on the hind legs
  21 columns   two JointEffortActionCfg terms splitting a walker's joints, a dict scale and a clip

  --mode kernel   `iters` launches of k_actions_process
  --mode torch    `iters` compositions: prev_action / action copies, per term raw_actions, the affine map, the clamps,
                  the rescale and the moving average, and the write of the term's targets into the joint target buffer
  --mode both     the two alternating, window by window, in one process

The script times windows of back-to-back iterations with device events (launch overhead included), and profiles one
iteration of each mode with torch.profiler for the number of device kernels and their summed device time; it prints
one JSON line, and --out also writes it.  A record, not a threshold (DESIGN.md §3 "Action manager").  The kernels need
no env: the buffers are made here.

    python scripts/bench_actions.py [--mode both] [--iters 2000] [--n 4096] [--out profiles/actions_cost.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from allsteps_isaaclab_amd import _native  # noqa: E402
from allsteps_isaaclab_amd.envs.actions import (KIND_EFFORT, KIND_EMA, KIND_POSITION, ActContext,  # noqa: E402
                                                ActionTerms)
from allsteps_isaaclab_amd.utils import actions as AC  # noqa: E402

DEV = "cuda:0"
JOINTS12 = [f"{leg}_{j}" for j in ("HAA", "HFE", "KFE") for leg in ("LF", "LH", "RF", "RH")]
JOINTS21 = [f"j{k:02d}" for k in range(21)]


def specs() -> dict:
    rng = np.random.default_rng(0)

    def ctx(names, actuator):
        k = len(names)
        lim = np.stack([-1.5 + 0.4 * rng.uniform(0, 1, k), 1.0 + 0.6 * rng.uniform(0, 1, k)], -1).astype(np.float32)
        return ActContext(joint_names=names, default_joint_pos=(0.4 * rng.uniform(-1, 1, k)).astype(np.float32),
                          soft_joint_pos_limits=lim, actuator=actuator, action_space=k)

    t12 = {"front": AC.JointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".F_.*"], scale=0.9),
           "hind": AC.EMAJointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".H_.*"], scale=0.6,
                                                        alpha={".*_HAA": 0.3, ".*_HFE": 0.8, ".*_KFE": 0.55})}
    t21 = {"lower": AC.JointEffortActionCfg(asset_name="robot", joint_names=["j0.", "j1[0-4]"],
                                            scale={"j0.": 45.0, "j1.": 80.5}, offset=0.125),
           "upper": AC.JointEffortActionCfg(asset_name="robot", joint_names=["j1[5-9]", "j2."], scale=33.3,
                                            clip={"j2.": (-20.0, 25.5)})}
    return {"12": ActionTerms(t12, ctx(JOINTS12, _native.ACT_DC_MOTOR)),
            "21": ActionTerms(t21, ctx(JOINTS21, _native.ACT_TORQUE))}


class Buffers:
    def __init__(self, spec, n):
        D, J = spec.total, len(spec.ctx.joint_names)
        z = lambda c: torch.zeros(n, c, device=DEV)  # noqa: E731
        self.cols = torch.as_tensor(spec.rows.copy(), device=DEV)
        self.action, self.prev_action, self.processed, self.prev_applied, self.cmd = z(D), z(D), z(D), z(D), z(J)
        g = torch.Generator(device=DEV).manual_seed(1)
        self.inp = torch.rand(n, D, device=DEV, generator=g) * 2.6 - 1.3


def kernel_launch(b: Buffers):
    stream = torch.cuda.current_stream().cuda_stream
    return lambda: _native.actions_step(b.cols, b.inp, b.action, b.prev_action, b.processed, b.prev_applied, b.cmd,
                                        stream=stream)


def torch_composition(spec, b: Buffers, n: int):
    """ActionManager.process_action + apply_action by hand, term by term, as the reference's term classes write them."""
    rows = torch.as_tensor(spec.rows.copy(), device=DEV)
    action, prev_action = torch.zeros_like(b.action), torch.zeros_like(b.action)
    targets = torch.zeros_like(b.cmd)
    terms = []
    for t, lo in zip(spec.terms, spec.starts):
        r = rows[lo:lo + t.action_dim]
        f = lambda k: r[:, k].unsqueeze(0).repeat(n, 1)  # noqa: E731  (the reference keeps (N, dim) tensors)
        terms.append({"kind": t.kind, "sl": slice(lo, lo + t.action_dim), "ids": torch.as_tensor(t.joint_ids, device=DEV),
                      "scale": f(4), "offset": f(5), "clo": f(6), "chi": f(7), "lo": f(8), "hi": f(9), "alpha": f(10),
                      "clip": bool(np.isfinite(t.rows.view(np.float32)[:, 6:8]).any()),
                      "rescale": bool(t.rows.view(np.int32)[0, 2]), "raw": torch.zeros(n, t.action_dim, device=DEV),
                      "prev": torch.zeros(n, t.action_dim, device=DEV)})

    def compose():
        prev_action[:] = action
        action[:] = b.inp
        for t in terms:
            t["raw"][:] = b.inp[:, t["sl"]]
            if t["kind"] in (KIND_POSITION, KIND_EFFORT):
                p = t["raw"] * t["scale"] + t["offset"]
                if t["clip"]:
                    p = torch.clamp(p, min=t["clo"], max=t["chi"])
            else:
                p = t["raw"] * t["scale"]
                if t["clip"]:
                    p = torch.clamp(p, min=t["clo"], max=t["chi"])
                if t["rescale"]:
                    x = p.clamp(-1.0, 1.0)
                    p[:] = x * (t["hi"] - t["lo"]) * 0.5 + (t["lo"] + t["hi"]) * 0.5
                if t["kind"] == KIND_EMA:
                    e = t["alpha"] * p
                    e += (1.0 - t["alpha"]) * t["prev"]
                    p[:] = torch.clamp(e, t["lo"], t["hi"])
                    t["prev"][:] = p[:]
            targets[:, t["ids"]] = p
        return targets

    return compose


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("kernel", "torch", "both"), default="both")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_actions.py measures on the HIP device; none is available")
    modes = ("kernel", "torch") if a.mode == "both" else (a.mode,)
    res = {"device": torch.cuda.get_device_name(0), "n": a.n, "iters": a.iters,
           "lib": os.path.basename(_native.lib_path()), "columns": {}}
    for name, spec in specs().items():
        b = Buffers(spec, a.n)
        fns = {"kernel": kernel_launch(b), "torch": torch_composition(spec, b, a.n)}
        us = {m: [] for m in modes}
        first = {m: fns[m]() for m in modes}  # (warm-up; both start from a zero state)
        torch.cuda.synchronize()
        if a.mode == "both":  # the composition is the kernel's, to rounding (torch's device kernels may contract)
            assert torch.allclose(first["torch"], b.cmd, rtol=1e-5, atol=1e-6), name
        for _ in range(a.windows):
            for m in modes:
                us[m].append(window_us(fns[m], a.iters if m == "kernel" else max(1, a.iters // 10)))
        out = {"terms": len(spec.terms)}
        for m in modes:
            out[m] = {"window_us": us[m], "median_us": sorted(us[m])[len(us[m]) // 2], **profile_once(fns[m])}
        # distinct bytes of one launch: the input and action read, four buffers and the command written
        out["bytes_per_launch"] = 4 * a.n * (6 * spec.total + len(spec.ctx.joint_names))
        res["columns"][name] = out
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
