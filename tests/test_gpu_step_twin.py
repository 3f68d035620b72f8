"""k_step against its diagnostic twin k_step_diag, bit for bit, and the twin's stamps.

The phase stamps of as_debug_stamps are compiled into k_step_diag alone (csrc/step_lanes.h Stamp<kOn>,
csrc/allsteps_kernels.hip step_body<NV, SKIP, kDiag>); launch_step runs the twin exactly when a stamp buffer is
set.  Both are one body, so two envs from the same seed and actions -- one plain, one with a stamp buffer --
must agree after every step in every state field, observation row, reward, terminated, truncated, the step
counters and dropped_contacts() (torch.equal / ==), while the twin's buffer fills:

  * walker, n = 66, 12 steps: ragged grid, an invalid half-wave, no wave map; aggregate mode.  The per-phase
    sums over the 33 waves are all non-zero; slot 15 holds the slowest wave's total and slots 16.. the
    per-phase maxima, so the sums add up to at least that total and at most 33 times it, and the maxima to at
    least it;
  * walker, n = 512, 8 steps: the smallest size with a wave map; per-wave record mode.  Every one of the 256
    records is written in every launch: start < end on both clocks, its phases add up to its recorded total
    exactly, its rows lie in [3 x contacts, substeps x AS_MAX_ROWS] per env and a launch's records differ from
    the launch before (the cost word of the side buffer, which holds the same row count for the next launch's
    placement, stays on the device: the C ABI has no call that reads it);
  * walker, n = 2, 10 steps with max_episode_length = 6: both envs time out and are reset inside the kernel,
    and again; aggregate mode on one wave, the buffer cleared per launch, so the fifteen phase sums add up to
    the recorded total exactly;
  * quadruped (Allsteps-AnymalC-v0), n = 66, 8 steps: each a k_step<18> physics launch and the task epilogue
    of k_quad; aggregate mode.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NP = 15  # kNumStamps
REC_FLAG, REC_BASE, REC_WORDS = 31, 64, 30  # kWaveRecFlag / kWaveRecBase / kWaveRecWords
MAX_ROWS, MAX_CONTACTS = 30, 10  # AS_MAX_ROWS, AS_MAX_CONTACTS


def _walker(n, seed=42, episode_steps=None):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.seed = seed
    if episode_steps is not None:
        cfg.episode_length_s = (episode_steps - 0.5) * cfg.sim.dt * cfg.decimation
        assert cfg.max_episode_length == episode_steps
    env = AllstepsEnv(cfg)
    env.reset()
    return env


def _quadruped(n):
    from allsteps_isaaclab_amd import registry

    cfg = registry.load_cfg_from_registry("Allsteps-AnymalC-v0", "env_cfg_entry_point")
    cfg.scene.num_envs = n
    env = registry.make("Allsteps-AnymalC-v0", cfg=cfg)
    env.reset()
    return env


def _stamp_buffer(n, records):
    buf = torch.zeros(REC_BASE + ((n + 1) // 2) * REC_WORDS, dtype=torch.int64, device="cuda:0")
    if records:
        buf[REC_FLAG] = 1
    return buf


def _state(env):
    return env.get_state() if hasattr(env, "get_state") else env.state


def _assert_same(plain, twin, out_p, out_t, t):
    """Every output of step t and the whole state, plain == twin."""
    torch.cuda.synchronize()
    sp, st = _state(plain), _state(twin)
    assert sp.keys() == st.keys()
    bad = [k for k in sp if not torch.equal(sp[k], st[k])]
    for name, a, b in (("obs", out_p[0]["policy"], out_t[0]["policy"]), ("reward", out_p[1], out_t[1]),
                       ("terminated", out_p[2], out_t[2]), ("truncated", out_p[3], out_t[3])):
        if not torch.equal(a, b):
            bad.append(name)
    cp, ct = plain._native.counters_host(), twin._native.counters_host()
    if cp != ct:
        bad.append(f"counters {cp} != {ct}")
    assert not bad, f"step {t}: k_step and k_step_diag differ in {bad}"
    if hasattr(plain, "dropped_contacts"):
        assert plain.dropped_contacts() == twin.dropped_contacts()


def _lockstep(plain, twin, buf, steps, dof, seed, after_launch=None, clear=False):
    """`steps` steps of both envs from the same actions; the twin's launches write `buf`."""
    twin._native.debug_stamps(buf)
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    resets = 0
    try:
        for t in range(steps):
            a = (torch.rand(plain.num_envs, dof, device="cuda:0", generator=gen) * 2.4 - 1.2).contiguous()
            if clear:
                buf[:REC_FLAG].zero_()
            out_p = plain.step(a)
            out_t = twin.step(a)
            _assert_same(plain, twin, out_p, out_t, t)
            resets += int((out_p[2].bool() | out_p[3].bool()).sum())
            if after_launch is not None:
                after_launch(t, out_t)
    finally:
        twin._native.debug_stamps(None)
        plain.close()
        twin.close()
    return resets


def _check_aggregate(buf, waves):
    w = buf[:REC_FLAG].cpu().numpy()
    sums, slowest, maxima = w[:NP], int(w[NP]), w[16:16 + NP]
    print(f"[step twin] phase sums {sums.tolist()} slowest wave {slowest} phase maxima {maxima.tolist()}")
    assert (sums > 0).all(), sums
    assert slowest > 0 and (maxima > 0).all() and (maxima <= sums).all()
    assert slowest <= int(sums.sum()) <= waves * slowest
    assert int(maxima.sum()) >= slowest
    return sums, slowest


def test_walker_aggregate_stamps():
    n = 66
    buf = _stamp_buffer(n, records=False)
    _lockstep(_walker(n), _walker(n), buf, 12, 21, seed=66)
    _check_aggregate(buf, 12 * ((n + 1) // 2))  # (summed over the 12 launches; the maxima are over all of them)


def test_walker_wave_records():
    n, steps = 512, 8
    buf = _stamp_buffer(n, records=True)
    nblk = n // 2
    seen = []

    def check(t, out):
        r = buf[REC_BASE:].view(nblk, REC_WORDS).cpu().numpy().astype(np.int64)
        assert (r[:, :NP] > 0).all(), f"launch {t}: records {np.flatnonzero((r[:, :NP] <= 0).any(1))[:8]} not written"
        assert (r[:, :NP].sum(1) == r[:, NP]).all()
        assert (r[:, NP + 1] < r[:, NP + 2]).all() and (r[:, NP + 9] < r[:, NP + 10]).all()
        rows, cons = r[:, NP + 5:NP + 7], r[:, NP + 7:NP + 9]
        substeps = 4
        assert (cons >= 0).all() and (cons <= substeps * MAX_CONTACTS).all()
        assert (rows >= 3 * cons).all() and (rows <= substeps * MAX_ROWS).all()
        if seen:  # (on the 100 MHz clock the CUs share: s_memtime counts each CU's own)
            assert (r[:, NP + 9] >= seen[-1][:, NP + 10].max()).all(), "a record of the launch before"
        seen.append(r)

    plain, twin = _walker(n), _walker(n)
    assert twin.cfg.decimation == 4
    _lockstep(plain, twin, buf, steps, 21, seed=512, after_launch=check)
    assert len(seen) == steps and sum(int(r[:, NP + 5:NP + 7].sum()) for r in seen) > 0


def test_walker_reset_path_across_time_out():
    n = 2
    buf = _stamp_buffer(n, records=False)
    truncs = []

    def check(t, out):
        truncs.append(int(out[3].sum()))
        sums, slowest = _check_aggregate(buf, 1)
        assert int(sums.sum()) == slowest  # one wave, the buffer cleared before the launch

    resets = _lockstep(_walker(n, episode_steps=6), _walker(n, episode_steps=6), buf, 10, 21, seed=2,
                       after_launch=check, clear=True)
    assert sum(truncs) >= 2 and resets >= 2, (truncs, resets)


def test_quadruped_aggregate_stamps():
    n = 66
    buf = _stamp_buffer(n, records=False)
    _lockstep(_quadruped(n), _quadruped(n), buf, 8, 12, seed=18)
    # a physics launch has no task, reset or observation phase of its own, but every mark still lands
    _check_aggregate(buf, 8 * ((n + 1) // 2))
