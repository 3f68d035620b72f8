"""Bit-exact HIP <-> oracle lock-step at the shapes where k_step's batched launch loads can go wrong.

k_step reads its per-lane constants from the host-built lane table (csrc/allsteps_lane_table.h), loads
every per-env word of a launch in one batch at its start -- the task epilogue's scalars included, parked
in LDS across the substeps -- and k_obs issues its loads ahead of its stores.  Every value read is the
value read before, so each case below is a == comparison with the oracle of every state field,
observation, reward, done flag and the dropped-contact counter, in the manner of test_gpu_exact._run:

  * n = 1, 3: a workgroup with an invalid half (its env index clamped to n - 1); from the spawn pose a
    robot needs a dozen steps to fall, so k_obs takes its restore path in most of the 20 launches;
  * n = 66: no wave map, a ragged last workgroup, more than one k_obs block;
  * n = 512: the smallest size with the cost-balanced wave map;
  * across the 899-step time-out with the episode counters preset to 890 + e % 9: every env resets
    inside the window, one half of a wave before the other;
  * set_state on idx / ep_len / pot between two steps: the parked scalars are re-read in every launch;
  * the quadruped (k_step<18> physics + k_quad) at n = 3 and 512, from reset and across its time-out.
"""

import numpy as np
import pytest
import torch

from test_gpu_exact import THREADS, _describe, _env, _mismatch, _to_oracle

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 66, 512)


def _step_both(env, orc, st, act, n, t, seed=42):
    """One step on the GPU and in the oracle; asserts every output equal.  Returns (terminated, truncated)."""
    o_g, r_g, t_g, tr_g, _ = env.step(torch.from_numpy(act).cuda())
    torch.cuda.synchronize()
    o_c, r_c, t_c, tr_c, _ = orc.env_step(st, act, seed=seed, nthreads=THREADS)
    gs = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    bad = _mismatch(gs, st, n)
    bad["terminated"] = np.flatnonzero(t_g.cpu().numpy() != t_c)
    bad["truncated"] = np.flatnonzero(tr_g.cpu().numpy() != tr_c)
    bad["obs"] = np.flatnonzero((o_g["policy"].cpu().numpy() != o_c).any(1))
    bad["reward"] = np.flatnonzero(r_g.cpu().numpy() != r_c)
    nbad = len(set().union(*[set(v.tolist()) for v in bad.values()]))
    d_g = env.dropped_contacts()
    print(f"[launch loads n={n}] step {t}: {nbad} of {n} envs mismatched, resets {int((t_c | tr_c).sum())}, "
          f"contacts dropped {d_g} = oracle {orc.last_dropped}")
    assert d_g == orc.last_dropped, (t, d_g, orc.last_dropped)
    assert nbad == 0, f"step {t}: {nbad} envs differ\n" + _describe(gs, st, n, bad) + "\n" + \
        "\n".join(f"  {k}: {len(v)} envs" for k, v in bad.items() if len(v))
    return t_c, tr_c


def _start(orc, n, seed=42, ep_len=None):
    env = _env(n, 0, seed)
    env.reset()
    if ep_len is not None:
        env.set_state({"ep_len": ep_len})
    torch.cuda.synchronize()
    st = orc.state(n)
    _to_oracle(env, st)
    return env, st


@pytest.mark.parametrize("n", SIZES)
def test_walker_from_reset(orc, n):
    env, st = _start(orc, n)
    rng = np.random.default_rng(2000 + n)
    quiet = 0  # launches in which no env reset: k_obs restores the tick-#1 state from the side buffer
    for t in range(20):
        t_c, tr_c = _step_both(env, orc, st, rng.uniform(-1.2, 1.2, (n, 21)).astype(np.float32), n, t)
        quiet += not (t_c | tr_c).any()
    env.close()
    if n <= 3:  # from the spawn pose a robot needs a dozen steps to fall: most launches are quiet
        assert quiet >= 10, f"only {quiet} of 20 launches took k_obs's restore path"


@pytest.mark.parametrize("n", SIZES)
def test_walker_across_time_out(orc, n):
    ep_len = (890 + torch.arange(n) % 9).to(torch.int32).reshape(1, n)
    env, st = _start(orc, n, ep_len=ep_len)
    rng = np.random.default_rng(3000 + n)
    done = np.zeros(n, bool)
    truncs = 0
    first = {}
    for t in range(12):
        t_c, tr_c = _step_both(env, orc, st, rng.uniform(-1.2, 1.2, (n, 21)).astype(np.float32), n, t)
        for e in np.flatnonzero(t_c | tr_c):
            first.setdefault(int(e), t)
        done |= t_c | tr_c
        truncs += int(tr_c.sum())
    env.close()
    assert done.all(), f"envs {np.flatnonzero(~done)[:8]} never reset inside the window"
    assert truncs > 0
    if n >= 2:  # the two envs of a wave (2 k, 2 k + 1 without a wave map) reset in different launches
        assert any(first[2 * k] != first[2 * k + 1] for k in range(n // 2))


def test_parked_scalars_are_reloaded_every_launch(orc):
    n = 66
    env, st = _start(orc, n)
    rng = np.random.default_rng(4000)
    for t in range(3):
        _step_both(env, orc, st, rng.uniform(-1.2, 1.2, (n, 21)).astype(np.float32), n, t)
    new = {"idx": np.full((1, n), 3, np.int32), "prev": np.full((1, n), 2, np.int32),
           "next": np.full((1, n), 4, np.int32), "ep_len": (100 + np.arange(n, dtype=np.int32)).reshape(1, n),
           "pot": np.full((1, n), -5.0, np.float32)}
    env.set_state({k: torch.from_numpy(v) for k, v in new.items()})
    torch.cuda.synchronize()
    for k, v in new.items():
        st[k][...] = v.reshape(st[k].shape)
    t_c, tr_c = _step_both(env, orc, st, rng.uniform(-1.2, 1.2, (n, 21)).astype(np.float32), n, 3)
    live = ~(t_c | tr_c)
    gs = env.get_state()
    assert live.any()
    # the step counted from the new episode length and kept the new target (no foot is on stone 3)
    assert (gs["ep_len"].cpu().numpy().reshape(n)[live] == (101 + np.arange(n))[live]).all()
    assert (gs["idx"].cpu().numpy().reshape(n)[live] == 3).all()
    for t in range(4, 6):
        _step_both(env, orc, st, rng.uniform(-1.2, 1.2, (n, 21)).astype(np.float32), n, t)
    env.close()


# ---- the quadruped (C5): k_step<18> in physics mode, then k_quad

@pytest.fixture(scope="module")
def quad(oracle_mod):
    import test_quadruped_task as Q
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    qmodel = load_model(ANYMAL_C_JSON)
    qorc = oracle_mod.Oracle(cfg=Q.CFG, model=qmodel)
    return qorc, Q._act_struct(oracle_mod, qmodel), Q._task_struct(oracle_mod), Q.QUAD_TASK


def _quad_lockstep(quad, n, steps, near_timeout):
    from allsteps_isaaclab_amd import registry

    qorc, act, Q, task = quad
    cfg = registry.load_cfg_from_registry("Allsteps-AnymalC-v0", "env_cfg_entry_point")
    cfg.scene.num_envs = n
    env = registry.make("Allsteps-AnymalC-v0", cfg=cfg)
    env.reset()
    if near_timeout:  # counters max - 10 .. max - 2: every env meets ep_len >= max - 1 inside 12 steps
        env.state["ep_len"][...] = (task["max_episode_length"] - 10 + torch.arange(n, device="cuda:0") % 9).to(torch.int32)
    torch.cuda.synchronize()
    st = qorc.state(n)
    for k, v in env.state.items():
        if k != "curriculum":
            st[k][...] = v.cpu().numpy().reshape(st[k].shape).view(st[k].dtype)
    gen = torch.Generator(device="cuda:0").manual_seed(11 + n)
    done = np.zeros(n, bool)
    truncs = 0
    for t in range(steps):
        a = (torch.rand(n, 12, device="cuda:0", generator=gen) * 2.4 - 1.2).contiguous()
        obs_g, rew_g, term_g, trunc_g, _ = env.step(a)
        torch.cuda.synchronize()
        obs_c, rew_c, term_c, trunc_c = qorc.quad_step(st, act, Q, a.cpu().numpy(), seed=42, nthreads=THREADS)
        g = {k: v.cpu().numpy() for k, v in env.state.items()}
        bad = [k for k in st.a if k != "curriculum"
               and not np.array_equal(g[k].view(st[k].dtype).reshape(st[k].shape), st[k])]
        print(f"[launch loads quad n={n}] step {t}: state fields that differ {bad}, resets {int((term_c | trunc_c).sum())}")
        assert not bad
        np.testing.assert_array_equal(obs_g["policy"].cpu().numpy(), obs_c)
        np.testing.assert_array_equal(rew_g.cpu().numpy(), rew_c)
        assert np.array_equal(term_g.cpu().numpy(), term_c) and np.array_equal(trunc_g.cpu().numpy(), trunc_c)
        done |= term_c | trunc_c
        truncs += int(trunc_c.sum())
    env.close()
    return done, truncs


@pytest.mark.parametrize("n", (3, 512))
def test_quadruped_from_reset(quad, n):
    _quad_lockstep(quad, n, 20, False)


@pytest.mark.parametrize("n", (3, 512))
def test_quadruped_across_time_out(quad, n):
    done, truncs = _quad_lockstep(quad, n, 12, True)
    assert done.all() and truncs > 0
