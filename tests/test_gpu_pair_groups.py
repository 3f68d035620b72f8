"""collide()'s pass B on lane groups (csrc/allsteps_pair_group.h) against the oracle, bit for bit.

k_step tests a stone pair on a group of 2^L lanes, L chosen per flush from the wave's pending pairs (at
most 2: L = 4, 4: L = 3, 8: L = 2, more: one lane per pair as before); ALLSTEPS_PAIR_GROUP caps L at
as_create.  Whatever the level, the contact list is the oracle's, so 80 steps from reset with U(-1.2, 1.2)
actions -- the walkers fall and lie on the stones, which gives the pair counts that select each level --
run in lock-step with oracle/physics.c + task.c must agree in every state field, observation, reward,
done flag, contact mask and in the dropped-contact count:

  * n = 1 (the wave's second half is invalid), n = 3 (ragged grid), n = 66, at stone level 0, and n = 66 at
    level 9, each under every cap 1, 2, 3, 4;
  * n = 66 once more with the whole state written back through set_state between the steps;
  * the n = 66 runs at the default cap also read the per-wave diagnostic record (as_debug_stamps record
    mode: flushes per level) and must have used every level, the one-lane fallback included; the runs
    under a cap must not have used a level above it;
  * the quadruped (C5 task) at n = 66 with the default cap.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT_FIELDS = ("idx", "prev", "next", "count", "swing", "ep_len", "episode", "contact_mask")
FLOAT_FIELDS = ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "body_pos", "pot", "old_pot",
                "foot_contact", "stones")
STEPS = 80
REC_BASE, REC_WORDS, REC_LEVELS = 64, 30, 15 + 13  # k_step's per-wave record (kWaveRecBase / Words, kNumStamps + 13)


def _env(n, level, seed=42):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = "cuda:0"
    cfg.seed = seed
    cfg.initial_stone_curriculum = level
    return AllstepsEnv(cfg)


def _lockstep(orc, n, level, records=False, write_back=False, steps=STEPS, seed=42):
    """80 steps from reset against the oracle; returns the flushes per level [one lane, L2, L3, L4] summed
    over steps and waves (records=True), the contacts dropped and the envs seen in contact."""
    env = _env(n, level, seed)
    env.reset()
    torch.cuda.synchronize()
    st = orc.state(n)
    for k, v in env.get_state().items():
        st[k][...] = v.cpu().numpy().reshape(st[k].shape).view(st[k].dtype)
    nblk = (n + 1) // 2
    buf = None
    if records:
        buf = torch.zeros(REC_BASE + nblk * REC_WORDS, dtype=torch.int64, device="cuda:0")
        buf[31] = 1
        env._native.debug_stamps(buf)
    levels = np.zeros(4, np.int64)
    dropped = contacts = 0
    rng = np.random.default_rng(2000 + n + level)
    try:
        for t in range(steps):
            act = rng.uniform(-1.2, 1.2, (n, 21)).astype(np.float32)
            o_g, r_g, t_g, tr_g, _ = env.step(torch.from_numpy(act).cuda())
            torch.cuda.synchronize()
            o_c, r_c, t_c, tr_c, _ = orc.env_step(st, act, seed=seed, nthreads=4)
            gs = {k: v.cpu().numpy() for k, v in env.get_state().items()}
            bad = []
            for k in INT_FIELDS + FLOAT_FIELDS:
                g, c = gs[k].reshape(-1, n), st[k].reshape(-1, n)
                if k in INT_FIELDS:
                    g, c = g.view(np.uint32), c.view(np.uint32)
                if (g != c).any():
                    bad.append((k, np.flatnonzero((g != c).any(0))[:4].tolist()))
            if int(gs["curriculum"][0]) != int(st["curriculum"][0]):
                bad.append(("curriculum", []))
            if (o_g["policy"].cpu().numpy() != o_c).any():
                bad.append(("obs", np.flatnonzero((o_g["policy"].cpu().numpy() != o_c).any(1))[:4].tolist()))
            for name, g, c in (("reward", r_g, r_c), ("terminated", t_g, t_c), ("truncated", tr_g, tr_c)):
                if (g.cpu().numpy() != c).any():
                    bad.append((name, np.flatnonzero(g.cpu().numpy() != c)[:4].tolist()))
            assert not bad, f"n={n} level={level} step {t}: GPU and oracle differ in {bad}"
            d_g = env.dropped_contacts()
            assert d_g == orc.last_dropped, (t, d_g, orc.last_dropped)
            dropped += d_g
            contacts += int((st["contact_mask"] != 0).any(0).sum())
            if records:
                w = buf[REC_BASE:].view(nblk, REC_WORDS)[:, REC_LEVELS].cpu().numpy()
                levels += np.array([((w >> (8 * i)) & 0xff).sum() for i in range(4)])
            if write_back:  # the oracle's state (== the GPU's) through set_state, every field
                env.set_state({k: torch.from_numpy(st[k].view(gs[k].dtype).reshape(gs[k].shape).copy())
                               for k in gs if k != "curriculum"})
    finally:
        if records:
            env._native.debug_stamps(None)
        env.close()
    return levels, dropped, contacts


@pytest.mark.parametrize("cap", [1, 2, 3, 4])
@pytest.mark.parametrize("n,level", [(1, 0), (3, 0), (66, 0), (66, 9)])
def test_group_levels_bit_exact(orc, monkeypatch, n, level, cap):
    monkeypatch.setenv("ALLSTEPS_PAIR_GROUP", str(cap))
    levels, dropped, contacts = _lockstep(orc, n, level, records=n == 66)
    print(f"[pair groups n={n} level={level} cap={cap}] flushes one-lane / L2 / L3 / L4: {levels.tolist()}, "
          f"contacts dropped {dropped}, env-steps in contact {contacts}")
    if n == 66:
        assert contacts > 0, "no env touched a stone"
        want = [True, cap >= 2, cap >= 3, cap >= 4]
        assert [bool(x) for x in levels > 0] == want, f"levels used {levels.tolist()} under cap {cap}"


@pytest.mark.parametrize("level", [0, 9])
def test_default_cap_uses_every_level(orc, monkeypatch, level):
    """No switch set: L up to 4.  The records must show every level and the one-lane fallback."""
    monkeypatch.delenv("ALLSTEPS_PAIR_GROUP", raising=False)
    levels, dropped, contacts = _lockstep(orc, 66, level, records=True)
    print(f"[pair groups n=66 level={level} default cap] flushes one-lane / L2 / L3 / L4: {levels.tolist()}, "
          f"contacts dropped {dropped}")
    assert (levels > 0).all(), f"a level was never used: {levels.tolist()}"


def test_set_state_between_steps(orc, monkeypatch):
    monkeypatch.delenv("ALLSTEPS_PAIR_GROUP", raising=False)
    _, _, contacts = _lockstep(orc, 66, 0, write_back=True)
    assert contacts > 0


def test_switch_rejects_other_values(monkeypatch):
    from allsteps_isaaclab_amd import _native

    monkeypatch.setenv("ALLSTEPS_PAIR_GROUP", "5")
    with pytest.raises(_native.NativeError, match="ALLSTEPS_PAIR_GROUP"):
        _env(2, 0)


def test_quadruped_bit_exact(oracle_mod, monkeypatch):
    """The C5 task (ANYmal-C on the stones) at n = 66, default cap: state, observations, rewards, dones."""
    from allsteps_isaaclab_amd import registry
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.envs.quadruped import stand_pose
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    monkeypatch.delenv("ALLSTEPS_PAIR_GROUP", raising=False)
    n = 66
    qcfg, qmodel = AnymalCStonesEnvCfg(), load_model(ANYMAL_C_JSON)
    qorc = oracle_mod.Oracle(cfg=qcfg, model=qmodel)
    act = oracle_mod.OrActuator()
    act.mode = 1
    act.action_scale = qcfg.action_scale
    act.default_q[:12] = [float(x) for x in stand_pose(qmodel["dof_names"])]
    for k, v in qcfg.actuator().items():
        setattr(act, k, v)
    Q = oracle_mod.OrQuadTask()
    for k, v in qcfg.quad_task().items():
        if isinstance(v, (list, tuple)):
            getattr(Q, k)[:] = v
        else:
            setattr(Q, k, v)
    cfg = registry.load_cfg_from_registry("Allsteps-AnymalC-v0", "env_cfg_entry_point")
    cfg.scene.num_envs = n
    env = registry.make("Allsteps-AnymalC-v0", cfg=cfg)
    env.reset()
    torch.cuda.synchronize()
    st = qorc.state(n)
    for k, v in env.state.items():
        if k != "curriculum":
            st[k][...] = v.cpu().numpy().reshape(st[k].shape).view(st[k].dtype)
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    contacts = 0
    try:
        for t in range(STEPS):
            a = (torch.rand(n, 12, device="cuda:0", generator=gen) * 2.4 - 1.2).contiguous()
            obs_g, rew_g, term_g, trunc_g, _ = env.step(a)
            torch.cuda.synchronize()
            obs_c, rew_c, term_c, trunc_c = qorc.quad_step(st, act, Q, a.cpu().numpy(), seed=42, nthreads=4)
            g = {k: v.cpu().numpy() for k, v in env.state.items()}
            bad = [k for k in st.a if k != "curriculum"
                   and not np.array_equal(g[k].view(st[k].dtype).reshape(st[k].shape), st[k])]
            assert not bad, f"step {t}: state fields differ {bad}"
            np.testing.assert_array_equal(obs_g["policy"].cpu().numpy(), obs_c)
            np.testing.assert_array_equal(rew_g.cpu().numpy(), rew_c)
            assert np.array_equal(term_g.cpu().numpy(), term_c) and np.array_equal(trunc_g.cpu().numpy(), trunc_c)
            contacts += int((st["contact_mask"] != 0).any(axis=0).sum())
    finally:
        env.close()
    assert contacts > 0, "no foot touched a stone"
