"""The action manager on the device: k_actions_process / k_actions_reset against the host restatement and the
reference's fixture, the joint-command seam of the physics step, and cfg.actions on both envs.

"Bit for bit" compares the words of the float32 values; two NaNs count as equal whichever NaN they are (an operation
that makes a NaN gives it another sign on gfx950 than on x86; tests/test_actions_host.py)."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THREADS = 256  # kActionThreads: one thread per (env, column)
GUARD = 12345.0


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """Bit for bit; two NaNs are equal."""
    a, b = torch.as_tensor(a).contiguous().cpu(), torch.as_tensor(b).contiguous().cpu()
    nan = torch.isnan(a) & torch.isnan(b) if a.dtype.is_floating_point else torch.zeros_like(a, dtype=torch.bool)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | nan).all())


def _sizes(cols):
    """One env; one block of (env, column) threads plus two envs; four blocks plus one env."""
    return [1, THREADS // cols + 2, 4 * THREADS // cols + 1]


def _guarded(n, cols):
    """(buffer, view): a float32 device tensor with 64 guard words behind it."""
    buf = torch.full((n * cols + 64,), GUARD, dtype=torch.float32, device=DEV)
    buf[: n * cols] = 0
    return buf, buf[: n * cols].view(n, cols)


def _guards_intact(*bufs):
    return all(bool((b[-64:] == GUARD).all()) for b in bufs)


@pytest.fixture(scope="module")
def cases():
    from _actions_cases import load_cases

    return load_cases()


KEYS = ("action", "prev_action", "processed", "prev_applied", "cmd")


def _device_state(n, cols, joints):
    return {k: _guarded(n, joints if k == "cmd" else cols) for k in KEYS}


def _process(rows_dev, inp, dev):
    from allsteps_isaaclab_amd import _native

    _native.actions_step(rows_dev, inp, *(dev[k][1] for k in KEYS), stream=_stream())


# ------------------------------------------------------------------ 1. the kernels against the host restatement
def test_kernels_equal_the_host_restatement(cases):
    """Every fixture case (12 and 21 columns) at n = 1, one block plus two envs and four blocks plus one env: the
    fixture's rows repeat past its 16 envs (an env depends on itself only).  Resets through one mask, two masks and
    no mask; guard words behind every buffer stay intact."""
    from _actions_cases import host_process, host_reset, zero_state
    from allsteps_isaaclab_amd import _native

    assert sorted({c["spec"].total for c in cases}) == [12, 21]
    rng = np.random.default_rng(5)
    for c in cases:
        spec, D, J = c["spec"], c["spec"].total, c["joints"]
        rows_dev = torch.as_tensor(spec.rows.copy(), device=DEV)
        for n in _sizes(D):
            pick = np.arange(n) % c["n"]
            st, dev = zero_state(n, D, J), _device_state(n, D, J)
            for s in range(c["steps"]):
                raw, jp = c["raw"][s][pick], np.ascontiguousarray(c["joint_pos"][s][pick].T)
                host_process(spec.rows, raw, st)
                _process(rows_dev, torch.from_numpy(raw).to(DEV), dev)
                torch.cuda.synchronize()
                where = (c["name"], n, s)
                for k in KEYS:
                    assert _same(dev[k][1], st[k]), (where, k)
                m1, m2 = (rng.uniform(0, 1, n) < 0.3), (rng.uniform(0, 1, n) < 0.3)
                mode = s % 4  # one mask, two masks, no reset, every env
                q = torch.from_numpy(jp).to(DEV)
                u8 = lambda m: torch.from_numpy(m.astype(np.uint8)).to(DEV)  # noqa: E731
                args = (rows_dev, dev["action"][1], dev["prev_action"][1], dev["prev_applied"][1], q)
                if mode == 0:
                    host_reset(spec.rows, st, jp, m1)
                    _native.actions_reset(*args, u8(m1), None, stream=_stream())
                elif mode == 1:
                    host_reset(spec.rows, st, jp, m1 | m2)
                    _native.actions_reset(*args, u8(m1), u8(m2), stream=_stream())
                elif mode == 3:
                    host_reset(spec.rows, st, jp, None)
                    _native.actions_reset(*args, stream=_stream())
                torch.cuda.synchronize()
                for k in KEYS:
                    assert _same(dev[k][1], st[k]), (where, k, "after the reset", mode)
                assert _guards_intact(*(b for b, _ in dev.values())), where


def test_kernels_equal_the_fixture(cases):
    """The reference's own arrays at the fixture's 16 envs: action, prev_action, processed, prev_applied, the targets
    handed to the articulation, and the state after each reset(env_ids)."""
    from allsteps_isaaclab_amd import _native

    for c in cases:
        spec, D, J, n, ref = c["spec"], c["spec"].total, c["joints"], c["n"], c["ref"]
        rows_dev = torch.as_tensor(spec.rows.copy(), device=DEV)
        dev = _device_state(n, D, J)
        for s in range(c["steps"]):
            _process(rows_dev, torch.from_numpy(c["raw"][s]).to(DEV), dev)
            torch.cuda.synchronize()
            where = (c["name"], s)
            for k in ("action", "prev_action", "processed", "prev_applied"):
                assert _same(dev[k][1], ref[k][s]), (where, k)
            assert _same(dev["action"][1], ref["raw"][s]) and _same(dev["cmd"][1], ref["targets"][s]), where
            if s in c["resets"]:
                mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
                mask[c["resets"][s]] = 1
                q = torch.from_numpy(np.ascontiguousarray(c["joint_pos"][s].T)).to(DEV)
                _native.actions_reset(rows_dev, dev["action"][1], dev["prev_action"][1], dev["prev_applied"][1], q,
                                      mask, stream=_stream())
                torch.cuda.synchronize()
            for k in ("action", "prev_action", "prev_applied"):
                assert _same(dev[k][1], ref["post_" + k][s]), (where, "post_" + k)
            assert _guards_intact(*(b for b, _ in dev.values())), where


def test_invalid_calls_are_refused_before_any_launch(cases):
    from allsteps_isaaclab_amd import _native

    c = cases[0]
    rows = torch.as_tensor(c["spec"].rows.copy(), device=DEV)
    dev = _device_state(4, 12, 12)
    inp = torch.zeros(4, 12, device=DEV)
    L = _native.load()
    p = lambda k: dev[k][1].data_ptr()  # noqa: E731
    ok = [rows.data_ptr(), 12, inp.data_ptr(), p("action"), p("prev_action"), p("processed"), p("prev_applied"),
          p("cmd"), 12, 4, _stream()]
    assert L.as_actions_step(*ok) == 0
    for at, bad, text in ((0, None, "null cols"), (1, 0, "num_cols 0 outside"), (1, 22, "num_cols 22 outside"),
                          (2, None, "null argument"), (7, None, "null argument"), (8, 0, "joint count 0 outside"),
                          (8, 22, "joint count 22 outside"), (9, 0, "n outside")):
        args = list(ok)
        args[at] = bad
        assert L.as_actions_step(*args) != 0
        assert text in L.as_last_error().decode(), (at, bad, L.as_last_error())
    q = torch.zeros(12, 4, device=DEV)
    ok = [rows.data_ptr(), 12, p("action"), p("prev_action"), p("prev_applied"), q.data_ptr(), 12, None, None, 4,
          _stream()]
    assert L.as_actions_reset(*ok) == 0
    for at, bad, text in ((0, None, "null cols"), (2, None, "null argument"), (5, None, "null argument"),
                          (6, 30, "joint count 30 outside"), (9, -1, "n outside")):
        args = list(ok)
        args[at] = bad
        assert L.as_actions_reset(*args) != 0
        assert text in L.as_last_error().decode(), (at, bad, L.as_last_error())
    assert L.as_set_joint_commands(None, None) != 0 and "null handle" in L.as_last_error().decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the envs
def _env(kind, n, seed=42, **extra):
    if kind == "walker":
        from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv as Env
        from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg as Cfg
    else:
        from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv as Env
        from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg as Cfg
    cfg = Cfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    for k, v in extra.items():
        setattr(cfg, k, v)
    return Env(cfg)


def _actions(n, cols, steps, seed=3, reach=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [(torch.rand(n, cols, device=DEV, generator=g) * 2 - 1) * reach for _ in range(steps)]


def _near_time_out(env, left=2):
    """Every third env (env 0 among them) `left` steps from its time-out: the step resets them in-kernel."""
    env.state["ep_len"][::3] = env.max_episode_length - left


STATE_KEYS = ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "body_pos", "ep_len", "idx", "contact_mask")


def _states_equal(a, b, keys=STATE_KEYS):
    return [k for k in keys if not _same(a.state[k], b.state[k])]


def _walker_gains(env):
    """float32(gain * gear) per joint in cfg dof order, as the step's prologue forms it."""
    gain = torch.as_tensor(np.float32(env.applied_gain_curriculum.cpu().numpy()[int(env.cfg.initial_stone_curriculum)]),
                           device=DEV)
    gear = torch.as_tensor(np.asarray(env.model["gear"][:21], np.float32), device=DEV)
    return gain * gear


def _hand_command(kind, env, a):
    """The command of the default path, formed as the prologue forms it."""
    c = torch.clamp(a, -1.0, 1.0)
    if kind == "walker":
        return (_walker_gains(env) * c).contiguous()
    scaled = torch.as_tensor(np.float32(env.cfg.action_scale), device=DEV) * c
    return (scaled + env.default_joint_pos.to(torch.float32)).contiguous()


# ------------------------------------------------------------------ 2. the seam
@pytest.mark.parametrize("n", [1, 3, 66])
@pytest.mark.parametrize("kind, cols", [("walker", 21), ("quadruped", 12)])
def test_seam_with_the_default_path_s_command_is_the_default_step(kind, cols, n):
    """A hand-made command buffer through as_set_joint_commands, holding what the prologue's own formula gives for the
    action: state, observation, reward and flags are bitwise those of the default step, across in-kernel resets."""
    seam, plain = _env(kind, n), _env(kind, n)
    cmd = torch.zeros(n, cols, device=DEV)
    seam._native.set_joint_commands(cmd)
    o1, _ = seam.reset()
    o2, _ = plain.reset()
    assert _same(o1["policy"], o2["policy"])
    resets = 0
    for k, a in enumerate(_actions(n, cols, 8, reach=1.3)):
        if k == 2:
            _near_time_out(seam)
            _near_time_out(plain)
        cmd.copy_(_hand_command(kind, seam, a))
        o1, r1, t1, u1, _ = seam.step(a)
        o2, r2, t2, u2, _ = plain.step(a)
        torch.cuda.synchronize()
        assert _same(o1["policy"], o2["policy"]) and _same(r1, r2), k
        assert torch.equal(t1, t2) and torch.equal(u1, u2), k
        assert _states_equal(seam, plain) == [], k
        resets += int((t1 | u1).sum())
    assert resets > 0
    # switched off again, the handle is the default one
    seam._native.set_joint_commands(None)
    cmd.fill_(float("nan"))
    a = _actions(n, cols, 1, seed=9)[0]
    o1, r1, _, _, _ = seam.step(a)
    o2, r2, _, _, _ = plain.step(a)
    torch.cuda.synchronize()
    assert _same(o1["policy"], o2["policy"]) and _same(r1, r2) and _states_equal(seam, plain) == []
    with pytest.raises(Exception, match="as_set_joint_commands: cmd must be a contiguous float32 device tensor"):
        seam._native.set_joint_commands(torch.zeros(n, cols + 1, device=DEV))
    for e in (seam, plain):
        e.close()


@pytest.mark.parametrize("n", [1, 3, 66])
def test_seam_holds_the_quadruped_s_targets_while_the_task_sees_the_raw_action(n):
    """cmd = default_q with random raw actions: the physics state is bitwise that of a default step with zero
    actions, while the observation's action columns and the action cost show the raw actions."""
    seam, zero = _env("quadruped", n), _env("quadruped", n)
    cmd = seam.default_joint_pos.to(torch.float32).unsqueeze(0).repeat(n, 1).contiguous()
    seam._native.set_joint_commands(cmd)
    seam.reset()
    zero.reset()
    differ = False
    for k, a in enumerate(_actions(n, 12, 6, reach=1.3)):
        if k == 2:
            _near_time_out(seam)
            _near_time_out(zero)
        o1, r1, t1, u1, _ = seam.step(a)
        o2, r2, t2, u2, _ = zero.step(torch.zeros_like(a))
        torch.cuda.synchronize()
        keys = ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "ep_len", "contact_mask")
        assert _states_equal(seam, zero, keys) == [], k
        assert torch.equal(t1, t2) and torch.equal(u1, u2), k
        live = ~(t1 | u1)
        assert _same(o1["policy"][:, :52], o2["policy"][:, :52]), k
        # the policy's action as k_quad shows it (clipped to +-1, as in the default step), not the held command
        assert _same(o1["policy"][live, 52:], torch.clamp(a, -1.0, 1.0)[live]), k
        assert not o1["policy"][~live, 52:].any() and not o2["policy"][:, 52:].any(), k
        differ |= bool((r1[live] != r2[live]).any())
    assert differ  # the action cost saw the raw actions
    for e in (seam, zero):
        e.close()


@pytest.mark.parametrize("n", [1, 3, 66])
def test_seam_applies_no_clamp_walker_against_the_oracle_with_scaled_gears(oracle_mod, n):
    """Commands at 1.5 times the clamp's reach -- float32(gain * float32(1.5 gear)) * a for |a| <= 1 -- through
    physics launches: the state equals the CPU oracle's on a model whose gear is scaled by 1.5 and the plain action a.
    The default path, which clamps, cannot reach these efforts."""
    from allsteps_isaaclab_amd.model import load_model

    env = _env("walker", n)
    env.reset()
    torch.cuda.synchronize()
    model = load_model()
    model15 = dict(model, gear=[float(np.float32(g) * np.float32(1.5)) for g in model["gear"]])
    orc = oracle_mod.Oracle(env.cfg, model=model15)
    st = orc.state(n)
    for k, v in env.get_state().items():
        st[k][...] = v.cpu().numpy().reshape(st[k].shape).view(st[k].dtype)
    gear15 = torch.as_tensor(np.asarray(model15["gear"][:21], np.float32), device=DEV)
    gain = torch.as_tensor(np.float32(env.applied_gain_curriculum.cpu().numpy()[int(env.cfg.initial_stone_curriculum)]),
                           device=DEV)
    cmd = torch.zeros(n, 21, device=DEV)
    env._native.set_joint_commands(cmd)
    for k, a in enumerate(_actions(n, 21, 3, seed=11)):
        cmd.copy_((gain * gear15) * a)
        assert bool((cmd.abs() > _walker_gains(env)).any())  # past what clip(a) can reach
        env.physics_step(a)
        torch.cuda.synchronize()
        orc.physics_step(st, a.cpu().numpy())
        gs = env.get_state()
        for key in ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "body_pos", "contact_mask"):
            g = gs[key].cpu().numpy().reshape(st[key].shape).view(st[key].dtype)
            assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                  st[key].view(np.uint32) if st[key].dtype == np.float32 else st[key]), (k, key)
    env.close()


# ------------------------------------------------------------------ 3. cfg.actions on the envs
def _quad_terms(env_cfg_scale=None, **kw):
    from allsteps_isaaclab_amd.utils import actions as AC

    return {"joint_pos": AC.JointPositionActionCfg(asset_name="robot", joint_names=[".*"], scale=env_cfg_scale,
                                                   use_default_offset=True, **kw)}


def test_quadruped_with_the_velocity_task_s_term_is_the_default_env_inside_the_clip():
    """JointPositionActionCfg(joint_names=[".*"], scale=action_scale, use_default_offset=True): bit for bit the default
    env's trajectory while |a| <= 1, in-kernel resets included; one action beyond 1 departs from it, where the default
    path clips and the term does not."""
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    n = 66
    scale = AnymalCStonesEnvCfg().action_scale
    env, plain = _env("quadruped", n, actions=_quad_terms(scale)), _env("quadruped", n)
    mgr = env.action_manager
    assert mgr.active_terms == ["joint_pos"] and mgr.total_action_dim == 12 and mgr.action_term_dim == [12]
    o1, _ = env.reset()
    o2, _ = plain.reset()
    assert _same(o1["policy"], o2["policy"])
    prev, seen = torch.zeros(n, 12, device=DEV), False
    for k, a in enumerate(_actions(n, 12, 8)):
        if k == 2:
            _near_time_out(env)
            _near_time_out(plain)
        launches = env._action_terms.launches
        o1, r1, t1, u1, _ = env.step(a)
        o2, r2, t2, u2, _ = plain.step(a)
        torch.cuda.synchronize()
        assert env._action_terms.launches == launches + 2, k  # process and reset: one launch each
        assert _same(o1["policy"], o2["policy"]) and _same(r1, r2), k
        assert torch.equal(t1, t2) and torch.equal(u1, u2), k
        assert _states_equal(env, plain, ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "ep_len")) == [], k
        done = t1 | u1
        assert _same(mgr.action[~done], a[~done]) and not mgr.action[done].any(), k
        assert _same(mgr.prev_action[~done], prev[~done]) and not mgr.prev_action[done].any(), k
        term = mgr.get_term("joint_pos")
        assert _same(term.raw_actions, mgr.action) and term.action_dim == 12
        want = a * torch.as_tensor(np.float32(scale), device=DEV) + env.default_joint_pos.float()
        assert _same(term.processed_actions, want) and _same(mgr.joint_commands, want), k
        prev = mgr.action.clone()
        seen |= bool(done.any())
    assert seen  # the step reset envs on the way
    a = _actions(n, 12, 1, seed=8, reach=1.6)[0]
    assert bool((a.abs() > 1).any())
    env.step(a)
    plain.step(a)
    torch.cuda.synchronize()
    assert _states_equal(env, plain, ("q", "qd")) != []
    assert mgr.get_active_iterable_terms(0)[0][0] == "joint_pos" and len(mgr.get_active_iterable_terms(0)[0][1]) == 12
    assert "<ActionManager> contains 1 active terms." in str(mgr) and mgr.reset([0]) == {}
    with pytest.raises(ValueError, match="Invalid action shape, expected: 12, received: 11."):
        mgr.process_action(torch.zeros(n, 11, device=DEV))
    for e in (env, plain):
        e.close()


def _walker_terms(env_like):
    """A JointEffortActionCfg whose per-joint dict scale is the default path's float32(gain * gear)."""
    from allsteps_isaaclab_amd.utils import actions as AC

    gains = _walker_gains(env_like).cpu().numpy()
    names = list(env_like.robot.data.joint_names)
    return {"effort": AC.JointEffortActionCfg(asset_name="robot", joint_names=[".*"],
                                              scale={n_: float(g) for n_, g in zip(names, gains)})}


def test_walker_with_an_effort_term_and_a_per_joint_scale():
    """scale[joint] = float32(gain * gear): inside the clip the env reproduces the default env bit for bit (the task's
    costs, reward and observation read the policy's action as before); beyond it the efforts are not clipped.  With an
    observation group, last_action is the manager's action: unclamped, zero for the envs the step reset; the reward
    manager's action_rate_l2 is the one of an env without cfg.actions."""
    from allsteps_isaaclab_amd.utils import observations as OB
    from allsteps_isaaclab_amd.utils import rewards as RW

    n = 66
    plain = _env("walker", n)
    terms = _walker_terms(plain)
    g = OB.ObservationGroupCfg()
    g.last_action = OB.ObservationTermCfg(func=OB.last_action)
    rewards = {"rate": RW.RewardTermCfg(func=RW.action_rate_l2, weight=-0.01)}
    env = _env("walker", n, actions=terms, observations={"obs": g}, rewards=rewards)
    twin = _env("walker", n, rewards=rewards)  # the same reward manager, no action manager
    for e in (env, plain, twin):
        e.reset()
    mgr = env.action_manager
    for k, a in enumerate(_actions(n, 21, 6)):
        if k == 2:
            for e in (env, plain, twin):
                _near_time_out(e)
        o1, r1, t1, u1, _ = env.step(a)
        o2, r2, t2, u2, _ = plain.step(a)
        twin.step(a)
        torch.cuda.synchronize()
        assert _same(o1["policy"], o2["policy"]) and _same(r1, r2), k
        assert torch.equal(t1, t2) and torch.equal(u1, u2) and _states_equal(env, plain) == [], k
        assert _same(o1["obs"], mgr.action), k
        assert _same(env._rewards.step_reward, twin._rewards.step_reward), k  # action_rate_l2 is unchanged
    # beyond the clip: the manager's action and last_action are not clamped, the efforts are not clipped
    a = _actions(n, 21, 1, seed=8, reach=1.6)[0]
    o1, _, t1, u1, _ = env.step(a)
    plain.step(a)
    torch.cuda.synchronize()
    live = ~(t1 | u1)
    assert bool((o1["obs"].abs() > 1).any()) and _same(o1["obs"][live], a[live]) and not o1["obs"][~live].any()
    assert _same(mgr.joint_commands, a * _walker_gains(env) + 0.0)
    assert _states_equal(env, plain, ("q", "qd")) != []
    for e in (env, plain, twin):
        e.close()


def _ema_terms():
    from allsteps_isaaclab_amd.utils import actions as AC

    return {"front": AC.JointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".F_.*"], scale=0.4),
            "hind": AC.EMAJointPositionToLimitsActionCfg(asset_name="robot", joint_names=[".H_.*"], scale=0.4,
                                                         alpha={".*_HAA": 0.3, ".*_HFE": 0.8, ".*_KFE": 1.0})}


def test_manager_state_after_a_step_reset_round_trip_and_hand_calls():
    """Quadruped, a to-limits term on the front legs and an EMA term on the hind legs.  After a step: action is zero
    for the envs the step reset, prev_action holds the previous action, the EMA columns' prev_applied equals joint_pos
    there and the processed action elsewhere.  get_state / set_state round-trips the manager; env.reset() resets it."""
    n = 66
    env = _env("quadruped", n, actions=_ema_terms())
    mgr, A = env.action_manager, env._action_terms
    assert mgr.active_terms == ["front", "hind"] and mgr.action_term_dim == [6, 6]
    hind = mgr.get_term("hind")
    ids = torch.as_tensor(hind._joint_ids, device=DEV)
    assert [env.robot.data.joint_names[j] for j in hind._joint_ids] == hind._joint_names
    assert all(name[1] == "H" for name in hind._joint_names)
    env.reset()
    torch.cuda.synchronize()
    assert _same(hind.prev_applied_actions, env.robot.data.joint_pos[:, ids])  # reset: the current joint positions
    assert not mgr.get_term("front").prev_applied_actions.any()
    prev = torch.zeros(n, 12, device=DEV)
    seen = False
    for k, a in enumerate(_actions(n, 12, 6, reach=1.4)):
        if k == 2:
            _near_time_out(env)
        _, _, t, u, _ = env.step(a)
        torch.cuda.synchronize()
        done = t | u
        assert _same(mgr.action[~done], a[~done]) and not mgr.action[done].any(), k
        assert _same(mgr.prev_action[~done], prev[~done]) and not mgr.prev_action[done].any(), k
        assert _same(hind.prev_applied_actions[done], env.robot.data.joint_pos[done][:, ids]), k
        assert _same(hind.prev_applied_actions[~done], hind.processed_actions[~done]), k
        assert _same(mgr.joint_commands[:, ids], hind.processed_actions), k
        lim = env.robot.data.soft_joint_pos_limits[0]
        assert bool(((mgr.joint_commands >= lim[:, 0]) & (mgr.joint_commands <= lim[:, 1])).all()), k
        prev = mgr.action.clone()
        seen |= bool(done.any())
    assert seen
    # state round trip: a twin loaded with the state takes the same next step
    twin = _env("quadruped", n, actions=_ema_terms())
    twin.reset()
    state = env.get_state()
    assert {"action_action", "action_prev_action", "action_processed", "action_prev_applied",
            "action_commands"} <= set(state)
    twin.set_state(state)
    a = _actions(n, 12, 1, seed=21)[0]
    o1, r1, _, _, _ = env.step(a)
    o2, r2, _, _, _ = twin.step(a)
    torch.cuda.synchronize()
    assert _same(o1["policy"], o2["policy"]) and _same(r1, r2)
    for key, v in A.tensors().items():
        assert _same(v, twin._action_terms.tensors()[key]), key
    # by hand: reset(env_ids) and process_action
    assert mgr.reset([0, 5]) == {}
    torch.cuda.synchronize()
    assert not mgr.action[[0, 5]].any() and bool(mgr.action.any())
    assert _same(hind.prev_applied_actions[[0, 5]], env.robot.data.joint_pos[[0, 5]][:, ids])
    mgr.process_action(a)
    mgr.apply_action()
    hind.apply_actions()
    torch.cuda.synchronize()
    assert _same(mgr.action, a)
    for e in (env, twin):
        e.close()


def test_step_with_actions_replays_from_a_graph():
    """A walker step with cfg.actions captured under torch.cuda.graph: 5 replays equal 5 eager steps of a twin bit for
    bit, the manager's buffers included."""
    n = 64
    envs = []
    for graph in (False, True):
        e = _env("walker", n)
        terms = _walker_terms(e)
        e.close()
        e = _env("walker", n, actions=terms)
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(n, 21, 7, reach=1.3)
    static = acts[0].clone()
    ge.step(static)  # warm-up, eager
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    for k in range(1, 6):
        if k == 2:
            _near_time_out(eager)
            _near_time_out(ge)
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        ge.account_steps(1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        for key, v in eager._action_terms.tensors().items():
            assert _same(v, ge._action_terms.tensors()[key]), (k, key)
    for e in envs:
        e.close()


def test_a_default_env_has_no_action_state_and_the_refusals_reach_the_constructor():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils import actions as AC

    for kind, cols in (("walker", 21), ("quadruped", 12)):
        env = _env(kind, 4)
        assert env._action_terms is None and not hasattr(env, "action_manager")
        assert not [k for k in env.get_state() if k.startswith("action_")]
        env.reset()
        n0 = env._launches
        env.step(torch.zeros(4, cols, device=DEV))
        assert env._launches == n0 + 1  # one launch of the step per step, as before
        env.close()
    pos = AC.JointPositionActionCfg(asset_name="robot", joint_names=[".*"], scale=0.5)
    eff = AC.JointEffortActionCfg(asset_name="robot", joint_names=[".*"])
    with pytest.raises(_native.NativeError, match="a joint position term needs the DC-motor actuator"):
        _env("walker", 4, actions={"p": pos})
    with pytest.raises(_native.NativeError, match="a joint effort term needs the torque actuator"):
        _env("quadruped", 4, actions={"e": eff})
    with pytest.raises(_native.NativeError, match="RelativeJointPositionActionCfg is not served"):
        _env("quadruped", 4, actions={"r": AC.RelativeJointPositionActionCfg(asset_name="robot", joint_names=[".*"])})
    with pytest.raises(_native.NativeError, match="exactly once: not commanded"):
        _env("quadruped", 4, actions={"p": AC.JointPositionActionCfg(asset_name="robot", joint_names=[".*_HAA"])})
    with pytest.raises(ValueError, match="cfg.action_space = 20 but the terms of cfg.actions take 21"):
        _env("walker", 4, actions={"e": eff}, action_space=20)
