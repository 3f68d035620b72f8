"""The reward manager on the device (k_rewards_step / k_rewards_reset, cfg.rewards): the kernel against the host
restatement of csrc/allsteps_rewards.h (tests/_rewards_cases.py, which tests/test_rewards_host.py holds equal to the
header and, under its rules, to the reference's fixture), the reset kernel, and the envs -- the step unchanged, the
manager's buffers against a host replay, the torch callables of utils/rewards.py on the views, the replaced task
reward, HIP-graph replay with a live set_term_cfg, state round trip and the default path."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W = 64, 8  # kRewEnvs: envs per block; kRewWaves: waves per block
SIZES = [1, B + 2, 4 * B + 1]


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """Bit for bit; two NaNs are equal."""
    a, b = torch.as_tensor(a).contiguous().cpu(), torch.as_tensor(b).contiguous().cpu()
    nan = torch.isnan(a) & torch.isnan(b)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | nan).all())


def _rows(a, n, axis=-1):
    """The first n envs of an array; past the fixture's 66 the envs repeat (an env depends on itself only)."""
    return np.ascontiguousarray(np.take(a, np.arange(n) % a.shape[axis], axis=axis))


GUARD = 12345.0


def _guarded(shape, fill=0.0):
    """(buffer, view): a device tensor with 64 guard words behind it."""
    size = int(np.prod(shape))
    buf = torch.full((size + 64,), GUARD, dtype=torch.float32, device=DEV)
    buf[:size] = fill
    return buf, buf[:size].view(shape)


def _guards_intact(*bufs):
    return all(bool((b[-64:] == GUARD).all()) for b in bufs)


@pytest.fixture(scope="module")
def cases():
    """The fixture's cases a, b, c, c1 (1 term), and on case a's inputs a list of W + 1 terms (one wave takes two)
    and one of AS_MAX_REW_TERMS."""
    from _rewards_cases import context, load_cases, load_fixture, term_cfgs
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.rewards import RewardTerms

    z, meta = load_fixture()
    loaded = {c["name"]: c for c in load_cases()}
    a = loaded["a"]
    ctx = context(z, meta, next(c for c in meta["cases"] if c["name"] == "a"))
    pick = [t for t in a["terms"] if t["name"] in ("alive", "jvel_l2", "jlim", "act_rate", "undesired", "forces", "air",
                                                     "biped", "track_lin")]
    more = a["terms"] + [dict(t, name=t["name"] + "_2", weight=t["weight"] * -0.75) for t in a["terms"][:11]]
    assert len(pick) == W + 1 and len(more) == _native.MAX_REW_TERMS
    out = [loaded[k] for k in ("a", "b", "c", "c1")]
    for name, terms in (("nine", pick), ("max", more)):
        spec = RewardTerms(term_cfgs(terms), ctx)
        out.append(dict(a, name=name, terms=terms, names=[t["name"] for t in terms], steps=4, specs=[spec] * 4))
    return out


def _device_inputs(c, s, n):
    x = {k: _rows(v[s], n, axis=0 if k == "actions" else -1) for k, v in c["inputs"].items()}
    return x, {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}


# ------------------------------------------------------------------ 1. the kernel against the host restatement
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_host_restatement(orc, cases, n):
    from _rewards_cases import host_step, oracle_exp, zero_state
    from allsteps_isaaclab_amd import _native

    exp = oracle_exp(orc)
    for c in cases:
        T, A = len(c["names"]), c["inputs"]["actions"].shape[2]
        state = zero_state(T, n, A)
        rb, reward = _guarded((n,), 7.0)
        sb, sums = _guarded((T, n))
        pb, step = _guarded((T, n))
        lb, last = _guarded((T, n))
        ab, prev = _guarded((n, A))
        for s in range(c["steps"]):
            spec = c["specs"][s]
            x, t = _device_inputs(c, s, n)
            done = _rows(c["reset"][s], n)
            want, state, _ = host_step(spec, x, state, done, c["dt"], c["sim_dt"], exp)
            src = _native.make_reward_sources(t, c["sim_dt"])
            desc, table = (torch.as_tensor(spec.rows.copy(), device=DEV), torch.as_tensor(spec.table.copy(), device=DEV))
            # the dones split over the two masks, as the step's terminated / truncated
            d = torch.from_numpy(done).to(DEV)
            r1, r2 = d * (torch.arange(n, device=DEV) % 2 == 0), d * (torch.arange(n, device=DEV) % 2 == 1)
            _native.rewards_step(desc, table, spec.kinds, src, reward, sums, step, last, prev,
                                 reset=r1.to(torch.uint8), reset2=r2.to(torch.uint8), dt=c["dt"], stream=_stream())
            torch.cuda.synchronize()
            where = (c["name"], n, s)
            assert _same(reward, want), where
            assert _same(sums, state["episode_sums"]), where
            assert _same(step, state["step_reward"]), where
            assert _same(last, state["last_episode_sums"]), where
            assert _same(prev, state["prev_actions"]), where
            assert _guards_intact(rb, sb, pb, lb, ab), where


# ------------------------------------------------------------------ 2. the reset kernel
def test_reset_kernel_clears_the_masked_envs_only():
    from allsteps_isaaclab_amd import _native

    n, T, A = 4 * B + 1, 5, 12
    sb, sums = _guarded((T, n), 1.5)
    ab, prev = _guarded((n, A), 2.5)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[[0, 63, 64, n - 1]] = 1
    _native.rewards_reset(sums, prev, mask=mask, stream=_stream())
    torch.cuda.synchronize()
    m = mask.bool()
    assert bool((sums[:, m] == 0).all()) and bool((sums[:, ~m] == 1.5).all())
    assert bool((prev[m] == 0).all()) and bool((prev[~m] == 2.5).all())
    # no prev_actions: only the sums; no mask: every env
    _native.rewards_reset(sums, None, mask=None, stream=_stream())
    torch.cuda.synchronize()
    assert bool((sums == 0).all()) and bool((prev[~m] == 2.5).all()) and _guards_intact(sb, ab)


def test_optional_outputs_are_not_written_and_invalid_calls_are_refused(cases):
    from allsteps_isaaclab_amd import _native

    c = next(k for k in cases if k["name"] == "c1")
    n, spec = 66, c["specs"][0]
    _, t = _device_inputs(c, 0, n)
    src = _native.make_reward_sources(t, c["sim_dt"])
    desc, table = torch.as_tensor(spec.rows.copy(), device=DEV), torch.as_tensor(spec.table.copy(), device=DEV)
    rb, reward = _guarded((n,))
    sb, sums = _guarded((1, n))
    pb, step = _guarded((1, n))
    _native.rewards_step(desc, table, spec.kinds, src, reward, sums, step, None, None, dt=0.02, stream=_stream())
    torch.cuda.synchronize()
    assert _guards_intact(rb, sb, pb) and bool((step[0, 3:] != 0).any())
    rate = 1 << _native.REW_KINDS.index("action_rate_l2")
    with pytest.raises(_native.NativeError, match="prev_actions"):  # an action-rate term without prev_actions
        _native.rewards_step(desc, table, rate, src, reward, sums, step, None, None, dt=0.02, stream=_stream())
    t2 = dict(t, qd=None)
    with pytest.raises(_native.NativeError, match="q / qd"):  # a term whose source is NULL
        _native.rewards_step(desc, table, spec.kinds, _native.make_reward_sources(t2, c["sim_dt"]), reward, sums,
                             step, dt=0.02, stream=_stream())
    ab, prev = _guarded((n, 12))
    with pytest.raises(_native.NativeError, match="prev_actions without actions"):
        _native.rewards_step(desc, table, spec.kinds, _native.make_reward_sources(dict(t, actions=None), c["sim_dt"]),
                             reward, sums, step, None, prev, dt=0.02, stream=_stream())
    with pytest.raises(_native.NativeError, match="dt"):
        _native.rewards_step(desc, table, spec.kinds, src, reward, sums, step, dt=0.0, stream=_stream())


# ------------------------------------------------------------------ 3. the envs
def _commands():
    from allsteps_isaaclab_amd.utils.commands import UniformVelocityCommandCfg as U

    return {"base_velocity": U(asset_name="robot", resampling_time_range=(0.02, 0.05), rel_standing_envs=0.2,
                               ranges=U.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), ang_vel_z=(-1.0, 1.0)))}


def _rewards():
    from allsteps_isaaclab_amd.utils import rewards as RW
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    T = RW.RewardTermCfg
    feet, cmd = SceneEntityCfg("sensor"), {"command_name": "base_velocity"}
    return {
        "alive": T(func=RW.is_alive, weight=0.5), "terminated": T(func=RW.is_terminated, weight=-200.0),
        "lin_vel_z": T(func=RW.lin_vel_z_l2, weight=-2.0), "ang_vel_xy": T(func=RW.ang_vel_xy_l2, weight=-0.05),
        "flat": T(func=RW.flat_orientation_l2, weight=-5.0),
        "height": T(func=RW.base_height_l2, weight=-1.5, params={"target_height": 0.6}),
        "jvel_l1": T(func=RW.joint_vel_l1, weight=-0.01, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[3])}),
        "jvel_l2": T(func=RW.joint_vel_l2, weight=-0.001),
        "jdev": T(func=RW.joint_deviation_l1, weight=-0.1,
                  params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[0, 2, 5, 7, 11])}),
        "jlim": T(func=RW.joint_pos_limits, weight=-1.0), "jacc": T(func=RW.joint_acc_l2, weight=-2.5e-7),
        "act": T(func=RW.action_l2, weight=-0.01), "act_rate": T(func=RW.action_rate_l2, weight=-0.01),
        "undesired": T(func=RW.undesired_contacts, weight=-1.0, params={"threshold": 1.0, "sensor_cfg": feet}),
        "forces": T(func=RW.contact_forces, weight=-0.001, params={"threshold": 5.0, "sensor_cfg": feet}),
        "air": T(func=RW.feet_air_time, weight=0.125, params={"threshold": 0.05, "sensor_cfg": feet, **cmd}),
        "biped": T(func=RW.feet_air_time_positive_biped, weight=0.25,
                   params={"threshold": 0.1, "sensor_cfg": feet, **cmd}),
        "track_lin": T(func=RW.track_lin_vel_xy_exp, weight=1.0, params={"std": 2.0, **cmd}),
        "track_ang": T(func=RW.track_ang_vel_z_exp, weight=0.5, params={"std": 2.0, **cmd}),
        "track_world": T(func=RW.track_ang_vel_z_world_exp, weight=0.5, params={"std": 2.0, **cmd}),
        "track_yaw": T(func=RW.track_lin_vel_xy_yaw_frame_exp, weight=0.75, params={"std": 2.0, **cmd}),
    }


def _env(kind, n, rewards=None, replace=False, seed=42):
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
    if rewards is not None:
        cfg.rewards, cfg.rewards_replace_task_reward = rewards, replace
        cfg.commands, cfg.contact_forces, cfg.contact_air_time = _commands(), True, True
    return Env(cfg)


def _actions(n, cols, steps, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.rand(n, cols, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(steps)]


def _host_inputs(env):
    """The rows the kernel read in the last step, as numpy in the layout of _rewards_cases."""
    t = env._rewards_sources(net=True)
    x = {k: v.detach().cpu().numpy().copy() for k, v in t.items() if v is not None}
    x["terminated"] = env.reset_terminated.cpu().numpy().astype(np.uint8)
    return x


def _host_state(env):
    r = env._rewards
    return {"episode_sums": r.episode_sums.cpu().numpy().copy(), "step_reward": r.step_reward.cpu().numpy().copy(),
            "last_episode_sums": r.last_episode_sums.cpu().numpy().copy(),
            "prev_actions": r.prev_actions.cpu().numpy().copy()}


# The torch callables of utils/rewards.py on the views, evaluated on the device, against the kernel's term values
# (the host replay's, which the kernel equals bit for bit):
#   EXACT      elementwise float32 operations, comparisons, minima and sums of one element on the same bits: bit for
#              bit.
#   the rest   the case-b rule of tests/test_rewards_host.py: over all steps and envs, the kernel's max abs error
#              against the callable evaluated in float64 (_view64: the same views cast to float64) is at most twice the
#              float32 callable's own, exact where that is 0.  These are the reductions (another association of the same
#              addends) and the base-frame terms: the device's torch.cross and torch.bmm do not round as the
#              reference's CPU kernels do, which the kernel follows, so quat_rotate_inverse is not the same bits there
#              (measured below: the share of words that differ).
#   base frame in addition, the kernel's formula downstream of the rotation on the view's own root_*_vel_b /
#              projected_gravity_b bits is the callable bit for bit (the squares) or within 3 ulp (the exp terms:
#              as_expf's 2 plus the device exp's 1; + 2^-126, below which as_expf gives +0): a wrong sign or a swapped
#              component cannot hide in a rounding bound.
#   exp        the case-b rule is asked of the argument; the value is within 3 ulp (+ 2^-126) of the device's exp of the
#              kernel's own argument.
#   yaw frame  its argument goes through the library's atan2 / sincos: argument and value against float64 under
#              _rewards_cases.yaw_frame_bounds, as on the host.
EXACT = ("alive", "terminated", "height", "jvel_l1", "undesired", "biped")
SQUARES = {"lin_vel_z": ("root_lin_vel_b", (2,)), "ang_vel_xy": ("root_ang_vel_b", (0, 1)),
           "flat": ("projected_gravity_b", (0, 1))}
EXPS = ("track_lin", "track_ang", "track_world")


def _view64(env, prev):
    """What the callables read of an env, cast to float64 (the base-frame quantities and joint_acc formed in
    float64 from the cast rows, as the views form them in float32)."""
    from types import SimpleNamespace as NS

    f64 = lambda t: t.to(torch.float64)  # noqa: E731
    d, rep, dt = env.robot.data, env._report, env.cfg.sim.dt
    q = f64(d.root_quat_w)
    D = NS(joint_names=d.joint_names, _rotate_inverse=d._rotate_inverse, root_quat_w=q, root_pos_w=f64(d.root_pos_w),
           root_lin_vel_w=f64(d.root_lin_vel_w), root_ang_vel_w=f64(d.root_ang_vel_w), joint_pos=f64(d.joint_pos),
           joint_vel=f64(d.joint_vel), default_joint_pos=f64(d.default_joint_pos),
           soft_joint_pos_limits=f64(d.soft_joint_pos_limits))
    D.root_lin_vel_b, D.root_ang_vel_b = d._rotate_inverse(q, D.root_lin_vel_w), d._rotate_inverse(q, D.root_ang_vel_w)
    g = torch.tensor((0.0, 0.0, -1.0), dtype=torch.float64, device=q.device).repeat(q.shape[0], 1)
    D.projected_gravity_b = d._rotate_inverse(q, g)
    D.joint_acc = (D.joint_vel - f64(rep.qd_prev[: D.joint_vel.shape[1]].T)) / dt
    sd = env.sensor.data
    net = rep.forces()[1][:, [rep.foot_body[f] for f in env.sensor._feet]].permute(3, 0, 1, 2)
    S = NS(body_names=env.sensor.body_names,
           data=NS(net_forces_w_history=f64(net) / dt, last_air_time=f64(sd.last_air_time),
                   current_air_time=f64(sd.current_air_time), current_contact_time=f64(sd.current_contact_time)))
    S.compute_first_contact = lambda step_dt, abs_tol=1.0e-8: ((S.data.current_contact_time > 0.0)
                                                               * (S.data.current_contact_time < (step_dt + abs_tol)))
    return NS(robot=NS(data=D), sensor=S, scene=NS(sensors={}), reset_terminated=env.reset_terminated,
              actions=f64(env.actions), reward_manager=NS(prev_actions=f64(prev)), step_dt=env.step_dt,
              command_manager=NS(get_command=lambda name: f64(env.command_manager.get_command(name))))


def _exp_argument(view, name, t):
    """The argument of an exp term's callable, in the view's precision."""
    d, cmd = view.robot.data, view.command_manager.get_command(t.params["command_name"])
    if name == "track_lin":
        e = torch.sum(torch.square(cmd[:, :2] - d.root_lin_vel_b[:, :2]), dim=1)
    else:
        e = torch.square(cmd[:, 2] - (d.root_ang_vel_b if name == "track_ang" else d.root_ang_vel_w)[:, 2])
    return -e / t.params["std"] ** 2


def _ulps(a, b):
    """|a - b| in units of the last place (float32 tensors of one sign)."""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


class _Errors:
    """Per term, the largest |value - float64| of the kernel and of the float32 callable, over the steps."""

    def __init__(self):
        self.kernel, self.torch, self.differ = {}, {}, {}

    def add(self, name, got, want32, want64):
        self.kernel[name] = max(self.kernel.get(name, 0.0), float((got.double() - want64).abs().max()))
        self.torch[name] = max(self.torch.get(name, 0.0), float((want32.double() - want64).abs().max()))
        a, b = self.differ.get(name, (0, 0))
        self.differ[name] = (a + int((_bits(got) != _bits(want32)).sum()), b + got.numel())

    def check(self):
        for name, ek in self.kernel.items():
            et = self.torch[name]
            assert ek <= 2.0 * et, (name, ek, et)

    def __str__(self):
        return ", ".join(f"{k} {self.kernel[k] / self.torch[k] if self.torch[k] else 0.0:.2f} "
                         f"({self.differ[k][0]}/{self.differ[k][1]} words differ)" for k in self.kernel)


def _against_torch(env, cfgs, names, got, args, prev, x, exp, errors, k):
    """got: the kernel's term values of the step; args: its exp terms' arguments by term index; prev: prev_actions
    as the launch read them; x: the rows the launch read (numpy)."""
    from _rewards_cases import yaw_frame_bounds, yaw_frame_f64

    v64 = _view64(env, prev)
    d = env.robot.data
    floor = 2.0 ** -126
    for i, name in enumerate(names):
        t = cfgs[name]
        want = t.func(env, **t.params).float()
        g = got[i]
        if name in EXACT:
            assert _same(g, want), (k, name)
            continue
        if name == "track_yaw":
            row, std = env._rewards.spec.terms[i].cmd_row, t.params["std"]
            arg64, val64 = yaw_frame_f64(x, row, std)
            darg, dval = yaw_frame_bounds(x, row, std)
            assert (np.abs(args[i].astype(np.float64) - arg64) <= darg).all(), (k, name)
            assert (np.abs(g.cpu().numpy().astype(np.float64) - val64) <= dval).all(), (k, name)
            assert (np.abs(want.cpu().numpy().astype(np.float64) - val64) <= dval).all(), (k, name)
            continue
        if name in EXPS:
            a = torch.from_numpy(args[i]).to(DEV)
            errors.add(name + " argument", a, _exp_argument(env, name, t).float(), _exp_argument(v64, name, t))
            assert bool(((g - torch.exp(a)).abs() <= 3 * 2.0 ** -23 * g + floor).all()), (k, name)
            # the formula downstream of the rotation, on the view's own bits
            mine = torch.from_numpy(exp(_exp_argument(env, name, t).float().cpu().numpy())).to(DEV)
            assert bool(((mine - want).abs() <= 3 * 2.0 ** -23 * want + floor).all()), (k, name)
            continue
        errors.add(name, g, want, t.func(v64, **t.params).double())
        if name in SQUARES:
            src, cols = SQUARES[name]
            o = getattr(d, src)
            mine = o[:, cols[0]] * o[:, cols[0]]
            for c in cols[1:]:
                mine = mine + o[:, c] * o[:, c]
            assert _same(mine, want), (k, name)


@pytest.mark.parametrize("kind,cols", [("walker", 21), ("quadruped", 12)])
def test_env_steps_unchanged_and_the_manager_follows_the_host_replay(orc, kind, cols):
    from _rewards_cases import host_step, oracle_exp, term_values
    from allsteps_isaaclab_amd.envs.views import RewardManagerView

    n, steps = 64, 16
    cfgs = _rewards()
    env, clean = _env(kind, n, cfgs), _env(kind, n)
    m = env.reward_manager
    assert isinstance(m, RewardManagerView) and m.active_terms == list(cfgs) and "Active Reward Terms" in str(m)
    exp = oracle_exp(orc)
    o0, _ = env.reset()
    c0, _ = clean.reset()
    assert torch.equal(_bits(o0["policy"]), _bits(c0["policy"]))
    resets = 0
    errors = _Errors()
    for k, a in enumerate(_actions(n, cols, steps)):
        state = _host_state(env)
        prev_before = env._rewards.prev_actions.clone()
        launches = env._rewards.launches
        o, r, te, tr, _ = env.step(a)
        oc, rc, tec, trc, _ = clean.step(a)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o["policy"]), _bits(oc["policy"])) and torch.equal(_bits(r), _bits(rc)), k
        assert torch.equal(te, tec) and torch.equal(tr, trc), k
        assert env._rewards.launches == launches + 1, k
        done = (te | tr).cpu().numpy()
        resets += int(done.sum())
        spec = env._rewards.spec
        x = _host_inputs(env)
        want, state, fv = host_step(spec, x, state, done, env.step_dt, env.physics_dt, exp,
                                    clamp=env._actions_clamped)
        assert _same(m.reward_buf, want), k
        for key, have in state.items():
            assert _same(getattr(env._rewards, key), have), (k, key)
        assert m._step_reward.shape == (n, len(cfgs)) and m._episode_sums["alive"].shape == (n,)
        # the torch callables on the views against the kernel's term values; action_rate_l2 read the previous
        # step's prev_actions, which the launch has since replaced
        vals = [torch.from_numpy(fv[i]).to(DEV) for i in range(len(cfgs))]
        args = {}
        term_values(spec, x, prev_before.cpu().numpy(), env.physics_dt, exp, env._actions_clamped, exp_args=args)
        prev_now = env._rewards.prev_actions.clone()
        env._rewards.prev_actions.copy_(prev_before)
        _against_torch(env, cfgs, list(cfgs), vals, args, prev_before, x, exp, errors, k)
        env._rewards.prev_actions.copy_(prev_now)
    print(f"{kind}: {resets} env resets in {steps} steps; max abs error against float64, kernel / torch callable on "
          f"the device: {errors}")
    errors.check()
    assert resets > 0 or kind != "walker"  # (the quadruped stands through 16 random steps)
    before = env._rewards.episode_sums.clone()
    extras = m.reset([0, 5])
    torch.cuda.synchronize()
    assert set(extras) == {f"Episode_Reward/{name}" for name in cfgs}
    assert bool((env._rewards.episode_sums[:, [0, 5]] == 0).all()) and bool((env._rewards.prev_actions[[0, 5]] == 0).all())
    keep = [e for e in range(n) if e not in (0, 5)]
    assert _same(env._rewards.episode_sums[:, keep], before[:, keep]) and bool((before[0] != 0).any())
    want = float(before[0, [0, 5]].mean() / env.max_episode_length_s)
    assert abs(extras["Episode_Reward/alive"] - want) <= 1e-6 * max(1.0, abs(want))
    for e in (env, clean):
        e.close()


def test_replaced_task_reward_is_the_managers_buffer():
    n = 64
    cfgs = _rewards()
    env, twin = _env("quadruped", n, cfgs, replace=True), _env("quadruped", n, cfgs)
    env.reset()
    twin.reset()
    for a in _actions(n, 12, 3):
        o, r, te, tr, _ = env.step(a)
        o2, r2, te2, tr2, _ = twin.step(a)
        torch.cuda.synchronize()
        assert r is env.reward_manager.reward_buf and _same(r, twin.reward_manager.reward_buf)
        assert not _same(r, r2) and _same(env.reward_buf, r2)  # the task's own reward is still computed
        assert torch.equal(te, te2) and torch.equal(tr, tr2) and _same(o["policy"], o2["policy"])
    for e in (env, twin):
        e.close()


def test_env_step_replays_from_a_graph_with_a_live_weight_change():
    """A step captured under torch.cuda.graph replays: 6 replays equal 6 eager steps of a twin env bit for bit; a
    weight set to 0 after the capture skips the term in the replays that follow, and set back it counts again."""
    from allsteps_isaaclab_amd.utils import rewards as RW

    n = 64
    envs = []
    for graph in (False, True):
        e = _env("walker", n, _rewards())
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(n, 21, 8)
    static = acts[0].clone()
    ge.step(static)  # warm-up, eager
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    k_alive = ge.reward_manager.active_terms.index("alive")
    frozen = None
    for k in range(1, 7):
        if k in (3, 5):
            new = RW.RewardTermCfg(func=RW.is_alive, weight=0.0 if k == 3 else 2.0)
            for e in envs:
                e.reward_manager.set_term_cfg("alive", new)
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        ge.account_steps(1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        for key, v in eager._rewards.tensors().items():
            assert _same(v, ge._rewards.tensors()[key]), (k, key)
        assert _same(eager.reward_manager.reward_buf, ge.reward_manager.reward_buf), k
        step = ge.reward_manager._step_reward[:, k_alive].clone()
        if k == 2:
            frozen = step
        if k in (3, 4):  # skipped: the entry stays as the last launch that computed it left it
            assert _same(step, frozen), k
        if k >= 5:
            alive = (~out[2]).float() * 2.0
            assert _same(step, alive), k
    for e in envs:
        e.close()


def test_state_round_trip_and_compute_by_hand():
    n = 64
    env = _env("quadruped", n, _rewards())
    env.reset()
    acts = _actions(n, 12, 6)
    for a in acts[:2]:
        env.step(a)
    state = env.get_state()
    keys = {"reward_episode_sums", "reward_step", "reward_last_episode_sums", "reward_prev_actions"}
    assert keys <= set(state)
    first = []
    for a in acts[2:5]:
        env.step(a)
        first.append({k: v.clone() for k, v in env._rewards.tensors().items()} | {"r": env.reward_manager.reward_buf.clone()})
    env.set_state(state)
    for a, want in zip(acts[2:5], first):
        env.step(a)
        torch.cuda.synchronize()
        for k, v in env._rewards.tensors().items():
            assert _same(v, want[k]), k
        assert _same(env.reward_manager.reward_buf, want["r"])
    # compute(dt) by hand: one more launch on the state as it stands, no env done; the sums grow by the values
    before = env._rewards.episode_sums.clone()
    buf = env.reward_manager.compute(env.step_dt)
    torch.cuda.synchronize()
    assert buf is env.reward_manager.reward_buf
    grown = env._rewards.episode_sums - before
    assert bool((grown[0] >= 0).all()) and bool((grown[0] > 0).any())  # alive
    terms = env.reward_manager.get_active_iterable_terms(3)
    assert [t[0] for t in terms] == env.reward_manager.active_terms and len(terms[0][1]) == 1
    assert env.reward_manager.get_term_cfg("act").func.__name__ == "action_l2"
    # a cfg with another term function is refused: the sources a launch is given follow the kinds
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils import rewards as RW

    with pytest.raises(_native.NativeError, match="changes the term's function from action_l2 to action_rate_l2"):
        env.reward_manager.set_term_cfg("act", RW.RewardTermCfg(func=RW.action_rate_l2, weight=-0.01))
    env.reward_manager.set_term_cfg("act", RW.RewardTermCfg(func=RW.action_l2, weight=-0.02))
    assert env.reward_manager.get_term_cfg("act").weight == -0.02
    env.close()


def test_a_default_env_has_no_reward_state():
    for kind, cols in (("walker", 21), ("quadruped", 12)):
        clean = _env(kind, 4)
        assert clean._rewards is None and not hasattr(clean, "reward_manager")
        clean.reset()
        launches = clean._launches
        clean.step(_actions(4, cols, 1)[0])
        assert clean._launches == launches + 1
        assert not any(k.startswith("reward_") for k in clean.get_state())
        clean.close()


def test_env_refuses_a_term_whose_sensor_the_cfg_lacks():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    for field in ("contact_forces", "contact_air_time", "commands"):
        cfg = AllstepsEnvCfg()
        cfg.scene.num_envs = 4
        cfg.sim.device = DEV
        cfg.rewards = _rewards()
        cfg.commands, cfg.contact_forces, cfg.contact_air_time = _commands(), True, True
        setattr(cfg, field, None if field == "commands" else False)
        if field == "contact_forces":  # (the timers bring the report: the forces are then there as well)
            cfg.contact_air_time = False
            match = "cfg.contact"
        else:
            match = "cfg." + field
        with pytest.raises(_native.NativeError, match=match):
            AllstepsEnv(cfg)
