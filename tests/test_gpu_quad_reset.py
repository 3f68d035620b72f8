"""AnymalCStonesEnv._reset_idx(env_ids): the masked reset of the quadruped (as_quad_reset_mask, k_quad<true>).

Expected values come from the oracle without a change to it: an env's reset reads only its own state, the seed and
its global id, so for a state S and a mask m the expectation is where(m, R, S) field by field, R being
or_quad_post_physics(reset_all = 1) on a copy of S, and where(m, obs_R, obs_before) for the observation buffer.
Every comparison is bitwise.  Sizes: 3 (less than a wave), 67 (a full 64-env workgroup and a 3-env one, tail
lanes in the last wave), 130 (three workgroups)."""

import ctypes as C

import numpy as np
import pytest
import torch

from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
from allsteps_isaaclab_amd.envs.quadruped import stand_pose

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG = AnymalCStonesEnvCfg()
SEED = 42
WARM = 30


@pytest.fixture(scope="module")
def qmodel():
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    return load_model(ANYMAL_C_JSON)


@pytest.fixture(scope="module")
def qorc(oracle_mod, qmodel):
    return oracle_mod.Oracle(cfg=CFG, model=qmodel)


@pytest.fixture(scope="module")
def structs(oracle_mod, qmodel):
    """(OrActuator, OrQuadTask) of the default cfg, as tests/test_quadruped_task.py builds them."""
    A = oracle_mod.OrActuator()
    A.mode = 1
    A.action_scale = CFG.action_scale
    A.default_q[:12] = [float(x) for x in stand_pose(qmodel["dof_names"])]
    for k, v in CFG.actuator().items():
        setattr(A, k, v)
    Q = oracle_mod.OrQuadTask()
    for k, v in CFG.quad_task().items():
        if isinstance(v, (list, tuple)):
            getattr(Q, k)[:] = v
        else:
            setattr(Q, k, v)
    return A, Q


def _env(n, offset=0, **extra):
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv

    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = SEED
    for k, v in extra.items():
        setattr(cfg, k, v)
    return AnymalCStonesEnv(cfg, env_id_offset=offset)


def _actions(n, steps, seed=7):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [(torch.rand(n, 12, device=DEV, generator=g) * 2.4 - 1.2).contiguous() for _ in range(steps)]


def _warm(env, acts=None):
    """reset, then WARM steps of random actions in [-1.2, 1.2]; every third env starts five steps from its time-out,
    so the warm-up holds in-step resets and `episode` differs between envs."""
    env.reset()
    env.state["ep_len"][::3] = env.max_episode_length - 5
    for a in (_actions(env.num_envs, WARM) if acts is None else acts):
        env.step(a)
    torch.cuda.synchronize()
    ep = env.state["episode"].cpu().numpy()
    assert ep.min() != ep.max(), "the warm-up produced no in-step reset"


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _state_np(env):
    return {k: _np(v) for k, v in env.state.items() if k != "curriculum"}


def _fill(st, S):
    for k, v in S.items():
        st[k][...] = v.reshape(st[k].shape).view(st[k].dtype)


def _expect(qorc, structs, S, obs_before, m):
    """where(m, R, S) per field and where(m, obs_R, obs_before): R = the oracle's reset of every env from S."""
    n = obs_before.shape[0]
    st = qorc.state(n)
    _fill(st, S)
    obs_r = qorc.quad_reset_all(st, *structs, seed=SEED)
    E = {}
    for k, v in S.items():
        r = st[k].view(v.dtype).reshape(v.shape)
        E[k] = np.where(m, r, v)  # (the env axis is the last one)
    return E, np.where(m[:, None], obs_r, obs_before)


def _differing(env, E):
    g = _state_np(env)
    return [k for k in E if not _same(g[k], E[k])]


def _masks(n):
    rng = np.random.default_rng(5)
    first = np.zeros(n, bool)
    first[:64] = True  # exactly the first workgroup's envs and none of the next
    one = lambda i: np.arange(n) == i  # noqa: E731
    return [("zeros", np.zeros(n, bool)), ("env 0", one(0)), ("env n-1", one(n - 1)), ("first workgroup", first),
            ("random half", rng.random(n) < 0.5), ("ones", np.ones(n, bool))]


# ------------------------------------------------------------------ 1. masks against the oracle
@pytest.mark.parametrize("contact_forces", [False, True])
@pytest.mark.parametrize("n", [3, 67, 130])
def test_masks_against_the_oracle(qorc, structs, n, contact_forces):
    env = _env(n, contact_forces=contact_forces)
    _warm(env)
    for name, m in _masks(n):
        S, obs_before = _state_np(env), _np(env.obs_buf).copy()
        cnt_before = _np(env._report.count).copy() if contact_forces else None
        term, trunc = env.reset_terminated.clone(), env.reset_time_outs.clone()
        E, obs_e = _expect(qorc, structs, S, obs_before, m)
        out = env._reset_idx(torch.as_tensor(m, device=DEV))
        torch.cuda.synchronize()
        assert out["policy"] is env.obs_buf
        bad = _differing(env, E)
        print(f"[quad reset n={n} report={contact_forces}] {name}: {int(m.sum())} envs, fields differing: {bad}")
        assert not bad, (name, bad)
        assert _same(_np(env.obs_buf), obs_e), name
        if m.any():  # the reset moved something, and the action columns of its rows are zero
            assert not _same(_np(env.obs_buf), obs_before) and not _np(env.obs_buf)[m, 52:].any(), name
        else:  # an all-zero mask leaves every state key and the observation buffer bit-identical
            assert _differing(env, S) == [] and _same(_np(env.obs_buf), obs_before)
        for k in ("contact_mask", "contact_mask_hind"):
            assert not _np(env.state[k])[:, m].any() and _same(_np(env.state[k])[:, ~m], S[k][:, ~m]), (name, k)
        if contact_forces:
            assert _same(_np(env._report.count), np.where(m, 0, cnt_before).astype(cnt_before.dtype)), name
        assert torch.equal(term, env.reset_terminated) and torch.equal(trunc, env.reset_time_outs), name
    env.close()


# ------------------------------------------------------------------ 2. all ones = env.reset(); 3. the forms
def _twins(n, k, **extra):
    """k envs in one state: the first is warmed up, the others take its state by get_state / set_state."""
    envs = [_env(n, **extra) for _ in range(k)]
    _warm(envs[0])
    saved = envs[0].get_state()
    for e in envs[1:]:
        e.reset()
        e.set_state(saved)
        e.obs_buf.copy_(envs[0].obs_buf)
    torch.cuda.synchronize()
    return envs


def _equal_envs(a, b):
    sa, sb = a.get_state(), b.get_state()
    assert sorted(sa) == sorted(sb)
    return [k for k in sa if not _same(_np(sa[k]), _np(sb[k]))] + (
        [] if _same(_np(a.obs_buf), _np(b.obs_buf)) else ["obs_buf"])


def test_all_ones_equals_reset_and_the_forms_of_env_ids():
    n = 67
    a, b, c, d, e, f = envs = _twins(n, 6)
    a._reset_idx(torch.ones(n, dtype=torch.bool, device=DEV))
    obs, _ = b.reset()
    assert obs["policy"] is b.obs_buf
    c._reset_idx(None)
    torch.cuda.synchronize()
    assert _equal_envs(a, b) == [] and _equal_envs(c, b) == []
    ids = [0, 5, 63, 64, n - 1]
    mask = torch.zeros(n, dtype=torch.bool)
    mask[ids] = True
    d._reset_idx(ids)
    e._reset_idx(torch.tensor(ids, dtype=torch.long))
    f._reset_idx(mask)
    torch.cuda.synchronize()
    assert _equal_envs(d, e) == [] and _equal_envs(d, f) == []
    assert _equal_envs(d, a) != []  # (and the subset is not the full reset)
    before = d.get_state()
    for bad in ([n], [-1], torch.tensor([0, n + 3])):
        with pytest.raises(IndexError):
            d._reset_idx(bad)
    for shape in ((n + 1,), (n - 1,), (1, n)):
        with pytest.raises(ValueError):
            d._reset_idx(torch.zeros(shape, dtype=torch.bool))
    torch.cuda.synchronize()
    after = d.get_state()
    assert all(_same(_np(before[k]), _np(after[k])) for k in before)  # a refused call changes nothing
    for x in envs:
        x.close()


# ------------------------------------------------------------------ 4. steps after the reset
def test_steps_after_a_masked_reset_stay_on_the_oracle(qorc, structs):
    n = 67
    env = _env(n)
    _warm(env)
    m = np.random.default_rng(9).random(n) < 0.5
    m[[0, 63, 64, n - 1]] = [True, False, True, True]
    E, obs_e = _expect(qorc, structs, _state_np(env), _np(env.obs_buf).copy(), m)
    env._reset_idx(torch.as_tensor(m, device=DEV))
    torch.cuda.synchronize()
    assert _differing(env, E) == [] and _same(_np(env.obs_buf), obs_e)
    st = qorc.state(n)
    _fill(st, E)
    for t, a in enumerate(_actions(n, 5, seed=13)):
        obs_g, rew_g, term_g, trunc_g, _ = env.step(a)
        torch.cuda.synchronize()
        obs_c, rew_c, term_c, trunc_c = qorc.quad_step(st, *structs, _np(a), seed=SEED, nthreads=16)
        g = _state_np(env)
        bad = [k for k in g if not _same(g[k], st[k].view(g[k].dtype).reshape(g[k].shape))]
        assert not bad, (t, bad)
        assert _same(_np(obs_g["policy"]), obs_c) and _same(_np(rew_g), rew_c), t
        assert np.array_equal(_np(term_g), term_c) and np.array_equal(_np(trunc_g), trunc_c), t
    env.close()


# ------------------------------------------------------------------ 5. graph capture
def test_captured_masked_reset_and_step_replay_equal_to_an_eager_twin():
    n = 67
    eager, ge = _twins(n, 2)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    acts = _actions(n, 5, seed=17)
    rng = np.random.default_rng(3)
    masks = [torch.as_tensor((rng.random(n) < p).astype(np.uint8), device=DEV) for p in (0.5, 0.0, 0.1, 1.0, 0.3)]
    mask, act = masks[0].clone(), acts[0].clone()
    bufs = []
    for e in (eager, ge):
        bufs.append((e.obs_buf, torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV),
                     torch.zeros(n, dtype=torch.bool, device=DEV)))

    def both(e, out, mk, a):
        e._native.quad_reset_mask(mk, out[0], stream=stream())
        e._native.quad_step(a, *out, stream=stream())

    saved = ge.get_state()
    both(ge, bufs[1], mask, act)  # warm-up, eager; then back to the common state
    ge.set_state(saved)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both(ge, bufs[1], mask, act)
    ge.set_state(saved)  # (a capture runs nothing; this only makes that plain)
    torch.cuda.synchronize()
    for k in range(5):
        mask.copy_(masks[k])  # the mask's contents change in place between replays
        act.copy_(acts[k])
        graph.replay()
        both(eager, bufs[0], masks[k], acts[k])
        torch.cuda.synchronize()
        bad = [key for key in eager.state if not _same(_np(eager.state[key]), _np(ge.state[key]))]
        assert not bad, (k, bad)
        for x, y in zip(*bufs):
            assert _same(_np(x), _np(y)), k
    eager.close(), ge.close()


# ------------------------------------------------------------------ 6. the stateful parts follow the mask
def _env_axis(t, n):
    ax = [i for i, s in enumerate(t.shape) if s == n]
    assert len(ax) == 1, tuple(t.shape)
    return ax[0]


def _follows_the_mask(got, untouched, fully_reset, m, n):
    """got == untouched on the envs outside m and == fully_reset on those inside, bit for bit."""
    ax = _env_axis(got, n)
    g, u, r = (np.moveaxis(_np(x), ax, -1) for x in (got, untouched, fully_reset))
    return _same(g[..., ~m], u[..., ~m]) and _same(g[..., m], r[..., m])


def _three(n, **extra):
    """Three envs stepped alike (the contact report is not part of get_state): reset by mask, untouched, reset whole."""
    envs = [_env(n, **extra) for _ in range(3)]
    acts = _actions(n, WARM)
    for e in envs:
        _warm(e, acts)
    return envs


def test_contact_timers_and_force_views_follow_the_mask():
    n = 67
    env, twin, whole = envs = _three(n, contact_air_time=True, contact_forces=True)
    m = np.random.default_rng(21).random(n) < 0.5
    m[[0, 64]] = True
    m[[1, n - 1]] = False
    env._reset_idx(torch.as_tensor(m, device=DEV))
    whole._reset_idx(None)
    torch.cuda.synchronize()
    for key in ("timers", "timestamp"):
        got = getattr(env._contact_timers, key)
        assert _follows_the_mask(got, getattr(twin._contact_timers, key), getattr(whole._contact_timers, key), m, n), key
        assert not np.moveaxis(_np(got), _env_axis(got, n), -1)[..., m].any(), key
    assert _np(twin._contact_timers.timers)[..., ~m].any() and _np(twin._contact_timers.timers)[..., m].any()
    view = lambda e: e.scene.sensors["contact_forces"].data.net_forces_w_history  # noqa: E731
    got, ref = view(env), view(twin)
    assert _follows_the_mask(got, ref, view(whole), m, n)
    assert not _np(got)[m].any() and _np(ref)[m].any() and _np(ref)[~m].any()
    fm = lambda e: e.sensor.data.force_matrix_w  # noqa: E731
    assert _follows_the_mask(fm(env), fm(twin), fm(whole), m, n) and not _np(fm(env))[m].any()
    for e in envs:
        e.close()


def test_action_and_observation_managers_follow_the_mask():
    from allsteps_isaaclab_amd.utils import actions as AC
    from allsteps_isaaclab_amd.utils import observations as OB

    def terms():
        g = OB.ObservationGroupCfg(enable_corruption=False)
        g.joint_pos = OB.ObservationTermCfg(func=OB.joint_pos_rel, history_length=3)
        g.actions = OB.ObservationTermCfg(func=OB.last_action)
        return {"actions": {"joint_pos": AC.JointPositionActionCfg(asset_name="robot", joint_names=[".*"],
                                                                     scale=CFG.action_scale, use_default_offset=True)},
                "observations": {"hist": g}}

    n = 67
    env, twin, whole = envs = [_env(n, **terms()) for _ in range(3)]
    acts = _actions(n, WARM)
    for e in envs:
        _warm(e, acts)
    m = np.random.default_rng(22).random(n) < 0.5
    m[[0, 64]] = True
    m[[1, n - 1]] = False
    env._reset_idx(torch.as_tensor(np.flatnonzero(m), device=DEV))
    whole._reset_idx(None)
    torch.cuda.synchronize()
    assert _follows_the_mask(env.action_manager.prev_action, twin.action_manager.prev_action,
                             whole.action_manager.prev_action, m, n)
    assert _np(twin.action_manager.prev_action)[m].any() and not _np(env.action_manager.prev_action)[m].any()
    sg, st, sw = env.get_state(), twin.get_state(), whole.get_state()
    keys = [k for k in sg if k.startswith(("action_", "observation_"))]
    assert {"action_prev_action", "action_action", "observation_count", "observation_history_hist"} <= set(keys)
    for k in keys:
        assert _follows_the_mask(sg[k], st[k], sw[k], m, n), k
    assert not _same(_np(sg["observation_count"]), _np(st["observation_count"]))  # the histories did restart
    # and the next step fills the restarted histories as a whole reset's: the masked rows equal `whole`'s
    a = _actions(n, 1, seed=23)[0]
    og, ot, ow = (e.step(a)[0]["hist"] for e in envs)
    torch.cuda.synchronize()
    assert _follows_the_mask(og, ot, ow, m, n)
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 7. global ids
def test_a_shard_resets_as_its_rows_of_the_unsharded_run():
    n, cut = 130, 66
    whole, lo, hi = _env(n), _env(cut), _env(n - cut, offset=cut)
    acts = _actions(n, WARM)
    _warm(whole, acts)
    _warm(lo, [a[:cut].contiguous() for a in acts])
    _warm(hi, [a[cut:].contiguous() for a in acts])
    m = np.random.default_rng(31).random(n) < 0.5
    m[[0, cut - 1, cut, n - 1]] = True
    for e, sl in ((whole, slice(0, n)), (lo, slice(0, cut)), (hi, slice(cut, n))):
        e._reset_idx(torch.as_tensor(m[sl], device=DEV))
    torch.cuda.synchronize()
    W = _state_np(whole)
    for e, sl in ((lo, slice(0, cut)), (hi, slice(cut, n))):
        g = _state_np(e)
        bad = [k for k in g if not _same(g[k], W[k][..., sl])]
        assert not bad, (sl, bad)
        assert _same(_np(e.obs_buf), _np(whole.obs_buf)[sl])
    # the draws are keyed by the global id: without the offset the upper shard's joint noise is another
    plain = _env(n - cut)
    _warm(plain, [a[cut:].contiguous() for a in acts])
    plain._reset_idx(torch.as_tensor(m[cut:], device=DEV))
    torch.cuda.synchronize()
    assert not _same(_np(plain.state["q"]), W["q"][..., cut:])
    for e in (whole, lo, hi, plain):
        e.close()
