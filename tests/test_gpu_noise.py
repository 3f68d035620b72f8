"""The action / observation noise models on the device (csrc/noise_kernels.h, envs/direct_rl_env.py).

Kernel level: the reference's own outputs from injected draws (tests/golden/noise.npz) bit for bit; the
Philox path against the oracle's or_philox_block -- uniform draws bitwise, normal draws within 1e-5 of a
float64 Box-Muller (r <= sqrt(48 ln 2) ~ 5.8; the f32 angle 2 pi u carries up to 2.4e-7; cos, sin and log a
few ulp: ~3.5e-6 worst case, x3 for the device libm) and with the moments of 241,664 draws inside 5 sigma.
Env level: lock-step against a clean env, biases over resets, determinism, shards, state round trip, HIP-graph
replay and the trainer's rollout replayed from graphs against the same rollout run eagerly."""

import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _padded(n, cols):
    """(buffer, view): an (n, cols) view with NaN guard words behind it."""
    buf = torch.full((n * cols + 64,), float("nan"), device=DEV)
    return buf, buf[: n * cols].view(n, cols)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. the reference's outputs, injected draws

@pytest.fixture(scope="module")
def cases():
    from _noise_cases import load_cases

    return load_cases(DEV)


@pytest.mark.parametrize("n", [1, 3, 66])
def test_kernels_reproduce_the_reference_from_injected_draws(cases, n):
    """Every fixture case through both kernels on the first n rows: k_noise_post as the env runs it (bias
    re-draw of the masked envs from the old bias, term + bias in place, t + 1), k_noise_actions out of place
    with the bias the reference held, and the action model's bias re-draw of k_noise_post."""
    from allsteps_isaaclab_amd import _native

    for c in cases:
        st, cols = c["state"], c["cols"]
        x, draws = _cuda(c["x"][:n]), _cuda(c["draws"][:n])
        t = torch.full((n,), 7, dtype=torch.int32, device=DEV)
        if st.bias is not None:
            st.bias.zero_()
        for s, (mask, bdraw, bias, out) in enumerate(c["steps"]):
            buf, obs = _padded(n, cols)
            obs.copy_(x)
            _native.noise_post(None, st.desc, obs, t, reset=_cuda(mask[:n]), obs_draws=draws,
                               obs_bias_draws=_cuda(bdraw[:n]), stream=_stream())
            torch.cuda.synchronize()
            assert torch.equal(_bits(obs), _bits(_cuda(out[:n]))), (c["name"], s, "post")
            assert torch.isnan(buf[n * cols:]).all(), (c["name"], "wrote past the rows")
            assert torch.equal(t, torch.full_like(t, 8 + s))
            if st.bias is not None:
                assert torch.equal(_bits(st.bias[:n]), _bits(_cuda(bias[:n]))), (c["name"], s, "bias")
                assert float(st.bias[n:].abs().sum()) == 0.0, (c["name"], "bias past n")
            # the same model as an action model: out of place, the caller's tensor unchanged
            buf, o = _padded(n, cols)
            _native.noise_actions(st.desc, x, o, t, draws=draws, stream=_stream())
            torch.cuda.synchronize()
            assert torch.equal(_bits(o), _bits(_cuda(out[:n]))), (c["name"], s, "actions")
            assert torch.isnan(buf[n * cols:]).all() and torch.equal(x, _cuda(c["x"][:n]))
        if st.bias is not None:  # the action model's bias takes the same walk in k_noise_post (no obs)
            st.bias.zero_()
            for s, (mask, bdraw, bias, _) in enumerate(c["steps"]):
                _native.noise_post(st.desc, None, None, t, reset=_cuda(mask[:n]), action_bias_draws=_cuda(bdraw[:n]),
                                   stream=_stream())
                assert torch.equal(_bits(st.bias[:n]), _bits(_cuda(bias[:n]))), (c["name"], s, "action bias")


# ------------------------------------------------------------------ 2, 3. the Philox path

def _philox_uniforms(orc, seed, env0, t, cols, tag):
    """(n, 4 * ceil(cols / 4)) uniforms of the stream (seed, env0 + e, t[e], b, tag) from the oracle."""
    fn = orc.L.or_philox_block
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    nb = (cols + 3) // 4
    u = np.zeros((len(t), 4 * nb), np.float32)
    buf = (C.c_float * 4)()
    for e in range(len(t)):
        for b in range(nb):
            fn(seed, (env0 + e) & 0xFFFFFFFF, int(t[e]), b, tag, buf)
            u[e, 4 * b: 4 * b + 4] = buf[:]
    return u


def _model(term, bias=None):
    from allsteps_isaaclab_amd.utils import noise as N

    return N.NoiseModelCfg(noise_cfg=term) if bias is None else \
        N.NoiseModelWithAdditiveBiasCfg(noise_cfg=term, bias_noise_cfg=bias)


SEED, ENV0 = 0x1234_5678_9ABC_DEF1, 1000


@pytest.mark.parametrize("cols", [59, 21, 12])
@pytest.mark.parametrize("n", [1, 3, 66])
def test_philox_uniform_draws_are_the_oracles_bitwise(orc, n, cols):
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.noise import NoiseModelState
    from allsteps_isaaclab_amd.utils import noise as N

    lo, hi = -0.37, 0.81
    st = NoiseModelState(_model(N.UniformNoiseCfg(n_min=lo, n_max=hi)), n, cols, torch.device(DEV), "m")
    rng = np.random.default_rng(n * 100 + cols)
    x = rng.normal(0, 1, (n, cols)).astype(np.float32)
    t0 = (np.arange(n) * 3 + 5).astype(np.int32)
    w, lo32 = np.float32(hi - lo), np.float32(lo)
    for which, tag in (("actions", _native.NOISE_TAGS[0]), ("post", _native.NOISE_TAGS[1])):
        u = _philox_uniforms(orc, SEED, ENV0, t0, cols, tag)[:, :cols]
        want = (x + u * w) + lo32
        t = _cuda(t0)
        buf, o = _padded(n, cols)
        if which == "actions":
            _native.noise_actions(st.desc, _cuda(x), o, t, seed=SEED, env_offset=ENV0, stream=_stream())
        else:
            o.copy_(_cuda(x))
            _native.noise_post(None, st.desc, o, t, reset=torch.zeros(n, dtype=torch.uint8, device=DEV), seed=SEED,
                               env_offset=ENV0, stream=_stream())
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy().view(np.int32), want.view(np.int32)), which
        assert torch.isnan(buf[n * cols:]).all()
        assert np.array_equal(t.cpu().numpy(), t0 + (which == "post"))


def _box_muller64(u):
    u = u.astype(np.float64)
    r0, r1 = (np.sqrt(-2.0 * np.log(1.0 - u[:, k::4])) for k in (0, 2))
    a0, a1 = (2.0 * np.pi * u[:, k::4] for k in (1, 3))
    z = np.empty_like(u)
    z[:, 0::4], z[:, 1::4], z[:, 2::4], z[:, 3::4] = r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)
    return z


@pytest.mark.parametrize("cols", [59, 21, 12])
@pytest.mark.parametrize("n", [1, 3, 66])
def test_philox_gaussian_draws_within_1e5_of_float64_box_muller(orc, n, cols):
    """Unit normals (operation abs, mean 0, std 1: the output is the draw) against a float64 Box-Muller of the
    oracle's uniforms: absolute error per unit normal <= 1e-5."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.noise import NoiseModelState
    from allsteps_isaaclab_amd.utils import noise as N

    st = NoiseModelState(_model(N.GaussianNoiseCfg(operation="abs")), n, cols, torch.device(DEV), "m")
    t0 = (np.arange(n) * 7 + 1).astype(np.int32)
    t = _cuda(t0)
    obs = torch.zeros(n, cols, device=DEV)
    _native.noise_post(None, st.desc, obs, t, reset=torch.zeros(n, dtype=torch.uint8, device=DEV), seed=SEED,
                       env_offset=ENV0, stream=_stream())
    torch.cuda.synchronize()
    want = _box_muller64(_philox_uniforms(orc, SEED, ENV0, t0, cols, _native.NOISE_TAGS[1]))[:, :cols]
    err = np.abs(obs.cpu().numpy().astype(np.float64) - want).max()
    print(f"n={n} cols={cols}: max |z_device - z_float64| = {err:.3e}")
    assert err <= 1e-5


def test_philox_gaussian_moments():
    """4096 x 59 = 241,664 draws: |mean| < 5 / sqrt(N) = 0.0102, |var - 1| < 5 sqrt(2 / N) = 0.0144."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.noise import NoiseModelState
    from allsteps_isaaclab_amd.utils import noise as N

    n, cols = 4096, 59
    st = NoiseModelState(_model(N.GaussianNoiseCfg(operation="abs")), n, cols, torch.device(DEV), "m")
    t = torch.zeros(n, dtype=torch.int32, device=DEV)
    obs = torch.zeros(n, cols, device=DEV)
    _native.noise_post(None, st.desc, obs, t, reset=torch.zeros(n, dtype=torch.uint8, device=DEV), seed=42,
                       stream=_stream())
    z = obs.double()
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"mean {mean:.5f} var {var:.5f}")
    N_ = n * cols
    assert abs(mean) < 5 / math.sqrt(N_) and abs(var - 1.0) < 5 * math.sqrt(2 / N_)


# ------------------------------------------------------------------ 4 - 8. the envs

def _walker(n, obs_model=None, act_model=None, seed=42, offset=0):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.observation_noise_model, cfg.action_noise_model = obs_model, act_model
    return AllstepsEnv(cfg, env_id_offset=offset)


def _quadruped(n, obs_model=None):
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.observation_noise_model = obs_model
    return AnymalCStonesEnv(cfg)


def _actions(n, cols, steps, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.rand(n, cols, device=DEV, generator=g) * 2 - 1 for _ in range(steps)]


@pytest.mark.parametrize("make,n,cols", [(_walker, 66, 21), (_quadruped, 66, 12)], ids=["walker", "quadruped"])
def test_env_observation_constant_add(make, n, cols):
    """Observation model constant add 0.25 in lock-step with a clean env: observations are the clean ones
    plus f32 0.25 bitwise, rewards and dones identical, the observation reset() returns is not noised."""
    from allsteps_isaaclab_amd.utils import noise as N

    clean, noisy = make(n), make(n, obs_model=_model(N.ConstantNoiseCfg(bias=0.25)))
    assert noisy._noise is not None and clean._noise is None
    oc, on = clean.reset()[0]["policy"], noisy.reset()[0]["policy"]
    assert torch.equal(oc, on)
    for k, a in enumerate(_actions(n, cols, 30)):
        (oc, rc, tc, uc, _), (on, rn, tn, un, _) = clean.step(a), noisy.step(a)
        assert torch.equal(_bits(on["policy"]), _bits(oc["policy"] + 0.25)), k
        assert torch.equal(rc, rn) and torch.equal(tc, tn) and torch.equal(uc, un), k
    assert torch.equal(noisy._noise.t, torch.full((n,), 31, dtype=torch.int32, device=DEV))  # reset + 30 steps
    clean.close(), noisy.close()


def test_env_action_constant_add():
    """Action model constant add b equals a clean env fed a + b (f32) bitwise; env.actions shows the noisy
    action and the caller's tensor is untouched."""
    from allsteps_isaaclab_amd.utils import noise as N

    n, b = 66, 0.3
    clean, noisy = _walker(n), _walker(n, act_model=_model(N.ConstantNoiseCfg(bias=b)))
    clean.reset(), noisy.reset()
    for k, a in enumerate(_actions(n, 21, 10)):
        keep = a.clone()
        (oc, rc, tc, uc, _), (on, rn, tn, un, _) = clean.step(a + np.float32(b)), noisy.step(a)
        assert torch.equal(_bits(on["policy"]), _bits(oc["policy"])) and torch.equal(_bits(rc), _bits(rn)), k
        assert torch.equal(tc, tn) and torch.equal(uc, un), k
        assert torch.equal(noisy.actions, torch.clamp(a + np.float32(b), -1.0, 1.0)) and torch.equal(a, keep), k
    clean.close(), noisy.close()


def test_env_bias_lives_with_the_episode():
    """Observation model with a zero-std term and a uniform `abs` bias: obs = clean obs + bias[env], one value
    per env, unchanged while the env lives, re-drawn exactly at the steps where the env is in reset_buf;
    _reset_idx([i]) re-draws env i's alone."""
    from allsteps_isaaclab_amd.utils import noise as N

    n = 66
    model = _model(N.GaussianNoiseCfg(mean=0.0, std=0.0), N.UniformNoiseCfg(n_min=0.1, n_max=0.9, operation="abs"))
    clean, noisy = _walker(n), _walker(n, obs_model=model)
    assert float(noisy._noise.obs.bias.abs().sum()) == 0.0  # NoiseModelWithAdditiveBias starts from zeros
    clean.reset(), noisy.reset()
    bias = noisy.get_state()["noise_obs_bias"]
    assert torch.equal(bias, noisy._noise.obs.bias)
    assert bool(((bias >= 0.1) & (bias < 0.9)).all()) and len(torch.unique(bias)) == n
    resets = 0
    for k, a in enumerate(_actions(n, 21, 400)):
        (oc, _, _, _, _), (on, _, tn, un, _) = clean.step(a), noisy.step(a)
        new = noisy._noise.obs.bias.clone()
        # (d + 0) + 0 z = d + 0: the clean value (a -0 becomes +0, which the bias add cannot tell apart)
        assert torch.equal(_bits(on["policy"]), _bits((oc["policy"] + 0.0) + new[:, None])), k
        assert torch.equal(new != bias, noisy.reset_buf) and torch.equal(noisy.reset_buf, tn | un), k
        resets += int(noisy.reset_buf.sum())
        bias = new
        if resets >= 3 and k >= 20:
            break
    assert resets >= 1, "no natural reset: the test did not see a bias re-drawn by the step"
    noisy._reset_idx([5])
    new = noisy.get_state()["noise_obs_bias"]
    changed = new != bias
    assert bool(changed[5]) and int(changed.sum()) == 1
    noisy._reset_idx(None)
    assert bool((noisy.get_state()["noise_obs_bias"] != new).all())
    clean.close(), noisy.close()


def _both_models():
    from allsteps_isaaclab_amd.utils import noise as N

    obs = _model(N.GaussianNoiseCfg(mean=0.0, std=0.05), N.GaussianNoiseCfg(mean=0.0, std=0.02, operation="abs"))
    act = _model(N.UniformNoiseCfg(n_min=-0.1, n_max=0.1), N.UniformNoiseCfg(n_min=-0.05, n_max=0.05, operation="add"))
    return obs, act


def _rollout(env, acts):
    out = []
    for a in acts:
        o, r, t, u, _ = env.step(a)
        out.append((o["policy"].clone(), r.clone(), t.clone(), u.clone()))
    return out


def _same(a, b):
    return all(torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[1]), _bits(y[1]))
               and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]) for x, y in zip(a, b))


def test_env_noise_is_deterministic_and_seeded():
    n = 66
    acts = _actions(n, 21, 8)
    runs = []
    for seed in (42, 42, 43):
        obs, act = _both_models()
        env = _walker(n, obs, act, seed=seed)
        env.reset()
        runs.append(_rollout(env, acts))
        env.close()
    assert _same(runs[0], runs[1])
    assert not torch.equal(runs[0][0][0], runs[2][0][0])
    # reset(seed=...) reaches the noise stream: a seed-42 env re-seeded to 43 repeats the seed-43 run
    obs, act = _both_models()
    env = _walker(n, obs, act, seed=42)
    env.reset(seed=43)
    assert env._noise.seed == 43
    env.close()


def test_env_noise_shards_match_unsharded():
    """n = 130 whole equals shards 66 + 64 with env_id_offset: the global env id enters the Philox key."""
    n, h = 130, 66
    acts = _actions(n, 21, 12)
    envs = []
    for m, off in ((n, 0), (h, 0), (n - h, h)):
        obs, act = _both_models()
        envs.append(_walker(m, obs, act, offset=off))
        envs[-1].reset()
    full = _rollout(envs[0], acts)
    parts = [_rollout(envs[1], [a[:h] for a in acts]), _rollout(envs[2], [a[h:] for a in acts])]
    for k in range(len(acts)):
        for j in range(4):
            assert torch.equal(torch.cat([parts[0][k][j], parts[1][k][j]]), full[k][j]), (k, j)
    sf = envs[0].get_state()
    for key in ("noise_t", "noise_action_bias", "noise_obs_bias"):
        assert torch.equal(torch.cat([envs[1].get_state()[key], envs[2].get_state()[key]]), sf[key]), key
    for e in envs:
        e.close()


def test_env_state_round_trip_repeats_the_noise():
    n = 66
    obs, act = _both_models()
    env = _walker(n, obs, act)
    env.reset()
    acts = _actions(n, 21, 6)
    _rollout(env, acts[:3])
    st = env.get_state()
    assert {"noise_t", "noise_action_bias", "noise_obs_bias"} <= set(st)
    first = _rollout(env, acts[3:])
    env.set_state(st)
    assert _same(first, _rollout(env, acts[3:]))
    env.close()
    clean = _walker(n)
    assert not any(k.startswith("noise") for k in clean.get_state())
    clean.close()


def test_env_step_with_noise_replays_from_a_graph():
    """A step captured under torch.cuda.graph replays with fresh noise: three replays equal three eager steps
    of a twin env bitwise (the observation model is `abs`, so the observation IS the noise field; the action
    model's noise shows in the rewards), and the three fields differ from one another."""
    from allsteps_isaaclab_amd.utils import noise as N

    n = 66
    envs = []
    for graph in (False, True):
        _, act = _both_models()
        obs = _model(N.GaussianNoiseCfg(mean=0.0, std=1.0, operation="abs"),
                     N.UniformNoiseCfg(n_min=-0.5, n_max=0.5, operation="abs"))
        e = _walker(n, obs, act)
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(n, 21, 5)
    static = acts[0].clone()
    ge.step(static)  # warm-up, eager
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    fields = []
    for k in range(1, 4):
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        fields.append(out[0]["policy"].clone())
    assert not torch.equal(fields[0], fields[1]) and not torch.equal(fields[1], fields[2])
    assert not torch.equal(fields[0], fields[2])
    assert torch.equal(ge._noise.t, eager._noise.t)
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 9. the trainer

def _train(tmp, replay):
    """Two epochs of the trainer on a 64-env walker with a Gaussian observation model; replay False runs the
    rollout's step body (policy forward, Philox sampling, env step with its noise kernels, bookkeeping) eagerly
    every time instead of capturing and replaying it."""
    from allsteps_isaaclab_amd import registry
    from allsteps_isaaclab_amd.learning.a2c_continuous import A2CAgent
    from allsteps_isaaclab_amd.rl_games import RlGamesGpuEnv, RlGamesVecEnvWrapper, env_configurations, vecenv
    from allsteps_isaaclab_amd.utils import noise as N

    n = 64
    cfg = registry.load_cfg_from_registry("Allsteps-v0", "env_cfg_entry_point")
    cfg.scene.num_envs = n
    cfg.seed = 11
    cfg.observation_noise_model = _model(N.GaussianNoiseCfg(mean=0.0, std=0.05))
    env = RlGamesVecEnvWrapper(registry.make("Allsteps-v0", cfg=cfg), DEV, math.inf, 1.0)
    vecenv.register("IsaacRlgWrapper", lambda name, a, **kw: RlGamesGpuEnv(name, a, **kw))
    env_configurations.register("rlgpu", {"vecenv_type": "IsaacRlgWrapper", "env_creator": lambda **kw: env})
    params = registry.load_cfg_from_registry("Allsteps-v0", "rl_games_cfg_entry_point")["params"]
    params["seed"] = 11
    params["config"].update(num_actors=n, horizon_length=8, minibatch_size=n * 8, mini_epochs=2, max_epochs=2,
                            train_dir=str(tmp), print_stats=False, rollout_graphs=True)
    torch.manual_seed(11)
    agent = A2CAgent("run", params)
    if not replay:
        agent._play_step_graph = agent._play_step_body
    agent.train()
    uw = env.unwrapped
    assert uw._noise is not None and agent._play_graphs is not None
    if replay:
        assert len(agent._play_graphs) == 8
        assert all(isinstance(g, torch.cuda.CUDAGraph) for g in agent._play_graphs.values())
    else:
        assert not agent._play_graphs
    out = (agent.flat.params.clone(), uw.get_state(), agent.tensor_dict["obses"].clone(), uw.common_step_counter)
    env.close()
    return out


def test_trainer_with_observation_noise_replayed_equals_eager(tmp_path):
    """Two epochs at 64 envs, horizon 8, a Gaussian observation model, with the rollout graphs replayed (epoch
    1 eager, epoch 2 captured and replayed) and with the same rollout step run eagerly throughout: identical
    observations, parameters and state -- the replayed noise is the eager noise.

    The trainer's rollout_graphs = False switch is not the eager side here: it also swaps the policy's sampler
    (torch's generator instead of the rollout's Philox kernel), so the two settings draw different actions for
    a clean env as well and their parameters cannot be compared."""
    p0, s0, o0, c0 = _train(tmp_path / "eager", False)
    p1, s1, o1, c1 = _train(tmp_path / "graphs", True)
    assert torch.equal(o0, o1), "the rollouts' (noised) observations differ"
    assert torch.equal(p0, p1)
    for key in ("q", "qd", "root_pos", "idx", "episode", "noise_t"):
        assert torch.equal(s0[key], s1[key]), key
    assert c0 == c1 == 2 * 8
    assert int(s0["noise_t"][0]) == 1 + 2 * 8  # reset + epochs x horizon
