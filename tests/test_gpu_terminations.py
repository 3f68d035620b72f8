"""The termination manager on the device (k_terminations_step, cfg.terminations): the kernel against the host
restatement of csrc/allsteps_terminations.h (tests/_terminations_cases.py, which tests/test_terminations_host.py holds
equal to the header and to the reference's fixture), and the envs -- the step unchanged without terminations_reset, the
manager's flags against the torch callables of utils/terminations.py on the views, HIP-graph replay with a live
set_term_cfg, the walker's terminations_reset, state round trip, the all-body contact sensor and the default path."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, W = 64, 4  # kTermEnvs: envs per block; kTermWaves: waves per block
SIZES = [1, B + 2, 4 * B + 1]
GUARD = 0xA5


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """Bit for bit; two NaNs are equal."""
    a, b = torch.as_tensor(a).contiguous().cpu(), torch.as_tensor(b).contiguous().cpu()
    nan = torch.isnan(a) & torch.isnan(b) if a.dtype.is_floating_point else torch.zeros_like(a, dtype=torch.bool)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | nan).all())


def _rows(a, n, axis=-1):
    """The first n envs of an array; past the fixture's 66 the envs repeat (an env depends on itself only)."""
    return np.ascontiguousarray(np.take(a, np.arange(n) % a.shape[axis], axis=axis))


def _guarded(shape, fill=0):
    """(buffer, view): a uint8 device tensor with 64 guard bytes behind it."""
    size = int(np.prod(shape))
    buf = torch.full((size + 64,), GUARD, dtype=torch.uint8, device=DEV)
    buf[:size] = fill
    return buf, buf[:size].view(shape)


def _guards_intact(*bufs):
    return all(bool((b[-64:] == GUARD).all()) for b in bufs)


@pytest.fixture(scope="module")
def cases():
    """The fixture's cases a, b, c (nine terms: with four waves a block, wave 0 takes three and the others two), and
    on case a's inputs a list of one term and one of AS_MAX_TERMINATION_TERMS."""
    from _terminations_cases import context, load_cases, load_fixture, term_cfgs
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.terminations import TerminationTerms

    z, meta = load_fixture()
    loaded = {c["name"]: c for c in load_cases()}
    a = loaded["a"]
    assert W < len(a["names"]) < 3 * W  # some wave takes more terms than another
    ctx = context(z, meta, next(c for c in meta["cases"] if c["name"] == "a"))
    one = [t for t in a["terms"] if t["name"] == "contact_all"]
    more = a["terms"] + [dict(t, name=t["name"] + "_2", time_out=not t["time_out"]) for t in a["terms"][:7]]
    assert len(more) == _native.MAX_TERMINATION_TERMS
    out = [loaded[k] for k in ("a", "b", "c")]
    for name, terms in (("one", one), ("max", more)):
        spec = TerminationTerms(term_cfgs(terms), ctx)
        out.append(dict(a, name=name, terms=terms, names=[t["name"] for t in terms], steps=4, specs=[spec] * 4))
    return out


def _device_inputs(c, s, n):
    x = {k: _rows(v[s], n) for k, v in c["inputs"].items()}
    return x, {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}


# ------------------------------------------------------------------ 1. the kernel against the host restatement
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_host_restatement(orc, cases, n):
    from _terminations_cases import BUFFERS, host_step, oracle_atan2, zero_state
    from allsteps_isaaclab_amd import _native

    atan2 = oracle_atan2(orc)
    rng = np.random.default_rng(11)
    assert [len(c["names"]) for c in cases] == [9, 9, 9, 1, 16]
    for c in cases:
        T = len(c["names"])
        state = zero_state(T, n)
        bufs = {k: _guarded((T, n) if k in ("term_dones", "last_episode_dones") else (n,), 7) for k in BUFFERS}
        bufs["last_episode_dones"][1].zero_()
        for s in range(c["steps"]):
            spec = c["specs"][s]
            x, t = _device_inputs(c, s, n)
            # the step's own flags: none in the first step (NULL pointers), then a seventh of the envs each
            flags = {} if s == 0 else {k: (rng.uniform(0, 1, n) < 0.15).astype(np.uint8)
                                       for k in ("step_terminated", "step_truncated")}
            state = host_step(spec, x, state, c["sim_dt"], atan2, **flags)
            t.update({k: torch.from_numpy(v).to(DEV) for k, v in flags.items()})
            src = _native.make_termination_sources(t, c["sim_dt"])
            desc, table = (torch.as_tensor(spec.rows.copy(), device=DEV), torch.as_tensor(spec.table.copy(), device=DEV))
            _native.terminations_step(desc, table, spec.kinds, src, *(bufs[k][1] for k in BUFFERS), stream=_stream())
            torch.cuda.synchronize()
            where = (c["name"], n, s)
            for k in BUFFERS:
                assert _same(bufs[k][1], state[k]), (where, k)
            assert _guards_intact(*(b for b, _ in bufs.values())), where


def test_optional_outputs_are_not_written_and_invalid_calls_are_refused(cases):
    from _terminations_cases import BUFFERS
    from allsteps_isaaclab_amd import _native

    c = cases[0]
    n, spec, T = 66, c["specs"][0], 9
    _, t = _device_inputs(c, 0, n)
    src = _native.make_termination_sources(t, c["sim_dt"])
    desc, table = torch.as_tensor(spec.rows.copy(), device=DEV), torch.as_tensor(spec.table.copy(), device=DEV)
    bufs = {k: _guarded((T, n) if k in ("term_dones", "last_episode_dones") else (n,), 7) for k in BUFFERS}
    main = [bufs[k][1] for k in BUFFERS[:4]]
    _native.terminations_step(desc, table, spec.kinds, src, *main, None, None, stream=_stream())
    torch.cuda.synchronize()
    assert bool((bufs["last_episode_dones"][1] == 7).all()) and bool((bufs["reset_request"][1] == 7).all())
    assert bool((bufs["dones"][1] <= 1).all()) and _guards_intact(*(b for b, _ in bufs.values()))
    for name, message in (("root_quat", "root_quat"), ("q", "needs the source q"), ("net", "net"), ("ep_len", "ep_len"),
                          ("time_left", "time_left / command_counter")):  # a term whose source is NULL
        with pytest.raises(_native.NativeError, match=message):
            _native.terminations_step(desc, table, spec.kinds,
                                      _native.make_termination_sources(dict(t, **{name: None}), c["sim_dt"]), *main,
                                      stream=_stream())
    with pytest.raises(_native.NativeError, match="unknown kinds"):
        _native.terminations_step(desc, table, 1 << 8, src, *main, stream=_stream())
    with pytest.raises(_native.NativeError, match="num_terms 17 outside"):
        _native.terminations_step(torch.zeros(17, 8, device=DEV), table, 1, src, *main, stream=_stream())
    # ids outside the rows passed by value read as 0: no flag from them, nothing written out of bounds
    rows = spec.rows.copy()
    tab = spec.table.copy()
    tab[0] = np.full(tab[0].shape, 1 << 20, np.int32).view(np.float32)
    _native.terminations_step(torch.as_tensor(rows, device=DEV), torch.as_tensor(tab, device=DEV), spec.kinds, src,
                              *main, stream=_stream())
    torch.cuda.synchronize()
    k = c["names"].index("contact_all")
    assert not bool(bufs["term_dones"][1][k].any()) and _guards_intact(*(b for b, _ in bufs.values()))


# ------------------------------------------------------------------ the envs
def _commands():
    from allsteps_isaaclab_amd.utils.commands import UniformVelocityCommandCfg as U

    return {"base_velocity": U(asset_name="robot", resampling_time_range=(0.02, 0.05), rel_standing_envs=0.2,
                               ranges=U.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), ang_vel_z=(-1.0, 1.0)))}


def _terminations(kind):
    from allsteps_isaaclab_amd.utils import terminations as TM
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    T = TM.TerminationTermCfg
    trunk = "torso" if kind == "walker" else "base"
    return {
        "time_out": T(func=TM.time_out, time_out=True),
        "resample": T(func=TM.command_resample, params={"command_name": "base_velocity", "num_resamples": 2},
                      time_out=True),
        "tilt": T(func=TM.bad_orientation, params={"limit_angle": 0.15}),
        "low": T(func=TM.root_height_below_minimum, params={"minimum_height": 1.3 if kind == "walker" else 0.55}),
        "jlim": T(func=TM.joint_pos_out_of_limit, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[0, 2, 5, 7])}),
        "jman": T(func=TM.joint_pos_out_of_manual_limit, params={"bounds": (-1.2, 1.2)}),
        "jvel": T(func=TM.joint_vel_out_of_manual_limit,
                  params={"max_velocity": 3.0, "asset_cfg": SceneEntityCfg("robot", joint_ids=[3])}),
        "base_contact": T(func=TM.illegal_contact,
                          params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("contact_forces", body_names=trunk)}),
        "limbs": T(func=TM.illegal_contact, params={"threshold": 150.0, "sensor_cfg": SceneEntityCfg("contact_forces")}),
        "feet": T(func=TM.illegal_contact, params={"threshold": 300.0, "sensor_cfg": SceneEntityCfg("sensor")}),
    }


def _env(kind, n, terminations=None, reset=False, seed=42, extra=None):
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
    if terminations is not None:
        cfg.terminations, cfg.terminations_reset = terminations, reset
        cfg.commands, cfg.contact_forces = _commands(), True
    for k, v in (extra or {}).items():
        setattr(cfg, k, v)
    return Env(cfg)


def _actions(n, cols, steps, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.rand(n, cols, device=DEV, generator=g) * 2.4 - 1.2 for _ in range(steps)]


def _near_time_out(env, stride=5, left=2):
    """Every stride-th env `left` steps from its time-out."""
    env.state["ep_len"][::stride] = env.max_episode_length - left


# ------------------------------------------------------------------ 2. the step is the step
@pytest.mark.parametrize("kind, cols", [("walker", 21), ("quadruped", 12)])
def test_without_terminations_reset_the_step_is_bitwise_the_steps(kind, cols):
    """16 random steps at 128 envs: observation, reward and dones are those of an env without the manager (which has
    the commands and the contact report too: they write only their own buffers), with time-outs on the way."""
    n = 128
    env, clean = _env(kind, n, _terminations(kind)), _env(kind, n)
    assert env._terminations is not None and clean._terminations is None
    o1, _ = env.reset()
    o2, _ = clean.reset()
    assert _same(o1["policy"], o2["policy"])
    seen = torch.zeros(len(env.termination_manager.active_terms), dtype=torch.bool, device=DEV)
    for k, a in enumerate(_actions(n, cols, 16)):
        if k == 4:
            _near_time_out(env)
            _near_time_out(clean)
        launches = env._terminations.launches
        o1, r1, t1, u1, _ = env.step(a)
        o2, r2, t2, u2, _ = clean.step(a)
        torch.cuda.synchronize()
        assert env._terminations.launches == launches + 1, k  # one launch a step
        assert _same(o1["policy"], o2["policy"]) and _same(r1, r2), k
        assert t1.dtype == torch.bool and torch.equal(t1, t2) and torch.equal(u1, u2), k
        seen |= env._terminations.term_dones.bool().any(dim=1)
    for key in ("root_pos", "q", "qd", "ep_len"):
        assert _same(env.state[key], clean.state[key]), key
    print("terms seen set:", dict(zip(env.termination_manager.active_terms, seen.tolist())))
    assert bool(seen[env.termination_manager.active_terms.index("time_out")])
    for e in (env, clean):
        e.close()


# ------------------------------------------------------------------ 3. the flags are the torch callables' on the views
@pytest.mark.parametrize("kind, cols", [("walker", 21), ("quadruped", 12)])
def test_flags_equal_the_torch_callables_on_the_views(kind, cols):
    """Every term's flag against its callable of utils/terminations.py evaluated on the env's views after the step,
    bit for bit; bad_orientation through the band of _terminations_cases (the device's torch.cross / bmm and acos
    do not round as the kernel's operations do); the unions, last_episode_dones and reset_request follow."""
    from types import SimpleNamespace as NS

    from _terminations_cases import orientation_angle64, orientation_band

    n = 128
    terms = _terminations(kind)
    env = _env(kind, n, terms)
    env.reset()
    mgr = env.termination_manager
    names = mgr.active_terms
    seen = {k: [False, False] for k in names}
    last = torch.zeros(len(names), n, dtype=torch.bool, device=DEV)
    for k, a in enumerate(_actions(n, cols, 16, seed=5)):
        if k == 4:
            _near_time_out(env)
        # the commands move after the terminations, as in the reference: command_resample reads the rows as they
        # stand before the step
        cm = env._commands
        before = NS(time_left=cm.time_left[0].clone(), command_counter=cm.counter[0].clone())
        _, _, term, trunc, _ = env.step(a)
        torch.cuda.synchronize()
        early = NS(step_dt=env.step_dt, command_manager=NS(get_term=lambda name: before))
        want = {name: t.func(early if name == "resample" else env, **t.params) for name, t in terms.items()}
        quat = env.state["root_quat"].cpu().numpy()
        _, a64 = orientation_angle64(quat)
        limit = float(np.float32(terms["tilt"].params["limit_angle"]))
        held = torch.from_numpy(np.abs(a64 - limit) > orientation_band(quat)).to(DEV)
        assert torch.equal(mgr.get_term("tilt")[held], torch.from_numpy(a64 > limit).to(DEV)[held]), k
        flags = []
        for name in names:
            got = mgr.get_term(name)
            assert got.dtype == torch.bool and got.shape == (n,)
            if name == "tilt":
                assert torch.equal(got[held], want[name][held]), (k, name)
            else:
                assert torch.equal(got, want[name]), (k, name)
            seen[name][0] |= bool(got.any())
            seen[name][1] |= bool((~got).any())
            flags.append(got)
        flags = torch.stack(flags)
        to = torch.stack([f for f, t in zip(flags, terms.values()) if t.time_out]).any(dim=0)
        te = torch.stack([f for f, t in zip(flags, terms.values()) if not t.time_out]).any(dim=0)
        assert torch.equal(mgr.time_outs, to) and torch.equal(mgr.terminated, te) and torch.equal(mgr.dones, to | te), k
        assert torch.equal(mgr.reset_request, (to | te) & ~(term | trunc)), k
        last = torch.where((to | te | term | trunc).unsqueeze(0), flags, last)
        assert torch.equal(torch.stack(list(mgr.last_episode_dones.values())), last), k
        assert bool((mgr.get_term("time_out") | ~trunc).all()), k  # a step's time-out is the manager's
    print({k: v for k, v in seen.items()})
    # what the random walk is sure to reach in 16 steps on either robot; the walker also sinks below the height and
    # touches its trunk (the quadruped does neither in 16 steps: the printed record)
    for name in ("time_out", "tilt", "jvel") + (("low", "base_contact") if kind == "walker" else ()):
        assert seen[name] == [True, True], (name, seen[name])
    counts = mgr.reset([0, 5, 7])
    assert counts == {f"Episode_Termination/{name}": int(mgr.get_term(name)[[0, 5, 7]].sum()) for name in names}
    assert "<TerminationManager> contains 10 active terms." in str(mgr)
    env.close()


# ------------------------------------------------------------------ 4. graph replay with a live set_term_cfg
def test_env_step_replays_from_a_graph_with_a_live_term_change():
    """A step captured under torch.cuda.graph replays: 6 replays equal 6 eager steps of a twin env bit for bit; a
    threshold changed and a time_out flipped after the capture show in the next replay."""
    from allsteps_isaaclab_amd.utils import terminations as TM

    n = 64
    envs = []
    for graph in (False, True):
        e = _env("walker", n, _terminations("walker"))
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
    mgr = ge.termination_manager
    for k in range(1, 7):
        if k == 3:  # every env is below 10 m: the term is set everywhere, and now it is a time-out
            new = TM.TerminationTermCfg(func=TM.root_height_below_minimum, params={"minimum_height": 10.0}, time_out=True)
            for e in envs:
                e.termination_manager.set_term_cfg("low", new)
        if k == 5:
            new = TM.TerminationTermCfg(func=TM.root_height_below_minimum, params={"minimum_height": -10.0})
            for e in envs:
                e.termination_manager.set_term_cfg("low", new)
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        ge.account_steps(1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        for key, v in eager._terminations.tensors().items():
            assert _same(v, ge._terminations.tensors()[key]), (k, key)
        low = mgr.get_term("low")
        if k in (3, 4):
            assert bool(low.all()) and bool(mgr.time_outs.all()), k
        if k >= 5:
            assert not bool(low.any()), k
        if k == 2:
            assert not bool(mgr.time_outs.all())
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 5. terminations_reset
def _reset_env(n, graph=False):
    from allsteps_isaaclab_amd.utils import observations as OB
    from allsteps_isaaclab_amd.utils import rewards as RW
    from allsteps_isaaclab_amd.utils import terminations as TM

    g = OB.ObservationGroupCfg(history_length=3)
    g.base_pos_z = OB.ObservationTermCfg(func=OB.base_pos_z)
    terms = {"time_out": TM.TerminationTermCfg(func=TM.time_out, time_out=True),
             "low": TM.TerminationTermCfg(func=TM.root_height_below_minimum, params={"minimum_height": 1.3})}
    env = _env("walker", n, terms, reset=True,
               extra={"rewards": {"alive": RW.RewardTermCfg(func=RW.is_alive, weight=0.5)}, "observations": {"obs": g},
                      "contact_air_time": True})
    env.set_graph_capture(graph)
    return env


def test_terminations_reset_ends_and_resets_the_envs_the_manager_names():
    """Walker, root_height_below_minimum at 1.3 m (the walker starts near 1.5 m and the task itself lets it sink much
    further).  A twin env without the manager is loaded with the env's state before every step and takes the same
    step: its observation is the step's own, and its ``_reset_idx`` of the envs the manager named is the independent
    reset.  In the step an env trips: the returned terminated is set, its episode length is 0, its observation row
    and its state are those of the twin's ``_reset_idx``, its reward sums are cleared (the sums it had are in
    last_episode_sums) and its observation history is refilled -- once: the next step's sum is that step's value; an
    env that did not trip keeps the step's own observation row bit for bit, in every step."""
    n = 128
    env, twin = _reset_env(n), _env("walker", n)
    env.reset()
    twin.reset()
    t = env._terminations
    tripped_ever = torch.zeros(n, dtype=torch.bool, device=DEV)
    check_next = None
    value = float(np.float32(np.float32(1.0) * np.float32(0.5)) * np.float32(env.step_dt))
    for k, a in enumerate(_actions(n, 21, 16, seed=9)):
        sums_before = env._rewards.episode_sums.clone()
        twin.set_state(env.get_state())
        o, r, term, trunc, _ = env.step(a)
        o2, r2, term2, trunc2, _ = twin.step(a)
        torch.cuda.synchronize()
        req = t.reset_request.bool()
        own_term, own_trunc = env.reset_terminated, env.reset_time_outs
        assert torch.equal(own_term, term2) and torch.equal(own_trunc, trunc2) and _same(r, r2), k
        assert torch.equal(req, env.termination_manager.get_term("low") & ~(own_term | own_trunc)), k
        assert torch.equal(term, own_term | env.termination_manager.terminated), k
        assert torch.equal(trunc, own_trunc | env.termination_manager.time_outs), k
        assert bool(term[req].all()), k
        assert bool((env.state["ep_len"][req] == 0).all()) and bool((env.state["ep_len"][~(term | trunc)] > 0).all()), k
        assert _same(o["policy"][~req], o2["policy"][~req]), k  # the step's own rows, bit for bit, in every step
        if bool(req.any()):
            want = twin._reset_idx(req)["policy"]
            torch.cuda.synchronize()
            assert _same(o["policy"][req], want[req]), k  # the reset's rows
            assert not _same(want[req], o2["policy"][req]), k
            # the managers reset these envs once, in the step: sums cleared and kept aside, history refilled
            sums, lastsum = env._rewards.episode_sums, env._rewards.last_episode_sums
            assert bool((sums[:, req] == 0).all()), k
            assert _same(lastsum[0, req], sums_before[0, req] + 0.0 * value), k  # terminated: is_alive adds 0
            hist = o["obs"][req]
            assert hist.shape[1] == 3 and bool((hist == hist[:, :1]).all()), k
            assert bool((env.sensor.data.current_air_time[req] == 0).all()), k
        for key in ("root_pos", "root_quat", "q", "qd", "ep_len", "episode", "idx", "swing", "foot_contact"):
            assert _same(env.state[key], twin.state[key]), (k, key)  # the tick for every env included
        if check_next is not None:  # the step after a trip: not cleared a second time
            live = check_next & ~(term | trunc)
            assert _same(env._rewards.episode_sums[0, live], torch.full((int(live.sum()),), value)), k
        check_next = req.clone()
        tripped_ever |= req
    print("envs the manager reset:", int(tripped_ever.sum()), "of", n)
    assert 0 < int(tripped_ever.sum())
    for e in (env, twin):
        e.close()


def test_terminations_reset_replays_from_a_graph():
    """run() is purely stream-ordered under as_set_graph_safe, in reset mode too: a captured step with
    terminations_reset replays, equal to an eager twin bit for bit."""
    n = 64
    eager, ge = _reset_env(n), _reset_env(n, graph=True)
    for e in (eager, ge):
        e.reset()
    acts = _actions(n, 21, 13, seed=9)
    static = acts[0].clone()
    ge.step(static)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    tripped = 0
    for k in range(1, 13):
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        ge.account_steps(1)
        torch.cuda.synchronize()
        assert _same(o1["policy"], out[0]["policy"]) and _same(o1["obs"], out[0]["obs"]) and _same(r1, out[1]), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        for key in ("root_pos", "q", "ep_len"):
            assert _same(eager.state[key], ge.state[key]), (k, key)
        tripped += int(ge._terminations.reset_request.sum())
    assert tripped > 0
    for e in (eager, ge):
        e.close()


# ------------------------------------------------------------------ 6. state round trip
def test_state_round_trip_and_compute_by_hand():
    n = 64
    env = _env("quadruped", n, _terminations("quadruped"))
    env.reset()
    acts = _actions(n, 12, 6)
    for a in acts[:2]:
        env.step(a)
    state = env.get_state()
    keys = {"termination_" + k for k in ("term_dones", "time_outs", "terminated", "dones", "last_episode_dones",
                                         "reset_request")}
    assert keys <= set(state) and state["termination_term_dones"].dtype == torch.uint8
    first = []
    for a in acts[2:5]:
        env.step(a)
        first.append({k: v.clone() for k, v in env._terminations.tensors().items()})
    env.set_state(state)
    for k, v in env._terminations.tensors().items():
        assert _same(v, state[k]), k
    for a, want in zip(acts[2:5], first):
        env.step(a)
        torch.cuda.synchronize()
        for k, v in env._terminations.tensors().items():
            assert _same(v, want[k]), k
    # compute() by hand: one more launch on the state as it stands; no env counts as reset by the step
    mgr = env.termination_manager
    flags = torch.stack([mgr.get_term(k) for k in mgr.active_terms]).clone()
    dones = mgr.compute()
    torch.cuda.synchronize()
    assert dones.dtype == torch.bool and torch.equal(dones, mgr.dones)
    assert torch.equal(mgr.reset_request, dones)
    k = mgr.active_terms.index("low")
    assert torch.equal(mgr.get_term("low"), flags[k])  # the same state: the same flag
    terms = mgr.get_active_iterable_terms(3)
    assert [t[0] for t in terms] == mgr.active_terms and terms[0][1] in ([0.0], [1.0])
    assert mgr.get_term_cfg("low").func.__name__ == "root_height_below_minimum"
    env.close()


# ------------------------------------------------------------------ 7. the all-body contact sensor
@pytest.mark.parametrize("kind, cols, trunk", [("walker", 21, "torso"), ("quadruped", 12, "base")])
def test_illegal_contact_through_the_all_body_contact_sensor(kind, cols, trunk):
    from allsteps_isaaclab_amd.utils import terminations as TM
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    n = 64
    env = _env(kind, n, _terminations(kind))
    sensor = env.scene.sensors["contact_forces"]
    assert sensor.body_names == list(env.robot.data.body_names) and sensor.num_bodies == len(sensor.body_names)
    ids, names = sensor.find_bodies(trunk)
    assert names == [trunk] and ids == [sensor.body_names.index(trunk)]
    assert sensor.find_bodies([".*"])[0] == list(range(sensor.num_bodies))
    with pytest.raises(ValueError, match="match no body"):
        sensor.find_bodies("no_such_body")
    env.reset()
    feet = [sensor.body_names.index(b) for b in env.sensor.body_names]
    hit_trunk = hit_any = False
    for a in _actions(n, cols, 12, seed=13):
        launches = env._launches
        env.step(a)
        hist = sensor.data.net_forces_w_history
        assert env._launches == launches + 1  # the view adds no launch that changes the report
        assert hist.shape == (n, env.cfg.decimation, sensor.num_bodies, 3)
        assert _same(sensor.data.net_forces_w, hist[:, 0])
        assert _same(hist[:, :, feet], env.sensor.data.net_forces_w_history)  # the foot rows, bitwise
        want = TM.illegal_contact(env, 1.0, SceneEntityCfg("contact_forces", body_names=trunk))
        assert torch.equal(env.termination_manager.get_term("base_contact"), want)
        by_hand = (hist[:, :, ids[0]].norm(dim=-1).max(dim=1)[0] > 1.0)
        assert torch.equal(want, by_hand)
        hit_trunk |= bool(want.any())
        hit_any |= bool(env.termination_manager.get_term("limbs").any())
    print(kind, "trunk contact seen:", hit_trunk, "any body above 150 N:", hit_any)
    assert hit_any
    env.close()


def test_a_default_env_has_no_termination_state_and_the_refusals_reach_the_constructor():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils import terminations as TM
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    for kind, cols in (("walker", 21), ("quadruped", 12)):
        clean = _env(kind, 4)
        assert clean._terminations is None and not hasattr(clean, "termination_manager")
        assert clean.scene.sensors == {}
        clean.reset()
        launches = clean._launches
        clean.step(_actions(4, cols, 1)[0])
        assert clean._launches == launches + 1
        assert not any(k.startswith("termination_") for k in clean.get_state())
        clean.close()
    with pytest.raises(_native.NativeError, match="terminations_reset is not served by the quadruped"):
        _env("quadruped", 4, _terminations("quadruped"), reset=True)
    contact = {"c": TM.TerminationTermCfg(func=TM.illegal_contact,
                                          params={"threshold": 1.0, "sensor_cfg": SceneEntityCfg("contact_forces")})}
    with pytest.raises(_native.NativeError, match="set cfg.contact_forces"):
        _env("walker", 4, contact, extra={"contact_forces": False})
