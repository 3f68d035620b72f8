"""The observation manager on the device (k_observations / k_observations_reset, cfg.observations): the kernel against
the reference's fixture from injected draws, its Philox path against the oracle's uniforms, and the envs -- the step
unchanged, the groups against the torch callables on the views, sensor and command refresh, HIP-graph replay with a
live set_term_cfg, state round trip, reset() and the default path."""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16  # kObsTile: envs per block
SIZES = [1, 66, 16 * TILE + 1]  # one env, a partial tile (four blocks and two envs), seventeen blocks


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """Bit for bit; two NaNs are equal."""
    a, b = a.contiguous(), b.contiguous()
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((_bits(a) == _bits(b)) | nan).all())


def _rows(a, n, axis=-1):
    """The first n envs of an array; past the fixture's 66 the envs repeat (an env's row depends on itself only)."""
    return np.ascontiguousarray(np.take(a, np.arange(n) % a.shape[axis], axis=axis))


def _guarded(shape, dtype=torch.float32, fill=0):
    """(buffer, view): a device tensor with 64 guard words behind it."""
    size = int(np.prod(shape))
    buf = torch.full((size + 64,), 12345, dtype=dtype, device=DEV)
    buf[:size] = fill
    return buf, buf[:size].view(shape)


@pytest.fixture(scope="module")
def cases():
    from _observations_cases import load_cases

    return load_cases()


def _tables(spec):
    return (torch.as_tensor(spec.rows.copy(), device=DEV), torch.as_tensor(spec.cols.copy(), device=DEV),
            torch.as_tensor(spec.omap.copy(), device=DEV))


def _sources(inputs, s, n):
    from allsteps_isaaclab_amd import _native

    t = {k: torch.from_numpy(_rows(v[s], n, axis=0 if k == "actions" else -1)).to(DEV) for k, v in inputs.items()}
    return t, _native.make_observation_sources(t)


# ------------------------------------------------------------------ 1. the kernel against the reference

@pytest.mark.parametrize("n", SIZES)
def test_kernel_reproduces_the_fixture_from_injected_draws(cases, n):
    """Every case, every step, every output word equals the reference's bit for bit (the host header does,
    tests/test_observations_host.py, so no tolerance is recorded); the guard words behind out, count and t stay."""
    from allsteps_isaaclab_amd import _native

    for c in cases:
        g = c["spec"]
        desc, cols, omap = _tables(g)
        obuf, out = _guarded((n, g.out_cols))
        cbuf, count = _guarded((n,), torch.int32)
        tbuf, t = _guarded((n,), torch.int32)
        for s in range(c["steps"]):
            keep, src = _sources(c["inputs"], s, n)
            draws = torch.from_numpy(_rows(c["draws"][s], n)).to(DEV)
            reset = torch.from_numpy(_rows(c["reset"][s], n)).to(DEV)
            _native.observations_step(desc, cols, omap, g.d0, g.out_cols, 0, src, out, count, t, reset=reset,
                                      draws=draws, stream=_stream())
            torch.cuda.synchronize()
            want = torch.from_numpy(_rows(c["out"][s], n, axis=0)).to(DEV)
            assert _same(out, want), (c["name"], s, n)
        assert bool((t == c["steps"]).all())
        for buf, size in ((obuf, n * g.out_cols), (cbuf, n), (tbuf, n)):
            assert bool((buf[size:] == 12345).all()), c["name"]


def test_reset_kernel_clears_the_masked_rows_only(cases):
    from allsteps_isaaclab_amd import _native

    n, cols = 66, 171
    obuf, out = _guarded((n, cols), fill=1.5)
    cbuf, count = _guarded((n,), torch.int32, fill=7)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[[0, 15, 16, 65]] = 1
    _native.observations_reset(out, count, mask=mask, stream=_stream())
    torch.cuda.synchronize()
    m = mask.bool()
    assert bool((out[m] == 0).all()) and bool((out[~m] == 1.5).all())
    assert bool((count[m] == 0).all()) and bool((count[~m] == 7).all())
    _native.observations_reset(out, count, mask=None, stream=_stream())
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((count == 0).all())
    assert bool((obuf[n * cols:] == 12345).all()) and bool((cbuf[n:] == 12345).all())


# ------------------------------------------------------------------ 2. the Philox path

def _philox_uniforms(orc, seed, env0, t, group, d0):
    """(d0, n): the uniform of every column from the oracle's blocks at (seed, env0 + e, t[e], 64 group + c / 4)."""
    from allsteps_isaaclab_amd import _native

    fn = orc.L.or_philox_block
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    buf = (C.c_float * 4)()
    u = np.zeros((4 * ((d0 + 3) // 4), len(t)), np.float32)
    for e in range(len(t)):
        for b in range((d0 + 3) // 4):
            fn(seed, (env0 + e) & 0xFFFFFFFF, int(t[e]), 64 * group + b, _native.OBS_TAG, buf)
            u[4 * b:4 * b + 4, e] = buf[:]
    return u


def _draw_group(kind_cfg, n):
    """A 63-column group whose output is the draw itself: operation abs with (0, 1) parameters."""
    from _observations_cases import context, load_fixture

    from allsteps_isaaclab_amd.envs.observations import ObservationGroups
    from allsteps_isaaclab_amd.utils import observations as OB
    from allsteps_isaaclab_amd.utils import sensors as SN
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    g = OB.ObservationGroupCfg(enable_corruption=True)
    for name, func, params in (("a", OB.joint_pos, {}), ("b", OB.base_lin_vel, {}), ("c", OB.joint_vel, {}),
                               ("d", OB.last_action, {}), ("e", SN.height_scan,
                                                           {"sensor_cfg": SceneEntityCfg("height_scanner")}),
                               ("f", OB.joint_pos, {}), ("g", OB.root_ang_vel_w, {})):
        setattr(g, name, OB.ObservationTermCfg(func=func, params=params, noise=kind_cfg))
    # no sources are passed: every term's value reads as 0 and the abs operation replaces it anyway
    return ObservationGroups({"g": g}, context(*load_fixture())).groups[0]


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    """obs_draw of the host header (tests/observations_check.cpp --draws), built once: (kind, seed, env0, t, group,
    d0) -> (d0, n) float32."""
    import shutil
    import struct
    import subprocess

    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the host header's draws need a host C++ compiler"
    tmp = tmp_path_factory.mktemp("obs_draws")
    exe = tmp / "observations_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-o", str(exe),
                        os.path.join(ROOT, "tests", "observations_check.cpp")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def draws(kind, seed, env0, t, group, d0):
        with open(tmp / "req.bin", "wb") as f:
            f.write(struct.pack("7I", seed & 0xFFFFFFFF, seed >> 32, env0, group, d0, kind, len(t)))
            f.write(np.ascontiguousarray(t, np.uint32).tobytes())
        r = subprocess.run([str(exe), "--draws", str(tmp / "req.bin"), str(tmp / "out.bin")], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.fromfile(tmp / "out.bin", np.float32).reshape(d0, len(t))

    return draws


# A unit normal is r cos a or r sin a with r = sqrtf(-2 logf(1 - u0)) <= sqrt(48 ln 2) < 5.8 and a = 2 pi u1.  Host
# and device share every operation but logf, cosf / sinf (sqrtf and the products are correctly rounded on both).
# With each library within 2 ulp: the logarithm's 4 ulp between the two are halved by the root (2 ulp of r, one more
# for the root's own rounding of a different argument), cos / sin differ by at most 4 ulp of 1, the product rounds
# once more on each side: |z_device - z_host| <= 5.8 (3 + 4 + 2) 2^-24 < 5.8 * 16 * 2^-24 = 5.6e-6, asked with the
# 16 for slack that is not measured.
NORMAL_BOUND = 5.8 * 16 * 2.0 ** -24


@pytest.mark.parametrize("n", SIZES)
def test_philox_draws_equal_the_host_headers(orc, host_draws, n):
    """Philox draws on the device against the host header's obs_draw for the same seed, env offset and counter:
    uniform draws bit for bit (and equal to the oracle's blocks); unit normals, which pass through each side's own
    logf / cosf / sinf, within NORMAL_BOUND -- the measured difference is printed (DESIGN.md records it)."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.utils import noise as N

    seed, env0, group = 0x9E3779B97F4A7C15, 1000, 2
    t0 = (np.arange(n) * 5 + 3).astype(np.int32)
    src = _native.make_observation_sources({})
    for kind in ("uniform", "gaussian"):
        cfg = (N.UniformNoiseCfg(operation="abs", n_min=0.0, n_max=1.0) if kind == "uniform"
               else N.GaussianNoiseCfg(operation="abs", mean=0.0, std=1.0))
        g = _draw_group(cfg, n)
        assert g.d0 == 63  # no multiple of 4: the last block is used in part
        desc, cols, omap = _tables(g)
        out = torch.zeros(n, g.out_cols, device=DEV)
        count = torch.zeros(n, dtype=torch.int32, device=DEV)
        t = torch.from_numpy(t0.copy()).to(DEV)
        _native.observations_step(desc, cols, omap, g.d0, g.out_cols, group, src, out, count, t, seed=seed,
                                  env_offset=env0, stream=_stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy().T
        want = host_draws(_native.NOISE_UNIFORM if kind == "uniform" else _native.NOISE_GAUSSIAN, seed, env0, t0,
                          group, g.d0)
        if kind == "uniform":
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            u = _philox_uniforms(orc, seed, env0, t0, group, g.d0)
            assert np.array_equal(got.view(np.uint32), u[:g.d0].view(np.uint32))
        else:
            err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
            differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            print(f"n={n}: max |z_device - z_host_header| = {err:.3e} ({differ} of {got.size} words differ)")
            assert err <= NORMAL_BOUND
        assert bool((t.cpu() == torch.from_numpy(t0) + 1).all()) and bool((count == 1).all())


# ------------------------------------------------------------------ 3. the envs

def _scanner_cfg(leaf):
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg, patterns

    return RayCasterCfg(prim_path="/World/envs/env_.*/Robot/" + leaf,
                        offset=RayCasterCfg.OffsetCfg(pos=(0.027, 0.031, 20.0)), attach_yaw_only=True,
                        pattern_cfg=patterns.GridPatternCfg(resolution=0.2, size=[0.8, 0.4]), debug_vis=False,
                        mesh_prim_paths=["/World/ground", "/World/envs/env_.*/step_.*"])


def _commands():
    from allsteps_isaaclab_amd.utils.commands import UniformVelocityCommandCfg as U

    return {"base_velocity": U(asset_name="robot", resampling_time_range=(0.02, 0.05), rel_standing_envs=0.1,
                               ranges=U.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), ang_vel_z=(-1.0, 1.0)))}


def _policy(noise: bool, history=None):
    """The velocity task's policy group plus an IMU term and the remaining robot terms, as 'obs'."""
    from allsteps_isaaclab_amd.utils import commands as CM
    from allsteps_isaaclab_amd.utils import noise as N
    from allsteps_isaaclab_amd.utils import observations as OB
    from allsteps_isaaclab_amd.utils import sensors as SN
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    T = OB.ObservationTermCfg
    u = lambda a: N.UniformNoiseCfg(n_min=-a, n_max=a)  # noqa: E731
    g = OB.ObservationGroupCfg(enable_corruption=noise, history_length=history)
    g.base_lin_vel = T(func=OB.base_lin_vel, noise=u(0.1))
    g.base_ang_vel = T(func=OB.base_ang_vel, noise=u(0.2))
    g.projected_gravity = T(func=OB.projected_gravity, noise=u(0.05))
    g.velocity_commands = T(func=CM.generated_commands, params={"command_name": "base_velocity"})
    g.joint_pos = T(func=OB.joint_pos_rel, noise=u(0.01))
    g.joint_vel = T(func=OB.joint_vel_rel, noise=N.GaussianNoiseCfg(mean=0.0, std=0.5), scale=0.05)
    g.actions = T(func=OB.last_action)
    g.height_scan = T(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")}, noise=u(0.1),
                      clip=(-1.0, 1.0))
    g.imu_lin_acc = T(func=SN.imu_lin_acc)
    g.imu_orientation = T(func=SN.imu_orientation)
    g.limits = T(func=OB.joint_pos_limit_normalized, params={"asset_cfg": SceneEntityCfg("robot", joint_ids=[0, 3])})
    g.root_quat = T(func=OB.root_quat_w, params={"make_quat_unique": True})
    g.root_pos = T(func=OB.root_pos_w)
    g.base_pos_z = T(func=OB.base_pos_z, scale=2.0)
    return g


def _env(kind, n, observations=None, seed=42):
    from allsteps_isaaclab_amd.utils.sensors import ImuCfg

    if kind == "walker":
        from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv as Env
        from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg as Cfg
        leaf = "walker3d"
    else:
        from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv as Env
        from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg as Cfg
        leaf = "base"
    cfg = Cfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    if observations is not None:
        cfg.observations = observations
        cfg.commands = _commands()
        cfg.height_scanner = _scanner_cfg(leaf)
        cfg.imu = ImuCfg(prim_path="/World/envs/env_.*/Robot/" + leaf)
    return Env(cfg)


def _actions(n, cols, steps, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.rand(n, cols, device=DEV, generator=g) * 2 - 1 for _ in range(steps)]


def _torch_group(env, group_cfg, names, reset):
    """The group from the torch callables on the views, as the reference composes it without noise: per term the
    function, clip, scale; last_action zero for the envs the step reset."""
    from allsteps_isaaclab_amd.utils import observations as OB

    out = {}
    for name in names:
        t = getattr(group_cfg, name)
        v = t.func(env, **t.params).clone().float()
        if t.func is OB.last_action:
            v[reset] = 0.0
        if t.clip:
            v = v.clip_(min=t.clip[0], max=t.clip[1])
        if t.scale is not None:
            v = v.mul_(torch.tensor(t.scale, dtype=torch.float, device=v.device))
        out[name] = v
    return out


# The base-frame terms on the device follow the reference's CPU rounding (the fixture's); torch's GPU kernels may
# contract or order the cross product and the bmm's dot differently.  quat_rotate_inverse is a - b + c with
# |a| <= |u|, |b| <= |u|, |c| <= 2 |u| for a unit quaternion, each from at most five rounded operations on values of
# that size, so two evaluations differ by at most 2 (5 + 5 + 5 + 2) 2^-24 (2 |u|) < 2^-18 |u| -- asked with |u|
# replaced by max(1, the largest component's magnitude), which only tightens it for |u| with several components.
ROTATED = ("base_lin_vel", "base_ang_vel", "projected_gravity")


@pytest.mark.parametrize("kind,cols", [("walker", 21), ("quadruped", 12)])
def test_step_is_unchanged_and_the_group_equals_the_torch_callables(kind, cols):
    n, steps = 66, 20
    group = _policy(noise=False)
    env, clean = _env(kind, n, {"obs": group}), _env(kind, n)
    assert env.observation_manager.active_terms["obs"][0] == "base_lin_vel"
    o0, _ = env.reset()
    c0, _ = clean.reset()
    assert set(o0) == {"policy", "obs"} and set(c0) == {"policy"}
    assert torch.equal(_bits(o0["policy"]), _bits(c0["policy"]))
    names = env.observation_manager.active_terms["obs"]
    dims = [d[0] for d in env.observation_manager.group_obs_term_dim["obs"]]
    resets, worst = 0, 0.0
    for k, a in enumerate(_actions(n, cols, steps)):
        launches = (env.height_scanner.launches, env._imus.launches, env._observations.launches)
        o, r, te, tr, _ = env.step(a)
        oc, rc, tec, trc, _ = clean.step(a)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o["policy"]), _bits(oc["policy"])) and torch.equal(_bits(r), _bits(rc)), k
        assert torch.equal(te, tec) and torch.equal(tr, trc), k
        # the step brought the two sensors up to date (one launch each) and launched the group once ...
        assert (env.height_scanner.launches, env._imus.launches, env._observations.launches) == \
            tuple(x + 1 for x in launches), k
        reset = te | tr
        resets += int(reset.sum())
        want = _torch_group(env, group, names, reset)
        # ... so reading them afterwards launches nothing, and the command is this step's
        assert (env.height_scanner.launches, env._imus.launches) == (launches[0] + 1, launches[1] + 1), k
        got = dict(zip(names, torch.split(o["obs"], dims, dim=1)))
        assert o["obs"].shape == (n, sum(dims)) and o["obs"] is env.observation_manager._o.buffer["obs"]
        assert torch.equal(got["velocity_commands"], env.command_manager.get_command("base_velocity")), k
        for name in names:
            if name in ROTATED:
                u = {"base_lin_vel": env.robot.data.root_lin_vel_w, "base_ang_vel": env.robot.data.root_ang_vel_w,
                     "projected_gravity": torch.ones(1, device=DEV)}[name]
                size = max(1.0, float(u.abs().max()))
                tol = 2.0 ** -18 * size
                err = float((got[name] - want[name]).abs().max())
                worst = max(worst, err / size)
                assert err <= tol, (k, name, err, tol)
            else:
                assert _same(got[name], want[name]), (k, name)
    print(f"{kind}: {resets} env resets in {steps} steps; rotated terms against torch on the device: largest "
          f"difference {worst:.3e} = {worst * 2.0 ** 24:.2f} x 2^-24 per unit of the vector's size (bound 2^-18)")
    for e in (env, clean):
        e.close()


def test_env_step_replays_from_a_graph_with_a_live_set_term_cfg():
    """A step captured under torch.cuda.graph replays with fresh draws and a moving history: 5 replays equal 5 eager
    steps of a twin env bit for bit, history and draws included; a clip set after the capture holds in the replays
    that follow."""
    from allsteps_isaaclab_amd.utils import observations as OB
    from allsteps_isaaclab_amd.utils import sensors as SN
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg

    n = 66
    envs = []
    for graph in (False, True):
        e = _env("walker", n, {"obs": _policy(noise=True, history=3)})
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(n, 21, 7)
    static = acts[0].clone()
    ge.step(static)  # warm-up, eager
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    names = ge.observation_manager.active_terms["obs"]
    hs = names.index("height_scan")
    lo = sum(d[0] for d in ge.observation_manager.group_obs_term_dim["obs"][:hs])
    width = ge.observation_manager.group_obs_term_dim["obs"][hs][0]
    seen, dones = [], []
    for k in range(1, 6):
        if k == 4:
            new = OB.ObservationTermCfg(func=SN.height_scan, params={"sensor_cfg": SceneEntityCfg("height_scanner")},
                                        clip=(-0.01, 0.01))
            for e in envs:
                e.observation_manager.set_term_cfg("obs", "height_scan", new)
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        ge.account_steps(1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        assert _same(o1["obs"], out[0]["obs"]), k
        newest = out[0]["obs"][:, lo + width - width // 3: lo + width]  # the term's last slot
        assert bool((newest.abs() <= 0.01).all()) == (k >= 4), k
        seen.append(out[0]["obs"].clone())
        dones.append((out[2] | out[3]).clone())
    assert not _same(seen[0], seen[1])
    # the history moved: for the envs replay 3 did not reset, a slot of replay 2 is the next older slot of replay 3
    d = width // 3
    keep = ~dones[2]
    assert bool(keep.any())
    assert _same(seen[1][keep, lo + d: lo + 2 * d], seen[2][keep, lo: lo + d])
    assert _same(seen[1][keep, lo + 2 * d: lo + 3 * d], seen[2][keep, lo + d: lo + 2 * d])
    st1, st2 = eager.get_state(), ge.get_state()
    for key in ("observation_t", "observation_count", "observation_history_obs"):
        assert _same(st1[key].float(), st2[key].float()), key
    for e in envs:
        e.close()


def test_state_round_trip_reset_and_manager_calls():
    n = 66
    env = _env("quadruped", n, {"obs": _policy(noise=True, history=3),
                                "split": _split_group()})
    o0, _ = env.reset()
    torch.cuda.synchronize()
    m = env.observation_manager
    assert m.group_obs_concatenate == {"obs": True, "split": False}
    assert m.group_obs_dim["split"] == [(2, 12), (9,)] and o0["split"]["joint_pos"].shape == (n, 2, 12)
    assert "Active Observation Terms in Group: 'split'" in str(m)
    # reset() fills the history with the first value: the three slots of every term are equal, pushed once; the last
    # action reads zero
    at = 0
    for name, (dim,) in zip(m.active_terms["obs"], m.group_obs_term_dim["obs"]):
        slots = o0["obs"][:, at:at + dim].reshape(n, 3, dim // 3)
        assert _same(slots[:, 0], slots[:, 2]) and _same(slots[:, 1], slots[:, 2]), name
        if name == "actions":
            assert bool((slots == 0).all())
        at += dim
    assert bool((env._observations.count == 1).all()) and bool((env._observations.t == 1).all())
    acts = _actions(n, 12, 6)
    for a in acts[:2]:
        env.step(a)
    state = env.get_state()
    assert {"observation_t", "observation_count", "observation_history_obs", "observation_history_split"} <= set(state)
    first = [{k: (v.clone() if torch.is_tensor(v) else {x: y.clone() for x, y in v.items()})
              for k, v in env.step(a)[0].items()} for a in acts[2:5]]
    env.set_state(state)
    for a, want in zip(acts[2:5], first):
        got = env.step(a)[0]
        torch.cuda.synchronize()
        assert _same(got["obs"], want["obs"]) and _same(got["policy"], want["policy"])
        assert all(_same(got["split"][x], want["split"][x]) for x in want["split"])
    # compute() by hand launches again and pushes again: the newest slot moves one slot back
    before = env._observations.buffer["split"]["joint_pos"].clone()
    count = env._observations.count.clone()
    again = m.compute()
    torch.cuda.synchronize()
    assert bool((env._observations.count == count + 1).all())
    assert _same(again["split"]["joint_pos"][:, 0], before[:, 1])
    m.compute_group("split")
    torch.cuda.synchronize()
    assert bool((env._observations.count[1] == count[1] + 2).all()) and \
        bool((env._observations.count[0] == count[0] + 1).all())
    # reset(env_ids) clears those envs' rows and push counts, computes nothing
    assert m.reset([0, 65]) == {}
    torch.cuda.synchronize()
    assert bool((env._observations.out[0][[0, 65]] == 0).all()) and bool((env._observations.count[:, [0, 65]] == 0).all())
    assert bool((env._observations.count[:, 1:65] > 0).all())
    # the env's own masked reset path resets the masked envs' history only
    env._sensors_reset(torch.tensor([e == 7 for e in range(n)], device=DEV))
    torch.cuda.synchronize()
    assert int((env._observations.count[0] == 0).sum()) == 3
    assert m.get_term_cfg("obs", "actions").func.__name__ == "last_action"
    env.close()


def _split_group():
    from allsteps_isaaclab_amd.utils import observations as OB

    g = OB.ObservationGroupCfg(concatenate_terms=False)
    g.joint_pos = OB.ObservationTermCfg(func=OB.joint_pos, history_length=2, flatten_history_dim=False)
    g.base_ang_vel = OB.ObservationTermCfg(func=OB.base_ang_vel, history_length=3)
    return g


def test_a_clean_env_allocates_and_launches_nothing():
    for kind, cols in (("walker", 21), ("quadruped", 12)):
        clean = _env(kind, 4)
        assert clean._observations is None and not hasattr(clean, "observation_manager")
        obs, _ = clean.reset()
        launches = clean._launches
        out = clean.step(_actions(4, cols, 1)[0])
        assert clean._launches == launches + 1  # the step's own launch and nothing beside it
        assert set(obs) == {"policy"} and set(out[0]) == {"policy"}
        assert not any(k.startswith("observation") for k in clean.get_state())
        clean.close()


def test_env_refuses_a_term_whose_sensor_the_cfg_lacks():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = 4
    cfg.sim.device = DEV
    cfg.observations = {"obs": _policy(noise=False)}
    with pytest.raises(_native.NativeError, match="cfg.commands"):
        AllstepsEnv(cfg)
