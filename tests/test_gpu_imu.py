"""The IMU sensors on the device (csrc/imu_kernels.h, envs/views.py; -m gpu).

The kernel is held, bit for bit, to the NumPy float32 restatement of csrc/allsteps_imu.h (_imu_cases.py, itself equal
to the header's host program bit for bit: test_imu_host.py), fed with as_body_state's rows of the same state
(robot.data) and its own previous velocities: the walker at n = 67 (odd: the last workgroup has a dead env slot; more
than one wave of envs) with three sensors -- the torso, a foot (the deepest chain) under a tilted offset, a thigh
without bias --, the quadruped at n = 6 with two.  Then the lazy rule: a skipped read differences against the last
read, a masked reset recomputes its envs alone against their old prev, `launches` counts one per dirty read; HIP-graph
replay of step + update(force_recompute=True); a get_state / set_state round trip; the feature-off env; and a check
that shares no code with the header: the torso's lin_acc_b turned back into the world equals the change of the body's
velocity over the step, in float64."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _imu_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILTED = tuple(float(x) for x in np.array([0.8, 0.3, -0.4, 0.2]) / np.linalg.norm([0.8, 0.3, -0.4, 0.2]))  # case b's


def _bits(t):
    return t.contiguous().view(torch.int32)


def _imu_cfg(leaf, **kw):
    from allsteps_isaaclab_amd.utils.sensors import ImuCfg

    return ImuCfg(prim_path="/World/envs/env_.*/Robot/" + leaf, **kw)


def _walker_imus():
    from allsteps_isaaclab_amd.utils.sensors import ImuCfg

    return {"imu": _imu_cfg("torso"),
            "foot_imu": _imu_cfg("left_foot", offset=ImuCfg.OffsetCfg(pos=(0.1, -0.05, 0.2), rot=TILTED)),
            "thigh_imu": _imu_cfg("right_thigh", gravity_bias=(0.0, 0.0, 0.0))}


def _walker(n=67, imu="three", seed=42):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.imu = _walker_imus() if imu == "three" else imu
    return AllstepsEnv(cfg)


def _quadruped(n=6, seed=42):
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.utils.sensors import ImuCfg

    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.imu = {"imu": _imu_cfg("base", offset=ImuCfg.OffsetCfg(pos=(0.05, 0.0, 0.1))),
               "foot_imu": _imu_cfg("LF_SHANK", offset=ImuCfg.OffsetCfg(pos=(0.0, 0.0, -0.3), rot=TILTED))}
    return AnymalCStonesEnv(cfg)


def _actions(n, cols, steps, seed=3, amp=1.2):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.uniform(-amp, amp, (n, cols)).astype(np.float32)).to(DEV) for _ in range(steps)]


def _buffers(g):
    torch.cuda.synchronize()
    return g.data.cpu().numpy().copy(), g.prev.cpu().numpy().copy()


def _restate(env, data, prev, mask, dt):
    """What one launch must leave: per sensor the restatement's masked update of (data, prev) -- (19, S, n) and
    (6, S, n) host arrays -- from as_body_state's rows of the state as it stands."""
    g = env._imus
    rows = env.robot.data._bodies().cpu().numpy()  # (16, B, n)
    t = g._table
    out_d, out_p = data.copy(), prev.copy()
    for s, b in enumerate(g._spec.bodies):
        r = rows[:, b]
        out_d[:, s], out_p[:, s] = ic.masked_update(
            data[:, s], prev[:, s], mask, r[0:3], r[3:7], r[13:16], r[10:13], list(t.offset_pos[s]),
            list(t.offset_rot[s]), list(t.com[s]), list(t.gravity_bias[s]), dt)
    return out_d, out_p


def _read_and_compare(env, data, prev, mask, dt, tag):
    """Read every sensor's data (one launch at most) and hold the buffers to the restatement; returns them."""
    g = env._imus
    want_d, want_p = _restate(env, data, prev, mask, dt)
    before = g.launches
    for s in g.sensors.values():
        s.data.lin_acc_b
    assert g.launches == before + 1, tag
    got_d, got_p = _buffers(g)
    assert not bool(g.outdated.any()), tag
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)), \
        (tag, np.argwhere(got_d.view(np.uint32) != want_d.view(np.uint32))[:5])
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), tag
    for s in g.sensors.values():
        s.data.pos_w, s.data.quat_w
    assert g.launches == before + 1, tag  # a second read launches nothing
    return got_d, got_p


def _run(env, cols, steps):
    n, g = env.num_envs, env._imus
    all_envs = np.ones(n, np.uint8)
    dt = env.physics_dt
    env.reset()
    assert g.launches == 0
    data, prev = _buffers(g)
    assert (data[3] == 1).all() and not data[[0, 1, 2] + list(range(4, 19))].any() and not prev.any()
    data, prev = _read_and_compare(env, data, prev, all_envs, dt, "reset")  # the first update: prev = 0
    for k, act in enumerate(_actions(n, cols, steps)):
        env.step(act)
        assert g.launches == k + 1  # the step launches nothing for the sensors
        data, prev = _read_and_compare(env, data, prev, all_envs, dt, f"step {k}")
    assert np.isfinite(data).all() and np.abs(data[13:16]).max() > 1.0
    return data, prev


def test_walker_three_sensors_equal_the_restatement_bit_for_bit():
    env = _walker()
    assert env.scene["imu"] is env.scene.sensors["imu"] and set(env.scene.sensors) == set(_walker_imus())
    assert not hasattr(env, "imu")  # the dict form registers by name only
    data, prev = _run(env, 21, 6)
    g = env._imus
    all_envs, dt, n = np.ones(67, np.uint8), env.physics_dt, 67
    acts = _actions(n, 21, 3, seed=5)
    # a skipped read: the next read differences against the last READ
    env.step(acts[0])
    env.step(acts[1])
    data, prev = _read_and_compare(env, data, prev, all_envs, dt, "after a skipped read")
    # a masked reset after a read: the other envs are not recomputed, the reset ones are, against their old prev
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[0, 31, 32, 63, 64, 66]] = True
    env._reset_idx(mask)
    assert g.outdated.cpu().numpy().tolist() == mask.cpu().numpy().astype(np.uint8).tolist()
    m = mask.cpu().numpy()
    new_d, new_p = _read_and_compare(env, data, prev, m.astype(np.uint8), dt, "masked reset")
    assert np.array_equal(new_d[..., ~m].view(np.uint32), data[..., ~m].view(np.uint32))
    assert np.array_equal(new_p[..., ~m].view(np.uint32), prev[..., ~m].view(np.uint32))
    assert not np.array_equal(new_d[13:16][..., m], data[13:16][..., m])
    # a user's update sets its own dt, for every later update; forced, it launches even with nothing outdated
    env.step(acts[2])
    want_d, want_p = _restate(env, new_d, new_p, all_envs, env.step_dt)
    n0 = g.launches
    env.scene["imu"].update(env.step_dt, force_recompute=True)
    got_d, got_p = _buffers(g)
    assert g.launches == n0 + 1 and np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    env.scene["foot_imu"].update(env.step_dt, force_recompute=True)
    again_d, again_p = _buffers(g)
    assert g.launches == n0 + 2 and np.array_equal(again_d.view(np.uint32), got_d.view(np.uint32))
    assert np.array_equal(again_p.view(np.uint32), got_p.view(np.uint32))
    # the robot view's writers do not mark the sensor
    pose = torch.cat([env.robot.data.root_pos_w, env.robot.data.root_quat_w], 1).clone()
    env.robot.write_root_pose_to_sim(pose)
    env.scene["imu"].data
    assert g.launches == n0 + 2
    env.account_steps(1)  # graph-replay accounting does, with the physics dt
    env.scene["imu"].data
    assert g.launches == n0 + 3 and g.dt == env.physics_dt
    env.close()


def test_quadruped_two_sensors_equal_the_restatement_bit_for_bit():
    env = _quadruped()
    _run(env, 12, 6)
    env.close()


def test_captured_step_and_forced_update_replay_equal_to_an_eager_run():
    envs = []
    for graph in (False, True):
        e = _walker()
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(67, 21, 5)
    static = acts[0].clone()
    for e in envs:  # warm-up, eager, both
        e.step(acts[0])
        e.scene["imu"].update(e.physics_dt, force_recompute=True)
    eager.set_state(ge.get_state())  # the same state, the sensors' previous velocities included
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ge.step(static)
        ge.scene["imu"].update(ge.physics_dt, force_recompute=True)
    a, b = eager._imus, ge._imus
    for k in range(1, 5):  # 4 replays against 4 eager steps
        eager.step(acts[k])
        eager.scene["imu"].update(eager.physics_dt, force_recompute=True)
        static.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.data), _bits(b.data)) and torch.equal(_bits(a.prev), _bits(b.prev)), k
        assert not bool(b.outdated.any())
        for key in ("q", "qd", "root_pos", "root_lin"):
            assert torch.equal(_bits(eager.state[key]), _bits(ge.state[key])), (k, key)
        ge.account_steps(1)
    # every replay recomputed every env: prev is the velocity of the replayed state
    rows = ge.robot.data._bodies()
    torso = ge._imus._spec.bodies[0]
    assert torch.equal(_bits(b.prev[3:6, 0]), _bits(rows[10:13, torso]))
    for e in envs:
        e.close()


def _rollout(env, acts):
    out = []
    for act in acts:
        env.step(act)
        env.scene["imu"].data
        out.append(tuple(x.clone() for x in (env._imus.data, env._imus.prev, env.state["q"], env.state["root_lin"])))
    return out


def test_state_round_trip_continues_to_the_same_bits():
    env = _walker()
    acts = _actions(67, 21, 6)
    env.reset()
    _rollout(env, acts[:3])
    st = env.get_state()
    assert st["imu_prev_lin_vel"].shape == st["imu_prev_ang_vel"].shape == (3, 3, 67)
    assert bool(st["imu_prev_lin_vel"].any()) and bool(st["imu_prev_ang_vel"].any())
    first = _rollout(env, acts[3:])
    fresh = _walker()
    fresh.reset()
    fresh.scene["imu"].data
    fresh.set_state(st)
    assert torch.equal(_bits(fresh._imus.prev), _bits(torch.cat([st["imu_prev_lin_vel"], st["imu_prev_ang_vel"]])))
    second = _rollout(fresh, acts[3:])
    for k, (x, y) in enumerate(zip(first, second)):
        for p, q in zip(x, y):
            assert torch.equal(_bits(p), _bits(q)), k
    env.close(), fresh.close()


def test_without_cfg_imu_there_is_no_sensor_and_no_state_key():
    env = _walker(imu=None)
    env.reset()
    env.step(_actions(67, 21, 1)[0])
    assert not hasattr(env, "imu") and env._imus is None and env.scene.sensors == {}
    st = env.get_state()
    assert set(st) == set(env.state) and not any(k.startswith("imu") for k in st)
    with pytest.raises(KeyError):
        env.scene["imu"]
    env.close()


def _rotate64(q, u):
    """R(q) u in float64, q = (w, x, y, z) rows: the textbook u + 2 w (r x u) + 2 r x (r x u)."""
    w, r = q[:, :1], q[:, 1:]
    t = 2.0 * np.cross(r, u)
    return u + w * t + np.cross(r, t)


def test_torso_acceleration_is_the_velocity_change_over_the_physics_step():
    """Independent of the header: lin_acc_b turned back by quat_w equals (v_after - v_before) / physics_dt + g in
    float64, v the sensor point's velocity from robot.data read before and after a step.  Bound, per env, from float32
    rounding of the kernel's handful of operations: 32 eps32 max(|v|, |w| |o - c|, |g| dt) / dt.  Measured: worst
    error 0.142 of the bound."""
    env = _walker(imu=_imu_cfg("torso"))
    imu = env.imu
    assert imu is env.scene["imu"] and imu.num_instances == 67
    b = env.robot.data.body_names.index("torso")
    o = np.array(imu.cfg.offset.pos, np.float64)
    c = np.asarray(env.model["body_com"][b], np.float64)
    g = np.array(imu.cfg.gravity_bias, np.float64)
    dt = float(np.float32(env.physics_dt))
    eps = float(np.finfo(np.float32).eps)

    def point_velocity():
        r = env.robot.data._bodies().cpu().numpy().astype(np.float64)[:, b].T  # (n, 16)
        arm = _rotate64(r[:, 3:7], np.broadcast_to(o - c, (len(r), 3)))
        return r[:, 13:16] + np.cross(r[:, 10:13], arm), np.linalg.norm(r[:, 10:13], axis=1)

    env.reset()
    imu.data
    worst = 0.0
    for k, act in enumerate(_actions(67, 21, 4, seed=9)):
        v0, w0 = point_velocity()
        env.step(act)
        v1, w1 = point_velocity()
        d = imu.data
        acc_w = _rotate64(d.quat_w.cpu().numpy().astype(np.float64), d.lin_acc_b.cpu().numpy().astype(np.float64))
        want = (v1 - v0) / dt + g
        scale = np.maximum.reduce([np.linalg.norm(v0, axis=1), np.linalg.norm(v1, axis=1),
                                   np.maximum(w0, w1) * np.linalg.norm(o - c),
                                   np.full(len(v0), np.linalg.norm(g) * dt)])
        bound = 32 * eps * scale / dt
        ratio = float((np.abs(acc_w - want).max(1) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"step {k}: worst error / bound {ratio:.3f}"
    print(f"torso lin_acc against the float64 velocity change: worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"worst error / bound {worst:.3f}"
    assert imu.launches == 5
    env.close()
