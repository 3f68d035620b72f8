"""The frame transformers on the device (csrc/frame_transformer_kernels.h, envs/views.py; -m gpu).

The kernel is held, bit for bit, to the NumPy float32 restatement of csrc/allsteps_frame_transformer.h
(_frame_transformer_cases.py, itself equal to the header's host program bit for bit:
test_frame_transformer_host.py), fed with as_body_state's rows 0:7 of the same state (robot.data) and its steps_pos:
the walker at n = 67 (odd: the last workgroup has a dead env slot; more than one wave of envs) with two sensors --
the torso to the feet and a toe frame under a tilted offset, the left foot under a source offset to the 20 stones --,
the quadruped at n = 6 from the base to its shanks.  Then the lazy rule: `launches` counts one per dirty read, and a
masked reset, a writer call and stone regeneration each make the next read relaunch; HIP-graph replay of step +
update(force_recompute=True); the feature-off env; and a check that shares no code with the header, in float64."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _frame_transformer_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = "/World/envs/env_.*"
TILTED = (0.8, 0.3, -0.4, 0.2)  # (not normalised: an offset's rot is used as given)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _walker_cfgs():
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg as FT
    from allsteps_isaaclab_amd.utils.sensors import OffsetCfg

    return {"feet": FT(prim_path=f"{NS}/Robot/torso",
                       target_frames=[FT.FrameCfg(prim_path=f"{NS}/Robot/.*_foot"),
                                      FT.FrameCfg(prim_path=f"{NS}/Robot/left_foot", name="left_toe",
                                                  offset=OffsetCfg(pos=(0.12, 0.0, -0.03), rot=TILTED))]),
            "stones": FT(prim_path="{ENV_REGEX_NS}/Robot/left_foot",
                         source_frame_offset=OffsetCfg(pos=(0.0, 0.0, -0.05), rot=(0.9, -0.1, 0.3, 0.2)),
                         target_frames=[FT.FrameCfg(prim_path="{ENV_REGEX_NS}/step_.*")])}


def _walker(n=67, ft="two", seed=42):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.frame_transformer = _walker_cfgs() if ft == "two" else ft
    return AllstepsEnv(cfg)


def _quadruped(n=6, seed=42):
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg as FT

    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.frame_transformer = FT(prim_path=f"{NS}/Robot/base", target_frames=[FT.FrameCfg(prim_path=f"{NS}/Robot/.*_SHANK")])
    return AnymalCStonesEnv(cfg)


def _actions(n, cols, steps, seed=3, amp=1.2):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.uniform(-amp, amp, (n, cols)).astype(np.float32)).to(DEV) for _ in range(steps)]


def _buffers(g):
    torch.cuda.synchronize()
    return g.source.cpu().numpy().copy(), g.target.cpu().numpy().copy()


def _poses(env):
    """(B + num_steps, 7, n) float32: as_body_state rows 0:7 of every body, then the stones with (1, 0, 0, 0)."""
    rows = env.robot.data._bodies().cpu().numpy()[0:7].transpose(1, 0, 2)  # (B, 7, n)
    stones = env.state["stones"].cpu().numpy()  # (3 * 20, n)
    ns = int(env.cfg.num_steps)
    st = np.zeros((ns, 7, rows.shape[2]), np.float32)
    st[:, 0:3] = stones[: 3 * ns].reshape(ns, 3, -1)
    st[:, 3] = 1.0
    return np.concatenate([rows, st]), rows.shape[0]


def _restate(env):
    """What one launch must leave: (source (7, S, n), target (14, F, n)) of the restatement on the state as it is."""
    g = env._frame_transformers
    spec = g._spec
    poses, nb = _poses(env)
    index = lambda body: body[1] + (nb if body[0] == "stone" else 0)  # noqa: E731
    src, tgt = [], []
    for s in range(spec.num_sensors):
        so = [*spec.source_offsets[s][0], *spec.source_offsets[s][1]]
        frames = [(index(body), [*pos, *rot]) for body, pos, rot in spec.frames[s]]
        a, b = fc.frames_of(poses, index(spec.sources[s]), so, spec.apply_source[s], frames, spec.apply_target[s])
        src.append(a)
        tgt.append(b)
    return np.stack(src, 1), np.concatenate(tgt, 1)


def _read_and_compare(env, tag):
    """Read every sensor's data (one launch in all) and hold the buffers to the restatement; returns them."""
    g = env._frame_transformers
    want_s, want_t = _restate(env)
    before = g.launches
    for s in g.sensors.values():
        s.data.target_pos_source
    assert g.launches == before + 1, tag
    got_s, got_t = _buffers(g)
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), \
        (tag, np.argwhere(got_s.view(np.uint32) != want_s.view(np.uint32))[:5])
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)), \
        (tag, np.argwhere(got_t.view(np.uint32) != want_t.view(np.uint32))[:5])
    for s in g.sensors.values():
        s.data.source_pos_w, s.data.target_quat_w
    assert g.launches == before + 1, tag  # a second read launches nothing
    return got_s, got_t


def _run(env, cols, steps):
    n, g = env.num_envs, env._frame_transformers
    env.reset()
    assert g.launches == 0
    source, target = _buffers(g)
    assert not source.any() and not target.any()  # zeros before the first update
    _read_and_compare(env, "reset")
    for k, act in enumerate(_actions(n, cols, steps)):
        env.step(act)
        assert g.launches == k + 1  # the step launches nothing for the sensors
        source, target = _read_and_compare(env, f"step {k}")
    assert np.isfinite(source).all() and np.isfinite(target).all()
    return source, target


def test_walker_two_sensors_equal_the_restatement_bit_for_bit():
    env = _walker()
    g = env._frame_transformers
    assert set(env.scene.sensors) == {"feet", "stones"} and env.scene["feet"] is g.sensors["feet"]
    assert not hasattr(env, "frame_transformer")  # the dict form registers by name only
    feet, stones = env.scene["feet"], env.scene["stones"]
    names = g._spec.frame_names[1]  # (not through .data: nothing is launched before the first reset)
    assert g._spec.frame_names[0] == ["left_foot", "left_toe", "right_foot"]
    assert len(names) == 20 and names.index("step_10") < names.index("step_2") and g.num_frames == 23
    assert g._spec.apply_source == [False, True] and g._spec.apply_target == [True, False]
    source, target = _run(env, 21, 6)
    d = feet.data
    assert d.target_frame_names == g._spec.frame_names[0] and stones.data.target_frame_names == names
    assert d.target_pos_w.shape == (67, 3, 3) and d.target_quat_source.shape == (67, 3, 4)
    assert d.source_pos_w.shape == (67, 3) and stones.data.target_pos_source.shape == (67, 20, 3)
    # the views are the buffers: the feet's link positions are robot.data's, the source the torso's
    bodies = env.robot.data.body_names
    pos = env.robot.data.body_link_pos_w
    assert torch.equal(_bits(d.target_pos_w[:, 0]), _bits(pos[:, bodies.index("left_foot")]))
    assert torch.equal(_bits(d.target_pos_w[:, 2]), _bits(pos[:, bodies.index("right_foot")]))
    assert torch.equal(_bits(d.source_pos_w), _bits(pos[:, bodies.index("torso")]))
    assert not torch.equal(d.target_pos_w[:, 1], d.target_pos_w[:, 0])  # the toe is off the foot
    # the stones' world poses are steps_pos in the sensor's order, with the identity quaternion
    order = [int(x.split("_")[1]) for x in names]
    assert torch.equal(_bits(stones.data.target_pos_w), _bits(env.steps_pos[:, order]))
    assert bool((stones.data.target_quat_w == torch.tensor([1.0, 0, 0, 0], device=DEV)).all())
    env.close()


def test_quadruped_base_to_shanks_equals_the_restatement_bit_for_bit():
    env = _quadruped()
    ft = env.frame_transformer
    assert ft is env.scene["frame_transformer"] and ft.num_instances == 6
    _run(env, 12, 6)
    assert ft.data.target_frame_names == ["LF_SHANK", "LH_SHANK", "RF_SHANK", "RH_SHANK"]
    assert "source body frame: base\n" in str(ft)
    env.close()


def test_masked_reset_writer_and_stone_regeneration_each_relaunch():
    env = _walker()
    n, g = 67, env._frame_transformers
    env.reset()
    for act in _actions(n, 21, 2, seed=5):
        env.step(act)
    _read_and_compare(env, "steps")
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[0, 31, 32, 63, 64, 66]] = True
    env._reset_idx(mask)
    before = _buffers(g)
    source, target = _read_and_compare(env, "masked reset")
    m = mask.cpu().numpy()
    assert not np.array_equal(target[:, :3][..., m], before[1][:, :3][..., m])  # the reset envs moved
    assert np.array_equal(target[:, :3][..., ~m].view(np.uint32), before[1][:, :3][..., ~m].view(np.uint32))
    pose = torch.cat([env.robot.data.root_pos_w, env.robot.data.root_quat_w], 1).clone()
    pose[:, 0] += 0.25
    env.robot.write_root_pose_to_sim(pose)
    moved, _ = _read_and_compare(env, "write_root_pose_to_sim")
    assert not np.array_equal(moved, source)
    vel = torch.zeros(n, 6, device=DEV)
    env.robot.write_root_velocity_to_sim(vel)
    _read_and_compare(env, "write_root_velocity_to_sim")
    env.robot.write_joint_state_to_sim(env.robot.data.joint_pos * 0.5, env.robot.data.joint_vel.clone())
    _read_and_compare(env, "write_joint_state_to_sim")
    env.generate_foot_steps(3)
    _, regenerated = _read_and_compare(env, "generate_foot_steps")
    assert not np.array_equal(regenerated[:, 3:], target[:, 3:])  # the stones' frames moved
    k = g.launches
    env.scene["stones"].reset()
    env.scene["feet"].data
    env.scene["feet"].update(env.step_dt)  # not forced: nothing
    assert g.launches == k + 1
    env.set_state(env.get_state())
    _read_and_compare(env, "set_state")
    env.account_steps(1)
    _read_and_compare(env, "account_steps")
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
        e.scene["feet"].update(e.step_dt, force_recompute=True)
    eager.set_state(ge.get_state())  # the same state
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ge.step(static)
        ge.scene["feet"].update(ge.step_dt, force_recompute=True)
    a, b = eager._frame_transformers, ge._frame_transformers
    launches = b.launches
    for k in range(1, 5):  # 4 replays against 4 eager steps
        eager.step(acts[k])
        eager.scene["stones"].update(eager.step_dt, force_recompute=True)
        static.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.source), _bits(b.source)) and torch.equal(_bits(a.target), _bits(b.target)), k
        for key in ("q", "qd", "root_pos", "root_lin", "stones"):
            assert torch.equal(_bits(eager.state[key]), _bits(ge.state[key])), (k, key)
        ge.account_steps(1)
    assert b.launches == launches  # the replays are the graph's, not the host's
    want_s, want_t = _restate(ge)
    got_s, got_t = _buffers(b)
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
    for e in envs:
        e.close()


def test_without_the_cfg_there_is_no_sensor_no_launch_and_no_state_key():
    env = _walker(ft=None)
    env.reset()
    env.step(_actions(67, 21, 1)[0])
    assert not hasattr(env, "frame_transformer") and env._frame_transformers is None
    assert env.scene.sensors == {} and env._lazy_sensors == ()
    st = env.get_state()
    assert set(st) == set(env.state) and not any("frame" in k for k in st)
    with pytest.raises(KeyError):
        env.scene["frame_transformer"]
    env.close()
    # a sensor name already registered in the scene is refused at construction
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.utils.sensors import ImuCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs, cfg.sim.device = 4, DEV
    cfg.imu = {"feet": ImuCfg(prim_path=f"{NS}/Robot/torso")}
    cfg.frame_transformer = _walker_cfgs()
    with pytest.raises(_native.NativeError, match=r"cfg\.frame_transformer: the sensor names \['feet'\] are already"):
        AllstepsEnv(cfg)


def _mul64(a, b):
    """The Hamilton product of (w, x, y, z) rows in float64, the textbook form."""
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)


def _matrix64(q):
    """(n, 3, 3) rotation matrices of unit (w, x, y, z) rows in float64."""
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


K = 40


def test_relative_poses_recompose_to_the_world_poses_in_float64():
    """Independent of the header, in float64 (rotation matrices and the textbook quaternion product):
      * source o target_in_source reproduces target_w: p_s + R(q_s / |q_s|) p_ts = p_t and (q_s / |q_s|) q_ts = q_t,
        every frame of two sensors -- the torso under a tilted source offset to the feet and the toe frame under a
        target offset, and the offset-free torso to the 20 stones;
      * for a stone under that offset-free torso source, target_pos_source = R(q)^T (steps_pos - p),
        p, q the torso's pose from robot.data.
    Bound per env and frame: K eps32 scale, K = 40, scale the largest length involved (|p_s|, |p_t|, |p_t - p_s|; 1 and
    |q_t| for the quaternion).  K from the float32 operations on the path: the difference (1 rounding) and
    quat_apply's two cross products, scalings and sums (18) each round an intermediate no larger than 2 scale, so at
    most eps32 scale each: 19; quat_inv's norm, root and quotient (9 roundings, eps32 / 2 relative each) perturb the
    inverse quaternion, to which the rotated vector's sensitivity is at most 4 scale: 18; together 37, rounded up to
    40.  The quaternion's path (quat_inv and quat_mul's 8 operations per component on values below 2) is shorter.
    Measured: worst error 0.035 of the bound (positions), 0.045 (quaternions)."""
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg as FT

    cfgs = {"feet": _walker_cfgs()["feet"]}  # (20 + 3 + 20 frames would be past AS_MAX_FRAMES)
    cfgs["feet"].source_frame_offset = _walker_cfgs()["stones"].source_frame_offset
    cfgs["stones_in_torso"] = FT(prim_path=f"{NS}/Robot/torso", target_frames=[FT.FrameCfg(prim_path=f"{NS}/step_.*")])
    env = _walker(ft=cfgs)
    eps = float(np.finfo(np.float32).eps)
    env.reset()
    worst_p = worst_q = 0.0
    f64 = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    for k, act in enumerate(_actions(67, 21, 4, seed=9)):
        env.step(act)
        for name, sensor in env.scene.sensors.items():
            d = sensor.data
            p_s, q_s = f64(d.source_pos_w), f64(d.source_quat_w)
            R = _matrix64(q_s / np.linalg.norm(q_s, axis=1, keepdims=True))
            for f in range(len(d.target_frame_names)):
                p_t, q_t = f64(d.target_pos_w[:, f]), f64(d.target_quat_w[:, f])
                p_ts, q_ts = f64(d.target_pos_source[:, f]), f64(d.target_quat_source[:, f])
                scale = np.maximum.reduce([np.linalg.norm(p_s, axis=1), np.linalg.norm(p_t, axis=1),
                                           np.linalg.norm(p_t - p_s, axis=1)])
                err = np.abs(p_s + np.einsum("nij,nj->ni", R, p_ts) - p_t).max(1)
                worst_p = max(worst_p, float((err / (K * eps * scale)).max()))
                qs = np.maximum(1.0, np.linalg.norm(q_t, axis=1))
                err = np.abs(_mul64(q_s / np.linalg.norm(q_s, axis=1, keepdims=True), q_ts) - q_t).max(1)
                worst_q = max(worst_q, float((err / (K * eps * qs)).max()))
        # the stones in the torso frame, from robot.data and steps_pos alone
        d = env.scene["stones_in_torso"].data
        b = env.robot.data.body_names.index("torso")
        p, q = f64(env.robot.data.body_link_pos_w[:, b]), f64(env.robot.data.body_quat_w[:, b])
        R = _matrix64(q / np.linalg.norm(q, axis=1, keepdims=True))
        steps = f64(env.steps_pos)
        for f, frame in enumerate(d.target_frame_names):
            s = steps[:, int(frame.split("_")[1])]
            want = np.einsum("nji,nj->ni", R, s - p)
            scale = np.maximum.reduce([np.linalg.norm(p, axis=1), np.linalg.norm(s, axis=1),
                                       np.linalg.norm(s - p, axis=1)])
            err = np.abs(f64(d.target_pos_source[:, f]) - want).max(1)
            worst_p = max(worst_p, float((err / (K * eps * scale)).max()))
    print(f"recomposed poses in float64: worst error / bound {worst_p:.3f} (positions), {worst_q:.3f} (quaternions)")
    assert worst_p <= 1.0 and worst_q <= 1.0, (worst_p, worst_q)
    assert env._frame_transformers.launches == 4
    env.close()
