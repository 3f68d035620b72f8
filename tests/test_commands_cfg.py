"""The command manager's Python surface, no GPU: the cfg field, the reference-named cfg classes through the compat
imports, parsing order, the refusal of everything the device kernel does not serve (each with its reason), the
reference's two constructor checks, the descriptor rows against hand values, the host side of set_term_cfg / refresh,
the C ABI's new names and argument checks, the fixture's own coverage and its regeneration."""

import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _uniform(**kw):
    from allsteps_isaaclab_amd.utils import commands as CM

    ranges = kw.pop("ranges", None) or CM.UniformVelocityCommandCfg.Ranges(
        lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), ang_vel_z=(-1.0, 1.0), heading=kw.pop("heading", None))
    d = dict(asset_name="robot", resampling_time_range=(10.0, 10.0), ranges=ranges)
    d.update(kw)
    return CM.UniformVelocityCommandCfg(**d)


def _normal(**kw):
    from allsteps_isaaclab_amd.utils import commands as CM

    d = dict(asset_name="robot", resampling_time_range=(5.0, 8.0), rel_standing_envs=0.1,
             ranges=CM.NormalVelocityCommandCfg.Ranges(mean_vel=(0.5, 0.1, -0.3), std_vel=(0.4, 0.25, 0.6),
                                                       zero_prob=(0.2, 0.3, 0.1)))
    d.update(kw)
    return CM.NormalVelocityCommandCfg(**d)


def _cpu_cfg(commands=None, n=4):
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = n
    cfg.commands = commands
    return cfg


def test_cfg_field_defaults_to_none_and_costs_nothing():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.commands is None
    env = DirectRLEnv(_cpu_cfg())
    assert env._commands is None and not hasattr(env, "command_manager")
    assert env._commands_get_state() == {}


def test_cfg_classes_carry_the_reference_fields_and_defaults():
    from allsteps_isaaclab_amd.utils import commands as CM

    t = CM.CommandTermCfg()
    assert t.class_type is CM.MISSING and t.resampling_time_range is CM.MISSING and t.debug_vis is False
    u = CM.UniformVelocityCommandCfg()
    assert u.asset_name is CM.MISSING and u.ranges is CM.MISSING and u.heading_command is False
    assert (u.heading_control_stiffness, u.rel_standing_envs, u.rel_heading_envs) == (1.0, 0.0, 1.0)
    r = CM.UniformVelocityCommandCfg.Ranges()
    assert r.lin_vel_x is CM.MISSING and r.lin_vel_y is CM.MISSING and r.ang_vel_z is CM.MISSING and r.heading is None
    nr = CM.NormalVelocityCommandCfg.Ranges()
    assert nr.mean_vel is CM.MISSING and nr.std_vel is CM.MISSING and nr.zero_prob is CM.MISSING
    assert issubclass(CM.NormalVelocityCommandCfg, CM.UniformVelocityCommandCfg)
    assert issubclass(CM.UniformVelocityCommandCfg, CM.CommandTermCfg)
    assert CM.NullCommandCfg().resampling_time_range == (math.inf, math.inf)
    # the marker / debug-vis fields are accepted and ignored
    _uniform(debug_vis=True, goal_vel_visualizer_cfg=object(), current_vel_visualizer_cfg=object())


def test_reference_style_cfg_through_the_compat_imports():
    """A reference locomotion cfg's command block (velocity_env_cfg.py), written against isaaclab.envs.mdp, builds
    the env's device state (on the CPU here: tensors only, no launch), in cfg order, None entries skipped."""
    code = """
from allsteps_isaaclab_amd import compat
compat.install()
import math, numpy as np, torch
from isaaclab.managers import CommandTermCfg
import isaaclab.envs.mdp as mdp
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

class CommandsCfg:
    base_velocity = mdp.UniformVelocityCommandCfg(
        asset_name="robot", resampling_time_range=(10.0, 10.0), rel_standing_envs=0.02, rel_heading_envs=1.0,
        heading_command=True, heading_control_stiffness=0.5, debug_vis=True,
        ranges=mdp.UniformVelocityCommandCfg.Ranges(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-1.0, 1.0),
                                                    ang_vel_z=(-1.0, 1.0), heading=(-math.pi, math.pi)))
    disabled = None
    second = mdp.NormalVelocityCommandCfg(
        asset_name="robot", resampling_time_range=(2.0, 4.0),
        ranges=mdp.NormalVelocityCommandCfg.Ranges(mean_vel=(1.0, 0.0, 0.0), std_vel=(0.5, 0.1, 0.2),
                                                   zero_prob=(0.0, 0.5, 0.5)))

assert issubclass(mdp.UniformVelocityCommandCfg, CommandTermCfg) and callable(mdp.generated_commands)
assert issubclass(mdp.NullCommandCfg, CommandTermCfg)
cfg = AllstepsEnvCfg()
cfg.sim.device = "cpu"
cfg.scene.num_envs = 8
cfg.commands = CommandsCfg()
env = DirectRLEnv(cfg)
c, m = env._commands, env.command_manager
assert m.active_terms == ["base_velocity", "second"]
assert c.desc.shape == (2, 21) and c.vel.shape == (2, 3, 8) and c.flags.shape == (2, 5, 8) and c.t.shape == (8,)
assert c.metrics.shape == c.last_metrics.shape == (2, 2, 8) and c.counter.dtype == torch.int32
assert c.dt == float(np.float32(cfg.sim.dt * cfg.decimation))
term = m.get_term("base_velocity")
assert term.command.shape == (8, 3) and term.command.data_ptr() == c.vel[0].data_ptr()
assert mdp.generated_commands(env, "base_velocity").data_ptr() == m.get_command("base_velocity").data_ptr()
assert m.get_command("second").data_ptr() == c.vel[1].data_ptr()
assert term.is_heading_env.dtype == torch.bool and term.is_standing_env.shape == (8,)
assert sorted(term.metrics) == ["error_vel_xy", "error_vel_yaw"] == sorted(term.last_episode_metrics)
assert term.cfg is cfg.commands.base_velocity and term.time_left.shape == term.command_counter.shape == (8,)
assert sorted(env._commands_get_state()) == sorted(c.STATE_KEYS)
s = str(m)
assert "<CommandManager> contains 2 active terms." in s and "Active Command Terms" in s
assert "UniformVelocityCommand" in s and "NormalVelocityCommand" in s and "base_velocity" in s
assert "Heading probability: 1.0" in str(term) and "Command dimension: (3,)" in str(term)
print("compat commands ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "compat commands ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_descriptor_rows_against_hand_values():
    """Every constant as the reference forms it: the ranges rounded to float32 and then subtracted (uniform_), the
    clip bounds, the stiffness and the probabilities rounded to float32, max_command_step divided in double."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.commands import term_row
    from allsteps_isaaclab_amd.utils import commands as CM

    f = np.float32
    lo, hi = 0.05, 0.18
    assert f(hi - lo) != f(hi) - f(lo)  # the two orders differ for this pair
    step_dt = 4 / 240
    cfg = _uniform(resampling_time_range=(lo, hi), heading_command=True, heading_control_stiffness=0.7,
                   rel_heading_envs=0.6, rel_standing_envs=0.15,
                   ranges=CM.UniformVelocityCommandCfg.Ranges(lin_vel_x=(-1.1, 1.3), lin_vel_y=(lo, hi),
                                                              ang_vel_z=(-0.8, 0.9), heading=(-3.1, 3.1)))
    row = term_row("t", cfg, step_dt)
    assert row.dtype == np.float32 and row.shape == (_native.COMMAND_TERM_WORDS,) == (21,)
    assert row[:2].view(np.int32).tolist() == [_native.COMMAND_UNIFORM, 1]
    assert row[2] == f(lo) and row[3] == f(hi) - f(lo)
    assert row[4:8].tolist() == [f(-1.1), f(lo), f(-0.8), f(-3.1)]
    assert row[8:12].tolist() == [f(1.3) - f(-1.1), f(hi) - f(lo), f(0.9) - f(-0.8), f(3.1) - f(-3.1)]
    assert (row[12], row[13], row[14], row[15], row[16]) == (f(-0.8), f(0.9), f(0.7), f(0.6), f(0.15))
    assert not row[17:20].any() and row[20] == f(hi / step_dt)
    plain = term_row("t", _uniform(), step_dt)  # no heading: its range and probability are not read
    assert plain[:2].view(np.int32).tolist() == [0, 0] and plain[7] == 0 and plain[11] == 0
    assert plain[3] == 0 and plain[20] == f(10.0 / step_dt)
    nrow = term_row("n", _normal(), step_dt)
    assert nrow[:2].view(np.int32).tolist() == [_native.COMMAND_NORMAL, 0]
    assert nrow[4:7].tolist() == [f(0.5), f(0.1), f(-0.3)] and nrow[8:11].tolist() == [f(0.4), f(0.25), f(0.6)]
    assert nrow[17:20].tolist() == [f(0.2), f(0.3), f(0.1)] and nrow[16] == f(0.1)
    assert nrow[2] == 5.0 and nrow[3] == 3.0 and nrow[20] == f(8.0 / step_dt)


def test_the_two_constructor_checks_of_the_reference():
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    with pytest.raises(ValueError, match=r"heading commands active \(heading_command=True\) but the `ranges.heading`"):
        DirectRLEnv(_cpu_cfg({"v": _uniform(heading_command=True)}))
    with pytest.warns(UserWarning, match="'ranges.heading' attribute set to .* but the heading command is not active"):
        DirectRLEnv(_cpu_cfg({"v": _uniform(heading=(-1.0, 1.0))}))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        DirectRLEnv(_cpu_cfg({"v": _uniform(heading=(-1.0, 1.0), heading_command=True)}))
        DirectRLEnv(_cpu_cfg({"v": _uniform()}))


def _refusals():
    from allsteps_isaaclab_amd.utils import commands as CM

    R = CM.UniformVelocityCommandCfg.Ranges
    NR = CM.NormalVelocityCommandCfg.Ranges

    class UniformPoseCommandCfg(CM.CommandTermCfg):
        pass

    return {
        "null": (CM.NullCommandCfg(), "NullCommandCfg has no command to serve"),
        "pose": (UniformPoseCommandCfg(resampling_time_range=(1.0, 2.0)),
                 "UniformPoseCommandCfg is not a served command term"),
        "asset": (_uniform(asset_name="cube"), "asset_name = 'cube' is not 'robot'"),
        "no ranges": (_uniform(ranges=CM.MISSING) if False else CM.UniformVelocityCommandCfg(
            asset_name="robot", resampling_time_range=(1.0, 2.0)), "ranges is not set"),
        "no time": (CM.UniformVelocityCommandCfg(asset_name="robot", ranges=R((0, 1), (0, 1), (0, 1))),
                    "resampling_time_range is not set"),
        "inverted time": (_uniform(resampling_time_range=(3.0, 1.0)), "hi < lo"),
        "infinite time": (_uniform(resampling_time_range=(1.0, math.inf)), "is not finite"),
        "bad time": (_uniform(resampling_time_range=(1.0,)), "resampling_time_range = .* is not a tuple of 2 numbers"),
        "missing range": (_uniform(ranges=R(lin_vel_x=(0.0, 1.0), lin_vel_y=(0.0, 1.0))), "ranges.ang_vel_z"),
        "inverted range": (_uniform(ranges=R((1.0, 0.0), (0, 1), (0, 1))), "ranges.lin_vel_x = .* has hi < lo"),
        "bad stiffness": (_uniform(heading_control_stiffness="stiff"), "heading_control_stiffness"),
        "bad probability": (_uniform(rel_standing_envs=None), "rel_standing_envs = None is not a number"),
        "short mean": (_normal(ranges=NR(mean_vel=(0.0, 0.0), std_vel=(1, 1, 1), zero_prob=(0, 0, 0))),
                       "ranges.mean_vel = .* is not a tuple of 3 numbers"),
        "negative std": (_normal(ranges=NR(mean_vel=(0, 0, 0), std_vel=(1, -1, 1), zero_prob=(0, 0, 0))),
                         "negative entry"),
    }


@pytest.mark.parametrize("what", ["null", "pose", "asset", "no ranges", "no time", "inverted time", "infinite time",
                                  "bad time", "missing range", "inverted range", "bad stiffness", "bad probability",
                                  "short mean", "negative std", "too many terms"])
def test_unsupported_terms_raise_at_construction_with_their_reason(what):
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    if what == "too many terms":
        commands = {f"v{i}": _uniform() for i in range(_native.MAX_COMMAND_TERMS + 1)}
        match = "5 terms.*at most AS_MAX_COMMAND_TERMS = 4"
    else:
        term, reason = _refusals()[what]
        commands = {"ok": _uniform(), "odd": term}
        match = f"'odd'.*{reason}"
    with pytest.raises(_native.NativeError, match=match) as ei:
        DirectRLEnv(_cpu_cfg(commands))
    if what != "too many terms":
        assert "supported: UniformVelocityCommandCfg(asset_name='robot'" in str(ei.value)
    commands.pop("odd", None)
    commands.pop("v4", None)
    assert len(DirectRLEnv(_cpu_cfg(commands))._commands.terms.names) == len(commands)


def test_a_term_that_is_no_command_term_cfg_is_a_type_error():
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    with pytest.raises(TypeError, match="term 'odd' is not of type CommandTermCfg"):
        DirectRLEnv(_cpu_cfg({"odd": {"ranges": None}}))


def test_term_cfg_round_trip_and_refresh_on_the_host():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.commands import term_row
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    first, second = _uniform(), _normal()
    cfg = _cpu_cfg({"a": first, "b": second})
    env = DirectRLEnv(cfg)
    m, c = env.command_manager, env._commands
    dt = env.step_dt
    assert m.get_term_cfg("a") is first and m.get_term("b").cfg is second
    ptr, before = c.desc.data_ptr(), c.desc.clone()
    new = _uniform(resampling_time_range=(1.0, 2.0))
    m.set_term_cfg("b", new)
    assert c.desc.data_ptr() == ptr and torch.equal(c.desc[0], before[0])
    assert np.array_equal(c.desc[1].numpy().view(np.uint32), term_row("b", new, dt).view(np.uint32))
    first.ranges.lin_vel_x = (-2.0, 3.0)  # a curriculum's in-place edit
    assert torch.equal(c.desc[0], before[0])
    m.refresh()
    assert c.desc.data_ptr() == ptr and float(c.desc[0, 4]) == -2.0 and float(c.desc[0, 8]) == 5.0
    with pytest.raises(ValueError, match="Command term 'c' not found"):
        m.set_term_cfg("c", new)
    with pytest.raises(_native.NativeError, match="'b'.*asset_name"):
        m.set_term_cfg("b", _uniform(asset_name="cube"))
    assert m.get_term_cfg("b") is new


def test_reseed_rekeys_the_stream_and_keeps_the_state():
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    cfg = _cpu_cfg({"a": _uniform()})
    cfg.seed = 7
    env = DirectRLEnv(cfg)
    env._commands.time_left.fill_(3.0)
    assert env._commands.seed == 7
    env._reseed(11)
    assert env._commands.seed == 11 and bool((env._commands.time_left == 3.0).all())
    st = env._commands_get_state()
    st["command_time_left"] = st["command_time_left"] + 1
    rest = env._commands_set_state({**st, "root_pos": 0})
    assert list(rest) == ["root_pos"] and bool((env._commands.time_left == 4.0).all())


def test_abi_exports_the_command_entry_points_and_checks_their_arguments():
    """Every refusal is made before any device call: null pointers, num_terms, n, dt."""
    from allsteps_isaaclab_amd import _native

    assert {"as_commands_step", "as_commands_reset"} <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    names = ("terms", "k", "quat", "lin", "ang", "vel", "heading", "flags", "tl", "counter", "metrics", "last", "t",
             "reset", "reset2", "n", "dt", "draws")

    def step(**kw):
        a = dict(zip(names, (p, 1, p, p, p, p, p, p, p, p, p, None, p, None, None, 4, 1.0 / 60, None)))
        a.update(kw)
        return L.as_commands_step(*(a[k] for k in names), 0, 0, None)

    rnames = ("terms", "k", "vel", "heading", "flags", "tl", "counter", "metrics", "last", "t", "mask", "n", "draws")

    def reset(**kw):
        a = dict(zip(rnames, (p, 1, p, p, p, p, p, p, None, p, None, 4, None)))
        a.update(kw)
        return L.as_commands_reset(*(a[k] for k in rnames), 0, 0, None)

    refusals = [(lambda k=k: step(**{k: None}), b"null") for k in ("terms", "quat", "lin", "ang", "vel", "heading",
                                                                    "flags", "tl", "counter", "metrics", "t")]
    refusals += [(lambda k=k: reset(**{k: None}), b"null") for k in ("terms", "vel", "heading", "flags", "tl",
                                                                     "counter", "metrics", "t")]
    refusals += [
        (lambda: step(k=0), b"num_terms 0"), (lambda: step(k=_native.MAX_COMMAND_TERMS + 1), b"num_terms 5"),
        (lambda: step(n=0), b"n 0"), (lambda: step(n=(1 << 24) + 1), b"AS_MAX_ENVS"), (lambda: step(dt=0.0), b"dt"),
        (lambda: step(dt=float("nan")), b"dt"), (lambda: step(dt=-0.1), b"dt"),
        (lambda: reset(k=0), b"num_terms 0"), (lambda: reset(k=5), b"num_terms 5"), (lambda: reset(n=-1), b"n -1"),
    ]
    for call, msg in refusals:
        rc = call()
        assert rc == -1, msg
        assert msg in L.as_last_error(), (msg, L.as_last_error())


def test_the_fixture_covers_what_it_claims():
    """The generator's own coverage conditions, restated on the committed fixture (the reference alone)."""
    from _commands_cases import load_cases

    cases = {c["name"]: c for c in load_cases()}
    a = cases["a"]
    rs, fl, vel = a["resampled"], a["flags"], a["vel"]
    assert a["steps"] >= 60 and rs.shape[2] == 2
    assert (rs.sum(axis=(0, 1)) >= 2).all()  # every env resamples at least twice in every term
    assert fl[:, 0, 0].mean() >= 0.25 and fl[:, :, 1].mean(axis=(0, 2)).min() >= 0.05  # heading, standing envs
    assert a["reset"].sum() >= 10 and (rs[:, 0] & rs[:, 1]).sum() >= 1  # resets, a double resample
    moving = (fl[:, 0, 0] == 1) & (fl[:, 0, 1] == 0)
    lo, hi = np.float32(-0.8), np.float32(0.9)
    assert (vel[:, 0, 2][moving] == hi).any() and (vel[:, 0, 2][moving] == lo).any()  # both clip bounds
    assert ((vel[:, 0, 2][moving] > lo) & (vel[:, 0, 2][moving] < hi)).any()
    b = cases["b"]
    assert b["rows"][0, :1].view(np.int32)[0] == 1 and b["flags"][:, 0, 1:].any(axis=(0, 2)).all()
    r = cases["c"]["resampled"][0, 1, 0]
    assert r[0] and r[1] and not r[2] and 0 < r[9:].sum() < r.size - 9  # exactly dt, one ulp either side
    d = cases["d"]
    assert d["resampled"][:, 1].all() and np.isinf(d["metrics"]).all()
    half_pi = np.float32(0.5) * np.float32(math.pi)
    assert (d["vel"][:, 0, 2] == half_pi).any() and (d["vel"][:, 0, 2] == -half_pi).any()  # the wrap's two ends


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout here")
def test_fixture_regenerates_byte_for_byte():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_commands.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
