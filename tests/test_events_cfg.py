"""The interval events' Python surface, no GPU: the cfg field, the reference-named cfg classes through the compat
imports, the refusal of everything the device kernel does not serve (each with its reason), the host side of
set_term_cfg / get_term_cfg, the C ABI's new names and argument checks, and the fixture's regeneration."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"


def _push(**kw):
    from allsteps_isaaclab_amd.utils import events as E

    d = dict(func=E.push_by_setting_velocity, mode="interval", interval_range_s=(10.0, 15.0),
             params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})
    d.update(kw)
    return E.EventTermCfg(**d)


def _cpu_cfg(events=None, n=4):
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.sim.device = "cpu"
    cfg.scene.num_envs = n
    cfg.events = events
    return cfg


def test_cfg_field_defaults_to_none_and_costs_nothing():
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    for cfg in (AllstepsEnvCfg(), AnymalCStonesEnvCfg()):
        assert cfg.events is None
    env = DirectRLEnv(_cpu_cfg())
    assert env._events is None and not hasattr(env, "event_manager")
    assert env._events_get_state() == {}


def test_cfg_classes_carry_the_reference_fields_and_defaults():
    from allsteps_isaaclab_amd.utils import events as E

    t = E.EventTermCfg()
    assert t.func is E.MISSING and t.mode is E.MISSING and t.params == {}
    assert (t.interval_range_s, t.is_global_time, t.min_step_count_between_reset) == (None, False, 0)
    assert E.EventTermCfg().params is not t.params
    s = E.SceneEntityCfg("robot")
    assert s.name == "robot" and s.body_names is None and s.joint_names is None
    assert s.body_ids == slice(None) and s.joint_ids == slice(None) and s.preserve_order is False
    assert s.whole() and not E.SceneEntityCfg("robot", body_names="base").whole()
    with pytest.raises(NotImplementedError, match="no host implementation"):
        E.push_by_setting_velocity(None, None, velocity_range={})


def test_reference_style_cfg_through_the_compat_imports():
    """A reference locomotion cfg's event block (velocity_env_cfg.py), written against isaaclab.managers and
    isaaclab.envs.mdp, builds the env's device state (on the CPU here: tensors only, no launch)."""
    code = """
from allsteps_isaaclab_amd import compat
compat.install()
import numpy as np, torch
from isaaclab.managers import EventTermCfg as EventTerm
from isaaclab.managers import SceneEntityCfg
import isaaclab.envs.mdp as mdp
from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

class EventCfg:
    push_robot = EventTerm(func=mdp.push_by_setting_velocity, mode="interval", interval_range_s=(10.0, 15.0),
                           params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})
    base_push = EventTerm(func=mdp.push_by_setting_velocity, mode="interval", interval_range_s=(0.1, 0.3),
                          params={"velocity_range": {"yaw": (-0.1, 0.2)}, "asset_cfg": SceneEntityCfg("robot")})
    disabled = None

cfg = AllstepsEnvCfg()
cfg.sim.device = "cpu"
cfg.scene.num_envs = 8
cfg.events = EventCfg()
env = DirectRLEnv(cfg)
ev, m = env._events, env.event_manager
assert m.active_terms == {"interval": ["push_robot", "base_push"]} and m.available_modes == ["interval"]
assert ev.desc.shape == (2, 14) and ev.time_left.shape == (2, 8) and ev.t.shape == (8,) and ev.fired.shape == (2, 8)
assert ev.t.dtype == torch.int32 and ev.fired.dtype == torch.uint8 and m.last_triggered.dtype == torch.bool
assert ev.dt == float(np.float32(cfg.sim.dt * cfg.decimation))
assert sorted(env._events_get_state()) == ["event_t", "event_time_left"]
assert "push_robot" in str(m) and "(10.0, 15.0)" in str(m) and "interval" in str(m)
print("compat events ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "compat events ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_widths_follow_torch_the_interval_in_double_the_velocity_in_float32():
    """w = float32(double(hi) - double(lo)) for the interval (rand * (upper - lower) with Python floats),
    w = float32(hi) - float32(lo) for the velocity (the ranges pass through torch.tensor); the values below
    are chosen so that the two orders differ."""
    from allsteps_isaaclab_amd.envs.events import term_row

    lo, hi = 0.05, 0.18
    f = np.float32
    assert f(hi - lo) != f(hi) - f(lo)
    row = term_row("t", _push(interval_range_s=(lo, hi), params={"velocity_range": {"roll": (lo, hi)}}))
    assert row.dtype == np.float32 and row.shape == (14,)
    assert row[0] == f(lo) and row[1] == f(hi - lo)
    assert row[2 + 3] == f(lo) and row[8 + 3] == f(hi) - f(lo)
    ranges = torch.tensor([(lo, hi)])
    assert float(row[8 + 3]) == float(ranges[0, 1] - ranges[0, 0])
    assert not row[[2, 3, 4, 6, 7, 8, 9, 10, 12, 13]].any()  # a missing key is (0.0, 0.0)


def _other(env, env_ids):
    pass


def apply_external_force_torque(env, env_ids, force_range=(0, 0), torque_range=(0, 0)):
    pass


REFUSALS = {
    "startup": (dict(mode="startup"), "per-env model tables"),
    "reset": (dict(mode="reset"), "the task's own reset overwrites"),
    "other mode": (dict(mode="on_demand"), "mode = 'on_demand'"),
    "global time": (dict(is_global_time=True), "env_ids = None"),
    "other func": (dict(func=_other), "func = _other is not a served event function"),
    "external force": (dict(func=apply_external_force_torque), "acts inside the physics substeps"),
    "missing func": (dict(func=None), "not a served event function"),
    "no interval": (dict(interval_range_s=None), "interval_range_s is not specified"),
    "inverted interval": (dict(interval_range_s=(3.0, 1.0)), "hi < lo"),
    "bad interval": (dict(interval_range_s=(1.0,)), "not a .lo, hi. pair"),
    "no velocity_range": (dict(params={}), "params lack 'velocity_range'"),
    "extra param": (dict(params={"velocity_range": {}, "force_range": (0, 1)}), "force_range"),
    "bad range": (dict(params={"velocity_range": {"x": "fast"}}), r"velocity_range\['x'\]"),
}


@pytest.mark.parametrize("what", list(REFUSALS) + ["asset name", "asset part", "too many terms"])
def test_unsupported_terms_raise_at_construction_with_their_reason(what):
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.utils import events as E

    if what == "asset name":
        events = {"shove": _push(params={"velocity_range": {}, "asset_cfg": E.SceneEntityCfg("cube")})}
        match = "shove.*is not the whole 'robot'"
    elif what == "asset part":
        events = {"shove": _push(params={"velocity_range": {}, "asset_cfg": E.SceneEntityCfg("robot", body_names="torso")})}
        match = "shove.*is not the whole 'robot'"
    elif what == "too many terms":
        events = {f"push{i}": _push() for i in range(_native.MAX_EVENT_TERMS + 1)}
        match = "5 terms.*at most AS_MAX_EVENT_TERMS = 4"
    else:
        kw, reason = REFUSALS[what]
        if kw.get("func", 0) is None:
            kw = dict(kw, func=E.MISSING)
        events = {"ok": _push(), "shove": _push(**kw)}
        match = f"'shove'.*{reason}"
    with pytest.raises(_native.NativeError, match=match) as ei:
        DirectRLEnv(_cpu_cfg(events))
    if what != "too many terms":
        assert "supported: EventTermCfg(func=push_by_setting_velocity, mode='interval'" in str(ei.value)
    # the same terms without the refused one build
    events.pop("shove", None)
    events.pop("push4", None)
    assert len(DirectRLEnv(_cpu_cfg(events))._events.terms.names) == len(events)


def test_a_term_that_is_no_event_term_cfg_is_a_type_error():
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    with pytest.raises(TypeError, match="term 'shove' is not of type EventTermCfg"):
        DirectRLEnv(_cpu_cfg({"shove": {"func": "push"}}))


def test_term_cfg_round_trip_on_the_host():
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv
    from allsteps_isaaclab_amd.envs.events import term_row

    first, second = _push(), _push(interval_range_s=(0.5, 0.75), params={"velocity_range": {"z": (0.0, 1.0)}})
    env = DirectRLEnv(_cpu_cfg({"a": first, "b": second}))
    m = env.event_manager
    assert m.get_term_cfg("a") is first and m.get_term_cfg("b") is second
    before = env._events.desc.clone()
    new = _push(interval_range_s=(1.0, 2.0), params={"velocity_range": {"yaw": (-1.0, 1.0)}})
    m.set_term_cfg("b", new)
    assert m.get_term_cfg("b") is new and m.get_term_cfg("a") is first
    assert torch.equal(env._events.desc[0], before[0])
    assert np.array_equal(env._events.desc[1].numpy(), term_row("b", new))
    with pytest.raises(ValueError, match="Event term 'c' not found"):
        m.get_term_cfg("c")
    with pytest.raises(ValueError, match="Event term 'c' not found"):
        m.set_term_cfg("c", new)
    with pytest.raises(_native.NativeError, match="'b'.*per-env model tables"):
        m.set_term_cfg("b", _push(mode="startup"))
    assert m.get_term_cfg("b") is new and np.array_equal(env._events.desc[1].numpy(), term_row("b", new))


def test_set_term_cfg_writes_the_tensor_the_kernel_reads():
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    env = DirectRLEnv(_cpu_cfg({"a": _push()}))
    ptr = env._events.desc.data_ptr()
    env.event_manager.set_term_cfg("a", _push(interval_range_s=(1.0, 2.0)))
    assert env._events.desc.data_ptr() == ptr and float(env._events.desc[0, 0]) == 1.0


def test_reseed_rekeys_the_stream_and_keeps_the_timers():
    from allsteps_isaaclab_amd.envs.direct_rl_env import DirectRLEnv

    cfg = _cpu_cfg({"a": _push()})
    cfg.seed = 7
    env = DirectRLEnv(cfg)
    env._events.time_left.fill_(3.0)
    assert env._events.seed == 7
    env._reseed(11)
    assert env._events.seed == 11 and bool((env._events.time_left == 3.0).all())


def test_abi_exports_the_event_entry_points_and_checks_their_arguments():
    """Every refusal is made before any device call: null pointers, num_terms, n, dt."""
    from allsteps_isaaclab_amd import _native

    assert {"as_events_init", "as_events_interval"} <= set(_native.EXPORTED_SYMBOLS)
    L = _native.load()
    assert L.as_abi_version() == 6 == _native.ABI_VERSION
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data

    def init(terms=p, k=1, tl=p, t=p, n=4):
        return L.as_events_init(terms, k, tl, t, n, None, 0, 0, None)

    def interval(terms=p, k=1, lin=p, ang=p, tl=p, t=p, n=4, dt=1.0 / 60):
        return L.as_events_interval(terms, k, lin, ang, tl, t, None, n, dt, None, None, 0, 0, None)

    refusals = [
        (lambda: init(terms=None), b"null"), (lambda: init(tl=None), b"null"), (lambda: init(t=None), b"null"),
        (lambda: init(k=0), b"num_terms 0"), (lambda: init(k=5), b"num_terms 5"), (lambda: init(n=0), b"n 0"),
        (lambda: interval(terms=None), b"null"), (lambda: interval(lin=None), b"null"),
        (lambda: interval(ang=None), b"null"), (lambda: interval(tl=None), b"null"),
        (lambda: interval(t=None), b"null"), (lambda: interval(k=0), b"num_terms 0"),
        (lambda: interval(k=_native.MAX_EVENT_TERMS + 1), b"num_terms 5"), (lambda: interval(n=-1), b"n -1"),
        (lambda: interval(n=(1 << 24) + 1), b"AS_MAX_ENVS"), (lambda: interval(dt=0.0), b"dt"),
        (lambda: interval(dt=float("nan")), b"dt"), (lambda: interval(dt=-0.1), b"dt"),
    ]
    for call, msg in refusals:
        rc = call()
        assert rc == -1, msg
        assert msg in L.as_last_error(), (msg, L.as_last_error())


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout here")
def test_fixture_regenerates_byte_for_byte():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_events.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
