"""The host side of ``cfg.imu``: one ``ImuCfg`` or a dict of name -> ``ImuCfg``, checked against what the device
kernel serves and turned into the ``as_imu_table_t`` of one launch (no device needed).  ``views._ImuSet`` holds the
device buffers.

An IMU sits on any body of the model: the kernel runs the step's own forward kinematics for the body's pose and
centre-of-mass velocities (csrc/imu_kernels.h).  Everything the kernel does not serve is refused here with a
``NativeError`` that names the field.
"""

from __future__ import annotations

import math

from .. import _native

DEFAULT_NAME = "imu"  # the name of the single-cfg form: mdp.imu_*'s default SceneEntityCfg("imu")


def _refuse(name: str, field: str, detail: str) -> "_native.NativeError":
    where = "cfg.imu" if name == DEFAULT_NAME else f"cfg.imu[{name!r}]"
    return _native.NativeError(f"{where}.{field}: {detail}.  The sensor is updated by a HIP kernel on the robot's "
                               f"bodies (no host fallback)")


def named_cfgs(cfg) -> dict:
    """``cfg.imu`` as a dict name -> ImuCfg: a single cfg is registered as ``"imu"``."""
    if isinstance(cfg, dict):
        if len(cfg) == 0:
            raise _native.NativeError("cfg.imu: an empty dict names no sensor; use None for no IMU")
        for name in cfg:
            if not isinstance(name, str) or not name:
                raise _native.NativeError(f"cfg.imu: the key {name!r} is not a sensor name")
        return dict(cfg)
    return {DEFAULT_NAME: cfg}


class ImuSpec:
    """The checked sensors of a ``cfg.imu``: ``names``, ``bodies`` (index into ``model["body_names"]`` per sensor),
    ``cfgs`` and ``table()``, the ``as_imu_table_t`` of the launch that serves them all."""

    def __init__(self, cfg, *, model: dict, step_dt: float):
        cfgs = named_cfgs(cfg)
        if len(cfgs) > _native.MAX_IMUS:
            raise _native.NativeError(f"cfg.imu: {len(cfgs)} sensors; one launch of the HIP kernel serves at most "
                                      f"AS_MAX_IMUS = {_native.MAX_IMUS}")
        body_names = list(model["body_names"])
        self.names, self.cfgs, self.bodies = list(cfgs), list(cfgs.values()), []
        self._model = model
        for name, c in cfgs.items():
            path = getattr(c, "prim_path", None)
            if not isinstance(path, str) or not path:
                raise _refuse(name, "prim_path", f"{path!r} is not a prim path")
            leaf = path.split("/")[-1]
            if body_names.count(leaf) != 1:
                raise _refuse(name, "prim_path", f"{path!r} attaches the sensor to {leaf!r}, which is not exactly one "
                                                 f"of the robot's bodies {body_names}")
            self.bodies.append(body_names.index(leaf))
            period = float(getattr(c, "update_period", 0.0))
            if not period <= step_dt:
                raise _refuse(name, "update_period", f"{period!r} s is longer than the env step ({step_dt!r} s): the "
                                                     f"data would have to go stale across steps, and the sensor keeps "
                                                     f"no timestamp")
            history = getattr(c, "history_length", 0)
            if history != 0:
                raise _refuse(name, "history_length", f"{history!r} is not 0: a history forces an update per physics "
                                                      f"step (sensor_base.py:204), and the sensor is updated from the "
                                                      f"state between env steps")
            if getattr(c, "debug_vis", False):
                raise _refuse(name, "debug_vis", "True asks for visualization markers, which a headless env has not")
            offset = getattr(c, "offset", None)
            pos, rot = list(getattr(offset, "pos", ())), list(getattr(offset, "rot", ()))
            if len(pos) != 3 or len(rot) != 4 or not all(math.isfinite(float(x)) for x in pos + rot):
                raise _refuse(name, "offset", f"pos {pos!r} / rot {rot!r} is not a finite position and quaternion")
            bias = list(getattr(c, "gravity_bias", ()))
            if len(bias) != 3 or not all(math.isfinite(float(x)) for x in bias):
                raise _refuse(name, "gravity_bias", f"{bias!r} is not a finite 3-vector")

    num_sensors = property(lambda self: len(self.names))

    def table(self) -> "_native.AsImuTable":
        m, t = self._model, _native.AsImuTable()
        t.num_sensors = self.num_sensors
        for s, (c, b) in enumerate(zip(self.cfgs, self.bodies)):
            t.link[s] = int(m["body_link"][b])
            t.body_offset_pos[s][:] = [float(x) for x in m["body_offset_pos"][b]]
            t.body_offset_quat[s][:] = [float(x) for x in m["body_offset_quat"][b]]
            t.com[s][:] = [float(x) for x in m["body_com"][b]]
            t.offset_pos[s][:] = [float(x) for x in c.offset.pos]
            t.offset_rot[s][:] = [float(x) for x in c.offset.rot]
            t.gravity_bias[s][:] = [float(x) for x in c.gravity_bias]
        return t
