"""The host side of ``cfg.frame_transformer``: one ``FrameTransformerCfg`` or a dict of name -> cfg, checked against
what the device kernel serves and turned into frame names and the ``as_frame_table_t`` of one launch (no device
needed).  ``views._FrameTransformerSet`` holds the device buffers.

A frame sits on a body of the robot or on a stone of the env.  A prim path is resolved by its leaf, the text after
the last ``/``, taken as a regular expression (``re.fullmatch``): against the robot's ``body_names`` when the
parent path contains ``/Robot``, against the stone names ``step_0 .. step_{num_steps-1}`` when the parent is the env
namespace itself (``{ENV_REGEX_NS}`` or ``/World/envs/env_.*``; the reference's stones are
``/World/envs/env_.*/step_<i>``).  The source must match exactly one body or stone; a target may match several, and
each match becomes a frame named ``FrameCfg.name``, or the body's name when that is None.

*Frame order* (frame_transformer.py:233-293): the tracked bodies sorted by prim path as strings, and for each body
its frames.  Here the sort key is (robot before stone, leaf as a Python string) -- the reference's key wherever the
robot's bodies share a parent, because ``"/Robot..." < "/step_..."``.  So ``step_10`` comes before ``step_2`` and
``LF_SHANK`` before ``base``, and the order of the cfg's list does not matter between bodies.  The source body is
among the targets only if some target path matches it (the reference's ``_source_is_also_target_frame``).
*One decided deviation:* where several frames sit on one body the reference iterates a Python ``set`` of their
names, whose order changes from process to process; here they come in the order of ``target_frames``.

*The two switches* are formed as the reference forms them (frame_transformer.py:105-113, 182-189; math.py:728-746):
``apply_source_offset`` unless ``torch.allclose`` holds the float32 offset to the identity pose (rtol 1e-5, atol
1e-8); ``apply_target_offset`` per sensor, if any of its frames' offsets is not identity by the same test -- then
every frame's offset is applied, identity ones included.

Everything the kernel does not serve is refused here with a ``NativeError`` that names the field.
"""

from __future__ import annotations

import math
import re

import torch

from .. import _native

DEFAULT_NAME = "frame_transformer"  # the name of the single-cfg form
ENV_NS = ("{ENV_REGEX_NS}", "/World/envs/env_.*")


def _where(name: str) -> str:
    return "cfg.frame_transformer" if name == DEFAULT_NAME else f"cfg.frame_transformer[{name!r}]"


def _refuse(name: str, field: str, detail: str) -> "_native.NativeError":
    return _native.NativeError(f"{_where(name)}.{field}: {detail}.  The frames are formed by a HIP kernel on the "
                               f"robot's bodies and the env's stones (no host fallback)")


def named_cfgs(cfg) -> dict:
    """``cfg.frame_transformer`` as a dict name -> FrameTransformerCfg: a single cfg is registered as
    ``"frame_transformer"``."""
    if isinstance(cfg, dict):
        if len(cfg) == 0:
            raise _native.NativeError("cfg.frame_transformer: an empty dict names no sensor; use None for no frame "
                                      "transformer")
        for name in cfg:
            if not isinstance(name, str) or not name:
                raise _native.NativeError(f"cfg.frame_transformer: the key {name!r} is not a sensor name")
        return dict(cfg)
    return {DEFAULT_NAME: cfg}


def is_identity_pose(pos, rot) -> bool:
    """math.py:728-746 on float32 tensors, as the reference calls it."""
    p, r = torch.tensor([float(x) for x in pos]), torch.tensor([float(x) for x in rot])
    return bool(torch.allclose(p, torch.zeros_like(p)) and torch.allclose(r, torch.tensor([1.0, 0.0, 0.0, 0.0])))


def _offset(name: str, field: str, offset):
    pos, rot = list(getattr(offset, "pos", ())), list(getattr(offset, "rot", ()))
    try:
        ok = len(pos) == 3 and len(rot) == 4 and all(math.isfinite(float(x)) for x in pos + rot)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise _refuse(name, field, f"pos {pos!r} / rot {rot!r} is not a finite position and quaternion")
    return tuple(float(x) for x in pos), tuple(float(x) for x in rot)


class FrameTransformerSpec:
    """The checked sensors of a ``cfg.frame_transformer``.  Per sensor s: ``names[s]``, ``cfgs[s]``, ``sources[s]``
    (a body), ``apply_source[s]`` / ``apply_target[s]`` (the two switches), ``frame_names[s]``, ``frames[s]`` (per
    target frame, in the module docstring's order: (body, offset pos, offset rot)) and ``slices[s]``, its frames'
    range in the launch's F = ``num_frames`` lanes.  A body is ``("robot", index into model["body_names"], name)`` or
    ``("stone", stone index, name)``.  ``table()`` is the ``as_frame_table_t`` of the launch that serves them all."""

    def __init__(self, cfg, *, model: dict, num_steps: int, step_dt: float):
        cfgs = named_cfgs(cfg)
        if len(cfgs) > _native.MAX_FRAME_TRANSFORMERS:
            raise _native.NativeError(f"cfg.frame_transformer: {len(cfgs)} sensors; one launch of the HIP kernel serves "
                                      f"at most AS_MAX_FRAME_TRANSFORMERS = {_native.MAX_FRAME_TRANSFORMERS}")
        self._model = model
        self._bodies = [str(b) for b in model["body_names"]]
        self._stones = [f"step_{i}" for i in range(int(num_steps))]
        self.names, self.cfgs = list(cfgs), list(cfgs.values())
        self.sources, self.source_offsets, self.apply_source, self.apply_target = [], [], [], []
        self.frame_names, self.frames, self.slices = [], [], []
        total = 0
        for name, c in cfgs.items():
            self._resolve(name, c, step_dt)
            count = len(self.frames[-1])
            self.slices.append(slice(total, total + count))
            total += count
        if total > _native.MAX_FRAMES:
            raise _native.NativeError(f"cfg.frame_transformer: {total} target frames over the env's sensors; one launch "
                                      f"of the HIP kernel serves at most AS_MAX_FRAMES = {_native.MAX_FRAMES} (a lane "
                                      f"each)")

    num_sensors = property(lambda self: len(self.names))
    num_frames = property(lambda self: sum(len(f) for f in self.frames))

    def _match(self, name: str, field: str, path) -> list:
        """The bodies a prim path matches, as (kind, index, leaf)."""
        if not isinstance(path, str) or not path:
            raise _refuse(name, field, f"{path!r} is not a prim path")
        parent, _, leaf = path.rpartition("/")
        if "/Robot" in parent:
            kind, pool = "robot", self._bodies
        elif parent in ENV_NS:
            kind, pool = "stone", self._stones
        else:
            raise _refuse(name, field, f"{path!r} matches nothing: a frame sits on a body of the robot "
                                       f"('.../Robot/<body>') or on a stone of the env ('{ENV_NS[0]}/step_<i>')")
        try:
            pattern = re.compile(leaf)
        except re.error as err:
            raise _refuse(name, field, f"{path!r}: the leaf {leaf!r} is not a regular expression ({err})") from None
        found = [(kind, i, b) for i, b in enumerate(pool) if pattern.fullmatch(b)]
        if not found:
            raise _refuse(name, field, f"{path!r} matches nothing: no {'body' if kind == 'robot' else 'stone'} of "
                                       f"{pool} has the name {leaf!r}")
        return found

    def _resolve(self, name: str, c, step_dt: float) -> None:
        source = self._match(name, "prim_path", getattr(c, "prim_path", None))
        if len(source) != 1:
            raise _refuse(name, "prim_path", f"{c.prim_path!r} matches {len(source)} bodies "
                                             f"({[b for _, _, b in source]}); the source frame sits on exactly one")
        period = float(getattr(c, "update_period", 0.0))
        if not period <= step_dt:
            raise _refuse(name, "update_period", f"{period!r} s is longer than the env step ({step_dt!r} s): the data "
                                                 f"would have to go stale across steps, and the sensor keeps no "
                                                 f"timestamp")
        history = getattr(c, "history_length", 0)
        if history != 0:
            raise _refuse(name, "history_length", f"{history!r} is not 0: a history forces an update per physics step "
                                                  f"(sensor_base.py:204), and the sensor is updated from the state "
                                                  f"between env steps")
        if getattr(c, "debug_vis", False):
            raise _refuse(name, "debug_vis", "True asks for visualization markers, which a headless env has not")
        src_off = _offset(name, "source_frame_offset", getattr(c, "source_frame_offset", None))
        targets = getattr(c, "target_frames", None)
        if not isinstance(targets, (list, tuple)) or len(targets) == 0:
            raise _refuse(name, "target_frames", f"{targets!r} names no target frame")
        per_body: dict = {}  # (kind order, leaf) -> [body, [frame names in cfg order]]
        offsets: dict = {}  # frame name -> (pos, rot)
        apply_target = False
        for i, t in enumerate(targets):
            field = f"target_frames[{i}]"
            off = _offset(name, f"{field}.offset", getattr(t, "offset", None))
            apply_target = apply_target or not is_identity_pose(*off)
            frame = getattr(t, "name", None)
            if frame is not None and (not isinstance(frame, str) or not frame):
                raise _refuse(name, f"{field}.name", f"{frame!r} is not a frame name")
            for body in self._match(name, f"{field}.prim_path", getattr(t, "prim_path", None)):
                frame_name = body[2] if frame is None else frame
                if offsets.setdefault(frame_name, off) != off:
                    raise _refuse(name, f"{field}.offset", f"the frame name {frame_name!r} is already taken by a target "
                                                           f"frame with another offset (the reference would silently "
                                                           f"keep the last)")
                names = per_body.setdefault((body[0] == "stone", body[2]), [body, []])[1]
                if frame_name not in names:
                    names.append(frame_name)
        frames = [(body, *offsets[f]) for _, (body, names) in sorted(per_body.items()) for f in names]
        self.sources.append(source[0])
        self.source_offsets.append(src_off)
        self.apply_source.append(not is_identity_pose(*src_off))
        self.apply_target.append(apply_target)
        self.frame_names.append([f for _, (_, names) in sorted(per_body.items()) for f in names])
        self.frames.append(frames)

    def _fill(self, entry, body, pos, rot) -> None:
        m = self._model
        kind, i, _ = body
        if kind == "robot":
            entry.link, entry.stone = int(m["body_link"][i]), -1
            entry.body_offset_pos[:] = [float(x) for x in m["body_offset_pos"][i]]
            entry.body_offset_quat[:] = [float(x) for x in m["body_offset_quat"][i]]
        else:
            entry.link, entry.stone = -1, int(i)
            entry.body_offset_pos[:] = [0.0, 0.0, 0.0]
            entry.body_offset_quat[:] = [1.0, 0.0, 0.0, 0.0]
        entry.offset_pos[:] = pos
        entry.offset_rot[:] = rot

    def table(self) -> "_native.AsFrameTable":
        t = _native.AsFrameTable()
        t.num_sensors, t.num_frames = self.num_sensors, self.num_frames
        f = 0
        for s in range(self.num_sensors):
            t.apply_source_offset[s] = int(self.apply_source[s])
            t.apply_target_offset[s] = int(self.apply_target[s])
            self._fill(t.source[s], self.sources[s], *self.source_offsets[s])
            for body, pos, rot in self.frames[s]:
                self._fill(t.target[f], body, pos, rot)
                t.sensor[f] = s
                f += 1
        return t
