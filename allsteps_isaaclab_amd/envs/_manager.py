"""The host layer the env managers share (noise, events, commands, observations, rewards, terminations, actions).

What may live here: host code that two or more managers need in the same form and that never asks which manager it
serves -- a difference between managers is an argument or a class attribute of the caller, never a branch on the
caller.  The kernels, the descriptor words, the term parsers and every message's wording stay in the managers' own
modules.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..utils.events import SceneEntityCfg
from ..utils.observations import resolve_joint_ids
from ..utils.rewards import resolve_body_ids


def is_number(x) -> bool:
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool)


def u8(x):
    """A flag tensor as the kernels take it: contiguous uint8 (a bool tensor is viewed, not copied); None passes."""
    if x is None:
        return None
    x = x.view(torch.uint8) if x.dtype == torch.bool else x.to(torch.uint8)
    return x.contiguous()


def cfg_items(obj, term_type, *, private: str = "skip", class_attrs: bool = True, ignore: tuple = (), error=None):
    """Yield (name, term cfg) of a cfg object in cfg order.  A dict keeps its order; an object gives its instance
    attributes, then -- ``class_attrs`` -- its classes' attributes of ``term_type`` (a type or a tuple of types), base
    classes first, each name once, the first one met (the reference's configclass turns those into instance fields).

    None entries and the names in ``ignore`` are left out.  ``private`` says which names that begin with ``_`` are
    left out with them: ``"skip"`` all, ``"attrs"`` an object's only (every key of a dict counts), ``"keep"`` none.
    An entry that remains and is not of ``term_type`` raises ``error(name, value)``, by default the reference's
    TypeError; it is raised when the walk reaches the entry, after the entries before it were yielded."""
    if isinstance(obj, dict):
        items, drop_private = list(obj.items()), private == "skip"
    else:
        items, drop_private = list(vars(obj).items()), private != "keep"
        seen = {k for k, _ in items}
        for klass in reversed(type(obj).__mro__[:-1]) if class_attrs else ():
            for k, v in vars(klass).items():
                if k not in seen and not k.startswith("_") and isinstance(v, term_type):
                    items.append((k, v))
                    seen.add(k)
    for name, v in items:
        if v is None or name in ignore or (drop_private and name.startswith("_")):
            continue
        if not isinstance(v, term_type):
            if error is not None:
                raise error(name, v)
            raise TypeError(f"Configuration for the term '{name}' is not of type {term_type.__name__}. Received: "
                            f"'{type(v)}'.")
        yield name, v


class DeviceState:
    """A part of an env whose state is a fixed set of device tensors: ``tensors()`` names them, and the env's
    get_state / set_state go through the three methods below.  A class says which keys are its own by
    ``STATE_KEYS`` (a closed set) or by ``STATE_PREFIX`` (every key that begins with it)."""

    STATE_KEYS: tuple = ()
    STATE_PREFIX: str | None = None

    def tensors(self) -> dict:
        """{key: device tensor} of what exists in this object (keys only for what exists)."""
        raise NotImplementedError

    @classmethod
    def owns(cls, key: str) -> bool:
        """Whether ``key`` is a state key of this class -- of an object the env has or of one it was built without."""
        return key in cls.STATE_KEYS if cls.STATE_PREFIX is None else key.startswith(cls.STATE_PREFIX)

    def get_state(self) -> dict:
        return {k: v.clone() for k, v in self.tensors().items()}

    def set_state(self, state: dict) -> bool:
        """Load the keys of ``state`` that this object has, whatever their dtype, shape or device; the others are
        left alone.  Returns whether a key was loaded."""
        loaded = False
        for k, v in self.tensors().items():
            if k in state:
                v.copy_(torch.as_tensor(state[k]).to(v.device, v.dtype).reshape(v.shape))
                loaded = True
        return loaded


# ---------------------------------------------------------------------- events, commands: one descriptor row per term
class RowTerms:
    """Base of EventTerms / CommandTerms: ``names``, ``cfgs`` and the descriptor ``rows`` (terms, WORDS) of a cfg,
    checked (no device needed).  A subclass gives ``row(name, cfg)`` and the four attributes below."""

    NOUN = ""  # "event": cfg.events, the event kernel, "Event term '...' not found."
    TERM_TYPE: type = object
    WORDS = 0
    LIMIT = ("", 0)  # the kernel's most terms: the macro's name and its value

    def __init__(self, cfg):
        terms = list(cfg_items(cfg, self.TERM_TYPE))
        macro, most = self.LIMIT
        if len(terms) > most:
            raise _native.NativeError(f"cfg.{self.NOUN}s has {len(terms)} terms ({[k for k, _ in terms]}); the "
                                      f"{self.NOUN} kernel takes at most {macro} = {most}")
        self.names = [k for k, _ in terms]
        self.cfgs = [c for _, c in terms]
        self.rows = np.stack([self.row(k, c) for k, c in terms]) if terms else np.zeros((0, self.WORDS), np.float32)

    def row(self, name: str, cfg) -> np.ndarray:
        raise NotImplementedError

    def index(self, term_name: str) -> int:
        if term_name not in self.names:
            raise ValueError(f"{self.NOUN.capitalize()} term '{term_name}' not found.")
        return self.names.index(term_name)

    def set(self, term_name: str, cfg) -> int:
        k = self.index(term_name)
        self.rows[k] = self.row(term_name, cfg)
        self.cfgs[k] = cfg
        return k


# ---------------------------------------------------------------------- rewards, terminations: the term table
@dataclass
class SensorInfo:
    """A contact sensor as the terms address it: its bodies' names, and per body the row of the net forces and --
    where the terms read them -- of the timers."""

    body_names: list
    net_bodies: list  # body b of the sensor -> body row of the contact report's net impulses
    timer_bodies: list | None = None  # body b of the sensor -> body row of the contact timers


def check_params(unsupported, params: dict, required: tuple, optional: tuple, t: str) -> None:
    extra = sorted(set(params) - set(required) - set(optional))
    if extra:
        raise unsupported(t, f"params {extra} are not parameters of the term function (it takes "
                             f"{list(required + optional)})")
    missing = [k for k in required if k not in params]
    if missing:
        raise unsupported(t, f"the term function needs params {missing}")


def number(unsupported, x, key: str, t: str) -> np.float32:
    """A Python scalar as torch takes it in an operation with a float32 tensor."""
    if not is_number(x):
        raise unsupported(t, f"{key} = {x!r} is not a number")
    return np.float32(x)


def robot_asset(unsupported, params: dict, t: str):
    """params['asset_cfg'], which must name the robot; without one, the whole robot."""
    asset = params.get("asset_cfg", None)
    if asset is None:
        return SceneEntityCfg("robot")
    if not hasattr(asset, "name"):
        raise unsupported(t, f"params['asset_cfg'] = {asset!r} is not a SceneEntityCfg")
    if asset.name != "robot":
        raise unsupported(t, f"asset_cfg.name = {asset.name!r} is not 'robot' (the env's articulation)")
    return asset


def joint_ids(unsupported, asset, joint_names: list, t: str) -> list:
    """The joints an asset cfg selects, as indices; a selection of none is refused."""
    try:
        ids = resolve_joint_ids(asset, joint_names, "asset_cfg")
    except ValueError as e:
        raise unsupported(t, str(e)) from None
    ids = list(range(len(joint_names))) if ids is None else ids
    if not ids:
        raise unsupported(t, "asset_cfg selects no joint")
    return ids


def sensor_bodies(unsupported, params: dict, ctx, t: str, timers: bool = False) -> list:
    """The rows of the net forces (or of the timers) that sensor_cfg's bodies read."""
    if timers and not ctx.contact_air_time:
        raise unsupported(t, "the term reads the contact sensors' air / contact timers: set cfg.contact_air_time")
    if not timers and not ctx.contact_forces:
        raise unsupported(t, "the term reads the contact sensors' net forces: set cfg.contact_forces")
    sensor = params.get("sensor_cfg", None)
    sname = getattr(sensor, "name", None)
    if sname not in ctx.sensors:
        raise unsupported(t, f"sensor_cfg names the sensor {sname!r}; the env has the contact sensors "
                             f"{sorted(ctx.sensors)}")
    info = ctx.sensors[sname]
    try:
        ids = resolve_body_ids(sensor, info.body_names, "sensor_cfg")
    except ValueError as e:
        raise unsupported(t, str(e)) from None
    ids = list(range(len(info.body_names))) if ids is None else ids
    if not ids:
        raise unsupported(t, "sensor_cfg selects no body")
    rows = info.timer_bodies if timers else info.net_bodies
    return [int(rows[k]) for k in ids]


class TermTable:
    """Base of RewardTerms / TerminationTerms: the terms of a cfg in cfg order, checked (no device needed), and the
    device tables as host arrays -- the descriptor ``rows`` (terms, WORDS), the index ``table`` (its rows 0..2: a
    term's ids, a and b) and the ``kinds`` mask.  A subclass gives the attributes below and ``pack`` / ``column``;
    a term spec has name, cfg, kind, ids, a and b."""

    NOUN = ""  # "Reward": <RewardManager>, "Reward term '...' not found.", the reward kernel
    TERM_TYPE: type = object
    KINDS: tuple = ()  # the kinds' names, by kind
    WORDS = 0
    TABLE = (0, 0, 0)  # (table rows, most terms, most ids)
    LIMIT = ""  # the macro that names the most terms
    COLUMN = ("", str.center)  # the third column of __str__: its header and its cells' alignment
    MAY_CHANGE = ""  # what set_term_cfg may change, for its refusal
    parse_term = unsupported = None  # the module's own (staticmethod)

    def __init__(self, cfg, ctx):
        self.ctx = ctx
        self.terms = [self.parse_term(name, c, ctx) for name, c in cfg_items(cfg, self.TERM_TYPE, private="attrs")]
        if not self.terms:
            raise self.unsupported(None, "there are no terms")
        if len(self.terms) > self.TABLE[1]:
            raise self.unsupported(None, f"{len(self.terms)} terms; the {self.NOUN.lower()} kernel takes at most "
                                         f"{self.LIMIT} = {self.TABLE[1]}")
        self.build()

    names = property(lambda self: [t.name for t in self.terms])

    def pack(self, row: np.ndarray, ints: np.ndarray, t) -> None:
        """Fill a term's descriptor words: ``row`` as float32, ``ints`` the same words as int32."""
        raise NotImplementedError

    def column(self, t) -> str:
        raise NotImplementedError

    def build(self) -> None:
        """The descriptor rows, the index table and the kinds mask from the term specs as they stand."""
        f32, i32 = np.float32, np.int32
        rows = np.zeros((len(self.terms), self.WORDS), f32)
        table = np.zeros(self.TABLE, f32)
        self.kinds = 0
        for k, t in enumerate(self.terms):
            self.pack(rows[k], rows[k].view(i32), t)
            table[0, k, :len(t.ids)] = np.asarray(t.ids, i32).view(f32)
            table[1, k, :len(t.a)] = t.a
            table[2, k, :len(t.b)] = t.b
            self.kinds |= 1 << t.kind
        self.rows, self.table = rows, table

    def index(self, term_name: str) -> int:
        if term_name not in self.names:
            raise ValueError(f"{self.NOUN} term '{term_name}' not found.")
        return self.names.index(term_name)

    def uses(self, *kinds: str) -> bool:
        return any(self.KINDS[t.kind] in kinds for t in self.terms)

    def replace(self, term_name: str, cfg, desc: torch.Tensor, table: torch.Tensor) -> None:
        """set_term_cfg: parse the new cfg, rebuild the tables and copy them into the device tensors in place; a
        cfg with another term function is refused."""
        k = self.index(term_name)
        new, old = self.parse_term(term_name, cfg, self.ctx), self.terms[k]
        if new.kind != old.kind:  # (the sources a launch is given, a captured one too, follow the kinds)
            raise self.unsupported(term_name, f"the new cfg changes the term's function from {self.KINDS[old.kind]} "
                                              f"to {self.KINDS[new.kind]}; the terms' functions are fixed at "
                                              f"construction ({self.MAY_CHANGE} may change)")
        self.terms[k] = new
        self.build()
        desc.copy_(torch.as_tensor(self.rows.copy()))
        table.copy_(torch.as_tensor(self.table.copy()))

    def table_str(self) -> str:
        """The manager's __str__ in the reference's form."""
        rows = [(str(i), t.name, self.column(t)) for i, t in enumerate(self.terms)]
        head, align = ("Index", "Name", self.COLUMN[0]), self.COLUMN[1]
        w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
        line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
        total = len(line) - 3
        fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), align(r[2], w[2]))) + " |\n"  # noqa: E731
        msg = f"<{self.NOUN}Manager> contains {len(rows)} active terms.\n"
        msg += "+" + "-" * total + "+\n" + "|" + f"Active {self.NOUN} Terms".center(total) + "|\n"
        msg += line + "| " + " | ".join(h.center(x) for h, x in zip(head, w)) + " |\n" + line
        return msg + "".join(fmt(r) for r in rows) + line
