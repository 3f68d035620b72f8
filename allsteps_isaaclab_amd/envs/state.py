"""The SoA device state of a native env (``as_state_t``, include/allsteps.h), allocated in one place."""

from __future__ import annotations

import torch

from .._native import STATE_LAYOUT

_DTYPES = {"f": torch.float32, "i": torch.int32}


def alloc_state(n: int, device, *, hind: bool = False, feet: bool = False) -> dict[str, torch.Tensor]:
    """Zeroed state of ``n`` envs, field -> tensor ([field][env], resident in HBM).  The ``STATE_LAYOUT`` fields
    are views of one fp32 and one int32 slab ``[rows][n]`` in layout order (a one-row field is the 1-D row);
    ``curriculum`` is a separate int32[1].  The quadruped's extras are separate too: ``hind`` adds
    ``contact_mask_hind`` (2, n) (sensors RH, LH), ``feet`` adds ``feet`` (8, n) (per-foot targets | reach counts)."""
    state: dict[str, torch.Tensor] = {}
    for t, dtype in _DTYPES.items():
        fields = [(name, rows) for name, rows, k in STATE_LAYOUT if k == t]
        slab = torch.zeros((sum(rows for _, rows in fields), n), dtype=dtype, device=device)
        o = 0
        for name, rows in fields:
            state[name] = slab[o:o + rows] if rows > 1 else slab[o]
            o += rows
    state["curriculum"] = torch.zeros(1, dtype=torch.int32, device=device)
    if hind:
        state["contact_mask_hind"] = torch.zeros((2, n), dtype=torch.int32, device=device)
    if feet:
        state["feet"] = torch.zeros((8, n), dtype=torch.int32, device=device)
    return state
