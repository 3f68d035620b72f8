"""Generate tests/golden/noise.npz from the reference's own noise code.

Loads ``isaaclab/utils/noise/noise_model.py`` of a reference checkout BY PATH (it imports only torch) and runs
its functions and its ``NoiseModelWithAdditiveBias`` on the CPU with ``torch.rand_like`` / ``torch.randn_like``
replaced by recorded draws, so the fixture holds inputs, draws and the reference's outputs:

  term cases   every kind x operation, n = 66: per-column tensor parameters at 59 columns, Python-float
               parameters at 21 columns, Python floats under a bias model at 12 columns
  bias cases   NoiseModelWithAdditiveBias: reset() of all envs, apply, reset(ids) of a subset, apply -- bias
               terms with `add` (a random walk: the old bias is the data) and `abs` (a fresh draw)

    python tests/golden/gen_noise.py [--reference DIR] [--check]

--check regenerates into memory and compares with the committed file byte for byte.
"""

from __future__ import annotations

import argparse
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "noise.npz")
DEFAULT_REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "/root/reference")
REL = os.path.join("source", "isaaclab", "isaaclab", "utils", "noise", "noise_model.py")
N = 66
COLS = (59, 21, 12)
KINDS = ("constant", "uniform", "gaussian")
OPS = ("add", "scale", "abs")
PARAMS = {"constant": ("bias", None), "uniform": ("n_min", "n_max"), "gaussian": ("mean", "std")}


class _Draws:
    """Stands in for the module's ``torch``: rand_like / randn_like hand out the queued draws."""

    def __init__(self):
        self.queue: list[torch.Tensor] = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _next(self, data):
        d = self.queue.pop(0)
        assert d.shape == data.shape, (d.shape, data.shape)
        return d

    def rand_like(self, data):
        return self._next(data)

    def randn_like(self, data):
        return self._next(data)


def load_reference(root: str):
    path = os.path.join(root, REL)
    spec = importlib.util.spec_from_file_location("_reference_noise_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.torch = _Draws()
    return mod


def _cfg(mod, kind: str, op: str, p0, p1):
    c = types.SimpleNamespace(func=getattr(mod, f"{kind}_noise"), operation=op)
    a, b = PARAMS[kind]
    setattr(c, a, p0)
    if b:
        setattr(c, b, p1)
    return c


def _scalar_params(kind: str, k: int):
    """Python floats that are not float32 values (so the double -> float32 rounding of w matters)."""
    if kind == "constant":
        return 0.1 + 0.07 * k, 0.0
    if kind == "uniform":
        return -0.3 - 0.011 * k, 0.7 + 0.013 * k
    return 0.05 * (k - 1), 0.3 + 0.017 * k


def _column_params(kind: str, cols: int, rng):
    a = rng.uniform(-0.5, 0.5, cols).astype(np.float32)
    b = (a + rng.uniform(0.1, 1.0, cols)).astype(np.float32) if kind == "uniform" else \
        rng.uniform(0.1, 1.0, cols).astype(np.float32)
    return a, b


def generate(reference: str) -> dict:
    mod = load_reference(reference)
    draws = mod.torch
    rng = np.random.default_rng(20251019)
    arrays: dict[str, np.ndarray] = {}
    cases = []
    for cols in COLS:
        arrays[f"x{cols}"] = rng.normal(0.0, 1.5, (N, cols)).astype(np.float32)
        arrays[f"u{cols}"] = (rng.integers(0, 1 << 24, (N, cols)).astype(np.float32) / np.float32(1 << 24))
        arrays[f"z{cols}"] = rng.normal(0.0, 1.0, (N, cols)).astype(np.float32)

    def term_draws(kind, cols):
        return None if kind == "constant" else arrays[("u" if kind == "uniform" else "z") + str(cols)]

    def bias_draw(kind):
        if kind == "uniform":
            return rng.integers(0, 1 << 24, N).astype(np.float32) / np.float32(1 << 24)
        return rng.normal(0.0, 1.0, N).astype(np.float32)

    def term_cfg(name, kind, op, cols, columns, k):
        if columns:
            a, b = _column_params(kind, cols, rng)
            arrays[f"{name}_p0"], arrays[f"{name}_p1"] = a, b
            return _cfg(mod, kind, op, torch.from_numpy(a.copy()), torch.from_numpy(b.copy())), None
        p = _scalar_params(kind, k)
        return _cfg(mod, kind, op, p[0], p[1]), list(p)

    def run_bias_model(name, case, tcfg, bcfg, bkind, cols, subset):
        """reset() -> apply -> reset(subset) -> apply of the reference's NoiseModelWithAdditiveBias."""
        x = torch.from_numpy(arrays[f"x{cols}"])
        td = term_draws(case["kind"], cols)
        model = mod.NoiseModelWithAdditiveBias(types.SimpleNamespace(noise_cfg=tcfg, bias_noise_cfg=bcfg), N, "cpu")
        ids, masks = [None], [np.ones(N, np.uint8)]
        if subset is not None:
            ids.append(torch.from_numpy(np.flatnonzero(subset)))
            masks.append(subset.astype(np.uint8))
        for s in range(2 if subset is not None else 1):
            bd = bias_draw(bkind) if bkind != "constant" else np.zeros(N, np.float32)
            if bkind != "constant":
                sel = torch.from_numpy(bd).reshape(N, 1)
                draws.queue.append(sel if ids[s] is None else sel[ids[s]])
            model.reset(ids[s])
            if td is not None:
                draws.queue.append(torch.from_numpy(td))
            out = model.apply(x)
            arrays[f"{name}_mask{s}"], arrays[f"{name}_bdraw{s}"] = masks[s], bd
            arrays[f"{name}_bias{s}"] = model._bias.reshape(N).numpy().copy()
            arrays[f"{name}_out{s}"] = out.numpy().copy()
        case["steps"] = 2 if subset is not None else 1

    # ---- term cases: every kind x op
    k = 0
    for cols, columns, with_bias in ((59, True, False), (21, False, False), (12, False, True)):
        for kind in KINDS:
            for op in OPS:
                name = f"t{cols}_{kind}_{op}"
                tcfg, p = term_cfg(name, kind, op, cols, columns, k)
                case = {"name": name, "cols": cols, "kind": kind, "op": op, "p": p, "bias": None}
                if with_bias:
                    bkind = KINDS[1 + k % 2]
                    bp = [-0.2 + 0.01 * k, 0.35 + 0.01 * k] if bkind == "uniform" else [0.03 * k, 0.25]
                    case["bias"] = {"kind": bkind, "op": "abs", "p": bp}
                    run_bias_model(name, case, tcfg, _cfg(mod, bkind, "abs", bp[0], bp[1]), bkind, cols, None)
                else:
                    td = term_draws(kind, cols)
                    if td is not None:
                        draws.queue.append(torch.from_numpy(td))
                    arrays[f"{name}_out0"] = tcfg.func(torch.from_numpy(arrays[f"x{cols}"]), tcfg).numpy().copy()
                    case["steps"] = 1
                cases.append(case)
                k += 1

    # ---- bias cases: reset of all envs, then of a subset, for `add` (random walk) and `abs`
    subset = rng.uniform(size=N) < 0.4
    subset[0], subset[N - 1] = True, False
    for j, (cols, kind, op, columns, bkind, bop, bp) in enumerate((
            (12, "gaussian", "add", False, "gaussian", "add", [0.05, 0.2]),
            (21, "uniform", "scale", False, "uniform", "abs", [-0.3, 0.4]),
            (59, "constant", "add", True, "uniform", "add", [-0.15, 0.25]),
            (12, "uniform", "abs", False, "gaussian", "abs", [0.1, 0.3]),
            (21, "gaussian", "abs", True, "constant", "add", [0.125, 0.0]))):
        name = f"b{j}_{cols}_{kind}_{op}_{bkind}_{bop}"
        tcfg, p = term_cfg(name, kind, op, cols, columns, j)
        case = {"name": name, "cols": cols, "kind": kind, "op": op, "p": p,
                "bias": {"kind": bkind, "op": bop, "p": bp}}
        run_bias_model(name, case, tcfg, _cfg(mod, bkind, bop, bp[0], bp[1]), bkind, cols, subset)
        cases.append(case)
    assert not draws.queue
    arrays["cases"] = np.array(json.dumps(cases))
    return arrays


def serialise(arrays: dict) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, **{k: arrays[k] for k in sorted(arrays)})
    return buf.getvalue()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=DEFAULT_REFERENCE, help="root of a reference checkout")
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    a = ap.parse_args(argv)
    data = serialise(generate(a.reference))
    if a.check:
        same = os.path.exists(OUT) and open(OUT, "rb").read() == data
        print(f"noise.npz: {'identical' if same else 'DIFFERS'} ({len(data)} bytes)")
        return 0 if same else 1
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT} ({len(data)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
