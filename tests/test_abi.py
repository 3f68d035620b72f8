"""C-ABI checks that need no GPU: the library loads, exports every entry point include/allsteps.h
declares, the ctypes structs match the header's field lists, and errors surface as exceptions."""

import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "allsteps.h")


def _declared_functions():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(as_\w+)\(", src, re.M)))


def test_header_declares_abi():
    fns = _declared_functions()
    assert "as_create" in fns and "as_step" in fns and len(fns) >= 12


def test_library_exports_every_declared_symbol():
    from allsteps_isaaclab_amd import _native

    L = _native.load()
    for fn in _declared_functions():
        assert hasattr(L, fn), f"{fn} declared in allsteps.h but not exported"
    assert set(_native.EXPORTED_SYMBOLS) == set(_declared_functions())
    assert L.as_abi_version() == _native.ABI_VERSION


def _struct_fields(name):
    src = open(HEADER).read()
    m = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + ";", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            nm = re.findall(r"\*?\s*(\w+)\s*(?:\[[^\]]*\])*\s*$", part.strip())
            names.append(nm[0])
    return names


@pytest.mark.parametrize("cname,pyname", [("as_model_t", "AsModel"), ("as_sim_t", "AsSim"),
                                          ("as_task_t", "AsTask"), ("as_state_t", "AsState")])
def test_ctypes_structs_match_header(cname, pyname):
    from allsteps_isaaclab_amd import _native

    py = [f[0] for f in getattr(_native, pyname)._fields_]
    assert py == _struct_fields(cname)


def test_model_struct_size_matches_c():
    """sizeof(as_model_t) etc. via a tiny C program compiled against the header."""
    import subprocess
    import tempfile

    from allsteps_isaaclab_amd import _native

    prog = r"""
#include <stdio.h>
#include "allsteps.h"
int main(void){printf("%zu %zu %zu %zu\n", sizeof(as_model_t), sizeof(as_sim_t), sizeof(as_task_t), sizeof(as_state_t));return 0;}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    sizes = [C.sizeof(_native.AsModel), C.sizeof(_native.AsSim), C.sizeof(_native.AsTask), C.sizeof(_native.AsState)]
    assert [int(x) for x in out] == sizes


def test_create_without_device_fails_loudly():
    """No silent CPU fallback: without a GPU the product path raises."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = 4
    cfg.sim.device = "cpu"
    with pytest.raises(_native.NativeError):
        AllstepsEnv(cfg)


def test_null_arguments_return_error():
    from allsteps_isaaclab_amd import _native

    L = _native.load()
    rc = L.as_step(None, None, None, None, None, None, None, None)
    assert rc == -1
    assert b"null" in L.as_last_error()
    h = C.c_void_p()
    assert L.as_create(0, None, None, None, None, 0, 0, 0, C.byref(h)) == -1


# ---------------------------------------------------------------- libppo_hip.so (include/ppo.h)

PPO_HEADER = os.path.join(ROOT, "include", "ppo.h")


def test_ppo_library_exports_every_declared_symbol():
    from allsteps_isaaclab_amd.learning import fused

    src = open(PPO_HEADER).read()
    declared = sorted(set(re.findall(r"^(?:int|const char\*)\s+(ppo_\w+)\(", src, re.M)))
    assert len(declared) >= 14
    L = fused.load()
    for fn in declared:
        assert hasattr(L, fn), f"{fn} declared in ppo.h but not exported"
    assert set(fused.EXPORTED_SYMBOLS) == set(declared)
    assert L.ppo_abi_version() == fused.PPO_ABI_VERSION
    # block-count helpers are pure host functions
    assert L.ppo_loss_blocks(32768) == 256 and L.ppo_elu_bwd_blocks(32768) == 256


@pytest.mark.parametrize("cname,pyname", [("ppo_loss_cfg_t", "PpoLossCfg"), ("ppo_seg_t", "PpoSeg")])
def test_ppo_structs_match_header(cname, pyname):
    from allsteps_isaaclab_amd.learning import fused

    src = open(PPO_HEADER).read()
    m = re.search(r"typedef struct \{([^{}]*)\}\s*" + cname + ";", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [p.strip().split()[-1] for p in decl.split(",")]
    assert [f[0] for f in getattr(fused, pyname)._fields_] == names


def _valid_args():
    """Model / sim / task / state structs of the walker, as the env builds them (no device needed:
    as_create validates every field before it touches HIP)."""
    import numpy as np

    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg
    from allsteps_isaaclab_amd.model import load_model

    cfg = AllstepsEnvCfg()
    m = load_model()
    M, S, T = _native.make_model(m), _native.make_sim(cfg), _native.make_task(cfg, m["dof_names"])
    st = _native.AsState()
    buf = np.zeros(64, np.float32)
    for name, _ in st._fields_:
        setattr(st, name, buf.ctypes.data)
    st.contact_mask_hind = None
    return M, S, T, st, buf


@pytest.mark.parametrize("field,mutate,msg", [
    ("num_self_pairs", lambda M: setattr(M, "num_self_pairs", 257), b"num_self_pairs"),
    ("num_self_pairs<0", lambda M: setattr(M, "num_self_pairs", -1), b"num_self_pairs"),
    ("self_pair order", lambda M: M.self_pair.__setitem__(0, 5 | (3 << 8)), b"self_pair[0]"),
    ("self_pair range", lambda M: M.self_pair.__setitem__(1, 2 | (200 << 8)), b"self_pair[1]"),
    ("num_priority_geoms", lambda M: setattr(M, "num_priority_geoms", 33), b"num_priority_geoms"),
    ("geom_foot", lambda M: M.geom_foot.__setitem__(3, 2), b"geom_foot[3]"),
    ("geom_foot<-1", lambda M: M.geom_foot.__setitem__(4, -2), b"geom_foot[4]"),
    ("geom_link", lambda M: M.geom_link.__setitem__(0, 22), b"geom_link[0]"),
    ("geom_type", lambda M: M.geom_type.__setitem__(1, 2), b"geom_type[1]"),
])
def test_create_rejects_malformed_model(field, mutate, msg):
    """as_create rejects every model field the kernels index with: AS_ERR_INVALID and a
    message naming the field, before any device call."""
    from allsteps_isaaclab_amd import _native

    L = _native.load()
    M, S, T, st, _buf = _valid_args()
    mutate(M)
    h = C.c_void_p()
    rc = L.as_create(4, C.byref(M), C.byref(S), C.byref(T), C.byref(st), 0, 0, 0, C.byref(h))
    assert rc == -1, (field, rc)
    assert msg in L.as_last_error(), L.as_last_error()


def test_create_rejects_more_envs_than_32_bit_offsets_reach():
    """num_envs above AS_MAX_ENVS (2^24: the kernels' field-major offsets are 32-bit) is refused before any
    device call, with a message naming the limit; 2^24 itself passes validation."""
    import torch

    from allsteps_isaaclab_amd import _native

    L = _native.load()
    M, S, T, st, _buf = _valid_args()
    h = C.c_void_p()
    assert L.as_create((1 << 24) + 1, C.byref(M), C.byref(S), C.byref(T), C.byref(st), 0, 0, 0, C.byref(h)) == -1
    assert b"AS_MAX_ENVS" in L.as_last_error()
    if not torch.cuda.is_available():  # validation passes; the error is the missing device's
        assert L.as_create(1 << 24, C.byref(M), C.byref(S), C.byref(T), C.byref(st), 0, 0, 0, C.byref(h)) == -3


def test_create_accepts_the_walker_model_up_to_the_device():
    """The unmodified walker passes validation: without a device the error is the device's."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from allsteps_isaaclab_amd import _native

    L = _native.load()
    M, S, T, st, _buf = _valid_args()
    h = C.c_void_p()
    rc = L.as_create(4, C.byref(M), C.byref(S), C.byref(T), C.byref(st), 0, 0, 0, C.byref(h))
    assert rc == -3, L.as_last_error()


# ---------------------------------------------------------------- provenance (as_build_id / ppo_build_id)

def test_libraries_carry_the_tree_source_digest():
    """Both shipped libraries were compiled from exactly this tree's csrc/ + include/ (VERDICT r04 weak 7)."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.learning import fused

    digest = _native.source_digest()
    assert len(digest) == 16
    assert _native.load().as_build_id().decode() == digest
    assert fused.load().ppo_build_id().decode() == digest


def test_source_digest_tracks_every_source_byte(monkeypatch, tmp_path):
    import shutil

    from allsteps_isaaclab_amd import _native

    base = _native.source_digest()
    csrc = tmp_path / "csrc"
    shutil.copytree(_native.CSRC, csrc)
    monkeypatch.setattr(_native, "CSRC", str(csrc))
    assert _native.source_digest() == base  # the digest does not depend on where the tree lives
    p = csrc / "allsteps_kernels.hip"
    p.write_bytes(p.read_bytes() + b"\n")
    assert _native.source_digest() != base


def test_loader_refuses_a_library_built_from_other_sources(monkeypatch):
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.learning import fused

    monkeypatch.delenv("ALLSTEPS_HIP_LIB", raising=False)
    monkeypatch.delenv("PPO_HIP_LIB", raising=False)
    monkeypatch.setattr(_native, "_LIB", None)
    monkeypatch.setattr(fused, "_LIB", None)
    monkeypatch.setattr(_native, "source_digest", lambda: "0123456789abcdef")
    with pytest.raises(_native.NativeError, match="built from other sources"):
        _native.load()
    with pytest.raises(_native.NativeError, match="built from other sources"):
        fused.load()
    # an explicitly chosen library (A/B variants under abtest/) is loaded as asked
    monkeypatch.setenv("ALLSTEPS_HIP_LIB", _native.LIB_PATH)
    monkeypatch.setenv("PPO_HIP_LIB", _native.PPO_LIB_PATH)
    assert _native.load() is not None and fused.load() is not None


def _structural_skip_mask(m: dict) -> int:
    """Python restatement of the kernel's structural sweep (csrc/allsteps_consts.h sweep_skip_mask):
    padded layout AS_SWEEP_PAD, last block first, a quad skippable when the pivot rows are zero there."""
    import numpy as np

    nl, nv = int(m["num_links"]), 6 + int(m["num_hinges"])
    parent = [int(x) for x in m["parent"][:nl]]
    NP = (nv + 3) // 4 * 4
    NB, PAD = NP // 4, {27: 19, 18: 15}.get(nv, nv)
    NQ = NB - 1

    def on_path(a, l):
        while l >= 0:
            if l == a:
                return True
            l = parent[l] if l > 0 else -1
        return False

    link = lambda d: 0 if d < 6 else d - 5  # noqa: E731
    padded = lambda k: k if k < PAD else k + (NP - nv)  # noqa: E731
    S = np.zeros((NP, NP), bool)
    for i in range(nv):
        for j in range(nv):
            S[padded(i), padded(j)] = on_path(link(i), link(j)) or on_path(link(j), link(i))
    for q in range(NP - nv):
        S[PAD + q, PAD + q] = True
    mask = 0
    for r in range(NB):
        b = NB - 1 - r
        P = list(range(4 * b, 4 * b + 4))
        colany, rowany = S[P, :].any(0), S[:, P].any(1)
        for jb in range(NQ):
            bb = (b - 1 - jb) % NB
            if not colany[4 * bb: 4 * bb + 4].any():
                mask |= 1 << (r * NQ + jb)
        S = S | np.outer(rowany, colany)
        S[:, P] = rowany[:, None]
        S[P, :] = colany[None, :]
        S[np.ix_(P, P)] = True
    return mask


def test_sweep_plan_skips_only_structural_zeros():
    """as_sweep_plan (no device): the walker and the C5 quadruped take the compiled sweep skips (their
    structurally-zero quads include every compiled one: 14 of the walker's 42 quad updates, 6 of the
    quadruped's 20), the C++ structural sweep equals its Python restatement, and a tree whose zeros do not
    cover the compiled skips (a chain: every dof on one root path) falls back to the full sweep."""
    from allsteps_isaaclab_amd import _native
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    walker, quad = load_model(), load_model(ANYMAL_C_JSON)
    for m, compiled, n in ((walker, 207817167, 14), (quad, 3219, 6)):
        use, mask = _native.sweep_plan(m)
        assert use == 1 and mask & compiled == compiled and bin(compiled).count("1") == n
        assert mask == _structural_skip_mask(m)
    chain = dict(walker)
    chain["parent"] = [-1] + list(range(walker["num_links"] - 1)) + [0] * (len(walker["parent"]) - walker["num_links"])
    use, mask = _native.sweep_plan(chain)
    assert use == 0 and mask == _structural_skip_mask(chain) == 0
    bad = dict(walker)
    bad["parent"] = [-1, 3] + list(walker["parent"][2:])
    with pytest.raises(_native.NativeError, match="topological"):
        _native.sweep_plan(bad)
    # the model checks are as_create's: a hinge count that is not num_links - 1 is refused, not swept
    bad = dict(walker)
    bad["num_hinges"] = walker["num_hinges"] - 1
    with pytest.raises(_native.NativeError, match="num_hinges"):
        _native.sweep_plan(bad)
