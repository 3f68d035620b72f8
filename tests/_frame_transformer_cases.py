"""Shared by the frame-transformer tests: the fixture's cases (tests/golden/frame_transformer.npz), hand cases with
exact answers, the binary files tests/frame_transformer_check.cpp reads and writes, and a NumPy float32 restatement
of csrc/allsteps_frame_transformer.h.

The restatement mirrors the header operation by operation -- every NumPy ufunc on float32 arrays rounds once, to
float32, and none fuses a product into a sum -- so it equals the host program bit for bit
(test_frame_transformer_host.py), and the GPU tests hold the kernel to it without a compiler on the GPU machine.

A case: n, pose (U, B, 7, n) the link poses of B bodies per update (pos 3 | quat 4 (w, x, y, z); a stone has
(1, 0, 0, 0)), source (index into B), source_offset (7,), apply_source, frames [(body index, offset (7,))],
apply_target.  The replay returns source (U, 7, n) and target (U, 14, F, n).
"""

from __future__ import annotations

import json
import os
import shutil
import struct
import subprocess

import numpy as np

from _imu_cases import cross, quat_mul  # allsteps_imu.h's, as they are

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_transformer.npz")
SRC = os.path.join(ROOT, "tests", "frame_transformer_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]

SOURCE_FIELDS = (("source_pos_w", 0, 3), ("source_quat_w", 3, 7))
TARGET_FIELDS = (("target_pos_w", 0, 3), ("target_quat_w", 3, 7), ("target_pos_source", 7, 10),
                 ("target_quat_source", 10, 14))
SOURCE_ROWS, TARGET_ROWS = 7, 14
F = np.float32
IDENTITY = (0, 0, 0, 1, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ the fixture
def spec_of(c: dict):
    """The fixture case's cfg through the package's own host resolution (FrameTransformerSpec)."""
    from allsteps_isaaclab_amd.envs.frame_transformer import FrameTransformerSpec
    from allsteps_isaaclab_amd.utils.sensors import FrameTransformerCfg, OffsetCfg

    k = c["cfg"]
    off = lambda o: OffsetCfg(pos=tuple(o["pos"]), rot=tuple(o["rot"]))  # noqa: E731
    cfg = FrameTransformerCfg(prim_path=k["prim_path"], source_frame_offset=off(k["source_frame_offset"]),
                              target_frames=[FrameTransformerCfg.FrameCfg(prim_path=t["prim_path"], name=t["name"],
                                                                          offset=off(t["offset"]))
                                             for t in k["target_frames"]])
    return FrameTransformerSpec(cfg, model={"body_names": c["robot_bodies"]}, num_steps=c["num_steps"],
                                step_dt=4 / 240)


def load_cases() -> list:
    """The fixture's cases, resolved by FrameTransformerSpec: frame order and switches are the package's."""
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    for c in cases:
        c["source64"], c["target64"] = z[f"{c['name']}_source64"], z[f"{c['name']}_target64"]
        c["pose"] = z[f"{c['motion']}_pose"]
        spec = spec_of(c)
        index = {b: i for i, b in enumerate(c["bodies"])}
        c["frame_names"] = spec.frame_names[0]
        c["source"] = index[spec.sources[0][2]]
        c["source_offset"] = np.asarray([*spec.source_offsets[0][0], *spec.source_offsets[0][1]], F)
        c["apply_source"], c["apply_target"] = spec.apply_source[0], spec.apply_target[0]
        c["frames"] = [(index[body[2]], np.asarray([*pos, *rot], F)) for body, pos, rot in spec.frames[0]]
    return cases


def _case(name, bodies, source, frames, source_offset=IDENTITY, apply_source=False, apply_target=False, **extra):
    pose = np.asarray(bodies, F).reshape(1, len(bodies), 7, 1)
    return dict(name=name, n=1, pose=pose, source=source, source_offset=np.asarray(source_offset, F),
                apply_source=apply_source, apply_target=apply_target,
                frames=[(b, np.asarray(o, F)) for b, o in frames], **extra)


def hand_cases() -> list:
    """Dyadic values, exact answers.  expect_source (7,), expect_target (14, F)."""
    zt = (0, 0, 0, 1)  # 180 degrees about z: R u = (-ux, -uy, uz)
    xt = (0, 1, 0, 0)  # 180 degrees about x
    yt = (0, 0, 1, 0)  # z-turn times x-turn: 180 degrees about y, R u = (-ux, uy, -uz)
    out = []
    # identity: the difference of the positions
    out.append(_case("h_identity", [(1, 2, 3, 1, 0, 0, 0), (2, 4, 3.5, 1, 0, 0, 0)], 0, [(1, IDENTITY)],
                     expect_source=(1, 2, 3, 1, 0, 0, 0),
                     expect_target=[(2, 4, 3.5, 1, 0, 0, 0, 1, 2, 0.5, 1, 0, 0, 0)]))
    # both bodies turned 180 degrees about z: the difference turned back, the relative rotation the identity
    out.append(_case("h_body_180z", [(1, 2, 3, *zt), (2, 4, 3.5, *zt)], 0, [(1, IDENTITY)],
                     expect_source=(1, 2, 3, *zt), expect_target=[(2, 4, 3.5, *zt, -1, -2, 0.5, 1, 0, 0, 0)]))
    # a source offset only: source = (1, 2, 3) + Rz (0.5, 0, 0), zt * xt = yt
    src_off = (0.5, 0, 0, *xt)
    out.append(_case("h_source_offset", [(1, 2, 3, *zt), (0.5, 2, 4, *yt)], 0, [(1, IDENTITY)], source_offset=src_off,
                     apply_source=True, expect_source=(0.5, 2, 3, *yt),
                     expect_target=[(0.5, 2, 4, *yt, 0, 0, -1, 1, 0, 0, 0)]))
    # a target offset only: target = (2, 2, 3) + Rz (0.5, 0.25, 0)
    tgt_off = (0.5, 0.25, 0, *xt)
    out.append(_case("h_target_offset", [(1, 2, 3, 1, 0, 0, 0), (2, 2, 3, *zt)], 0, [(1, tgt_off)], apply_target=True,
                     expect_source=(1, 2, 3, 1, 0, 0, 0),
                     expect_target=[(1.5, 1.75, 3, *yt, 0.5, -0.25, 0, *yt)]))
    # both: Ry^-1 ((1.5, 1.75, 3) - (0.5, 2, 3)) = (-1, -0.25, 0)
    out.append(_case("h_both", [(1, 2, 3, *zt), (2, 2, 3, *zt)], 0, [(1, tgt_off)], source_offset=src_off,
                     apply_source=True, apply_target=True, expect_source=(0.5, 2, 3, *yt),
                     expect_target=[(1.5, 1.75, 3, *yt, -1, -0.25, 0, 1, 0, 0, 0)]))
    # a stone target (quaternion (1, 0, 0, 0)) seen from a turned body, and the body itself as a second frame
    out.append(_case("h_stone", [(1, 2, 3, *zt), (3, 2, 0.5, 1, 0, 0, 0)], 0, [(0, IDENTITY), (1, IDENTITY)],
                     expect_source=(1, 2, 3, *zt),
                     expect_target=[(1, 2, 3, *zt, 0, 0, 0, 1, 0, 0, 0), (3, 2, 0.5, 1, 0, 0, 0, -2, 0, -2.5, 0, 0, 0, -1)]))
    for c in out:
        c["expect_source"] = np.asarray(c["expect_source"], F).reshape(1, 7, 1)
        c["expect_target"] = np.asarray(c["expect_target"], F).T.reshape(1, 14, len(c["frames"]), 1)
    return out


def all_cases() -> list:
    return load_cases() + hand_cases()


# ------------------------------------------------------------------------------------- NumPy float32 restatement
def quat_apply(q, v):
    w, xyz = q[0], q[1:]
    t = cross(xyz, v) * F(2.0)
    return (v + w * t) + cross(xyz, t)


def quat_inv(q):
    s = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    d = np.where(s > F(1e-9), s, F(1e-9)).astype(F)
    return np.stack([q[0] / d, -q[1] / d, -q[2] / d, -q[3] / d])


def combine(t01, q01, t12, q12):
    return t01 + quat_apply(q01, t12), quat_mul(q01, q12)


def subtract(t01, q01, t02, q02):
    q10 = quat_inv(q01)
    return quat_apply(q10, t02 - t01), quat_mul(q10, q02)


def _col(k, n):
    return np.repeat(np.asarray(k, F)[:, None], n, 1)


def frame_source(p, q, apply, offset):
    """allsteps_frame_transformer.h frame_source on float32 (3|4, n) arrays; returns (7, n)."""
    assert p.dtype == F and q.dtype == F
    if apply:
        p, q = combine(p, q, _col(offset[:3], p.shape[1]), _col(offset[3:], p.shape[1]))
    out = np.concatenate([p, q])
    assert out.dtype == F
    return out


def frame_target(source, p, q, apply, offset):
    """frame_target: (14, n) from the source rows (7, n) and the target body's link pose."""
    assert p.dtype == F and q.dtype == F and source.dtype == F
    if apply:
        p, q = combine(p, q, _col(offset[:3], p.shape[1]), _col(offset[3:], p.shape[1]))
    pr, qr = subtract(source[0:3], source[3:7], p, q)
    out = np.concatenate([p, q, pr, qr])
    assert out.dtype == F and out.shape == (TARGET_ROWS, p.shape[1])
    return out


def frames_of(poses, source, source_offset, apply_source, frames, apply_target):
    """One launch for one sensor: poses (B, 7, n) -> (source (7, n), target (14, F, n))."""
    with np.errstate(all="ignore"):
        src = frame_source(poses[source, 0:3], poses[source, 3:7], apply_source, np.asarray(source_offset, F))
        tgt = [frame_target(src, poses[b, 0:3], poses[b, 3:7], apply_target, np.asarray(o, F)) for b, o in frames]
    return src, np.stack(tgt, 1)


def replay(case: dict):
    """(source (U, 7, n), target (U, 14, F, n)) of the restatement on a case."""
    out = [frames_of(p, case["source"], case["source_offset"], case["apply_source"], case["frames"],
                     case["apply_target"]) for p in case["pose"]]
    return np.stack([s for s, _ in out]), np.stack([t for _, t in out])


# ------------------------------------------------------------------------------------------------ the program
def write_cases_bin(path: str, cases: list) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("=i", len(cases)))
        for c in cases:
            U, B, _, n = c["pose"].shape
            f.write(struct.pack("=iiiiiii", n, U, B, len(c["frames"]), c["source"], int(c["apply_source"]),
                                int(c["apply_target"])))
            f.write(np.asarray(c["source_offset"], F).tobytes())
            f.write(np.asarray([b for b, _ in c["frames"]], np.int32).tobytes())
            f.write(np.asarray([o for _, o in c["frames"]], F).tobytes())
            f.write(np.ascontiguousarray(c["pose"], F).tobytes())


def read_out_bin(path: str, cases: list) -> list:
    out = []
    with open(path, "rb") as f:
        for c in cases:
            U, _, _, n = c["pose"].shape
            nf = len(c["frames"])
            s = np.frombuffer(f.read(4 * U * SOURCE_ROWS * n), F).reshape(U, SOURCE_ROWS, n)
            t = np.frombuffer(f.read(4 * U * TARGET_ROWS * nf * n), F).reshape(U, TARGET_ROWS, nf, n)
            out.append({"source": s, "target": t})
        assert f.read() == b""
    return out


def build_program(exe: str, flags=()) -> None:
    r = subprocess.run([CXX, *CXXFLAGS, *flags, "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def run_program(exe: str, workdir: str, cases: list):
    """(stdout, outputs per case) of one run of the built program on `cases`."""
    cases_bin, out_bin = os.path.join(workdir, "cases.bin"), os.path.join(workdir, "out.bin")
    write_cases_bin(cases_bin, cases)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout, read_out_bin(out_bin, cases)
