"""Shared by the IMU tests: the fixture's cases (tests/golden/imu.npz), hand cases with exact answers, the binary
files tests/imu_check.cpp reads and writes, and a NumPy float32 restatement of csrc/allsteps_imu.h.

The restatement mirrors the header operation by operation -- every NumPy ufunc on float32 arrays rounds once, to
float32, and none fuses a product into a sum -- so it equals the host program bit for bit (test_imu_host.py), and the
GPU tests hold the kernel to it without a compiler on the GPU machine.

A case: n, dt, offset_pos, offset_rot, com, gravity_bias, pose (U, 7, n), vel (U, 6, n), upd (R,) and mask (R, n):
record r is an update of the envs of mask[r] from the pose and velocities of update upd[r]; an env outside the mask
keeps its data and prev.  The replay returns data (R, 19, n) and prev (R, 6, n) after every record.
"""

from __future__ import annotations

import json
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imu.npz")
SRC = os.path.join(ROOT, "tests", "imu_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]

FIELDS = (("pos_w", 0, 3), ("quat_w", 3, 7), ("lin_vel_b", 7, 10), ("ang_vel_b", 10, 13), ("lin_acc_b", 13, 16),
          ("ang_acc_b", 16, 19))
DATA_ROWS, PREV_ROWS = 19, 6
F = np.float32


# ------------------------------------------------------------------------------------------------ the fixture
def load_cases() -> list:
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    for c in cases:
        for k in ("upd", "mask", "data64"):
            c[k] = z[f"{c['name']}_{k}"]
        c["pose"], c["vel"] = z[f"{c['motion']}_pose"], z[f"{c['motion']}_vel"]
    return cases


def _case(name, n, dt, pose, vel, upd, mask, o=(0, 0, 0), r=(1, 0, 0, 0), c=(0, 0, 0), g=(0, 0, 9.81), **extra):
    return dict(name=name, n=n, dt=dt, offset_pos=[float(F(x)) for x in o], offset_rot=[float(F(x)) for x in r],
                com=[float(F(x)) for x in c], gravity_bias=[float(F(x)) for x in g],
                pose=np.asarray(pose, F), vel=np.asarray(vel, F), upd=np.asarray(upd, np.int32),
                mask=np.asarray(mask, np.uint8), **extra)


def hand_cases() -> list:
    """Dyadic values, exact answers.  All: w = (0, 0, 2), o - c = (0.5, 0, 0), v = (1, 0, 0), dt = 0.25, bias
    (0, 0, 8), the same inputs at two updates: lin_acc_w = (4, 4, 8) R then (0, 0, 8), ang_acc_w = (0, 0, 8) then 0."""
    def two(q):
        pose = np.zeros((2, 7, 1), F)
        pose[:, :3, 0] = (1.0, 2.0, 3.0)
        pose[:, 3:, 0] = q
        vel = np.zeros((2, 6, 1), F)
        vel[:, :, 0] = (1, 0, 0, 0, 0, 2)
        return pose, vel

    out = []
    kw = dict(n=1, dt=0.25, upd=[0, 1], mask=[[1], [1]], g=(0, 0, 8))
    # identity: world = body; lin_vel_w = (1, 0, 0) + (0, 0, 2) x (0.5, 0, 0) = (1, 1, 0)
    pose, vel = two((1, 0, 0, 0))
    exp = np.zeros((2, 19, 1), F)
    exp[:, :7, 0] = (1.5, 2, 3, 1, 0, 0, 0)
    exp[:, 7:13, 0] = (1, 1, 0, 0, 0, 2)
    exp[0, 13:, 0] = (4, 4, 8, 0, 0, 8)
    exp[1, 13:, 0] = (0, 0, 8, 0, 0, 0)
    prev = np.zeros((2, 6, 1), F)
    prev[:, :, 0] = (1, 1, 0, 0, 0, 2)
    out.append(_case("h_identity", pose=pose, vel=vel, o=(0.5, 0, 0), expect=exp, expect_prev=prev, **kw))
    # the same with o = (0.75, 0, 0) and c = (0.25, 0, 0): o - c is what the velocity sees, o what the position sees
    exp2 = exp.copy()
    exp2[:, 0, 0] = 1.75
    out.append(_case("h_com", pose=pose, vel=vel, o=(0.75, 0, 0), c=(0.25, 0, 0), expect=exp2, expect_prev=prev, **kw))
    # the body turned 180 degrees about z: R u = (-ux, -uy, uz); arm = (-0.5, 0, 0), lin_vel_w = (1, -1, 0)
    pose, vel = two((0, 0, 0, 1))
    exp = np.zeros((2, 19, 1), F)
    exp[:, :7, 0] = (0.5, 2, 3, 0, 0, 0, 1)
    exp[:, 7:13, 0] = (-1, 1, 0, 0, 0, 2)
    exp[0, 13:, 0] = (-4, 4, 8, 0, 0, 8)
    exp[1, 13:, 0] = (0, 0, 8, 0, 0, 0)
    prev = np.zeros((2, 6, 1), F)
    prev[:, :, 0] = (1, -1, 0, 0, 0, 2)
    out.append(_case("h_body_180z", pose=pose, vel=vel, o=(0.5, 0, 0), expect=exp, expect_prev=prev, **kw))
    # the sensor turned 180 degrees about x in an unturned body: quat_w = (0, 1, 0, 0), body u = (ux, -uy, -uz)
    pose, vel = two((1, 0, 0, 0))
    exp = np.zeros((2, 19, 1), F)
    exp[:, :7, 0] = (1.5, 2, 3, 0, 1, 0, 0)
    exp[:, 7:13, 0] = (1, -1, 0, 0, 0, -2)
    exp[0, 13:, 0] = (4, -4, -8, 0, 0, -8)
    exp[1, 13:, 0] = (0, 0, -8, 0, 0, 0)
    prev = np.zeros((2, 6, 1), F)
    prev[:, :, 0] = (1, 1, 0, 0, 0, 2)
    out.append(_case("h_sensor_180x", pose=pose, vel=vel, o=(0.5, 0, 0), r=(0, 1, 0, 0), expect=exp, expect_prev=prev,
                     **kw))
    # the per-env outdated rule: v = (u, 0, 0) at update u, no rotation, no arm, no bias; record 1 updates env 1
    # alone, record 2 all: env 0 and 2 difference update 2 against update 0, env 1 against update 1
    n = 3
    pose = np.zeros((3, 7, n), F)
    pose[:, 3] = 1
    pose[:, 0] = np.arange(3, dtype=F)[:, None]  # x = u
    vel = np.zeros((3, 6, n), F)
    vel[:, 0] = np.arange(3, dtype=F)[:, None]
    exp = np.zeros((3, 19, n), F)
    exp[:, 3] = 1
    exp[0, 0], exp[0, 7], exp[0, 13] = 0, 0, 0
    exp[1] = exp[0]
    exp[1, 0, 1], exp[1, 7, 1], exp[1, 13, 1] = 1, 1, 4
    exp[2, 0], exp[2, 7] = 2, 2
    exp[2, 13] = (8, 4, 8)
    prev = np.zeros((3, 6, n), F)
    prev[1, 0, 1] = 1
    prev[2, 0] = 2
    out.append(_case("h_outdated", n=n, dt=0.25, pose=pose, vel=vel, upd=[0, 1, 2], mask=[[1, 1, 1], [0, 1, 0], [1, 1, 1]],
                     g=(0, 0, 0), expect=exp, expect_prev=prev))
    return out


def all_cases() -> list:
    return load_cases() + hand_cases()


# ------------------------------------------------------------------------------------- NumPy float32 restatement
def cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def quat_mul(q1, q2):
    w1, x1, y1, z1 = q1
    w2, x2, y2, z2 = q2
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = (ww + yy) + zz
    qq = F(0.5) * (xx + (z1 - x1) * (x2 - y2))
    return np.stack([(qq - ww) + (z1 - y1) * (y2 - z2), (qq - xx) + (x1 + w1) * (x2 + w2),
                     (qq - yy) + (w1 - x1) * (y2 + z2), (qq - zz) + (z1 + y1) * (w2 - x2)])


def quat_rotate(q, u, inverse=False):
    qw, xyz = q[0], q[1:]
    s = F(2.0) * (qw * qw) - F(1.0)
    x = cross(xyz, u)
    dot = (xyz[0] * u[0] + xyz[1] * u[1]) + xyz[2] * u[2]
    a = u * s
    b = (x * qw) * F(2.0)
    c = (xyz * dot) * F(2.0)
    return ((a - b) if inverse else (a + b)) + c


def imu_update(p, q, v, w, o, r, c, g, dt, prev):
    """allsteps_imu.h imu_update on float32 (3|4, n) arrays, constants as float32 3- / 4-vectors; prev (6, n).
    Returns (data (19, n), new prev (6, n))."""
    n = p.shape[1]
    assert all(x.dtype == F for x in (p, q, v, w, prev))
    col = lambda k: np.repeat(np.asarray(k, F)[:, None], n, 1)  # noqa: E731
    o, r, c, g, dt = col(o), col(r), col(c), col(g), F(dt)
    pos_w = p + quat_rotate(q, o)
    quat_w = quat_mul(q, r)
    lin_vel_w = v + cross(w, quat_rotate(q, o - c))
    lin_acc_w = (lin_vel_w - prev[0:3]) / dt + g
    ang_acc_w = (w - prev[3:6]) / dt
    data = np.concatenate([pos_w, quat_w, quat_rotate(quat_w, lin_vel_w, True), quat_rotate(quat_w, w, True),
                           quat_rotate(quat_w, lin_acc_w, True), quat_rotate(quat_w, ang_acc_w, True)])
    new_prev = np.concatenate([lin_vel_w, w])
    assert data.dtype == F and new_prev.dtype == F and data.shape == (DATA_ROWS, n)
    return data, new_prev


def initial_buffers(n: int):
    data = np.zeros((DATA_ROWS, n), F)
    data[3] = 1
    return data, np.zeros((PREV_ROWS, n), F)


def masked_update(data, prev, mask, p, q, v, w, o, r, c, g, dt):
    """One launch: the envs of `mask` updated, the others untouched; returns new (data, prev)."""
    d, pv = imu_update(p, q, v, w, o, r, c, g, dt, prev)
    m = np.asarray(mask).astype(bool)[None]
    return np.where(m, d, data), np.where(m, pv, prev)


def replay(case: dict):
    """(data (R, 19, n), prev (R, 6, n)) of the restatement on a case."""
    data, prev = initial_buffers(case["n"])
    out_d, out_p = [], []
    with np.errstate(all="ignore"):
        for u, mask in zip(case["upd"], case["mask"]):
            ps, vl = case["pose"][u], case["vel"][u]
            data, prev = masked_update(data, prev, mask, ps[0:3], ps[3:7], vl[0:3], vl[3:6], case["offset_pos"],
                                       case["offset_rot"], case["com"], case["gravity_bias"], case["dt"])
            out_d.append(data)
            out_p.append(prev)
    return np.stack(out_d), np.stack(out_p)


# ------------------------------------------------------------------------------------------------ the program
def write_cases_bin(path: str, cases: list) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("=i", len(cases)))
        for c in cases:
            U, R = c["pose"].shape[0], len(c["upd"])
            f.write(struct.pack("=iii", c["n"], U, R))
            f.write(np.asarray([c["dt"], *c["offset_pos"], *c["offset_rot"], *c["com"], *c["gravity_bias"]],
                               F).tobytes())
            for a, dt in ((c["pose"], F), (c["vel"], F), (c["upd"], np.int32), (c["mask"], np.uint8)):
                f.write(np.ascontiguousarray(a, dt).tobytes())


def read_out_bin(path: str, cases: list) -> list:
    out = []
    with open(path, "rb") as f:
        for c in cases:
            n, R = c["n"], len(c["upd"])
            d = np.frombuffer(f.read(4 * R * DATA_ROWS * n), F).reshape(R, DATA_ROWS, n)
            p = np.frombuffer(f.read(4 * R * PREV_ROWS * n), F).reshape(R, PREV_ROWS, n)
            out.append({"data": d, "prev": p})
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
