"""Cases of the ray-cast camera tests: the NumPy float32 restatement of csrc/allsteps_ray_camera.h, the loader of the
fixture (tests/golden/ray_camera.npz, from the reference's own RayCasterCamera code: gen_ray_camera.py), the hand
cases with their exact answers, a float64 check written independently of the header, and the runner of the host
program (tests/ray_camera_check.cpp).

A case is a dict in the device layouts: ``n``, ``width``, ``height``, ``surfaces`` (bit 0 the ground, bit 1 the
stones), ``clipping`` (0 none, 1 max, 2 zero), ``max_distance``, ``ground_z``, ``half`` (3,), ``num_steps``, ``dirs``
(3, R), ``offset`` (7, n), ``root_pos`` (3, n), ``root_quat`` (4, n), ``stones`` (60, n), all float32.  ``restate``
returns ``pose`` (7, n), ``plane`` (n, R), ``camera`` (n, R), ``normals`` (n, R, 3), ``dirs_w`` (n, R, 3), ``t`` (n, R)
and ``surface`` (n, R) int32: every operation a float32 NumPy operation in the header's order, so the bits are the
header's.
"""

from __future__ import annotations

import json
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ray_camera.npz")
SRC = os.path.join(ROOT, "tests", "ray_camera_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]

GROUND, STONES = 1, 2
HIT_GROUND, MISS = -1, -2
CLIP_NONE, CLIP_MAX, CLIP_ZERO = 0, 1, 2
CLIP = {"none": CLIP_NONE, "max": CLIP_MAX, "zero": CLIP_ZERO}
NUM_STONES = 20
CAST_MAX = np.float32(1e6)
F = np.float32
INF = F(np.inf)
OUTPUTS = (("pose", np.float32), ("plane", np.float32), ("camera", np.float32), ("normals", np.float32),
           ("dirs_w", np.float32), ("t", np.float32), ("surface", np.int32))


def out_shapes(n: int, R: int) -> dict:
    return {"pose": (7, n), "plane": (n, R), "camera": (n, R), "normals": (n, R, 3), "dirs_w": (n, R, 3), "t": (n, R),
            "surface": (n, R)}


# ------------------------------------------------------------------------------------- the float32 restatement
def quat_apply(q, v):
    """math.py:545-564 on float32 arrays (..., 4) and (..., 3), broadcast."""
    w, x, y, z = (q[..., k] for k in range(4))
    v0, v1, v2 = (v[..., k] for k in range(3))
    t0 = (y * v2 - z * v1) * F(2)
    t1 = (z * v0 - x * v2) * F(2)
    t2 = (x * v1 - y * v0) * F(2)
    return np.stack([(v0 + w * t0) + (y * t2 - z * t1), (v1 + w * t1) + (z * t0 - x * t2),
                     (v2 + w * t2) + (x * t1 - y * t0)], -1)


def quat_mul(a, b):
    """math.py:489-497 on float32 arrays (..., 4)."""
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = (ww + yy) + zz
    qq = F(0.5) * (xx + (z1 - x1) * (x2 - y2))
    return np.stack([(qq - ww) + (z1 - y1) * (y2 - z2), (qq - xx) + (x1 + w1) * (x2 + w2),
                     (qq - yy) + (w1 - x1) * (y2 + z2), (qq - zz) + (z1 + y1) * (w2 - x2)], -1)


def frame(c):
    """(pos_w (n, 3), quat_w (n, 4), q_inv (n, 4)) of a case."""
    rp, rq = np.ascontiguousarray(c["root_pos"].T, F), np.ascontiguousarray(c["root_quat"].T, F)
    off = np.ascontiguousarray(c["offset"].T, F)
    pos = rp + quat_apply(rq, off[:, :3])
    quat = quat_mul(rq, off[:, 3:])
    w, x, y, z = (quat[:, k] for k in range(4))
    nrm = np.fmax(np.sqrt(((w * w + x * x) + y * y) + z * z), F(1e-9))
    q_inv = np.stack([w / nrm, -x / nrm, -y / nrm, -z / nrm], -1)
    return pos, quat, q_inv


def _slab(o, d, inv, cc, h):
    lo, hi = cc - h, cc + h
    t1, t2 = (lo - o) * inv, (hi - o) * inv
    par = d == 0
    inside = (o >= lo) & (o <= hi)
    near = np.where(par, np.where(inside, -INF, INF), np.fmin(t1, t2))
    far = np.where(par, np.where(inside, INF, -INF), np.fmax(t1, t2))
    return near.astype(F), far.astype(F)


def _slabs(o, d, inv, ctr, half):
    """near, far (n, R, 3) of boxes with centres ctr (n, 1 | R, 3)."""
    return _slab(o, d, inv, ctr, half.reshape(1, 1, 3))


def restate(c, depth=None) -> dict:
    """The header on a case.  ``depth`` (n, R) float32 replaces the cast's distances (+inf: a miss) -- the
    post-processing alone, for the fixture's case z; surface and normals then mean nothing."""
    n, R = c["n"], c["width"] * c["height"]
    half = np.asarray(c["half"], F)
    mx, gz = F(c["max_distance"]), F(c["ground_z"])
    with np.errstate(all="ignore"):
        pos, quat, q_inv = frame(c)
        dl = np.ascontiguousarray(c["dirs"].T, F)  # (R, 3)
        d = quat_apply(quat[:, None, :], dl[None])  # (n, R, 3)
        o = np.broadcast_to(pos[:, None, :], d.shape)
        inv = F(1) / d
        t = np.full((n, R), INF, F)
        surf = np.full((n, R), MISS, np.int32)
        if c["surfaces"] & GROUND:
            tg = (gz - o[..., 2]) * inv[..., 2]
            ok = (d[..., 2] < 0) & (tg >= 0) & (tg <= CAST_MAX) & (tg < t)
            t, surf = np.where(ok, tg, t), np.where(ok, HIT_GROUND, surf)
        st = np.ascontiguousarray(c["stones"].T, F).reshape(n, NUM_STONES, 3)
        if c["surfaces"] & STONES:
            for s in range(c["num_steps"]):
                near, far = _slabs(o, d, inv, st[:, s][:, None, :], half)
                tn = np.fmax(np.fmax(near[..., 0], near[..., 1]), near[..., 2])
                tf = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2])
                ts = np.where(tn >= 0, tn, tf)
                ok = (tn <= tf) & (tf >= 0) & (ts <= CAST_MAX) & (ts < t)
                t, surf = np.where(ok, ts, t), np.where(ok, s, surf)
        t = t.astype(F) if depth is None else np.ascontiguousarray(depth, F)
        # distance_to_camera
        if c["clipping"] == CLIP_MAX:
            camera = np.where(t > mx, mx, t)
        elif c["clipping"] == CLIP_ZERO:
            camera = np.where(t > mx, F(0), t)
        else:
            camera = t
        # distance_to_image_plane
        plane = quat_apply(q_inv[:, None, :], t[..., None] * d)[..., 0]
        plane = np.where(np.isnan(plane), F(np.nan), plane)  # the canonical quiet NaN
        if c["clipping"] == CLIP_MAX:
            plane = np.where(plane > mx, mx, plane)
            plane = np.where(np.isnan(plane), mx, plane)
        elif c["clipping"] == CLIP_ZERO:
            plane = np.where(plane > mx, F(0), plane)
            plane = np.where(np.isnan(plane), F(0), plane)
        # normals
        ctr = np.take_along_axis(st, np.clip(surf, 0, NUM_STONES - 1)[..., None].repeat(3, -1), 1)  # (n, R, 3)
        near, far = _slabs(o, d, inv, ctr, half)
        tn = np.fmax(np.fmax(near[..., 0], near[..., 1]), near[..., 2])
        tf = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2])
        outside = tn >= 0
        ax_n = np.where(near[..., 0] == tn, 0, np.where(near[..., 1] == tn, 1, 2))
        ax_f = np.where(far[..., 0] == tf, 0, np.where(far[..., 1] == tf, 1, 2))
        axis = np.where(outside, ax_n, ax_f)
        da = np.take_along_axis(d, axis[..., None], -1)[..., 0]
        sign = np.where((da > 0) == outside, F(-1), F(1))
        face = np.where(np.arange(3) == axis[..., None], sign[..., None], F(0))
        normals = np.where((surf == MISS)[..., None], INF,
                           np.where((surf >= 0)[..., None], face, np.asarray([0, 0, 1], F)))
    return {"pose": np.concatenate([pos.T, quat.T]).astype(F), "plane": plane.astype(F), "camera": camera.astype(F),
            "normals": normals.astype(F), "dirs_w": d.astype(F), "t": t, "surface": surf}


def same_bits(a, b) -> int:
    """Words that differ between two arrays of equal shape and dtype (NaNs compared as bits)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


# ------------------------------------------------------------------------------------- the fixture
def load_fixture() -> dict:
    d = np.load(GOLDEN)
    out = {k: d[k] for k in d.files if k != "meta"}
    out["meta"] = json.loads(str(d["meta"]))
    return out


def make_case(n, width, height, dirs, offset, root_pos, root_quat, stones, *, surfaces=GROUND | STONES,
              clipping=CLIP_NONE, max_distance=1e6, ground_z=0.0, half=(0.25, 0.4, 0.1125), num_steps=NUM_STONES,
              name="") -> dict:
    f = lambda a, shape: np.ascontiguousarray(np.asarray(a, F).reshape(shape))  # noqa: E731
    return dict(name=name, n=n, width=width, height=height, surfaces=surfaces, clipping=clipping,
                max_distance=float(max_distance), ground_z=float(ground_z), half=np.asarray(half, F),
                num_steps=num_steps, dirs=f(dirs, (3, width * height)), offset=f(offset, (7, n)),
                root_pos=f(root_pos, (3, n)), root_quat=f(root_quat, (4, n)), stones=f(stones, (60, n)))


def world_case(fx: dict, **kw) -> dict:
    """The fixture's case w (24 root poses over stone walks, the 19 x 13 default pattern, a pitched offset in the
    "world" convention) as a case of the device layouts."""
    m = fx["meta"]["w"]
    return make_case(m["n"], m["width"], m["height"], fx["w_dirs"], fx["w_offset"], fx["w_root_pos"],
                     fx["w_root_quat"], fx["w_stones"], half=m["half"], name="w", **kw)


# ---- the hand cases: one env, one ray each, the camera at (0, 0, 2) with the identity orientation (root at the
# origin of orientation, offset (0, 0, 2) | identity), so that a world ray is its local ray exactly and the camera
# frame is the world's; every coordinate, half extent (0.5, 0.5, 0.25) and direction component is a small dyadic
# number and every reciprocal a power of two: all arithmetic is exact and the answers are stated, not computed.
H_HALF = (0.5, 0.5, 0.25)
FAR = (1024.0, 1024.0, -1024.0)  # where the unused stones lie
NAN = float("nan")
# name -> (stones {index: centre}, direction, clipping, max_distance, expected (t, plane, camera, normal, surface))
HAND = {
    # straight down onto the ground: t = 2; forward is +x, so the plane distance is 0
    "down": ({}, (0.0, 0.0, -1.0), "none", 1e6, (2.0, 0.0, 2.0, (0, 0, 1), HIT_GROUND)),
    # forward and down at 45 degrees onto the top (z = 1) of the box at (1, 0, 0.75): t = 1 in units of |d|
    "stone_top": ({0: (1.0, 0.0, 0.75)}, (1.0, 0.0, -1.0), "none", 1e6, (1.0, 1.0, 1.0, (0, 0, 1), 0)),
    # the camera inside the box at (0, 0, 2): the far face x = 0.5 along +x, normal +sign(d)
    "inside": ({0: (0.0, 0.0, 2.0)}, (1.0, 0.0, 0.0), "none", 1e6, (0.5, 0.5, 0.5, (1, 0, 0), 0)),
    "inside_back": ({0: (0.0, 0.0, 2.0)}, (-1.0, 0.0, 0.0), "none", 1e6, (0.5, -0.5, 0.5, (-1, 0, 0), 0)),
    # horizontal with nothing ahead: a miss
    "miss": ({}, (1.0, 0.0, 0.0), "none", 1e6, (np.inf, NAN, np.inf, (np.inf, np.inf, np.inf), MISS)),
    "miss_max": ({}, (1.0, 0.0, 0.0), "max", 8.0, (np.inf, 8.0, 8.0, (np.inf, np.inf, np.inf), MISS)),
    "miss_zero": ({}, (1.0, 0.0, 0.0), "zero", 8.0, (np.inf, 0.0, 0.0, (np.inf, np.inf, np.inf), MISS)),
    # the box at (2, 0, -0.25) has its top on the ground plane: equal t = 2 on both, the ground wins
    "tie_ground": ({0: (2.0, 0.0, -0.25)}, (1.0, 0.0, -1.0), "none", 1e6, (2.0, 2.0, 2.0, (0, 0, 1), HIT_GROUND)),
    # onto the edge x = 1.5, z = 0.5 of the box at (2, 0, 0.25): near distances 1.5 on x and on z, the lower axis
    "tie_edge": ({0: (2.0, 0.0, 0.25)}, (1.0, 0.0, -1.0), "none", 1e6, (1.5, 1.5, 1.5, (-1, 0, 0), 0)),
    # a hit beyond max_distance: clipped in both images, the normal stays
    "clip_max": ({}, (1.0, 0.0, -0.25), "max", 4.0, (8.0, 4.0, 4.0, (0, 0, 1), HIT_GROUND)),
    "clip_zero": ({}, (1.0, 0.0, -0.25), "zero", 4.0, (8.0, 0.0, 0.0, (0, 0, 1), HIT_GROUND)),
}


def hand_cases() -> list:
    out = []
    for name, (boxes, direction, clip, mx, expect) in HAND.items():
        stones = np.tile(np.asarray(FAR, F), NUM_STONES)
        for s, ctr in boxes.items():
            stones[3 * s: 3 * s + 3] = ctr
        c = make_case(1, 1, 1, direction, (0, 0, 2, 1, 0, 0, 0), (0, 0, 0), (1, 0, 0, 0), stones, clipping=CLIP[clip],
                      max_distance=mx, half=H_HALF, name=f"h_{name}")
        t, plane, camera, normal, surface = expect
        c["expect"] = dict(t=np.full((1, 1), t, F), plane=np.full((1, 1), plane, F), camera=np.full((1, 1), camera, F),
                           normals=np.asarray(normal, F).reshape(1, 1, 3), surface=np.full((1, 1), surface, np.int32),
                           pose=np.asarray((0, 0, 2, 1, 0, 0, 0), F).reshape(7, 1))
        out.append(c)
    return out


# ------------------------------------------------------------------------------------- the host program
def write_cases_bin(path: str, cases: list) -> None:
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            f.write(struct.pack("6i5f", c["n"], c["width"], c["height"], c["surfaces"], c["clipping"], c["num_steps"],
                                c["max_distance"], c["ground_z"], *[float(x) for x in c["half"]]))
            f.write(f32(c["dirs"]) + f32(c["offset"]) + f32(c["root_pos"]) + f32(c["root_quat"]) + f32(c["stones"]))


def read_out_bin(path: str, cases: list) -> list:
    raw = open(path, "rb").read()
    out, o = [], 0
    for c in cases:
        shapes = out_shapes(c["n"], c["width"] * c["height"])
        r = {}
        for name, dtype in OUTPUTS:
            size = int(np.prod(shapes[name])) * 4
            r[name] = np.frombuffer(raw[o:o + size], dtype).reshape(shapes[name]).copy()
            o += size
        out.append(r)
    assert o == len(raw), (o, len(raw))
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


# ------------------------------------------------------------------------------------- an independent float64 check
def rotation_matrix(q):
    """(n, 3, 3) float64 rotation matrices of (n, 4) quaternions (w, x, y, z), normalised first."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def independent64(c, pose):
    """Depth images in float64 by another route than the header's: rotation matrices instead of quaternion
    sandwiches, the scene moved into the CAMERA frame -- the ground as a general plane, the stones as oriented boxes
    cut by their six face planes one by one (no slabs, no reciprocals) -- and the local ray directions used as they
    are.  ``pose`` (7, n) is the camera pose to use (the sensor's own output, promoted).  Returns t (n, R) (inf: a
    miss), plane (n, R) (nan: a miss), normal (n, R, 3) in the world frame, and margin (n, R): how far, in metres
    along the face or in t, the hit-or-miss / which-face decision is from flipping."""
    n, R = c["n"], c["width"] * c["height"]
    pos = np.asarray(pose[:3].T, np.float64)
    rot = rotation_matrix(pose[3:].T)  # camera -> world
    dl = np.asarray(c["dirs"].T, np.float64)  # (R, 3), camera frame
    half = np.asarray(c["half"], np.float64)
    st = np.asarray(c["stones"].T, np.float64).reshape(n, NUM_STONES, 3)
    t_best = np.full((n, R), np.inf)
    nrm_best = np.full((n, R, 3), np.inf)
    margin = np.full((n, R), np.inf)
    axes_w = np.eye(3)
    for e in range(n):
        rt = rot[e].T  # world -> camera
        cands = []  # (t (R,), normal_w (3,), slack (R,))
        if c["surfaces"] & GROUND:
            # plane through p0 = rt (0, 0, gz - pos) with the normal rt z
            nc = rt @ axes_w[2]
            p0 = rt @ (np.array([0.0, 0.0, c["ground_z"]]) - pos[e])
            den = dl @ nc
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (p0 @ nc) / den
            ok = (den < 0) & (t >= 0) & (t <= 1e6)
            cands.append((np.where(ok, t, np.inf), axes_w[2], np.full(R, np.inf)))
        if c["surfaces"] & STONES:
            for s in range(c["num_steps"]):
                cc = rt @ (st[e, s] - pos[e])  # the box centre in the camera frame
                ax = [rt @ axes_w[k] for k in range(3)]  # its axes there
                inside = all(abs(cc @ ax[k]) <= half[k] for k in range(3))
                for k in range(3):
                    for sgn in (-1.0, 1.0):
                        nc = sgn * ax[k]
                        den = dl @ nc
                        with np.errstate(divide="ignore", invalid="ignore"):
                            t = ((cc + sgn * half[k] * ax[k]) @ nc) / den
                        p = t[:, None] * dl - cc  # the hit relative to the centre
                        others = [j for j in range(3) if j != k]
                        slack = np.min([half[j] - np.abs(p @ ax[j]) for j in others], 0)
                        facing = (den > 0) if inside else (den < 0)  # the far face from inside, the near one outside
                        ok = facing & (t >= 0) & (t <= 1e6) & (slack >= 0)
                        cands.append((np.where(ok, t, np.inf), sgn * axes_w[k], np.where(ok, slack, np.inf),
                                      np.where(facing & (t >= 0) & (slack < 0), -slack, np.inf)))
        ts = np.stack([cd[0] for cd in cands])  # (C, R)
        order = np.argsort(ts, 0, kind="stable")
        first = order[0]
        t_best[e] = ts[first, np.arange(R)]
        nrm_best[e] = np.where(np.isfinite(t_best[e])[:, None], np.stack([cd[1] for cd in cands])[first], np.inf)
        # the decision's margin: the winning face's slack to its edges, the gap in t to the runner-up with another
        # normal, and the nearest miss of any face by its edges
        slack = np.stack([cd[2] for cd in cands])[first, np.arange(R)]
        near_miss = np.min([cd[3] for cd in cands if len(cd) > 3] or [np.full(R, np.inf)], 0)
        second = ts[order[1], np.arange(R)] if len(cands) > 1 else np.full(R, np.inf)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(second), second - t_best[e], np.inf)
        margin[e] = np.minimum(np.minimum(slack, near_miss), gap)
    with np.errstate(invalid="ignore"):
        plane = np.where(np.isfinite(t_best), t_best * dl[None, :, 0], np.nan)  # the camera frame's x: no rotation
    return t_best, plane, nrm_best, margin
