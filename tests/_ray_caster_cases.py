"""Cases of the ray-caster tests: loaders of the two fixtures, the hand cases ``e`` with their exact answers, a
float64 slab oracle written independently of csrc/allsteps_ray_caster.h, and the runner of the host program.

A case is a dict in the device layouts: ``n``, ``num_rays``, ``attach_yaw_only``, ``surfaces`` (bit 0 the ground, bit 1
the stones), ``max_distance``, ``ground_z``, ``half`` (3,), ``rays`` (6, R), ``root_pos`` (3, n), ``root_quat``
(4, n), ``stones`` (60, n), all float32.  The fixture's cases (tests/golden/ray_caster.npz, from the reference's own
RayCaster code: gen_ray_caster.py) add ``starts_w`` / ``dirs_w`` (n, R, 3) float32, ``starts_w64`` / ``dirs_w64``
float64 and ``e_ref``; they are cast against both surfaces.

    python tests/_ray_caster_cases.py --write-host

rebuilds tests/golden/ray_caster_host.npz: the outputs of tests/ray_caster_check.cpp (the header alone, on the
host) on every case, which the GPU kernel must reproduce bit for bit.
"""

from __future__ import annotations

import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ray_caster.npz")
HOST = os.path.join(ROOT, "tests", "golden", "ray_caster_host.npz")
SRC = os.path.join(ROOT, "tests", "ray_caster_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]

GROUND, STONES = 1, 2
HIT_GROUND, MISS = -1, -2
NUM_STONES = 20
EPS32 = float(np.finfo(np.float32).eps)
INF = float("inf")


def load_cases() -> list:
    """The fixture's cases y, f, d."""
    d = np.load(GOLDEN)
    out = []
    for c in json.loads(str(d["cases"])):
        k = c["name"]
        out.append(dict(name=k, n=c["n"], num_rays=c["num_rays"], attach_yaw_only=bool(c["cfg"]["attach_yaw_only"]),
                        surfaces=GROUND | STONES, max_distance=float(c["cfg"]["max_distance"]),
                        ground_z=float(c["ground_z"]), half=np.asarray(c["half"], np.float32), cfg=c["cfg"],
                        e_ref=float(c["e_ref"]), rays=d[f"{k}_rays_local"], root_pos=d[f"{k}_root_pos"],
                        root_quat=d[f"{k}_root_quat"], stones=d[f"{k}_stones"], starts_w=d[f"{k}_starts_w"],
                        dirs_w=d[f"{k}_dirs_w"], starts_w64=d[f"{k}_starts_w64"], dirs_w64=d[f"{k}_dirs_w64"]))
    return out


# ---- the hand cases e: one env each, the root at the origin with the identity orientation and attach_yaw_only, so
# that a world ray is its local ray exactly (yaw = atan2(0, 1) = 0, sin 0 = 0, cos 0 = 1, norm 1); every coordinate,
# half extent (0.5, 0.5, 0.25) and direction component is a small dyadic number, every reciprocal a power of two:
# all arithmetic of the slab test is exact and the expected hits are stated, not computed.
E_HALF = (0.5, 0.5, 0.25)
FAR = (1024.0, 1024.0, -1024.0)  # where the unused stones lie
DOWN = (0.0, 0.0, -1.0)
ABOVE_4 = float(np.nextafter(np.float32(4.0), np.float32(np.inf)))
E_STONES = {
    0: (0.0, 0.0, 0.75),    # x, y in [-0.5, 0.5], top at z = 1
    1: (0.25, 0.0, 1.75),   # overlaps stone 0 in xy (x in [-0.25, 0.75]), top at z = 2: the higher one
    2: (4.0, 0.0, -0.5),    # top at z = -0.25, below the ground plane
    3: (8.0, 0.0, -0.25),   # top at z = 0: on the ground plane exactly
    4: (12.0, 0.0, 0.75),   # 4 and 5: one box twice
    5: (12.0, 0.0, 0.75),
}
# (name, surfaces, max_distance, [(start, direction, expected hit or None for a miss, expected surface)])
E_SCENES = [
    ("all", GROUND | STONES, 1e6, [
        ((-0.5, 0.0, 4.0), DOWN, (-0.5, 0.0, 1.0), 0),           # on the box's edge: the closed box is hit
        ((-0.5, -0.5, 4.0), DOWN, (-0.5, -0.5, 1.0), 0),         # on its corner
        ((0.0, 0.0, 4.0), DOWN, (0.0, 0.0, 2.0), 1),             # zero direction components, inside both slabs; and
                                                                 # two stones overlapping in xy: the higher one
        ((-0.75, 0.0, 4.0), DOWN, (-0.75, 0.0, 0.0), HIT_GROUND),  # zero component, outside the slab: the ground
        ((-0.4375, 0.0, 0.75), DOWN, (-0.4375, 0.0, 0.5), 0),    # start inside stone 0: its far (bottom) face
        ((20.0, 0.0, -1.0), DOWN, None, MISS),                   # start below the ground
        ((20.0, 0.0, 1.0), (0.0, 0.0, 1.0), None, MISS),         # upward
        ((4.0, 0.0, 4.0), DOWN, (4.0, 0.0, 0.0), HIT_GROUND),    # a stone top below the ground plane
        ((8.0, 0.0, 4.0), DOWN, (8.0, 0.0, 0.0), HIT_GROUND),    # equal t on the ground and a stone: the ground
        ((12.0, 0.0, 4.0), DOWN, (12.0, 0.0, 1.0), 4),           # equal t on two stones: the lower index
        ((-2.0, 0.0, 4.0), (0.5, 0.0, -1.0), (-0.5, 0.0, 1.0), 0),  # slanted, t = 3 in units of |dir|: the top edge
    ]),
    ("max_distance", GROUND | STONES, 3.0, [
        ((-0.5, 0.0, 4.0), DOWN, (-0.5, 0.0, 1.0), 0),           # t = 3 = max_distance: just inside
        ((-0.5, 0.0, ABOVE_4), DOWN, None, MISS),                # t = 3 + one ulp of 4: just beyond
        ((-0.75, 0.0, 4.0), DOWN, None, MISS),                   # the ground at t = 4
    ]),
    ("stones_only", STONES, 1e6, [
        ((-0.5, 0.0, 4.0), DOWN, (-0.5, 0.0, 1.0), 0),
        ((-0.75, 0.0, 4.0), DOWN, None, MISS),                   # nothing but the (unselected) ground below
    ]),
    ("ground_only", GROUND, 1e6, [
        ((-0.5, 0.0, 4.0), DOWN, (-0.5, 0.0, 0.0), HIT_GROUND),  # through the (unselected) stone
        ((20.0, 0.0, 1.0), (0.0, 0.0, 1.0), None, MISS),
    ]),
]


def hand_cases() -> list:
    """The scenes of E_SCENES as cases (n = 1) with ``expect_hits`` (3, R, 1) and ``expect_surface`` (R, 1)."""
    stones = np.tile(np.asarray(FAR, np.float32), NUM_STONES)
    for s, c in E_STONES.items():
        stones[3 * s: 3 * s + 3] = c
    out = []
    for name, surfaces, max_distance, rays in E_SCENES:
        R = len(rays)
        local = np.zeros((6, R), np.float32)
        hits = np.full((3, R, 1), np.inf, np.float32)
        surf = np.zeros((R, 1), np.int8)
        for r, (start, direction, hit, s) in enumerate(rays):
            local[:3, r], local[3:, r] = start, direction
            if hit is not None:
                hits[:, r, 0] = hit
            surf[r, 0] = s
        out.append(dict(name=f"e_{name}", n=1, num_rays=R, attach_yaw_only=True, surfaces=surfaces,
                        max_distance=max_distance, ground_z=0.0, half=np.asarray(E_HALF, np.float32), rays=local,
                        root_pos=np.zeros((3, 1), np.float32), root_quat=np.array([[1.0], [0], [0], [0]], np.float32),
                        stones=stones.reshape(60, 1).copy(), expect_hits=hits, expect_surface=surf))
    return out


def all_cases() -> list:
    return load_cases() + hand_cases()


def load_host() -> dict:
    """name -> dict(hits (3, R, n), surface (R, n) int8, pose (7, n)) of tests/golden/ray_caster_host.npz."""
    d = np.load(HOST)
    names = json.loads(str(d["names"]))
    return {k: {a: d[f"{k}_{a}"] for a in ("hits", "surface", "pose")} for k in names}


def tile_case(c: dict, n: int) -> dict:
    """The case's envs repeated (or cut) to n envs: env e is the case's env e % c['n']."""
    idx = np.arange(n) % c["n"]
    out = dict(c, n=n)
    for k in ("root_pos", "root_quat", "stones"):
        out[k] = np.ascontiguousarray(c[k][:, idx])
    return out


def cut_rays(c: dict, R: int) -> dict:
    """The case with its first R rays only."""
    return dict(c, num_rays=R, rays=np.ascontiguousarray(c["rays"][:, :R]))


# ---------------------------------------------------------------------------------------------- the host program
def write_cases_bin(path: str, cases: list) -> None:
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            f.write(struct.pack("5i5f", c["n"], c["num_rays"], int(c["attach_yaw_only"]), c["surfaces"], NUM_STONES,
                                c["max_distance"], c["ground_z"], *[float(x) for x in c["half"]]))
            f.write(f32(c["rays"]) + f32(c["root_pos"]) + f32(c["root_quat"]) + f32(c["stones"]))


def read_out_bin(path: str, cases: list) -> list:
    """Per case: dict(hits, surface, pose, starts_w (3, R, n), dirs_w (3, R, n)) of the program's output."""
    raw = open(path, "rb").read()
    out, o = [], 0
    for c in cases:
        n, R = c["n"], c["num_rays"]
        r = {}
        for name, dtype, shape in (("hits", np.float32, (3, R, n)), ("surface", np.int8, (R, n)),
                                   ("pose", np.float32, (7, n)), ("starts_w", np.float32, (3, R, n)),
                                   ("dirs_w", np.float32, (3, R, n))):
            size = int(np.prod(shape)) * np.dtype(dtype).itemsize
            r[name] = np.frombuffer(raw[o:o + size], dtype).reshape(shape).copy()
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


# ---------------------------------------------------------------------------------------------- float64 oracle
def oracle64(starts, dirs, stones, half, surfaces, max_distance, ground_z):
    """Nearest hit of world rays in float64.  starts, dirs (n, R, 3); stones (n, S, 3) centres; half (3,).  Returns
    t (n, R) (inf: a miss), surface (n, R) int, hit (n, R, 3).  Divisions by the direction (not reciprocals), boxes
    as intervals per axis; ties: the ground, then the lowest stone."""
    o, d = np.asarray(starts, np.float64), np.asarray(dirs, np.float64)
    n, R, _ = o.shape
    best_t = np.full((n, R), np.inf)
    best_s = np.full((n, R), MISS, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if surfaces & GROUND:
            t = (ground_z - o[..., 2]) / d[..., 2]
            ok = (d[..., 2] < 0) & (t >= 0) & (t <= max_distance)
            best_t, best_s = np.where(ok, t, best_t), np.where(ok, HIT_GROUND, best_s)
        if surfaces & STONES:
            c = np.asarray(stones, np.float64)
            h = np.asarray(half, np.float64)
            for s in range(c.shape[1]):
                lo, hi = (c[:, s] - h)[:, None, :], (c[:, s] + h)[:, None, :]  # (n, 1, 3)
                ta, tb = (lo - o) / d, (hi - o) / d
                par = d == 0
                inside = (o >= lo) & (o <= hi)
                near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
                far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
                tn, tf = near.max(-1), far.min(-1)
                t = np.where(tn >= 0, tn, tf)
                ok = (tn <= tf) & (tf >= 0) & (t <= max_distance) & (t < best_t)
                best_t, best_s = np.where(ok, t, best_t), np.where(ok, s, best_s)
    hit = np.where((best_s == MISS)[..., None], np.inf, o + np.where(np.isfinite(best_t), best_t, 0.0)[..., None] * d)
    return best_t, best_s, hit


def check_hits(name, starts32, dirs32, hits32, surface, stones, half, surfaces, max_distance, ground_z):
    """The rule of the issue for hits computed in float32 from the float32 world rays (n, R, 3): against the float64
    oracle on the same rays promoted, the surface is equal and |hit - hit64|inf <= 8 eps32 (|o|inf + |c|inf + |h|inf
    + t |d|inf), c and h the hit box's centre and half extents (the ground: its height and 0).  Rays whose hit-or-
    miss decision lies within 1e-4 m of a box edge -- the oracle's surface changes when every box grows or shrinks
    by 1e-4 m -- are skipped.  Returns (skipped share, stone-hit share of the judged rays, largest error / bound)."""
    half = np.asarray(half, np.float64)
    t, s, hit = oracle64(starts32, dirs32, stones, half, surfaces, max_distance, ground_z)
    skip = np.zeros(s.shape, bool)
    for dh in (1e-4, -1e-4):
        skip |= oracle64(starts32, dirs32, stones, half + dh, surfaces, max_distance, ground_z)[1] != s
    judged = ~skip
    assert np.array_equal(np.asarray(surface, np.int64)[judged], s[judged]), \
        (name, "surfaces differ on", int((np.asarray(surface)[judged] != s[judged]).sum()), "rays")
    o, d = np.asarray(starts32, np.float64), np.asarray(dirs32, np.float64)
    c = np.asarray(stones, np.float64)
    idx = np.clip(s, 0, c.shape[1] - 1)
    cmax = np.abs(np.take_along_axis(c, idx[..., None].repeat(3, -1), 1)).max(-1)  # (n, R)
    cmax = np.where(s >= 0, cmax, abs(ground_z))
    hmax = np.where(s >= 0, half.max(), 0.0)
    hitting = judged & (s != MISS)
    bound = 8 * EPS32 * (np.abs(o).max(-1) + cmax + hmax + np.where(hitting, t, 0.0) * np.abs(d).max(-1))
    err = np.abs(np.asarray(hits32, np.float64) - hit)
    err = np.where(np.isfinite(hit), err, np.where(np.asarray(hits32) == hit, 0.0, np.inf)).max(-1)
    worst = float((err[judged] / bound[judged]).max())
    assert worst <= 1.0, (name, "largest hit error / bound", worst)
    return float(skip.mean()), float((s[judged] >= 0).mean()), worst


def stones_nk3(stones_rows: np.ndarray) -> np.ndarray:
    """(60, n) device rows -> (n, 20, 3) centres."""
    return np.ascontiguousarray(stones_rows.T).reshape(-1, NUM_STONES, 3)


def main(argv=None) -> int:
    if (argv or sys.argv[1:]) != ["--write-host"]:
        print(__doc__)
        return 2
    cases = all_cases()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ray_caster_check")
        build_program(exe)
        stdout, outs = run_program(exe, tmp, cases)
    print(stdout)
    arrays = {"names": np.array(json.dumps([c["name"] for c in cases]))}
    for c, r in zip(cases, outs):
        for a in ("hits", "surface", "pose"):
            arrays[f"{c['name']}_{a}"] = r[a]
    np.savez_compressed(HOST, **arrays)
    print(f"wrote {HOST} ({os.path.getsize(HOST)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
