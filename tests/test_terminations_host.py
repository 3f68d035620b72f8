"""The termination manager's shared code (csrc/allsteps_terminations.h) on the host.

tests/terminations_check.cpp is a stand-alone program (its own main) around the header.  On
tests/golden/terminations.npz -- the reference's own TerminationManager.compute / reset / set_term_cfg with its term
functions on recorded inputs (tests/golden/gen_terminations.py) -- and the device tables the env's host code makes of
the same cfgs (envs/terminations.py):

  cases a, b, c: every flag of every term is the reference's bit for bit, and so are time_outs, terminated, dones and
      last_episode_dones; the counts of the by-hand resets are the reference's reset(env_ids) extras;
  bad_orientation, whose angle passes the library's atan2, is held to the reference's flag wherever the float64 angle
      lies farther from float32(limit_angle) than the bound B of _terminations_cases.orientation_band; the words
      inside the band are exactly the ones the fixture lists (none in cases a and b; in case c the envs with -g.z = -1,
      0 and nextafter(1, 2)), and of those the two that do not sit on the limit are held all the same;
  the header's angle itself lies within B of the float64 angle everywhere (a NaN only where x may pass 1);
  case d (case a's rows with step flags, made here): the NumPy restatement of tests/_terminations_cases.py equals the
      header in every word of every buffer, as it does on a, b and c.

term_acosf against float64 over a sweep of [-1, 1] stays under _terminations_cases.ACOS_ERR = 3 2^-22 = 7.2e-7 rad.
Measured: 3.125e-7 rad (at x = -0.665, where the result is above 2 and one ulp is 2.4e-7); the header's angle uses at
most 0.205 of B on the fixture.  Built once plain and once with -fsanitize=address,undefined; both run directly."""

import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "terminations_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]

sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_cases(path, cases) -> None:
    from _terminations_cases import SOURCES

    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            x = c["inputs"]
            flags = "step_terminated" in c
            f.write(struct.pack("8if", c["n"], len(c["names"]), c["steps"], x["q"].shape[1], x["net"].shape[1],
                                x["net"].shape[2], x["time_left"].shape[1], int(flags), c["sim_dt"]))
            for s in range(c["steps"]):
                spec = c["specs"][s]
                f.write(np.ascontiguousarray(spec.rows, np.float32).tobytes())
                f.write(np.ascontiguousarray(spec.table, np.float32).tobytes())
                for k in SOURCES:
                    f.write(np.ascontiguousarray(x[k][s]).tobytes())
                if flags:
                    f.write(np.ascontiguousarray(c["step_terminated"][s], np.uint8).tobytes())
                    f.write(np.ascontiguousarray(c["step_truncated"][s], np.uint8).tobytes())


def read_dump(path, cases) -> list:
    raw = np.fromfile(path, np.uint8)
    out, at = [], 0
    for c in cases:
        n, T = c["n"], len(c["names"])
        steps = []
        for _ in range(c["steps"]):
            d = {}
            for key, shape in (("term_dones", (T, n)), ("time_outs", (n,)), ("terminated", (n,)), ("dones", (n,)),
                               ("last_episode_dones", (T, n)), ("reset_request", (n,))):
                size = int(np.prod(shape))
                d[key] = raw[at:at + size].reshape(shape)
                at += size
            d["angle"] = raw[at:at + 4 * n].view(np.float32)
            at += 4 * n
            steps.append(d)
        out.append(steps)
    assert at == raw.size
    return out


def build_check(tmp_path, flags=()):
    exe = tmp_path / "terminations_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def cases():
    from _terminations_cases import load_cases

    return load_cases()


def with_step_flags(case: dict) -> dict:
    """Case d: a case's rows with step flags -- a seventh of the envs terminated by the step, a seventh truncated."""
    rng = np.random.default_rng(7)
    d = dict(case, name="d")
    d["step_terminated"] = (rng.uniform(0, 1, (case["steps"], case["n"])) < 0.15).astype(np.uint8)
    d["step_truncated"] = (rng.uniform(0, 1, (case["steps"], case["n"])) < 0.15).astype(np.uint8)
    return d


def test_fixture_is_small_and_has_the_cases(cases):
    from _terminations_cases import FIXTURE

    assert os.path.getsize(FIXTURE) <= 400 << 10  # well under the rewards fixture's 803 KiB: the flags are bytes
    assert [c["name"] for c in cases] == ["a", "b", "c"]
    a, b, c = cases
    assert a["n"] == 66 and len(a["names"]) == 9 and a["steps"] == 12 and b["steps"] == 6 and c["steps"] == 3
    assert a["inputs"]["q"].shape[1:] == (12, 66) and a["inputs"]["net"].shape[1:] == (4, 5, 3, 66)
    k = a["names"].index("height")
    assert [bool(s.terms[k].time_out) for s in a["specs"]] == [False] * 4 + [True] * 4 + [False] * 4
    assert [r["step"] for r in a["resets"]] == [3, 9] and a["resets"][0]["env_ids"] == [5, 40]
    assert a["band_words"] == [] and b["band_words"] == []
    assert sorted({e for _, e in c["band_words"]}) == [18, 19, 20]
    for case in cases:  # every term both set and clear, both kinds of done, not every env done
        f = case["flags"]
        assert f.any(axis=(0, 2)).all() and not f.all(axis=(0, 2)).any()
        assert case["time_outs"].any() and case["terminated"].any() and not case["dones"].all()
    x = c["inputs"]
    assert np.isnan(x["q"]).any() and np.isposinf(x["q"]).any() and np.isneginf(x["q"]).any()
    assert np.isnan(x["qd"]).any() and np.isposinf(x["qd"]).any() and np.isneginf(x["qd"]).any()
    assert not x["net"][:, :, :, :, 15].any()  # an all-zero history
    ids = {t["name"]: t["params"] for t in c["terms"]}
    assert ids["jvel_manual"]["joint_ids"] == [3] and "joint_ids" not in ids["jpos_manual"]
    assert ids["contact_base"]["body_ids"] == [0] and ids["contact_all"]["body_ids"] is None


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_terminations_header_reproduces_the_reference(tmp_path, orc, cases, flags):
    from _terminations_cases import (BUFFERS, host_step, oracle_atan2, orientation_angle64, orientation_band,
                                     orientation_dx, orientation_held, step_inputs, zero_state)

    run = list(cases) + [with_step_flags(cases[0])]
    write_cases(tmp_path / "cases.bin", run)
    exe = build_check(tmp_path, flags)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "dump.bin")], capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "terminations fixture: 4 cases" in r.stdout and " 0 set" not in r.stdout and " 0 done" not in r.stdout
    dump = read_dump(tmp_path / "dump.bin", run)
    atan2 = oracle_atan2(orc)
    worst = 0.0
    for c, steps in zip(run, dump):
        T, n = len(c["names"]), c["n"]
        state = zero_state(T, n)
        ko = c["names"].index("orientation")
        limit = c["terms"][ko]["params"]["limit_angle"]
        loose = np.zeros(n, bool)  # envs with an orientation word inside the band so far: their unions are not held
        for s, got in enumerate(steps):
            where = (c["name"], s)
            x = step_inputs(c, s)
            # the NumPy restatement equals the header, every word of every buffer
            flags_ = {k: c[k][s] for k in ("step_terminated", "step_truncated")} if c["name"] == "d" else {}
            state = host_step(c["specs"][s], x, state, c["sim_dt"], atan2, **flags_)
            for key in BUFFERS:
                assert np.array_equal(state[key], got[key]), (where, key)
            # the header's angle lies within B of the float64 angle
            _, a64 = orientation_angle64(x["root_quat"])
            band = orientation_band(x["root_quat"])
            x64, _ = orientation_angle64(x["root_quat"])
            nan = np.isnan(got["angle"])
            assert (np.abs(x64[nan]) + orientation_dx(x["root_quat"].astype(np.float64))[nan] > 1.0).all(), where
            fin = np.isfinite(band) & ~nan
            frac = np.abs(got["angle"][fin].astype(np.float64) - a64[fin]) / band[fin]
            worst = max(worst, float(frac.max()))
            assert frac.max() <= 1.0, (where, float(frac.max()))
            if c["name"] == "d":
                continue
            fin = np.isfinite(a64)
            assert np.allclose(a64[fin], c["angle64"][s][fin], rtol=0, atol=1e-12), where
            assert np.array_equal(np.isnan(a64), np.isnan(c["angle64"][s])), where
            # the reference's flags, bit for bit; bad_orientation where it is held
            held = orientation_held(x["root_quat"], limit)
            assert [[s, int(e)] for e in np.nonzero(~held)[0]] == [w for w in c["band_words"] if w[0] == s], where
            for k, name in enumerate(c["names"]):
                sel = held if k == ko else np.ones(n, bool)
                assert np.array_equal(got["term_dones"][k][sel], c["flags"][s, k][sel]), (where, name)
            if c["name"] == "c":  # -g.z = -1 and nextafter(1, 2) are exact inputs: held although B is infinite
                for e in (18, 20):
                    assert got["term_dones"][ko][e] == c["flags"][s, ko][e], (where, e)
                loose[19] = True
            keep = ~loose
            for key, ref in (("time_outs", "time_outs"), ("terminated", "terminated"), ("dones", "dones")):
                assert np.array_equal(got[key][keep], c[ref][s][keep]), (where, key)
            assert np.array_equal(got["last_episode_dones"][:, keep], c["last"][s][:, keep]), where
            assert np.array_equal(got["reset_request"], got["dones"]), where  # no step flags in the fixture's cases
            for reset in c["resets"]:
                if reset["step"] == s:
                    for k, name in enumerate(c["names"]):
                        count = int(np.count_nonzero(got["term_dones"][k][reset["env_ids"]]))
                        assert count == reset["extras"][f"Episode_Termination/{name}"], (where, name)
    print("bad_orientation: the header's angle uses at most", round(worst, 3), "of its band")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_acosf_against_float64_over_a_sweep(tmp_path, orc):
    from _terminations_cases import ACOS_ERR, acosf, oracle_atan2

    f = np.float32
    one = np.float32(1.0)
    near = np.float32(1.0) - np.arange(0, 8192, dtype=np.float64) * 2.0 ** -24  # every float32 just under 1
    x = np.concatenate([np.linspace(-1.0, 1.0, (1 << 21) + 1), near, -near, [0.0, -0.0, 2.0 ** -30, -2.0 ** -126,
                                                                              0.5, -0.5, 2.0 ** -0.5]]).astype(f)
    edge = np.array([np.nextafter(one, f(2)), -np.nextafter(one, f(2)), 2.0, -np.inf, np.inf, np.nan], f)
    x.tofile(tmp_path / "x.bin")
    edge.tofile(tmp_path / "edge.bin")
    exe = build_check(tmp_path)
    for name in ("x", "edge"):
        r = subprocess.run([str(exe), "acos", str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}_out.bin")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
    y = np.fromfile(tmp_path / "x_out.bin", f)
    err = np.abs(y.astype(np.float64) - np.arccos(x.astype(np.float64)))
    i = int(err.argmax())
    print(f"term_acosf: max |error| against float64 {err.max():.3e} rad at x = {x[i]!r}; bound {ACOS_ERR:.3e}")
    assert err.max() <= ACOS_ERR
    assert y[x == one][0] == 0.0 and abs(float(y[x == -one][0]) - np.pi) <= 2.0 ** -22
    assert np.isnan(np.fromfile(tmp_path / "edge_out.bin", f)).all()  # NaN outside [-1, 1] and for a NaN, as torch
    # the NumPy restatement is the same function
    got = acosf(x, oracle_atan2(orc))
    assert np.array_equal(got.view(np.uint32), y.view(np.uint32))
    assert np.isnan(acosf(edge, oracle_atan2(orc))).all()


def test_torch_takes_the_thresholds_as_float32(cases):
    """Case c's rows sit on float32(threshold) for thresholds that are not float32 values and round to the side on
    which a comparison made in double would raise the flag: the reference's flags there are clear."""
    c = cases[2]
    p = {t["name"]: t["params"] for t in c["terms"]}
    x, f32 = c["inputs"], np.float32
    v, h, thr = p["jvel_manual"]["max_velocity"], p["height"]["minimum_height"], p["contact_base"]["threshold"]
    lo, hi = p["jpos_manual"]["bounds"]
    assert float(f32(v)) > v and float(f32(h)) < h and float(f32(thr)) > thr and float(f32(hi)) > hi
    assert float(f32(lo)) < lo
    rows = (("jvel_manual", x["qd"][:, 3, 8], f32(v)), ("jvel_manual", x["qd"][:, 3, 9], -f32(v)),
            ("height", x["root_pos"][:, 2, 10], f32(h)), ("jpos_manual", x["q"][:, 4, 6], f32(hi)),
            ("jpos_manual", x["q"][:, 9, 6], f32(lo)),
            ("contact_base", x["net"][:, 2, 0, 0, 14] / f32(c["sim_dt"]), f32(thr)))
    for (name, row, value), e in zip(rows, (8, 9, 10, 6, 6, 14)):
        assert (row == value).all(), name
        assert not c["flags"][:, c["names"].index(name), e].any(), name


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_terminations.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
