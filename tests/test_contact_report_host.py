"""The contact report's shared host header (csrc/allsteps_contact_report.h) and its ABI, without a GPU.

* tests/contact_report_check.cpp is a stand-alone program (its own main) around the header: the ids packing, the
  buffer indices and the per-env reductions k_contact_forces runs, against a record-by-record restatement, in
  bits -- zero contacts, AS_MAX_CONTACTS contacts, repeated (foot, stone) keys, self-contacts, foot = -1, a
  second link that is some body's link, a sparse body table, 2000 random mixes; the env under test sits among
  envs of random filler.  Built once plain and once with -fsanitize=address,undefined; both run directly.
* the header's as_contact_report_t fields equal the ctypes struct's, and the header's declared functions equal
  EXPORTED_SYMBOLS (the checks tests/test_abi.py makes for the earlier structs);
* every geom link of both shipped models carries a body, so no contact falls outside the net-force view, and
  each sensor foot's link carries exactly one.
"""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "contact_report_check.cpp")
HEADER = os.path.join(ROOT, "include", "allsteps.h")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_contact_report_reductions(tmp_path, flags):
    exe = tmp_path / "contact_report_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "contact report: 2007 cases, 0 mismatches" in r.stdout


def _struct_fields(name):
    src = open(HEADER).read()
    m = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + ";", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            for part in decl.split(","):
                names.append(re.findall(r"\*?\s*(\w+)\s*(?:\[[^\]]*\])*\s*$", part.strip())[0])
    return names


def test_contact_report_struct_matches_header():
    from allsteps_isaaclab_amd import _native

    assert [f[0] for f in _native.AsContactReport._fields_] == _struct_fields("as_contact_report_t")
    assert _struct_fields("as_contact_report_t") == ["depth", "count", "records", "qd_prev"]


def test_header_functions_are_the_exported_symbols():
    from allsteps_isaaclab_amd import _native

    src = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(as_\w+)\(", src, re.M))
    assert {"as_set_contact_report", "as_contact_forces"} <= declared
    assert set(_native.EXPORTED_SYMBOLS) == declared
    L = _native.load()
    for fn in ("as_set_contact_report", "as_contact_forces"):
        assert hasattr(L, fn) and getattr(L, fn).argtypes is not None
    assert L.as_abi_version() == _native.ABI_VERSION == 6
    consts = dict(re.findall(r"^#define (AS_\w+) (\d+)", src, re.M))
    assert int(consts["AS_REPORT_WORDS"]) == _native.REPORT_WORDS and int(consts["AS_REPORT_FEET"]) == _native.REPORT_FEET
    assert int(consts["AS_MAX_CONTACTS"]) == _native.MAXC and int(consts["AS_NUM_STONES"]) == _native.NUM_STONES


def test_null_handle_and_null_outputs_are_refused_without_a_device():
    from allsteps_isaaclab_amd import _native

    L = _native.load()
    assert L.as_set_contact_report(None, None) == -1 and b"null handle" in L.as_last_error()
    assert L.as_contact_forces(None, None, None, None, None) == -1 and b"null argument" in L.as_last_error()


@pytest.mark.parametrize("which", ["walker3d", "anymal_c"])
def test_every_geom_link_carries_exactly_one_body(which):
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    m = load_model() if which == "walker3d" else load_model(ANYMAL_C_JSON)
    body_link = [int(x) for x in m["body_link"][: int(m["num_bodies"])]]
    geom_link = {int(x) for x in m["geom_link"][: int(m["num_geoms"])]}
    assert geom_link <= set(body_link), sorted(geom_link - set(body_link))
    # the sensor feet resolve to one body each (the views pick net_forces_w rows by these); bodies that a
    # fixed joint merged into one link (the walker's head / torso, lower arm / hand) each show that link's sum
    ng = int(m["num_geoms"])
    feet = sorted({int(f) for f in m["geom_foot"][:ng] if int(f) >= 0})
    assert feet == list(range(2 if which == "walker3d" else 4))
    for f in feet:
        links = {int(m["geom_link"][g]) for g in range(ng) if int(m["geom_foot"][g]) == f}
        assert len(links) == 1 and body_link.count(links.pop()) == 1
