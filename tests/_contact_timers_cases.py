"""The contact-timer fixture (tests/golden/contact_timers.npz, made by tests/golden/gen_contact_timers.py from the
reference's own ContactSensor) and a float32 numpy restatement of csrc/allsteps_contact_timers.h.

Every array is env-minor, the device layout: impulses (updates, B, 3, n), timers (records, 4, B, n) in the row
order current_air, last_air, current_contact, last_contact, timestamps (records, n), resets (updates, n): the
envs reset after that update.  A case stores a record after every ``stride`` updates, after the resets."""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact_timers.npz")
CUR_AIR, LAST_AIR, CUR_CONTACT, LAST_CONTACT = range(4)


def load_cases():
    """The fixture's cases: dicts with name, dt, threshold, updates, stride, n, bodies, impulses, resets (a bool
    array, all False where the case has none), timers, timestamp."""
    d = np.load(GOLDEN)
    out = []
    for c in json.loads(str(d["cases"])):
        k = c["name"]
        if f"{k}_impulses" in d.files:
            imp = d[f"{k}_impulses"]
        else:  # two vectors per body picked by a contact pattern (updates, B, n)
            pat, vec = d[f"{k}_pattern"], d[f"{k}_vectors"]
            imp = np.where(pat[:, :, None, :] != 0, vec[1][None], vec[0][None]).astype(np.float32)
        resets = d[f"{k}_resets"].astype(bool) if f"{k}_resets" in d.files else np.zeros((c["updates"], c["n"]), bool)
        out.append(dict(c, impulses=imp, resets=resets, timers=d[f"{k}_timers"], timestamp=d[f"{k}_timestamp"]))
    return out


def host_update(timers, ts, imp, dt, threshold):
    """One sensor update of every (env, body), in place: timers (4, B, n), ts (n,), imp (B, 3, n) net impulses.
    float32 throughout, every operation rounded on its own, the reference's four lines in its order."""
    assert timers.dtype == ts.dtype == imp.dtype == np.float32
    dt, threshold = np.float32(dt), np.float32(threshold)
    ts_new = ts + dt
    elapsed = (ts_new - ts)[None, :]  # the float32 difference of the two timestamps, not dt
    ts[:] = ts_new
    f = imp / dt
    contact = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]) > threshold
    zero = np.float32(0)
    first_contact = (timers[CUR_AIR] > 0) & contact
    first_detached = (timers[CUR_CONTACT] > 0) & ~contact
    timers[LAST_AIR] = np.where(first_contact, timers[CUR_AIR] + elapsed, timers[LAST_AIR])
    timers[CUR_AIR] = np.where(~contact, timers[CUR_AIR] + elapsed, zero)
    timers[LAST_CONTACT] = np.where(first_detached, timers[CUR_CONTACT] + elapsed, timers[LAST_CONTACT])
    timers[CUR_CONTACT] = np.where(contact, timers[CUR_CONTACT] + elapsed, zero)
    return contact, first_contact, first_detached


def host_reset(timers, ts, mask):
    """ContactSensor.reset of the envs in a bool mask (n,), in place."""
    timers[:, :, mask] = 0
    ts[mask] = 0


def host_step(timers, ts, net, dt, threshold, done):
    """An env step: net (T, B, 3, n) impulses of its substeps, slot 0 the latest -- T updates oldest first, then
    the reset of the envs in ``done``.  Returns the counts (first contacts, first detaches, resets of an env with
    a non-zero timer)."""
    fc = fd = 0
    for slot in range(net.shape[0] - 1, -1, -1):
        _, a, b = host_update(timers, ts, np.ascontiguousarray(net[slot]), dt, threshold)
        fc, fd = fc + int(a.sum()), fd + int(b.sum())
    live = int(((timers != 0).any((0, 1)) & done).sum())
    host_reset(timers, ts, done)
    return fc, fd, live


def first_contact(timers, dt, abs_tol=1.0e-8):
    """compute_first_contact on restated timers: (n, B) bool.  The comparison is torch's of a float32 tensor with
    a Python float: the scalar is rounded to float32 first."""
    t = timers[CUR_CONTACT].T
    return (t > 0) & (t < np.float32(dt + abs_tol))


def first_air(timers, dt, abs_tol=1.0e-8):
    t = timers[CUR_AIR].T
    return (t > 0) & (t < np.float32(dt + abs_tol))
