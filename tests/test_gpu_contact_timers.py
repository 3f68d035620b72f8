"""The contact sensors' air / contact timers on the device (csrc/contact_timer_kernels.h, envs/views.py; -m gpu).

Kernel level: as_contact_timers on hand-built contact reports that carry the fixture's impulses
(tests/golden/contact_timers.npz, the reference's own ContactSensor): timers and timestamps bit for bit after every
launch, with guard words behind both buffers, a six-body table (two body groups) and a self-contact record.  Env
level: the walker and the quadruped in lock-step with the float32 numpy restatement (_contact_timers_cases) fed the
net impulses the force views serve, HIP-graph replay, the reset paths, state round trip, shards, a feature-off
twin whose outputs and state must not move, and the entry point's refusals.

The envs' actions come from numpy generators on the host.  Seeds, amplitudes and lengths were chosen with the CPU
oracle (its contact probe for the walker, its contact masks for the quadruped) stepping the same actions: at 300
envs the walker makes some 2600 first contacts, 2200 first detaches and 1100 resets in 80 steps, the quadruped
7600 / 7300 and 13 resets in 40 steps at amplitude 3 (one reset at amplitude 1.2: too thin)."""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 300  # four 64-env workgroups and a fifth with a tail of 44
DEPTH = 4


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(shape):
    """(buffer, view): zeros of `shape` on the device with 64 NaN guard words behind them."""
    size = int(np.prod(shape))
    buf = torch.zeros(size + 64, dtype=torch.float32, device=DEV)
    buf[size:] = float("nan")
    return buf, buf[:size].view(shape)


@pytest.fixture(scope="module")
def cases():
    from _contact_timers_cases import load_cases

    return {c["name"]: c for c in load_cases()}


# ------------------------------------------------------------------ 1. the kernel against the fixture

# a record: (fixture body, scale, table body of its link, table body of its second link or None)
SIMPLE = dict(links=[5, 9], expect=[0, 1], records=[(0, 1.0, 0, None), (1, 1.0, 1, None)])
# six bodies = two body groups: body 2 takes fixture body 1's impulse as two halves (x / 2 + x / 2 is x), body 4
# takes fixture body 0's from a self-contact as its first link and body 5 as its second link -- the negated
# impulse, the same norm, so the same timers
SIX = dict(links=[5, 9, 2, 14, 7, 11], expect=[0, 1, 1, 0, 0, 0],
           records=[(0, 1.0, 0, None), (1, 1.0, 1, None), (1, 0.5, 2, None), (0, 1.0, 3, None), (1, 0.5, 2, None),
                    (0, 1.0, 4, 5)])


def _report_of(imp, n, layout):
    """(count (L, 4, n), records (L, 4, 8, 10, n)) int32 device tensors for impulses (U, B, 3, nfix): launch k holds
    updates 4 k .. 4 k + 3, the oldest in slot 3.  Slots past the count hold a live-looking record that must not
    be read."""
    from allsteps_isaaclab_amd import _native

    updates = imp.shape[0]
    assert updates % DEPTH == 0
    env = np.arange(n) % imp.shape[-1]
    launches = updates // DEPTH
    rec = np.zeros((launches, DEPTH, _native.REPORT_WORDS, _native.MAXC, n), np.int32)
    links = layout["links"]
    nrec = len(layout["records"])
    for c, (fb, scale, b1, b2) in enumerate(layout["records"]):
        v = (imp[:, fb][:, :, env] * np.float32(scale)).astype(np.float32)  # (U, 3, n)
        v = v.reshape(launches, DEPTH, 3, n)[:, ::-1]  # slot 0 = the launch's last update
        rec[:, :, 0:3, c] = v.view(np.int32)
        ids = links[b1] | ((links[b2] + 1) << 8 if b2 is not None else 0) | ((0 if b2 is not None else 1) << 16)
        rec[:, :, 7, c] = ids
    rec[:, :, 0:3, nrec] = np.float32(1e3).view(np.int32)  # past the count: a huge impulse on body 0's link
    rec[:, :, 7, nrec] = links[0] | 1 << 16
    count = np.full((launches, DEPTH, n), nrec, np.int32)
    return torch.from_numpy(count).to(DEV), torch.from_numpy(rec).to(DEV)


def _table(links):
    from allsteps_isaaclab_amd import _native

    t = _native.AsBodyTable()
    t.num_bodies = len(links)
    for k, link in enumerate(links):
        t.link[k] = link
    return t


def _run_case(orc, c, n, layout):
    """The fixture case through as_contact_timers, 4 updates a launch: mismatching words over all launches."""
    from _models import GpuPhysics

    from allsteps_isaaclab_amd import _native

    assert c["dt"] == 1 / 240  # the walker's sim.dt, which the kernel divides by
    gpu = GpuPhysics(orc.m, n)
    nat = gpu.native
    count = torch.zeros(DEPTH, n, dtype=torch.int32, device=DEV)
    records = torch.zeros(DEPTH, _native.REPORT_WORDS, _native.MAXC, n, dtype=torch.int32, device=DEV)
    qd_prev = torch.zeros(21, n, device=DEV)
    nat.set_contact_report(DEPTH, count, records, qd_prev)
    all_count, all_records = _report_of(c["impulses"], n, layout)
    env = np.arange(n) % c["n"]
    per_launch = DEPTH // c["stride"]  # fixture records per launch: the last one is the launch's
    want_t = torch.from_numpy(np.ascontiguousarray(
        c["timers"][per_launch - 1::per_launch][:, :, layout["expect"]][..., env])).to(DEV)
    want_ts = torch.from_numpy(np.ascontiguousarray(c["timestamp"][per_launch - 1::per_launch][:, env])).to(DEV)
    resets = torch.from_numpy(np.ascontiguousarray(c["resets"][DEPTH - 1::DEPTH][:, env]).astype(np.uint8)).to(DEV)
    table = _table(layout["links"])
    nb = len(layout["links"])
    bt, timers = _guarded((4, nb, n))
    bs, ts = _guarded((n,))
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    first_bad = None
    for k in range(all_count.shape[0]):
        count.copy_(all_count[k])
        records.copy_(all_records[k])
        nat.contact_timers(table, timers, ts, c["threshold"], DEPTH, resets[k], None, stream=_stream())
        miss = (_bits(timers) != _bits(want_t[k])).sum() + (_bits(ts) != _bits(want_ts[k])).sum()
        bad += miss
        if first_bad is None and c["updates"] <= 240 and int(miss):
            first_bad = k
    torch.cuda.synchronize()
    guards = bool(torch.isnan(bt[4 * nb * n:]).all()) and bool(torch.isnan(bs[n:]).all())
    live = int((want_t != 0).sum())
    gpu.close()
    return int(bad), first_bad, guards, live


@pytest.mark.parametrize("layout", [SIMPLE, SIX], ids=["two_bodies", "six_bodies_self_contact"])
def test_kernel_reproduces_the_reference_on_case_a(orc, cases, layout):
    """Case a (240 updates, contact made and broken, resets after env steps) in 60 launches at n = 300: timers and
    timestamps bit-equal to the reference after every launch."""
    bad, first_bad, guards, live = _run_case(orc, cases["a"], N, layout)
    assert bad == 0, f"{bad} words differ, first in launch {first_bad}"
    assert guards and live > 1000


@pytest.mark.parametrize("name,n", [("c0", 6), ("c1", 6), ("b", 3), ("a", 1), ("a", 65)])
def test_kernel_reproduces_the_threshold_edges_the_long_run_and_small_grids(orc, cases, name, n):
    """c0 / c1: forces exactly at the threshold and an ulp above it, default and non-default threshold; b: 900
    launches without a reset, where elapsed drifts from dt; a at n = 1 and at 65 (a second workgroup of one env)."""
    bad, first_bad, guards, live = _run_case(orc, cases[name], n, SIMPLE)
    assert bad == 0, f"{name}: {bad} words differ, first in launch {first_bad}"
    assert guards and live > 0


# ------------------------------------------------------------------ 2, 3. the envs against the restatement

def _walker(n=N, air=True, seed=42, offset=0, forces=False, threshold=None):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.contact_air_time = air
    cfg.contact_forces = forces
    if threshold is not None:
        cfg.contact_force_threshold = threshold
    return AllstepsEnv(cfg, env_id_offset=offset)


def _quadruped(n=N, air=True, seed=42):
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.contact_air_time = air
    return AnymalCStonesEnv(cfg)


def _actions(n, cols, steps, seed=3, amp=1.0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.uniform(-amp, amp, (n, cols)).astype(np.float32)).to(DEV) for _ in range(steps)]


def _foot_impulses(env):
    """(T, B, 3, N) float32 net impulses of the sensor feet over the last step's substeps, slot 0 the latest:
    what net_forces_w_history shows, before its division by dt."""
    rep = env._report
    _, net = rep.forces()
    feet = range(env._contact_timers.num_bodies)
    return net[:, [rep.foot_body[f] for f in feet]].cpu().numpy()


def _lock_step(env, cols, steps, amp):
    """Step the env and the restatement together; returns (first contacts, first detaches, resets of live timers)."""
    from _contact_timers_cases import first_air, first_contact, host_step

    tm = env._contact_timers
    n, nb = env.num_envs, tm.num_bodies
    timers, ts = np.zeros((4, nb, n), np.float32), np.zeros(n, np.float32)
    env.reset()
    assert not bool(tm.timers.any()) and not bool(tm.timestamp.any())
    dt, thr = env.cfg.sim.dt, env.cfg.contact_force_threshold
    totals = np.zeros(3, np.int64)
    seen_first = 0
    for k, act in enumerate(_actions(n, cols, steps, amp=amp)):
        _, _, term, trunc, _ = env.step(act)
        done = (term | trunc).cpu().numpy()
        totals += host_step(timers, ts, _foot_impulses(env), dt, thr, done)
        assert np.array_equal(tm.timers.cpu().numpy().view(np.uint32), timers.view(np.uint32)), k
        assert np.array_equal(tm.timestamp.cpu().numpy().view(np.uint32), ts.view(np.uint32)), k
        if k % 8 == 7:
            s = env.sensor
            fc, fa = s.compute_first_contact(env.step_dt), s.compute_first_air(env.step_dt)
            assert np.array_equal(fc.cpu().numpy(), first_contact(timers, env.step_dt)), k
            assert np.array_equal(fa.cpu().numpy(), first_air(timers, env.step_dt)), k
            seen_first += int(fc.sum()) + int(fa.sum())
    print(f"first contacts {totals[0]}, first detaches {totals[1]}, resets of an env with live timers {totals[2]}")
    assert steps < 8 or seen_first > 0, "compute_first_contact / compute_first_air never answered True"
    return totals, timers


def test_walker_timers_equal_the_restatement_step_by_step():
    env = _walker()
    assert env._report is not None and env.cfg.contact_forces is False  # the timers bring the report themselves
    totals, timers = _lock_step(env, 21, 80, 1.0)
    assert totals.min() >= 1, "the run missed a first contact, a first detach or a reset of live timers"
    # the three sensors share the one set: (N, B) zero-copy views in sensor order right, left
    d, r, l = env.sensor.data, env.sensor_right.data, env.sensor_left.data
    for row, name in enumerate(("current_air_time", "last_air_time", "current_contact_time", "last_contact_time")):
        v = getattr(d, name)
        assert v.shape == (N, 2) and v.data_ptr() == env._contact_timers.timers[row].data_ptr()
        assert np.array_equal(v.cpu().numpy(), timers[row].T)
        assert torch.equal(getattr(r, name), v[:, :1]) and torch.equal(getattr(l, name), v[:, 1:])
    assert env.sensor.data.net_forces_w.shape == (N, 2, 3)  # the force views work too
    env.close()


def test_quadruped_timers_equal_the_restatement_step_by_step():
    env = _quadruped()
    assert env._contact_timers.num_bodies == 4
    totals, timers = _lock_step(env, 12, 40, 3.0)
    assert totals.min() >= 1, "the run missed a first contact, a first detach or a reset of live timers"
    assert env.sensor.data.current_contact_time.shape == (N, 4)
    assert np.array_equal(env.sensor.data.last_air_time.cpu().numpy(), timers[1].T)
    env.reset()
    assert not bool(env._contact_timers.timers.any()) and not bool(env._contact_timers.timestamp.any())
    env.close()


def test_a_non_default_threshold_reaches_the_kernel():
    """At 200 N a standing foot is mostly not in contact: the restatement with the cfg's threshold still matches,
    and the timers differ from the default threshold's."""
    hi, lo = _walker(threshold=200.0), _walker()
    totals, timers = _lock_step(hi, 21, 12, 1.0)
    lo.reset()
    for act in _actions(N, 21, 12):
        lo.step(act)
    assert not torch.equal(hi._contact_timers.timers, lo._contact_timers.timers)
    hi.close(), lo.close()


# ------------------------------------------------------------------ 4. graph replay

def test_captured_step_replays_with_the_timers_on():
    envs = []
    for graph in (False, True):
        e = _walker()
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(N, 21, 21)
    static = acts[0].clone()
    ge.step(static)  # warm-up, eager
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    moved = 0
    for k in range(1, 21):  # 20 replays against 20 eager steps
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        ge.account_steps(1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        a, b = eager._contact_timers, ge._contact_timers
        assert torch.equal(_bits(a.timers), _bits(b.timers)) and torch.equal(_bits(a.timestamp), _bits(b.timestamp)), k
        for key in ("q", "qd", "root_pos"):
            assert torch.equal(_bits(eager.state[key]), _bits(ge.state[key])), (k, key)
        moved += int((b.timers[2] > 0).sum())
    assert moved > 0 and bool(ge._contact_timers.timestamp.any())
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 5. reset paths

def test_reset_zeroes_everything_and_a_masked_reset_exactly_the_masked_envs():
    env = _walker()
    env.reset()
    for act in _actions(N, 21, 6):
        env.step(act)
    tm = env._contact_timers
    before_t, before_ts = tm.timers.clone(), tm.timestamp.clone()
    live = (before_ts != 0).cpu().numpy()
    assert live.sum() > N // 2
    mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    mask[[0, 5, 63, 64, 255, 256, N - 1]] = True
    mask[64:128:3] = True
    env._reset_idx(mask)
    m = mask.cpu().numpy()
    assert not tm.timers[:, :, mask].any() and not tm.timestamp[mask].any()
    assert torch.equal(_bits(tm.timers[:, :, ~mask]), _bits(before_t[:, :, ~mask]))
    assert torch.equal(_bits(tm.timestamp[~mask]), _bits(before_ts[~mask])) and (live & ~m).sum() > 0
    ids = torch.tensor([7, 300 - 2], device=DEV)
    env._reset_idx(ids)
    assert not tm.timers[:, :, ids].any() and not tm.timestamp[ids].any() and bool(tm.timestamp.any())
    env.step(_actions(N, 21, 1, seed=9)[0])
    env._reset_idx(None)
    assert not tm.timers.any() and not tm.timestamp.any()
    env.step(_actions(N, 21, 1, seed=10)[0])
    assert bool(tm.timestamp.any())
    env.reset()
    assert not tm.timers.any() and not tm.timestamp.any()
    env.close()


# ------------------------------------------------------------------ 6. state round trip, shards

def _rollout(env, acts):
    out = []
    for a in acts:
        o, r, t, u, _ = env.step(a)
        tm = env._contact_timers
        out.append((o["policy"].clone(), r.clone(), t.clone(), u.clone(), tm.timestamp.clone(), tm.timers.clone()))
    return out


def test_state_round_trip_into_a_fresh_env():
    acts = _actions(N, 21, 20)
    env = _walker()
    env.reset()
    _rollout(env, acts[:10])
    st = env.get_state()
    assert st["contact_timers"].shape == (4, 2, N) and st["contact_timestamp"].shape == (N,)
    assert bool(st["contact_timers"].any())
    first = _rollout(env, acts[10:])
    fresh = _walker()
    fresh.reset()
    fresh.set_state(st)
    second = _rollout(fresh, acts[10:])
    for k, (x, y) in enumerate(zip(first, second)):
        for p, q in zip(x, y):
            same = torch.equal(_bits(p), _bits(q)) if p.dtype == torch.float32 else torch.equal(p, q)
            assert same, k
    env.close(), fresh.close()


def test_shards_match_the_unsharded_run():
    """n = 300 whole equals shards 166 + 134 with env_id_offset: the timers draw nothing, a pure layout check."""
    h = 166
    acts = _actions(N, 21, 20)
    envs = []
    for m, off in ((N, 0), (h, 0), (N - h, h)):
        envs.append(_walker(m, offset=off))
        envs[-1].reset()
    full = _rollout(envs[0], acts)
    parts = [_rollout(envs[1], [a[:h].contiguous() for a in acts]),
             _rollout(envs[2], [a[h:].contiguous() for a in acts])]
    for k in range(len(acts)):
        for j in range(6):
            got = torch.cat([parts[0][k][j], parts[1][k][j]], dim=-1 if j == 5 else 0)
            assert torch.equal(got, full[k][j]), (k, j)
    assert bool(full[-1][5].any())
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 7. nothing else moves

def test_the_feature_changes_no_output_and_the_default_env_has_no_timers():
    on, off = _walker(air=True), _walker(air=False)
    assert off._contact_timers is None and off._report is None
    assert off.sensor.data.current_air_time is None
    with pytest.raises(RuntimeError, match="not configured to track contact time"):
        off.sensor.compute_first_contact(off.step_dt)
    oa, ob = on.reset()[0]["policy"], off.reset()[0]["policy"]
    assert torch.equal(_bits(oa), _bits(ob))
    for k, act in enumerate(_actions(N, 21, 30)):
        (o1, r1, t1, u1, _), (o0, r0, t0, u0, _) = on.step(act), off.step(act)
        assert torch.equal(_bits(o1["policy"]), _bits(o0["policy"])) and torch.equal(_bits(r1), _bits(r0)), k
        assert torch.equal(t1, t0) and torch.equal(u1, u0), k
        s1, s0 = on.get_state(), off.get_state()
        assert set(s1) - set(s0) == {"contact_timers", "contact_timestamp"}
        for key in s0:
            assert torch.equal(s1[key].view(torch.int32), s0[key].view(torch.int32)), (k, key)
    on.close(), off.close()
    quad = _quadruped(8, air=False)
    assert quad._contact_timers is None and quad._report is None and quad.sensor.data.last_contact_time is None
    quad.close()


# ------------------------------------------------------------------ 8. refusals

def test_refusals(orc):
    from _models import GpuPhysics

    from allsteps_isaaclab_amd import _native

    n = 4
    gpu = GpuPhysics(orc.m, n)
    nat, L = gpu.native, gpu.native.L
    table = _table([5, 9])
    timers = torch.zeros(4, 2, n, device=DEV)
    ts = torch.zeros(n, device=DEV)
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)

    def refused(rc, word):
        msg = L.as_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    def call(tbl=table, t=timers, s=ts, thr=1.0, updates=0, r=None, r2=None):
        p = _native._ptr
        return L.as_contact_timers(nat.h, C.byref(tbl) if tbl is not None else None, p(t), p(s), thr, updates, p(r),
                                   p(r2), None)

    refused(call(), "no contact report")
    count = torch.zeros(DEPTH, n, dtype=torch.int32, device=DEV)
    records = torch.zeros(DEPTH, _native.REPORT_WORDS, _native.MAXC, n, dtype=torch.int32, device=DEV)
    nat.set_contact_report(DEPTH, count, records, torch.zeros(21, n, device=DEV))
    for updates in (1, 3, 5, -1):
        refused(call(updates=updates), "neither 0 nor")
    refused(call(t=None), "null argument")
    refused(call(s=None), "null argument")
    refused(call(tbl=None), "null argument")
    refused(call(r2=mask), "reset2 without reset")
    refused(call(thr=float("nan")), "force_threshold")
    refused(call(tbl=_table([5, 40])), "link out of range")
    refused(call(tbl=_table([])), "num_bodies")
    with pytest.raises(_native.NativeError, match="neither 0 nor"):
        nat.contact_timers(table, timers, ts, 1.0, 2)
    timers.fill_(3.0), ts.fill_(2.0)
    torch.cuda.synchronize()
    assert call(updates=DEPTH) == 0 and call(updates=0, r=mask * 0) == 0  # no reset mask: no reset; an empty mask
    torch.cuda.synchronize()
    assert bool((ts > 2.0).all()) and bool((timers[0] > 3.0).all()) and not bool(timers[2].any())
    assert call(updates=0) == 0  # reset-only without a mask: every env
    torch.cuda.synchronize()
    assert not bool(timers.any()) and not bool(ts.any())
    nat.set_contact_report()
    refused(call(), "no contact report")
    gpu.close()
