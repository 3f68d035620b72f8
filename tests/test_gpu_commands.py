"""The command manager on the device (csrc/command_kernels.h, envs/commands.py, envs/direct_rl_env.py).

Kernel level: the fixture of the reference's own command terms (tests/golden/commands.npz) through k_commands_step /
k_commands_reset with injected draws, with guard words behind every buffer: bit-equal to the host header's float32
restatement (_commands_cases.host_step with the oracle's as_atan2f, which tests/test_commands_host.py holds equal to
the header bit for bit), atan2 included, and so equal to the reference -- bit for bit in everything that is not
downstream of atan2, within the measured heading tolerance in the rest; the Philox path against the same restatement
fed the oracle's or_philox_block uniforms, bitwise.  Env level: an env with commands in lock-step with a clean env,
the command state against a host replay, determinism, re-seeding, shards, state round trip, HIP-graph replay and the
manager's reset / generated_commands."""

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
BLOCK = 256  # kCommandThreads: one thread per env
INT_GUARD, BYTE_GUARD = 0x5A5A5A5A, 0xA5
KEYS = ("vel", "heading_target", "flags", "time_left", "counter", "metrics", "last_metrics")


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _guarded(a, guard=float("nan")):
    """(buffer, view): the array on the device with 64 guard words behind it."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a).to(DEV)
    buf = torch.empty(a.size + 64, dtype=t.dtype, device=DEV)
    buf[a.size:] = guard
    buf[: a.size] = t.reshape(-1)
    return buf, buf[: a.size].view(a.shape)


def _guard_ok(buf, size, guard):
    tail = buf[size:]
    return bool(torch.isnan(tail).all()) if isinstance(guard, float) else bool((tail == guard).all())


def _rows(a, n):
    """The first n envs of an env-minor array; past the fixture's 66 the rows repeat (an env's step depends on
    its own row only)."""
    return np.ascontiguousarray(np.take(a, np.arange(n) % a.shape[-1], axis=-1))


class _Buffers:
    """The kernels' state buffers on the device, guarded."""

    GUARDS = {"flags": BYTE_GUARD, "counter": INT_GUARD, "t": INT_GUARD}

    def __init__(self, state: dict, n: int, t0: int):
        self.n = n
        arrays = {k: _rows(np.asarray(state[k]), n) for k in KEYS}
        arrays["flags"] = arrays["flags"].astype(np.uint8)
        arrays["counter"] = arrays["counter"].astype(np.int32)
        arrays["t"] = np.full(n, t0, np.int32)
        self.buf, self.view = {}, {}
        for k, a in arrays.items():
            self.buf[k], self.view[k] = _guarded(a, self.GUARDS.get(k, float("nan")))

    def args(self, last=True):
        v = self.view
        return (v["vel"], v["heading_target"], v["flags"], v["time_left"], v["counter"], v["metrics"],
                v["last_metrics"] if last else None, v["t"])

    def guards_ok(self):
        return all(_guard_ok(self.buf[k], self.view[k].numel(), self.GUARDS.get(k, float("nan"))) for k in self.buf)

    def equals(self, want: dict, where=""):
        for k in KEYS:
            got = self.view[k].cpu().numpy()
            w = _rows(np.asarray(want[k]), self.n).astype(got.dtype)
            same = np.array_equal(got.view(np.uint8), w.view(np.uint8))
            assert same, (where, k, np.argwhere(got.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[:4])


# ------------------------------------------------------------------ 1. the fixture, injected draws

@pytest.fixture(scope="module")
def cases(orc):
    """The fixture's cases, each with ``host``: the header's restatement of every step (computed once, at the
    fixture's 66 envs) and ``host0``: of the reset-only launch from the zero state."""
    from _commands_cases import STATE, host_step, load_cases, oracle_atan2

    atan2 = oracle_atan2(orc)
    out = load_cases()
    for c in out:
        zero = {k: np.zeros_like(c[k + "0"]) for k in STATE}
        zero["last_metrics"] = np.zeros_like(zero["metrics"])
        c["host0"], _ = host_step(c["rows"], c["dt"], zero, atan2, reset=np.ones(66, bool), draws=c["init_draws"][None],
                                  compute=False)
        st = {k: c[k + "0"].copy() for k in STATE}
        st["last_metrics"] = np.zeros_like(st["metrics"])
        c["start"], c["host"] = st, []
        for s in range(c["steps"]):
            st, _ = host_step(c["rows"], c["dt"], st, atan2, (c["root_quat"][s], c["root_lin"][s], c["root_ang"][s]),
                              c["reset"][s], c["draws"][s])
            c["host"].append(st)
    return out


def _against_the_reference(c, s, got: dict, n: int):
    """Rule 3: bit for bit with the reference's fixture but for the heading envs' yaw command and error_vel_yaw of a
    term with heading_command, which hold within the measured tolerance (a heading error of the reference within the
    tolerance of the wrap's ends is compared only when it is bit-equal)."""
    from _commands_cases import ERR_YAW_TOL, HEADING_TOL, heading_rows, row_fields

    ref = {k: _rows(c[k][s], n) for k in KEYS}
    for k in ("heading_target", "flags", "time_left", "counter"):
        assert np.array_equal(got[k].astype(ref[k].dtype).view(np.uint8), ref[k].view(np.uint8)), (c["name"], s, k)
    for ti, heading in enumerate(heading_rows(c)):
        f = row_fields(c["rows"][ti])
        soft = np.zeros((3, n), bool)
        if heading:
            soft[2] = (ref["flags"][ti, 0] != 0) & (ref["flags"][ti, 1] == 0)
        exact = ~soft
        assert np.array_equal(got["vel"][ti][exact].view(np.uint32), ref["vel"][ti][exact].view(np.uint32)), (c["name"], s)
        if heading:
            stiff = abs(float(f["stiffness"]))
            g, w = got["vel"][ti][2][soft[2]].astype(np.float64), ref["vel"][ti][2][soft[2]].astype(np.float64)
            edge = np.abs(np.abs(w) / stiff - np.pi) <= HEADING_TOL
            same = g.astype(np.float32).view(np.uint32) == w.astype(np.float32).view(np.uint32)
            ok = (np.abs(g - w) <= stiff * HEADING_TOL) | same
            assert (ok | (edge & same)).all() and (same | ~edge).all(), (c["name"], s, float(np.abs(g - w).max()))
        for key in ("metrics", "last_metrics"):
            assert np.array_equal(got[key][ti][0].view(np.uint32), ref[key][ti][0].view(np.uint32)), (c["name"], s, key)
            g, w = got[key][ti][1], ref[key][ti][1]
            if heading:
                fin = np.isfinite(w)
                assert np.array_equal(g[~fin].view(np.uint32), w[~fin].view(np.uint32))
                assert (np.abs(g[fin].astype(np.float64) - w[fin]) <= ERR_YAW_TOL).all(), (c["name"], s, key)
            else:
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (c["name"], s, key)


@pytest.mark.parametrize("n", [1, 3, 66, BLOCK + 1])
def test_kernels_reproduce_the_fixture_from_injected_draws(cases, n):
    """Every fixture case on the first n rows (BLOCK + 1: a second workgroup of one thread): the reset-only launch
    from the zero state, then every step through k_commands_step; every buffer and t bit-equal to the header's
    restatement and equal to the reference under the heading rule, guard words intact."""
    from allsteps_isaaclab_amd import _native

    for c in cases:
        desc = torch.from_numpy(c["rows"].copy()).to(DEV)
        if c["name"] != "c":  # (case c starts from hand-set timers)
            zero = {k: np.zeros_like(v) for k, v in c["host0"].items()}
            b0 = _Buffers(zero, n, 5)
            _native.commands_reset(desc, *b0.args(), draws=torch.from_numpy(_rows(c["init_draws"], n)).to(DEV),
                                   stream=_stream())
            torch.cuda.synchronize()
            b0.equals(c["host0"], (c["name"], "reset-only"))
            b0.equals({**{k: c[k + "0"] for k in KEYS if k != "last_metrics"}, "last_metrics": zero["last_metrics"]},
                      (c["name"], "reset-only against the reference"))
            assert torch.equal(b0.view["t"], torch.full_like(b0.view["t"], 6)) and b0.guards_ok()
        b = _Buffers(c["start"], n, 7)
        for s in range(c["steps"]):
            root = [torch.from_numpy(_rows(c[k][s], n)).to(DEV) for k in ("root_quat", "root_lin", "root_ang")]
            reset = torch.from_numpy(_rows(c["reset"][s], n)).to(DEV)
            # the two masks are ORed: split the step's mask over them
            r1, r2 = reset.clone(), reset.clone()
            r1[1::2] = 0
            r2[0::2] = 0
            _native.commands_step(desc, *root, *b.args(), float(c["dt"]), reset=r1, reset2=r2,
                                  draws=torch.from_numpy(_rows(c["draws"][s], n)).to(DEV), stream=_stream())
            torch.cuda.synchronize()
            b.equals(c["host"][s], (c["name"], s))
            _against_the_reference(c, s, {k: b.view[k].cpu().numpy() for k in KEYS}, n)
            assert torch.equal(b.view["t"], torch.full_like(b.view["t"], 8 + s)), (c["name"], s)
        assert b.guards_ok(), c["name"]


def test_null_optional_pointers_are_not_written_and_masks_select(cases):
    """last_metrics = NULL: the launch runs and leaves everything else as with it; reset masks NULL: no env resets;
    the reset-only launch with a mask touches the masked envs only (and advances t of every env)."""
    from allsteps_isaaclab_amd import _native

    c, n = cases[0], 66
    desc = torch.from_numpy(c["rows"].copy()).to(DEV)
    b = _Buffers(c["start"], n, 0)
    for s in range(6):
        root = [torch.from_numpy(c[k][s].copy()).to(DEV) for k in ("root_quat", "root_lin", "root_ang")]
        reset = torch.from_numpy(c["reset"][s].copy()).to(DEV)
        _native.commands_step(desc, *root, *b.args(last=False), float(c["dt"]), reset=reset if reset.any() else None,
                              draws=torch.from_numpy(c["draws"][s].copy()).to(DEV), stream=_stream())
    torch.cuda.synchronize()
    assert c["reset"][:6].any()
    b.equals({**c["host"][5], "last_metrics": c["start"]["last_metrics"]}, "last_metrics = NULL")
    before = {k: b.view[k].clone() for k in b.view}
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[[0, 7, 65]] = 1
    _native.commands_reset(desc, *b.args(), mask=mask, draws=torch.from_numpy(c["init_draws"].copy()).to(DEV),
                           stream=_stream())
    torch.cuda.synchronize()
    keep = (mask == 0)
    for k in KEYS:
        assert torch.equal(_bits(b.view[k][..., keep]), _bits(before[k][..., keep])), k
    assert bool((b.view["counter"][:, ~keep] == 1).all()) and bool((b.view["metrics"][..., ~keep] == 0).all())
    assert torch.equal(_bits(b.view["last_metrics"][..., ~keep]), _bits(before["metrics"][..., ~keep]))
    assert torch.equal(b.view["t"], before["t"] + 1) and b.guards_ok()


# ------------------------------------------------------------------ 2. the Philox path

SEED, ENV0 = 0x1234_5678_9ABC_DEF1, 1000


def _philox(orc):
    fn = orc.L.or_philox_block
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    buf = (C.c_float * 4)()

    def block(seed, env, t, b, tag):
        fn(seed & 0xFFFFFFFFFFFFFFFF, env & 0xFFFFFFFF, int(t) & 0xFFFFFFFF, b, tag, buf)
        return buf[:]

    return block


def _philox_draws(orc, rows, seed, env0, t, phases=(0, 1)):
    """(len(phases), terms, 11, n): the draws of csrc/allsteps_commands.h from the oracle's uniforms -- term k owns
    blocks 3k .. 3k + 2 of the phase's tag at counter t[e]; a uniform term consumes u0 .. u6; of a normal term the
    uniform draws only are formed here (u0 -> d0, u5 .. u11 -> d4 .. d10; its three normals stay 0)."""
    from _commands_cases import row_fields

    from allsteps_isaaclab_amd import _native

    block = _philox(orc)
    K, n = rows.shape[0], len(t)
    d = np.zeros((len(phases), K, 11, n), np.float32)
    for pi, phase in enumerate(phases):
        for k in range(K):
            normal = row_fields(rows[k])["kind"] == 1
            for e in range(n):
                u = sum((block(seed, env0 + e, t[e], 3 * k + b, _native.COMMAND_TAGS[phase]) for b in range(3)), [])
                if normal:
                    d[pi, k, 0, e] = u[0]
                    d[pi, k, 4:, e] = u[5:12]
                else:
                    d[pi, k, :7, e] = u[:7]
    return d


def _terms(step_dt, normal=True):
    from _commands_cases import term_cfg

    from allsteps_isaaclab_amd.envs.commands import CommandTerms

    terms = {"heading": term_cfg({"kind": "uniform", "resampling_time_range": [0.0, 0.09], "heading_command": True,
                                  "heading_control_stiffness": 0.7, "rel_heading_envs": 0.6, "rel_standing_envs": 0.15,
                                  "ranges": {"lin_vel_x": [-1.1, 1.3], "lin_vel_y": [-0.7, 0.9],
                                             "ang_vel_z": [-0.8, 0.9], "heading": [-3.1, 3.1]}}),
             "plain": term_cfg({"kind": "uniform", "resampling_time_range": [0.01, 0.05], "rel_standing_envs": 0.3,
                                "ranges": {"lin_vel_x": [0.1, 0.3], "lin_vel_y": [-0.07, 0.07],
                                           "ang_vel_z": [-0.9, -0.6]}})}
    if normal:
        terms["normal"] = term_cfg({"kind": "normal", "resampling_time_range": [0.0, 0.04], "rel_standing_envs": 0.2,
                                    "ranges": {"mean_vel": [0.5, 0.1, -0.3], "std_vel": [0.4, 0.25, 0.6],
                                               "zero_prob": [0.2, 0.3, 0.1]}})
    return terms, CommandTerms(terms, step_dt)


@pytest.mark.parametrize("n", [1, 3, 66, BLOCK + 1])
def test_philox_path_equals_the_host_restatement(orc, n):
    """A reset of every env, then six steps of three terms from the Philox streams (64-bit seed, env_id_offset
    1000) with resets in some: every buffer of the two uniform terms, and the timers, counters and masks of the normal
    term (its commands need the device's Box-Muller), equal the float32 numpy restatement on the oracle's uniforms,
    bitwise."""
    from _commands_cases import STATE, host_step, oracle_atan2

    from allsteps_isaaclab_amd import _native

    dt = np.float32(1 / 60)
    _, terms = _terms(1 / 60)
    K = 3
    atan2 = oracle_atan2(orc)
    desc = torch.from_numpy(terms.rows.copy()).to(DEV)
    rng = np.random.default_rng(n)
    shapes = {"vel": (K, 3, n), "heading_target": (K, n), "flags": (K, 5, n), "time_left": (K, n), "counter": (K, n),
              "metrics": (K, 2, n), "last_metrics": (K, 2, n)}
    st = {k: np.zeros(s, np.int32 if k == "counter" else np.uint8 if k == "flags" else np.float32)
          for k, s in shapes.items()}
    b = _Buffers(st, n, 0)
    _native.commands_reset(desc, *b.args(), seed=SEED, env_offset=ENV0, stream=_stream())
    st, _ = host_step(terms.rows, dt, st, atan2, reset=np.ones(n, bool),
                      draws=_philox_draws(orc, terms.rows, SEED, ENV0, np.zeros(n, np.int64), phases=(0,)), compute=False)

    def check(where):
        got = {k: b.view[k].cpu().numpy() for k in KEYS}
        for k in KEYS:
            w = st[k].astype(got[k].dtype)
            terms_cmp = slice(0, 2) if k in ("vel", "metrics", "last_metrics") else slice(0, 3)
            assert np.array_equal(got[k][terms_cmp].view(np.uint8), w[terms_cmp].view(np.uint8)), (where, k)
        return got

    torch.cuda.synchronize()
    check("reset")
    resamples = np.zeros(2, np.int64)
    for s in range(6):
        q = rng.normal(0, 1, (4, n))
        root = [(q / np.linalg.norm(q, axis=0)).astype(np.float32), rng.normal(0, 0.7, (3, n)).astype(np.float32),
                rng.normal(0, 0.9, (3, n)).astype(np.float32)]
        reset = rng.random(n) < (0.3 if s % 2 else 0.0)
        if s == 1:
            reset[0] = True
        tt = np.full(n, 1 + s, np.int64)
        st, rs = host_step(terms.rows, dt, st, atan2, root, reset, _philox_draws(orc, terms.rows, SEED, ENV0, tt))
        # the normal term's commands are the device's: take them over, so that its metrics do not enter the comparison
        _native.commands_step(desc, *(torch.from_numpy(x).to(DEV) for x in root), *b.args(), float(dt),
                              reset=torch.from_numpy(reset).to(DEV), seed=SEED, env_offset=ENV0, stream=_stream())
        torch.cuda.synchronize()
        got = check(s)
        for k in ("vel", "metrics", "last_metrics"):
            st[k][2] = got[k][2]
        assert torch.equal(b.view["t"], torch.full_like(b.view["t"], 2 + s)), s
        resamples += rs.sum(axis=(1, 2))
    assert resamples[0] >= 1 and resamples[1] >= 2 * n, "the test hardly saw a resample"
    assert b.guards_ok()


# ------------------------------------------------------------------ 3. the envs

def _walker(n, commands=None, seed=42, offset=0):
    from allsteps_isaaclab_amd.envs.allsteps_env import AllstepsEnv
    from allsteps_isaaclab_amd.envs.allsteps_env_cfg import AllstepsEnvCfg

    cfg = AllstepsEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.commands = commands
    return AllstepsEnv(cfg, env_id_offset=offset)


def _quadruped(n, commands=None, seed=42, offset=0):
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env_cfg import AnymalCStonesEnvCfg

    assert offset == 0
    cfg = AnymalCStonesEnvCfg()
    cfg.scene.num_envs = n
    cfg.sim.device = DEV
    cfg.seed = seed
    cfg.commands = commands
    return AnymalCStonesEnv(cfg)


def _actions(n, cols, steps, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.rand(n, cols, device=DEV, generator=g) * 2 - 1 for _ in range(steps)]


def _commands():
    """Two uniform terms with short resampling times (an env step is 1/60 s or 1/50 s)."""
    return _terms(1 / 60, normal=False)[0]


def _command_state(env):
    c = env._commands
    return {"vel": c.vel, "heading_target": c.heading_target, "flags": c.flags, "time_left": c.time_left,
            "counter": c.counter, "metrics": c.metrics, "last_metrics": c.last_metrics}


@pytest.mark.parametrize("make,cols", [(_walker, 21), (_quadruped, 12)], ids=["walker", "quadruped"])
def test_env_equals_a_clean_env_and_its_commands_follow_a_host_replay(orc, make, cols):
    """Env A has two command terms, env B none, both fed the same actions: observations, rewards, dones and state
    are bit-identical at every step -- the feature changes no existing behaviour.  A's command state equals a host
    replay (float32 numpy on the oracle's Philox uniforms) that reads A's root state after the step, the step's
    done masks and command_t before it, bitwise; the run is long enough that the step resets envs."""
    from _commands_cases import host_step, oracle_atan2

    n, steps = 66, 160
    a, b = make(n, _commands()), make(n)
    assert a._commands is not None and b._commands is None
    oa, ob = a.reset()[0]["policy"], b.reset()[0]["policy"]
    assert torch.equal(_bits(oa), _bits(ob))
    c = a._commands
    rows, dt, atan2 = c.terms.rows, np.float32(a.step_dt), oracle_atan2(orc)
    assert float(dt) == c.dt
    zero = {k: np.zeros_like(v.cpu().numpy()) for k, v in _command_state(a).items()}
    st, _ = host_step(rows, dt, zero, atan2, reset=np.ones(n, bool),
                      draws=_philox_draws(orc, rows, c.seed, 0, np.zeros(n, np.int64), phases=(0,)), compute=False)

    def check(where):
        for k, v in _command_state(a).items():
            got = v.cpu().numpy()
            assert np.array_equal(got.view(np.uint8), st[k].astype(got.dtype).view(np.uint8)), (where, k)

    check("reset")
    assert torch.equal(c.t, torch.ones(n, dtype=torch.int32, device=DEV))
    resets = resamples = doubles = 0
    for k, act in enumerate(_actions(n, cols, steps)):
        t_before = c.t.cpu().numpy()
        (oa, ra, ta, ua, _), (ob, rb, tb, ub, _) = a.step(act), b.step(act)
        assert torch.equal(_bits(oa["policy"]), _bits(ob["policy"])), k
        assert torch.equal(_bits(ra), _bits(rb)) and torch.equal(ta, tb) and torch.equal(ua, ub), k
        for key in b.state:
            assert torch.equal(_bits(a.state[key]), _bits(b.state[key])), (k, key)
        done = (ta | ua).cpu().numpy().astype(bool)
        root = [a.state[key].cpu().numpy() for key in ("root_quat", "root_lin", "root_ang")]
        st, rs = host_step(rows, dt, st, atan2, root, done, _philox_draws(orc, rows, c.seed, 0, t_before))
        check(k)
        resets += int(done.sum())
        resamples += int(rs.sum())
        doubles += int((rs[0] & rs[1]).sum())
    print(f"resets {resets}, resamples {resamples}, double resamples {doubles}")
    assert resets >= 1, "no env was reset by a step: the test did not see the reset phase"
    assert resamples >= 4 * n
    assert not a.extras.get("log"), "the in-step resets write nothing into extras"
    assert torch.equal(c.t, torch.full((n,), 1 + steps, dtype=torch.int32, device=DEV))
    assert set(b.get_state()) | set(c.STATE_KEYS) == set(a.get_state())
    a.close(), b.close()


def _rollout(env, acts):
    out = []
    for a in acts:
        o, r, t, u, _ = env.step(a)
        out.append((o["policy"].clone(), r.clone(), t.clone(), u.clone(),
                    *(v.clone() for v in _command_state(env).values())))
    return out


def _same(a, b):
    return len(a) == len(b) and all(all(torch.equal(_bits(p), _bits(q)) for p, q in zip(x, y)) for x, y in zip(a, b))


def test_env_commands_are_deterministic_and_seeded():
    """Equal seeds give equal commands, another seed others; reset(seed=) re-keys the stream: the commands after it
    are those of an env built with that seed whose stream counter stands where this one's does."""
    n = 66
    acts = _actions(n, 21, 20)
    runs, first = [], []
    for seed in (42, 42, 43):
        env = _walker(n, _commands(), seed=seed)
        env.reset()
        first.append(env._commands.vel.clone())
        runs.append(_rollout(env, acts))
        env.close()
    assert _same(runs[0], runs[1]) and torch.equal(first[0], first[1])
    assert not torch.equal(first[0], first[2])
    env = _walker(n, _commands(), seed=42)
    env.reset()
    t = env._commands.t.clone()
    env.reset(seed=43)
    assert env._commands.seed == 43 and torch.equal(env._commands.t, t + 1)
    assert not torch.equal(env._commands.vel, first[0])
    env.close()


def test_env_command_shards_match_unsharded():
    """n = 130 whole equals shards 66 + 64 with env_id_offset: the global env id enters the Philox key."""
    n, h = 130, 66
    acts = _actions(n, 21, 20)
    envs = []
    for m, off in ((n, 0), (h, 0), (n - h, h)):
        envs.append(_walker(m, _commands(), offset=off))
        envs[-1].reset()
    full = _rollout(envs[0], acts)
    parts = [_rollout(envs[1], [a[:h] for a in acts]), _rollout(envs[2], [a[h:] for a in acts])]
    for k in range(len(acts)):
        for j in range(len(full[k])):
            got = torch.cat([parts[0][k][j], parts[1][k][j]], dim=0 if j < 4 else -1)
            assert torch.equal(_bits(got), _bits(full[k][j])), (k, j)
    sf = envs[0].get_state()
    for key in ("command_t", "command_time_left", "command_vel_b", "root_lin"):
        got = torch.cat([envs[1].get_state()[key], envs[2].get_state()[key]], dim=-1)
        assert torch.equal(_bits(got), _bits(sf[key])), key
    for e in envs:
        e.close()


def test_env_state_round_trip_repeats_the_commands():
    n = 66
    env = _walker(n, _commands())
    env.reset()
    acts = _actions(n, 21, 30)
    _rollout(env, acts[:10])
    st = env.get_state()
    assert set(env._commands.STATE_KEYS) <= set(st)
    assert st["command_t"].shape == (n,) and st["command_vel_b"].shape == (2, 3, n)
    first = _rollout(env, acts[10:])
    env.set_state(st)
    assert _same(first, _rollout(env, acts[10:]))
    env.close()


def test_a_clean_env_has_no_command_state():
    for make in (_walker, _quadruped):
        clean = make(4)
        assert clean._commands is None and not hasattr(clean, "command_manager")
        assert not any(k.startswith("command") for k in clean.get_state())
        clean.close()


def test_env_step_with_commands_replays_from_a_graph():
    """A step captured under torch.cuda.graph replays with fresh draws: replays equal the eager steps of a twin env
    bitwise, the commands differ from replay to replay, and a range edit made after the capture (refresh) holds in
    the replays that follow."""
    n = 66

    def commands():
        t = _commands()
        t["plain"].resampling_time_range = (0.0, 0.01)  # below one step: every env resamples in every step
        return t

    envs = []
    for graph in (False, True):
        e = _walker(n, commands())
        assert e.graph_safe_step
        e.set_graph_capture(graph)
        e.reset()
        envs.append(e)
    eager, ge = envs
    acts = _actions(n, 21, 7)
    static = acts[0].clone()
    ge.step(static)  # warm-up, eager
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ge.step(static)
    eager.step(acts[0])
    seen = []
    for k in range(1, 6):
        if k == 4:
            for e in envs:
                e.command_manager.get_term_cfg("plain").ranges.lin_vel_x = (5.0, 6.0)
                e.command_manager.refresh()
        o1, r1, t1, u1, _ = eager.step(acts[k])
        static.copy_(acts[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(o1["policy"]), _bits(out[0]["policy"])) and torch.equal(_bits(r1), _bits(out[1])), k
        assert torch.equal(t1, out[2]) and torch.equal(u1, out[3]), k
        for (key, x), y in zip(_command_state(eager).items(), _command_state(ge).values()):
            assert torch.equal(_bits(x), _bits(y)), (k, key)
        vx = ge.command_manager.get_command("plain")[:, 0]
        moving = ~ge.command_manager.get_term("plain").is_standing_env
        assert bool(((vx[moving] >= 5.0) & (vx[moving] <= 6.0)).all()) == (k >= 4), k
        seen.append(ge._commands.vel.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert torch.equal(ge._commands.t, eager._commands.t)
    for e in envs:
        e.close()


def test_manager_reset_returns_the_means_and_generated_commands_is_the_storage():
    from allsteps_isaaclab_amd.utils.commands import generated_commands

    n = 66
    env = _walker(n, _commands())
    env.reset()
    for act in _actions(n, 21, 8):
        env.step(act)
    m = env.command_manager
    assert m.active_terms == ["heading", "plain"]
    cmd = generated_commands(env, "heading")
    assert cmd.shape == (n, 3) and cmd.data_ptr() == m.get_command("heading").data_ptr() == env._commands.vel[0].data_ptr()
    ids = [3, 5, 64]
    term = m.get_term("plain")
    want = {f"Metrics/{name}/{k}": torch.mean(v[ids]).item() for name in m.active_terms
            for k, v in m.get_term(name).metrics.items()}
    before, t = env._commands.metrics.clone(), env._commands.t.clone()
    counter = term.command_counter.clone()
    extras = m.reset(ids)
    assert extras == want and all(v > 0 for v in extras.values())
    assert bool((env._commands.metrics[..., ids] == 0).all()) and bool((term.command_counter[ids] == 1).all())
    rest = [e for e in range(n) if e not in ids]
    assert torch.equal(env._commands.metrics[..., rest], before[..., rest])
    assert torch.equal(term.command_counter[rest], counter[rest])
    assert torch.equal(term.last_episode_metrics["error_vel_xy"][ids], before[1, 0, ids])
    assert torch.equal(env._commands.t, t + 1)
    # compute(dt): one more launch on the state as it stands, no reset
    m.compute(env.step_dt)
    assert torch.equal(env._commands.t, t + 2) and bool((env._commands.metrics[:, 0, ids] > 0).all())
    assert sorted(m.reset()) == sorted(want)
    assert bool((env._commands.counter == 1).all())
    env.close()
