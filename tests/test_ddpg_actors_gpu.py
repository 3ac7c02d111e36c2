"""The device Pendulum actors (rth_ddpg_actor_step, reth_amd/ddpg_actors.VecDdpgActors) on the GPU:
one env step against the host class envs.Pendulum, the reset against the documented Philox draw,
acting against rth_ddpg_act and the host restatement of the OU noise on the documented normal
draws, the rows, determinism, graph replay, position independence / the grid-stride loop, buffer
bounds and the argument checks.

Bounds: the device's fp64 dynamics against the host's within 1e-12 (absolute where |x| <= 1,
relative otherwise); an f32 derived from two fp64 values that close is the same float or a
neighbouring one."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678
STREAM_PENDULUM, STREAM_OU = 11, 12
PI = math.pi
M = 2e-6  # how far the constructed cases sit from their boundary, at least
H1, H2 = 400, 300
EPSILON = "1,0.01,30000"
THETA, SIGMA = 0.15, 0.2
NAMES = ["state", "ep_steps", "t_dev", "stats", "ret_stats", "noise", "cur_obs", "act_det", "row_s0", "row_a", "row_r",
         "row_s1", "row_done"]


@pytest.fixture(scope="module")
def solver():
    from reth_amd.ddpg import DDPGSolver
    from reth_amd.solver import Box

    torch.manual_seed(3)
    s = DDPGSolver(Box(-1.0, 1.0, (3,)), Box(-2.0, 2.0, (1,)), device="cuda", impl="hip", cast_actions_to_long=False)
    assert s.impl_active == "hip" and s.actor.dims() == (3, 1, H1, H2)
    return s


def _actors(n, **kw):
    from reth_amd.ddpg_actors import VecDdpgActors

    kw.setdefault("seed", SEED)
    return VecDdpgActors("Pendulum-v0", n, device="cuda", **kw)


def _key(seed):
    return [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]


def _reset_state(orc, seed, i, t):
    """the documented reset draw (csrc/ddpg_actor.hpp): one Philox block per (seed, env, t)"""
    c = orc.philox4x32([i, t & 0xFFFFFFFF, t >> 32, STREAM_PENDULUM], _key(seed)).astype(np.float64)
    return np.array([-PI + (2.0 * PI * c[0]) / 2.0 ** 32, -1.0 + (2.0 * c[1]) / 2.0 ** 32, 0.0, 0.0])


def _normal(orc, seed, i, t, a=0):
    """the documented standard normal draw of (seed, env i, step t, component a)"""
    b, j = a // 4, (a % 4) // 2
    c = orc.philox4x32([i, t & 0xFFFFFFFF, t >> 32, STREAM_OU | (b << 16)], _key(seed)).astype(np.float64)
    u1, u2 = (c[2 * j] + 0.5) / 2.0 ** 32, c[2 * j + 1] / 2.0 ** 32
    r, ang = math.sqrt(-2.0 * math.log(u1)), 2.0 * PI * u2
    return r * (math.sin(ang) if a % 2 else math.cos(ang))


def _host_obs(s):
    return np.array([math.cos(s[0]), math.sin(s[0]), s[1]])


def _host_step(state, steps, action, max_steps):
    """envs.Pendulum from (state, step count): next state, observation, reward, done"""
    from reth_amd.envs import Pendulum

    h = Pendulum(max_steps)
    h.state, h._t = (float(state[0]), float(state[1])), int(steps)
    o, r, d, _ = h.step(np.asarray(action, np.float32))
    return np.array(h.state), o, r, d


def _err(got, want):
    """|got - want|, absolute where |want| <= 1, relative otherwise"""
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def _adjacent(got, want32):
    """f32 arrays equal or neighbouring floats"""
    return (np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32))).all()


def _raw(th, thdot, a):
    """theta_dot' before its clip, the way the host computes it"""
    u = min(max(float(np.float32(a)), -2.0), 2.0)
    return thdot + (-3.0 * 10.0 / (2.0 * 1.0) * math.sin(th + PI) + 3.0 / (1.0 * 1.0 ** 2) * u) * 0.05


def _margin(th, thdot, a):
    """the distance of a step from every decision it takes: the torque clip, the speed clip, the
    modulo's wrap"""
    m = (th + PI) % (2.0 * PI)
    return min(abs(abs(float(np.float32(a))) - 2.0), abs(abs(_raw(th, thdot, a)) - 8.0), m, 2.0 * PI - m)


def _cases(rng, n, max_steps):
    th, thdot = rng.uniform(-3.0, 3.0, n), rng.uniform(-6.5, 6.5, n)
    a = rng.uniform(-1.9, 1.9, n).astype(np.float32)
    steps = rng.integers(0, max_steps - 2, n)
    kind = np.array(["interior"] * n, dtype=object)
    k = 16
    for sign in (1.0, -1.0):
        # theta_dot' past +-8 by a wide and by a narrow margin, and just inside: theta' takes the unclipped value
        for off, tag in ((0.55, "speed-out"), (1.5 * M, "speed-out"), (-1.5 * M, "speed-in")):
            th[k], a[k] = sign * PI / 2, sign * 1.5
            thdot[k] = sign * (8.0 + off) - (_raw(th[k], 0.0, a[k]))
            kind[k] = tag
            k += 1
        # |action| > 2 by a wide and by a narrow margin, and just inside
        for v, tag in ((2.75, "torque-out"), (2.0 + 1.5 * M, "torque-out"), (2.0 - 1.5 * M, "torque-in")):
            a[k], kind[k] = sign * v, tag
            k += 1
        # theta outside [-pi, pi): the modulo's sign branch (theta + pi < 0) and its plain one
        for v in (3.5, 4.0, 10.0, PI + 1.5 * M, PI - 1.5 * M):
            th[k], kind[k] = sign * v, "wrap-neg" if sign * v + PI < 0 else "wrap"
            k += 1
    for v in (-PI, PI, -3 * PI):  # theta + pi an exact multiple of 2 pi: the modulo is exactly 0
        th[k], kind[k] = v, "exact"
        k += 1
    for j in range(k, k + 6):  # the time limit on interior states
        steps[j], kind[j] = max_steps - 1, "limit"
    assert k + 6 <= n
    margin = np.array([_margin(th[i], thdot[i], a[i]) for i in range(n)])
    return np.stack([th, thdot], 1), a, steps, kind, margin


# ---------------------------------------------------------------------------- dynamics
def test_env_step_matches_host(solver, capsys):
    """N = 64: interior states, every clip and the modulo's wrap approached from both sides with a
    margin of at least 2e-6, theta + pi an exact multiple of 2 pi, and the time limit"""
    from oracle import oracle as orc

    N, MAX, MU = 64, 200, 0.125
    rng = np.random.default_rng(5)
    st, a, steps, kind, margin = _cases(rng, N, MAX)
    x0 = rng.uniform(-0.5, 0.5, (N, 1))
    exp_s, exp_o, exp_r, exp_done = np.zeros((N, 4)), np.empty((N, 3)), np.empty(N), np.empty(N, bool)
    for i in range(N):
        exp_s[i, :2], exp_o[i], exp_r[i], exp_done[i] = _host_step(st[i], steps[i], [a[i]], MAX)
    # the constructed cases sit at least 2e-6 from every decision; theta + pi = 2 pi k exactly is the exception
    exact = kind == "exact"
    edge = ~np.isin(kind, ["interior", "limit", "exact"])
    assert edge.sum() == 22 and exact.sum() == 3 and (kind == "wrap-neg").sum() >= 3
    assert (margin[~exact] >= 1e-9).all() and (margin[edge] >= M).all()
    assert all((st[i, 0] + PI) % (2 * PI) == 0.0 for i in np.nonzero(exact)[0])
    assert (np.abs(exp_s[kind == "speed-out", 1]) == 8.0).all() and (np.abs(exp_s[kind == "speed-in", 1]) < 8.0).all()
    for i in np.nonzero(kind == "speed-out")[0]:  # theta' from the unclipped theta_dot'
        assert exp_s[i, 0] == st[i, 0] + _raw(st[i, 0], st[i, 1], a[i]) * 0.05 != st[i, 0] + exp_s[i, 1] * 0.05
    assert exp_done[kind == "limit"].all() and not exp_done[kind != "limit"].any()

    act = _actors(N, max_episode_steps=MAX, mu=MU)
    act.set_state(st, steps, noise=x0)
    obs0 = act.current_obs().cpu().numpy()
    want0 = np.stack([_host_obs(s) for s in st]).astype(np.float32)
    assert obs0.shape == (N, 3) and _adjacent(obs0, want0)
    a_dev = torch.as_tensor(a, device="cuda").reshape(N, 1)
    act.step(solver, a_dev)
    assert act.launches == 1 and act.pushes == 1
    s0, ra, rr, s1, rd = (t.cpu().numpy() for t in act.rows())
    done = rd != 0
    np.testing.assert_array_equal(done, exp_done)
    assert ra.tobytes() == a.reshape(N, 1).tobytes() and s0.tobytes() == obs0.tobytes()
    state, cur = act.state.cpu().numpy(), act.cur_obs.cpu().numpy()
    live = ~done
    err = _err(state[live, :2], exp_s[live, :2])
    with capsys.disabled():
        print(f"\n[ddpg_actors] Pendulum env-step max |device - host| / max(1, |host|) over {live.sum()} running "
              f"rows: {err.max():.3e}")
    assert err.max() <= 1e-12
    assert (state[:, 2:] == 0).all()  # the columns the env does not use
    assert _adjacent(rr, exp_r.astype(np.float32))
    assert _adjacent(s1, exp_o.astype(np.float32))  # the terminal observation of a finished episode
    assert cur[live, :3].tobytes() == s1[live].tobytes() and (cur[:, 3] == 0).all()
    # the noise advanced on the documented draw; a finished episode has it back at mu
    noise = act.noise.cpu().numpy()
    z = np.array([_normal(orc, SEED, i, 1) for i in range(N)])
    want_x = x0[:, 0] + (THETA * (MU - x0[:, 0]) + SIGMA * z)
    assert _err(noise[live, 0], want_x[live]).max() <= 1e-12
    assert (noise[done] == MU).all()
    # finished episodes: the documented Philox draw at t = 1 and its observation in cur_obs
    for i in np.nonzero(done)[0]:
        want_s = _reset_state(orc, SEED, int(i), 1)
        assert np.abs(state[i] - want_s).max() <= 1e-15
        assert _adjacent(cur[i, :3], _host_obs(want_s).astype(np.float32))
    # step counts, episode and return statistics
    np.testing.assert_array_equal(act.ep_steps.cpu().numpy(), np.where(done, 0, steps + 1))
    ep, tot, last = (t.cpu().numpy() for t in act.episode_stats())
    np.testing.assert_array_equal(ep, done.astype(np.int64))
    np.testing.assert_array_equal(tot, np.where(done, steps + 1, 0))
    np.testing.assert_array_equal(last, np.where(done, steps + 1, 0))
    run, rsum, rlast = (t.cpu().numpy() for t in act.return_stats())
    assert run.dtype == np.float64
    assert _err(run, np.where(done, 0.0, exp_r)).max() <= 1e-12
    assert _err(rsum, np.where(done, exp_r, 0.0)).max() <= 1e-12 and rsum.tobytes() == rlast.tobytes()
    assert (run[done] == 0).all() and (rsum[live] == 0).all()
    np.testing.assert_array_equal(act.t_dev.cpu().numpy(), np.ones(N, np.int64))


# ---------------------------------------------------------------------------- reset
@pytest.mark.parametrize("N", [1, 9, 64])
def test_initial_reset_is_the_documented_draw(N):
    from oracle import oracle as orc

    act = _actors(N, mu=0.25)
    state = act.state.cpu().numpy()
    want = np.stack([_reset_state(orc, SEED, i, 0) for i in range(N)])
    assert np.abs(state - want).max() <= 1e-15
    assert (want[:, 0] >= -PI).all() and (want[:, 0] < PI).all() and (np.abs(want[:, 1]) <= 1).all()
    cur = act.cur_obs.cpu().numpy()
    assert cur.shape == (N, 4) and (cur[:, 3] == 0).all()
    assert _adjacent(cur[:, :3], np.stack([_host_obs(s) for s in state]).astype(np.float32))
    assert int(act.t_dev.abs().sum()) == 0 and int(act.ep_steps.abs().sum()) == 0 and int(act.stats.abs().sum()) == 0
    assert float(act.ret_stats.abs().sum()) == 0.0 and (act.noise.cpu().numpy() == 0.25).all()
    assert act.max_episode_steps == 200 and act.pushes == 0


# ---------------------------------------------------------------------------- acting
def _eps(t):
    from reth_amd.schedule import Schedule

    return Schedule.from_str(EPSILON).value(t)


@pytest.mark.parametrize("N", [1, 9, 64])
@pytest.mark.parametrize("t0", [0, 29_999, 1_000_000])
def test_acting_matches_ddpg_act_and_the_host_noise(solver, N, t0):
    """three steps from t_dev = t0: t = 1.. (the schedule's start), t = 30,000.. (its last step and
    the clamp) and far beyond"""
    from oracle import oracle as orc

    assert _eps(1) == 1.0 + (0.01 - 1.0) * 1 / 30000 and _eps(30_000) == _eps(10 ** 7) and abs(_eps(30_000) - 0.01) < 1e-15
    z_max = math.sqrt(-2.0 * math.log(0.5 / 2.0 ** 32))  # the largest |z| the mapping yields
    act = _actors(N, epsilon=EPSILON)
    act.t_dev.fill_(t0)
    for t in range(t0 + 1, t0 + 4):
        obs = act.current_obs()
        det_ref = solver.act_batch(obs)
        x = act.noise.cpu().numpy().copy()
        act.step(solver)
        assert torch.equal(act.act_det, det_ref)  # bit-equal to rth_ddpg_act on the same observations
        z = np.array([[_normal(orc, SEED, i, t)] for i in range(N)])
        want_x = x + (THETA * (0.0 - x) + SIGMA * z)
        got_x = act.noise.cpu().numpy()
        assert _err(got_x, want_x).max() <= 1e-12
        det = det_ref.cpu().numpy()
        want_a = (det.astype(np.float64) + _eps(t) * want_x).astype(np.float32)
        got_a = act.row_a.cpu().numpy()
        assert _adjacent(got_a, want_a)
        # the noise is in, at the scale's size: from 0, |x| <= 3 sigma z_max after three steps
        assert (got_a != det).any() and np.abs(got_a - det).max() <= _eps(t) * 3 * SIGMA * z_max + 1e-6
    np.testing.assert_array_equal(act.t_dev.cpu().numpy(), np.full(N, t0 + 3))


def test_normal_draws_first_two_moments():
    """a sanity check of the documented mapping on the host restatement (not of the device):
    4,096 (env, t) pairs"""
    from oracle import oracle as orc

    z = np.array([_normal(orc, SEED, i, t) for i in range(64) for t in range(1, 65)])
    assert abs(z.mean()) < 0.1 and abs(z.var() - 1.0) < 0.15
    # the sine branch and a second block belong to the same family
    z2 = np.array([_normal(orc, SEED, i, 1, a) for i in range(512) for a in (1, 4, 7)])
    assert abs(z2.mean()) < 0.1 and abs(z2.var() - 1.0) < 0.15


# ---------------------------------------------------------------------------- rows
@pytest.mark.parametrize("N", [1, 9, 64])
def test_rows_match_a_host_pendulum(solver, N):
    """7 steps with injected actions and a time limit of 3: every row against envs.Pendulum driven
    with the same states and actions; s0 of a step is cur_obs of the step before, bit for bit"""
    MAX, K = 3, 7
    rng = np.random.default_rng(12)
    act = _actors(N, max_episode_steps=MAX)
    act.set_state(np.stack([rng.uniform(-3, 3, N), rng.uniform(-6, 6, N)], 1))
    dones = 0
    for k in range(K):
        state, steps = act.state.cpu().numpy(), act.ep_steps.cpu().numpy()
        cur = act.cur_obs.cpu().numpy()
        a = rng.uniform(-2.5, 2.5, (N, 1)).astype(np.float32)
        act.step(solver, torch.as_tensor(a, device="cuda"))
        s0, ra, rr, s1, rd = (t.cpu().numpy() for t in act.rows())
        assert s0.tobytes() == cur[:, :3].tobytes() and ra.tobytes() == a.tobytes()
        new = act.state.cpu().numpy()
        for i in range(N):
            want_s, want_o, want_r, want_d = _host_step(state[i], steps[i], a[i], MAX)
            assert rd[i] == float(want_d) and want_d == (steps[i] == MAX - 1)
            assert _adjacent(rr[i:i + 1], np.float32([want_r])) and _adjacent(s1[i], want_o.astype(np.float32))
            if not want_d:
                assert _err(new[i, :2], want_s).max() <= 1e-12
        dones += int(rd.sum())
    assert dones == N * (K // MAX)
    ep, tot, last = (t.cpu().numpy() for t in act.episode_stats())
    assert (ep == K // MAX).all() and (tot == MAX * (K // MAX)).all() and (last == MAX).all()


# ---------------------------------------------------------------------------- determinism, graph, position
def _snapshot(act):
    return {k: getattr(act, k).clone() for k in NAMES}


def _same(a, b):
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("N", [1, 9, 64])
def test_deterministic_and_graph_replay_equals_eager(solver, N):
    T = 20
    runs = []
    for _ in range(2):
        act = _actors(N, max_episode_steps=7)
        for _ in range(T):
            act.step(solver)
        runs.append(_snapshot(act))
    _same(runs[0], runs[1])
    assert int(runs[0]["stats"][:, 0].sum()) == N * (T // 7)
    act = _actors(N, max_episode_steps=7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records one step; nothing runs
        act.step(solver)
    assert int(act.t_dev.sum()) == 0
    for _ in range(T):
        g.replay()
    torch.cuda.synchronize()
    _same(runs[0], _snapshot(act))


def test_position_independence_grid_stride_and_single_env(solver):
    """envs 0..8 of N = 8 * 1024 + 9 (1026 tiles > the 1024-workgroup grid: the grid-stride loop)
    equal an N = 9 run after 3 steps, with the same states and noise injected by index; N = 1
    equals env 0"""
    NB = 8 * 1024 + 9
    rng = np.random.default_rng(9)
    st = np.stack([rng.uniform(-3, 3, NB), rng.uniform(-6, 6, NB)], 1)
    x0 = rng.uniform(-0.3, 0.3, (NB, 1))
    sets = [(_actors(n, max_episode_steps=2), n) for n in (NB, 9, 1)]
    for act, n in sets:
        act.set_state(st[:n], noise=x0[:n])
    for t in range(3):
        for act, _ in sets:
            act.step(solver)
        for k in NAMES:
            b, s, o = (getattr(act, k).cpu().numpy() for act, _ in sets)
            assert b[:9].tobytes() == s.tobytes(), (t, k)
            assert s[:1].tobytes() == o.tobytes(), (t, k)
    big = sets[0][0]
    # the tiles reached through the stride stepped too
    assert (big.t_dev.cpu().numpy() == 3).all() and (big.stats[:, 0].cpu().numpy() == 1).all()
    assert (big.row_done.cpu().numpy() == 0).all() and (big.ep_steps.cpu().numpy() == 1).all()


def test_no_write_outside_any_buffer(solver):
    from reth_amd.ddpg_actors import VecDdpgActors

    G = 64

    class Guarded(VecDdpgActors):
        def _alloc(self, shape, dtype):
            n = int(np.prod(shape))
            canary = 12345.5 if dtype.is_floating_point else 0x5A5A5A5A
            buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
            buf[G:G + n] = 0
            self.__dict__.setdefault("_guarded", []).append((buf, n, canary))
            return buf[G:G + n].view(shape)

    act = Guarded("Pendulum-v0", 9, max_episode_steps=2, seed=SEED, device="cuda")
    act.reset()
    for _ in range(5):
        act.step(solver)
    torch.cuda.synchronize()
    assert len(act._guarded) == len(NAMES) == 13  # every device buffer of the actor set
    assert (act.t_dev.cpu().numpy() == 5).all() and int(act.stats[:, 0].sum()) == 9 * 2
    for buf, n, canary in act._guarded:
        assert (buf[:G] == canary).all() and (buf[G + n:] == canary).all(), (buf.dtype, n)


# ---------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_before_any_launch(solver):
    from reth_amd import _lib

    ERR_INVALID = -1
    act = _actors(9)
    act.step(solver)
    torch.cuda.synchronize()
    before = _snapshot(act)
    lib, s = _lib.lib(), _lib.stream_ptr()

    def args(**kw):
        a = act._args(act._params(solver), None, act._dims)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    null_params = (_lib.c_vp * 6)(*([act._params_key[0]] * 5 + [None]))
    bad = [dict(env=7), dict(env=-1), dict(D=4), dict(Ad=2), dict(H1=402), dict(H2=516), dict(H1=0), dict(N=0),
           dict(N=-3), dict(N=1 << 31), dict(max_episode_steps=0), dict(eps_steps=0),
           dict(cur_obs=act.cur_obs.data_ptr() + 4), dict(actor=null_params),
           dict(actor=_lib.ctypes.POINTER(_lib.c_vp)())]
    bad += [{k: None} for k in ("state", "ep_steps", "t_dev", "stats", "ret_stats", "noise", "cur_obs", "row_s0", "row_a",
                                "row_r", "row_s1", "row_done")]
    for kw in bad:
        a = args(**kw)
        assert lib.rth_ddpg_actor_step(_lib.ctypes.byref(a), s) == ERR_INVALID, kw
        assert b"rth_ddpg_actor_step" in lib.rth_last_error(), kw
    for kw in (dict(env=7), dict(D=4), dict(H2=516), dict(N=0), dict(max_episode_steps=0), dict(state=None),
               dict(noise=None), dict(cur_obs=act.cur_obs.data_ptr() + 4)):
        a = args(**kw)
        assert lib.rth_ddpg_env_reset(_lib.ctypes.byref(a), s) == ERR_INVALID, kw
        assert b"rth_ddpg_env_reset" in lib.rth_last_error(), kw
    assert lib.rth_ddpg_actor_step(None, s) == ERR_INVALID and lib.rth_ddpg_env_reset(None, s) == ERR_INVALID
    with pytest.raises(_lib.RethHipError):
        _lib.call("rth_ddpg_actor_step", _lib.ctypes.byref(args(N=0)), s)
    with pytest.raises(ValueError, match="action_in"):
        act.step(solver, torch.zeros(9, 1, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    # nothing was launched: the device's own step counter and everything else stand as they were
    assert act.launches == 1 and (act.t_dev.cpu().numpy() == 1).all()
    _same(before, _snapshot(act))
    act.step(solver)  # and the good arguments still step
    assert (act.t_dev.cpu().numpy() == 2).all() and act.launches == 2
