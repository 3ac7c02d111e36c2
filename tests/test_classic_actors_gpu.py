"""The device classic-control actors (rth_env_actor_step, reth_amd/mlp_actors.VecMlpActors) on the
GPU: one env step of Acrobot and MountainCar against the host classes of reth_amd/envs.py, the
generic entry point against rth_mlp_actor_step on CartPole, acting against rth_mlp_q + the oracle's
ε-greedy on the documented Philox draws, the n-step rows against the oracle's NStepAdder,
determinism, graph replay, position independence / the grid-stride loop, and buffer bounds."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678
STREAM_EXPLORE, STREAM_RANDACT = 2, 3
PI = math.pi
ENVS = ["Acrobot-v1", "MountainCar-v0"]
# obs_dim, actions, ring row stride, the reset draw's Philox stream, state columns in use, TimeLimit
SPEC = {"Acrobot-v1": dict(D=6, A=3, LD=8, stream=9, K=4, limit=500),
        "MountainCar-v0": dict(D=2, A=3, LD=4, stream=10, K=2, limit=200)}
M = 2e-6  # how far the constructed cases sit from their boundary


def _net(env, seed=0):
    from reth_amd import model

    torch.manual_seed(seed)
    net = model.MLP_DQNNetwork((SPEC[env]["D"],), SPEC[env]["A"]).to("cuda")
    net.requires_grad_(False)
    return net


def _actors(env, n, **kw):
    from reth_amd.mlp_actors import VecMlpActors

    kw.setdefault("seed", SEED)
    return VecMlpActors(env, n, device="cuda", **kw)


def _mlp_q(net, obs):
    from reth_amd import _lib

    obs = obs.contiguous()
    D, _, A = net.dims()
    q = torch.empty((obs.shape[0], A), dtype=torch.float32, device=obs.device)
    arr = (_lib.c_vp * 6)(*[p.data_ptr() for p in net._params6()])
    _lib.call("rth_mlp_q", arr, obs.data_ptr(), D, obs.shape[0], D, 128, A, q.data_ptr(), None, _lib.stream_ptr())
    return q


def _key(seed):
    return [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]


def _reset_state(orc, env, seed, i, t):
    """the documented reset draw (csrc/env_actor.hpp): one Philox block per (seed, env, t)"""
    c = orc.philox4x32([i, t & 0xFFFFFFFF, t >> 32, SPEC[env]["stream"]], _key(seed)).astype(np.float64)
    if env == "Acrobot-v1":
        return -0.1 + (0.2 * c) / 2.0 ** 32
    return np.array([-0.6 + (0.2 * c[0]) / 2.0 ** 32, 0.0, 0.0, 0.0])


def _host_obs(env, s):
    if env == "Acrobot-v1":
        return np.array([math.cos(s[0]), math.sin(s[0]), math.cos(s[1]), math.sin(s[1]), s[2], s[3]])
    return np.array([s[0], s[1]])


def _host_env(env, max_steps):
    from reth_amd.envs import Acrobot, MountainCar

    return (Acrobot if env == "Acrobot-v1" else MountainCar)(max_steps)


# ---------------------------------------------------------------------------- the step's raw quantities on the host
def _acrobot_raw(s, a):
    """the RK4 step of envs.Acrobot before the wrap and the clamps"""
    from reth_amd.envs import Acrobot

    env = Acrobot()
    y0, tau, dt = tuple(float(v) for v in s), float(a - 1), env.dt
    k1 = env._dsdt(y0, tau)
    k2 = env._dsdt(tuple(y0[j] + dt / 2.0 * k1[j] for j in range(4)), tau)
    k3 = env._dsdt(tuple(y0[j] + dt / 2.0 * k2[j] for j in range(4)), tau)
    k4 = env._dsdt(tuple(y0[j] + dt * k3[j] for j in range(4)), tau)
    return [y0[j] + dt / 6.0 * (k1[j] + 2.0 * k2[j] + 2.0 * k3[j] + k4[j]) for j in range(4)]


def _wrap(x):
    while x > PI:
        x -= 2.0 * PI
    while x < -PI:
        x += 2.0 * PI
    return x


def _acrobot_height(s, a):
    y = _acrobot_raw(s, a)
    t1, t2 = _wrap(y[0]), _wrap(y[1])
    return -math.cos(t1) - math.cos(t2 + t1)


def _acrobot_margin(s, a):
    """the distance of a step from every decision it takes: the wrap edges, the velocity bounds,
    the height-1 line"""
    y = _acrobot_raw(s, a)
    d = [abs(abs(y[j]) - k * PI) for j in (0, 1) for k in (1, 3)]
    d += [abs(abs(y[2]) - 4 * PI), abs(abs(y[3]) - 9 * PI), abs(_acrobot_height(s, a) - 1.0)]
    return min(d)


def _mc_raw(s, a):
    """v before its clamp, p before its clamp, and the state after the step (the issue's formula)"""
    p, v = float(s[0]), float(s[1])
    v_raw = v + ((a - 1) * 0.001 + math.cos(3 * p) * (-0.0025))
    v = min(max(v_raw, -0.07), 0.07)
    p_raw = p + v
    p = min(max(p_raw, -1.2), 0.6)
    if p == -1.2 and v < 0:
        v = 0.0
    return v_raw, p_raw, p, v


def _mc_margin(s, a):
    v_raw, p_raw, p, v = _mc_raw(s, a)
    d = [abs(abs(v_raw) - 0.07), abs(p_raw + 1.2), abs(p_raw - 0.6), abs(p - 0.5)]
    if p >= 0.5 - 1e-3:
        d.append(abs(v))  # the goal's second condition v >= 0 (v = 0 exactly sits on it only behind the wall)
    return min(d)


def _solve(f, x, target):
    """x with f(x) = target, by the secant method from x (f smooth and monotonic near x)"""
    x0, x1 = x, x + 1e-3
    f0, f1 = f(x0) - target, f(x1) - target
    for _ in range(60):
        if abs(f1) < 1e-9:
            return x1
        x0, x1, f0 = x1, x1 - f1 * (x1 - x0) / (f1 - f0), f1
        f1 = f(x1) - target
    raise AssertionError("no convergence")


def _acrobot_cases(rng, n, max_steps):
    st = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-2, 2, n), rng.uniform(-3, 3, n)], axis=1)
    a = rng.integers(0, 3, n)
    steps = rng.integers(0, max_steps - 2, n)
    kind = np.array(["interior"] * n, dtype=object)
    k = 20
    for sign in (1.0, -1.0):
        for off, tag in ((M, "out"), (-M, "in")):  # beyond / inside each boundary by 2e-6
            # the height-1 line: -2 cos(th1) = 1 at th1 = 2 pi / 3, swinging up
            a[k] = 1
            th = _solve(lambda x: _acrobot_height((sign * x, 0.0, sign * 0.5, 0.0), 1), 2.0, 1.0 + off)
            st[k], kind[k] = (sign * th, 0.0, sign * 0.5, 0.0), "height-" + tag
            # both velocity bounds
            a[k + 1] = 1
            w = _solve(lambda x: sign * _acrobot_raw((0.0, 0.0, sign * x, 0.0), 1)[2], 13.3, 4 * PI + off)
            st[k + 1], kind[k + 1] = (0.0, 0.0, sign * w, 0.0), "w1-" + tag
            a[k + 2] = 1
            w = _solve(lambda x: sign * _acrobot_raw((0.0, 0.0, 0.0, sign * x), 1)[3], 28.26, 9 * PI + off)
            st[k + 2], kind[k + 2] = (0.0, 0.0, 0.0, sign * w), "w2-" + tag
            # both wrap edges, for either angle
            a[k + 3] = 1
            th = _solve(lambda x: sign * _acrobot_raw((sign * x, 0.3, sign * 2.0, 0.0), 1)[0], 2.8, PI + off)
            st[k + 3], kind[k + 3] = (sign * th, 0.3, sign * 2.0, 0.0), "wrap1-" + tag
            a[k + 4] = 1
            th = _solve(lambda x: sign * _acrobot_raw((0.2, sign * x, 0.0, sign * 3.0), 1)[1], 2.6, PI + off)
            st[k + 4], kind[k + 4] = (0.2, sign * th, 0.0, sign * 3.0), "wrap2-" + tag
            k += 5
    for j in range(k, k + 6):  # the time limit on interior states
        steps[j], kind[j] = max_steps - 1, "limit"
    margin = np.array([_acrobot_margin(st[i], int(a[i])) for i in range(n)])
    return st, a, steps, kind, margin


def _mc_cases(rng, n, max_steps):
    st = np.stack([rng.uniform(-0.9, 0.3, n), rng.uniform(-0.05, 0.05, n)], axis=1)
    a = rng.integers(0, 3, n)
    steps = rng.integers(0, max_steps - 2, n)
    kind = np.array(["interior"] * n, dtype=object)
    k = 20
    for off, tag in ((M, "out"), (-M, "in")):
        # the goal p >= 0.5, moving right; and v >= 0 beyond it
        a[k] = 2
        p = _solve(lambda x: _mc_raw((x, 0.03), 2)[2], 0.47, 0.5 + off)
        st[k], kind[k] = (p, 0.03), "goal-" + tag
        a[k + 1] = 0
        v = _solve(lambda x: _mc_raw((0.55, x), 0)[3], 0.001, off)
        st[k + 1], kind[k + 1] = (0.55, v), "goalv-" + tag
        # the left wall: p_raw below -1.2 is clamped and v zeroed; the right end of the track
        a[k + 2] = 0
        p = _solve(lambda x: _mc_raw((x, -0.03), 0)[1], -1.17, -1.2 - off)
        st[k + 2], kind[k + 2] = (p, -0.03), "wall-" + tag
        a[k + 3] = 2
        p = _solve(lambda x: _mc_raw((x, 0.03), 2)[1], 0.57, 0.6 + off)
        st[k + 3], kind[k + 3] = (p, 0.03), "end-" + tag
        # the speed limit, both signs
        for j, sign in ((4, 1.0), (5, -1.0)):
            a[k + j] = 1 + int(sign)
            v = _solve(lambda x: sign * _mc_raw((-0.5, sign * x), 1 + int(sign))[0], 0.069, 0.07 + off)
            st[k + j], kind[k + j] = (-0.5, sign * v), "speed-" + tag
        k += 6
    for j in range(k, k + 6):
        steps[j], kind[j] = max_steps - 1, "limit"
    margin = np.array([_mc_margin(st[i], int(a[i])) for i in range(n)])
    return st, a, steps, kind, margin


@pytest.mark.parametrize("env", ENVS)
def test_env_step_matches_host(env, capsys):
    """N = 67 (eight full tiles and a partial one): interior states, every terminal / clamp / wrap
    boundary approached from both sides with a 2e-6 margin, and the time limit"""
    from oracle import oracle as orc

    sp = SPEC[env]
    N, MAX, D, K = 67, sp["limit"], sp["D"], sp["K"]
    rng = np.random.default_rng(5)
    st, a, steps, kind, margin = (_acrobot_cases if env == "Acrobot-v1" else _mc_cases)(rng, N, MAX)
    exp_s, exp_o, exp_r, exp_done = np.zeros((N, 4)), np.empty((N, D)), np.empty(N, np.float32), np.empty(N, bool)
    for i in range(N):
        h = _host_env(env, MAX)
        h.state, h._t = tuple(st[i]), int(steps[i])
        o, r, d, _ = h.step(int(a[i]))
        exp_s[i, :K], exp_o[i], exp_r[i], exp_done[i] = h.state, o, r, d
    # no case sits within 1e-9 of a decision or a wrap edge on the host; the constructed ones are 1e-6..3e-6 off
    assert margin.min() >= 1e-9
    edge = ~np.isin(kind, ["interior", "limit"])
    assert edge.sum() == (20 if env == "Acrobot-v1" else 12)
    assert (margin[edge] >= 1e-6).all() and (margin[edge] <= 3e-6).all()
    assert exp_done[kind == "limit"].all() and (exp_r[kind == "limit"] == -1.0).all()
    if env == "Acrobot-v1":
        assert exp_done[kind == "height-out"].all() and (exp_r[kind == "height-out"] == 0.0).all()
        assert not exp_done[kind == "height-in"].any() and (exp_r[kind == "height-in"] == -1.0).all()
        for tag, col, bound in (("w1", 2, 4 * PI), ("w2", 3, 9 * PI)):
            assert (np.abs(exp_s[kind == tag + "-out", col]) == bound).all()
            assert (np.abs(exp_s[kind == tag + "-in", col]) < bound).all()
        for tag, col in (("wrap1", 0), ("wrap2", 1)):  # wrapped: the far side; not wrapped: just inside
            assert (np.abs(exp_s[kind == tag + "-out", col]) < PI).all()
            assert (np.sign(exp_s[kind == tag + "-out", col]) != np.sign(st[kind == tag + "-out", col])).all()
            assert (np.sign(exp_s[kind == tag + "-in", col]) == np.sign(st[kind == tag + "-in", col])).all()
    else:
        assert (exp_r == -1.0).all()
        assert exp_done[np.isin(kind, ["goal-out", "goalv-out", "end-out", "end-in"])].all()
        assert not exp_done[np.isin(kind, ["goal-in", "goalv-in", "wall-in", "wall-out", "speed-in", "speed-out"])].any()
        assert (exp_s[kind == "wall-out", 0] == -1.2).all() and (exp_s[kind == "wall-out", 1] == 0.0).all()
        assert (exp_s[kind == "wall-in", 0] > -1.2).all() and (exp_s[kind == "wall-in", 1] < 0.0).all()
        assert (np.abs(exp_s[kind == "speed-out", 1]) == 0.07).all() and (np.abs(exp_s[kind == "speed-in", 1]) < 0.07).all()
        assert (exp_s[kind == "end-out", 0] == 0.6).all() and (exp_s[kind == "end-in", 0] < 0.6).all()
    assert not exp_done[kind == "interior"].any()

    net = _net(env)
    act = _actors(env, N, n_step=1, max_episode_steps=MAX)
    assert act.obs_dim == D and act.num_actions == sp["A"] and act.obs_ring.shape == (N * act.ring + 1, sp["LD"])
    act.set_state(st, steps)
    obs0 = act.current_obs().cpu().numpy()
    want0 = np.stack([_host_obs(env, s) for s in np.pad(st, ((0, 0), (0, 4 - K)))]).astype(np.float32)
    assert obs0.shape == (N, D) and (np.abs(obs0 - want0) <= np.spacing(np.abs(want0))).all()
    a_dev = torch.as_tensor(a, dtype=torch.int64, device="cuda")
    assert act.step(net, a_dev) is False  # n = 1: the first push emits nothing
    assert int(act.emit.sum()) == 0
    done = act.done.cpu().numpy() != 0
    np.testing.assert_array_equal(done, exp_done)
    np.testing.assert_array_equal(act.reward.cpu().numpy(), exp_r)
    np.testing.assert_array_equal(act.action.cpu().numpy(), a)
    state = act.state.cpu().numpy()
    ring = act.obs_ring.cpu().numpy()
    s0_h, s1_h = act.s0_h.cpu().numpy(), act.s1_h.cpu().numpy()
    cur = (act._base + act.cur_slot).cpu().numpy()
    np.testing.assert_array_equal(ring[s0_h][:, :D], obs0)
    # running episodes: the fp64 state against the host's, 1e-12 * max(1, |v|)
    live = ~done
    assert live.sum() >= 30 and done.sum() >= 8
    err = np.abs(state[live] - exp_s[live]) / np.maximum(1.0, np.abs(exp_s[live]))
    with capsys.disabled():
        print(f"\n[classic_actors] {env} env-step max |device - host| / max(1, |host|) over {live.sum()} running rows: "
              f"{err.max():.3e}")
    assert err.max() <= 1e-12
    assert (state[:, K:] == 0).all()  # the columns the env does not use
    # the observation of the step (the terminal one of a finished episode): within one f32 spacing of float32(host obs)
    got, want = ring[s1_h][:, :D], exp_o.astype(np.float32)
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
    np.testing.assert_array_equal(cur[live], s1_h[live])
    # finished episodes: the documented Philox draw at t = 1, and its observation in the reset slot
    assert (cur[done] != s1_h[done]).all() and (cur[done] // act.ring == np.arange(N)[done]).all()
    for i in np.nonzero(done)[0]:
        want_s = _reset_state(orc, env, SEED, int(i), 1)
        np.testing.assert_array_equal(state[i], want_s)
        want_o = _host_obs(env, want_s).astype(np.float32)
        assert (np.abs(ring[cur[i], :D] - want_o) <= np.spacing(np.abs(want_o))).all()
        if env == "Acrobot-v1":
            assert (want_s >= -0.1).all() and (want_s < 0.1).all()
        else:
            assert -0.6 <= want_s[0] < -0.4
    assert (ring[:, D:] == 0).all()  # the pad floats of every row
    np.testing.assert_array_equal(ring[N * act.ring], np.zeros(sp["LD"], np.float32))  # the sink row stays zero
    # step counts, episode and return statistics
    np.testing.assert_array_equal(act.ep_steps.cpu().numpy(), np.where(done, 0, steps + 1))
    ep, tot, last = (t.cpu().numpy() for t in act.episode_stats())
    np.testing.assert_array_equal(ep, done.astype(np.int64))
    np.testing.assert_array_equal(tot, np.where(done, steps + 1, 0))
    np.testing.assert_array_equal(last, np.where(done, steps + 1, 0))
    run, rsum, rlast = (t.cpu().numpy() for t in act.return_stats())
    assert run.dtype == np.float64
    np.testing.assert_array_equal(run, np.where(done, 0.0, exp_r))
    np.testing.assert_array_equal(rsum, np.where(done, exp_r, 0.0))
    np.testing.assert_array_equal(rlast, np.where(done, exp_r, 0.0))
    np.testing.assert_array_equal(act.t_dev.cpu().numpy(), np.ones(N, np.int64))
    # the second step emits the first transition by value: s1 of a done row is the terminal obs
    assert act.step(net, a_dev) is True
    assert int(act.emit.sum()) == N
    s0, ra, rr, s1, rd = (t.cpu().numpy() for t in act.rows())
    assert s0.shape == (N, D) and s1.shape == (N, D)
    np.testing.assert_array_equal(s0, obs0)
    np.testing.assert_array_equal(s1, ring[s1_h][:, :D])
    np.testing.assert_array_equal(ra, a)
    np.testing.assert_array_equal(rr, exp_r)
    np.testing.assert_array_equal(rd, done.astype(np.float32))
    np.testing.assert_array_equal(act.row_s0.cpu().numpy(), s0_h)
    np.testing.assert_array_equal(act.row_s1.cpu().numpy(), s1_h)


@pytest.mark.parametrize("env", ENVS)
def test_initial_reset_is_the_documented_draw(env):
    from oracle import oracle as orc

    act = _actors(env, 5)
    state = act.state.cpu().numpy()
    for i in range(5):
        np.testing.assert_array_equal(state[i], _reset_state(orc, env, SEED, i, 0))
    want = np.stack([_host_obs(env, s) for s in state]).astype(np.float32)
    assert (np.abs(act.current_obs().cpu().numpy() - want) <= np.spacing(np.abs(want))).all()
    assert (act.cur_slot.cpu() == 1).all() and int(act.t_dev.sum()) == 0
    assert act.max_episode_steps == SPEC[env]["limit"] and float(act.ret_stats.abs().sum()) == 0.0


# ---------------------------------------------------------------------------- the generic entry point on CartPole
def test_generic_cartpole_equals_the_cartpole_actors():
    """VecMlpActors("CartPole-v0") against VecCartPoleActors: bit-identical at every one of 40
    steps that include episodes ended by either threshold and by the time limit, and their resets"""
    from reth_amd import model
    from reth_amd.mlp_actors import VecCartPoleActors

    N, T = 67, 40
    torch.manual_seed(7)
    net = model.MLP_DQNNetwork((4,), 2).to("cuda")
    net.requires_grad_(False)
    old = VecCartPoleActors(N, n_step=3, seed=SEED, device="cuda")
    new = _actors("CartPole-v0", N, n_step=3)
    assert new.max_episode_steps == old.max_episode_steps == 200 and new.ring == old.ring
    rng = np.random.default_rng(11)
    st = np.stack([rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(-0.1, 0.1, N), rng.uniform(-1, 1, N)], 1)
    st[:10, 0], st[:10, 1] = 2.39, 1.0          # leaves the track within a step
    st[10:20, 2], st[10:20, 3] = -0.2, -1.0     # falls within a step or two
    steps = rng.integers(0, 150, N)
    steps[20:26] = 197                          # the time limit within three steps
    for act in (old, new):
        act.set_state(st, steps)
    names = ["state", "ep_steps", "t_dev", "stats", "obs_ring", "cur_slot", "action", "reward", "done", "s0_h", "s1_h",
             "emit", "row_s0", "row_a", "row_s1", "row_r", "row_done", "row_obs0", "row_obs1"]
    for t in range(T):
        assert old.step(net) == new.step(net)
        for k in names:
            assert getattr(old, k).cpu().numpy().tobytes() == getattr(new, k).cpu().numpy().tobytes(), (t, k)
        assert torch.equal(old.current_obs(), new.current_obs())
        for x, y in zip(old.rows(), new.rows()):
            assert torch.equal(x, y)
    ep, tot, last = (x.cpu().numpy() for x in new.episode_stats())
    assert ep[:26].min() >= 1
    # reward 1 a step: the returns (counted from the injection, unlike the injected step counts) add up to T
    run, rsum, rlast = (x.cpu().numpy() for x in new.return_stats())
    np.testing.assert_array_equal(run + rsum, np.full(N, float(T)))
    assert (run[ep > 0] == new.ep_steps.cpu().numpy()[ep > 0]).all()
    assert (rlast[ep > 1] == last[ep > 1]).all()


# ---------------------------------------------------------------------------- acting and the adder
def _draws(orc, seed, n, t, A):
    u = np.array([orc.philox_uniform(seed, t, i, STREAM_EXPLORE) for i in range(n)])
    ra = np.array([(int(orc.philox4x32([i, t & 0xFFFFFFFF, t >> 32, STREAM_RANDACT], _key(seed))[0]) * A) >> 32
                   for i in range(n)], dtype=np.int64)
    return u, ra


@pytest.mark.parametrize("env", ENVS)
def test_acting_matches_mlp_q_and_oracle_eps_greedy(env):
    from oracle import oracle as orc

    N, A = 67, SPEC[env]["A"]
    eps = np.concatenate([np.zeros(20), np.ones(20), np.linspace(0.2, 0.8, N - 40)])
    net = _net(env, 1)
    act = _actors(env, N, eps=eps)
    q_out = act.want_q()
    explored, seen = 0, set()
    for t in (1, 2, 3):
        obs = act.current_obs()
        assert obs.shape == (N, SPEC[env]["D"])
        q_ref = _mlp_q(net, obs)
        act.step(net)
        assert torch.equal(q_out, q_ref)  # bit-equal to rth_mlp_q on the same observations
        u, ra = _draws(orc, SEED, N, t, A)
        want = orc.eps_greedy(q_ref.cpu().numpy(), eps, u, ra)
        np.testing.assert_array_equal(act.action.cpu().numpy(), want)
        explored += int((u < eps).sum())
        seen |= set(ra.tolist())
    assert 60 < explored < 3 * N - 60  # both branches ran
    assert seen == {0, 1, 2}


def _energetic(env, rng, n):
    """states from which episodes end by the env's own rule within a few steps"""
    if env == "Acrobot-v1":  # just below the height-1 line, swinging up
        sign = rng.choice([-1.0, 1.0], n)
        return np.stack([sign * rng.uniform(1.9, 2.05, n), np.zeros(n), sign * rng.uniform(0.5, 2.0, n), np.zeros(n)], 1)
    return np.stack([rng.uniform(0.40, 0.49, n), rng.uniform(0.02, 0.06, n)], 1)  # short of the goal, moving right


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("n_step,mode", [(1, 0), (3, 0), (3, 1)])
def test_nstep_rows_match_oracle(env, n_step, mode):
    from oracle import oracle as orc

    N, T, D = 20, 30, SPEC[env]["D"]
    net = _net(env, 3)
    act = _actors(env, N, n_step=n_step, gamma=0.99, max_episode_steps=6, nstep_mode=mode)
    act.set_state(_energetic(env, np.random.default_rng(2), N))
    adders = [orc.NStep(n_step, 0.99, mode) for _ in range(N)]
    trace = {}  # handle -> the observation it held when the trace last named it
    emitted = dones = zero_rewards = 0
    for t in range(T):
        act.step(net)
        ring = act.obs_ring.cpu().numpy()[:, :D]
        s0_h, a, r, s1_h, d = (x.cpu().numpy() for x in (act.s0_h, act.action, act.reward, act.s1_h, act.done))
        emit = act.emit.cpu().numpy()
        row = [x.cpu().numpy() for x in (act.row_s0, act.row_a, act.row_r, act.row_s1, act.row_done)]
        o0, o1 = act.row_obs0.cpu().numpy(), act.row_obs1.cpu().numpy()
        for i in range(N):
            trace[int(s0_h[i])], trace[int(s1_h[i])] = ring[s0_h[i]].copy(), ring[s1_h[i]].copy()
            out = adders[i].push(s0_h[i], a[i], r[i], s1_h[i], d[i])
            assert int(emit[i]) == (out is not None), (t, i)
            if out is None:
                continue
            emitted += 1
            assert (int(row[0][i]), int(row[1][i]), int(row[3][i])) == (out[0], out[1], out[3]), (t, i)
            assert row[2][i].tobytes() == np.float32(out[2]).tobytes(), (t, i)  # r: bitwise
            assert row[4][i] == out[4], (t, i)
            assert o0[i].tobytes() == trace[out[0]].tobytes() and o1[i].tobytes() == trace[out[3]].tobytes(), (t, i)
        dones += int(d.sum())
        zero_rewards += int((r == 0).sum())
        assert set(np.unique(r)) <= ({-1.0, 0.0} if env == "Acrobot-v1" else {-1.0})
        assert act.warm == (t + 1 > n_step)
    assert emitted == N * (T - n_step) and dones >= N * (T // 6)  # the time limit alone ends T / 6 episodes per env
    if env == "Acrobot-v1":
        assert zero_rewards >= 5  # terminal steps: the reward sums mix -1 and 0


# ---------------------------------------------------------------------------- determinism, graph, position
def _snapshot(act):
    names = ["state", "ep_steps", "t_dev", "stats", "ret_stats", "obs_ring", "cur_slot", "action", "reward", "done",
             "s0_h", "s1_h", "emit", "row_s0", "row_a", "row_s1", "row_r", "row_done", "row_obs0", "row_obs1"]
    return {k: getattr(act, k).clone() for k in names}


def _same(a, b):
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("env", ENVS)
def test_deterministic_and_graph_replay_equals_eager(env):
    N, T = 67, 20
    net = _net(env, 4)
    runs = []
    for _ in range(2):
        act = _actors(env, N, n_step=3, max_episode_steps=7)
        for _ in range(T):
            act.step(net)
        runs.append(_snapshot(act))
    _same(runs[0], runs[1])
    assert int(runs[0]["stats"][:, 0].sum()) >= N * (T // 7)
    # from the reset states no episode of 7 steps reaches a goal: reward -1 a step, return = -length
    assert float(runs[0]["ret_stats"][:, 1].sum()) == -float(runs[0]["stats"][:, 1].sum())
    act = _actors(env, N, n_step=3, max_episode_steps=7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records one step; nothing runs
        act.step(net)
    assert int(act.t_dev.sum()) == 0
    for _ in range(T):
        g.replay()
    torch.cuda.synchronize()
    _same(runs[0], _snapshot(act))


@pytest.mark.parametrize("env", ENVS)
def test_position_independence_grid_stride_and_single_env(env):
    """envs 0..7 of N = 8200 (1025 tiles > the 1024-workgroup grid: the grid-stride loop) equal an
    N = 8 run step for step; N = 1 equals env 0"""
    net = _net(env, 5)
    rng = np.random.default_rng(9)
    eps8 = np.array([0.0, 1.0, 0.3, 0.5, 0.7, 0.1, 0.9, 0.4])
    big = _actors(env, 8200, n_step=1, max_episode_steps=4, eps=np.concatenate([eps8, rng.uniform(0, 1, 8192)]))
    small = _actors(env, 8, n_step=1, max_episode_steps=4, eps=eps8)
    one = _actors(env, 1, n_step=1, max_episode_steps=4, eps=eps8[:1])
    keys = ["state", "ep_steps", "t_dev", "stats", "ret_stats", "cur_slot", "action", "reward", "done", "emit", "row_a",
            "row_r", "row_done", "row_obs0", "row_obs1"]
    for t in range(10):
        for act in (big, small, one):
            act.step(net)
        for k in keys:
            b, s, o = (getattr(act, k).cpu().numpy() for act in (big, small, one))
            assert b[:8].tobytes() == s.tobytes(), (t, k)
            assert s[:1].tobytes() == o.tobytes(), (t, k)
        np.testing.assert_array_equal(big.current_obs()[:8].cpu().numpy(), small.current_obs().cpu().numpy())
    # the last tile of the big run (envs 8192..8199, reached through the stride) stepped too
    assert (big.t_dev.cpu().numpy() == 10).all() and int(big.stats[8192:, 0].sum()) >= 8 * 2


@pytest.mark.parametrize("env", ENVS)
def test_no_write_outside_any_buffer(env):
    from reth_amd.mlp_actors import VecMlpActors

    G = 64

    class Guarded(VecMlpActors):
        def _alloc(self, shape, dtype):
            n = int(np.prod(shape))
            canary = 12345.5 if dtype.is_floating_point else 0x5A5A5A5A
            buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
            buf[G:G + n] = 0
            self.__dict__.setdefault("_guarded", []).append((buf, n, canary))
            return buf[G:G + n].view(shape)

    net = _net(env, 6)
    act = Guarded(env, 67, n_step=3, max_episode_steps=5, seed=SEED, device="cuda")
    act.want_q()
    for _ in range(12):
        act.step(net)
    torch.cuda.synchronize()
    assert len(act._guarded) == 22  # every device buffer of the actor set, ret_stats and q_out included
    assert int(act.emit.sum()) == 67 and int(act.stats[:, 0].sum()) >= 67 * 2
    for buf, n, canary in act._guarded:
        assert (buf[:G] == canary).all() and (buf[G + n:] == canary).all(), (buf.dtype, n)
