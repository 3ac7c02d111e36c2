"""The device CartPole actors (rth_mlp_actor_step, reth_amd/mlp_actors.py) on the GPU: the env
step against the host envs.CartPole, acting against rth_mlp_q + the oracle's ε-greedy on the
documented Philox draws, the n-step rows against the oracle's NStepAdder, determinism, graph
replay, position independence / the grid-stride loop, and buffer bounds."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678
STREAM_EXPLORE, STREAM_RANDACT, STREAM_CARTPOLE = 2, 3, 7
X_THR, TH_THR = 2.4, 12 * 2 * math.pi / 360


def _net(seed=0):
    from reth_amd import model

    torch.manual_seed(seed)
    net = model.MLP_DQNNetwork((4,), 2).to("cuda")
    net.requires_grad_(False)
    return net


def _actors(n, **kw):
    from reth_amd.mlp_actors import VecCartPoleActors

    kw.setdefault("seed", SEED)
    return VecCartPoleActors(n, device="cuda", **kw)


def _mlp_q(net, obs):
    from reth_amd import _lib

    obs = obs.contiguous()
    q = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=obs.device)
    arr = (_lib.c_vp * 6)(*[p.data_ptr() for p in net._params6()])
    _lib.call("rth_mlp_q", arr, obs.data_ptr(), 4, obs.shape[0], 4, 128, 2, q.data_ptr(), None, _lib.stream_ptr())
    return q


def _key(seed):
    return [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]


def _reset_state(orc, seed, i, t):
    """the documented reset draw (csrc/mlp_actor.hpp): one Philox block per (seed, env, t)"""
    c = orc.philox4x32([i, t & 0xFFFFFFFF, t >> 32, STREAM_CARTPOLE], _key(seed)).astype(np.float64)
    return -0.05 + (0.1 * c) / 2.0 ** 32


def _cases(rng, n, max_steps):
    """(states [n, 4], steps [n], kind [n]) -- see test_env_step_matches_host_cartpole"""
    st = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(-0.15, 0.15, n),
                   rng.uniform(-1, 1, n)], axis=1)
    steps = rng.integers(0, max_steps - 2, n)
    kind = np.array(["interior"] * n, dtype=object)
    tau, m = 0.02, 2e-6
    k = 30
    for sign in (1.0, -1.0):  # beyond / inside each of the four sides by 2e-6 (>= 1e-6 asked)
        for v in (1.0, 0.3):
            st[k, 0], st[k, 1], kind[k] = sign * (X_THR - tau * v + m), sign * v, "out"
            st[k + 1, 0], st[k + 1, 1], kind[k + 1] = sign * (X_THR - tau * v - m), sign * v, "in"
            st[k + 2, 2], st[k + 2, 3], kind[k + 2] = sign * (TH_THR - tau * v + m), sign * v, "out"
            st[k + 3, 2], st[k + 3, 3], kind[k + 3] = sign * (TH_THR - tau * v - m), sign * v, "in"
            k += 4
    for j in range(k, k + 6):  # the time limit on interior states
        steps[j], kind[j] = max_steps - 1, "limit"
    return st, steps, kind


def test_env_step_matches_host_cartpole(capsys):
    from oracle import oracle as orc
    from reth_amd.envs import CartPole

    N, MAX = 67, 200
    rng = np.random.default_rng(5)
    st, steps, kind = _cases(rng, N, MAX)
    a = rng.integers(0, 2, N)
    exp_s, exp_done = np.empty((N, 4)), np.empty(N, bool)
    for i in range(N):
        env = CartPole(MAX)
        env.state, env._t = st[i].copy(), int(steps[i])
        o, r, d, _ = env.step(int(a[i]))
        assert r == 1.0
        exp_s[i], exp_done[i] = o, d
    # no case sits within 1e-9 of a threshold on the host; the constructed sides are >= 1e-6 off
    dist = np.minimum(np.abs(np.abs(exp_s[:, 0]) - X_THR), np.abs(np.abs(exp_s[:, 2]) - TH_THR))
    assert dist.min() >= 1e-9
    edge = (kind == "out") | (kind == "in")
    assert edge.sum() == 16 and (dist[edge] >= 1e-6).all() and (dist[edge] <= 3e-6).all()
    assert exp_done[kind == "out"].all() and exp_done[kind == "limit"].all()
    assert not exp_done[kind == "in"].any() and not exp_done[kind == "interior"].any()

    net = _net()
    act = _actors(N, n_step=1, max_episode_steps=MAX)
    act.set_state(st, steps)
    obs0 = act.current_obs()
    assert torch.equal(obs0.cpu(), torch.as_tensor(st).float())
    a_dev = torch.as_tensor(a, dtype=torch.int64, device="cuda")
    assert act.step(net, a_dev) is False  # n = 1: the first push emits nothing
    assert int(act.emit.sum()) == 0
    done = act.done.cpu().numpy() != 0
    np.testing.assert_array_equal(done, exp_done)
    assert (act.reward.cpu().numpy() == 1.0).all()
    np.testing.assert_array_equal(act.action.cpu().numpy(), a)
    state = act.state.cpu().numpy()
    ring = act.obs_ring.cpu().numpy()
    s0_h, s1_h = act.s0_h.cpu().numpy(), act.s1_h.cpu().numpy()
    cur = (act._base + act.cur_slot).cpu().numpy()
    np.testing.assert_array_equal(ring[s0_h], st.astype(np.float32))
    # running episodes: the fp64 state against the host's, 1e-12 * max(1, |v|)
    live = ~done
    err = np.abs(state[live] - exp_s[live]) / np.maximum(1.0, np.abs(exp_s[live]))
    with capsys.disabled():
        print(f"\n[mlp_actors] env-step max |device - host| / max(1, |host|) over {live.sum()} running rows: "
              f"{err.max():.3e}")
    assert err.max() <= 1e-12
    np.testing.assert_array_equal(ring[s1_h[live]], state[live].astype(np.float32))  # obs = float32(own state)
    np.testing.assert_array_equal(cur[live], s1_h[live])
    # finished episodes: the fp64 state is already the reset one, so the terminal state is seen
    # through its f32 observation: float32 of a value within 1e-12 relative of the host's lies
    # within one f32 spacing of float32(host)
    term, want = ring[s1_h[done]], exp_s[done].astype(np.float32)
    assert (np.abs(term - want) <= np.spacing(np.abs(want))).all()
    assert (cur[done] != s1_h[done]).all() and (cur[done] // act.ring == np.arange(N)[done]).all()
    for i in np.nonzero(done)[0]:  # the reset: the documented Philox draw at t = 1, and its observation
        want_s = _reset_state(orc, SEED, int(i), 1)
        np.testing.assert_array_equal(state[i], want_s)
        assert (want_s >= -0.05).all() and (want_s < 0.05).all()
    np.testing.assert_array_equal(ring[cur[done]], state[done].astype(np.float32))
    np.testing.assert_array_equal(ring[N * act.ring], np.zeros(4, np.float32))  # the sink row stays zero
    # step counts and episode statistics
    np.testing.assert_array_equal(act.ep_steps.cpu().numpy(), np.where(done, 0, steps + 1))
    ep, tot, last = (t.cpu().numpy() for t in act.episode_stats())
    np.testing.assert_array_equal(ep, done.astype(np.int64))
    np.testing.assert_array_equal(tot, np.where(done, steps + 1, 0))
    np.testing.assert_array_equal(last, np.where(done, steps + 1, 0))
    np.testing.assert_array_equal(act.t_dev.cpu().numpy(), np.ones(N, np.int64))
    # the second step emits the first transition by value: s1 of a done row is the terminal obs
    assert act.step(net, a_dev) is True
    assert int(act.emit.sum()) == N
    s0, ra, rr, s1, rd = (t.cpu().numpy() for t in act.rows())
    np.testing.assert_array_equal(s0, st.astype(np.float32))
    np.testing.assert_array_equal(s1, ring[s1_h])
    np.testing.assert_array_equal(ra, a)
    np.testing.assert_array_equal(rr, np.ones(N, np.float32))
    np.testing.assert_array_equal(rd, done.astype(np.float32))
    np.testing.assert_array_equal(act.row_s0.cpu().numpy(), s0_h)
    np.testing.assert_array_equal(act.row_s1.cpu().numpy(), s1_h)


def test_initial_reset_is_the_documented_draw():
    from oracle import oracle as orc

    act = _actors(5)
    state = act.state.cpu().numpy()
    for i in range(5):
        np.testing.assert_array_equal(state[i], _reset_state(orc, SEED, i, 0))
    assert torch.equal(act.current_obs().cpu(), torch.as_tensor(state).float())
    assert (act.cur_slot.cpu() == 1).all() and int(act.t_dev.sum()) == 0


def _draws(orc, seed, n, t):
    u = np.array([orc.philox_uniform(seed, t, i, STREAM_EXPLORE) for i in range(n)])
    ra = np.array([(int(orc.philox4x32([i, t & 0xFFFFFFFF, t >> 32, STREAM_RANDACT], _key(seed))[0]) * 2) >> 32
                   for i in range(n)], dtype=np.int64)
    return u, ra


def test_acting_matches_mlp_q_and_oracle_eps_greedy():
    from oracle import oracle as orc

    N = 67
    eps = np.concatenate([np.zeros(20), np.ones(20), np.linspace(0.2, 0.8, N - 40)])
    net = _net(1)
    act = _actors(N, eps=eps)
    q_out = act.want_q()
    explored = 0
    for t in (1, 2, 3):
        obs = act.current_obs()
        q_ref = _mlp_q(net, obs)
        act.step(net)
        assert torch.equal(q_out, q_ref)  # bit-equal to rth_mlp_q on the same observations
        u, ra = _draws(orc, SEED, N, t)
        want = orc.eps_greedy(q_ref.cpu().numpy(), eps, u, ra)
        np.testing.assert_array_equal(act.action.cpu().numpy(), want)
        explored += int((u < eps).sum())
    assert 60 < explored < 3 * N - 60  # both branches ran


def test_tied_q_gives_action_zero_where_greedy():
    from oracle import oracle as orc

    N = 67
    eps = np.concatenate([np.zeros(30), np.full(N - 30, 0.5)])
    net = _net(2)
    net.nn[4].weight.zero_()
    net.nn[4].bias.zero_()
    act = _actors(N, eps=eps)
    q_out = act.want_q()
    act.step(net)
    assert (q_out == 0).all()
    u, ra = _draws(orc, SEED, N, 1)
    a = act.action.cpu().numpy()
    assert (a[u >= eps] == 0).all()
    np.testing.assert_array_equal(a[u < eps], ra[u < eps])


@pytest.mark.parametrize("n_step,mode", [(1, 0), (1, 1), (3, 0), (3, 1)])
def test_nstep_rows_match_oracle(n_step, mode):
    from oracle import oracle as orc

    N, T = 20, 40
    net = _net(3)
    act = _actors(N, n_step=n_step, gamma=0.99, max_episode_steps=5, nstep_mode=mode)
    adders = [orc.NStep(n_step, 0.99, mode) for _ in range(N)]
    trace = {}  # handle -> the observation it held when the trace last named it
    emitted = dones = 0
    for t in range(T):
        act.step(net)
        ring = act.obs_ring.cpu().numpy()
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
        assert act.warm == (t + 1 > n_step)
    assert emitted == N * (T - n_step) and dones >= N * (T // 5)  # the time limit alone ends T / 5 episodes per env


def _snapshot(act):
    names = ["state", "ep_steps", "t_dev", "stats", "obs_ring", "cur_slot", "action", "reward", "done", "s0_h", "s1_h",
             "emit", "row_s0", "row_a", "row_s1", "row_r", "row_done", "row_obs0", "row_obs1"]
    return {k: getattr(act, k).clone() for k in names}


def _same(a, b):
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_deterministic_and_graph_replay_equals_eager():
    N, T = 67, 30
    net = _net(4)
    runs = []
    for _ in range(2):
        act = _actors(N, n_step=3, max_episode_steps=7)
        for _ in range(T):
            act.step(net)
        runs.append(_snapshot(act))
    _same(runs[0], runs[1])
    assert int(runs[0]["stats"][:, 0].sum()) >= N * (T // 7)
    act = _actors(N, n_step=3, max_episode_steps=7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # records one step; nothing runs
        act.step(net)
    assert int(act.t_dev.sum()) == 0
    for _ in range(T):
        g.replay()
    torch.cuda.synchronize()
    _same(runs[0], _snapshot(act))


def test_position_independence_grid_stride_and_single_env():
    """envs 0..7 of N = 8200 (1025 tiles > the 1024-workgroup grid: the grid-stride loop) equal an
    N = 8 run step for step; N = 1 equals env 0"""
    net = _net(5)
    rng = np.random.default_rng(9)
    eps8 = np.array([0.0, 1.0, 0.3, 0.5, 0.7, 0.1, 0.9, 0.4])
    big = _actors(8200, n_step=1, max_episode_steps=4, eps=np.concatenate([eps8, rng.uniform(0, 1, 8192)]))
    small = _actors(8, n_step=1, max_episode_steps=4, eps=eps8)
    one = _actors(1, n_step=1, max_episode_steps=4, eps=eps8[:1])
    keys = ["state", "ep_steps", "t_dev", "stats", "cur_slot", "action", "done", "emit", "row_a", "row_r", "row_done",
            "row_obs0", "row_obs1"]
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


def test_no_write_outside_any_buffer():
    from reth_amd.mlp_actors import VecCartPoleActors

    G = 64

    class Guarded(VecCartPoleActors):
        def _alloc(self, shape, dtype):
            n = int(np.prod(shape))
            canary = 12345.5 if dtype.is_floating_point else 0x5A5A5A5A
            buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
            buf[G:G + n] = 0
            self.__dict__.setdefault("_guarded", []).append((buf, n, canary))
            return buf[G:G + n].view(shape)

    net = _net(6)
    act = Guarded(67, n_step=3, max_episode_steps=5, seed=SEED, device="cuda")
    act.want_q()
    for _ in range(12):
        act.step(net)
    torch.cuda.synchronize()
    assert len(act._guarded) == 21  # every device buffer of the actor set, q_out included
    assert int(act.emit.sum()) == 67 and int(act.stats[:, 0].sum()) >= 67 * 2
    for buf, n, canary in act._guarded:
        assert (buf[:G] == canary).all() and (buf[G + n:] == canary).all(), (buf.dtype, n)
