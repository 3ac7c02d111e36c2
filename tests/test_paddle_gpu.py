"""The device-resident Paddle game (csrc/game.hpp; rth_game_reset / rth_game_env_step /
rth_game_actor_tail, VecActors(env="paddle"), ApexDQN(env="paddle")) against its host restatement
reth_amd.envs.Paddle fed the device's documented Philox draws.  Everything compared is an integer
or a copied byte (the |td| of the tail: the same f32 operations as rth_td_huber), so every
comparison is bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STREAM_GAME = 8
RING = 16  # VecActors' ring for n_step = 3


def _draw(orc, seed):
    """envs.Paddle's draw(env, t): words 0..2 of the block {env, t lo, t hi, 8} under key = seed"""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    return lambda env, t: orc.philox4x32([env, t & 0xFFFFFFFF, t >> 32, STREAM_GAME], key)[:3]


def _host_games(orc, seed, N, A, balls):
    from reth_amd.envs import Paddle

    games = [Paddle(A, balls, draw=_draw(orc, seed), env=i) for i in range(N)]
    return games, [g.reset() for g in games]


def _track(state):
    target, px = int(state[0]) - 4, int(state[4])
    return 0 if abs(px - target) < 2 else (1 if px < target else 2)


class _Slots:
    """the frame-ring slot arithmetic of env_step_one, on the host"""

    def __init__(self, N, ring):
        self.ring, self.cur, self.base = ring, np.ones(N, np.int64), np.arange(N, dtype=np.int64) * ring

    def step(self, t, done):
        nxt, rst = (2 * t) % self.ring, (2 * t + 1) % self.ring
        s0h, s1h = self.base + self.cur, self.base + nxt
        self.cur = np.where(done, rst, nxt)
        return s0h, s1h, self.base + rst


def _game_buffers(dev, N, ring, seed, balls, action_in=None):
    from reth_amd import _lib

    frames = torch.zeros((N * ring + 1, 4, 84, 84), dtype=torch.uint8, device=dev)
    z = lambda dt, *s: torch.zeros((N, *s), dtype=dt, device=dev)
    b = dict(frames=frames, cur=z(torch.int64), state=z(torch.int32, 8), stats=z(torch.int64, 4), r=z(torch.float32),
             done=z(torch.float32), s0h=z(torch.int64), s1h=z(torch.int64))
    b["args"] = _lib.GameArgs(b["state"].data_ptr(), b["stats"].data_ptr(), _lib.ptr(action_in), seed, N, balls, 0)
    _lib.call("rth_game_reset", _lib.ctypes.byref(b["args"]), frames.data_ptr(), N, ring, b["cur"].data_ptr(),
              _lib.stream_ptr())
    return b


def test_game_env_step_matches_host_game(dev, orc):
    """N = 8 envs, 2 balls an episode, 120 scripted steps: state, reward, done, handles, cur_slot,
    stats and the full bytes of every stack written (shifted, terminal, reset x4) after every step.
    Envs 0-3 play scripted noise, envs 4-7 track the ball (with noise every 9th step): the run
    holds catches, misses, bounces on both walls and an episode end in every env (asserted)."""
    from reth_amd import _lib

    N, A, balls, seed, T = 8, 6, 2, 20260, 120
    games, obs = _host_games(orc, seed, N, A, balls)
    b = _game_buffers(dev, N, RING, seed, balls)
    slots = _Slots(N, RING)
    assert np.array_equal(b["state"].cpu().numpy(), np.stack([g.state for g in games]))
    assert np.array_equal(b["frames"][slots.base + 1].cpu().numpy(), np.stack(obs))  # the reset stack, slot 1
    assert bool((b["cur"] == 1).all()) and not bool(b["stats"].any())
    rng = np.random.RandomState(1)
    stats = np.zeros((N, 4), np.int64)
    seen = dict(catch=0, miss=0, left=0, right=0, ends=np.zeros(N, int))
    action = torch.zeros(N, dtype=torch.int64, device=dev)
    for t in range(1, T + 1):
        a = np.array([rng.randint(A) if i < 4 or t % 9 == 0 else _track(games[i].state) for i in range(N)])
        action.copy_(torch.from_numpy(a))
        _lib.call("rth_game_env_step", _lib.ctypes.byref(b["args"]), b["frames"].data_ptr(), N, RING, t, None,
                  b["cur"].data_ptr(), action.data_ptr(), b["r"].data_ptr(), b["done"].data_ptr(),
                  b["s0h"].data_ptr(), b["s1h"].data_ptr(), _lib.stream_ptr())
        want_r, want_d, nxt_obs, rst_obs = np.zeros(N, np.float32), np.zeros(N, bool), [], {}
        for i, g in enumerate(games):
            vx = int(g.state[2])
            o, want_r[i], want_d[i], _ = g.step(a[i])
            nxt_obs.append(o)
            seen["catch"] += want_r[i] > 0
            seen["miss"] += want_r[i] < 0
            if want_r[i] == 0 and int(g.state[2]) == -vx:
                seen["left" if vx < 0 else "right"] += 1
            if want_d[i]:
                stats[i] += (1, g.state[6], 0, 0)
                stats[i, 2:] = g.state[6], g.state[7]
                seen["ends"][i] += 1
                rst_obs[i] = g.reset()
        s0h, s1h, rsth = slots.step(t, want_d)
        assert np.array_equal(b["state"].cpu().numpy(), np.stack([g.state for g in games])), t
        assert np.array_equal(b["r"].cpu().numpy(), want_r) and np.array_equal(b["done"].cpu().numpy() != 0, want_d), t
        assert np.array_equal(b["s0h"].cpu().numpy(), s0h) and np.array_equal(b["s1h"].cpu().numpy(), s1h), t
        assert np.array_equal(b["cur"].cpu().numpy(), slots.cur) and np.array_equal(b["stats"].cpu().numpy(), stats), t
        assert np.array_equal(b["frames"][torch.from_numpy(s1h).to(dev)].cpu().numpy(), np.stack(nxt_obs)), t
        for i, o in rst_obs.items():
            assert np.array_equal(b["frames"][int(rsth[i])].cpu().numpy(), o), (t, i)
    assert seen["catch"] > 0 and seen["miss"] > 0 and seen["left"] > 0 and seen["right"] > 0, seen
    assert (seen["ends"] >= 1).all(), seen
    assert not bool(b["frames"][-1].any())  # the sink stack stays zero


@pytest.mark.parametrize("A", [3, 6, 12])
def test_game_actor_tail_matches_the_separate_calls(dev, A):
    """rth_game_actor_tail = rth_eps_greedy + rth_td_huber + rth_game_env_step + rth_nstep_push:
    actions, |td|, transitions, rows, frames, state and stats equal over 45 steps of one-ball
    episodes (every env ends one).  A = 3, 6: the in-register heads rows (MAXL = 8); A = 12: the
    general form."""
    from reth_amd import _lib
    from reth_amd._lib import call, ptr, stream_ptr
    from reth_amd.solver import td_huber_forward

    N, n, gamma, seed, T = 8, 3, 0.99, 77, 45
    gamma_n = float(np.float32(gamma ** n))
    g = torch.Generator(device=dev).manual_seed(A)
    eps = torch.tensor([0.0, 1.0, 0.5, 0.3, 0.0, 0.9, 0.5, 0.1], dtype=torch.float64, device=dev)
    z = lambda dt: torch.zeros(N, dtype=dt, device=dev)
    t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    sides = []
    for _ in range(2):
        b = _game_buffers(dev, N, RING, seed, 1)
        h = _lib.c_vp()
        call("rth_nstep_create", N, n, gamma, 0, dev.index or 0, _lib.ctypes.byref(h))
        b.update(h=h.value, action=z(torch.int64), emit=z(torch.int32), td=z(torch.float32),
                 rows=[z(torch.int64), z(torch.int64), z(torch.float32), z(torch.int64), z(torch.float32)])
        sides.append(b)
    sep, fused = sides
    try:
        ends = 0
        for t in range(1, T + 1):
            t_dev.fill_(t)
            q = torch.randn((N, A + 1), device=dev, generator=g)
            qcache = torch.randn((N * RING + 1, A + 1), device=dev, generator=g)
            ps0, ps1 = (torch.randint(0, N * RING + 1, (N,), device=dev, generator=g) for _ in range(2))
            pa = torch.randint(0, A, (N,), device=dev, generator=g)
            pr = torch.randint(-1, 2, (N,), device=dev, generator=g).float()
            pd = torch.randint(0, 2, (N,), device=dev, generator=g).float()
            # the separate calls
            b = sep
            call("rth_eps_greedy", ptr(q), N, A, 1, ptr(eps), None, None, seed, 0, ptr(t_dev), ptr(b["action"]),
                 stream_ptr())
            _, td, _ = td_huber_forward(qcache[ps0], qcache[ps1], qcache[ps1], pa, pr, pd, None, gamma_n, True,
                                        want_dq=False, dueling=True)
            call("rth_game_env_step", _lib.ctypes.byref(b["args"]), ptr(b["frames"]), N, RING, 0, ptr(t_dev),
                 ptr(b["cur"]), ptr(b["action"]), ptr(b["r"]), ptr(b["done"]), ptr(b["s0h"]), ptr(b["s1h"]),
                 stream_ptr())
            call("rth_nstep_push", b["h"], ptr(b["s0h"]), ptr(b["action"]), ptr(b["r"]), ptr(b["s1h"]), ptr(b["done"]),
                 ptr(b["emit"]), *[ptr(x) for x in b["rows"]], stream_ptr())
            # one launch
            f = fused
            args = _lib.ActorTailArgs(ptr(q), ptr(eps), ptr(t_dev), ptr(f["action"]), ptr(qcache), ptr(ps0), ptr(pa),
                                      ptr(ps1), ptr(pr), ptr(pd), ptr(f["td"]), ptr(f["frames"]), ptr(f["cur"]),
                                      ptr(f["r"]), ptr(f["done"]), ptr(f["s0h"]), ptr(f["s1h"]), seed, N, gamma_n,
                                      0.0, 0.0, RING, A, 0)
            call("rth_game_actor_tail", f["h"], _lib.ctypes.byref(args), _lib.ctypes.byref(f["args"]), ptr(f["emit"]),
                 *[ptr(x) for x in f["rows"]], stream_ptr())
            assert torch.equal(b["action"], f["action"]) and torch.equal(td, f["td"]), t
            for k in ("r", "done", "s0h", "s1h", "cur", "state", "stats", "emit"):
                assert torch.equal(b[k], f[k]), (t, k)
            if t > n:
                assert bool(f["emit"].all())
                for x, y in zip(b["rows"], f["rows"]):
                    assert torch.equal(x, y), t
            ends += int(f["done"].sum())
        assert torch.equal(sep["frames"], fused["frames"])
        assert ends >= N and bool((fused["stats"][:, 0] >= 1).all())
    finally:
        for b in sides:
            _lib.lib().rth_nstep_destroy(b["h"])


def _net(dev, hip, A=6):
    from reth_amd.model import DQNNetwork

    torch.manual_seed(0)
    if not hip:
        return DQNNetwork((4, 84, 84), A).to(dev)
    net = DQNNetwork((4, 84, 84), A).to(dev, memory_format=torch.channels_last)
    net.hwc_features = True
    net.requires_grad_(False)
    return net


def _actor_run(dev, orc, mode, T=48, N=8, seed=5):
    """T steps of VecActors(env="paddle"), one-ball episodes, checked against the host game fed the
    device's actions and the oracle's NStepAdder fed its transitions; returns the run's trace"""
    from reth_amd.actors import VecActors

    hip = mode == "fused"
    net = _net(dev, hip)
    act = VecActors(N, 6, n_step=3, gamma=0.99, device=dev, seed=seed, channels_last=hip, env="paddle",
                    balls_per_episode=1)
    assert act.ring == RING
    games, _ = _host_games(orc, seed, N, 6, 1)
    slots = _Slots(N, RING)
    adders = [orc.NStep(3, 0.99, 0) for _ in range(N)]
    trace, ends = [], 0
    for t in range(1, T + 1):
        if hip:
            act.step_fused(net)
        else:
            act.step(net)
        a = act.action.cpu().numpy()
        r, d = np.zeros(N, np.float32), np.zeros(N, bool)
        obs = []
        for i, g in enumerate(games):
            o, r[i], d[i], _ = g.step(a[i])
            obs.append(o)
            if d[i]:
                g.reset()
        s0h, s1h, _ = slots.step(t, d)
        assert np.array_equal(act.reward.cpu().numpy(), r) and np.array_equal(act.done.cpu().numpy() != 0, d), t
        assert np.array_equal(act.s0_h.cpu().numpy(), s0h) and np.array_equal(act.s1_h.cpu().numpy(), s1h), t
        assert np.array_equal(act.frames[act.s1_h].cpu().numpy(), np.stack(obs)), t
        assert np.array_equal(act.frames[act.current_obs_handles()].cpu().numpy(),
                              np.stack([g._stack for g in games])), t
        rows = [adders[i].push(s0h[i], a[i], r[i], s1h[i], np.float32(d[i])) for i in range(N)]
        got = [x.cpu().numpy() for x in (act.row_s0, act.row_a, act.row_r, act.row_s1, act.row_done)]
        if t > 3:
            for i in range(N):
                assert tuple(c[i] for c in got) == rows[i], (t, i)
        else:
            assert all(x is None for x in rows)
        ends += int(d.sum())
        trace.append((a, got))
    ep, ret, last, length = (x.cpu().numpy() for x in act.episode_stats())
    assert ends >= N and ep.sum() == ends and (np.abs(last) == 1).all() and ((25 <= length) & (length <= 38)).all()
    return trace, act.frames.cpu(), act.game_state.cpu()


@pytest.mark.parametrize("mode", ["step", "fused"])
def test_vec_actors_paddle_rows_match_oracle_and_repeat(dev, orc, mode):
    """step() and step_fused() (the tail kernel, full and dedup forwards): the transitions are the
    host game's under the device's actions, the n-step rows the oracle NStepAdder's; a second run
    gives the same actions, rows, frames and state"""
    tr1, f1, s1 = _actor_run(dev, orc, mode)
    tr2, f2, s2 = _actor_run(dev, orc, mode)
    assert torch.equal(f1, f2) and torch.equal(s1, s2)
    for (a1, g1), (a2, g2) in zip(tr1, tr2):
        assert np.array_equal(a1, a2) and all(np.array_equal(x, y) for x, y in zip(g1, g2))


def test_vec_actors_rejects_unknown_env(dev):
    from reth_amd.actors import VecActors

    with pytest.raises(ValueError, match="paddle"):
        VecActors(4, 6, device=dev, env="pong")


def _apex(dev, iters, **kw):
    from reth_amd.apex import ApexConfig, ApexDQN
    from reth_amd.replay import FrameStacks

    base = dict(n_actors=16, capacity=1024, batch_size=32, sample_start=64, seed=4, send_weights_interval=3,
                recv_weights_interval=4, update_target_interval=5, env="paddle", balls_per_episode=1)
    base.update(kw)
    ax = ApexDQN(ApexConfig(**base), device=dev)
    snaps = []
    for _ in range(iters):
        ax.iteration()
        with torch.cuda.stream(ax._stream):  # the stream the actor steps run on
            snaps.append(ax.actors.game_stats[:, 0].sum())
    torch.cuda.synchronize()
    assert (ax._graphs is not None) == bool(base.get("hip_graph"))
    s, m, v = ax.replay.tree.export()
    cols = ax.replay.gather(torch.arange(ax.replay.info()[0], device=dev))
    cols = [c.stacks() if isinstance(c, FrameStacks) else c for c in cols]
    out = dict(tree=[s.cpu(), m.cpu(), v.cpu()], cols=[c.cpu() for c in cols], info=ax.replay.info(),
               state=ax.actors.game_state.cpu(), stats=ax.actors.game_stats.cpu(), frames=ax.actors.frames.cpu(),
               params=torch.cat([p.detach().flatten() for p in ax.solver._params]).cpu(),
               episodes=[int(x) for x in snaps], updates=ax.updates)
    ax.close()
    return out


def _same(a, b, keys):
    for k in keys:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), k


def test_apex_paddle_graph_replay_matches_eager(dev):
    """lr = 0 (fixed networks): the captured two-stream loop leaves the replay, the tree, the frame
    ring and the game exactly where the eager loop does, through episode ends in every env"""
    a = _apex(dev, 45, learning_rate=0.0, hip_graph=False)
    b = _apex(dev, 45, learning_rate=0.0, hip_graph=True)
    assert a["info"] == b["info"] and a["episodes"] == b["episodes"]
    _same(a, b, ["tree", "cols", "state", "stats", "frames"])
    assert bool((b["stats"][:, 0] >= 1).all())


def test_apex_paddle_learning_loop(dev):
    """learning on, 50 iterations of the captured loop: finite weights, n-step rewards of the
    replay rows in {-1, 0, 1} x {1, gamma, gamma^2} (balls are 25+ steps apart: at most one reward
    per 3-step window; 1-step rewards are in {-1, 0, 1}), and as many done rows as the device
    statistics counted episodes by the step the last appended rows were emitted from"""
    T, n = 50, 3
    o = _apex(dev, T, hip_graph=True)
    assert o["updates"] > 30 and bool(torch.isfinite(o["params"]).all())
    rows = o["info"][0]
    assert rows == 16 * (T - n - 1)  # fused actors: a step's rows are appended one step later
    g = [np.float32(1.0), np.float32(0.99), np.float32(0.99 * 0.99)]
    allowed = np.array([0.0] + [s * x for x in g for s in (1, -1)], np.float32)
    r = o["cols"][2].numpy()
    assert np.isin(r, allowed).all() and (r != 0).any(), np.unique(r)
    done = o["cols"][4].numpy()
    assert set(np.unique(done)) == {0.0, 1.0}
    # a done row is emitted with its own 1-step reward only
    assert np.isin(r[done != 0], [-1.0, 1.0]).all()
    # rows emitted so far cover the transitions of steps 1 .. T - n - 1
    assert int(done.sum()) == o["episodes"][T - n - 2] > 0


def test_apex_paddle_frame_store_rows_equal_full_rows(dev):
    """with the frame store attached (the game's frames enter it once, rows are frame ids) every
    replay row, the tree and the learner's parameters equal the full-row loop's"""
    full = _apex(dev, 110, hip_graph=True, seed=6)
    fs = _apex(dev, 110, hip_graph=True, seed=6, frame_store=True, frame_store_bound="expected")
    assert full["info"] == fs["info"] and full["updates"] == fs["updates"] > 50 and fs["info"][0] == 1024
    _same(full, fs, ["cols", "tree", "frames", "state", "params"])
    assert bool((fs["cols"][4] != 0).any())


def test_greedy_eval(dev, orc):
    """greedy_eval = the mean of each env's first-episode return as the device statistics hold
    it; a paddle-tracking action table fed through action_in returns +balls"""
    from reth_amd.apex import ApexConfig, ApexDQN

    balls = 2
    ax = ApexDQN(ApexConfig(n_actors=16, capacity=1024, batch_size=32, seed=2, env="paddle", balls_per_episode=balls),
                 device=dev)
    seen = []

    def watch(ev):  # before every step: the statistics so far
        seen.append((ev, ev.game_stats.clone()))
        return None

    v = ax.greedy_eval(n_envs=32, seed=11, action_fn=watch)
    assert len(seen) == 38 * balls
    snaps = [s.cpu().numpy() for _, s in seen] + [seen[-1][0].game_stats.cpu().numpy()]
    first = np.full(32, np.nan)
    for s in snaps:
        new = np.isnan(first) & (s[:, 0] > 0)
        first[new] = s[new, 2]
    assert not np.isnan(first).any() and v == float(first.sum() / 32) and -balls <= v <= balls
    assert ax.greedy_eval(n_envs=32, seed=11) == v  # the same network, the same envs

    def track(ev):
        st = ev.game_state
        target, px = st[:, 0] - 4, st[:, 4]
        move = torch.where(px < target, 1, 2)
        return torch.where((px - target).abs() < 2, 0, move).to(torch.int64).contiguous()

    assert ax.greedy_eval(n_envs=32, seed=11, action_fn=track) == float(balls)
    assert -balls <= ax.greedy_eval(n_envs=32, seed=11, eps=1.0) <= balls  # the random policy over the same envs
    ax.close()
