"""The Paddle game on the host (reth_amd.envs.Paddle): the integer rules on hand-built states,
the render, and the two policies that bracket what a learner can reach.  The device game
(csrc/game.hpp) is compared against this restatement bit for bit in test_paddle_gpu.py."""
import numpy as np
import pytest

from reth_amd.envs import Paddle, make

BX, BY, VX, VY, PX, BALLS, RET, STEPS = range(8)


def _env(state, A=6, balls=5, draws=None):
    """a game standing at `state` = (ball_x, ball_y, vx, vy, paddle_x[, balls_left]); spawns
    take `draws` (uint32 triples) in turn"""
    it = iter(draws or [])
    e = Paddle(A, balls, draw=lambda env, t: (0, 0, 0))
    e.reset()
    e.draw = lambda env, t: next(it)
    e.state[:len(state)] = state
    return e


def track(e):
    """move the paddle's centre under the ball's"""
    target = int(e.state[BX]) - 4
    px = int(e.state[PX])
    return 0 if abs(px - target) < 2 else (1 if px < target else 2)


@pytest.mark.parametrize("bx,vx,want_bx", [(2, -3, 1), (0, -1, 1), (1, -1, 0), (79, 3, 78), (80, 2, 78), (79, 1, 80)])
def test_wall_bounce(bx, vx, want_bx):
    """ball_x = -1 reflects to 1, ball_x = 82 to 160 - 82 = 78; touching the wall is no bounce"""
    e = _env((bx, 10, vx, 2, 36))
    e.step(0)
    bounced = not (0 <= bx + vx <= 80)
    assert e.state[BX] == want_bx and e.state[VX] == (-vx if bounced else vx)
    assert e.state[BY] == 12 and e.state[STEPS] == 1


@pytest.mark.parametrize("bx,px,reward", [(33, 36, 1.0), (32, 36, -1.0), (47, 36, 1.0), (48, 36, -1.0),
                                          (0, 3, 1.0), (0, 4, -1.0), (80, 69, 1.0), (80, 68, -1.0)])
def test_catch_and_miss_at_the_overlap_edges(bx, px, reward):
    """one pixel of overlap on either side is a catch, one pixel further a miss"""
    e = _env((bx, 73, 1 if bx < 80 else -1, 2, px), draws=[(5, 5, 5)])
    e.state[BX] -= e.state[VX]
    _, r, done, _ = e.step(0)
    assert r == reward and not done
    assert e.state[RET] == int(reward) and e.state[BALLS] == 4 and e.state[BY] == 0  # a new ball


def test_resolve_threshold():
    """ball_y + 4 > 78 resolves: ball_y = 74 does not, 75 does"""
    e = _env((40, 72, 1, 2, 36))
    assert e.step(0)[1:3] == (0.0, False) and e.state[BY] == 74 and e.state[BALLS] == 5
    e = _env((40, 72, 1, 3, 36), draws=[(0, 0, 0)])
    assert e.step(0)[1] == 1.0 and e.state[BALLS] == 4


@pytest.mark.parametrize("A", [3, 6])
def test_action_table_and_clamp(A):
    moves = {0: 0, 1: 4, 2: -4, 3: 4, 4: -4, 5: 4}
    for a in range(A):
        e = _env((40, 10, 1, 2, 36), A=A)
        e.step(a)
        assert e.state[PX] == 36 + moves[a], a
    with pytest.raises(AssertionError):
        _env((40, 10, 1, 2, 36), A=A).step(A)
    for px, a, want in [(2, 2, 0), (0, 2, 0), (70, 1, 72), (72, 1, 72), (72, 2, 68), (0, 1, 4)]:
        e = _env((40, 10, 1, 2, px), A=A)
        e.step(a)
        assert e.state[PX] == want


def test_last_ball_ends_the_episode_and_reset_starts_a_new_one():
    e = _env((40, 74, 1, 3, 36, 1))
    e.state[RET], e.state[STEPS] = -2, 77
    obs, r, done, _ = e.step(0)
    assert done and r == 1.0 and tuple(e.state) == (41, 77, 1, 3, 36, 0, -1, 78)
    assert np.array_equal(obs[3], e.render())  # the terminal observation: the ball at the paddle rows
    e.draw = lambda env, t: (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)
    obs = e.reset()
    assert tuple(e.state) == (80, 0, 3, 3, 36, 5, 0, 0)
    assert all(np.array_equal(obs[k], e.render()) for k in range(4))
    e.draw = lambda env, t: (0, 0, 0)
    e.reset()
    assert tuple(e.state[:4]) == (0, 0, -3, 2)


def test_draw_is_asked_for_the_step_counter():
    """a spawn at step t and the reset after a done at step t draw (env, t); the first reset t = 0"""
    asked = []

    def draw(env, t):
        asked.append((env, t))
        return (1 << 31, 1 << 31, 0)

    e = Paddle(3, 2, draw=draw, env=7)
    e.reset()
    done, n = False, 0
    while not done:
        done = e.step(0)[2]
        n += 1
    e.reset()
    assert asked == [(7, 0), (7, 38), (7, 76)] and n == 76  # vy = 2: 38 steps a ball


def test_render_is_a_rectangle_fill():
    e = _env((17, 5, 1, 2, 60))
    want = np.zeros((84, 84), np.uint8)
    for y in range(78, 81):
        for x in range(60, 72):
            want[y, x] = 160
    for y in range(5, 9):
        for x in range(17, 21):
            want[y, x] = 255
    assert np.array_equal(e.render(), want) and e.render().dtype == np.uint8
    # the ball is drawn over the paddle (a terminal state: ball rows 77..80)
    f = e.render((62, 77, 1, 2, 60))
    assert (f[77, 62:66] == 255).all() and (f[78:81, 62:66] == 255).all()
    assert (f[78:81, 60:62] == 160).all() and (f[78:81, 66:72] == 160).all() and int((f != 0).sum()) == 16 + 36 - 12


def test_observations_shift_like_framestack():
    e = make("Paddle-v0", num_actions=6, seed=3)
    assert e.action_space.n == 6 and e.observation_space.shape == (4, 84, 84)
    obs = e.reset()
    assert obs.dtype == np.uint8 and obs.shape == (4, 84, 84) and all(np.array_equal(obs[0], obs[k]) for k in range(4))
    for _ in range(5):
        nxt = e.step(1)[0]
        assert np.array_equal(nxt[:3], obs[1:]) and np.array_equal(nxt[3], e.render())
        obs = nxt


def test_tracking_policy_catches_every_ball_and_random_does_not():
    """the game is solvable and the gap to random is wide; no episode outlasts 38 steps a ball"""
    balls = 5
    rng = np.random.RandomState(0)
    for policy, check in [(track, lambda rets: all(r == balls for r in rets)),
                          (lambda e: rng.randint(6), lambda rets: np.mean(rets) < -2.0)]:
        rets = []
        for ep in range(60):
            e = Paddle(6, balls, seed=ep)
            e.reset()
            done, ret, n = False, 0.0, 0
            while not done:
                _, r, done, _ = e.step(policy(e))
                assert r in (-1.0, 0.0, 1.0)
                ret += r
                n += 1
            assert 25 * balls <= n <= 38 * balls and e.state[STEPS] == n and e.state[RET] == ret
            rets.append(ret)
        assert check(rets), rets
