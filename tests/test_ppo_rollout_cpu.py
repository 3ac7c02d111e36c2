"""ppo_actors.HostRollout -- the numpy statement of the device rollout's store, finish and carry
(csrc/ppo_actor.hpp), the oracle of tests/test_ppo_actors_gpu.py -- against the reference's
episode-buffer / data-buffer logic as examples/cartpole_ppo_hip.py runs it, and its returns against
reth_amd.ppo.calculate_discount_rewards_with_dones.  No GPU."""
import numpy as np
import pytest

from reth_amd.host_buffer import HostNumpyBuffer
from reth_amd.ppo import calculate_discount_rewards_with_dones
from reth_amd.ppo_actors import HostRollout, episode_returns

GAMMA = 0.99
RET_TOL = 1e-5  # absolute, on normalised returns (unit variance): see test_returns_match_the_reference


def example_loop(stream, interval):
    """examples/cartpole_ppo_hip.py:47-61 on a scripted stream of (s0, a, r, logp, done): the batch
    of every update (complete episodes only; the running episode's rows stay in the episode buffer)"""
    episode_buffer = HostNumpyBuffer(4096, circular=False)
    data_buffer = HostNumpyBuffer(4096, circular=False)
    batches = []
    for k, (s0, a, r, logp, done) in enumerate(stream):
        episode_buffer.append((s0, a, r, logp, done))
        if done:
            s, act, rew, lp, dn = (c.copy() for c in episode_buffer.data)
            rew = calculate_discount_rewards_with_dones(rew, dn, GAMMA)
            data_buffer.append_batch((s, act, rew, lp))
            episode_buffer.clear()
        if (k + 1) % interval == 0:
            batches.append([c.copy() for c in data_buffer.data] if data_buffer.size else None)
            data_buffer.clear()
    return batches


def scripted_stream(rewards, rng):
    """60 steps: episodes of 1, 2 and 7 steps, one of 25 that straddles the update at step 30, one
    of 20, and 5 steps of an episode still running at the end"""
    ends = np.cumsum([1, 2, 7, 25, 20]) - 1
    out = []
    for k in range(60):
        r = np.float32(rng.choice([-1.0, 1.0]) if rewards == "pm1" else rng.standard_normal())
        out.append((rng.standard_normal(4).astype(np.float32), np.int64(rng.integers(0, 2)), r,
                    np.float32(-rng.random()), bool(k in ends)))
    return out


@pytest.mark.parametrize("rewards", ["pm1", "normal"])
def test_host_rollout_reproduces_the_examples_buffers(rewards):
    rng = np.random.default_rng(3)
    stream = scripted_stream(rewards, rng)
    want = example_loop(stream, 30)
    roll = HostRollout(1, 64, 4)
    got = []
    for k, (s0, a, r, logp, done) in enumerate(stream):
        roll.store(s0[None], [a], [r], [done], [logp])
        if (k + 1) % 30 == 0:
            got.append(roll.finish(GAMMA))
    assert [len(b[1]) for b in want] == [10, 45] and [g[4] for g in got] == [10, 45]
    assert int(roll.fill[0]) == 5 and int(roll.complete[0]) == 0 and int(roll.dropped[0]) == 0
    for (ws, wa, wret, wlp), (s, a, ret, lp, n) in zip(want, got):
        assert s.tobytes() == ws.tobytes() and a.tobytes() == wa.astype(np.int64).tobytes()
        assert lp.tobytes() == wlp.tobytes()
        err = float(np.abs(ret.astype(np.float64) - wret.astype(np.float64)).max())
        print(f"{rewards}: n = {n}, max |ret - reference| = {err:.3e}")
        assert err <= RET_TOL
    # the second batch opens with the 25-step episode: 20 carried rows with their first-rollout
    # log-probabilities, then its 5 rows of the second rollout
    assert got[1][3][:25].tobytes() == np.array([x[3] for x in stream[10:35]], np.float32).tobytes()


def test_returns_match_the_reference():
    """The fp64 form (ppo_actors.episode_returns: what the kernel computes) against the reference's
    fp32 function over episode lengths 1..500 with rewards +1, -1 and N(0, 1), the last row done.
    Measured with these draws: max |difference| 2.7e-6 (normal rewards, L = 164; 2.4e-6 at L = 186
    was measured with other draws when the bound was set); the bound of 1e-5 absolute is about four
    times that.  Normalised returns have unit variance, so an absolute bound is a relative one."""
    rng = np.random.default_rng(0)
    worst = (0.0, None)
    for L in range(1, 501):
        done = np.zeros(L, bool)
        done[-1] = True
        for kind in ("+1", "-1", "normal"):
            r = {"+1": np.ones(L), "-1": -np.ones(L), "normal": rng.standard_normal(L)}[kind].astype(np.float32)
            want = calculate_discount_rewards_with_dones(r, done, GAMMA)
            got = episode_returns(r, done, GAMMA)
            assert got.dtype == np.float32 and np.isfinite(got).all()
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            if err > worst[0]:
                worst = (err, (L, kind))
    print(f"max |fp64 form - reference| = {worst[0]:.3e} at (L, rewards) = {worst[1]}")
    assert worst[0] <= RET_TOL


def test_an_episode_of_one_step_returns_zero():
    assert episode_returns([1.0], [True], GAMMA).tolist() == [0.0]
    assert episode_returns([-3.5], [True], GAMMA).tolist() == [0.0]
    roll = HostRollout(1, 4, 2)
    roll.store(np.ones((1, 2)), [1], [1.0], [True], [-0.5])
    s, a, ret, lp, n = roll.finish(GAMMA)
    assert n == 1 and ret.tolist() == [0.0] and lp.tolist() == [-0.5] and int(roll.fill[0]) == 0


def test_the_carry_keeps_old_logprobs_and_rows():
    roll = HostRollout(2, 8, 1)
    # env 0: an episode of 2, then 3 rows of a running one; env 1: 5 rows, no done
    dones = [[0, 0], [1, 0], [0, 0], [0, 0], [0, 0]]
    for t, d in enumerate(dones):
        roll.store([[10.0 + t], [20.0 + t]], [t, t + 5], [1.0, 1.0], d, [-0.1 * t, -1.0 - 0.1 * t])
    s, a, ret, lp, n = roll.finish(GAMMA)
    assert n == 2 and s[:, 0].tolist() == [10.0, 11.0] and a.tolist() == [0, 1]
    assert roll.fill.tolist() == [3, 5] and roll.complete.tolist() == [0, 0]
    assert roll.seg_s[0, :3, 0].tolist() == [12.0, 13.0, 14.0] and roll.seg_a[1, :5].tolist() == [5, 6, 7, 8, 9]
    assert roll.seg_logp[0, :3].tobytes() == np.array([-0.2, -0.3, -0.4], np.float32).tobytes()
    # both episodes end: the batch is env-major, then time
    roll.store([[15.0], [25.0]], [9, 9], [1.0, 1.0], [1, 1], [-7.0, -8.0])
    s, a, ret, lp, n = roll.finish(GAMMA)
    assert n == 10 and s[:, 0].tolist() == [12.0, 13.0, 14.0, 15.0, 20.0, 21.0, 22.0, 23.0, 24.0, 25.0]
    assert lp[:4].tobytes() == np.array([-0.2, -0.3, -0.4, -7.0], np.float32).tobytes()
    assert roll.fill.tolist() == [0, 0]


def test_envs_and_loop_defaults():
    """the env table is the classic-control actors' at PPO's shapes, and the loop's defaults are the
    reference's examples/ppo values: 10 x 200 = UPDATE_INTERVAL"""
    from reth_amd import _lib, mlp_actors
    from reth_amd.ppo_actors import ENVS
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    assert ENVS == {"CartPole-v0": (_lib.ENV_CARTPOLE, 4, 2, 200), "Acrobot-v1": (_lib.ENV_ACROBOT, 6, 3, 500),
                    "MountainCar-v0": (_lib.ENV_MOUNTAINCAR, 2, 3, 200)}
    assert all(mlp_actors.ENVS[k] == v for k, v in ENVS.items())
    c = PpoLoopConfig()
    assert (c.env, c.n_actors, c.horizon, c.gamma, c.k_epochs, c.eps_clip, c.learning_rate, c.max_episode_steps,
            c.seed) == ("CartPole-v0", 10, 200, 0.99, 4, 0.2, 0.01, None, 0)
    assert c.n_actors * c.horizon == 2000
    for name in ("iteration", "run", "graph_ready", "capture", "mean_last_length", "rollout_length"):
        assert callable(getattr(PpoLoop, name))
    with pytest.raises(ValueError, match="horizon 100 < max_episode_steps 200"):
        PpoLoop(PpoLoopConfig(horizon=100), device="cpu")  # refused before anything touches a device
    with pytest.raises(ValueError, match="the device envs are"):
        PpoLoop(PpoLoopConfig(env="Pendulum-v0"), device="cpu")


def test_cap_is_never_exceeded_when_horizon_covers_an_episode():
    """cap = horizon + limit - 1 with horizon >= limit: 1,000 random steps (done with probability
    0.1, a time limit of 8) in rollouts of `horizon` steps drop nothing, and every finish leaves
    fewer than `limit` rows behind"""
    limit, horizon, N = 8, 8, 3
    roll = HostRollout(N, horizon + limit - 1, 1)
    rng = np.random.default_rng(5)
    steps = np.zeros(N, int)
    for k in range(1000):
        steps += 1
        done = (rng.random(N) < 0.1) | (steps >= limit)
        roll.store(np.zeros((N, 1)), np.zeros(N), np.ones(N), done, np.zeros(N))
        steps[done] = 0
        assert (roll.fill <= roll.cap).all()
        if (k + 1) % horizon == 0:
            n = roll.finish(GAMMA)[4]
            assert n >= N and (roll.fill < limit).all()
    assert int(roll.dropped.sum()) == 0
