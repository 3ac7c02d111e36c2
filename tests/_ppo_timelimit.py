"""Inputs of the time-limit step tests (helper of test_ppo_timelimit_cpu.py and
test_ppo_timelimit_gpu.py; numpy and the host envs of reth_amd.envs, nothing runs on a GPU).

A step table is (states [N, k] fp64, actions [T, N]) for one env kind, N envs and a time limit L, T =
L + 3 steps.  A done row is one of three kinds -- terminal only, time limit only (truncated), both
causes on the same step (terminal, NOT truncated) -- and the CartPole tables hold all of them:
  env 0        falls on exactly step L under the constant action 1 (both causes), from an angle found
               by stepping the host env
  env 1, 2     about to fall: terminal on step 1 (with L = 1 that is both causes again)
  the others   small random states: they run into the limit (with L = 1 every step does)
first_episode_kinds counts the kinds over every env's first episode on the host, where the device's
reset draws play no part.

learn / truncated_row_targets run the loop on CartPole-v0 (on a GPU; the test and
scripts/bench_ppo_timelimit.py share them)."""
import functools

import numpy as np

from reth_amd import envs

LIMITS = (1, 5, 7)
SIZES = (1, 9, 64)
KINDS = ("not done", "terminal only", "time limit only", "both")
ABOUT_TO_FALL = {"CartPole-v0": (0.0, 0.0, 0.2, 1.0),      # theta + 0.02 theta_dot past 12 degrees
                 "Acrobot-v1": (2.8, 0.0, 0.0, 0.0),       # both links up: -cos t1 - cos(t1 + t2) > 1
                 "MountainCar-v0": (0.49, 0.05)}           # at the goal on the next step
COLUMNS = {"CartPole-v0": 4, "Acrobot-v1": 4, "MountainCar-v0": 2}
NUM_ACTIONS = {"CartPole-v0": 2, "Acrobot-v1": 3, "MountainCar-v0": 3}


def host_step(env, state, steps, action, limit):
    """one host step from (state, steps of the running episode): (observation, reward, done,
    terminal, state after) -- terminal is the done flag of the same step without a time limit"""
    out = []
    for lim in (limit, 1 << 30):
        h = envs.make_host(env)
        h.max_episode_steps = lim
        h.state, h._t = tuple(float(v) for v in state), int(steps)
        o, r, d, _ = h.step(int(action))
        out.append((np.asarray(o, np.float64), r, bool(d), np.asarray(h.state, np.float64)))
    (o, r, done, after), (_, _, terminal, _) = out
    assert done == (terminal or steps + 1 >= limit)
    return o, r, done, terminal, after


def cartpole_fall_step(theta, give_up, action=1):
    """(the step on which CartPole falls from (0, 0, theta, 0) under a constant action, its margin:
    how far past a threshold the falling step ends up, relative to the threshold); (None, 0) where
    it still stands after `give_up` steps"""
    st = (0.0, 0.0, float(theta), 0.0)
    for t in range(give_up):
        _, _, _, terminal, st = host_step("CartPole-v0", st, t, action, 1 << 30)
        if terminal:
            h = envs.CartPole
            return t + 1, max(abs(st[0]) / h.x_threshold, abs(st[2]) / h.theta_threshold) - 1.0
    return None, 0.0


@functools.lru_cache(maxsize=None)
def falls_on(step):
    """the first angle of a fixed grid from which CartPole falls on exactly `step` under action 1,
    clear of the threshold by 1e-6 of it (the device's fp64 state is within 1e-12 of the host's)"""
    for theta in np.linspace(0.2, -0.209, 410):
        t, margin = cartpole_fall_step(theta, step)
        if t == step and margin > 1e-6:
            return float(theta)
    raise AssertionError(f"no angle of the grid falls on step {step}")


def step_table(env, n, limit, seed=0):
    """(states [n, k], actions [T, n]), T = limit + 3"""
    k, T = COLUMNS[env], limit + 3
    rng = np.random.default_rng(1000 * limit + n + seed)
    if env == "CartPole-v0":
        st = rng.uniform(-0.04, 0.04, (n, k))
    elif env == "Acrobot-v1":
        st = rng.uniform(-1.0, 1.0, (n, k))
    else:
        st = np.stack([rng.uniform(-1.0, 0.3, n), rng.uniform(-0.03, 0.03, n)], 1)
    st[1:3] = ABOUT_TO_FALL[env]
    actions = rng.integers(0, NUM_ACTIONS[env], (T, n))
    if env == "CartPole-v0":
        st[0] = (0.0, 0.0, ABOUT_TO_FALL[env][2], ABOUT_TO_FALL[env][3]) if limit == 1 else (0.0, 0.0, falls_on(limit), 0.0)
        actions[:, 0] = 1
    return st, actions


def first_episode_kinds(env, states, actions, limit):
    """{kind: rows} over every env's first episode, stepped on the host"""
    count = dict.fromkeys(KINDS, 0)
    for i, st in enumerate(states):
        st = tuple(st) + (0.0,) * (4 - len(st)) if env != "MountainCar-v0" else tuple(st)
        for t in range(len(actions)):
            _, _, done, terminal, st = host_step(env, st, t, actions[t, i], limit)
            limited = t + 1 >= limit
            count[KINDS[(1 if terminal else 0) + (2 if limited else 0)]] += 1
            if done:
                break
    return count


# ---------------------------------------------------------------------------- learning (these run on the GPU)
def truncated_row_targets(loop):
    """(mean ret over the last rollout's truncated rows with the bootstrap, without it, their count):
    the rollout stays in the segments after its finish, so it is finished twice more with the current
    value network, once through each entry point.  (nan, nan, 0) where no row is truncated."""
    act, cfg = loop.actors, loop.cfg
    tr = act.seg_trunc.reshape(-1) == 1
    out = []
    for option in (True, False):
        act.fill.fill_(act.cap)
        act.time_limit_bootstrap = option
        (_, _, ret, _, _), n_dev = act.finish_gae(loop.solver, cfg.gamma, cfg.gae_lambda)
        out.append(float(ret[:act.N * act.cap][tr].mean()) if bool(tr.any()) else float('nan'))
    act.time_limit_bootstrap = True
    return out[0], out[1], int(tr.sum())


def learn(option, learning_rate=0.01, seeds=(0, 1, 2)):
    """(trained, untrained, truncated_row_targets per seed -- with the option only)"""
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    trained, untrained, targets = [], [], []
    for seed in seeds:
        cfg = PpoLoopConfig(n_actors=64, horizon=32, gae_lambda=0.95, normalize_adv=True, seed=seed,
                            bootstrap_time_limit=option, learning_rate=learning_rate)
        loop = PpoLoop(cfg, device="cuda", impl="hip")
        untrained.append(loop.rollout_length())
        loop.run(50)
        trained.append(loop.mean_last_length())
        assert int(loop.actors.dropped.sum()) == 0
        if option:
            targets.append(truncated_row_targets(loop))
    return trained, untrained, targets
