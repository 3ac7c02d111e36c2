"""The classic-control family, the parts that need no GPU: the host environments Acrobot and
MountainCar (reth_amd/envs.py, the definitions the device envs of csrc/env_actor.hpp follow), and
the argument checks of rth_env_reset / rth_env_actor_step, which run before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

from reth_amd import _lib
from reth_amd.envs import Acrobot, MountainCar, make

PI = math.pi


# ---------------------------------------------------------------------------- make()
@pytest.mark.parametrize("name,cls,D,limit", [("Acrobot-v1", Acrobot, 6, 500), ("MountainCar-v0", MountainCar, 2, 200)])
def test_make_contract(name, cls, D, limit):
    env = make(name, seed=3)
    assert isinstance(env, cls) and env.max_episode_steps == limit
    assert env.observation_space.shape == (D,) and env.action_space.n == 3
    for _ in range(20):  # the reset range
        obs = env.reset()
        assert isinstance(obs, np.ndarray) and obs.shape == (D,) and obs.dtype == np.float64
        s = np.asarray(env.state, np.float64)
        if cls is Acrobot:
            assert s.shape == (4,) and (s >= -0.1).all() and (s < 0.1).all()
            np.testing.assert_array_equal(obs, [math.cos(s[0]), math.sin(s[0]), math.cos(s[1]), math.sin(s[1]),
                                                s[2], s[3]])
        else:
            assert -0.6 <= s[0] < -0.4 and s[1] == 0.0
            np.testing.assert_array_equal(obs, s)
    env.reset()
    for t in range(1, limit + 1):  # action 1 (no torque / no force) never reaches either goal
        obs, r, done, info = env.step(1)
        assert obs.shape == (D,) and obs.dtype == np.float64 and isinstance(r, float) and isinstance(done, bool)
        assert r == -1.0 and info == {}
        assert done == (t == limit), t
    with pytest.raises(AssertionError):
        env.step(3)


def test_make_names_the_new_envs_in_its_error():
    with pytest.raises(NotImplementedError, match="Acrobot-v1.*MountainCar-v0"):
        make("Pendulum-v0")


def test_same_seed_same_episode():
    for name in ("Acrobot-v1", "MountainCar-v0"):
        a, b = make(name, seed=11), make(name, seed=11)
        np.testing.assert_array_equal(a.reset(), b.reset())
        for t in range(30):
            oa, ob = a.step(t % 3), b.step(t % 3)
            np.testing.assert_array_equal(oa[0], ob[0])
            assert oa[1:] == ob[1:]


# ---------------------------------------------------------------------------- MountainCar
def _mc(p, v, a, t=0):
    env = MountainCar()
    env.state, env._t = (p, v), t
    obs, r, done, _ = env.step(a)
    assert r == -1.0
    return obs[0], obs[1], done


def test_mountaincar_left_wall_zeroes_a_negative_velocity():
    p, v, done = _mc(-1.19, -0.05, 0)
    assert p == -1.2 and v == 0.0 and not done
    p, v, done = _mc(-1.2, 0.0, 2)  # at the wall, pushed right: the slope and the force move it off again
    assert p > -1.2 and v > 0.0


def test_mountaincar_clamps():
    for a in (0, 1, 2):
        assert _mc(0.0, 0.0699, a)[1] <= 0.07 and _mc(0.0, -0.0699, a)[1] >= -0.07
    assert _mc(0.0, 0.5, 2)[1] == 0.07 and _mc(0.0, -0.5, 0)[1] == -0.07
    assert _mc(0.58, 0.07, 2)[0] == 0.6 and _mc(-1.15, -0.07, 0)[0] == -1.2
    rng = np.random.RandomState(0)
    for _ in range(500):
        p, v, _ = _mc(rng.uniform(-1.2, 0.6), rng.uniform(-0.07, 0.07), int(rng.randint(3)))
        assert -1.2 <= p <= 0.6 and -0.07 <= v <= 0.07


def test_mountaincar_done_only_at_the_goal_moving_right():
    assert _mc(0.48, 0.05, 2) [2] is True          # p = 0.53.., v > 0
    assert _mc(0.40, 0.05, 2)[2] is False         # short of the goal
    rng = np.random.RandomState(1)
    seen = 0
    for _ in range(3000):
        p, v, done = _mc(rng.uniform(0.3, 0.6), rng.uniform(-0.07, 0.07), int(rng.randint(3)))
        assert done == (p >= 0.5 and v >= 0.0)
        seen += done
    assert 100 < seen < 2900
    assert _mc(0.55, -0.05, 0)[2] is False        # beyond the goal but moving left


@pytest.mark.parametrize("a", [0, 1, 2])
def test_mountaincar_one_hand_evaluated_step(a):
    v = 0.0 + ((a - 1) * 0.001 + math.cos(3 * -0.5) * (-0.0025))
    assert abs(v) < 0.07
    p = -0.5 + v
    got = _mc(-0.5, 0.0, a)
    assert got == (p, v, False)
    assert abs(v - ((a - 1) * 0.001 - 0.0025 * 0.0707372016677029)) < 1e-15  # cos(-1.5) = 0.07073720166770291


# ---------------------------------------------------------------------------- Acrobot
def _ac(s, a, t=0):
    env = Acrobot()
    env.state, env._t = tuple(s), t
    obs, r, done, _ = env.step(a)
    return np.array(env.state), obs, r, done


def test_acrobot_wraps_both_sides():
    for sign in (1.0, -1.0):
        s, _, _, _ = _ac((sign * 3.1, 0.0, sign * 3.0, 0.0), 1)   # theta1 swings past +-pi
        assert -PI <= s[0] <= PI and s[0] * sign < 0 and abs(s[0]) > 2.0
        s, _, _, _ = _ac((0.0, sign * 3.1, 0.0, sign * 5.0), 1)   # theta2 swings past +-pi
        assert -PI <= s[1] <= PI and s[1] * sign < 0 and abs(s[1]) > 1.5


def test_acrobot_velocity_clamps():
    for sign in (1.0, -1.0):
        s, obs, _, _ = _ac((sign * 0.3, 0.0, sign * 20.0, 0.0), 1)  # injected beyond the bound: still beyond after a step
        assert s[2] == sign * 4 * PI and obs[4] == s[2] and abs(s[3]) < 9 * PI
        s, obs, _, _ = _ac((0.0, 0.0, 0.0, sign * (9 * PI - 0.01)), 1)  # just inside, accelerated across
        assert s[3] == sign * 9 * PI and obs[5] == s[3] and abs(s[2]) < 4 * PI
    rng = np.random.RandomState(2)
    for _ in range(300):
        s0 = (rng.uniform(-PI, PI), rng.uniform(-PI, PI), rng.uniform(-4 * PI, 4 * PI), rng.uniform(-9 * PI, 9 * PI))
        s, _, _, _ = _ac(s0, int(rng.randint(3)))
        assert abs(s[0]) <= PI and abs(s[1]) <= PI and abs(s[2]) <= 4 * PI and abs(s[3]) <= 9 * PI


def test_acrobot_terminal_step_gives_reward_zero_and_done():
    s, obs, r, done = _ac((PI - 0.1, 0.0, 0.0, 0.0), 1)  # nearly upright: height 2 cos(0.1) > 1
    assert -math.cos(s[0]) - math.cos(s[0] + s[1]) > 1.0
    assert r == 0.0 and done is True
    s, obs, r, done = _ac((0.1, 0.0, 0.0, 0.0), 1)       # hanging
    assert r == -1.0 and done is False
    s, obs, r, done = _ac((0.1, 0.0, 0.0, 0.0), 1, t=499)  # the time limit ends the episode, reward stays -1
    assert r == -1.0 and done is True


def test_acrobot_mirror_symmetry():
    rng = np.random.RandomState(3)
    worst = 0.0
    for _ in range(200):
        s0 = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-6, 6), rng.uniform(-12, 12)])
        a = int(rng.randint(3))
        s, _, r, d = _ac(s0, a)
        m, _, rm, dm = _ac(-s0, 2 - a)
        if min(PI - abs(s[0]), PI - abs(s[1])) < 1e-9:  # a wrap edge: the mirror image may wrap the other way
            continue
        worst = max(worst, float(np.abs(s + m).max()))
        height = -math.cos(s[0]) - math.cos(s[0] + s[1])
        if abs(height - 1.0) > 1e-9:
            assert (r, d) == (rm, dm)
    assert worst <= 1e-12, worst


def test_acrobot_rest_state_stays_at_rest():
    env = Acrobot()
    env.state = (0.0, 0.0, 0.0, 0.0)
    for _ in range(50):
        obs, r, done, _ = env.step(1)
        assert np.abs(np.array(env.state)).max() <= 1e-12 and r == -1.0 and not done
    np.testing.assert_allclose(obs, [1, 0, 1, 0, 0, 0], atol=1e-12)


# ---------------------------------------------------------------------------- entry points
FAKE = 0x1000  # a non-NULL "device pointer": no check dereferences it, and nothing is launched
SHAPES = {_lib.ENV_CARTPOLE: (4, 2), _lib.ENV_ACROBOT: (6, 3), _lib.ENV_MOUNTAINCAR: (2, 3)}


def _args(**over):
    params = (_lib.c_vp * 6)(*[FAKE] * 6)
    kw = dict(params=params, env=_lib.ENV_ACROBOT, H=128, seed=1, N=8, ring=8, max_episode_steps=500)
    for name, typ in _lib.EnvActorArgs._fields_:
        if typ is _lib.c_vp:
            kw[name] = FAKE
    kw["action_in"] = kw["q_out"] = None  # the nullable ones
    kw.update(over)
    if kw["env"] in SHAPES:
        kw.setdefault("D", SHAPES[kw["env"]][0])
        kw.setdefault("A", SHAPES[kw["env"]][1])
    else:
        kw.setdefault("D", 4)
        kw.setdefault("A", 2)
    a = _lib.EnvActorArgs(**kw)
    a._keep = params
    return a


class _FakeNStep(ctypes.Structure):
    """the leading fields of the library's rth_nstep (N, n): only read by the checks"""
    _fields_ = [("N", ctypes.c_int64), ("n", ctypes.c_int32), ("gamma", ctypes.c_double), ("mode", ctypes.c_int32),
                ("device", ctypes.c_int), ("mem", ctypes.c_void_p), ("st", ctypes.c_void_p * 6)]


def _step(args, N=8, n=1, handle=True):
    h = _FakeNStep(N, n, 0.99, 0, 0, None)
    lib = _lib.lib()
    rc = lib.rth_env_actor_step(ctypes.addressof(h) if handle else None, ctypes.byref(args), None)
    return rc, lib.rth_last_error()


def _reset(args):
    lib = _lib.lib()
    return lib.rth_env_reset(ctypes.byref(args), None), lib.rth_last_error()


BAD_ENV = [dict(env=3), dict(env=-1), dict(env=1 << 40)]
# the shape of another env, of no env, and shapes the MLP kernels do not build
BAD_SHAPES = [dict(env=_lib.ENV_ACROBOT, D=4, A=2), dict(env=_lib.ENV_ACROBOT, D=2, A=3),
              dict(env=_lib.ENV_MOUNTAINCAR, D=6, A=3), dict(env=_lib.ENV_MOUNTAINCAR, D=4, A=2),
              dict(env=_lib.ENV_CARTPOLE, D=6, A=3), dict(env=_lib.ENV_CARTPOLE, D=2, A=3),
              dict(D=5), dict(D=8), dict(A=2), dict(A=4), dict(H=64), dict(D=0), dict(A=19)]
BAD_COMMON = [dict(N=0), dict(N=-1), dict(N=1 << 31), dict(ring=3), dict(ring=0), dict(max_episode_steps=0),
              dict(max_episode_steps=-5), dict(obs_ring=FAKE + 8)]
STATE_PTRS = ["state", "ep_steps", "t_dev", "stats", "ret_stats", "obs_ring", "cur_slot"]
STEP_PTRS = ["eps", "action", "reward", "done", "s0_h", "s1_h", "emit", "row_s0", "row_a", "row_s1", "row_r",
             "row_done", "row_obs0", "row_obs1"]


@pytest.mark.parametrize("over", BAD_ENV + BAD_SHAPES + BAD_COMMON + [{p: None} for p in STATE_PTRS])
def test_reset_rejects(over):
    rc, msg = _reset(_args(**over))
    assert rc != 0 and b"rth_env_reset" in msg, (over, msg)


@pytest.mark.parametrize("over", BAD_ENV + BAD_SHAPES + BAD_COMMON + [dict(row_obs0=FAKE + 8), dict(row_obs1=FAKE + 4)]
                         + [{p: None} for p in STATE_PTRS + STEP_PTRS + ["params"]])
def test_step_rejects(over):
    rc, msg = _step(_args(**over))
    assert rc != 0 and b"rth_env_actor_step" in msg, (over, msg)


def test_unknown_env_and_wrong_shape_are_named():
    assert b"env id" in _reset(_args(env=7))[1]
    assert b"shape" in _step(_args(env=_lib.ENV_MOUNTAINCAR, D=6, A=3))[1]


def test_step_rejects_adder_mismatch_and_null():
    rc, msg = _step(_args(N=8), N=9)
    assert rc != 0 and b"rth_env_actor_step" in msg and b"adder" in msg
    rc, msg = _step(_args(), handle=False)
    assert rc != 0 and b"rth_env_actor_step" in msg
    rc, msg = _step(_args(ring=8), n=3)  # an emitted row's observations would be overwritten: ring < 2 (n + 2)
    assert rc != 0 and b"rth_env_actor_step" in msg and b"ring" in msg
    lib = _lib.lib()
    assert lib.rth_env_actor_step(None, None, None) != 0 and b"rth_env_actor_step" in lib.rth_last_error()
    assert lib.rth_env_reset(None, None) != 0 and b"rth_env_reset" in lib.rth_last_error()


def test_step_rejects_null_parameter():
    params = (_lib.c_vp * 6)(*([FAKE] * 5 + [None]))
    rc, msg = _step(_args(params=params))
    assert rc != 0 and b"rth_env_actor_step" in msg


def test_struct_layout_matches_header():
    """rth_mlp_actor_args (232 bytes, unchanged) plus the env id and the return statistics: 28
    pointers / int64 fields of 8 bytes, the seed, N and two int32"""
    assert ctypes.sizeof(_lib.MlpActorArgs) == 232
    assert ctypes.sizeof(_lib.EnvActorArgs) == 8 * 28 + 8 + 8 + 4 + 4 == 248
    names = [n for n, _ in _lib.EnvActorArgs._fields_]
    assert names[:5] == ["params", "env", "D", "H", "A"] and names[-4:] == ["seed", "N", "ring", "max_episode_steps"]


def test_modules_import_without_gpu():
    from reth_amd import mlp_actors, mlp_apex

    assert issubclass(mlp_actors.VecCartPoleActors, mlp_actors.VecMlpActors) and mlp_apex.MlpApexDQN
    assert mlp_apex.MlpApexConfig().env == "CartPole-v0"
    assert {k: v[1:] for k, v in mlp_actors.ENVS.items()} == {
        "CartPole-v0": (4, 2, 200), "CartPole-v1": (4, 2, 500), "Acrobot-v1": (6, 3, 500),
        "MountainCar-v0": (2, 3, 200)}
