"""DDPG (reth_amd/ddpg.py, csrc/ddpg.hpp), the parts that need no GPU: the C ABI's shape
pre-checks, the seeded initialisation and the torch path against the reference's recorded run
(tests/golden/ddpg_pendulum_b64.npz, written by tests/golden/make_golden_ddpg.py), the action-cast
switch, the Pendulum environment, OU noise and the Worker / YAML plumbing of the example."""
import hashlib
import io
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from reth_amd import _lib, envs, presets
from reth_amd.ddpg import Actor, Critic, DDPGSolver, generate_ddpg_model
from reth_amd.noise import OUNoise, OUNoiseExploration
from reth_amd.solver import Box, get_solver

CONFIG = os.path.join(ROOT, "examples", "pendulum_ddpg.yaml")
NAMES = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
OBS, ACT = Box(-1, 1, (3,)), Box(-2, 2, (1,))
BAD_SHAPES = [(0, 1, 400, 300), (65, 1, 400, 300), (3, 0, 400, 300), (3, 9, 400, 300), (3, 1, 0, 300),
              (3, 1, 402, 300), (3, 1, 516, 300), (3, 1, 400, 0), (3, 1, 400, 301), (3, 1, 400, 1000)]


# ------------------------------------------------------------------ ABI shape checks
def test_supported_shapes():
    lib = _lib.lib()
    for shape in [(3, 1, 400, 300), (1, 1, 4, 4), (64, 8, 512, 512), (7, 2, 36, 20), (17, 6, 64, 128)]:
        assert lib.rth_ddpg_supported(*shape) == 1, shape
    for shape in BAD_SHAPES:
        assert lib.rth_ddpg_supported(*shape) == 0, shape


def test_workspace_size():
    lib = _lib.lib()
    prev = 0
    for B in [1, 2, 5, 64, 67, 130, 257, 4096]:
        for shape in [(1, 1, 4, 4), (64, 8, 512, 512)]:
            assert lib.rth_ddpg_workspace(B, *shape) > 0
        size = lib.rth_ddpg_workspace(B, 3, 1, 400, 300)
        # the actions, the loss elements and every activation / pre-activation gradient of a row
        assert size % 16 == 0 and size >= prev and size >= 4 * B * (1 + 1 + 1 + 401 + 300 + 400 + 300)
        prev = size
    for shape in BAD_SHAPES:
        assert lib.rth_ddpg_workspace(64, *shape) <= 0, shape
        err = lib.rth_last_error()
        assert b"rth_ddpg_workspace" in err and b"1..64" in err and b"1..8" in err and b"4..512" in err
    assert lib.rth_ddpg_workspace(0, 3, 1, 400, 300) <= 0


# ------------------------------------------------------------------ init and the torch path vs the golden
def _sha1(t):
    return hashlib.sha1(np.ascontiguousarray(t.detach().numpy()).tobytes()).hexdigest().encode()


def test_seeded_init_is_the_references(golden):
    g = golden("ddpg_pendulum_b64.npz")
    torch.manual_seed(int(g["seed"]))
    models = generate_ddpg_model(OBS, ACT, 1e-4, 1e-3)
    for net in ("actor", "actor_target", "critic", "critic_target"):
        assert [n for n, _ in models[net].named_parameters()] == NAMES
        assert all(a is b for a, b in zip(models[net]._params6(), models[net].parameters()))
        for k, v in models[net].state_dict().items():
            assert _sha1(v) == bytes(g[f"init/{net}/{k}"]), (net, k)
    assert models["actor"].dims() == models["critic"].dims() == (3, 1, 400, 300)
    assert tuple(models["critic"].fc2.weight.shape) == (300, 401)
    # the solver draws the same networks and then makes the targets copies of the online pair
    torch.manual_seed(int(g["seed"]))
    s = DDPGSolver(OBS, ACT, device="cpu")
    for k, v in s.actor.state_dict().items():
        assert _sha1(v) == bytes(g[f"init/actor/{k}"])
        assert torch.equal(v, s.actor_target.state_dict()[k])
    for k, v in s.critic.state_dict().items():
        assert _sha1(v) == bytes(g[f"init/critic/{k}"])
        assert torch.equal(v, s.critic_target.state_dict()[k])


def _golden_solver(g, **kw):
    torch.manual_seed(int(g["seed"]))
    return DDPGSolver(OBS, ACT, device="cpu", **kw)


def check_against_golden(solver, g, rtol=1e-5, atol=1e-6):
    """three updates, act and the final parameters of `solver` against the fixture (shared with
    the GPU tests)"""
    batch = [g["s0"], g["a"], g["r"], g["s1"], g["done"]]
    for k in range(3):
        td = solver.update(batch, weights=g["w"])
        assert td.shape == (64,) and td.dtype == torch.float32 and td.device.type == "cpu"
        err = np.abs(td.numpy() - g[f"upd{k}_abs_td"]).max()
        print(f"update {k}: max |td - golden| {err:.3e} (|td| up to {g[f'upd{k}_abs_td'].max():.2f})")
        np.testing.assert_allclose(td.numpy(), g[f"upd{k}_abs_td"], rtol=rtol, atol=atol)
    acts = np.stack([solver.act(s) for s in g["act_states"]])
    assert acts.shape == (4, 1) and acts.dtype == np.float32
    np.testing.assert_allclose(acts, g["act"], rtol=rtol, atol=atol)
    for net in ("actor", "critic"):
        for k, v in getattr(solver, net).state_dict().items():
            err = np.abs(v.cpu().numpy() - g[f"final/{net}/{k}"]).max()
            print(f"final {net}.{k}: max difference {err:.3e}")
            np.testing.assert_allclose(v.cpu().numpy(), g[f"final/{net}/{k}"], rtol=rtol, atol=atol)
    for net in ("actor_target", "critic_target"):
        for k, v in getattr(solver, net).state_dict().items():
            ref = float(g[f"tsum/{net}/{k}"])
            assert abs(float(v.double().sum()) - ref) <= 1e-5 * max(1.0, abs(ref)) + 1e-6 * v.numel(), (net, k)


def test_torch_path_reproduces_the_golden(golden):
    g = golden("ddpg_pendulum_b64.npz")
    solver = _golden_solver(g)
    assert solver.impl_active == "torch" and solver.device.type == "cpu"
    assert float(g["done"].sum()) >= 1 and abs(g["a"]).max() > 1  # terminal rows; actions the cast changes
    check_against_golden(solver, g)
    assert solver.hip_launches == 0


def test_action_cast(golden):
    g = golden("ddpg_pendulum_b64.npz")
    batch = [g["s0"], g["a"], g["r"], g["s1"], g["done"]]
    cast, raw = _golden_solver(g), _golden_solver(g, cast_actions_to_long=False)
    assert cast.cast_actions_to_long and not raw.cast_actions_to_long
    td_cast, td_raw = cast.calc_loss(batch), raw.calc_loss(batch)
    td0 = cast.update(batch, weights=g["w"])
    np.testing.assert_allclose(td0.numpy(), g["upd0_abs_td"], rtol=1e-5, atol=1e-6)
    assert torch.equal(td_cast, td0)  # calc_loss is the update's |td|
    assert float((td_cast - td_raw).abs().max()) > 1e-4
    # the cast is truncation toward zero
    trunc = _golden_solver(g, cast_actions_to_long=False)
    assert torch.equal(trunc.calc_loss([g["s0"], np.trunc(g["a"]), g["r"], g["s1"], g["done"]]), td_cast)


def test_get_solver_and_explicit_hip_on_cpu():
    s = get_solver("ddpg", observation_space=OBS, action_space=ACT, device="cpu")
    assert isinstance(s, DDPGSolver) and s.impl_active == "torch"
    assert (s.gamma, s.tau) == (0.99, 0.001)
    assert s.actor_optimizer.param_groups[0]["lr"] == 1e-4 and s.critic_optimizer.param_groups[0]["lr"] == 1e-3
    assert type(s.actor_optimizer) is torch.optim.Adam and type(s.critic_optimizer) is torch.optim.Adam
    with pytest.raises(ValueError, match="not a GPU"):
        DDPGSolver(OBS, ACT, device="cpu", impl="hip")
    with pytest.raises(NotImplementedError):
        DDPGSolver(Box(0, 255, (4, 84, 84)), ACT, device="cpu")
    with pytest.raises(NotImplementedError):
        DDPGSolver(OBS, ACT, device="cpu", is_image=True)
    with pytest.raises(NotImplementedError, match="ddpg"):
        get_solver("ppo")


def test_weights_stream_is_the_actors_state_dict():
    torch.manual_seed(3)
    a, b = DDPGSolver(OBS, ACT, device="cpu"), DDPGSolver(OBS, ACT, device="cpu")
    stream = a.save_weights()
    states = torch.load(io.BytesIO(stream.getvalue()), weights_only=True)
    assert list(states) == NAMES
    stream.seek(0)
    b.load_weights(stream)
    for k in NAMES:
        assert torch.equal(b.actor.state_dict()[k], a.actor.state_dict()[k])
        assert torch.equal(b.actor_target.state_dict()[k], a.actor.state_dict()[k])
    x = np.array([0.6, -0.8, 0.3])
    assert np.array_equal(a.act(x), b.act(x)) and a.act(x).shape == (1,)


def test_compat_reexports():
    import sys

    compat = os.path.join(ROOT, "reth_amd", "compat")
    sys.path.insert(0, compat)
    try:
        from reth.algorithm import DDPGSolver as D2
        from reth.utils import OUNoise as N2, OUNoiseExploration as E2
    finally:
        sys.path.remove(compat)
    assert D2 is DDPGSolver and N2 is OUNoise and E2 is OUNoiseExploration


# ------------------------------------------------------------------ Pendulum
def test_pendulum_is_resolved_by_make_host_not_by_make():
    """make() keeps the envs of the DQN loops (discrete actions); the host-only Pendulum-v0 comes
    from make_host, which is what the YAML factories and the compat `reth.env.make` call"""
    import sys

    with pytest.raises(NotImplementedError):
        envs.make("Pendulum-v0")
    assert type(envs.make_host("Pendulum-v0", seed=1)) is envs.Pendulum
    assert type(envs.make_host("CartPole-v0")) is envs.CartPole
    with pytest.raises(NotImplementedError):
        envs.make_host("LunarLander-v2")
    assert type(presets.get_env({"env": {"name": "Pendulum-v0"}})) is envs.Pendulum
    compat = os.path.join(ROOT, "reth_amd", "compat")
    sys.path.insert(0, compat)
    try:
        from reth.env import make as compat_make
    finally:
        sys.path.remove(compat)
    assert compat_make is envs.make_host


def test_pendulum_one_hand_computed_step():
    env = envs.make_host("Pendulum-v0", seed=0)
    assert type(env) is envs.Pendulum and env.max_episode_steps == 200
    assert env.observation_space.shape == (3,) and env.action_space.shape == (1,)
    assert float(env.action_space.low) == -2.0 and float(env.action_space.high) == 2.0
    env.reset()
    th, thdot, u = 0.5, -1.0, 1.5
    env.state = (th, thdot)
    obs, r, done, info = env.step(np.array([u]))
    # g = 10, m = l = 1, dt = 0.05: thdot' = thdot + (-15 sin(th + pi) + 3 u) dt; th' = th + thdot' dt
    nthdot = thdot + (-15.0 * math.sin(th + math.pi) + 3.0 * u) * 0.05
    nth = th + nthdot * 0.05
    assert abs(nthdot - (-0.415431)) < 1e-6 and abs(nth - 0.479228) < 1e-6  # by hand
    np.testing.assert_allclose(obs, [math.cos(nth), math.sin(nth), nthdot], rtol=0, atol=1e-15)
    assert abs(r + (0.5 ** 2 + 0.1 * 1.0 + 0.001 * 2.25)) < 1e-15  # the cost of the state before the step
    assert done is False and info == {} and isinstance(r, float) and obs.dtype == np.float64


def test_pendulum_clips_and_limits():
    env = envs.make_host("Pendulum-v0", seed=1)
    env.reset()
    env.state = (0.0, 0.0)
    o_big, r_big, _, _ = env.step(np.array([50.0]))
    env.state = (0.0, 0.0)
    o_two, r_two, _, _ = env.step(np.array([2.0]))
    assert np.array_equal(o_big, o_two) and r_big == r_two == -0.004  # torque clipped to 2
    # the speed is clipped to 8 AFTER the angle has moved with the unclipped speed
    env.state = (math.pi / 2, 7.9)
    obs, _, _, _ = env.step(np.array([2.0]))
    raw = 7.9 + (-15.0 * math.sin(math.pi / 2 + math.pi) + 6.0) * 0.05
    assert raw > 8.0 and obs[2] == 8.0 and env.state[1] == 8.0
    assert abs(env.state[0] - (math.pi / 2 + raw * 0.05)) < 1e-15
    env.state = (-math.pi / 2, -7.9)
    assert env.step(np.array([-2.0]))[0][2] == -8.0
    # angle_normalize: 2 pi + 0.25 costs what 0.25 costs
    env.state = (2 * math.pi + 0.25, 0.0)
    assert abs(env.step(np.array([0.0]))[1] + 0.0625) < 1e-12
    # observations stay inside their bounds; the only episode end is the 200-step limit
    env.reset()
    rng = np.random.RandomState(0)
    for t in range(1, 201):
        obs, r, done, _ = env.step(rng.uniform(-3, 3, 1))
        assert abs(obs[0]) <= 1 and abs(obs[1]) <= 1 and abs(obs[2]) <= 8 and r <= 0
        assert done == (t == 200), t


def test_pendulum_seeded_reset():
    a, b, c = (envs.make_host("Pendulum-v0", seed=s) for s in (5, 5, 6))
    oa, ob, oc = a.reset(), b.reset(), c.reset()
    assert np.array_equal(oa, ob) and not np.array_equal(oa, oc)
    assert -math.pi <= a.state[0] <= math.pi and -1 <= a.state[1] <= 1
    assert abs(oa[0] ** 2 + oa[1] ** 2 - 1) < 1e-12 and oa[2] == a.state[1]
    for _ in range(5):
        assert np.array_equal(a.step(np.array([0.7]))[0], b.step(np.array([0.7]))[0])
    assert np.array_equal(a.reset(), b.reset())


# ------------------------------------------------------------------ noise and Worker
def test_ounoise_recurrence():
    np.random.seed(11)
    n = OUNoise(3, mu=0.1, theta=0.15, sigma=0.2)
    assert np.array_equal(n.state, np.full(3, 0.1))
    got = [n.noise().copy() for _ in range(5)]
    np.random.seed(11)
    x = np.ones(3) * 0.1
    for k in range(5):
        dx = 0.15 * (0.1 - x) + 0.2 * np.random.randn(3)
        x = x + dx
        assert np.array_equal(got[k], x), k
    n.reset()
    assert np.array_equal(n.state, np.full(3, 0.1))


class _FixedSolver:
    device = "cpu"

    def act(self, state):
        return np.array([0.25], dtype=np.float32)


def test_ounoise_exploration_adds_scheduled_noise():
    np.random.seed(2)
    ref = OUNoise(1)
    noises = [ref.noise().copy() for _ in range(6)]
    np.random.seed(2)
    e = OUNoiseExploration(_FixedSolver(), ACT, epsilon="1,0,4")
    for k, eps in enumerate([0.75, 0.5, 0.25, 0.0, 0.0, 0.0]):  # the schedule steps before it is read
        a = e.act(None)
        assert a.dtype == np.float32 and a.shape == (1,) and e.schedule.value() == eps
        want = np.array([0.25], dtype=np.float32)
        want += eps * noises[k]
        assert np.array_equal(a, want), k
    assert abs(noises[0][0]) > 0.01 and a[0] == np.float32(0.25)  # no clip; eps = 0: the solver's action


def test_worker_ounoise_dict_steps_pendulum_and_resets_noise():
    env = envs.make_host("Pendulum-v0", seed=0)
    np.random.seed(0)
    w = presets.Worker(env, _FixedSolver(), logger=False, print_interval=None,
                       exploration={"name": "ounoise", "epsilon": 1, "sigma": 0.3})
    assert isinstance(w.exploration, OUNoiseExploration) and w.exploration.noise.sigma == 0.3
    assert w.exploration.reset in w.on_episode_end
    for t in range(1, 200):
        s0, a, r, s1, done = w.step()
        assert not done and a.shape == (1,) and s1.shape == (3,)
    assert float(abs(w.exploration.noise.state[0])) > 0
    assert w.step()[4] is True  # step 200: the episode ends and the noise starts over
    assert np.array_equal(w.exploration.noise.state, np.zeros(1)) and w.cur_episode == 2
    # the other forms behave as before
    w2 = presets.Worker(env, _FixedSolver(), logger=False, print_interval=None,
                        exploration={"name": "random", "epsilon": 0})
    assert type(w2.exploration) is presets.RandomExploration and w2.on_episode_end == []
    assert type(presets.Worker(env, _FixedSolver(), logger=False, exploration="1,0.1,100").exploration) \
        is presets.RandomExploration
    obj = OUNoiseExploration(_FixedSolver(), ACT, epsilon=1)
    assert presets.Worker(env, _FixedSolver(), logger=False, exploration=obj).exploration is obj
    assert presets.Worker(env, _FixedSolver(), logger=False).exploration is None
    with pytest.raises(ValueError, match="Invalid exploration name"):
        presets.Worker(env, _FixedSolver(), logger=False, exploration={"name": "boltzmann"})


def test_yaml_factories_load_the_example_config(monkeypatch):
    cfg = presets._parse_input(CONFIG)
    assert cfg["solver"] == {"name": "ddpg", "gamma": 0.99, "tau": 0.001, "learning_rate_actor": 0.0001,
                             "learning_rate_critic": 0.001}
    env = presets.get_env(CONFIG, seed=0)
    assert type(env) is envs.Pendulum
    solver = presets.get_solver(CONFIG, env=env, device="cpu")
    assert isinstance(solver, DDPGSolver) and solver.impl_active == "torch" and solver.actor.dims() == (3, 1, 400, 300)
    worker = presets.get_worker(CONFIG, solver=solver, env=env, logger=False)
    assert isinstance(worker.exploration, OUNoiseExploration)
    sch = worker.exploration.schedule
    assert (sch.value(), sch.end, sch.max_steps) == (1.0, 0.01, 30000)
    trainer = presets.get_trainer(CONFIG, solver=solver, logger=False)
    assert trainer.solver is solver and trainer.on_step_end[0].interval == 100
    # (the device buffer itself needs a GPU: the arguments it is built from)
    seen = {}
    monkeypatch.setattr(presets, "PrioritizedBuffer", lambda **kw: seen.update(kw) or "buffer")
    assert presets.get_replay_buffer(CONFIG) == "buffer"
    assert seen == {"beta": "0.4,1,100000", "alpha": 0.6, "capacity": 100000}
    # the worker's transitions feed an update of the shared solver
    rows = [worker.step() for _ in range(8)]
    batch = [np.stack([np.asarray(r[i]) for r in rows]) for i in range(5)]
    td = trainer.step(batch, weights=np.ones(8, np.float32))
    assert td.shape == (8,) and bool(torch.isfinite(td).all()) and trainer.cur_step == 1
