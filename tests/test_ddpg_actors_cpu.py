"""The device Pendulum actors and the DDPG loop without a GPU: the env table, the loop's defaults
against the reference's YAML, importability, the C ABI's declarations and bindings, and that
envs.make keeps refusing Pendulum-v0."""
import os
import re

import pytest
import yaml

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "reth_hip.h")
YAML = os.path.join(ROOT, "examples", "pendulum_ddpg.yaml")
ENTRY_POINTS = ("rth_ddpg_env_reset", "rth_ddpg_actor_step")


def test_envs_table():
    from reth_amd import _lib
    from reth_amd.ddpg_actors import ENVS
    from reth_amd.envs import Pendulum

    assert ENVS == {"Pendulum-v0": (_lib.DDPG_ENV_PENDULUM, 3, 1, 200)}
    env = Pendulum()
    assert env.observation_space.shape == (3,) and env.action_space.shape == (1,) and env.max_episode_steps == 200
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"RTH_DDPG_ENV_PENDULUM\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.DDPG_ENV_PENDULUM


def test_config_defaults_are_the_yaml():
    from reth_amd.ddpg_apex import DdpgApexConfig
    from reth_amd.noise import OUNoise

    with open(YAML) as f:
        y = yaml.safe_load(f)
    c = DdpgApexConfig()
    assert c.env == y["env"]["name"]
    s = y["solver"]
    assert (c.gamma, c.tau, c.learning_rate_actor, c.learning_rate_critic) == (
        s["gamma"], s["tau"], s["learning_rate_actor"], s["learning_rate_critic"])
    assert (c.gamma, c.tau, c.learning_rate_actor, c.learning_rate_critic) == (0.99, 0.001, 1e-4, 1e-3)
    assert c.epsilon == y["worker"]["exploration"]["epsilon"] == "1,0.01,30000"
    r = y["replay_buffer"]
    assert r["prioritized"] is True
    assert (c.capacity, c.alpha, c.beta) == (r["capacity"], r["alpha"], r["beta"]) == (100000, 0.6, "0.4,1,100000")
    n = OUNoise(1)  # the reference's noise defaults
    assert (c.ou_mu, c.ou_theta, c.ou_sigma) == (n.mu, n.theta, n.sigma) == (0, 0.15, 0.2)
    assert (c.n_actors, c.batch_size, c.sample_start) == (64, 64, 1000)  # examples/ddpg/run.py
    assert c.cast_actions_to_long is False


def test_importable_without_a_gpu():
    from reth_amd.ddpg_actors import VecDdpgActors, _linear
    from reth_amd.ddpg_apex import DdpgApex

    for cls, names in ((VecDdpgActors, ("reset", "step", "rows", "columns", "current_obs", "set_state",
                                        "episode_stats", "return_stats", "_alloc")),
                       (DdpgApex, ("iteration", "run", "graph_ready", "capture", "greedy_eval"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert _linear("1,0.01,30000") == (1.0, 0.01, 30000) and _linear(0.0) == (0.0, 0.0, 1)
    with pytest.raises(ValueError):
        _linear("exp,1,0.01,30000")
    with pytest.raises(ValueError, match="unknown env"):
        VecDdpgActors("CartPole-v0", 4, device="cpu")


def test_header_declares_and_binding_covers_the_entry_points():
    import ctypes

    from reth_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in reth_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[0].startswith("const rth_ddpg_actor_args *") and len(params) == 2
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_i32 and len(args) == 2 and args[0]._type_ is _lib.DdpgActorArgs
        assert hasattr(_lib.lib(), name), f"{name} declared but not exported"
    # the struct's fields in the header's order, pointers and scalars of the same widths
    body = re.search(r"typedef struct rth_ddpg_actor_args \{(.*?)\} rth_ddpg_actor_args;", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.search(r"(\w+)\s*$", first).group(1)] + [re.sub(r"[\s\*]", "", r) for r in rest]
    assert names == [f[0] for f in _lib.DdpgActorArgs._fields_]
    assert ctypes.sizeof(_lib.DdpgActorArgs) == 8 * 22 + 8 * 5 + 8 + 4 + 4


def test_make_still_refuses_pendulum():
    from reth_amd import envs

    with pytest.raises(NotImplementedError):
        envs.make("Pendulum-v0")
    assert type(envs.make_host("Pendulum-v0", seed=1)) is envs.Pendulum
