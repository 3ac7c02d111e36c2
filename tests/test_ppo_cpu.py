"""PPO (reth_amd/ppo.py, csrc/ppo.hpp), the parts that need no GPU: the C ABI's shape pre-checks,
the seeded initialisation and the torch path against the reference's recorded run
(tests/golden/ppo_cartpole_b64.npz, written by tests/golden/make_golden_ppo.py), the weights
stream, sync_weights, the two return functions, the YAML plumbing of the example, the compat
re-exports and the analytic gradient the kernels implement against autograd in fp64."""
import hashlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from conftest import ROOT
from reth_amd import _lib, envs, presets
from reth_amd.ppo import (ENT_COEF, PARAM_KEYS, VF_COEF, ActorNetwork, PPOSolver, ValueNetwork, _params6,
                          calculate_discount_rewards, calculate_discount_rewards_with_dones,
                          generate_discrite_ppo_model)
from reth_amd.solver import Box, Discrete

CONFIG = os.path.join(ROOT, "examples", "cartpole_ppo.yaml")
OBS, ACT = Box(-1, 1, (4,)), Discrete(2)
NETS = (("actor", "actor_network", "action_layer"), ("value", "value_network", "value_layer"))


# ------------------------------------------------------------------ ABI shape checks
def test_supported_shapes_and_workspace():
    lib = _lib.lib()
    for shape in [(4, 64, 2), (1, 64, 2), (64, 64, 18), (7, 64, 3), (17, 64, 6)]:
        assert lib.rth_ppo_supported(*shape) == 1, shape
    bad = [(0, 64, 2), (65, 64, 2), (4, 100, 2), (4, 128, 2), (4, 64, 1), (4, 64, 19)]
    for shape in bad:
        assert lib.rth_ppo_supported(*shape) == 0, shape
        assert lib.rth_ppo_workspace(64, *shape) <= 0, shape
        err = lib.rth_last_error()
        assert b"rth_ppo_workspace" in err and b"unsupported shape" in err and b"1..64" in err and b"2..18" in err
    prev = 0
    for B in [1, 5, 64, 67, 8200]:
        size = lib.rth_ppo_workspace(B, 4, 64, 2)
        # the log-probabilities, the loss parts and both networks' activations and gradients of a row
        assert size % 16 == 0 and size > prev and size >= 4 * B * (3 + 2 + 1 + 8 * 64)
        prev = size
    assert lib.rth_ppo_workspace(0, 4, 64, 2) <= 0


# ------------------------------------------------------------------ init and the torch path vs the golden
def _sha1(t):
    return hashlib.sha1(np.ascontiguousarray(t.detach().numpy()).tobytes()).hexdigest().encode()


def golden_solver(g, device="cpu", **kw):
    torch.manual_seed(int(g["seed"]))
    return PPOSolver(OBS, ACT, device=device, **kw)


def golden_batch(g):
    return [g["states"], g["actions"], g["returns"], g["old_logprobs"]]


def test_seeded_init_and_keys_are_the_references(golden):
    g = golden("ppo_cartpole_b64.npz")
    torch.manual_seed(int(g["seed"]))
    models = generate_discrite_ppo_model(OBS, ACT, hidden_size=64, learning_rate=0.01)
    assert list(models) == ["value_network", "value_optimizer", "actor_network", "actor_optimizer"]
    for name, key, layer in NETS:
        sd = models[key].state_dict()
        assert list(sd) == bytes(g[f"keys/{name}"]).decode().split("\n") == [f"{layer}.{k}" for k in PARAM_KEYS]
        for k, v in sd.items():
            assert _sha1(v) == bytes(g[f"init/{name}/{k}"]), (name, k)
        assert all(a is b for a, b in zip(_params6(models[key]), models[key].parameters()))
        assert type(models[key.replace("network", "optimizer")]) is torch.optim.Adam
    s = golden_solver(g)
    for name, key, _ in NETS:
        for k, v in getattr(s, key).state_dict().items():
            assert _sha1(v) == bytes(g[f"init/{name}/{k}"]), (name, k)
    assert float(g["ratio_margin"]) > 1e-4 and float(g["drift_param"]) < 1e-6 and float(g["drift_loss"]) < 1e-6


def test_torch_path_reproduces_the_golden(golden):
    g = golden("ppo_cartpole_b64.npz")
    solver = golden_solver(g)
    assert solver.impl_active == "torch" and solver.device.type == "cpu" and solver.k_epochs == 4
    assert sorted(set(g["actions"].tolist())) == [0, 1]
    for k in range(3):
        loss = solver.update(golden_batch(g))
        assert loss.shape == (64,) and loss.dtype == torch.float32 and loss.device.type == "cpu"
        err = np.abs(loss.numpy() - g[f"upd{k}_abs_loss"]).max()
        print(f"update {k}: max ||loss| - golden| {err:.3e} (|loss| up to {g[f'upd{k}_abs_loss'].max():.2f})")
        np.testing.assert_allclose(loss.numpy(), g[f"upd{k}_abs_loss"], rtol=1e-5, atol=1e-6)
    for name, key, _ in NETS:
        for k, v in getattr(solver, key).state_dict().items():
            np.testing.assert_allclose(v.numpy(), g[f"final/{name}/{k}"], rtol=1e-5, atol=1e-6)
    torch.manual_seed(int(g["act_seed"]))
    res = [solver.act(s) for s in g["act_states"]]
    assert all(type(a) is int and type(lp) is float for a, lp in res)
    assert [a for a, _ in res] == g["act_actions"].tolist()
    np.testing.assert_allclose([lp for _, lp in res], g["act_logprobs"], rtol=1e-5, atol=1e-6)
    assert solver.hip_launches == 0
    # act_batch with given uniforms: the inverse CDF of the same probabilities
    a, lp, p = solver.act_batch(g["act_states"], uniforms=[0.0, 0.999999, 0.5, 0.25], return_probs=True)
    assert a.dtype == torch.int64 and lp.dtype == torch.float32 and p.shape == (4, 2)
    assert a.tolist() == [0, 1, int(p[2, 0] <= 0.5), int(p[3, 0] <= 0.25)]
    assert torch.allclose(lp, p.gather(1, a[:, None])[:, 0].log(), rtol=1e-6, atol=1e-7)


def test_weights_stream_round_trip_and_sync_weights():
    torch.manual_seed(3)
    a, b = PPOSolver(OBS, ACT, device="cpu"), PPOSolver(OBS, ACT, device="cpu")
    stream = a.save_weights()
    states = torch.load(io.BytesIO(stream.getvalue()), weights_only=True)
    assert list(states) == [f"action_layer.{k}" for k in PARAM_KEYS]  # the actor alone, as the reference's
    value_before = [p.clone() for p in b.value_network.parameters()]
    stream.seek(0)
    b.load_weights(stream)
    for k, v in a.actor_network.state_dict().items():
        assert torch.equal(b.actor_network.state_dict()[k], v)
    assert all(torch.equal(p, q) for p, q in zip(b.value_network.parameters(), value_before))
    assert not torch.equal(next(b.value_network.parameters()), next(a.value_network.parameters()))
    ptrs = [p.data_ptr() for n in (b.actor_network, b.value_network) for p in n.parameters()]
    b.sync_weights(a)  # both networks, in place
    for net in ("actor_network", "value_network"):
        for p, q in zip(getattr(b, net).parameters(), getattr(a, net).parameters()):
            assert torch.equal(p, q) and p.data_ptr() != q.data_ptr()
    assert ptrs == [p.data_ptr() for n in (b.actor_network, b.value_network) for p in n.parameters()]
    torch.manual_seed(9)
    x = a.act(np.array([0.1, 0.2, 0.03, -0.4]))
    torch.manual_seed(9)
    assert x == b.act(np.array([0.1, 0.2, 0.03, -0.4]))


def test_return_functions_against_the_golden(golden):
    g = golden("ppo_cartpole_b64.npz")
    assert int(g["ret/n"]) >= 3
    for i in range(int(g["ret/n"])):
        r, done = g[f"ret/{i}/r"], g[f"ret/{i}/done"]
        got = calculate_discount_rewards_with_dones(r, done, 0.99)
        assert got.dtype == np.float32 and np.array_equal(got, g[f"ret/{i}/with_dones"]), i
        assert np.array_equal(calculate_discount_rewards(r, 0.99), g[f"ret/{i}/plain"]), i
        # device-buffer columns arrive as tensors
        assert np.array_equal(calculate_discount_rewards_with_dones(torch.as_tensor(r), torch.as_tensor(done), 0.99),
                              got)
    assert bool(g["ret/0/done"][4]) and not bool(g["ret/0/done"][5])  # a done in mid-sequence
    # the quirks by hand: a done row gets 0 and the running sum runs on through it
    raw = np.zeros(4, np.float32)
    raw[3] = 1.0
    raw[2] = 0.0
    raw[1] = np.float32(1.0 * 0.5 + 1.0)
    raw[0] = np.float32(1.5 * 0.5 + 1.0)
    want = (raw - raw.mean()) / ((raw - raw.mean()).std() + 1e-7)
    got = calculate_discount_rewards_with_dones(np.ones(4), np.array([False, False, True, False]), 0.5)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)


def test_presets_get_solver_and_explicit_hip_on_cpu():
    cfg = presets._parse_input(CONFIG)
    assert cfg["env"] == {"name": "CartPole-v0"}
    assert cfg["solver"] == {"name": "ppo", "k_epochs": 4, "eps_clip": 0.2, "learning_rate": 0.01}
    env = presets.get_env(CONFIG, seed=0)
    assert type(env) is envs.CartPole
    s = presets.get_solver(CONFIG, env=env, device="cpu")
    assert isinstance(s, PPOSolver) and s.impl_active == "torch" and (s.k_epochs, s.eps_clip) == (4, 0.2)
    assert type(s.actor_network) is ActorNetwork and type(s.value_network) is ValueNetwork
    assert s.actor_optimizer.param_groups[0]["lr"] == 0.01 and s.value_optimizer.param_groups[0]["lr"] == 0.01
    assert type(s.actor_optimizer) is torch.optim.Adam
    assert tuple(s.actor_network.action_layer[4].weight.shape) == (2, 64)
    assert presets.get_solver(CONFIG, env=env, device="cpu", k_epochs=2, hidden_size=32).k_epochs == 2
    with pytest.raises(ValueError, match="not a GPU"):
        PPOSolver(OBS, ACT, device="cpu", impl="hip")
    with pytest.raises(ValueError, match="impl="):
        PPOSolver(OBS, ACT, device="cpu", impl="triton")
    # the worker and the trainer of the example's loop on that solver
    worker = presets.get_worker(CONFIG, solver=s, env=env, logger=False)
    trainer = presets.get_trainer(CONFIG, solver=s, logger=False)
    rows = []
    for _ in range(8):
        a, lp = s.act(worker.s0)
        s0, a, r, s1, done = worker.step(a)
        rows.append((s0, a, r, lp))
    batch = [np.stack([np.asarray(r[i]) for r in rows]) for i in range(4)]
    loss = trainer.step(batch)
    assert loss.shape == (8,) and bool(torch.isfinite(loss).all()) and trainer.cur_step == 1


def test_compat_reexports():
    compat = os.path.join(ROOT, "reth_amd", "compat")
    sys.path.insert(0, compat)
    try:
        from reth.algorithm import PPOSolver as P2
        from reth.algorithm.util import (calculate_discount_rewards as c1, calculate_discount_rewards_with_dones as c2,
                                         soft_update as s2)
        from reth.presets.config import get_solver as gs
    finally:
        sys.path.remove(compat)
    from reth_amd.ddpg import soft_update

    assert P2 is PPOSolver and c1 is calculate_discount_rewards and c2 is calculate_discount_rewards_with_dones
    assert s2 is soft_update and gs is presets.get_solver


# ------------------------------------------------------------------ the analytic gradient
def analytic_logit_and_value_grads(z, v, a, ret, old, eps, vf, ent):
    """what csrc/ppo.hpp back-propagates: d(mean loss)/d(logits) [B, A] and d/d(value) [B]"""
    B = z.shape[0]
    logp = torch.log_softmax(z, 1)
    p = logp.exp()
    H = -(p * logp).sum(1)
    rho = (logp.gather(1, a[:, None])[:, 0] - old).exp()
    adv = ret - v
    s1, s2 = rho * adv, rho.clamp(1 - eps, 1 + eps) * adv
    k = torch.where((s1 < s2) | ((rho >= 1 - eps) & (rho <= 1 + eps)), -s1, torch.zeros_like(s1))
    onehot = F.one_hot(a, z.shape[1]).to(z.dtype)
    gz = (k[:, None] * (onehot - p) + ent * p * (logp + H[:, None])) / B
    return gz, 2 * vf * (v - ret) / B


@pytest.mark.parametrize("B,A", [(1, 2), (5, 2), (64, 2), (67, 3), (130, 6), (257, 18)])
def test_analytic_gradient_is_autograds_in_fp64(B, A):
    g = torch.Generator().manual_seed(B * 31 + A)
    z = (2 * torch.randn(B, A, generator=g, dtype=torch.float64)).requires_grad_()
    v = torch.randn(B, generator=g, dtype=torch.float64).requires_grad_()
    ret = torch.randn(B, generator=g, dtype=torch.float64)
    a = torch.randint(0, A, (B,), generator=g)
    cycle = torch.tensor([0.5, 0.75, 0.9, 1.0, 1.1, 1.25, 1.6], dtype=torch.float64)
    old = torch.log_softmax(z.detach(), 1).gather(1, a[:, None])[:, 0] - cycle[torch.arange(B) % 7].log()
    # the reference's expression (ppo_solver.py:53-91)
    dist = Categorical(torch.softmax(z, 1))
    ratios = torch.exp(dist.log_prob(a) - old)
    adv = ret - v.detach()
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 0.8, 1.2) * adv) + VF_COEF * F.mse_loss(v, ret)
            - ENT_COEF * dist.entropy())
    loss.mean().backward()
    gz, gv = analytic_logit_and_value_grads(z.detach(), v.detach(), a, ret, old, 0.2, VF_COEF, ENT_COEF)
    assert float((gz - z.grad).abs().max()) <= 1e-13 * max(1.0, float(z.grad.abs().max()))
    assert float((gv - v.grad).abs().max()) <= 1e-13 * max(1.0, float(v.grad.abs().max()))
    if B >= 64:
        assert float(z.grad.abs().max()) > 0 and bool((ratios.detach() > 1.2).any()) and bool((ratios < 0.8).any())
