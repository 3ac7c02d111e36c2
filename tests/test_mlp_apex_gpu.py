"""MlpApexDQN (reth_amd/mlp_apex.py): the device CartPole loop -- bookkeeping, graph == eager,
that it learns, that it refuses to run without the fused MLP kernels, and the example."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip_mlp(monkeypatch):
    from reth_amd import model

    monkeypatch.setattr(model, "MLP_IMPL", "hip")


def _loop(**kw):
    from reth_amd.mlp_apex import MlpApexConfig, MlpApexDQN

    return MlpApexDQN(MlpApexConfig(**kw), device="cuda")


def test_bookkeeping(hip_mlp):
    K, N, B, n = 40, 16, 16, 3
    loop = _loop(n_actors=N, batch_size=B, n_step=n, sample_start=64, capacity=4096, seed=3)
    loop.run(K)
    torch.cuda.synchronize()
    rows = N * (K - n)  # every actor emits once its deque is full
    updates = K - n - 3  # the 4th emitting step stores the 64th row
    assert loop.rows_emitted == rows and loop.replay.size == rows
    assert loop.updates == updates and loop.env_steps == N * K
    root, v = loop.replay.tree.sum(), loop.replay.tree.export()[2]  # v: the stored priorities, one per slot
    stored = v[:rows].sum().item()
    assert abs(root - stored) <= 1e-9 * stored and (v[:rows] > 0).all() and (v[rows:] == 0).all()
    assert loop.replay.beta.cur_step == updates and loop.replay.info()[4] == updates
    assert loop.actors.launches == K
    assert loop.solver_calls == (K - n) + updates and loop.solver.mlp_hip_launches == loop.solver_calls
    assert int(loop.actors.t_dev[0]) == K


def test_graph_equals_eager(hip_mlp):
    K = 30
    cfg = dict(n_actors=16, batch_size=16, n_step=3, sample_start=64, capacity=4096, seed=5,
               update_target_interval=7, max_episode_steps=9)
    eager, graph = _loop(**cfg), _loop(**cfg)
    eager.run(K)
    with pytest.raises(RuntimeError, match="steady-state"):
        graph.capture()
    graph.run(10)
    graph.capture()
    graph.run(K - 10)
    torch.cuda.synchronize()
    assert graph._graph is not None and graph.updates == eager.updates and graph.rows_emitted == eager.rows_emitted
    assert graph.actors.launches == K and graph.solver.mlp_hip_launches == eager.solver.mlp_hip_launches
    same = lambda a, b: a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()
    for (k, p), q in zip(eager.solver.q_network.named_parameters(), graph.solver.q_network.parameters()):
        assert same(p, q), k
        se, sg = eager.solver.optimizer.state[p], graph.solver.optimizer.state[q]
        assert same(se["exp_avg"], sg["exp_avg"]) and same(se["exp_avg_sq"], sg["exp_avg_sq"]), k
        assert int(se["step"]) == int(sg["step"]) == eager.updates
    for p, q in zip(eager.solver.target_q_network.parameters(), graph.solver.target_q_network.parameters()):
        assert same(p, q)
    te, tg = eager.replay.tree.export(), graph.replay.tree.export()
    assert all(same(a, b) for a, b in zip(te, tg)) and float(te[2].sum()) > 0
    for k in ("state", "ep_steps", "t_dev", "stats", "obs_ring", "cur_slot"):
        assert same(getattr(eager.actors, k), getattr(graph.actors, k)), k
    assert graph.replay.beta.cur_step == eager.replay.beta.cur_step


def _random_policy_mean(episodes=2000):
    from reth_amd.envs import CartPole

    env = CartPole(200, seed=0)
    rng = np.random.RandomState(1)
    total = 0
    for _ in range(episodes):
        env.reset()
        done = False
        while not done:
            _, _, done, _ = env.step(int(rng.randint(2)))
            total += 1
    return total / episodes


def test_learns_cartpole(hip_mlp, capsys):
    """fixed seed, 3,000 iterations of N = 64 / B = 64: the best greedy mean episode length of the
    three checkpoints is at least 3x the random policy's (measured here on the host env)"""
    base = _random_policy_mean()
    loop = _loop(n_actors=64, batch_size=64, n_step=1, learning_rate=1e-3, update_target_interval=200, seed=0)
    curve = []
    for _ in range(3):
        loop.run(1000)
        curve.append(loop.greedy_eval(256))
    with capsys.disabled():
        print(f"\n[mlp_apex] random-policy mean episode length {base:.2f}; greedy mean after 1000/2000/3000 "
              f"iterations: {', '.join(f'{c:.1f}' for c in curve)} ({loop.updates} updates, {loop.env_steps} env steps)")
    assert 15 < base < 30
    assert max(curve) >= 3 * base


def test_refuses_without_the_switch():
    from reth_amd import model
    from reth_amd.mlp_apex import MlpApexDQN

    assert model.MLP_IMPL is None
    with pytest.raises(RuntimeError, match="MLP_IMPL"):
        MlpApexDQN(device="cuda")


def test_example_smoke(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import cartpole_apex_hip
    finally:
        sys.path.pop(0)
    from reth_amd import model

    loop = cartpole_apex_hip.main(iterations=200, eval_every=100, eval_envs=32)
    assert model.MLP_IMPL is None  # restored
    assert loop.iterations == 200 and loop.actors.launches == 200 and loop.updates > 0
    out = capsys.readouterr().out
    assert "env-steps/s" in out and "updates/s" in out and "mean episode length" in out
