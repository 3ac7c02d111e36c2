"""MlpApexDQN on the other classic-control envs (MlpApexConfig.env): bookkeeping and graph == eager
on Acrobot-v1, a MountainCar-v0 run, that Acrobot learns, and the Acrobot example."""
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


def test_acrobot_bookkeeping(hip_mlp):
    from reth_amd.mlp_actors import VecMlpActors

    K, N, B, n = 40, 16, 16, 3
    loop = _loop(env="Acrobot-v1", n_actors=N, batch_size=B, n_step=n, sample_start=64, capacity=4096, seed=3)
    assert isinstance(loop.actors, VecMlpActors) and loop.max_episode_steps == 500
    assert loop.solver.q_network.dims() == (6, 128, 3)
    assert [tuple(b.shape) for b in loop.batch] == [(B, 6), (B,), (B,), (B, 6), (B,)]
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
    # the running returns: -1 a step, no episode of 40 steps from the reset states ends
    np.testing.assert_array_equal(loop.actors.return_stats()[0].cpu().numpy(), np.full(N, -float(K)))


def test_acrobot_graph_equals_eager(hip_mlp):
    K = 30
    cfg = dict(env="Acrobot-v1", n_actors=16, batch_size=16, sample_start=64, capacity=4096, seed=5,
               update_target_interval=7)
    eager, graph = _loop(**cfg), _loop(**cfg)
    eager.run(K)
    with pytest.raises(RuntimeError, match="steady-state"):
        graph.capture()
    graph.run(10)
    graph.capture()
    graph.run(K - 10)
    torch.cuda.synchronize()
    assert graph._graph is not None and graph.updates == eager.updates > 0 and graph.rows_emitted == eager.rows_emitted
    assert graph.actors.launches == K and graph.solver.mlp_hip_launches == eager.solver.mlp_hip_launches
    same = lambda a, b: a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()
    for (k, p), q in zip(eager.solver.q_network.named_parameters(), graph.solver.q_network.parameters()):
        assert same(p, q), k
    for p, q in zip(eager.solver.target_q_network.parameters(), graph.solver.target_q_network.parameters()):
        assert same(p, q)
    te, tg = eager.replay.tree.export(), graph.replay.tree.export()
    assert all(same(a, b) for a, b in zip(te, tg)) and float(te[2].sum()) > 0
    for k in ("state", "ep_steps", "t_dev", "stats", "ret_stats", "obs_ring", "cur_slot"):
        assert same(getattr(eager.actors, k), getattr(graph.actors, k)), k


def test_mountaincar_runs_and_updates(hip_mlp):
    K, N = 60, 16
    loop = _loop(env="MountainCar-v0", n_actors=N, batch_size=16, sample_start=64, capacity=4096, seed=1,
                 max_episode_steps=25)
    assert loop.solver.q_network.dims() == (2, 128, 3) and loop.max_episode_steps == 25
    before = [p.detach().clone() for p in loop.solver.q_network.parameters()]
    loop.run(K)
    torch.cuda.synchronize()
    assert loop.updates == K - 1 - 3 and loop.env_steps == N * K and loop.replay.size == N * (K - 1)
    assert any(not torch.equal(b, p) for b, p in zip(before, loop.solver.q_network.parameters()))
    assert all(torch.isfinite(p).all() for p in loop.solver.q_network.parameters())
    ep, tot, last = (x.cpu().numpy() for x in loop.actors.episode_stats())
    _, rsum, rlast = (x.cpu().numpy() for x in loop.actors.return_stats())
    assert (ep == 2).all() and (last == 25).all()  # the time limit ends them: nothing reaches the goal in 25 steps
    np.testing.assert_array_equal(rsum, -tot.astype(np.float64))
    np.testing.assert_array_equal(rlast, -last.astype(np.float64))
    assert loop.greedy_eval(32) == 25.0 and loop.greedy_eval(32, metric="return") == -25.0


def _random_policy_mean(episodes=40):
    from reth_amd.envs import Acrobot

    env = Acrobot(500, seed=0)
    rng = np.random.RandomState(1)
    total = 0
    for _ in range(episodes):
        env.reset()
        done = False
        while not done:
            _, _, done, _ = env.step(int(rng.randint(3)))
            total += 1
    return total / episodes


# the smallest multiple of 1,000 at which the measured curve of this configuration reaches 0.4 x the random policy's
# mean length (profiles/r11/classic_control.txt: 89.3 at 9,000); the assertion below is at 0.5 x
ACROBOT_ITERATIONS = 9000


def test_learns_acrobot(hip_mlp, capsys):
    """fixed seed, 9,000 iterations of N = 64 / B = 64 / n_step = 3 (the steady-state iteration as
    a replayed graph): the best greedy mean episode length of the nine checkpoints is at most half
    the random policy's (measured here on the host env)"""
    base = _random_policy_mean()
    loop = _loop(env="Acrobot-v1", n_actors=64, batch_size=64, n_step=3, learning_rate=1e-3, update_target_interval=200,
                 seed=0)
    curve = []
    for _ in range(ACROBOT_ITERATIONS // 1000):
        for _ in range(1000):
            if loop._graph is None and loop.graph_ready():
                loop.capture()
            loop.iteration()
        curve.append(loop.greedy_eval(256))
    with capsys.disabled():
        print(f"\n[mlp_apex] Acrobot random-policy mean episode length {base:.1f}; greedy mean every 1000 iterations: "
              f"{', '.join(f'{c:.1f}' for c in curve)} ({loop.updates} updates, {loop.env_steps} env steps, "
              f"greedy mean return {loop.greedy_eval(256, metric='return'):.1f})")
    assert 400 < base <= 500
    assert min(curve) <= 0.5 * base


def test_example_smoke(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import acrobot_apex_hip
    finally:
        sys.path.pop(0)
    from reth_amd import model

    loop = acrobot_apex_hip.main(iterations=200, eval_every=100, eval_envs=32)
    assert model.MLP_IMPL is None  # restored
    assert loop.cfg.env == "Acrobot-v1" and loop._graph is not None
    assert loop.iterations == 200 and loop.actors.launches == 200 and loop.updates > 0
    out = capsys.readouterr().out
    assert "env-steps/s" in out and "updates/s" in out and "greedy mean return" in out and "(graph)" in out
