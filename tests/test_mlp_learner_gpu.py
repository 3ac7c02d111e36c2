"""DQNSolver with model.MLP_IMPL = "hip" (the MLP Q-network's act / calc_loss / update on the
fused kernels of csrc/mlp.hpp): the reference's golden CartPole updates, agreement with the
default torch path, a captured and replayed update, and the CartPole example."""
import os
import sys

import numpy as np
import pytest
import torch

from reth_amd import model
from reth_amd.solver import Box, DQNSolver, Discrete
from reth_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solver(dev, seed, **kw):
    torch.manual_seed(seed)
    args = dict(gamma=0.99, clip_value=40, double_q=True, dueling=True, learning_rate=1e-4,
                update_target_interval=200, device=dev)
    args.update(kw)
    return DQNSolver(Box(-1, 1, (4,)), Discrete(2), **args)


@pytest.fixture
def hip(monkeypatch):
    monkeypatch.setattr(model, "MLP_IMPL", "hip")


def test_cartpole_golden_three_updates_on_hip(golden, dev, hip):
    """test_cartpole_mlp_three_updates' asserts with the switch on"""
    g = golden("dqn_cartpole_b64.npz")
    solver = _solver(dev, int(g["seed"]))
    assert solver.mlp_impl == "hip" and solver.mlp_impl_active == "hip"
    batch = [g["s0"], g["a"], g["r"], g["s1"], g["done"]]
    np.testing.assert_allclose(solver.calc_loss(batch).numpy(), np.abs(g["td"]), rtol=1e-5, atol=1e-6)
    for k in range(3):
        before = solver.mlp_hip_launches
        td = solver.update(batch).numpy()
        assert solver.mlp_hip_launches == before + 1  # the update ran on rth_mlp_dqn_grads
        np.testing.assert_allclose(td, g[f"upd{k}_abs_td"], rtol=1e-5, atol=1e-6)
    for k, v in solver.q_network.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g[f"final/{k}"], rtol=1e-5, atol=1e-6)
    assert solver.mlp_hip_launches > 0


def test_agrees_with_the_default_path(golden, dev, monkeypatch):
    g = golden("dqn_cartpole_b64.npz")
    batch = [g["s0"], g["a"], g["r"], g["s1"], g["done"]]
    isw = np.linspace(0.2, 1.0, 64)
    default = _solver(dev, 11)
    monkeypatch.setattr(model, "MLP_IMPL", "hip")
    hip = _solver(dev, 11)
    assert default.mlp_impl_active is None and hip.mlp_impl_active == "hip"
    for p, q in zip(default.q_network.parameters(), hip.q_network.parameters()):
        assert torch.equal(p, q)
    td_d, td_h = default.compute_grads(batch, isw), hip.compute_grads(batch, isw)

    def close(a, b):
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=2e-6 * np.abs(b).max())

    close(td_h, td_d)
    close(hip.last_loss, default.last_loss)
    assert hip.last_loss.shape == default.last_loss.shape
    for p, q in zip(hip.q_network.parameters(), default.q_network.parameters()):
        assert p.grad is not None and p.grad.shape == p.shape
        close(p.grad, q.grad)
    assert not getattr(td_h, "_rth_mean_tracked", False)
    close(hip.calc_loss(batch), default.calc_loss(batch))
    n0 = hip.mlp_hip_launches
    acts_h = [hip.act(s) for s in g["s0"]]
    assert hip.mlp_hip_launches == n0 + 64
    assert acts_h == [default.act(s) for s in g["s0"]]
    ab = hip.act_batch(g["s0"])
    assert ab.dtype == torch.int32 and ab.is_cuda and ab.shape == (64,) and ab.cpu().tolist() == acts_h
    assert default.act_batch(g["s0"]).cpu().tolist() == acts_h
    assert default.mlp_hip_launches == 0
    # a precomputed q1t: the existing path runs (and agrees)
    q1t = hip.target_heads(g["s1"])
    n0 = hip.mlp_hip_launches
    close(hip.compute_grads(batch, isw, q1t=q1t), td_d)
    assert hip.mlp_hip_launches == n0


def test_two_solvers_do_not_share_a_workspace(dev, hip):
    a, b = _solver(dev, 1), _solver(dev, 2)
    wa, wb = a.q_network._mlp_workspace(dev, 64), b.q_network._mlp_workspace(dev, 64)
    assert wa.data_ptr() != wb.data_ptr() and a.q_network._mlp_workspace(dev, 64) is wa
    assert a.q_network._mlp_workspace(dev, 32) is not wa


def test_captured_update_replays_bitwise(golden, dev, hip):
    """one trainer.train captured on a side stream (a single stream, no parallel branches) and
    replayed three times after an eager warm-up == four eager updates from the same start"""
    g = golden("dqn_cartpole_b64.npz")
    batch = [torch.as_tensor(g[k], device=dev) for k in ("s0", "a", "r", "s1", "done")]
    batch = [batch[0].float(), batch[1].long(), batch[2].float(), batch[3].float(), batch[4].float()]
    isw = torch.linspace(0.2, 1.0, 64, dtype=torch.float64, device=dev)
    eager = Trainer(_solver(dev, 7, update_target_interval=1000), logger=False)
    tds = [eager.train(batch, weights=isw).clone() for _ in range(4)]
    torch.cuda.synchronize()

    tr = Trainer(_solver(dev, 7, update_target_interval=1000), logger=False)
    assert tr.solver.mlp_impl_active == "hip"
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = [tr.train(batch, weights=isw).clone()]  # warm-up = update 1
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        td = tr.train(batch, weights=isw)
    for _ in range(3):
        graph.replay()
        got.append(td.clone())
    torch.cuda.synchronize()
    for a, b in zip(got, tds):
        assert torch.equal(a, b)
    for p, q in zip(tr.solver.q_network.parameters(), eager.solver.q_network.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(tr._err_acc, eager._err_acc)
    assert not any(torch.equal(tds[0], t) for t in tds[1:])  # the updates did move the weights


def test_cartpole_hip_example_runs(dev):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import cartpole_dqn_hip

    worker, trainer, buffer = cartpole_dqn_hip.main(max_ts=40)
    assert trainer.cur_step == 40
    assert buffer.size == 1000 + 40 * 64 and worker.cur_step == buffer.size
    assert trainer.solver.mlp_impl_active == "hip" and trainer.solver.mlp_hip_launches >= 80
    assert model.MLP_IMPL is None  # the example restores the switch
