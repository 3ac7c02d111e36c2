"""The MLP Q-network's fused HIP kernels (csrc/mlp.hpp), the parts that need no GPU: the shape
pre-check and workspace size of the C ABI, the model.MLP_IMPL switch's default, and that the
switch leaves the host solver (device="cpu") alone."""
import numpy as np
import torch

from reth_amd import _lib, model
from reth_amd.solver import Box, DQNSolver, Discrete


def test_supported_shapes():
    lib = _lib.lib()
    for shape in [(4, 128, 2), (1, 128, 1), (64, 128, 18)]:
        assert lib.rth_mlp_supported(*shape) == 1, shape
    for shape in [(0, 128, 2), (65, 128, 2), (4, 64, 2), (4, 128, 19), (4, 128, 0)]:
        assert lib.rth_mlp_supported(*shape) == 0, shape


def test_workspace_size():
    lib = _lib.lib()
    prev = 0
    for B in [1, 2, 5, 64, 67, 130, 257, 512, 4096]:
        for D, A in [(4, 2), (1, 1), (64, 18)]:
            assert lib.rth_mlp_workspace(B, D, 128, A) > 0
        size = lib.rth_mlp_workspace(B, 4, 128, 2)
        assert size % 16 == 0 and size >= prev
        prev = size
    for shape in [(0, 128, 2), (65, 128, 2), (4, 64, 2), (4, 128, 19), (4, 128, 0)]:
        assert lib.rth_mlp_workspace(64, *shape) <= 0, shape
        assert b"rth_mlp_workspace" in lib.rth_last_error()
    assert lib.rth_mlp_workspace(0, 4, 128, 2) <= 0


def test_switch_defaults_to_none():
    assert model.MLP_IMPL is None


def test_params6_order():
    net = model.MLP_DQNNetwork((4,), 2)
    names = [n for n, _ in net.named_parameters()]
    assert names == ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "nn.4.weight", "nn.4.bias"]
    assert all(a is b for a, b in zip(net._params6(), net.parameters()))
    assert net.dims() == (4, 128, 2)


def test_cpu_solver_ignores_the_switch(golden, monkeypatch):
    """test_cpu_solver's golden CartPole updates with MLP_IMPL = "hip": still the host solver"""
    from reth_amd.cpu_solver import CpuDQNSolver

    monkeypatch.setattr(model, "MLP_IMPL", "hip")
    g = golden("dqn_cartpole_b64.npz")
    torch.manual_seed(int(g["seed"]))
    solver = DQNSolver(Box(-1, 1, (4,)), Discrete(2), gamma=0.99, clip_value=40, double_q=True, dueling=True,
                       learning_rate=1e-4, update_target_interval=200, device="cpu")
    assert isinstance(solver, CpuDQNSolver) and solver.device.type == "cpu"
    assert getattr(solver, "mlp_impl_active", None) is None
    batch = [g["s0"], g["a"], g["r"], g["s1"], g["done"]]
    np.testing.assert_array_equal(solver.calc_loss(batch).numpy(), np.abs(g["td"]))
    for k in range(3):
        np.testing.assert_array_equal(solver.update(batch).numpy(), g[f"upd{k}_abs_td"])
    for k, v in solver.q_network.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), g[f"final/{k}"])
