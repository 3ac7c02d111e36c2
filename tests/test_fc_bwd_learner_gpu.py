"""model.FC1_BWD = "hip" (r07): the learner's update with FC1's backward on rth_fc_bwd instead of
the two hipBLASLt GEMMs.  End to end, test_learner_full_gpu's own test (the captured learner
graph against the reference's updates: per-tensor gradient, total norm, |td|, the parameters
after two updates) runs with the switch on and must hold its bounds unchanged; the path check
shows the switch reaches the explicit pass (the network owns an "fc1_bwd" workspace afterwards,
and none without it); and the autograd path's _LinearReLU.backward gives the same gradients
within the kernel's bound either way, computing only what needs_input_grad asks for."""
import numpy as np
import pytest
import torch

import test_learner_full_gpu as base

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["dqn_pong_b512.npz", "dqn_beamrider_b64.npz"])
def test_apex_learner_graph_vs_reference_fc1_bwd_hip(golden, dev, name, monkeypatch):
    from reth_amd import model

    monkeypatch.setattr(model, "FC1_BWD", "hip")
    base.test_apex_learner_graph_vs_reference(golden, dev, name)


@pytest.mark.parametrize("switch", ["hip", None])
def test_fc1_bwd_switch_reaches_the_learner(dev, monkeypatch, switch):
    from reth_amd import model
    from reth_amd.apex import ApexConfig, ApexDQN

    monkeypatch.setattr(model, "FC1_BWD", switch)
    cfg = ApexConfig(n_actors=16, capacity=2048, batch_size=64, sample_start=64, seed=3)
    ax = ApexDQN(cfg, device=dev)
    ax.prefill(cfg.capacity)
    for _ in range(8):
        ax.iteration()
        if ax.updates >= 1:
            break
    torch.cuda.synchronize()
    assert ax.updates >= 1
    net = ax.solver.q_network
    kinds = {k[1] for k in net.__dict__.get("_workspaces", {})}
    assert ("fc1_bwd" in kinds) == (switch == "hip"), kinds
    assert all(torch.isfinite(p.grad).all() for p in net.parameters())
    ax.close()


def test_linear_relu_autograd_backward(dev, monkeypatch):
    from reth_amd import model

    B, N, K = 64, 128, 192
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.rand((B, K), device=dev, generator=g) * 3 / np.sqrt(B)
    w = (torch.rand((N, K), device=dev, generator=g) * 2 - 1) / np.sqrt(K)
    b = (torch.rand(N, device=dev, generator=g) * 2 - 1) * 0.1
    gout = torch.rand((B, N), device=dev, generator=g) * 2 - 1
    # float64 on the CPU, with the ReLU mask of the device forward (the mask is not under test)
    with torch.no_grad():
        mask = (model.fc1_relu(x, w, b) > 0).cpu()
    gy = gout.cpu().double() * mask
    want_gx, want_gw = gy @ w.cpu().double(), gy.t() @ x.cpu().double()
    gy32 = gy.float()
    e32x = ((gy32 @ w.cpu()).double() - want_gx).abs().max().item()
    e32w = ((gy32.t() @ x.cpu()).double() - want_gw).abs().max().item()
    for switch in ("hip", None):
        monkeypatch.setattr(model, "FC1_BWD", switch)
        xs, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        model._LinearReLU.apply(xs, wr, br).backward(gout)
        ex = (xs.grad.double().cpu() - want_gx).abs().max().item()
        ew = (wr.grad.double().cpu() - want_gw).abs().max().item()
        print(f"_LinearReLU backward FC1_BWD={switch}: gx {ex:.3e} (cpu fp32 {e32x:.3e}), gw {ew:.3e} ({e32w:.3e})")
        assert ex <= max(4 * e32x, 2e-6) and ew <= max(4 * e32w, 2e-6), (switch, ex, e32x, ew, e32w)
        assert torch.allclose(br.grad.cpu().double(), gy.sum(0), rtol=0, atol=1e-5)
        # only the weight asks for a gradient: the same weight gradient without the data gradient
        wr2 = w.clone().requires_grad_()
        gw_only = torch.autograd.grad(model._LinearReLU.apply(x, wr2, b), [wr2], gout)[0]
        assert (gw_only.double().cpu() - want_gw).abs().max().item() <= max(4 * e32w, 2e-6)
        if switch == "hip":  # a gradient's bits do not depend on whether the other is asked for
            assert torch.equal(gw_only, wr.grad)
    # the Function itself returns None for x: called directly, with needs_input_grad as autograd sets it
    monkeypatch.setattr(model, "FC1_BWD", "hip")

    class Ctx:
        needs_input_grad = (False, True, False, False)
        owner = None
        saved_tensors = (x, w, model.fc1_relu(x, w, b))

    gxn, gwn, gbn, _ = model._LinearReLU.backward(Ctx, gout)
    assert gxn is None and gbn is None and gwn is not None
