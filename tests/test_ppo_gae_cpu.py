"""GAE(lambda) for the device PPO loop, the parts that need no GPU: ppo_actors.gae (the numpy
restatement of csrc/ppo_actor.hpp's scan) against the textbook double sum and at its edges,
HostRollout.finish_gae's row order, PPOSolver's torch path on a 5-column batch against hand-written
autograd in fp64, and PpoLoopConfig's refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from reth_amd.ppo import ENT_COEF, VF_COEF, PPOSolver, _params6
from reth_amd.ppo_actors import HostRollout, gae
from reth_amd.solver import Box, Discrete


def textbook(r, done, v, v_last, gamma, lam):
    """adv_t = sum_l (gamma lam)^l [prod_{j<l} (1 - done_{t+j})] delta_{t+l} in plain fp64, a double sum"""
    r, done, v = (np.asarray(x, np.float64) for x in (r, done, v))
    T = len(r)
    nv = np.append(v[1:], np.float64(v_last))
    delta = r + gamma * nv * (1 - done) - v
    adv = np.zeros(T)
    for t in range(T):
        w = 1.0
        for l in range(T - t):
            adv[t] += w * delta[t + l]
            w *= gamma * lam * (1 - done[t + l])
    return adv, adv + v


def _rows(T, seed, p_done=0.15):
    rng = np.random.default_rng(seed)
    r, v = rng.standard_normal(T).astype(np.float32), rng.standard_normal(T).astype(np.float32)
    done = (rng.random(T) < p_done).astype(np.float32)
    return r, done, v, np.float32(rng.standard_normal())


@pytest.mark.parametrize("gamma", [0.0, 0.99, 1.0])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("T", [1, 2, 33, 200])
def test_gae_is_the_textbook_sum(T, gamma, lam):
    """the scan before its one rounding to fp32 (dtype=np.float64) against the double sum, to 1e-12 of
    the largest |value|; the fp32 outputs are those values rounded once"""
    r, done, v, v_last = _rows(T, T)
    adv, ret = gae(r, done, v, v_last, gamma, lam)
    adv64, ret64 = gae(r, done, v, v_last, gamma, lam, dtype=np.float64)
    want_adv, want_ret = textbook(r, done, v, v_last, gamma, lam)
    assert adv.dtype == ret.dtype == np.float32 and adv.shape == ret.shape == (T,) and adv64.dtype == np.float64
    for got, want in ((adv64, want_adv), (ret64, want_ret)):
        assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    assert np.array_equal(adv, adv64.astype(np.float32)) and np.array_equal(ret, ret64.astype(np.float32))


def test_lambda_one_gives_the_discounted_return():
    """lambda = 1 and one episode ending in done: ret_t = sum_l gamma^l r_{t+l}, whatever the values"""
    T, gamma = 40, 0.99
    r, _, v, v_last = _rows(T, 7)
    done = np.zeros(T, np.float32)
    done[-1] = 1.0
    _, ret = gae(r, done, v, v_last, gamma, 1.0)
    want = np.zeros(T)
    run = 0.0
    for t in range(T - 1, -1, -1):
        run = np.float64(r[t]) + gamma * run
        want[t] = run
    assert float(np.abs(ret.astype(np.float64) - want).max()) <= 1e-6 * float(np.abs(want).max())


def test_lambda_zero_gives_the_td_error():
    T, gamma = 25, 0.9
    r, done, v, v_last = _rows(T, 8)
    adv, ret = gae(r, done, v, v_last, gamma, 0.0)
    nv = np.append(v[1:], v_last).astype(np.float64)
    delta = (r.astype(np.float64) + (np.float64(gamma) * nv) * (1.0 - done.astype(np.float64))) - v.astype(np.float64)
    assert np.array_equal(adv, delta.astype(np.float32))
    assert np.array_equal(ret, (delta + v.astype(np.float64)).astype(np.float32))
    assert done.sum() > 0 and done.sum() < T


def test_a_done_on_the_last_row_ignores_v_last():
    r, done, v, _ = _rows(17, 9)
    done[-1] = 1.0
    a = gae(r, done, v, 5.0, 0.99, 0.95)
    b = gae(r, done, v, -1e6, 0.99, 0.95)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    done[-1] = 0.0
    c = gae(r, done, v, -1e6, 0.99, 0.95)
    assert not np.array_equal(a[0], c[0])


def test_host_rollout_finish_gae_row_order_with_ragged_fills():
    N, cap, D = 5, 6, 3
    fills = [3, 0, 6, 1, 4]
    rng = np.random.default_rng(3)
    host = HostRollout(N, cap, D)
    host.seg_s[...] = rng.standard_normal((N, cap, D))
    host.seg_a[...] = rng.integers(0, 3, (N, cap))
    host.seg_r[...] = rng.standard_normal((N, cap))
    host.seg_logp[...] = -rng.random((N, cap))
    host.seg_done[2, 2] = host.seg_done[4, 3] = 1.0
    host.fill[:] = fills
    host.complete[:] = [0, 0, 3, 0, 4]
    v, v_last = rng.standard_normal((N, cap)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    seg = {k: getattr(host, k).copy() for k in ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp")}
    s, a, ret, logp, adv, n = host.finish_gae(v, v_last, 0.99, 0.95)
    assert n == sum(fills) and len(s) == len(a) == len(ret) == len(logp) == len(adv) == n
    off = 0
    for i, m in enumerate(fills):
        assert np.array_equal(s[off:off + m], seg["seg_s"][i, :m]) and np.array_equal(a[off:off + m], seg["seg_a"][i, :m])
        assert np.array_equal(logp[off:off + m], seg["seg_logp"][i, :m])
        want = gae(seg["seg_r"][i, :m], seg["seg_done"][i, :m], v[i, :m], v_last[i], 0.99, 0.95)
        assert np.array_equal(adv[off:off + m], want[0]) and np.array_equal(ret[off:off + m], want[1])
        off += m
    assert not host.fill.any() and not host.complete.any()
    assert host.finish_gae(v, v_last, 0.99, 0.95)[-1] == 0


@pytest.mark.parametrize("B,A", [(1, 2), (64, 2), (67, 3)])
def test_torch_path_takes_the_advantage_as_given(B, A):
    """one epoch of update() on a 5-column batch, fp64 networks, plain SGD so that the step shows the
    gradient: against the loss written out by hand with the given advantages (1e-13, as
    test_ppo_cpu.py's analytic gradient)"""
    D = 4
    g = torch.Generator().manual_seed(B + A)
    torch.manual_seed(B)
    solver = PPOSolver(Box(-1, 1, (D,)), Discrete(A), k_epochs=1, device="cpu", impl="torch")
    for net in (solver.actor_network, solver.value_network):
        net.double()
    solver.actor_optimizer = torch.optim.SGD(solver.actor_network.parameters(), lr=1.0)
    solver.value_optimizer = torch.optim.SGD(solver.value_network.parameters(), lr=1.0)
    solver._tensor = lambda x, dtype: torch.as_tensor(x).to(torch.float64 if dtype == torch.float32 else dtype)
    s = torch.randn(B, D, generator=g, dtype=torch.float64)
    ret, adv = torch.randn(B, generator=g, dtype=torch.float64), torch.randn(B, generator=g, dtype=torch.float64)
    a = torch.randint(0, A, (B,), generator=g)
    cycle = torch.tensor([0.5, 0.75, 0.9, 1.0, 1.1, 1.25, 1.6], dtype=torch.float64)
    with torch.no_grad():
        old = Categorical(solver.actor_network(s)).log_prob(a) - cycle[torch.arange(B) % 7].log()
    before = [p.detach().clone() for n in (solver.actor_network, solver.value_network) for p in _params6(n)]
    # by hand, on copies
    ps = [p.clone().requires_grad_() for p in before]

    def forward(w, x):
        h = torch.tanh(F.linear(x, w[0], w[1]))
        return F.linear(torch.tanh(F.linear(h, w[2], w[3])), w[4], w[5])

    logp_all = torch.log_softmax(forward(ps[:6], s), 1)
    v = forward(ps[6:], s)[:, 0]
    rho = (logp_all.gather(1, a[:, None])[:, 0] - old).exp()
    ent = -(logp_all.exp() * logp_all).sum(1)
    loss = -torch.min(rho * adv, rho.clamp(0.8, 1.2) * adv) + VF_COEF * ((v - ret) ** 2).mean() - ENT_COEF * ent
    loss.mean().backward()
    loss_abs = solver.update([s, a, ret, old, adv])
    assert float((loss_abs - loss.detach().abs()).abs().max()) <= 1e-13 * max(1.0, float(loss.abs().max()))
    after = [p.detach() for n in (solver.actor_network, solver.value_network) for p in _params6(n)]
    for k, (p0, p1, w) in enumerate(zip(before, after, ps)):
        step = p0 - p1  # lr = 1: the gradient
        assert float((step - w.grad).abs().max()) <= 1e-13 * max(1.0, float(w.grad.abs().max())), k
    assert float(ps[4].grad.abs().max()) > 0 and float(ps[10].grad.abs().max()) > 0
    with pytest.raises(ValueError, match="batch"):
        solver.update([s, a, ret])


def test_config_refusals():
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    with pytest.raises(ValueError, match="normalize_adv"):
        PpoLoop(PpoLoopConfig(normalize_adv=True))
    with pytest.raises(ValueError, match="gae_lambda"):
        PpoLoop(PpoLoopConfig(gae_lambda=1.5, horizon=32))
    with pytest.raises(ValueError, match="horizon 0"):
        PpoLoop(PpoLoopConfig(gae_lambda=0.95, horizon=0))
    # None: the refusal of a short horizon and its message are as they were
    with pytest.raises(ValueError, match="horizon 32 < max_episode_steps 200"):
        PpoLoop(PpoLoopConfig(horizon=32))
    cfg = PpoLoopConfig()
    assert cfg.gae_lambda is None and cfg.normalize_adv is False
