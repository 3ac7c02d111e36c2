"""rth_mlp_q / rth_mlp_dqn_grads (csrc/mlp.hpp: the MLP Q-network's fused fp32 kernels) against
fp64 on the CPU, against themselves (position independence, determinism, bounds) and against
rth_td_huber; and the solver's fallback for a shape the kernels are not built for.

Inputs of the fp64 comparisons keep the discrete decisions safe: for seeds 0..39 the two networks
(default init) and s0 / s1 (standard normal) are drawn, the three forwards computed in fp64, and
the first seed taken at which every hidden pre-activation's magnitude and the gap between the top
two actions of the selecting network on s1 exceed 5e-6 (a ReLU or an argmax that fp32 rounding
could flip would compare two different functions)."""
import functools

import numpy as np
import pytest
import torch

from reth_amd import _lib, model
from reth_amd._lib import c_vp, call
from reth_amd.model import MLP_DQNNetwork
from reth_amd.solver import Box, DQNSolver, Discrete, td_huber_forward

pytestmark = pytest.mark.gpu

H = 128
SHAPES = [(5, 4, 2), (64, 4, 2), (67, 7, 3), (130, 33, 18), (64, 64, 18), (257, 8, 4)]
GAMMA_N = float(np.float32(0.99 ** 3))
MARGIN = 5e-6


def _forward64(net, x):
    """(Q, smallest hidden pre-activation magnitude) in fp64 on the CPU"""
    ps = [p.detach().double() for p in net._params6()]
    z1 = x.double() @ ps[0].t() + ps[1]
    z2 = z1.clamp(min=0) @ ps[2].t() + ps[3]
    q = z2.clamp(min=0) @ ps[4].t() + ps[5]
    return q, min(float(z1.abs().min()), float(z2.abs().min()))


def _gap(q):
    if q.shape[1] < 2:
        return float("inf")
    top = q.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


@functools.lru_cache(maxsize=None)
def case(B, D, A, double_q=True):
    """the first safe seed's networks and batch (CPU tensors; shared, never modified)"""
    for seed in range(40):
        torch.manual_seed(seed)
        online, target = MLP_DQNNetwork((D,), A), MLP_DQNNetwork((D,), A)
        s0, s1 = torch.randn(B, D), torch.randn(B, D)
        q0, m0 = _forward64(online, s0)
        q1o, m1 = _forward64(online, s1)
        q1t, m2 = _forward64(target, s1)
        if min(m0, m1, m2) > MARGIN and _gap(q1o if double_q else q1t) > MARGIN:
            break
    else:
        raise AssertionError(f"no safe seed in 0..39 for {(B, D, A, double_q)}")
    g = torch.Generator().manual_seed(1000 + seed)
    a = torch.randint(0, A, (B,), generator=g)
    r = torch.randn(B, generator=g)
    r[torch.arange(B) % 2 == 1] *= 3  # |td| on both sides of 1
    done = (torch.rand(B, generator=g) < 0.25).float()
    if B > 1:
        done[1] = 1.0
    isw = (0.1 + 0.9 * torch.rand(B, generator=g, dtype=torch.float64)).clamp(max=1.0)
    return dict(seed=seed, online=online, target=target, s0=s0, s1=s1, a=a, r=r, done=done, isw=isw, q0=q0, q1o=q1o,
                q1t=q1t)


def _loss_and_grads(online, target, c, double_q, isw, dtype):
    """dqn_solver.py:68-117 with torch ops on the CPU in `dtype`: (|td|, loss, six gradients)"""
    on = MLP_DQNNetwork(*_ctor(online)).to(dtype)
    on.load_state_dict({k: v.to(dtype) for k, v in online.state_dict().items()})
    tg = MLP_DQNNetwork(*_ctor(target)).to(dtype)
    tg.load_state_dict({k: v.to(dtype) for k, v in target.state_dict().items()})
    A = on.dims()[2]
    s0, s1, r, done = (c[k].to(dtype) for k in ("s0", "s1", "r", "done"))
    q = (on(s0) * torch.nn.functional.one_hot(c["a"], A).to(dtype)).sum(1)
    with torch.no_grad():
        nq = tg(s1)
        sel = torch.argmax(on(s1) if double_q else nq, 1)
        nqb = (nq * torch.nn.functional.one_hot(sel, A).to(dtype)).sum(1)
        expected = r + torch.tensor(GAMMA_N, dtype=dtype) * nqb * (1 - done)
    td = q - expected
    loss = torch.nn.functional.smooth_l1_loss(td, torch.zeros_like(td), reduction="none")
    if isw is not None:
        loss = loss * isw.to(dtype)
    loss = loss.mean()
    loss.backward()
    return td.detach().abs(), loss.detach(), [p.grad for p in on._params6()]


def _ctor(net):
    D, _, A = net.dims()
    return (D,), A


def _arr(ts):
    return (c_vp * 6)(*[t.data_ptr() for t in ts])


def _dev_params(net, dev):
    return [p.detach().to(dev).contiguous() for p in net._params6()]


def mlp_q(ps, x, A, n=None, want_argmax=True, q=None, am=None):
    """rth_mlp_q over the rows of the (possibly row-strided) device matrix x"""
    n = x.shape[0] if n is None else n
    D = ps[0].shape[1]
    q = torch.empty((n, A), dtype=torch.float32, device=x.device) if q is None else q
    am = (torch.empty(n, dtype=torch.int32, device=x.device) if am is None else am) if want_argmax else None
    assert x.stride(1) == 1
    call("rth_mlp_q", _arr(ps), x.data_ptr(), x.stride(0), n, D, H, A, q.data_ptr(),
         am.data_ptr() if am is not None else None, _lib.stream_ptr())
    return q, am


def mlp_grads(on, tg, c, dev, double_q, isw=None, backward=True, grads=None, td_abs=None, loss=None, s0=None,
              s1=None, ws=None):
    """rth_mlp_dqn_grads on the case's batch -> (td_abs, loss, grads)"""
    A, D = on[4].shape[0], on[0].shape[1]
    s0 = c["s0"].to(dev) if s0 is None else s0
    s1 = c["s1"].to(dev) if s1 is None else s1
    B = s0.shape[0]
    a, r, done = c["a"].to(dev), c["r"].to(dev), c["done"].to(dev)
    isw = None if isw is None else isw.to(dev)
    grads = [torch.full_like(p, float("nan")) for p in on] if grads is None else grads
    td_abs = torch.full((B,), float("nan"), device=dev) if td_abs is None else td_abs
    loss = torch.full((1,), float("nan"), device=dev) if loss is None else loss
    if ws is None:
        ws = torch.empty(_lib.lib().rth_mlp_workspace(B, D, H, A) // 4, dtype=torch.float32, device=dev)
    call("rth_mlp_dqn_grads", _arr(on), _arr(tg), s0.data_ptr(), s0.stride(0), s1.data_ptr(), s1.stride(0),
         a.data_ptr(), r.data_ptr(), done.data_ptr(), isw.data_ptr() if isw is not None else None, B, D, H, A, GAMMA_N,
         int(double_q), _arr(grads) if backward else None, td_abs.data_ptr(), loss.data_ptr(), ws.data_ptr(),
         _lib.stream_ptr())
    torch.cuda.synchronize()
    return td_abs, loss, grads


# ------------------------------------------------------------------ 1. forward vs fp64
@pytest.mark.parametrize("B,D,A", SHAPES + [(1, 1, 1)])
def test_forward_vs_fp64(dev, B, D, A):
    for double_q in (True, False):
        c = case(B, D, A, double_q)
        net, q64 = (c["online"], c["q1o"]) if double_q else (c["target"], c["q1t"])
        with torch.no_grad():
            e_ref = float((net(c["s1"]).double() - q64).abs().max())  # torch's fp32 CPU forward
        q, am = mlp_q(_dev_params(net, dev), c["s1"].to(dev), A)
        e_ours = float((q.cpu().double() - q64).abs().max())
        bound = max(1.5 * e_ref, 1e-6 * float(q64.abs().max()))
        print(f"forward {(B, D, A)} seed {c['seed']} double_q={double_q}: |ours - fp64| {e_ours:.3e}  "
              f"|torch fp32 - fp64| {e_ref:.3e}  bound {bound:.3e}")
        assert e_ours <= bound, (e_ours, e_ref, bound)
        assert torch.equal(am.cpu().long(), torch.argmax(q64, 1))


# ------------------------------------------------------------------ 2. ties
def test_argmax_ties_take_the_first(dev):
    torch.manual_seed(0)
    net = MLP_DQNNetwork((7,), 5)
    with torch.no_grad():
        net.nn[4].weight.copy_(net.nn[4].weight[0].expand(5, H))
        net.nn[4].bias.fill_(0.25)
    x = torch.randn(19, 7, device=dev)
    q, am = mlp_q(_dev_params(net, dev), x, 5)
    assert bool((q == q[:, :1]).all()) and bool((am == 0).all())
    with torch.no_grad():  # actions 1 and 2 the joint maximum
        net.nn[4].bias.copy_(torch.tensor([0.25, 1.0, 1.0, 0.25, 0.25]))
    q, am = mlp_q(_dev_params(net, dev), x, 5)
    assert bool((q[:, 1] == q[:, 2]).all()) and bool((q[:, 1] > q[:, 0]).all()) and bool((am == 1).all())


# ------------------------------------------------------------------ 3. position independence
def test_q_is_position_independent(dev):
    c = case(130, 33, 18)
    ps = _dev_params(c["online"], dev)
    x = c["s0"].to(dev)
    q, am = mlp_q(ps, x, 18)
    one = torch.cat([mlp_q(ps, x[i:i + 1], 18)[0] for i in range(130)])
    assert torch.equal(one, q)
    rq, ram = mlp_q(ps, x.flip(0).contiguous(), 18)
    assert torch.equal(rq.flip(0), q) and torch.equal(ram.flip(0), am)
    wide = torch.full((130, 33 + 3), 7.0, device=dev)
    wide[:, :33] = x
    sq, sam = mlp_q(ps, wide[:, :33], 18)
    assert wide[:, :33].stride(0) == 36 and torch.equal(sq, q) and torch.equal(sam, am)


@pytest.mark.parametrize("double_q", [True, False])
@pytest.mark.parametrize("with_isw", [False, True])
def test_td_equals_td_huber_on_mlp_q(dev, double_q, with_isw):
    """the forwards inside rth_mlp_dqn_grads are rth_mlp_q's, the TD arithmetic rth_td_huber's"""
    c = case(67, 7, 3, double_q)
    on, tg = _dev_params(c["online"], dev), _dev_params(c["target"], dev)
    isw = c["isw"] if with_isw else None
    td_abs, loss, _ = mlp_grads(on, tg, c, dev, double_q, isw)
    q0 = mlp_q(on, c["s0"].to(dev), 3)[0]
    q1o = mlp_q(on, c["s1"].to(dev), 3)[0] if double_q else None
    q1t = mlp_q(tg, c["s1"].to(dev), 3)[0]
    ref_loss, ref_td, _ = td_huber_forward(q0, q1o, q1t, c["a"].to(dev), c["r"].to(dev), c["done"].to(dev),
                                           None if isw is None else isw.to(dev), GAMMA_N, double_q, want_dq=False)
    assert torch.equal(td_abs, ref_td)
    assert float((td_abs < 1).sum()) > 0 and float((td_abs > 1).sum()) > 0  # both Huber branches
    assert abs(float(loss) - float(ref_loss)) <= 1e-6 * abs(float(ref_loss))
    # calc_loss form (no gradients): the same |td| and loss
    td2, loss2, g2 = mlp_grads(on, tg, c, dev, double_q, isw, backward=False)
    assert torch.equal(td2, td_abs) and torch.equal(loss2, loss)


# ------------------------------------------------------------------ 4. gradients vs fp64 autograd
@pytest.mark.parametrize("double_q", [True, False])
@pytest.mark.parametrize("B,D,A", SHAPES)
def test_grads_vs_fp64_autograd(dev, B, D, A, double_q):
    c = case(B, D, A, double_q)
    on, tg = _dev_params(c["online"], dev), _dev_params(c["target"], dev)
    for isw in (None, c["isw"]):
        td64, loss64, g64 = _loss_and_grads(c["online"], c["target"], c, double_q, isw, torch.float64)
        td32, loss32, g32 = _loss_and_grads(c["online"], c["target"], c, double_q, isw, torch.float32)
        td_abs, loss, grads = mlp_grads(on, tg, c, dev, double_q, isw)
        assert float((td_abs.cpu().double() - td64).abs().max()) <= 1e-5
        assert abs(float(loss) - float(loss64)) <= 1e-5 * max(1.0, abs(float(loss64)))
        names = ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "nn.4.weight", "nn.4.bias"]
        fails = []
        for name, g, ref32, ref64 in zip(names, grads, g32, g64):
            gmax = float(ref64.abs().max())
            e_ours = float((g.cpu().double() - ref64).abs().max()) / gmax
            e_ref = float((ref32.double() - ref64).abs().max()) / gmax
            bound = max(1.5 * e_ref, 1e-6)
            print(f"grads {(B, D, A)} seed {c['seed']} double_q={double_q} isw={isw is not None} {name:12s} "
                  f"|ours - fp64|/max {e_ours:.3e}  |torch fp32 - fp64|/max {e_ref:.3e}  "
                  f"ratio {e_ours / max(e_ref, 1e-30):.2f}  bound {bound:.3e}")
            if not e_ours <= bound:
                fails.append((name, e_ours, e_ref, bound))
        assert not fails, fails


# ------------------------------------------------------------------ 5. every element written
def test_every_output_element_is_written(dev):
    c = case(67, 7, 3)
    on, tg = _dev_params(c["online"], dev), _dev_params(c["target"], dev)
    td_abs, loss, grads = mlp_grads(on, tg, c, dev, True, c["isw"])  # outputs pre-filled with NaN
    assert not bool(torch.isnan(td_abs).any()) and not bool(torch.isnan(loss).any())
    assert [tuple(g.shape) for g in grads] == [(H, 7), (H,), (H, H), (H,), (3, H), (3,)]
    assert not any(bool(torch.isnan(g).any()) for g in grads)
    # grads == NULL: the buffers stay as they are
    keep = [torch.full_like(p, float("nan")) for p in on]
    td2, loss2, _ = mlp_grads(on, tg, c, dev, True, c["isw"], backward=False, grads=keep)
    assert all(bool(torch.isnan(g).all()) for g in keep)
    assert torch.equal(td2, td_abs) and not bool(torch.isnan(loss2).any())


# ------------------------------------------------------------------ 6. bounds
def test_nothing_outside_the_rows_and_columns_is_touched(dev):
    B, D, A, PAD, S = 67, 7, 3, 5, 12345.0
    c = case(B, D, A)
    on, tg = _dev_params(c["online"], dev), _dev_params(c["target"], dev)
    td_c, loss_c, g_c = mlp_grads(on, tg, c, dev, True, c["isw"])
    q_c, am_c = mlp_q(on, c["s0"].to(dev), A)

    def embed(x):  # sentinel rows before / after and sentinel columns between D and the row stride
        big = torch.full((B + 2 * PAD, D + 4), float("nan"), device=dev)
        big[PAD:PAD + B, :D] = x.to(dev)
        return big, big[PAD:PAD + B, :D]

    def guarded(numel, dtype=torch.float32):
        big = torch.full((numel + 2 * 64,), S, device=dev).to(dtype)
        return big, big[64:64 + numel]

    big0, s0 = embed(c["s0"])
    big1, s1 = embed(c["s1"])
    nan0, nan1 = torch.isnan(big0).clone(), torch.isnan(big1).clone()
    gbig, grads = zip(*[guarded(p.numel()) for p in on])
    grads = [g.view(p.shape) for g, p in zip(grads, on)]
    tbig, td = guarded(B)
    lbig, loss = guarded(1)
    size = _lib.lib().rth_mlp_workspace(B, D, H, A) // 4
    wbig, ws = guarded(size)
    mlp_grads(on, tg, c, dev, True, c["isw"], grads=grads, td_abs=td, loss=loss, s0=s0, s1=s1, ws=ws)
    qbig, q = guarded(B * A)
    abig, am = guarded(B, torch.int32)
    mlp_q(on, s0, A, q=q.view(B, A), am=am)
    torch.cuda.synchronize()
    for big, n in [(b, g.numel()) for b, g in zip(gbig, grads)] + [(tbig, B), (lbig, 1), (wbig, size), (qbig, B * A),
                                                                     (abig, B)]:
        assert bool((big[:64] == S).all()) and bool((big[64 + n:] == S).all())
    assert torch.equal(torch.isnan(big0), nan0) and torch.equal(torch.isnan(big1), nan1)  # inputs unchanged
    # ... and nothing read there: the results are those of the compact inputs, bit for bit
    assert torch.equal(td, td_c) and torch.equal(loss, loss_c)
    assert all(torch.equal(a, b) for a, b in zip(grads, g_c))
    assert torch.equal(q.view(B, A), q_c) and torch.equal(am, am_c)
    assert not bool(torch.isnan(td).any()) and not any(bool(torch.isnan(g).any()) for g in grads)


# ------------------------------------------------------------------ 7. determinism
def test_twenty_repetitions_are_bit_identical(dev):
    c = case(130, 33, 18)
    on, tg = _dev_params(c["online"], dev), _dev_params(c["target"], dev)
    first = None
    for _ in range(20):
        td_abs, loss, grads = mlp_grads(on, tg, c, dev, True, c["isw"])
        out = [td_abs, loss, *grads]
        if first is None:
            first = out
        assert all(torch.equal(a, b) for a, b in zip(out, first))


# ------------------------------------------------------------------ 8. unsupported shapes
def test_unsupported_shape_is_an_error_and_launches_nothing(dev):
    ps = [torch.zeros(s, device=dev) for s in [(64, 4), (64,), (64, 64), (64,), (2, 64), (2,)]]
    x = torch.zeros(3, 4, device=dev)
    q = torch.full((3, 2), 5.0, device=dev)
    am = torch.full((3,), 5, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.RethHipError, match="unsupported shape"):
        call("rth_mlp_q", _arr(ps), x.data_ptr(), 4, 3, 4, 64, 2, q.data_ptr(), am.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((q == 5).all()) and bool((am == 5).all())


def test_solver_falls_back_for_an_unsupported_shape(dev, monkeypatch):
    def run():
        torch.manual_seed(5)
        s = DQNSolver(Box(-1, 1, (100,)), Discrete(3), learning_rate=1e-3, device=dev)
        g = torch.Generator().manual_seed(6)
        batch = [torch.randn(32, 100, generator=g).numpy(), torch.randint(0, 3, (32,), generator=g).numpy(),
                 torch.randn(32, generator=g).numpy(), torch.randn(32, 100, generator=g).numpy(),
                 np.zeros(32, np.float32)]
        tds = [s.update(batch) for _ in range(2)]
        return s, tds

    default, td_d = run()
    monkeypatch.setattr(model, "MLP_IMPL", "hip")
    hip, td_h = run()
    assert hip.mlp_impl == "hip" and hip.mlp_impl_active is None and hip.mlp_hip_launches == 0
    assert default.mlp_impl is None and default.mlp_impl_active is None
    assert all(torch.equal(a, b) for a, b in zip(td_d, td_h))
    for p, q in zip(default.q_network.parameters(), hip.q_network.parameters()):
        assert torch.equal(p, q)
