"""rth_ddpg_act / rth_ddpg_critic_grads / rth_ddpg_actor_grads / rth_soft_update (csrc/ddpg.hpp)
against fp64 on the CPU and against themselves (position independence, determinism, bounds), and
DDPGSolver's HIP path against the reference's recorded run, against its torch path and as a
replayed graph.

Shapes are (B, D, Ad, H1, H2).  Inputs of the fp64 comparisons keep the ReLU decisions safe: for
seeds 0..39 the four networks (the reference's initialisation) and the batch are drawn, the
differentiated forwards -- the critic on (s0, a), the actor on s0, the critic on (s0, actor(s0)) --
are computed in fp64, and the first seed is taken at which every hidden pre-activation's magnitude
exceeds 5e-6 (a ReLU that fp32 rounding could flip would compare two different functions).

The error bound is the project's: |ours - fp64| <= max(1.5 |torch fp32 CPU - fp64|, 1e-6 max|fp64|)
per tensor."""
import functools
import os
import runpy
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from reth_amd import _lib
from reth_amd._lib import c_i64, c_vp, call
from reth_amd.ddpg import Actor, Critic, DDPGSolver, generate_ddpg_model
from reth_amd.solver import Box
from test_ddpg_cpu import ACT, NAMES, OBS, check_against_golden

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 4, 4), (5, 3, 1, 400, 300), (64, 3, 1, 400, 300), (67, 7, 2, 36, 20), (130, 17, 6, 64, 128),
          (257, 8, 4, 128, 64), (16, 64, 8, 512, 512)]
GAMMA = float(np.float32(0.99))
MARGIN = 5e-6


def _nets(D, Ad, H1, H2, dtype=torch.float32, like=None):
    """(actor, critic, actor_target, critic_target), optionally copies of `like` in `dtype`"""
    nets = [Actor((D,), (Ad,), h1=H1, h2=H2), Critic((D,), (Ad,), h1=H1, h2=H2), Actor((D,), (Ad,), h1=H1, h2=H2),
            Critic((D,), (Ad,), h1=H1, h2=H2)]
    if like is not None:
        for n, src in zip(nets, like):
            n.to(dtype)
            n.load_state_dict({k: v.to(dtype) for k, v in src.state_dict().items()})
    return nets


def _hidden(net, x, a=None):
    """(output, smallest hidden pre-activation magnitude) of an Actor / Critic forward"""
    z1 = net.fc1(x)
    h = torch.relu(z1)
    z2 = net.fc2(h if a is None else torch.cat((h, a), 1))
    out = net.fc3(torch.relu(z2))
    return (torch.tanh(out) if a is None else out), min(float(z1.abs().min()), float(z2.abs().min()))


@functools.lru_cache(maxsize=None)
def case(B, D, Ad, H1, H2):
    """the first safe seed's networks and batch (CPU tensors; shared, never modified)"""
    for seed in range(40):
        torch.manual_seed(seed)
        nets = _nets(D, Ad, H1, H2)
        s0, s1 = torch.randn(B, D), torch.randn(B, D)
        a = torch.rand(B, Ad) * 4 - 2
        n64 = _nets(D, Ad, H1, H2, torch.float64, nets)
        with torch.no_grad():
            _, m0 = _hidden(n64[1], s0.double(), a.double())
            act64, m1 = _hidden(n64[0], s0.double())
            _, m2 = _hidden(n64[1], s0.double(), act64)
        if min(m0, m1, m2) > MARGIN:
            break
    else:
        raise AssertionError(f"no safe seed in 0..39 for {(B, D, Ad, H1, H2)}")
    g = torch.Generator().manual_seed(1000 + seed)
    r = torch.randn(B, generator=g)
    done = (torch.rand(B, generator=g) < 0.25).float()
    if B > 1:
        done[1] = 1.0
    isw = (0.1 + 0.9 * torch.rand(B, generator=g)).clamp(max=1.0)
    return dict(seed=seed, shape=(B, D, Ad, H1, H2), nets=nets, s0=s0, s1=s1, a=a, r=r, done=done, isw=isw)


def critic_ref(c, isw, dtype):
    """ddpg_solver.py:79-94 with torch ops on the CPU in `dtype`: (|td|, loss, the critic's six gradients)"""
    _, critic, actor_t, critic_t = _nets(*c["shape"][1:], dtype, c["nets"])
    s0, s1, a, r, done = (c[k].to(dtype) for k in ("s0", "s1", "a", "r", "done"))
    with torch.no_grad():
        y = r[:, None] + (1 - done[:, None]) * torch.tensor(GAMMA, dtype=dtype) * critic_t(s1, actor_t(s1))
    td = (critic(s0, a) - y).squeeze(1)
    loss = td.pow(2)
    if isw is not None:
        loss = loss * isw.to(dtype)
    loss = loss.mean()
    loss.backward()
    return td.detach().abs(), loss.detach(), [p.grad for p in critic._params6()]


def actor_ref(c, dtype):
    """ddpg_solver.py:98-101: (actions, loss, the actor's six gradients)"""
    actor, critic, _, _ = _nets(*c["shape"][1:], dtype, c["nets"])
    s0 = c["s0"].to(dtype)
    act = actor(s0)
    loss = (-critic(s0, act)).mean()
    loss.backward()
    return act.detach(), loss.detach(), [p.grad for p in actor._params6()]


def _arr(ts):
    return (c_vp * len(ts))(*[t.data_ptr() for t in ts])


def _dev_params(net, dev):
    return [p.detach().to(dev).contiguous() for p in net._params6()]


def _ws(c, dev):
    return torch.empty(_lib.lib().rth_ddpg_workspace(*c["shape"]) // 4, dtype=torch.float32, device=dev)


def ddpg_act(ps, x, dims, out=None):
    """rth_ddpg_act over the rows of the (possibly row-strided) device matrix x"""
    D, Ad, H1, H2 = dims
    n = x.shape[0]
    out = torch.full((n, Ad), float("nan"), device=x.device) if out is None else out
    assert x.stride(1) == 1
    call("rth_ddpg_act", _arr(ps), x.data_ptr(), x.stride(0), n, D, Ad, H1, H2, out.data_ptr(), _lib.stream_ptr())
    return out


def critic_grads(P, c, dev, isw=None, backward=True, grads=None, td_abs=None, loss=None, s0=None, s1=None, a=None,
                 ws=None):
    """rth_ddpg_critic_grads on the case's batch -> (td_abs, loss, grads); P: the four networks'
    device parameters"""
    B, D, Ad, H1, H2 = c["shape"]
    s0 = c["s0"].to(dev) if s0 is None else s0
    s1 = c["s1"].to(dev) if s1 is None else s1
    a = c["a"].to(dev) if a is None else a
    r, done = c["r"].to(dev), c["done"].to(dev)
    isw = None if isw is None else isw.to(dev)
    grads = [torch.full_like(p, float("nan")) for p in P[1]] if grads is None else grads
    td_abs = torch.full((B,), float("nan"), device=dev) if td_abs is None else td_abs
    loss = torch.full((1,), float("nan"), device=dev) if loss is None else loss
    ws = _ws(c, dev) if ws is None else ws
    call("rth_ddpg_critic_grads", _arr(P[1]), _arr(P[2]), _arr(P[3]), s0.data_ptr(), s0.stride(0), a.data_ptr(),
         a.stride(0), r.data_ptr(), done.data_ptr(), s1.data_ptr(), s1.stride(0),
         isw.data_ptr() if isw is not None else None, B, D, Ad, H1, H2, GAMMA, _arr(grads) if backward else None,
         td_abs.data_ptr(), loss.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return td_abs, loss, grads


def actor_grads(P, c, dev, grads=None, loss=None, s0=None, ws=None):
    """rth_ddpg_actor_grads -> (the internal actions [B, Ad], loss, grads)"""
    B, D, Ad, H1, H2 = c["shape"]
    s0 = c["s0"].to(dev) if s0 is None else s0
    grads = [torch.full_like(p, float("nan")) for p in P[0]] if grads is None else grads
    loss = torch.full((1,), float("nan"), device=dev) if loss is None else loss
    ws = _ws(c, dev) if ws is None else ws
    call("rth_ddpg_actor_grads", _arr(P[0]), _arr(P[1]), s0.data_ptr(), s0.stride(0), B, D, Ad, H1, H2, _arr(grads),
         loss.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return ws[:B * Ad].view(B, Ad).clone(), loss, grads


def _params(c, dev):
    return [_dev_params(n, dev) for n in c["nets"]]


def _check(label, ours, ref32, ref64, fails):
    """the bound of the module docstring on one tensor"""
    scale = float(ref64.abs().max())
    e_ours = float((ours.cpu().double() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    bound = max(1.5 * e_ref, 1e-6 * scale)
    print(f"{label:44s} |ours - fp64| {e_ours:.3e}  |torch fp32 - fp64| {e_ref:.3e}  bound {bound:.3e}  "
          f"max|fp64| {scale:.3e}")
    if not e_ours <= bound:
        fails.append((label, e_ours, e_ref, bound))


# ------------------------------------------------------------------ 1. the actor forward
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_act_vs_fp64(dev, shape):
    c = case(*shape)
    a64, _, _ = actor_ref(c, torch.float64)
    a32, _, _ = actor_ref(c, torch.float32)
    out = ddpg_act(_dev_params(c["nets"][0], dev), c["s0"].to(dev), shape[1:])
    fails = []
    _check(f"act {shape} seed {c['seed']}", out, a32, a64, fails)
    assert not fails, fails
    assert not bool(torch.isnan(out).any()) and float(out.abs().max()) < 1.0


def test_act_is_position_independent(dev):
    shape = (130, 17, 6, 64, 128)
    c = case(*shape)
    ps, x, dims = _dev_params(c["nets"][0], dev), c["s0"].to(dev), shape[1:]
    out = ddpg_act(ps, x, dims)
    one = torch.cat([ddpg_act(ps, x[i:i + 1], dims) for i in range(shape[0])])
    assert torch.equal(one, out)
    assert torch.equal(ddpg_act(ps, x.flip(0).contiguous(), dims).flip(0), out)
    wide = torch.full((shape[0], 17 + 3), 7.0, device=dev)
    wide[:, :17] = x
    assert wide[:, :17].stride(0) == 20 and torch.equal(ddpg_act(ps, wide[:, :17], dims), out)


# ------------------------------------------------------------------ 2. the critic's gradients
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_critic_grads_vs_fp64_autograd(dev, shape):
    c = case(*shape)
    P = _params(c, dev)
    assert shape[0] == 1 or float(c["done"].sum()) >= 1  # terminal rows are present
    fails = []
    for isw in (None, c["isw"]):
        td64, loss64, g64 = critic_ref(c, isw, torch.float64)
        td32, loss32, g32 = critic_ref(c, isw, torch.float32)
        td_abs, loss, grads = critic_grads(P, c, dev, isw)
        tag = f"critic {shape} seed {c['seed']} isw={isw is not None} "
        _check(tag + "|td|", td_abs, td32, td64, fails)
        _check(tag + "loss", loss.view(()), loss32, loss64, fails)
        for name, g, r32, r64 in zip(NAMES, grads, g32, g64):
            assert g.shape == r64.shape
            _check(tag + name, g, r32, r64, fails)
        # the calc_loss form: the same |td| and loss bit for bit, the gradient buffers left alone
        keep = [torch.full_like(p, float("nan")) for p in P[1]]
        td2, loss2, _ = critic_grads(P, c, dev, isw, backward=False, grads=keep)
        assert torch.equal(td2, td_abs) and torch.equal(loss2, loss)
        assert all(bool(torch.isnan(k).all()) for k in keep)
    assert not fails, fails


# ------------------------------------------------------------------ 3. the actor's gradients
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_actor_grads_vs_fp64_autograd(dev, shape):
    c = case(*shape)
    P = _params(c, dev)
    before = [p.clone() for p in P[1]]
    _, _, cgrads = critic_grads(P, c, dev, c["isw"])  # a critic gradient buffer the actor pass must not touch
    ckeep = [g.clone() for g in cgrads]
    a64, loss64, g64 = actor_ref(c, torch.float64)
    a32, loss32, g32 = actor_ref(c, torch.float32)
    act, loss, grads = actor_grads(P, c, dev)
    fails = []
    tag = f"actor {shape} seed {c['seed']} "
    _check(tag + "loss", loss.view(()), loss32, loss64, fails)
    for name, g, r32, r64 in zip(NAMES, grads, g32, g64):
        assert g.shape == r64.shape
        _check(tag + name, g, r32, r64, fails)
    assert not fails, fails
    assert all(torch.equal(a, b) for a, b in zip(P[1], before))
    assert all(torch.equal(a, b) for a, b in zip(cgrads, ckeep))
    # its internal action is rth_ddpg_act's, bit for bit
    assert torch.equal(act, ddpg_act(P[0], c["s0"].to(dev), shape[1:]))


# ------------------------------------------------------------------ 4. the Polyak update
def soft_update(tgt, src, tau):
    call("rth_soft_update", _arr(tgt), _arr(src), (c_i64 * len(tgt))(*[t.numel() for t in tgt]), len(tgt), tau,
         _lib.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("tau", [0.25, 0.001])
def test_soft_update_is_torchs_expression(dev, tau):
    g = torch.Generator().manual_seed(3)
    sizes = [1, 3, 401, 120300]
    tgt_c = [torch.randn(n, generator=g) for n in sizes]
    src_c = [torch.randn(n, generator=g) for n in sizes]
    tgt, src = [t.to(dev) for t in tgt_c], [t.to(dev) for t in src_c]
    for _ in range(2):
        want = [t * (1.0 - tau) + p * tau for t, p in zip(tgt_c, src_c)]  # util.py:24 on the CPU
        want_dev = [t * (1.0 - tau) + p * tau for t, p in zip(tgt, src)]
        soft_update(tgt, src, tau)
        for t, w, wd, p, pc in zip(tgt, want, want_dev, src, src_c):
            assert torch.equal(t.cpu(), w) and torch.equal(t, wd)
            assert torch.equal(p.cpu(), pc)  # sources unchanged
        tgt_c = want
    # the 2-D weights of a network, targets and sources inside guarded buffers
    S = 777.0
    big = torch.full((300 * 401 + 128,), S, device=dev)
    t2 = big[64:64 + 300 * 401].view(300, 401)
    t2.copy_(torch.randn(300, 401, generator=g))
    p2 = torch.randn(300, 401, generator=g).to(dev)
    want = t2 * (1.0 - tau) + p2 * tau
    soft_update([t2], [p2], tau)
    assert torch.equal(t2, want) and bool((big[:64] == S).all()) and bool((big[-64:] == S).all())
    with pytest.raises(_lib.RethHipError, match="n_tensors"):
        call("rth_soft_update", _arr([t2] * 17), _arr([p2] * 17), (c_i64 * 17)(*[1] * 17), 17, tau, _lib.stream_ptr())


# ------------------------------------------------------------------ 5. bounds
def test_nothing_outside_the_rows_columns_and_buffers_is_touched(dev):
    shape = (67, 7, 2, 36, 20)
    B, D, Ad, H1, H2 = shape
    PAD, S = 5, 12345.0
    c = case(*shape)
    P = _params(c, dev)
    td_c, loss_c, g_c = critic_grads(P, c, dev, c["isw"])  # outputs pre-filled with NaN
    act_c, aloss_c, ag_c = actor_grads(P, c, dev)
    out_c = ddpg_act(P[0], c["s0"].to(dev), shape[1:])
    for t in [td_c, loss_c, aloss_c, out_c, act_c, *g_c, *ag_c]:  # every output element is written
        assert not bool(torch.isnan(t).any())
    assert [tuple(g.shape) for g in g_c] == [(H1, D), (H1,), (H2, H1 + Ad), (H2,), (1, H2), (1,)]
    assert [tuple(g.shape) for g in ag_c] == [(H1, D), (H1,), (H2, H1), (H2,), (Ad, H2), (Ad,)]

    def embed(x):  # NaN rows before / after and NaN columns between the width and the row stride
        w = x.shape[1]
        big = torch.full((B + 2 * PAD, w + 4), float("nan"), device=dev)
        big[PAD:PAD + B, :w] = x.to(dev)
        return big, big[PAD:PAD + B, :w]

    def guarded(numel):
        big = torch.full((numel + 2 * 64,), S, device=dev)
        return big, big[64:64 + numel]

    big0, s0 = embed(c["s0"])
    big1, s1 = embed(c["s1"])
    biga, a = embed(c["a"])
    nans = [torch.isnan(b).clone() for b in (big0, big1, biga)]
    gbig, grads = zip(*[guarded(p.numel()) for p in P[1]])
    grads = [g.view(p.shape) for g, p in zip(grads, P[1])]
    abig, agrads = zip(*[guarded(p.numel()) for p in P[0]])
    agrads = [g.view(p.shape) for g, p in zip(agrads, P[0])]
    tbig, td = guarded(B)
    lbig, loss = guarded(1)
    albig, aloss = guarded(1)
    size = _lib.lib().rth_ddpg_workspace(*shape) // 4
    wbig, ws = guarded(size)
    obig, out = guarded(B * Ad)
    critic_grads(P, c, dev, c["isw"], grads=grads, td_abs=td, loss=loss, s0=s0, s1=s1, a=a, ws=ws)
    assert bool((wbig[:64] == S).all()) and bool((wbig[64 + size:] == S).all())
    act, _, _ = actor_grads(P, c, dev, grads=agrads, loss=aloss, s0=s0, ws=ws)
    ddpg_act(P[0], s0, shape[1:], out=out.view(B, Ad))
    torch.cuda.synchronize()
    checks = [(b, g.numel()) for b, g in zip(gbig, grads)] + [(b, g.numel()) for b, g in zip(abig, agrads)]
    for big, n in checks + [(tbig, B), (lbig, 1), (albig, 1), (wbig, size), (obig, B * Ad)]:
        assert bool((big[:64] == S).all()) and bool((big[64 + n:] == S).all())
    for big, nan in zip((big0, big1, biga), nans):  # inputs unchanged
        assert torch.equal(torch.isnan(big), nan)
    # ... and nothing read there: the results are those of the compact inputs, bit for bit
    assert torch.equal(td, td_c) and torch.equal(loss, loss_c) and torch.equal(aloss, aloss_c)
    assert all(torch.equal(x, y) for x, y in zip(grads, g_c)) and all(torch.equal(x, y) for x, y in zip(agrads, ag_c))
    assert torch.equal(out.view(B, Ad), out_c) and torch.equal(act, act_c)


# ------------------------------------------------------------------ 6. determinism
def test_twenty_repetitions_are_bit_identical(dev):
    shape = (130, 17, 6, 64, 128)
    c = case(*shape)
    P = _params(c, dev)
    first = None
    for _ in range(20):
        td_abs, loss, grads = critic_grads(P, c, dev, c["isw"])
        act, aloss, agrads = actor_grads(P, c, dev)
        out = [td_abs, loss, *grads, act, aloss, *agrads, ddpg_act(P[0], c["s0"].to(dev), shape[1:])]
        if first is None:
            first = out
        assert all(torch.equal(x, y) for x, y in zip(out, first))


# ------------------------------------------------------------------ 7. unsupported shapes
def test_unsupported_shape_is_an_error_and_launches_nothing(dev):
    D, Ad, H1, H2 = 3, 1, 1000, 300
    actor = [torch.zeros(s, device=dev) for s in [(H1, D), (H1,), (H2, H1), (H2,), (Ad, H2), (Ad,)]]
    critic = [torch.zeros(s, device=dev) for s in [(H1, D), (H1,), (H2, H1 + Ad), (H2,), (1, H2), (1,)]]
    x, a, col = torch.zeros(3, D, device=dev), torch.zeros(3, Ad, device=dev), torch.zeros(3, device=dev)
    out = torch.full((3, Ad), 5.0, device=dev)
    td, loss = torch.full((3,), 5.0, device=dev), torch.full((1,), 5.0, device=dev)
    grads = [torch.full_like(p, 5.0) for p in critic]
    agrads = [torch.full_like(p, 5.0) for p in actor]
    ws = torch.full((3 * 4096,), 5.0, device=dev)
    sp = _lib.stream_ptr()
    with pytest.raises(_lib.RethHipError, match="unsupported shape.*4..512"):
        call("rth_ddpg_act", _arr(actor), x.data_ptr(), D, 3, D, Ad, H1, H2, out.data_ptr(), sp)
    with pytest.raises(_lib.RethHipError, match="unsupported shape.*4..512"):
        call("rth_ddpg_critic_grads", _arr(critic), _arr(actor), _arr(critic), x.data_ptr(), D, a.data_ptr(), Ad,
             col.data_ptr(), col.data_ptr(), x.data_ptr(), D, None, 3, D, Ad, H1, H2, GAMMA, _arr(grads),
             td.data_ptr(), loss.data_ptr(), ws.data_ptr(), sp)
    with pytest.raises(_lib.RethHipError, match="unsupported shape.*4..512"):
        call("rth_ddpg_actor_grads", _arr(actor), _arr(critic), x.data_ptr(), D, 3, D, Ad, H1, H2, _arr(agrads),
             loss.data_ptr(), ws.data_ptr(), sp)
    with pytest.raises(_lib.RethHipError, match="ldx=2 < D=3"):  # a row stride below the width
        call("rth_ddpg_act", _arr(actor), x.data_ptr(), D - 1, 3, D, Ad, 400, H2, out.data_ptr(), sp)
    torch.cuda.synchronize()
    for t in [out, td, loss, ws, *grads, *agrads]:
        assert bool((t == 5).all())


# ------------------------------------------------------------------ 8. the solver
def _golden_solver(g, dev, **kw):
    torch.manual_seed(int(g["seed"]))
    return DDPGSolver(OBS, ACT, device=dev, **kw)


def test_solver_hip_reproduces_the_golden(dev, golden):
    g = golden("ddpg_pendulum_b64.npz")
    solver = _golden_solver(g, dev, impl="hip")
    assert solver.impl_active == "hip" and solver.hip_launches == 0
    check_against_golden(solver, g)
    assert solver.hip_launches == 3 * 3 + 4  # three ABI calls per update, one per act
    assert _golden_solver(g, dev).impl_active == "hip"  # the default takes the kernels on a GPU


def test_solver_hip_agrees_with_torch_path(dev, golden):
    g = golden("ddpg_pendulum_b64.npz")
    hip, ref = _golden_solver(g, dev, impl="hip"), _golden_solver(g, dev, impl="torch")
    assert (hip.impl_active, ref.impl_active) == ("hip", "torch")
    batch = [torch.as_tensor(g[k], device=dev) for k in ("s0", "a", "r", "s1", "done")]
    w = torch.as_tensor(g["w"], device=dev)
    assert torch.allclose(hip.calc_loss(batch), ref.calc_loss(batch), rtol=1e-5, atol=1e-6)
    for k in range(5):
        a, b = hip.update(batch, weights=w), ref.update(batch, weights=w)
        print(f"update {k}: max |hip - torch| {float((a - b).abs().max()):.3e} (|td| up to {float(b.max()):.2f})")
        assert a.shape == (64,) and torch.allclose(a, b, rtol=1e-5, atol=1e-6), k
    x = torch.as_tensor(g["act_states"], device=dev)
    assert torch.allclose(hip.act_batch(x), ref.act_batch(x), rtol=1e-5, atol=1e-6)
    for name in ("actor", "critic", "actor_target", "critic_target"):
        for (k, p), q in zip(getattr(hip, name).state_dict().items(), getattr(ref, name).state_dict().values()):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), (name, k)
    assert ref.hip_launches == 0 and hip.hip_launches == 1 + 5 * 3 + 1


def test_captured_update_replays(dev, golden):
    g = golden("ddpg_pendulum_b64.npz")
    eager, graph = _golden_solver(g, dev, impl="hip"), _golden_solver(g, dev, impl="hip")
    batch = [torch.as_tensor(g[k], device=dev).contiguous() for k in ("s0", "a", "r", "s1", "done")]
    w = torch.as_tensor(g["w"], device=dev)
    for s in (eager, graph):  # one eager update each: every persistent buffer exists
        s.cast_actions_to_long = False
        s.update_device(batch, weights=w)
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    td = eager.update_device(batch, weights=w)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n0  # update_device allocates nothing
    want = [td.clone()] + [eager.update_device(batch, weights=w).clone() for _ in range(2)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(cg, stream=stream):
            out = graph.update_device(batch, weights=w)
    torch.cuda.current_stream().wait_stream(stream)
    for k in range(3):
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[k]), k
    for name in ("actor", "critic", "actor_target", "critic_target"):
        for p, q in zip(getattr(graph, name).parameters(), getattr(eager, name).parameters()):
            assert torch.equal(p, q), name
    for a, b in ((graph.actor_optimizer, eager.actor_optimizer), (graph.critic_optimizer, eager.critic_optimizer)):
        assert int(a._step) == int(b._step) == 4


def test_solver_unsupported_shape(dev):
    def models():
        torch.manual_seed(5)
        return generate_ddpg_model(OBS, ACT, 1e-4, 1e-3, h1=1000)

    with pytest.raises(ValueError, match="impl='hip'.*4..512"):
        DDPGSolver(OBS, ACT, models=models(), device=dev, impl="hip")
    s = DDPGSolver(OBS, ACT, models=models(), device=dev)
    assert s.impl is None and s.impl_active == "torch"
    g = torch.Generator().manual_seed(6)
    batch = [torch.randn(32, 3, generator=g), torch.rand(32, 1, generator=g), torch.randn(32, generator=g),
             torch.randn(32, 3, generator=g), torch.zeros(32)]
    td = s.update(batch)
    assert td.shape == (32,) and bool(torch.isfinite(td).all()) and s.hip_launches == 0
    assert s.act(np.zeros(3)).shape == (1,) and s.hip_launches == 0
    with pytest.raises(ValueError, match="float32"):
        DDPGSolver(OBS, ACT, models={k: (v.double() if isinstance(v, torch.nn.Module) else v)
                                     for k, v in generate_ddpg_model(OBS, ACT, 1e-4, 1e-3).items()},
                   device=dev, impl="hip")


def test_replay_buffer_from_the_example_config(dev):
    from reth_amd import presets
    from reth_amd.buffer import PrioritizedBuffer

    buf = presets.get_replay_buffer(os.path.join(ROOT, "examples", "pendulum_ddpg.yaml"), device=dev)
    assert isinstance(buf, PrioritizedBuffer) and buf.capacity == 100000


# ------------------------------------------------------------------ 9. the example
@pytest.mark.parametrize("impl", ["hip", "torch"])
def test_example_runs_end_to_end(dev, impl, monkeypatch, capsys):
    path = os.path.join(ROOT, "examples", "pendulum_ddpg_hip.py")
    monkeypatch.setattr(sys, "argv", [path, "--impl", impl, "--steps", "300", "--seed", "1"])
    monkeypatch.setattr(sys, "path", list(sys.path))
    runpy.run_path(path, run_name="__main__")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("pendulum_ddpg ")][-1]
    fields = dict(f.split("=") for f in line.split()[1:])
    assert fields["impl"] == impl and fields["steps"] == "300" and fields["seed"] == "1"
    assert int(fields["episodes"]) == (1000 + 300 * 64) // 200
    assert np.isfinite(float(fields["mean_return_last10"])) and float(fields["random_policy"]) < 0
    assert (int(fields["hip_launches"]) > 300 * 3) == (impl == "hip")
