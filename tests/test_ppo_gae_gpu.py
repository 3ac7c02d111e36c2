"""GAE(lambda) on the device PPO loop, on the GPU: rth_ppo_gae_finish (csrc/ppo_actor.hpp) against
ppo_actors.gae on the kernel's own values, its values against fp64 and against rth_ppo_grads' own,
rth_ppo_grads_adv against fp64 autograd and against B = n, rth_ppo_adv_normalize against numpy,
bounds / counters / determinism / argument checks, PpoLoop with gae_lambda as the composition of
its parts and as a replayed graph, that it learns CartPole-v0 at 64 envs x 32 steps, and the example.

Segments are written directly (tests/_ppo_edges.finish_segments: Acrobot's D = 6, A = 3): N = 37
envs at cap 12 with ragged fills 0..12 (five tiles of 8 rows and a tail; a tile holds the bootstrap
row alone where fill % 8 == 0), one env at cap 300 (past one pass of the 256 lanes) and one at cap
4096 (the limit)."""
import functools
import os
import runpy
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from _ppo_edges import COLUMNS, finish_segments
from conftest import ROOT
from reth_amd import _lib
from reth_amd._lib import call
from reth_amd.ppo import ENT_COEF, VF_COEF, PPOSolver, ValueNetwork, _params6
from reth_amd.ppo_actors import HostRollout, VecPpoActors
from reth_amd.solver import Box, Discrete
from test_ppo_gpu import EPS, EPS32, GRAD_NAMES, H, _arr, _check, _nets, _params, case

pytestmark = pytest.mark.gpu

ENV, D, A = "Acrobot-v1", 6, 3
NAN = float("nan")
G = 64  # guard elements around every buffer


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _ulps(got, want):
    """the largest |got - want| in spacings of want (both float32 arrays)"""
    if len(want) == 0:
        return 0.0
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


class Guarded(VecPpoActors):
    """every device buffer between two runs of canaries"""

    def _alloc(self, shape, dtype):
        n = int(np.prod(shape))
        canary = 12345.5 if dtype.is_floating_point else 0x5A5A5A5A
        buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
        buf[G:G + n] = 0
        self.__dict__.setdefault("_guarded", []).append((buf, n, canary))
        return buf[G:G + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n, canary in self._guarded:
            assert (buf[:G] == canary).all() and (buf[G + n:] == canary).all(), (buf.dtype, n)


def _value_net(scale=1.0, seed=0):
    """a random value network on the GPU; scale multiplies its last layer (values in the hundreds)"""
    torch.manual_seed(seed)
    net = ValueNetwork((D,), 1, H)
    with torch.no_grad():
        net.value_layer[4].weight.mul_(float(scale))
    return net.to("cuda")


@pytest.fixture(scope="module")
def value_nets(dev):
    return {1: _value_net(1.0), 256: _value_net(256.0)}


def _ragged_cases(n_envs=37, cap=12, seed=3):
    rng = np.random.default_rng(seed)
    fills = [0, cap, 8, 7, 9, 1] + [int(v) for v in rng.integers(0, cap + 1, n_envs - 6)]
    return [(f, []) for f in fills]


def _dones(pattern, fills, cap, seed=0):
    """float32 [N, cap] done flags: none / every row / the last stored row only / random"""
    N = len(fills)
    dn = np.zeros((N, cap), np.float32)
    if pattern == "every":
        dn[:] = 1.0
    elif pattern == "last":
        for i, f in enumerate(fills):
            if f:
                dn[i, f - 1] = 1.0
    elif pattern == "random":
        dn[:] = np.random.default_rng(seed).random((N, cap)) < 0.2
    else:
        assert pattern == "none"
    return dn


def _load(act, cases, cap, dones, seed=0, zero_rewards=False):
    """finish_segments' random columns with `dones` into the actors, a random cur_obs, nonzero
    `complete` slots (the finish has to zero both)"""
    seg = finish_segments(cases, cap, D=D, A=A, seed=seed, zero_rewards=zero_rewards)
    seg["seg_done"] = torch.as_tensor(dones)
    for k in COLUMNS + ("fill",):
        getattr(act, k).copy_(seg[k])
    g = torch.Generator().manual_seed(100 + seed)
    act.cur_obs.zero_()
    act.cur_obs[:, :D] = torch.randn((act.N, D), generator=g).to(act.device)
    act._complete.fill_(3)
    return seg


def _values(value, obs, env=ENV):
    """value(obs_i) as rth_ppo_gae_finish computes it, bit for bit (the forward does not depend on a
    row's position): the rows as one-row segments of a scratch actor set"""
    n, d = obs.shape
    act = VecPpoActors(env, n, 1, max_episode_steps=8, cap=1, device="cuda")
    act.seg_s.copy_(obs.reshape(n, 1, d))
    act.fill.fill_(1)
    act.finish_gae(value, 0.5, 0.5)
    assert int(act.n_dev) == n
    return act.batch_v[:n].clone()


def _finish_and_check(act, value, seg, gamma, lam, label):
    """one finish_gae; everything but the values' accuracy is checked.  Returns (n, batch_v [n] numpy,
    the largest adv / ret difference from gae() in fp32 ulps)."""
    fills = seg["fill"].numpy()
    n = int(fills.sum())
    v_last = _values(value, act.cur_obs[:, :D].contiguous()).cpu().numpy()
    if act.batch_adv is None:
        act.finish_gae(value, 0.5, 0.5)  # (its further columns exist from the first call on)
    for k in COLUMNS + ("fill",):
        getattr(act, k).copy_(seg[k])
    act._complete.fill_(3)
    gen0, dropped0 = act.gen.clone(), act.dropped.clone()
    for b in act.batch + [act.batch_adv, act.batch_v]:
        b.fill_(-77)
    act.n_dev.fill_(-5)
    (s, a, ret, lp, adv), n_dev = act.finish_gae(value, gamma, lam)
    assert adv is act.batch_adv and int(n_dev) == n, label
    v = act.batch_v
    host = HostRollout(act.N, act.cap, D)
    for k in COLUMNS + ("fill",):
        getattr(host, k)[...] = seg[k].numpy()
    # batch_v in the segments' layout for the oracle
    vseg, off = np.zeros((act.N, act.cap), np.float32), 0
    vn = v[:n].cpu().numpy()
    for i, f in enumerate(fills):
        vseg[i, :f] = vn[off:off + f]
        off += f
    hs, ha, hret, hlp, hadv, hn = host.finish_gae(vseg, v_last, gamma, lam)
    assert hn == n
    assert _bits(s[:n]) == hs.tobytes() and _bits(a[:n]) == ha.tobytes() and _bits(lp[:n]) == hlp.tobytes(), label
    got_adv, got_ret = adv[:n].cpu().numpy(), ret[:n].cpu().numpy()
    assert np.isfinite(got_adv).all() and np.isfinite(got_ret).all() and np.isfinite(vn).all(), label
    ulps = max(_ulps(got_adv, hadv), _ulps(got_ret, hret))
    assert ulps <= 1.0, (label, ulps)
    for b in act.batch + [act.batch_adv, act.batch_v]:  # rows at n and beyond are left as they were
        assert (b[n:] == -77).all(), label
    assert (act.fill == 0).all() and (act._complete == 0).all() and _bits(act.gen) == _bits(gen0 + 1), label
    assert _bits(act.dropped) == _bits(dropped0), label
    for k in COLUMNS:  # the segments' rows are read, not written
        assert _bits(getattr(act, k)) == _bits(seg[k].to(getattr(act, k).dtype)), (label, k)
    return n, vn, ulps


# ---------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("pattern", ["none", "every", "last", "random"])
def test_scan_on_ragged_segments(value_nets, pattern):
    """N = 37, cap 12, ragged fills: gamma x lambda in {0, 0.99, 1} x {0, 0.95, 1}, both value
    networks, and all-zero rewards.  adv / ret against gae() on the kernel's own batch_v: the same
    fp64 operations in the same order, so 0 ulps are expected and 1 is allowed (test_ppo_actors_gpu's
    rule for the finish)."""
    cases, cap = _ragged_cases(), 12
    fills = [f for f, _ in cases]
    act = Guarded(ENV, len(cases), cap, max_episode_steps=8, cap=cap, device="cuda")
    dones = _dones(pattern, fills, cap)
    worst = 0.0
    for scale, value in value_nets.items():
        seg = _load(act, cases, cap, dones, seed=scale)
        for gamma in (0.0, 0.99, 1.0):
            for lam in (0.0, 0.95, 1.0):
                n, _, ulps = _finish_and_check(act, value, seg, gamma, lam, (pattern, scale, gamma, lam))
                worst = max(worst, ulps)
        assert n == sum(fills) and 0 in fills and cap in fills and 8 in fills
    seg = _load(act, cases, cap, dones, seed=5, zero_rewards=True)
    _, _, ulps = _finish_and_check(act, value_nets[1], seg, 0.99, 0.95, (pattern, "zero rewards"))
    act.intact()
    print(f"gae finish, done pattern {pattern!r}: max |adv, ret - gae(batch_v)| = {max(worst, ulps)} fp32 ulps")


@pytest.mark.parametrize("cap", [300, 4096])
def test_scan_on_one_long_segment(value_nets, cap):
    """one env with a full segment: past one pass of the 256 lanes, and the limit of 4096 rows"""
    act = Guarded(ENV, 1, cap, max_episode_steps=8, cap=cap, device="cuda")
    cases = [(cap, [])]
    worst = 0.0
    for pattern in ("none", "every", "last", "random"):
        seg = _load(act, cases, cap, _dones(pattern, [cap], cap, seed=cap), seed=cap)
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.0)):
            worst = max(worst, _finish_and_check(act, value_nets[1], seg, gamma, lam, (cap, pattern, gamma, lam))[2])
    worst = max(worst, _finish_and_check(act, value_nets[256], seg, 0.99, 0.95, (cap, "scaled"))[2])
    act.intact()
    print(f"gae finish, one env at cap {cap}: max |adv, ret - gae(batch_v)| = {worst} fp32 ulps")


@pytest.mark.parametrize("scale", [1, 256])
def test_batch_v_against_fp64(value_nets, scale):
    """the rows' values under the project's bound: |ours - fp64| <= max(1.5 |torch fp32 CPU - fp64|,
    1e-6 max|fp64|)"""
    cases, cap = _ragged_cases(), 12
    act = VecPpoActors(ENV, len(cases), cap, max_episode_steps=8, cap=cap, device="cuda")
    seg = _load(act, cases, cap, _dones("random", [f for f, _ in cases], cap))
    act.finish_gae(value_nets[scale], 0.99, 0.95)
    n = int(act.n_dev)
    rows = torch.cat([seg["seg_s"][i, :f] for i, (f, _) in enumerate(cases)])
    assert _bits(act.batch[0][:n]) == _bits(rows)
    net32 = ValueNetwork((D,), 1, H)
    net32.load_state_dict({k: v.cpu() for k, v in value_nets[scale].state_dict().items()})
    net64 = ValueNetwork((D,), 1, H).double()
    net64.load_state_dict({k: v.cpu().double() for k, v in value_nets[scale].state_dict().items()})
    with torch.no_grad():
        v32, v64 = net32(rows)[:, 0], net64(rows.double())[:, 0]
    fails = []
    _check(f"batch_v, last layer x {scale}", act.batch_v[:n], v32, v64, fails)
    assert not fails, fails
    assert float(v64.abs().max()) > (5 if scale == 256 else 0.01)


# ---------------------------------------------------------------------------- the same v in both kernels
def _grads_call(fn, P, cols, B, Dd, Aa, adv=None, n_dev=None, backward=True):
    """rth_ppo_grads (adv None) or rth_ppo_grads_adv on device columns (s, a, ret, old) -> (the
    twelve gradients, loss_abs [B], loss_mean [1], workspace), outputs pre-filled with NaN"""
    dev = cols[0].device
    s, a, ret, old = cols
    grads = [torch.full_like(p, NAN) for net in P for p in net]
    loss_abs, loss_mean = torch.full((B,), NAN, device=dev), torch.full((1,), NAN, device=dev)
    ws = torch.full((_lib.lib().rth_ppo_workspace(B, Dd, H, Aa) // 4,), NAN, device=dev)
    given = () if adv is None else (adv.data_ptr(),)
    count = () if adv is None else (None if n_dev is None else n_dev.data_ptr(),)
    call(fn, _arr(P[0]), _arr(P[1]), s.data_ptr(), s.stride(0), a.data_ptr(), ret.data_ptr(), *given, old.data_ptr(), B,
         Dd, H, Aa, EPS32, VF_COEF, ENT_COEF, _arr(grads[:6]) if backward else None,
         _arr(grads[6:]) if backward else None, loss_abs.data_ptr(), loss_mean.data_ptr(), ws.data_ptr(), *count,
         _lib.stream_ptr())
    torch.cuda.synchronize()
    return grads, loss_abs, loss_mean, ws


def test_the_finish_and_the_grads_kernel_compute_the_same_value(dev):
    """300 rows from finish_gae (two chunks of 128 rows and a ragged tail) with returns R: rth_ppo_grads
    (ret = R), which forms R - v itself, and rth_ppo_grads_adv (ret = R, adv = fl32(R - batch_v)) give
    the twelve gradients, loss_abs, loss_mean and the workspace's log-probabilities bit for bit"""
    torch.manual_seed(11)
    solver = PPOSolver(Box(-1, 1, (D,)), Discrete(A), device=dev, impl="hip")
    with torch.no_grad():
        solver.value_network.value_layer[4].weight.mul_(16.0)
    cases, cap = [(12, [])] * 25, 12
    act = VecPpoActors(ENV, 25, cap, max_episode_steps=8, cap=cap, device=dev)
    _load(act, cases, cap, _dones("random", [12] * 25, cap))
    (s, a, ret, lp, _), n_dev = act.finish_gae(solver, 0.99, 0.95)
    B = int(n_dev)
    assert B == 300
    g = torch.Generator().manual_seed(4)
    R = torch.randn(B, generator=g).to(dev)
    adv = R - act.batch_v[:B]  # one fp32 subtraction: fl32(R - v)
    P = [[p.detach() for p in _params6(n)] for n in (solver.actor_network, solver.value_network)]
    cols = [s[:B].contiguous(), a[:B].contiguous(), R, lp[:B].contiguous()]
    want = _grads_call("rth_ppo_grads", P, cols, B, D, A)
    got = _grads_call("rth_ppo_grads_adv", P, cols, B, D, A, adv=adv.contiguous())
    for k, (x, y) in enumerate(zip(got[0], want[0])):
        assert torch.isfinite(x).all() and _bits(x) == _bits(y), GRAD_NAMES[k]
    assert _bits(got[1]) == _bits(want[1]) and _bits(got[2]) == _bits(want[2])
    assert _bits(got[3][:B]) == _bits(want[3][:B])
    assert float(adv.abs().max()) > 1.0


# ---------------------------------------------------------------------------- rth_ppo_grads_adv against fp64
ADV_SHAPES = [(1, 4, 2), (64, 4, 2), (257, 64, 18), (300, 6, 3)]


@functools.lru_cache(maxsize=None)
def _given_adv(B):
    """advantages of both signs that have nothing to do with ret - v"""
    adv = torch.randn(B, generator=torch.Generator().manual_seed(77 + B))
    if B > 1:
        adv[0], adv[1] = -abs(adv[0]) - 0.5, abs(adv[1]) + 0.5
    return adv


@functools.lru_cache(maxsize=None)
def adv_ref(shape, dtype):
    """test_ppo_gpu.ref with the advantages given: the reference's expression (Categorical, torch.min,
    F.mse_loss) and autograd on the CPU in `dtype`.  Computed once per shape."""
    c = case(*shape)
    actor, value = _nets(*shape[1:], dtype, c["nets"])
    s, ret, old, adv = c["s"].to(dtype), c["ret"].to(dtype), c["old"].to(dtype), _given_adv(shape[0]).to(dtype)
    dist = Categorical(actor(s))
    logp = dist.log_prob(c["a"])
    v = torch.squeeze(value(s), -1)
    ratios = torch.exp(logp - old)
    rho = ratios.detach()
    ratio_ok = float(torch.minimum((rho - (1 - EPS)).abs(), (rho - (1 + EPS)).abs()).min()) >= 0.05 - 1e-6
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - EPS, 1 + EPS) * adv) + VF_COEF * F.mse_loss(v, ret)
            - ENT_COEF * dist.entropy())
    loss.mean().backward()
    grads = [p.grad for p in _params6(actor)] + [p.grad for p in _params6(value)]
    return dict(logp=logp.detach(), loss_abs=loss.detach().abs(), loss_mean=loss.detach().mean(), grads=grads,
                ratio_ok=ratio_ok)


@pytest.mark.parametrize("shape", ADV_SHAPES, ids=str)
def test_grads_adv_vs_fp64_autograd(dev, shape):
    B, Dd, Aa = shape
    c = case(*shape)
    P = _params(c, dev)
    r64, r32 = adv_ref(shape, torch.float64), adv_ref(shape, torch.float32)
    assert r64["ratio_ok"]
    adv = _given_adv(B).to(dev)
    assert B == 1 or (bool((adv > 0).any()) and bool((adv < 0).any()))
    cols = [c["s"].to(dev), c["a"].to(dev), c["ret"].to(dev), c["old"].to(dev)]
    grads, loss_abs, loss_mean, ws = _grads_call("rth_ppo_grads_adv", P, cols, B, Dd, Aa, adv=adv)
    fails = []
    tag = f"adv {shape} seed {c['seed']} "
    _check(tag + "|loss|", loss_abs, r32["loss_abs"], r64["loss_abs"], fails)
    _check(tag + "loss mean", loss_mean.view(()), r32["loss_mean"], r64["loss_mean"], fails)
    _check(tag + "new logp", ws[:B], r32["logp"], r64["logp"], fails)
    for name, g, g32, g64 in zip(GRAD_NAMES, grads, r32["grads"], r64["grads"]):
        assert g.shape == g64.shape
        _check(tag + name, g, g32, g64, fails)
    assert not fails, fails
    # evaluate only: the same loss, the gradient buffers left alone
    ev = _grads_call("rth_ppo_grads_adv", P, cols, B, Dd, Aa, adv=adv, backward=False)
    assert _bits(ev[1]) == _bits(loss_abs) and _bits(ev[2]) == _bits(loss_mean)
    assert all(bool(torch.isnan(g).all()) for g in ev[0])
    # a device count n < capacity, NaN in every row and advantage beyond n: B = n bit for bit
    capB = B + 21
    wide = [torch.full((capB,) + t.shape[1:], 99 if t.dtype == torch.int64 else NAN, dtype=t.dtype, device=dev)
            for t in cols + [adv]]
    for w, t in zip(wide, cols + [adv]):
        w[:B] = t
    n_dev = torch.tensor([B], dtype=torch.int64, device=dev)
    got = _grads_call("rth_ppo_grads_adv", P, wide[:4], capB, Dd, Aa, adv=wide[4], n_dev=n_dev)
    for k, (x, y) in enumerate(zip(got[0], grads)):
        assert torch.isfinite(x).all() and _bits(x) == _bits(y), GRAD_NAMES[k]
    assert _bits(got[1][:B]) == _bits(loss_abs) and _bits(got[2]) == _bits(loss_mean)
    assert _bits(got[3][:B]) == _bits(ws[:B]) and torch.isnan(got[1][B:]).all()


# ---------------------------------------------------------------------------- normalisation
@pytest.mark.parametrize("n", [0, 1, 2, 257, 8193])
def test_adv_normalize_against_numpy(dev, n):
    """fp64 mean and population std in another summation order move the result by ~n 2^-53 relative,
    far below half an fp32 spacing: only a rounding tie can differ, so 1 fp32 ulp is allowed"""
    B = n + 7
    rng = np.random.default_rng(n)
    x = (3.0 * rng.standard_normal(B) + 0.5).astype(np.float32)
    buf = torch.full((B + 2 * G,), 12345.5, device=dev)
    buf[G:G + B] = torch.as_tensor(x)
    adv = buf[G:G + B]
    n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
    call("rth_ppo_adv_normalize", adv.data_ptr(), B, n_dev.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = adv.cpu().numpy()
    assert np.array_equal(got[n:], x[n:]) and (buf[:G] == 12345.5).all() and (buf[G + B:] == 12345.5).all()
    if n:
        x64 = x[:n].astype(np.float64)
        want = ((x64 - x64.mean()) / (x64.std() + 1e-8)).astype(np.float32)
        ulps = _ulps(got[:n], want)
        print(f"adv normalize n={n}: max difference from numpy fp64 {ulps} fp32 ulps")
        assert np.isfinite(got).all() and ulps <= 1.0
        if n == 1:
            assert got[0] == 0.0
        if n > 2:
            assert abs(float(got[:n].astype(np.float64).mean())) < 1e-6 and abs(float(got[:n].astype(np.float64).std()) - 1) < 1e-6
    # no count: all B rows
    call("rth_ppo_adv_normalize", adv.data_ptr(), B, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert abs(float(adv.double().mean())) < 1e-6 and (buf[:G] == 12345.5).all() and (buf[G + B:] == 12345.5).all()


# ---------------------------------------------------------------------------- determinism, counters, bounds
def test_ten_repetitions_are_bit_identical_and_nothing_is_written_outside(value_nets):
    cases, cap = _ragged_cases(), 12
    fills = [f for f, _ in cases]
    act = Guarded(ENV, len(cases), cap, max_episode_steps=8, cap=cap, device="cuda")
    n_buffers = len(act._guarded)
    first = None
    for rep in range(10):
        seg = _load(act, cases, cap, _dones("random", fills, cap))
        act.n_dev.fill_(-5)
        (s, a, ret, lp, adv), n_dev = act.finish_gae(value_nets[1], 0.99, 0.95, normalize=True)
        out = [t.clone() for t in (s, a, ret, lp, adv, act.batch_v, n_dev)]
        first = out if first is None else first
        for x, y in zip(out, first):
            assert _bits(x) == _bits(y), rep
        assert (act.fill == 0).all() and (act._complete == 0).all() and (act.gen == rep + 1).all()
    assert len(act._guarded) == n_buffers + 2  # batch_adv and batch_v, made by the first call
    assert act.finishes == 10 and act.normalizes == 10 and int(act.n_dev) == sum(fills)
    n = sum(fills)
    assert abs(float(adv[:n].double().mean())) < 1e-6
    act.intact()
    # an empty rollout right behind it: n = 0, nothing written, the counters move
    for b in act.batch + [act.batch_adv, act.batch_v]:
        b.fill_(-77)
    act.finish_gae(value_nets[1], 0.99, 0.95, normalize=True)
    assert int(act.n_dev) == 0 and (act.gen == 11).all()
    for b in act.batch + [act.batch_adv, act.batch_v]:
        assert (b == -77).all()
    act.intact()


def test_steps_then_finish_gae_agree_with_host_rollout(dev):
    """a real rollout: 5 steps of 9 CartPole envs under a time limit of 3 (done rows in every
    segment), the segments as the step kernel leaves them, then finish_gae against HostRollout"""
    torch.manual_seed(2)
    solver = PPOSolver(Box(-1, 1, (4,)), Discrete(2), device=dev, impl="hip")
    act = VecPpoActors("CartPole-v0", 9, 5, seed=7, max_episode_steps=3, cap=5, device=dev)
    for rollout in range(2):
        for _ in range(5):
            act.step(solver)
        assert (act.fill == 5).all() and int(act.dropped.sum()) == 0
        host = HostRollout(9, 5, 4)
        for k in COLUMNS + ("fill",):
            getattr(host, k)[...] = getattr(act, k).cpu().numpy()
        assert host.seg_done.sum() >= 9
        cur = act.current_obs()
        (s, a, ret, lp, adv), n_dev = act.finish_gae(solver, 0.99, 0.95)
        assert int(n_dev) == 45
        v_last = _values(solver, cur, "CartPole-v0").cpu().numpy()
        hs, ha, hret, hlp, hadv, n = host.finish_gae(act.batch_v[:45].cpu().numpy().reshape(9, 5), v_last, 0.99, 0.95)
        assert _bits(s[:n]) == hs.tobytes() and _bits(a[:n]) == ha.tobytes() and _bits(lp[:n]) == hlp.tobytes()
        assert max(_ulps(adv[:n].cpu().numpy(), hadv), _ulps(ret[:n].cpu().numpy(), hret)) <= 1.0
        assert (act.fill == 0).all() and (act.gen == rollout + 1).all()


def test_bad_arguments_are_refused_before_any_launch(value_nets):
    ERR_INVALID = -1
    cases, cap = _ragged_cases(), 12
    act = VecPpoActors(ENV, len(cases), cap, max_episode_steps=8, cap=cap, device="cuda")
    value = value_nets[1]
    act.finish_gae(value, 0.99, 0.95)  # the columns exist
    _load(act, cases, cap, _dones("random", [f for f, _ in cases], cap))
    bufs = act.batch + [act.batch_adv, act.batch_v]
    for b in bufs:
        b.fill_(-77)
    torch.cuda.synchronize()
    before = {k: getattr(act, k).clone() for k in ("fill", "gen", "_complete", "n_dev") + COLUMNS}
    lib, st = _lib.lib(), _lib.stream_ptr()
    vp = act._value_params(value)
    s, a, ret, lp = act.batch
    b = [s.data_ptr(), a.data_ptr(), ret.data_ptr(), act.batch_adv.data_ptr(), act.batch_v.data_ptr(), lp.data_ptr(),
         act.n_dev.data_ptr()]

    def args(**kw):
        x = act._args()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    bad = [dict(env=7), dict(D=4), dict(A=2), dict(H=128), dict(N=0), dict(N=1 << 31), dict(cap=0), dict(cap=-1),
           dict(cap=4097), dict(max_episode_steps=0)]
    bad += [{k: None} for k in ("fill", "complete", "gen", "dropped", "cur_obs", "seg_s", "seg_a", "seg_r", "seg_done",
                                "seg_logp")]
    for kw in bad:
        x = args(**kw)
        assert lib.rth_ppo_gae_finish(_lib.ctypes.byref(x), vp, 0.99, 0.95, *b, st) == ERR_INVALID, kw
        assert b"rth_ppo_gae_finish" in lib.rth_last_error(), kw
    x = args()
    for j in range(7):
        assert lib.rth_ppo_gae_finish(_lib.ctypes.byref(x), vp, 0.99, 0.95, *[None if k == j else p for k, p in enumerate(b)],
                                      st) == ERR_INVALID, j
    for gamma, lam in ((1.5, 0.95), (-0.1, 0.95), (0.99, 1.5), (0.99, -0.5), (NAN, 0.5), (0.5, NAN)):
        assert lib.rth_ppo_gae_finish(_lib.ctypes.byref(x), vp, gamma, lam, *b, st) == ERR_INVALID, (gamma, lam)
    null_value = (_lib.c_vp * 6)(*([act._value_key[0]] * 5 + [None]))
    assert lib.rth_ppo_gae_finish(_lib.ctypes.byref(x), null_value, 0.99, 0.95, *b, st) == ERR_INVALID
    assert lib.rth_ppo_gae_finish(_lib.ctypes.byref(x), None, 0.99, 0.95, *b, st) == ERR_INVALID
    assert lib.rth_ppo_gae_finish(None, vp, 0.99, 0.95, *b, st) == ERR_INVALID
    assert lib.rth_ppo_adv_normalize(None, 5, None, st) == ERR_INVALID and b"rth_ppo_adv_normalize" in lib.rth_last_error()
    assert lib.rth_ppo_adv_normalize(act.batch_adv.data_ptr(), 0, None, st) == ERR_INVALID
    # rth_ppo_grads_adv: the advantage is required, the rest is rth_ppo_grads' checks
    c = case(64, 4, 2)
    P = _params(c, "cuda")
    cols = [c[k].to("cuda") for k in ("s", "a", "ret", "old")]
    la, ws = torch.full((64,), -77.0, device="cuda"), torch.full((64 * 1024,), -77.0, device="cuda")
    head = [_arr(P[0]), _arr(P[1]), cols[0].data_ptr(), 4, cols[1].data_ptr(), cols[2].data_ptr()]
    tail = [EPS32, VF_COEF, ENT_COEF, None, None, la.data_ptr(), None, ws.data_ptr(), None, st]
    adv = cols[2].data_ptr()
    assert lib.rth_ppo_grads_adv(*head, None, cols[3].data_ptr(), 64, 4, H, 2, *tail) == ERR_INVALID
    assert b"rth_ppo_grads_adv" in lib.rth_last_error()
    assert lib.rth_ppo_grads_adv(*head, adv, cols[3].data_ptr(), 0, 4, H, 2, *tail) == ERR_INVALID
    assert lib.rth_ppo_grads_adv(*head, adv, cols[3].data_ptr(), 64, 4, 100, 2, *tail) == ERR_INVALID
    assert lib.rth_ppo_grads_adv(*head, adv, cols[3].data_ptr(), 64, 4, H, 19, *tail) == ERR_INVALID
    assert lib.rth_ppo_grads_adv(*head, adv, None, 64, 4, H, 2, *tail) == ERR_INVALID
    assert b"rth_ppo_grads_adv" in lib.rth_last_error()
    with pytest.raises(ValueError, match="GAE finish runs"):
        act._value_key = None
        act.finish_gae(ValueNetwork((4,), 1, H).to("cuda"), 0.99, 0.95)
    with pytest.raises(ValueError, match="cap = 4097"):
        VecPpoActors(ENV, 2, 5, cap=4097, device="cuda")
    with pytest.raises(ValueError, match="cap = 0"):
        VecPpoActors(ENV, 2, 5, cap=0, device="cuda")
    torch.cuda.synchronize()
    for k, v in before.items():  # nothing ran
        assert _bits(getattr(act, k)) == _bits(v), k
    assert all(bool((t == -77).all()) for t in bufs + [la, ws])


# ---------------------------------------------------------------------------- the loop
def _loop(**kw):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    kw = dict(dict(n_actors=9, horizon=5, max_episode_steps=8, seed=5, gae_lambda=0.95), **kw)
    return PpoLoop(PpoLoopConfig(**kw), device="cuda", impl="hip")


def _same_params(a, b):
    for net in ("actor_network", "value_network"):
        for p, q in zip(_params6(getattr(a, net)), _params6(getattr(b, net))):
            assert _bits(p) == _bits(q), net


def _abi_calls(loop):
    act = loop.actors
    return act.launches + act.finishes + act.normalizes + loop.solver.hip_launches


@pytest.mark.parametrize("normalize", [False, True])
def test_the_gae_loop_is_the_composition_of_its_parts(dev, normalize):
    """3 eager iterations at 9 envs x 5 steps under a time limit of 8 (a short horizon: the default
    loop refuses it); a second actor set stepped and finished by hand and a second solver updated
    with update_device on its dense 5-column batch end with the loop's parameters, bit for bit"""
    loop = _loop(normalize_adv=normalize)
    cfg = loop.cfg
    assert loop.actors.cap == 5 and loop.gae
    other = PPOSolver(Box(-1, 1, (4,)), Discrete(2), k_epochs=cfg.k_epochs, eps_clip=cfg.eps_clip,
                      learning_rate=cfg.learning_rate, device=dev, impl="hip")
    other.sync_weights(loop.solver)
    mine = VecPpoActors(cfg.env, 9, 5, seed=cfg.seed, max_episode_steps=8, cap=5, device=dev)
    for k in range(3):
        loop.iteration()
        for _ in range(5):
            mine.step(other)
        batch, n_dev = mine.finish_gae(other, cfg.gamma, cfg.gae_lambda, normalize)
        n = int(n_dev)
        assert n == 45 and len(batch) == 5
        other.update_device([b[:n].clone() for b in batch])
        _same_params(loop.solver, other)
        for name in ("state", "t_dev", "fill", "gen", "seg_logp", "stats"):
            assert _bits(getattr(loop.actors, name)) == _bits(getattr(mine, name)), (k, name)
        for x, y in zip(batch + [mine.batch_v], loop.actors.batch + [loop.actors.batch_adv, loop.actors.batch_v]):
            assert _bits(x) == _bits(y), k
    assert (loop.iterations, loop.env_steps, loop.updates) == (3, 3 * 9 * 5, 3)
    assert _abi_calls(loop) == 3 * (5 + 1 + int(normalize) + 3 * cfg.k_epochs)
    assert int(loop.actors.dropped.sum()) == 0 and (loop.actors.t_dev == 15).all()
    assert int(loop.actors.stats[:, 0].sum()) > 0  # episodes ended inside the rollouts


@pytest.mark.parametrize("normalize", [False, True])
def test_captured_gae_iterations_equal_eager_ones(dev, normalize):
    eager, graph = _loop(normalize_adv=normalize), _loop(normalize_adv=normalize)
    with pytest.raises(RuntimeError, match="graph_ready"):
        graph.capture()
    eager.run(4)
    graph.iteration()
    graph.capture()
    graph.run(3)
    torch.cuda.synchronize()
    _same_params(eager.solver, graph.solver)
    for k in ("t_dev", "stats", "fill", "state", "gen", "seg_logp", "seg_s", "seg_r", "seg_done", "_complete", "n_dev",
              "batch_adv", "batch_v", "dropped"):
        assert _bits(getattr(eager.actors, k)) == _bits(getattr(graph.actors, k)), k
    for x, y in zip(eager.actors.batch, graph.actors.batch):
        assert _bits(x) == _bits(y)
    for k in ("iterations", "env_steps", "updates"):
        assert getattr(eager, k) == getattr(graph, k), k
    for k in ("pushes", "launches", "finishes", "normalizes"):
        assert getattr(eager.actors, k) == getattr(graph.actors, k), k
    assert _abi_calls(eager) == _abi_calls(graph) == 4 * (5 + 1 + int(normalize) + 3 * eager.cfg.k_epochs)
    assert int(graph.actors.dropped.sum()) == 0 and int(graph.actors.n_dev) == 45


def test_refusals(dev):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    with pytest.raises(ValueError, match="normalize_adv"):
        _loop(gae_lambda=None, horizon=8, normalize_adv=True)
    with pytest.raises(ValueError, match="gae_lambda"):
        _loop(gae_lambda=1.01)
    with pytest.raises(ValueError, match="horizon 0"):
        _loop(horizon=0)
    assert _loop(horizon=1).actors.cap == 1  # any horizon >= 1
    # without gae_lambda: as before
    with pytest.raises(ValueError, match="horizon 7 < max_episode_steps 8"):
        _loop(gae_lambda=None, horizon=7)
    with pytest.raises(ValueError, match="horizon 100 < max_episode_steps 200"):
        _loop(gae_lambda=None, horizon=100, max_episode_steps=None)
    with pytest.raises(ValueError, match="the device envs are"):
        _loop(env="Pendulum-v0")
    with pytest.raises(RuntimeError, match="no torch fallback"):
        PpoLoop(PpoLoopConfig(gae_lambda=0.95, horizon=32), device="cuda", impl="torch")
    assert _loop(gae_lambda=None, horizon=8).actors.cap == 15


def test_it_learns_cartpole_on_short_rollouts(dev):
    """CartPole-v0, 64 envs x 32 steps, lambda 0.95, normalised advantages, 50 iterations, seeds 0 / 1 /
    2: the median of the envs' mean last finished episode length reaches the midpoint between the
    untrained actor's figure (one rollout of 200 steps before any update, measured here) and the
    limit of 200 -- test_ppo_loop_gpu.test_it_learns_cartpole's criterion.  Measured on an MI355X:
    trained 181.4 / 187.7 / 180.6, untrained 22.0 / 26.3 / 22.5 (profiles/r23/ppo_gae.txt): the median
    181.4 against a midpoint of 111.2."""
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    trained, untrained = [], []
    for seed in (0, 1, 2):
        cfg = PpoLoopConfig(n_actors=64, horizon=32, gae_lambda=0.95, normalize_adv=True, seed=seed)
        loop = PpoLoop(cfg, device="cuda", impl="hip")
        untrained.append(loop.rollout_length())
        loop.run(50)
        trained.append(loop.mean_last_length())
        assert int(loop.actors.dropped.sum()) == 0
    print(f"ppo_loop GAE CartPole-v0 64 x 32, 50 iterations, seeds 0/1/2: mean last finished length {trained}, "
          f"untrained {untrained}")
    mid = (float(np.median(untrained)) + 200.0) / 2
    assert max(untrained) < 60
    assert float(np.median(trained)) >= mid, (trained, untrained, mid)


# ---------------------------------------------------------------------------- the example
@pytest.mark.parametrize("graph", [False, True])
def test_example_runs_end_to_end(dev, graph, monkeypatch, capsys):
    path = os.path.join(ROOT, "examples", "cartpole_ppo_gae_hip.py")
    monkeypatch.setattr(sys, "argv", [path, "--updates", "3", "--seed", "1"] + (["--graph"] if graph else []))
    monkeypatch.setattr(sys, "path", list(sys.path))
    runpy.run_path(path, run_name="__main__")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("cartpole_ppo_gae ")][-1]
    fields = dict(f.split("=") for f in line.split()[1:])
    assert fields["updates"] == "3" and fields["seed"] == "1" and fields["graph"] == str(int(graph))
    assert fields["env"] == "CartPole-v0" and fields["gae_lambda"] == "0.95"
    assert int(fields["env_steps"]) == 3 * 64 * 32 and int(fields["episodes"]) >= 64 and fields["dropped"] == "0"
    for k in ("mean_last_len", "untrained_mean_last_len"):
        assert 1 <= float(fields[k]) <= 200
    assert int(fields["hip_launches"]) == 3 * (32 + 1 + 1 + 3 * 4)
