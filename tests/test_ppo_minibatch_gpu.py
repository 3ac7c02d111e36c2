"""Shuffled minibatch epochs for device PPO, on the GPU: rth_ppo_shuffle (csrc/ppo_shuffle.hpp)
against the numpy restatement (reth_amd.ppo.minibatch_perm) -- the permutation, forced ties, the
gather bit for bit, the counter, bounds and argument checks --, its slices through the unchanged
gradient kernels against B = n on the gathered rows, PPOSolver(n_minibatches) as the hand composition
and against its torch path, PpoLoop with n_minibatches as the composition of its parts and as a
replayed graph that reshuffles, that it learns CartPole-v0, and the example.

Every output buffer of the kernel is filled with canaries, guards included, and compared whole
against an expectation built on the host: what is no position's destination keeps its canary."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from reth_amd import _lib
from reth_amd._lib import call
from reth_amd.ppo import ENT_COEF, VF_COEF, PPOSolver, _params6, minibatch_perm
from reth_amd.ppo_actors import VecPpoActors
from reth_amd.solver import Box, Discrete
from test_ppo_cpu import ACT, NETS, OBS, golden_batch, golden_solver
from test_ppo_gae_gpu import _given_adv
from test_ppo_gpu import EPS32, GRAD_NAMES, H, _arr, _close, _params, case

pytestmark = pytest.mark.gpu

G = 64  # guard elements around every buffer
NAN = float("nan")
CANARY = {np.float32: 12345.5, np.int64: 0x5A5A5A5A, np.int32: 0x5A5A5A5A}
ERR_INVALID = -1
SEED = 2 ** 40 + 12345  # (both key words in use)
LEARNING_RATE = 0.01  # the learning test's (its docstring)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _float_bits(rng, shape):
    """float32 values of every kind: random bit patterns (NaNs with payloads, infinities, subnormals)"""
    x = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return x


class Shuffle:
    """one rth_ppo_shuffle problem: a batch of capacity B whose first n rows count (n_dev given iff
    with_count), its guarded outputs, and the host's expectation"""

    OUT = ("mb_s", "mb_a", "mb_ret", "mb_adv", "mb_logp", "mb_n", "perm", "ws")

    def __init__(self, B, n, D, K, with_count=True, lds=None, with_adv=True, seed=0, dev="cuda"):
        assert with_count or n == B
        rng = np.random.default_rng(1000 * B + 10 * K + seed)
        self.B, self.n, self.D, self.K, self.lds, self.with_adv = B, n, D, K, D if lds is None else lds, with_adv
        self.Mcap = -(-B // K)
        src = dict(s=_float_bits(rng, (B, self.lds)), a=rng.integers(-2 ** 62, 2 ** 62, B, dtype=np.int64),
                   ret=_float_bits(rng, B), adv=_float_bits(rng, B), logp=_float_bits(rng, B))
        for k in ("ret", "adv", "logp"):
            if n > 1:  # -0.0 and a NaN with a payload
                src[k].view(np.uint32)[:2] = [0x80000000, 0x7FC12345]
            src[k][n:] = np.float32(NAN)  # rows at n and beyond never appear
        src["s"][n:] = np.float32(NAN)
        src["a"][n:] = 99
        self.src = src
        self.dev_src = {k: torch.as_tensor(v).to(dev) for k, v in src.items()}
        for k, v in self.dev_src.items():
            assert _bits(v) == src[k].tobytes()
        self.n_dev = torch.tensor([n], dtype=torch.int64, device=dev) if with_count else None
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        R = K * self.Mcap
        self.shapes = dict(mb_s=(R * D, np.float32), mb_a=(R, np.int64), mb_ret=(R, np.float32), mb_adv=(R, np.float32),
                           mb_logp=(R, np.float32), mb_n=(K, np.int64), perm=(B, np.int32),
                           ws=(_lib.lib().rth_ppo_shuffle_workspace(B) // 8, np.int64))
        self.buf = {}
        for k, (size, dt) in self.shapes.items():
            self.buf[k] = torch.as_tensor(np.full(size + 2 * G, CANARY[dt], dtype=dt)).to(dev)
        self.dev = dev

    def fill(self):
        for k, (size, dt) in self.shapes.items():
            self.buf[k].fill_(CANARY[dt])

    def args(self, keys=None, **kw):
        d, b = self.dev_src, {k: v[G:].data_ptr() for k, v in self.buf.items()}
        a = dict(s=d["s"].data_ptr(), lds=self.lds, a=d["a"].data_ptr(), ret=d["ret"].data_ptr(),
                 adv=d["adv"].data_ptr() if self.with_adv else None, logp=d["logp"].data_ptr(), B=self.B,
                 n_dev=None if self.n_dev is None else self.n_dev.data_ptr(), D=self.D, K=self.K, seed=SEED,
                 counter=self.counter.data_ptr(), keys=None if keys is None else keys.data_ptr(), mb_s=b["mb_s"],
                 mb_a=b["mb_a"], mb_ret=b["mb_ret"], mb_adv=b["mb_adv"] if self.with_adv else None, mb_logp=b["mb_logp"],
                 mb_n=b["mb_n"], perm=b["perm"], ws=b["ws"], stream=_lib.stream_ptr())
        a.update(kw)
        return list(a.values())

    def run(self, counter=0, keys=None):
        """fill the outputs with canaries, set the counter, one call; the device's key tensor is kept alive"""
        self.fill()
        self.counter.fill_(counter)
        self._keys = None if keys is None else torch.as_tensor(np.asarray(keys, dtype=np.uint64).view(np.int64)).to(self.dev)
        call("rth_ppo_shuffle", *self.args(self._keys))
        torch.cuda.synchronize()

    def expect(self, counter=0, keys=None):
        """every output buffer, guards and all, as the host builds it (the workspace: its guards only)"""
        n, K, D, Mcap = self.n, self.K, self.D, self.Mcap
        perm, sizes = minibatch_perm(SEED, counter, n, K, keys=keys)
        M = -(-n // K)
        q = np.arange(n)
        dst = (q // max(M, 1)) * Mcap + q % max(M, 1)
        out = {k: np.full(size + 2 * G, CANARY[dt], dtype=dt) for k, (size, dt) in self.shapes.items()}
        view = {k: v[G:G + self.shapes[k][0]] for k, v in out.items()}
        view["mb_s"].reshape(K * Mcap, D)[dst] = self.src["s"][perm, :D]
        for k in ("a", "ret", "logp") + (("adv",) if self.with_adv else ()):
            view["mb_" + k][dst] = self.src[k][perm]
        view["mb_n"][:] = sizes
        view["perm"][:n] = perm
        return out, perm, sizes

    def check(self, counter=0, keys=None, label=None):
        want, perm, sizes = self.expect(counter, keys)
        for k in self.OUT:
            got = self.buf[k].cpu().numpy()
            if k == "ws":  # the keys' scratch: only its guards
                assert got[:G].tobytes() == want[k][:G].tobytes() and got[-G:].tobytes() == want[k][-G:].tobytes(), label
            else:
                assert got.tobytes() == want[k].tobytes(), (label, k)
        assert int(self.counter) == counter + 1, label
        for k, v in self.dev_src.items():  # the batch is read, not written
            assert _bits(v) == self.src[k].tobytes(), (label, k)
        return perm, sizes

    def snapshot(self):
        return {k: _bits(v) for k, v in self.buf.items() if k != "ws"}


# ---------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257, 1000, 8193])
def test_permutation_and_counts_are_the_restatements(dev, n):
    """K in {1, 2, 4, 7} where K <= B; B = n without a device count and B = n + 37 with one; counters 0,
    5 and 2^32 + 1.  perm, mb_n and every gathered column equal the host's, perm[n..B) and every row
    that is no destination keep their canary."""
    runs = 0
    for K in (1, 2, 4, 7):
        for B, with_count in ((n, False), (n + 37, True)):
            if B < K or B < 1:
                continue
            sh = Shuffle(B, n, 4, K, with_count=with_count)
            for counter in (0, 5, 2 ** 32 + 1):
                sh.run(counter)
                perm, sizes = sh.check(counter, label=(n, K, B, counter))
                assert sorted(perm.tolist()) == list(range(n)) and int(sizes.sum()) == n
                runs += 1
    assert runs >= (12 if n >= 7 else 3)


@pytest.mark.parametrize("n", [257, 513])
def test_forced_ties_keep_their_order(dev, n):
    sh = Shuffle(n + 5, n, 4, 4)
    pad = np.zeros(5, np.uint64)  # (keys at n and beyond are not read into the order)
    equal = np.full(n, 2 ** 63 + 7, np.uint64)
    sh.run(3, keys=np.concatenate([equal, pad]))
    perm, _ = sh.check(3, keys=equal, label="all equal")
    assert np.array_equal(perm, np.arange(n))
    desc = np.uint64(2 ** 64 - 1) - np.arange(n, dtype=np.uint64)
    sh.run(3, keys=np.concatenate([desc, pad]))
    perm, _ = sh.check(3, keys=desc, label="descending")
    assert np.array_equal(perm, np.arange(n)[::-1])
    pairs = np.repeat(np.arange(n, 0, -1, dtype=np.uint64), 2)[:n]  # (k, k, k - 1, k - 1, ...): descending blocks of two
    sh.run(3, keys=np.concatenate([pairs, pad]))
    perm, _ = sh.check(3, keys=pairs, label="pairs")
    first = n % 2  # the odd row out has the smallest key alone
    assert perm[0] == n - 1 if first else True
    body = perm[first:].reshape(-1, 2)
    assert (body[:, 0] + 1 == body[:, 1]).all() and (np.diff(body[:, 0]) == -2).all()


# ---------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("D", [2, 4, 6, 64])
def test_gather_is_bit_for_bit(dev, D):
    """dense and strided sources (lds = D + 3), with and without the advantage column, a device count
    below the capacity: NaN payloads and -0.0 arrive as they were, NaN rows at n and beyond never do"""
    for lds in (D, D + 3):
        for with_adv in (True, False):
            sh = Shuffle(300, 263, D, 4, lds=lds, with_adv=with_adv, seed=D)
            sh.run(7)
            sh.check(7, label=(D, lds, with_adv))
            got = sh.buf["mb_ret"][G:G + 4 * sh.Mcap].cpu().numpy().view(np.uint32)
            assert (got == 0x80000000).sum() >= 1 and (got == 0x7FC12345).sum() >= 1
            if not with_adv:
                assert (sh.buf["mb_adv"] == CANARY[np.float32]).all()


# ---------------------------------------------------------------------------- the counter
def test_counter_advances_by_one_and_repetitions_are_identical(dev):
    sh = Shuffle(1037, 1000, 4, 4)
    keys = np.random.default_rng(1).integers(0, 50, 1037, dtype=np.uint64)  # many ties
    for rep in range(3):  # with keys_in the counter moves all the same
        sh.fill()
        before = int(sh.counter)
        dev_keys = torch.as_tensor(keys.view(np.int64)).to(dev)
        call("rth_ppo_shuffle", *sh.args(dev_keys))
        torch.cuda.synchronize()
        assert int(sh.counter) == before + 1 == rep + 1
    first = None
    for rep in range(10):
        sh.run(2 ** 32 + 1)
        snap = sh.snapshot()
        first = snap if first is None else first
        assert snap == first and int(sh.counter) == 2 ** 32 + 2, rep
    sh.check(2 ** 32 + 1)
    # successive calls walk the counter: each pass its own order
    sh.run(11)
    a = sh.buf["perm"][G:G + 1000].clone()
    sh.fill()
    call("rth_ppo_shuffle", *sh.args())
    torch.cuda.synchronize()
    assert int(sh.counter) == 13 and not torch.equal(a, sh.buf["perm"][G:G + 1000])
    assert np.array_equal(sh.buf["perm"][G:G + 1000].cpu().numpy(), minibatch_perm(SEED, 12, 1000, 4)[0])


# ---------------------------------------------------------------------------- slices through the gradient kernels
def _grads(P, s, lds, a, ret, adv, old, cap, Dd, Aa, n_dev=None):
    """rth_ppo_grads_adv (adv given) or rth_ppo_grads_n / rth_ppo_grads on device pointers -> (the twelve
    gradients, loss_abs [cap], loss_mean [1]), outputs pre-filled with NaN"""
    grads = [torch.full_like(p, NAN) for net in P for p in net]
    loss_abs, loss_mean = torch.full((cap,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    ws = torch.full((_lib.lib().rth_ppo_workspace(cap, Dd, H, Aa) // 4,), NAN, device="cuda")
    fn = "rth_ppo_grads_adv" if adv is not None else ("rth_ppo_grads" if n_dev is None else "rth_ppo_grads_n")
    given = () if adv is None else (adv,)
    count = () if fn == "rth_ppo_grads" else (n_dev,)
    call(fn, _arr(P[0]), _arr(P[1]), s, lds, a, ret, *given, old, cap, Dd, H, Aa, EPS32, VF_COEF, ENT_COEF, _arr(grads[:6]),
         _arr(grads[6:]), loss_abs.data_ptr(), loss_mean.data_ptr(), ws.data_ptr(), *count, _lib.stream_ptr())
    torch.cuda.synchronize()
    return grads, loss_abs, loss_mean


def _shuffled_case(n, K, D, A, with_adv, dev):
    """test_ppo_gpu.case's batch of n rows at capacity n + 11 (the rows beyond: NaN), shuffled"""
    c = case(n, D, A)
    B = n + 11
    sh = Shuffle(B, n, D, K, with_adv=with_adv)
    cols = dict(s=c["s"], a=c["a"], ret=c["ret"], logp=c["old"], adv=_given_adv(n))
    for k, v in cols.items():
        sh.src[k][:n] = v.numpy()
        sh.dev_src[k].copy_(torch.as_tensor(sh.src[k]))
    sh.run(4)
    perm, sizes = sh.check(4, label=(n, K, D, A))
    return c, sh, perm, sizes


@pytest.mark.parametrize("shape,want_sizes", [((300, 4, 6, 3), [75] * 4), ((45, 4, 4, 2), [12, 12, 12, 9]),
                                              ((3, 4, 4, 2), [1, 1, 1, 0])], ids=str)
def test_slices_through_grads_adv_equal_the_gathered_rows(dev, shape, want_sizes):
    """slice m of the shuffled copy, capacity Mcap and the device count mb_n + m, against
    rth_ppo_grads_adv(B = mb_n[m]) on the same rows gathered on the host: twelve gradients, |loss| and
    the loss mean bit for bit; an empty slice writes zero gradients and a zero mean"""
    n, K, D, A = shape
    c, sh, perm, sizes = _shuffled_case(n, K, D, A, True, dev)
    assert sizes.tolist() == want_sizes
    P = _params(c, dev)
    Mcap, M = sh.Mcap, -(-n // K)
    view = lambda k, m, w=1: sh.buf[k][G + m * Mcap * w:].data_ptr()
    for m in range(K):
        got = _grads(P, view("mb_s", m, D), D, view("mb_a", m), view("mb_ret", m), view("mb_adv", m), view("mb_logp", m),
                     Mcap, D, A, n_dev=sh.buf["mb_n"][G + m:].data_ptr())
        size = int(sizes[m])
        if size == 0:
            assert all(bool((g == 0).all()) for g in got[0]) and float(got[2]) == 0.0 and torch.isnan(got[1]).all()
            continue
        rows = torch.as_tensor(perm[m * M:m * M + size], device=dev)
        h = {k: v[rows].contiguous() for k, v in sh.dev_src.items()}
        want = _grads(P, h["s"].data_ptr(), D, h["a"].data_ptr(), h["ret"].data_ptr(), h["adv"].data_ptr(),
                      h["logp"].data_ptr(), size, D, A, n_dev=None)
        for k, (x, y) in enumerate(zip(got[0], want[0])):
            assert torch.isfinite(x).all() and _bits(x) == _bits(y), (m, GRAD_NAMES[k])
        assert _bits(got[1][:size]) == _bits(want[1]) and _bits(got[2]) == _bits(want[2]), m
        assert torch.isnan(got[1][size:]).all() and float(want[2]) != 0.0


def test_slices_through_grads_n_on_a_four_column_batch(dev):
    n, K, D, A = 45, 4, 4, 2
    c, sh, perm, sizes = _shuffled_case(n, K, D, A, False, dev)
    P = _params(c, dev)
    Mcap, M = sh.Mcap, 12
    for m in range(K):
        off = G + m * Mcap
        got = _grads(P, sh.buf["mb_s"][G + m * Mcap * D:].data_ptr(), D, sh.buf["mb_a"][off:].data_ptr(),
                     sh.buf["mb_ret"][off:].data_ptr(), None, sh.buf["mb_logp"][off:].data_ptr(), Mcap, D, A,
                     n_dev=sh.buf["mb_n"][G + m:].data_ptr())
        size = int(sizes[m])
        rows = torch.as_tensor(perm[m * M:m * M + size], device=dev)
        h = {k: v[rows].contiguous() for k, v in sh.dev_src.items()}
        want = _grads(P, h["s"].data_ptr(), D, h["a"].data_ptr(), h["ret"].data_ptr(), None, h["logp"].data_ptr(), size,
                      D, A)
        for k, (x, y) in enumerate(zip(got[0], want[0])):
            assert torch.isfinite(x).all() and _bits(x) == _bits(y), (m, GRAD_NAMES[k])
        assert _bits(got[1][:size]) == _bits(want[1]) and _bits(got[2]) == _bits(want[2]), m


# ---------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch(dev):
    lib = _lib.lib()
    sh = Shuffle(300, 263, 4, 4, lds=7)
    sh.fill()
    sh.counter.fill_(17)
    torch.cuda.synchronize()
    before = sh.snapshot()
    bad = [{k: None} for k in ("s", "a", "ret", "logp", "counter", "mb_s", "mb_a", "mb_ret", "mb_logp", "mb_n", "perm",
                               "ws")]
    bad += [dict(lds=3), dict(adv=None), dict(mb_adv=None), dict(D=0), dict(D=65, lds=65), dict(K=0), dict(K=65),
            dict(K=301), dict(B=0), dict(B=65537), dict(B=3, K=4), dict(D=-1), dict(K=-4), dict(B=-300)]
    for kw in bad:
        assert lib.rth_ppo_shuffle(*sh.args(**kw)) == ERR_INVALID, kw
        assert b"rth_ppo_shuffle" in lib.rth_last_error(), kw
    assert lib.rth_ppo_shuffle_workspace(0) < 0 and lib.rth_ppo_shuffle_workspace(65537) < 0
    assert b"rth_ppo_shuffle_workspace" in lib.rth_last_error()
    assert lib.rth_ppo_shuffle_workspace(65536) >= 65536 * 8
    # the limits themselves are taken
    assert lib.rth_ppo_shuffle(*sh.args(n_dev=None)) == 0
    torch.cuda.synchronize()
    assert int(sh.counter) == 18
    sh.fill()
    sh.counter.fill_(17)
    torch.cuda.synchronize()
    for kw in bad:
        assert lib.rth_ppo_shuffle(*sh.args(**kw)) == ERR_INVALID, kw
    torch.cuda.synchronize()
    assert sh.snapshot() == before and int(sh.counter) == 17  # nothing ran
    assert (sh.buf["ws"] == CANARY[np.int64]).all()


# ---------------------------------------------------------------------------- the solver
def _batch5(B, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, 4, generator=g)
    a = torch.randint(0, 2, (B,), generator=g)
    ret, adv = torch.randn(B, generator=g), torch.randn(B, generator=g)
    old = -torch.rand(B, generator=g) - 0.3
    s[n:], ret[n:], adv[n:], old[n:] = NAN, NAN, NAN, NAN
    return [t.to(dev) for t in (s, a, ret, old, adv)]


def _same_params(a, b):
    for net in ("actor_network", "value_network"):
        for p, q in zip(_params6(getattr(a, net)), _params6(getattr(b, net))):
            assert torch.isfinite(p).all() and _bits(p) == _bits(q), net


def _solver(dev, seed=3, **kw):
    torch.manual_seed(seed)
    return PPOSolver(OBS, ACT, device=dev, **kw)


@pytest.mark.parametrize("B,n", [(45, 45), (321, 300)])
def test_solver_hip_path_is_the_hand_composition(dev, B, n):
    """update_device with n_minibatches = 4 against the same ABI calls made here: per epoch one
    rth_ppo_shuffle into buffers of this test, then per slice rth_ppo_grads_adv and the two Adam steps"""
    K, D, A = 4, 4, 2
    solver, hand = _solver(dev, impl="hip", n_minibatches=K), _solver(dev, impl="hip")
    assert solver.seed == hand.seed and solver.hip_launches == 0 and hand.n_minibatches == 1
    batch = _batch5(B, n, dev)
    n_rows = None if n == B else torch.tensor([n], dtype=torch.int64, device=dev)
    out = solver.update_device(batch, n_rows=n_rows)
    assert solver.hip_launches == solver.k_epochs * 13 and solver.shuffle_calls == solver.k_epochs == 4
    Mcap, M = -(-B // K), -(-n // K)
    assert out.shape == (K * Mcap,) and solver.last_perm.shape == (B,) and solver.last_perm.dtype == torch.int32
    s, a, ret, old, adv = batch
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    mb = dict(s=z((K * Mcap, D)), a=z(K * Mcap, torch.int64), ret=z(K * Mcap), adv=z(K * Mcap), logp=z(K * Mcap),
              n=z(K, torch.int64), perm=z(B, torch.int32), loss=z(K * Mcap), mean=z(1))
    ws = z(_lib.lib().rth_ppo_shuffle_workspace(B) // 4)
    gws = z(_lib.lib().rth_ppo_workspace(Mcap, D, H, A) // 4)
    counter = z(1, torch.int64)
    for epoch in range(4):
        call("rth_ppo_shuffle", s.data_ptr(), D, a.data_ptr(), ret.data_ptr(), adv.data_ptr(), old.data_ptr(), B,
             None if n_rows is None else n_rows.data_ptr(), D, K, hand.seed, counter.data_ptr(), None,
             mb["s"].data_ptr(), mb["a"].data_ptr(), mb["ret"].data_ptr(), mb["adv"].data_ptr(), mb["logp"].data_ptr(),
             mb["n"].data_ptr(), mb["perm"].data_ptr(), ws.data_ptr(), _lib.stream_ptr())
        for m in range(K):
            r = slice(m * Mcap, (m + 1) * Mcap)
            p = hand._arrays()
            call("rth_ppo_grads_adv", p["actor"], p["value"], mb["s"][r].data_ptr(), D, mb["a"][r].data_ptr(),
                 mb["ret"][r].data_ptr(), mb["adv"][r].data_ptr(), mb["logp"][r].data_ptr(), Mcap, D, H, A,
                 float(hand.eps_clip), VF_COEF, ENT_COEF, p["actor_grads"], p["value_grads"], mb["loss"][r].data_ptr(),
                 mb["mean"].data_ptr(), gws.data_ptr(), mb["n"][m:].data_ptr(), _lib.stream_ptr())
            hand.actor_optimizer.step()
            hand.value_optimizer.step()
    torch.cuda.synchronize()
    _same_params(solver, hand)
    perm, sizes = minibatch_perm(solver.seed, 3, n, K)
    assert np.array_equal(solver.last_perm[:n].cpu().numpy(), perm) and _bits(mb["perm"][:n]) == _bits(solver.last_perm[:n])
    assert int(solver._shuffle_counter) == int(counter) == 4
    for m in range(K):  # |loss| in minibatch layout: the rows of each slice that count
        r = slice(m * Mcap, m * Mcap + int(sizes[m]))
        assert torch.isfinite(out[r]).all() and _bits(out[r]) == _bits(mb["loss"][r])
    assert _bits(solver.last_loss) == _bits(mb["mean"]) and int(sizes.sum()) == n
    # the 4-column batch goes through rth_ppo_grads_n, at the same count of calls
    solver.update_device(batch[:4], n_rows=n_rows)
    assert solver.hip_launches == 2 * 4 * 13 and solver.shuffle_calls == 8


def test_one_minibatch_is_the_solver_as_it_was(dev):
    """K = 1: no shuffle call, three ABI calls an epoch, the bits of a solver built without the keyword"""
    a, b = _solver(dev, impl="hip", n_minibatches=1), _solver(dev, impl="hip")
    batch = _batch5(45, 45, dev)
    x, y = a.update_device(batch), b.update_device(batch)
    _same_params(a, b)
    assert _bits(x) == _bits(y) and a.hip_launches == b.hip_launches == 12 and a.shuffle_calls == 0
    assert a.last_perm is None and int(a._shuffle_counter) == 0 and not a._per_shuffle


def test_solver_hip_against_the_torch_path(dev, golden):
    """the golden batch (64 rows, 4 columns), K = 4, one update from the same weights and seed, under
    test_ppo_gpu.test_solver_hip_against_the_golden_and_the_torch_path's bound (_close)"""
    g = golden("ppo_cartpole_b64.npz")
    dp, dl = float(g["drift_param"]), float(g["drift_loss"])
    hip = golden_solver(g, dev, impl="hip", n_minibatches=4)
    tor = golden_solver(g, dev, impl="torch", n_minibatches=4)
    tor.seed = hip.seed
    batch = [torch.as_tensor(x, device=dev) for x in golden_batch(g)]
    fails = []
    a, b = hip.update(batch), tor.update(batch)
    assert a.shape == b.shape == (64,) and hip.shuffle_calls == tor.shuffle_calls == 4
    assert np.array_equal(hip.last_perm.cpu().numpy(), tor.last_perm.cpu().numpy())
    _close("minibatch update |loss| hip vs torch", a, b, dl, fails)
    _close("minibatch last loss hip vs torch", hip.last_loss, tor.last_loss, dl, fails)
    for name, key, _ in NETS:
        for (k, p), q in zip(getattr(hip, key).state_dict().items(), getattr(tor, key).state_dict().values()):
            _close(f"minibatch final {name} {k} hip vs torch", p, q, dp, fails)
    assert not fails, fails


# ---------------------------------------------------------------------------- the loop
def _loop(**kw):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    kw = dict(dict(n_actors=9, horizon=5, max_episode_steps=8, seed=5, gae_lambda=0.95, n_minibatches=4), **kw)
    return PpoLoop(PpoLoopConfig(**kw), device="cuda", impl="hip")


def _abi_calls(loop):
    act = loop.actors
    return act.launches + act.finishes + act.normalizes + loop.solver.hip_launches


@pytest.mark.parametrize("normalize", [False, True])
def test_the_minibatch_loop_is_the_composition_of_its_parts(dev, normalize):
    """3 eager iterations at 9 envs x 5 steps, K = 4: a second actor set stepped and finished by hand
    and a second solver (the loop's seed) updated on its 5-column batch end with the loop's
    parameters, bit for bit (test_ppo_gae_gpu.test_the_gae_loop_is_the_composition_of_its_parts)"""
    loop = _loop(normalize_adv=normalize)
    cfg = loop.cfg
    assert loop.actors.cap == 5 and loop.gae and loop.solver.n_minibatches == 4
    other = PPOSolver(Box(-1, 1, (4,)), Discrete(2), k_epochs=cfg.k_epochs, eps_clip=cfg.eps_clip,
                      learning_rate=cfg.learning_rate, device=dev, impl="hip", n_minibatches=4)
    other.sync_weights(loop.solver)
    other.seed = loop.solver.seed
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
        assert _bits(loop.solver.last_perm) == _bits(other.last_perm) and _bits(loop.last_loss_abs) == _bits(
            other._per_shuffle[45]["loss_abs"])
        want = minibatch_perm(loop.solver.seed, 4 * (k + 1) - 1, 45, 4)[0]
        assert np.array_equal(loop.solver.last_perm.cpu().numpy(), want)
    assert (loop.iterations, loop.env_steps, loop.updates) == (3, 3 * 9 * 5, 3)
    assert loop.solver.shuffle_calls == int(loop.solver._shuffle_counter) == 12
    assert _abi_calls(loop) == 3 * (5 + 1 + int(normalize) + cfg.k_epochs * 13)
    assert int(loop.actors.dropped.sum()) == 0 and (loop.actors.t_dev == 15).all()


@pytest.mark.parametrize("normalize", [False, True])
def test_captured_minibatch_iterations_equal_eager_ones_and_reshuffle(dev, normalize):
    eager, graph = _loop(normalize_adv=normalize), _loop(normalize_adv=normalize)
    eager.run(4)
    graph.iteration()
    graph.capture()
    assert graph.solver.shuffle_calls == 4 and int(graph.solver._shuffle_counter) == 4  # recording ran nothing
    perms = []
    for _ in range(3):
        graph.iteration()
        perms.append(graph.solver.last_perm.clone())
    torch.cuda.synchronize()
    _same_params(eager.solver, graph.solver)
    for k in ("t_dev", "stats", "fill", "state", "gen", "seg_logp", "seg_s", "seg_r", "seg_done", "_complete", "n_dev",
              "batch_adv", "batch_v", "dropped"):
        assert _bits(getattr(eager.actors, k)) == _bits(getattr(graph.actors, k)), k
    for x, y in zip(eager.actors.batch, graph.actors.batch):
        assert _bits(x) == _bits(y)
    assert _bits(eager.solver.last_perm) == _bits(graph.solver.last_perm)
    assert _bits(eager.solver._shuffle_counter) == _bits(graph.solver._shuffle_counter)
    assert _bits(eager.last_loss_abs) == _bits(graph.last_loss_abs)
    # the replays reshuffle: the counter has advanced k_epochs per iteration, on the device and in its mirror
    assert int(graph.solver._shuffle_counter) == graph.solver.shuffle_calls == eager.solver.shuffle_calls == 4 * 4
    for k, p in enumerate(perms):
        want = minibatch_perm(graph.solver.seed, 4 * (k + 2) - 1, 45, 4)[0]
        assert np.array_equal(p.cpu().numpy(), want), k
    assert not torch.equal(perms[0], perms[1]) and not torch.equal(perms[1], perms[2])
    for k in ("iterations", "env_steps", "updates"):
        assert getattr(eager, k) == getattr(graph, k), k
    assert _abi_calls(eager) == _abi_calls(graph) == 4 * (5 + 1 + int(normalize) + eager.cfg.k_epochs * 13)
    assert int(graph.actors.dropped.sum()) == 0 and int(graph.actors.n_dev) == 45


def test_loop_refusals(dev):
    for K in (0, 65, -3):
        with pytest.raises(ValueError, match="n_minibatches"):
            _loop(n_minibatches=K)
    with pytest.raises(ValueError, match="n_minibatches 46: a batch can hold as few as 45 rows"):
        _loop(n_minibatches=46)
    with pytest.raises(ValueError, match="n_minibatches 10: a batch can hold as few as 9 rows"):
        _loop(gae_lambda=None, horizon=8, n_minibatches=10)
    with pytest.raises(ValueError, match="n_minibatches 2: the batch capacity n_actors . cap = 65568"):
        _loop(n_actors=2049, horizon=32, n_minibatches=2)
    assert _loop(n_actors=2049, horizon=32, n_minibatches=1).solver.n_minibatches == 1  # K = 1: no such limit
    assert _loop(n_minibatches=45).solver.n_minibatches == 45
    assert _loop(gae_lambda=None, horizon=8, n_minibatches=9).actors.cap == 15


def test_it_learns_cartpole_in_minibatches(dev):
    """CartPole-v0, 64 envs x 32 steps, lambda 0.95, normalised advantages, n_minibatches = 4, 50
    iterations, seeds 0 / 1 / 2, under test_ppo_gae_gpu.test_it_learns_cartpole_on_short_rollouts'
    criterion: the median of the envs' mean last finished episode length reaches the midpoint between
    the untrained actor's measured figure and the limit of 200, and max(untrained) < 60.
    Four times the optimiser steps: measured on an MI355X at the project's learning rate 0.01, trained
    200.0 / 191.6 / 200.0, and at 0.003, 198.7 / 184.7 / 197.1, untrained 22.0 / 26.3 / 22.5 in both
    (profiles/r24/ppo_minibatch.txt): 0.01 is stable and is what the test uses -- the median 200.0
    against a midpoint of 111.2 (full-batch epochs in the same session: 181.4 / 187.7 / 180.6)."""
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    trained, untrained = [], []
    for seed in (0, 1, 2):
        cfg = PpoLoopConfig(n_actors=64, horizon=32, gae_lambda=0.95, normalize_adv=True, seed=seed, n_minibatches=4,
                            learning_rate=LEARNING_RATE)
        loop = PpoLoop(cfg, device="cuda", impl="hip")
        untrained.append(loop.rollout_length())
        loop.run(50)
        trained.append(loop.mean_last_length())
        assert int(loop.actors.dropped.sum()) == 0 and loop.solver.shuffle_calls == 200
    print(f"ppo_loop minibatch CartPole-v0 64 x 32, K = 4, learning rate {LEARNING_RATE}, 50 iterations, seeds 0/1/2: "
          f"mean last finished length {trained}, untrained {untrained}")
    mid = (float(np.median(untrained)) + 200.0) / 2
    assert max(untrained) < 60
    assert float(np.median(trained)) >= mid, (trained, untrained, mid)


# ---------------------------------------------------------------------------- the example
@pytest.mark.parametrize("graph", [False, True])
def test_example_runs_end_to_end(dev, graph, monkeypatch, capsys):
    path = os.path.join(ROOT, "examples", "cartpole_ppo_minibatch_hip.py")
    monkeypatch.setattr(sys, "argv", [path, "--updates", "3", "--seed", "1"] + (["--graph"] if graph else []))
    monkeypatch.setattr(sys, "path", list(sys.path))
    runpy.run_path(path, run_name="__main__")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("cartpole_ppo_minibatch ")][-1]
    fields = dict(f.split("=") for f in line.split()[1:])
    assert fields["updates"] == "3" and fields["seed"] == "1" and fields["graph"] == str(int(graph))
    assert fields["env"] == "CartPole-v0" and fields["gae_lambda"] == "0.95" and fields["n_minibatches"] == "4"
    assert int(fields["env_steps"]) == 3 * 64 * 32 and int(fields["episodes"]) >= 64 and fields["dropped"] == "0"
    assert fields["shuffles"] == "12"
    for k in ("mean_last_len", "untrained_mean_last_len"):
        assert 1 <= float(fields[k]) <= 200
    assert int(fields["hip_launches"]) == 3 * (32 + 1 + 1 + 4 * 13)
