"""Shuffled minibatch epochs for PPO, the parts that need no GPU: the numpy Philox4x32-10 of
reth_amd.ppo against the oracle's, shuffle_keys / minibatch_perm (the host restatement of
csrc/ppo_shuffle.hpp's permutation) at their edges, the orders' uniformity, and PPOSolver's torch path
with n_minibatches against a hand-written loop over minibatch_perm's slices."""
import itertools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from reth_amd.ppo import (STREAM_PPO_SHUFFLE, PPOSolver, _params6, minibatch_perm, philox4x32, shuffle_keys)
from reth_amd.solver import Box, Discrete


def test_numpy_philox_is_the_oracles():
    """a few hundred (lane, counter, seed) triples, counter and seed at or above 2^32 and lane 65,535
    among them: the four output words, and shuffle_keys' 64-bit key built from the first two"""
    rng = np.random.default_rng(0)
    lanes = [0, 1, 255, 65535] + [int(v) for v in rng.integers(0, 65536, 12)]
    counters = [0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 12345] + [int(v) for v in rng.integers(0, 2 ** 62, 2)]
    seeds = [0, 11, 2 ** 32, 2 ** 32 + 7, 2 ** 62 - 1, 2 ** 64 - 1]
    triples = list(itertools.product(lanes, counters, seeds))
    assert len(triples) >= 300
    for counter, seed in itertools.product(counters, seeds):
        got = philox4x32(np.array(lanes), counter & 0xFFFFFFFF, counter >> 32, STREAM_PPO_SHUFFLE, seed & 0xFFFFFFFF,
                         seed >> 32)
        keys = shuffle_keys(seed, counter, 65536)
        assert keys.dtype == np.uint64 and keys.shape == (65536,)
        for k, lane in enumerate(lanes):
            want = orc.philox4x32([lane, counter & 0xFFFFFFFF, counter >> 32, STREAM_PPO_SHUFFLE],
                                  [seed & 0xFFFFFFFF, seed >> 32])
            assert [int(w[k]) for w in got] == [int(v) for v in want], (lane, counter, seed)
            assert int(keys[lane]) == int(want[0]) | (int(want[1]) << 32), (lane, counter, seed)
    assert STREAM_PPO_SHUFFLE == 14


@pytest.mark.parametrize("K", [1, 2, 4, 7])
@pytest.mark.parametrize("n", [0, 1, 3, 45, 257])
def test_minibatch_perm_is_a_permutation_with_clamped_sizes(n, K):
    perm, sizes = minibatch_perm(12345, 3, n, K)
    assert perm.shape == (n,) and sizes.shape == (K,)
    assert sorted(perm.tolist()) == list(range(n))
    M = (n + K - 1) // K
    assert sizes.tolist() == [min(max(n - m * M, 0), M) for m in range(K)] and int(sizes.sum()) == n
    keys = shuffle_keys(12345, 3, n)
    assert np.array_equal(perm, np.argsort(keys, kind="stable"))
    if n == 257:  # another pass, another order; the same pass, the same order
        assert not np.array_equal(perm, minibatch_perm(12345, 4, n, K)[0])
        assert not np.array_equal(perm, minibatch_perm(12346, 3, n, K)[0])
        assert np.array_equal(perm, minibatch_perm(12345, 3, n, K)[0])


def test_equal_keys_keep_their_order():
    n = 257
    perm, sizes = minibatch_perm(0, 0, n, 4, keys=np.full(n, 7, np.uint64))
    assert np.array_equal(perm, np.arange(n)) and sizes.tolist() == [65, 65, 65, 62]
    # pairs (k, k, k + 1, k + 1, ...) in descending blocks: each pair in its order, the blocks reversed
    keys = np.repeat(np.arange(100, 0, -1, dtype=np.uint64), 2)
    perm, _ = minibatch_perm(0, 0, 200, 4, keys=keys)
    assert np.array_equal(perm.reshape(100, 2), np.arange(200).reshape(100, 2)[::-1])
    # keys above 2^63 sort as unsigned, and keys beyond n are ignored
    keys = np.array([2 ** 64 - 1, 1, 2 ** 63, 0, 5], dtype=np.uint64)
    assert minibatch_perm(0, 0, 4, 2, keys=keys)[0].tolist() == [3, 1, 2, 0]


def test_every_order_of_three_rows_is_as_likely():
    """n = 3, counters 0..5,999: each of the 6 orders within 5 sigma of 1,000 (test_philox_draws' rule)"""
    counts = {}
    for c in range(6000):
        order = tuple(minibatch_perm(2024, c, 3, 1)[0].tolist())
        counts[order] = counts.get(order, 0) + 1
    assert sorted(counts) == sorted(itertools.permutations(range(3)))
    sigma = np.sqrt(6000 * (1 / 6) * (5 / 6))
    print("orders of 3 rows over 6,000 counters:", counts)
    assert all(abs(v - 1000) <= 5 * sigma for v in counts.values()), counts


def _batch(n, D=4, A=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(n, D, generator=g)
    a = torch.randint(0, A, (n,), generator=g)
    ret, adv = torch.randn(n, generator=g), torch.randn(n, generator=g)
    old = -torch.rand(n, generator=g) - 0.3
    return [s, a, ret, old, adv]


def _solver(**kw):
    torch.manual_seed(3)
    return PPOSolver(Box(-1, 1, (4,)), Discrete(2), device="cpu", impl="torch", **kw)


def _same(a, b):
    for net in ("actor_network", "value_network"):
        for p, q in zip(_params6(getattr(a, net)), _params6(getattr(b, net))):
            assert p.detach().numpy().tobytes() == q.detach().numpy().tobytes(), net


def test_torch_path_is_a_loop_over_minibatch_perms_slices():
    """45 rows, 5 columns, K = 4 (12 / 12 / 12 / 9 rows): update() ends with the parameters of the same
    steps taken by hand, one single-epoch full-batch update per slice, bit for bit"""
    batch = _batch(45)
    solver, hand = _solver(n_minibatches=4), _solver(k_epochs=1)
    _same(solver, hand)
    assert solver.n_minibatches == 4 and solver.shuffle_calls == 0 and hand.n_minibatches == 1
    out = solver.update(batch)
    assert solver.shuffle_calls == solver.k_epochs == 4 and out.shape == (48,)
    for c in range(4):
        perm, sizes = minibatch_perm(solver.seed, c, 45, 4)
        assert sizes.tolist() == [12, 12, 12, 9]
        for m in range(4):
            rows = torch.as_tensor(perm[m * 12:m * 12 + int(sizes[m])])
            loss = hand.update([b[rows] for b in batch])
            if c == 3:
                assert torch.equal(out[m * 12:m * 12 + len(rows)], loss)
    _same(solver, hand)
    assert torch.equal(solver.last_perm, torch.as_tensor(perm)) and torch.isnan(out[45:]).all()
    assert float(solver.last_loss) == float(hand.last_loss)
    # the 4-column batch takes the same route
    solver.update(batch[:4])
    assert solver.shuffle_calls == 8
    # a minibatch without rows is refused
    with pytest.raises(ValueError, match="empty"):
        solver.update([b[:3] for b in batch])
    with pytest.raises(ValueError, match="n_minibatches"):
        _solver(n_minibatches=0)
    with pytest.raises(ValueError, match="n_minibatches"):
        _solver(n_minibatches=65)


def test_one_minibatch_is_the_solver_without_the_keyword():
    batch = _batch(45, seed=1)
    with_kw, without = _solver(n_minibatches=1), _solver()
    a, b = with_kw.update(batch), without.update(batch)
    _same(with_kw, without)
    assert torch.equal(a, b) and a.shape == (45,) and with_kw.shuffle_calls == 0 and with_kw.last_perm is None
    # and neither draws from the global generator for a seed it does not need
    torch.manual_seed(9)
    _solver_state = torch.get_rng_state()
    torch.manual_seed(3)
    PPOSolver(Box(-1, 1, (4,)), Discrete(2), device="cpu", impl="torch")
    s0 = torch.get_rng_state()
    torch.manual_seed(3)
    PPOSolver(Box(-1, 1, (4,)), Discrete(2), device="cpu", impl="torch", n_minibatches=1)
    assert torch.equal(s0, torch.get_rng_state()) and not torch.equal(s0, _solver_state)


def test_loop_config_default_and_refusals():
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    assert PpoLoopConfig().n_minibatches == 1
    for K in (0, -1, 65):
        with pytest.raises(ValueError, match="n_minibatches"):
            PpoLoop(PpoLoopConfig(gae_lambda=0.95, horizon=32, n_minibatches=K))
    with pytest.raises(ValueError, match="n_minibatches 11: a batch can hold as few as 10 rows"):
        PpoLoop(PpoLoopConfig(n_minibatches=11))  # whole episodes: n_actors rows at the least
    with pytest.raises(ValueError, match="n_minibatches 7: a batch can hold as few as 6 rows"):
        PpoLoop(PpoLoopConfig(n_actors=2, horizon=3, gae_lambda=0.95, n_minibatches=7))
