"""rth_ppo_grads_n against rth_ppo_grads, and reth_amd.ppo_loop.PpoLoop: the loop as the composition
of its parts, as a replayed graph, its refusals, that it learns CartPole-v0, and the example."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from reth_amd import _lib
from reth_amd._lib import call
from reth_amd.ppo import ENT_COEF, VF_COEF, PPOSolver, _params6
from reth_amd.solver import Box, Discrete
from test_ppo_gpu import EPS32, H, _arr, _params, case

pytestmark = pytest.mark.gpu

CAP = 320
NAN = float("nan")


def _grads(P, cols, B, D, A, n_dev=None, backward=True):
    """rth_ppo_grads (n_dev None) or rth_ppo_grads_n with capacity B on the device columns
    (s, a, ret, old) -> (the twelve gradients, loss_abs [B], loss_mean [1], workspace)"""
    dev = cols[0].device
    s, a, ret, old = cols
    grads = [torch.full_like(p, NAN) for net in P for p in net]
    loss_abs, loss_mean = torch.full((B,), NAN, device=dev), torch.full((1,), NAN, device=dev)
    ws = torch.full((_lib.lib().rth_ppo_workspace(B, D, H, A) // 4,), NAN, device=dev)
    fn, count = ("rth_ppo_grads", ()) if n_dev is None else ("rth_ppo_grads_n", (n_dev.data_ptr(),))
    call(fn, _arr(P[0]), _arr(P[1]), s.data_ptr(), s.stride(0), a.data_ptr(), ret.data_ptr(), old.data_ptr(), B, D, H, A,
         EPS32, VF_COEF, ENT_COEF, _arr(grads[:6]) if backward else None, _arr(grads[6:]) if backward else None,
         loss_abs.data_ptr(), loss_mean.data_ptr(), ws.data_ptr(), *count, _lib.stream_ptr())
    torch.cuda.synchronize()
    return grads, loss_abs, loss_mean, ws


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("D,A", [(4, 2), (6, 3)])
def test_grads_n_equals_grads_on_the_first_n_rows(dev, D, A):
    """capacity 320; the rows at n and beyond hold NaN (an action out of range), so a read of one
    shows in every sum"""
    c = case(CAP, D, A)
    P = _params(c, dev)
    full = [c["s"].to(dev), c["a"].to(dev), c["ret"].to(dev), c["old"].to(dev)]
    for n in (1, 7, 8, 9, 128, 129, 300, 320, 10_000):
        m = min(n, CAP)
        want = _grads(P, [t[:m].contiguous() for t in full], m, D, A)
        cols = [t.clone() for t in full]
        for t in cols:
            t[m:] = 99 if t.dtype == torch.int64 else NAN
        n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
        got = _grads(P, cols, CAP, D, A, n_dev)
        for k, (g, w) in enumerate(zip(got[0], want[0])):
            assert torch.isfinite(g).all() and _bits(g) == _bits(w), (n, k)
        assert torch.isfinite(got[1][:m]).all() and _bits(got[1][:m]) == _bits(want[1]), n
        assert torch.isfinite(got[2]).all() and _bits(got[2]) == _bits(want[2]), n
        assert torch.isfinite(got[3][:m]).all() and _bits(got[3][:m]) == _bits(want[3][:m]), n  # the new log-probabilities
        assert torch.isnan(got[1][m:]).all()  # |loss| beyond the count is not written
        # evaluate only
        ev = _grads(P, cols, CAP, D, A, n_dev, backward=False)
        assert _bits(ev[1][:m]) == _bits(want[1]) and _bits(ev[2]) == _bits(want[2]), n
        assert _bits(ev[3][:m]) == _bits(want[3][:m]) and all(torch.isnan(g).all() for g in ev[0]), n
    # an empty batch: zero gradients and a zero loss mean, nothing else
    cols = [torch.full_like(t, 99 if t.dtype == torch.int64 else NAN) for t in full]
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    for n_dev in (zero, zero - 5):
        got = _grads(P, cols, CAP, D, A, n_dev)
        assert all((g == 0).all() for g in got[0]) and float(got[2]) == 0.0
        assert torch.isnan(got[1]).all()
    ev = _grads(P, cols, CAP, D, A, zero, backward=False)
    assert float(ev[2]) == 0.0
    # the count is required, and the capacity is checked as rth_ppo_grads checks B
    lib, s = _lib.lib(), _lib.stream_ptr()
    a = [_arr(P[0]), _arr(P[1]), full[0].data_ptr(), D, full[1].data_ptr(), full[2].data_ptr(), full[3].data_ptr()]
    b = [D, H, A, EPS32, VF_COEF, ENT_COEF, None, None, got[1].data_ptr(), None, got[3].data_ptr()]
    assert lib.rth_ppo_grads_n(*a, CAP, *b, None, s) == -1 and b"rth_ppo_grads_n" in lib.rth_last_error()
    assert lib.rth_ppo_grads_n(*a, 0, *b, zero.data_ptr(), s) == -1 and b"rth_ppo_grads_n" in lib.rth_last_error()


def test_update_device_with_a_device_row_count(dev):
    """PPOSolver.update_device(batch, n_rows=n) equals update_device on the first n rows, on both paths"""
    c = case(CAP, 4, 2)
    cols = [c["s"].to(dev), c["a"].to(dev), c["ret"].to(dev), c["old"].to(dev)]
    n = 129
    n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
    for impl in ("hip", "torch"):
        torch.manual_seed(3)
        a = PPOSolver(Box(-1, 1, (4,)), Discrete(2), device=dev, impl=impl)
        b = PPOSolver(Box(-1, 1, (4,)), Discrete(2), device=dev, impl=impl)
        b.sync_weights(a)
        for _ in range(2):
            la = a.update_device([t[:n].contiguous() for t in cols])
            lb = b.update_device(cols, n_rows=n_dev)
            assert _bits(la) == _bits(lb[:n]), impl
        for net in ("actor_network", "value_network"):
            for p, q in zip(_params6(getattr(a, net)), _params6(getattr(b, net))):
                assert _bits(p) == _bits(q), (impl, net)
        if impl == "hip":
            assert a.hip_launches == b.hip_launches == 2 * 3 * a.k_epochs
            with pytest.raises(ValueError, match="n_rows"):
                b.update_device(cols, n_rows=n)


# ---------------------------------------------------------------------------- the loop
def _loop(**kw):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    kw = dict(dict(n_actors=9, horizon=8, max_episode_steps=8, seed=5), **kw)
    return PpoLoop(PpoLoopConfig(**kw), device="cuda", impl="hip")


def _same_params(a, b):
    for net in ("actor_network", "value_network"):
        for p, q in zip(_params6(getattr(a, net)), _params6(getattr(b, net))):
            assert _bits(p) == _bits(q), net


def test_the_loop_is_the_composition_of_its_parts(dev):
    """3 eager iterations; a second solver updated with update_device on the n rows each finish
    produced, as dense tensors, ends with the loop's parameters bit for bit"""
    loop = _loop()
    other = PPOSolver(Box(-1, 1, (4,)), Discrete(2), k_epochs=loop.cfg.k_epochs, eps_clip=loop.cfg.eps_clip,
                      learning_rate=loop.cfg.learning_rate, device=dev, impl="hip")
    other.sync_weights(loop.solver)
    batches = []
    finish = loop.actors.finish

    def recording(gamma):
        batch, n_dev = finish(gamma)
        n = int(n_dev)
        batches.append([b[:n].cpu() for b in batch])
        return batch, n_dev

    loop.actors.finish = recording
    for k in range(3):
        loop.iteration()
        rows = batches[-1]
        assert 9 <= len(rows[1]) <= 9 * loop.actors.cap
        other.update_device([r.to(dev) for r in rows])
        _same_params(loop.solver, other)
    assert (loop.iterations, loop.env_steps, loop.updates) == (3, 3 * 9 * 8, 3)
    calls = loop.actors.launches + loop.actors.finishes + loop.solver.hip_launches
    assert calls == 3 * (8 + 1 + 3 * loop.cfg.k_epochs) and int(loop.actors.dropped.sum()) == 0
    assert (loop.actors.t_dev == 24).all() and len(batches) == 3


def test_captured_iterations_equal_eager_ones(dev):
    eager, graph = _loop(), _loop()
    assert not graph.graph_ready()
    with pytest.raises(RuntimeError, match="graph_ready"):
        graph.capture()
    eager.run(4)
    graph.iteration()
    assert graph.graph_ready()
    graph.capture()
    graph.capture()  # (a second call is a no-op)
    graph.run(3)
    torch.cuda.synchronize()
    _same_params(eager.solver, graph.solver)
    for k in ("t_dev", "stats", "fill", "state", "gen", "seg_logp"):
        assert _bits(getattr(eager.actors, k)) == _bits(getattr(graph.actors, k)), k
    assert _bits(eager.actors.n_dev) == _bits(graph.actors.n_dev)
    for k in ("iterations", "env_steps", "updates"):
        assert getattr(eager, k) == getattr(graph, k), k
    for k in ("pushes", "launches", "finishes"):
        assert getattr(eager.actors, k) == getattr(graph.actors, k), k
    assert eager.solver.hip_launches == graph.solver.hip_launches == 4 * 3 * eager.cfg.k_epochs


def test_refusals(dev):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    with pytest.raises(ValueError, match="horizon 7 < max_episode_steps 8"):
        _loop(horizon=7)
    with pytest.raises(ValueError, match="horizon 100 < max_episode_steps 200"):
        _loop(horizon=100, max_episode_steps=None)
    with pytest.raises(ValueError, match="the device envs are"):
        _loop(env="Pendulum-v0")
    with pytest.raises(RuntimeError, match="no torch fallback"):
        PpoLoop(PpoLoopConfig(), device="cuda", impl="torch")


def test_it_learns_cartpole(dev):
    """CartPole-v0 at the default config, 50 iterations, seeds 0 / 1 / 2: the median of the envs'
    mean last finished episode length reaches the midpoint between the untrained actor's figure
    (one rollout before any update, measured here) and the limit of 200.  Measured on an MI355X:
    trained 194.1 / 147.8 / 193.1, untrained 27.1 / 30.1 / 20.3 (profiles/r20/ppo_actors.txt): the
    median 193.1 against a midpoint of 113.6."""
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    trained, untrained = [], []
    for seed in (0, 1, 2):
        loop = PpoLoop(PpoLoopConfig(seed=seed), device="cuda", impl="hip")
        untrained.append(loop.rollout_length())
        loop.run(50)
        trained.append(loop.mean_last_length())
        assert int(loop.actors.dropped.sum()) == 0
    print(f"ppo_loop CartPole-v0 50 iterations, seeds 0/1/2: mean last finished length {trained}, untrained {untrained}")
    mid = (float(np.median(untrained)) + 200.0) / 2
    assert max(untrained) < 60
    assert float(np.median(trained)) >= mid, (trained, untrained, mid)


# ---------------------------------------------------------------------------- the example
@pytest.mark.parametrize("graph", [False, True])
def test_example_runs_end_to_end(dev, graph, monkeypatch, capsys):
    path = os.path.join(ROOT, "examples", "cartpole_ppo_loop_hip.py")
    monkeypatch.setattr(sys, "argv", [path, "--updates", "2", "--seed", "1"] + (["--graph"] if graph else []))
    monkeypatch.setattr(sys, "path", list(sys.path))
    runpy.run_path(path, run_name="__main__")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("cartpole_ppo_loop ")][-1]
    fields = dict(f.split("=") for f in line.split()[1:])
    assert fields["updates"] == "2" and fields["seed"] == "1" and fields["graph"] == str(int(graph))
    assert int(fields["env_steps"]) == 4000 and int(fields["episodes"]) >= 20 and fields["dropped"] == "0"
    for k in ("mean_last_len", "untrained_mean_last_len"):
        assert 1 <= float(fields[k]) <= 200
    assert int(fields["hip_launches"]) == 2 * (200 + 1 + 3 * 4)
